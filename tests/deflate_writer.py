"""A bit-level RFC 1951 writer for the tests of the two DEFLATE decoders (csrc/inflate_dev.hip on the device, csrc/inflate_fast.h on
the host): pure Python, nothing compiled.  zlib's compressor writes a narrow corner of the format; this writes the rest -- any code
lengths up to 15 bits, distance codes of one or no symbol, chosen 16/17/18 runs and hclen, stored blocks with chosen padding,
lengths under a chosen symbol -- and places a header, a LEN/NLEN pair or the longest symbol at a chosen byte of the stream.

    d = Deflate(); d.stored(b"abc"); d.fixed([65, (258, 1)]); d.dynamic(ll_lens, d_lens, tokens, final=True); stream, want = d.finish()

A token is a literal (an int) or a match (length, distance[, length symbol]); ("ll", sym), ("d", sym) and ("raw", value, bits) write
a bare code or bare bits -- what the streams that must be refused are made of.  replay() turns tokens into the bytes they stand for.
random_stream(seed) draws whole streams; corpus() is the list of named cases.  tests/test_deflate_writer_cpu.py holds every stream
this module makes to zlib's inflate, so the GPU and host checks can take the expected bytes as given."""
import zlib

import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32


def length_symbol(length):
    """the usual symbol of a match length (258 -> 285)"""
    for s in range(28, -1, -1):
        if LEN_BASE[s] <= length:
            return 257 + s
    raise ValueError(length)


def dist_symbol(dist):
    for s in range(29, -1, -1):
        if DIST_BASE[s] <= dist:
            return s
    raise ValueError(dist)


def canon(lens):
    """canonical codes (RFC 1951 3.2.2) of a vector of code lengths -> {symbol: (code, length)}; an incomplete or over-subscribed
    vector is coded by the same rule (codes cut to their length)"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l] & ((1 << l) - 1), l)
            nxt[l] += 1
    return out


class BitWriter:
    def __init__(self):
        self.buf, self.acc, self.n = bytearray(), 0, 0

    def bits(self, v, k):  # k bits of v, the lowest first
        self.acc |= (v & ((1 << k) - 1)) << self.n
        self.n += k
        while self.n >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):  # a Huffman code: its highest bit first
        self.bits(int(format(code, "0%db" % length)[::-1], 2), length)

    def align(self, pad=0):  # to the byte boundary, with the low bits of `pad`
        if self.n:
            self.bits(pad, 8 - self.n)

    def raw(self, data):  # whole bytes at a byte boundary
        assert self.n == 0
        self.buf += data

    def bit_pos(self):
        return len(self.buf) * 8 + self.n


def replay(tokens, out=None):
    """the bytes a token list stands for, appended to `out` (the stream's earlier output: matches reach into it)"""
    out = bytearray() if out is None else out
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            length, dist = t[0], t[1]
            assert 1 <= dist <= len(out), (dist, len(out))
            piece = bytes(out[-dist:])
            out += (piece * (length // dist + 1))[:length]
    return out


def encode_lengths(seq, rng=None):
    """code-length symbols [(symbol, extra value)] of a sequence of code lengths: greedy runs, or with `rng` runs cut at random"""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, r = seq[i], 1
        while i + r < n and seq[i + r] == v:
            r += 1
        if v == 0 and r >= 3 and not (rng is not None and rng.random() < 0.15):
            if rng is not None and i > 0 and seq[i - 1] == 0 and rng.random() < 0.3:
                t = int(rng.integers(3, min(r, 6) + 1))  # (a 16 behind a zero repeats the zero)
                out.append((16, t - 3))
            else:
                t = min(r, 138) if rng is None else int(rng.integers(3, min(r, 138) + 1))
                out.append((17, t - 3) if t <= 10 else (18, t - 11))
            i += t
        elif v != 0 and i > 0 and seq[i - 1] == v and r >= 3 and not (rng is not None and rng.random() < 0.15):
            t = min(r, 6) if rng is None else int(rng.integers(3, min(r, 6) + 1))
            out.append((16, t - 3))
            i += t
        else:
            out.append((v, 0))
            i += 1
    return out


def lens_from_syms(syms):
    """the code lengths a sequence of code-length symbols stands for"""
    out = []
    for s, x in syms:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + x)
        elif s == 17:
            out += [0] * (3 + x)
        else:
            out += [0] * (11 + x)
    return out


def flat_code(symbols, n):
    """a complete code of n symbols' lengths, as even as possible, on the given symbols (two at least)"""
    symbols = sorted(symbols)
    m = len(symbols)
    assert m >= 2
    k = m.bit_length() - 1
    short = (1 << (k + 1)) - m  # symbols of k bits; the others take k + 1
    lens = [0] * n
    for j, s in enumerate(symbols):
        lens[s] = k if j < short else k + 1
    return lens


def kraft_split(rng, m, max_bits, deep=0.5):
    """m lengths of a random complete code: a leaf is split in two until there are m; `deep`: how often the deepest leaf is taken"""
    assert 2 <= m <= 1 << max_bits
    leaves = [1, 1]
    while len(leaves) < m:
        open_ = [i for i, d in enumerate(leaves) if d < max_bits]
        if rng.random() < deep:
            top = max(leaves[i] for i in open_)
            open_ = [i for i in open_ if leaves[i] == top]
        i = open_[int(rng.integers(0, len(open_)))]
        leaves[i] += 1
        leaves.append(leaves[i])
    return leaves


def random_code(rng, used, n, max_bits=15, extra=0.3):
    """a random complete code over the alphabet [0, n) that covers `used` (and, two symbols at least, some others)"""
    syms = set(used)
    rest = [s for s in range(n) if s not in syms]
    rng.shuffle(rest)
    more = int(len(rest) * rng.random() * extra) if rng.random() < 0.7 else 0
    more = max(more, 2 - len(syms))
    syms |= set(rest[:more])
    syms = sorted(syms)
    lengths = kraft_split(rng, len(syms), max_bits, deep=float(rng.random()))
    rng.shuffle(lengths)
    lens = [0] * n
    for s, l in zip(syms, lengths):
        lens[s] = int(l)
    return lens


def auto_header(ll_lens, d_lens, rng=None):
    """a header for two code-length vectors: the smallest hlit, hdist and hclen and greedy runs, or with `rng` random ones"""
    hlit = max(257, max((i + 1 for i, l in enumerate(ll_lens) if l), default=0))
    hdist = max(1, max((i + 1 for i, l in enumerate(d_lens) if l), default=0))
    if rng is not None:
        hlit, hdist = int(rng.integers(hlit, 287)), int(rng.integers(hdist, 31))
    seq = (list(ll_lens) + [0] * 286)[:hlit] + (list(d_lens) + [0] * 30)[:hdist]
    syms = encode_lengths(seq, rng)
    used = {s for s, _ in syms}
    while len(used) < 2:
        used.add(min(set(range(19)) - used))
    if rng is None:
        cl_lens = flat_code(used, 19)
    else:
        cl_lens = random_code(rng, used, 19, max_bits=7)
    hclen = max(4, max(i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]))
    if rng is not None:
        hclen = int(rng.integers(hclen, 20))
    return dict(hlit=hlit, hdist=hdist, hclen=hclen, cl_lens=cl_lens, syms=syms)


class Deflate:
    """one raw DEFLATE stream under construction, with the bytes it stands for"""

    def __init__(self):
        self.w, self.out = BitWriter(), bytearray()

    def byte_pos(self):
        assert self.w.n == 0
        return len(self.w.buf)

    def stored(self, data, final=False, pad=0, nlen=None):
        w = self.w
        w.bits(1 if final else 0, 1)
        w.bits(0, 2)
        w.align(pad)
        w.bits(len(data), 16)
        w.bits(len(data) ^ 0xFFFF if nlen is None else nlen, 16)
        w.raw(data)
        self.out += data
        return self

    def _tokens(self, tokens, ll, dd, eob):
        w = self.w
        for t in tokens:
            if isinstance(t, int):
                w.code(*ll[t])
            elif t[0] == "ll":
                w.code(*ll[t[1]])
            elif t[0] == "d":
                w.code(*dd[t[1]])
            elif t[0] == "raw":
                w.bits(t[1], t[2])
            else:
                length, dist = t[0], t[1]
                ls = t[2] if len(t) > 2 else length_symbol(length)
                assert 0 <= length - LEN_BASE[ls - 257] < (1 << LEN_EXTRA[ls - 257]) or (ls == 284 and length == 258), t
                w.code(*ll[ls])
                w.bits(length - LEN_BASE[ls - 257], LEN_EXTRA[ls - 257])
                if dist is not None:  # (None: the distance follows as "d" or "raw" tokens)
                    ds = dist_symbol(dist)
                    w.code(*dd[ds])
                    w.bits(dist - DIST_BASE[ds], DIST_EXTRA[ds])
        if eob:
            w.code(*ll[256])
        if all(isinstance(t, int) or (not isinstance(t[0], str) and t[1] is not None) for t in tokens):
            replay(tokens, self.out)

    def fixed(self, tokens, final=False, eob=True):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(1, 2)
        self._tokens(tokens, canon(FIXED_LL), canon(FIXED_D), eob)
        return self

    def dynamic(self, ll_lens, d_lens, tokens, final=False, header=None, eob=True, rng=None, btype=2):
        """header: dict(hlit, hdist, hclen, cl_lens: the 19 lengths by symbol, syms: [(code-length symbol, extra value)]) as
        auto_header() makes it; given, it is written as it stands, whatever ll_lens and d_lens (which code the tokens) say"""
        w = self.w
        h = header or auto_header(ll_lens, d_lens, rng)
        w.bits(1 if final else 0, 1)
        w.bits(btype, 2)
        w.bits(h["hlit"] - 257, 5)
        w.bits(h["hdist"] - 1, 5)
        w.bits(h["hclen"] - 4, 4)
        for s in CL_ORDER[:h["hclen"]]:
            w.bits(h["cl_lens"][s], 3)
        cl = canon(h["cl_lens"])
        for s, x in h["syms"]:
            w.code(*cl[s])
            if s >= 16:
                w.bits(x, (2, 3, 7)[s - 16])
        self._tokens(tokens, canon(ll_lens), canon(d_lens), eob)
        return self

    def finish(self):
        self.w.align(0)
        return bytes(self.w.buf), bytes(self.out)


def header_bits(ll_lens, d_lens, header=None):
    """how many bits Deflate.dynamic() writes in front of the block's first symbol"""
    return Deflate().dynamic(ll_lens, d_lens, [], header=header, eob=False).w.bit_pos()


# ---- random streams

def _random_tokens(rng, n_out, have, mode):
    """tokens of about n_out bytes behind `have` bytes of earlier output.  mode 0: literals only, 1: matches of one distance
    symbol, 2: anything"""
    toks, made = [], 0
    nlit = int(rng.integers(1, 257)) if rng.random() < 0.7 else int(rng.integers(1, 5))
    alphabet = rng.permutation(256)[:nlit]
    one = int(rng.integers(0, 30))
    p_match = 0.0 if mode == 0 else float(rng.random()) * 0.6 + 0.02
    while made < n_out:
        pos = have + made
        if pos and rng.random() < p_match:
            length = (258, 3, 4, 64, 65, 257)[int(rng.integers(0, 6))] if rng.random() < 0.3 else int(rng.integers(3, 259))
            if mode == 1:
                ds = one
                while DIST_BASE[ds] > pos:
                    ds -= 1
                one = ds
            else:
                ds = int(rng.integers(0, 30))
                while DIST_BASE[ds] > pos:
                    ds = int(rng.integers(0, ds))
            dist = min(pos, DIST_BASE[ds] + int(rng.integers(0, 1 << DIST_EXTRA[ds])))
            if dist_symbol(dist) != ds:  # (pos cut it short)
                dist = DIST_BASE[ds]
            ls = 284 if length == 258 and rng.random() < 0.3 else length_symbol(length)
            toks.append((length, dist, ls))
            made += length
        else:
            toks.append(int(alphabet[int(rng.integers(0, nlit))]))
            made += 1
    return toks, made


def random_stream(seed):
    """a random valid stream and its bytes: one to four blocks of mixed types, 0 to 40 000 bytes of output, random complete codes
    of up to 15 bits, distance codes of many, one (a single 1-bit code) or no symbols, random headers"""
    rng = np.random.default_rng([0xDEF1A7E, seed])
    d = Deflate()
    n_blocks = int(rng.integers(1, 5))
    total = int(rng.integers(0, 40001)) if rng.random() < 0.8 else int(rng.integers(0, 300))
    cuts = sorted(int(x) for x in rng.integers(0, total + 1, n_blocks - 1)) + [total]
    at = 0
    for b, end in enumerate(cuts):
        n, final = end - at, b == n_blocks - 1
        at = end
        kind = int(rng.integers(0, 5))
        if kind == 0:
            d.stored(rng.bytes(min(n, 65535)), final, pad=int(rng.integers(0, 256)))
            continue
        mode = int(rng.integers(0, 3))
        toks, _ = _random_tokens(rng, n, len(d.out), mode)
        if kind == 1:
            d.fixed(toks, final)
            continue
        ll_used = {256} | {t if isinstance(t, int) else t[2] for t in toks}
        d_used = {dist_symbol(t[1]) for t in toks if not isinstance(t, int)}
        ll_lens = random_code(rng, ll_used, 286)
        if not d_used and rng.random() < 0.6:
            d_lens = [0]  # no distance code at all
        elif len(d_used) <= 1 and rng.random() < 0.7:
            d_lens = [0] * 30
            d_lens[min(d_used) if d_used else int(rng.integers(0, 30))] = 1  # a single 1-bit code
        else:
            d_lens = random_code(rng, d_used, 30)
        d.dynamic(ll_lens, d_lens, toks, final, rng=rng)
    return d.finish()


# ---- the corpus

STAIR = list(range(1, 15)) + [15, 15]  # a complete code with every length 1 .. 15


def _stair(n, symbols):
    """the stair code on `symbols` (16 of them, in the order of their lengths 1, 2, .., 14, 15, 15)"""
    lens = [0] * n
    for s, l in zip(symbols, STAIR):
        lens[s] = l
    return lens


def _filler(rng, d, upto, final=False):
    """stored blocks of random bytes until the output is `upto` bytes long"""
    while True:
        n = min(upto - len(d.out), 65535)
        d.stored(rng.bytes(n), final and len(d.out) + n == upto, pad=int(rng.integers(0, 256)))
        if len(d.out) == upto:
            return d


def _bulk(d, n):
    """about n bytes of output for ~n / 20 bytes of stream: a fixed block of a zero and matches at distance 1"""
    d.fixed([0] + [(258, 1)] * (n // 258 + 1))
    return d


# literal/length: literal 'x' on the 1-bit code, 284 (5 extra bits) and the end of block on the two 15-bit codes;
# distance: symbols 28 and 29 (13 extra bits) on the two 15-bit codes
S48_LL = _stair(286, [120] + list(range(1, 14)) + [284, 256])
S48_D = _stair(30, list(range(0, 14)) + [28, 29])


def _sym48(d, rng, p):
    """p 1-bit literals and the 48-bit symbol (15 + 5 + 15 + 13) as a final dynamic block"""
    ds = 28 + int(rng.integers(0, 2))
    dist = min(len(d.out) + p, DIST_BASE[ds] + int(rng.integers(0, 1 << 13)))
    assert dist_symbol(dist) == ds
    length = 227 + int(rng.integers(0, 32))
    d.dynamic(S48_LL, S48_D, [120] * p + [(length, dist, 284), 120, 5], final=True)


def _place(rng, d, target_bit):
    """a stored block of random bytes such that the stream is target_bit // 8 bytes long behind it"""
    n = target_bit // 8 - (d.w.bit_pos() + 3 + 7) // 8 - 4
    assert 0 <= n <= 65535, n
    d.stored(rng.bytes(n), pad=int(rng.integers(0, 256)))


def _simple_codes():
    """a small complete pair of codes: literals 'a' .. 'f' and the end of block, lengths 3 .. 10, 258; distances 1 .. 4"""
    ll = [0] * 286
    for s in (97, 98, 99, 100, 101, 102, 256, 285) + tuple(range(257, 265)):
        ll[s] = 4
    return ll, [2, 2, 2, 2]


def _header(hlit, hdist, cl_lens, syms, hclen=None):
    hclen = hclen or max(4, max(i + 1 for i, s in enumerate(CL_ORDER) if cl_lens[s]))
    return dict(hlit=hlit, hdist=hdist, hclen=hclen, cl_lens=cl_lens, syms=syms)


def _cl(**lens):
    """the 19 code-length-code lengths from s<symbol>=<length>"""
    out = [0] * 19
    for k, v in lens.items():
        out[int(k[1:])] = v
    return out


def _corpus():
    rng = np.random.default_rng(0xC0DE5)
    cases = []

    def add(name, d, valid=True):
        stream, want = d.finish() if isinstance(d, Deflate) else d
        cases.append((name, stream, want if valid else None))

    # ---------------- codes
    # every literal/length code length 1 .. 15; a literal (10 and 13 bits), a length with extra bits (11 and 14 bits), 285 (12 bits)
    # and the end of block (15 bits) behind codes of 10 to 15 bits
    ll = _stair(286, [97, 98, 99, 100, 101, 102, 103, 104, 105, 0xC3, 270, 285, 0, 284, 256, 255])
    d = Deflate().dynamic(ll, [1, 1], [97, 98, 99, 100, 101, 102, 103, 104, 105, 0xC3, 0, 255, (23, 2), (258, 1), (240, 2), 0xC3, 0, (26, 1), 255], final=True)
    add("ll_every_length", d)
    # every distance code length 1 .. 15; 28 and 29 (13 extra bits) on 14 and 15 bits
    dsyms = [0, 1, 2, 3, 4, 5, 6, 7, 10, 16, 20, 24, 26, 28, 29, 27]
    dl = _stair(30, dsyms)
    d = _filler(rng, Deflate(), 32768)
    ll_s, _ = _simple_codes()
    toks = []
    for s in dsyms:
        for x in {0, (1 << DIST_EXTRA[s]) - 1, int(rng.integers(0, 1 << DIST_EXTRA[s]))}:
            toks += [(int(rng.integers(3, 11)), DIST_BASE[s] + x), 97 + s % 6]
    d.dynamic(ll_s, dl, toks, final=True)
    add("dist_every_length", d)
    # the 48-bit symbol behind p 1-bit literals: every bit phase of the refill
    for p in range(64):
        d = _filler(rng, Deflate(), 32768)
        _sym48(d, rng, p)
        add("sym48_p%d" % p, d)
    # a single 1-bit distance code, used by matches: symbol 0, and a symbol with extra bits behind zeros
    d = Deflate().dynamic(ll_s, [1], [97, (5, 1), 98, (258, 1), 99, (3, 1)], final=True)
    add("single_dist_1bit_sym0", d)
    d = _filler(rng, Deflate(), 300).dynamic(ll_s, [0] * 15 + [1], [97, (5, 193), 98, (258, 256), (10, 200)], final=True)
    add("single_dist_1bit_sym15", d)
    add("hdist1_len0_literals_only", Deflate().dynamic(ll_s, [0], [97, 98, 99, 102, 102], final=True))
    # hlit and hdist at their ends
    ll257 = flat_code(list(range(60, 70)) + [256], 257)
    ll286 = flat_code(list(range(60, 70)) + [256, 270, 285], 286)
    d30 = flat_code([0, 3, 29], 30)
    for name, a, b, toks in (("hlit257_hdist1", ll257, [1], [60, 61, 69]), ("hlit286_hdist30", ll286, d30, [60, (258, 1), (24, 4), 69]),
                             ("hlit257_hdist30", ll257, d30, [60, 61, 62, 63]), ("hlit286_hdist1", ll286, [0], [60, 69])):
        h = auto_header(a, b)
        assert (h["hlit"], h["hdist"]) == (int(name[4:7]), int(name[13:]))
        add(name, Deflate().dynamic(a, b, toks, final=True))
    d = _filler(rng, Deflate(), 24577).dynamic(ll286, d30, [60, (258, 24577), (23, 24578), 69], final=True)
    add("hdist30_symbol29", d)
    # hclen 5 (code-length symbols 16, 17, 18, 0, 8: the smallest that can describe a code with an end of block -- 256 symbols of
    # eight bits) and 19 (symbol 15, the last in the order)
    ll8 = [8] * 255 + [0, 8]
    h = _header(257, 1, _cl(s0=1, s8=1), [(8, 0)] * 255 + [(0, 0), (8, 0), (0, 0)], hclen=5)
    add("hclen5", Deflate().dynamic(ll8, [0], [0, 1, 127, 128, 254], final=True, header=h))
    h = auto_header(ll, [1, 1])
    assert h["hclen"] == 19
    cl7 = [2, 3] + [5] * 9 + [6, 6, 6, 7, 7, 6, 6, 2]  # all 19 symbols, the stair's 14 and 15 on the two 7-bit codes
    add("hclen19_7bit_cl_codes", Deflate().dynamic(ll, [1, 1], [97, (258, 1), 255], final=True,
                                                   header=_header(h["hlit"], 2, cl7, encode_lengths(ll[:h["hlit"]] + [1, 1]))))
    # a 16-run that repeats the last literal/length length into the distance lengths: 'a' .. 'f', 256 and 257 on 3 bits,
    # distances 0 .. 7 too
    ll3 = [0] * 258
    for s in (97, 98, 99, 100, 101, 102, 256, 257):
        ll3[s] = 3
    syms = [(18, 97 - 11), (3, 0), (16, 5 - 3), (18, 138 - 11), (18, 15 - 11), (3, 0), (16, 6 - 3), (3, 0), (3, 0), (3, 0)]
    assert lens_from_syms(syms) == ll3 + [3] * 8
    add("run16_across_border", Deflate().dynamic(ll3, [3] * 8, [97, 102, (3, 2), (3, 4), 100], final=True,
                                                 header=_header(258, 8, _cl(s18=1, s3=2, s16=2), syms)))
    # the longest run of zeros that can cross the border: behind 256, 29 literal/length and 29 distance lengths
    ll_z = [0] * 286
    for s in (97, 98, 99, 256):
        ll_z[s] = 2
    d_z = [0] * 29 + [1]
    syms = [(18, 97 - 11), (2, 0), (2, 0), (2, 0), (18, 138 - 11), (18, 18 - 11), (2, 0), (18, 58 - 11), (1, 0)]
    assert lens_from_syms(syms) == ll_z + d_z
    d = Deflate().dynamic(ll_z, d_z, [97, 98, 99], final=True,
                                              header=_header(286, 30, _cl(s18=1, s2=2, s1=2), syms))
    add("run18_of_58_across_border", d)
    # a 16 directly behind a 17: it repeats the zero
    ll_r = [0] * 257
    for s in (97, 98, 110, 256):
        ll_r[s] = 2
    syms = [(18, 97 - 11), (2, 0), (2, 0), (17, 5 - 3), (16, 6 - 3), (2, 0), (18, 138 - 11), (17, 7 - 3), (2, 0), (0, 0)]
    assert lens_from_syms(syms) == ll_r + [0]
    add("run16_behind_17", Deflate().dynamic(ll_r, [0], [97, 110, 98], final=True, header=_header(257, 1, _cl(s2=1, s16=3, s17=3, s18=3, s0=3), syms)))
    add("len258_as_284_31_fixed", Deflate().fixed([7, (258, 1, 284), 8, (258, 2, 284), (258, 1)], final=True))
    ll_x = flat_code([97, 256, 284, 285], 286)
    add("len258_as_284_31_dynamic", Deflate().dynamic(ll_x, [1, 1], [97, (258, 1, 284), (258, 2, 285), (258, 2, 284)], final=True))

    # ---------------- blocks
    d = Deflate().stored(b"", pad=5).stored(b"").stored(b"", pad=255).fixed([65, 66]).stored(b"").dynamic(ll_s, [1], [97, (6, 1)])
    add("empty_stored_blocks", d.stored(b"").stored(b"xyz").stored(b"", final=True, pad=0x55))
    add("empty_fixed_block", Deflate().fixed([], final=True))
    add("empty_fixed_between", Deflate().fixed([72]).fixed([]).fixed([]).stored(b"i").fixed([], final=True))
    add("empty_dynamic_block", Deflate().dynamic(ll_s, [0], [], final=True))
    add("empty_dynamic_between", Deflate().fixed([72]).dynamic(ll_s, [0], []).dynamic(ll, [1, 1], []).fixed([(5, 1)], final=True))
    add("stored_1_and_65535", Deflate().stored(b"Q").stored(rng.bytes(65535), final=True))
    add("empty_fixed_empty_stored_65535", Deflate().fixed([]).stored(b"").stored(rng.bytes(65535)).fixed([], final=True))
    for j in range(8):  # 3 + 9 j + 7 bits of a fixed block: the stored block's header starts at each bit of a byte
        d = Deflate().fixed([200] * j)
        assert d.w.bit_pos() % 8 == (2 + j) % 8
        add("stored_behind_fixed_bit%d" % ((2 + j) % 8), d.stored(rng.bytes(37), pad=255).fixed([201] * j).stored(rng.bytes(5), final=True, pad=0xAA))
    add("final_stored", Deflate().stored(b"final", final=True))
    add("final_fixed", Deflate().fixed([102, 105, (4, 2)], final=True))
    add("final_dynamic", Deflate().dynamic(ll_s, [2, 2, 2, 2], [97, 98, (4, 2)], final=True))
    text = b"".join(b"chr%d\t%d\t%d\tACGT%04d-1\t1\n" % (1 + i % 7, 1000 + 13 * i, 1400 + 13 * i, i % 37) for i in range(1500))
    for name, mode in (("sync", zlib.Z_SYNC_FLUSH), ("full", zlib.Z_FULL_FLUSH), ("partial", zlib.Z_PARTIAL_FLUSH)):
        for level in (1, 6):
            co = zlib.compressobj(level, zlib.DEFLATED, -15)
            s, at = b"", 0
            for cut in (1, 2, 9, 300, 301, 4095, 4097, 20011, 33333, 33334, len(text)):
                s += co.compress(text[at:cut]) + co.flush(mode)
                at = cut
            add("zlib_%s_flush_level%d" % (name, level), (s + co.flush(), text))

    # ---------------- the input ring: 2048 bytes in 1024-byte chunks, a 16-byte mirror
    for k in range(1, 5):
        for dd in range(-9, 9):
            t = 1024 * k + dd
            # a dynamic header whose first bit is bit 0 of byte t
            d = Deflate()
            _place(rng, d, 8 * t)
            assert d.byte_pos() == t
            add("ring_header_at_%d" % t, d.dynamic(ll, dl, [97, 98, (23, 2), 0xC3, (258, 1), 255], final=True))
            # LEN at byte t
            d = Deflate()
            _place(rng, d, 8 * (t - 1))
            d.stored(rng.bytes(40), pad=int(rng.integers(0, 256)))
            assert d.byte_pos() == t + 44
            add("ring_len_at_%d" % t, d.fixed([33], final=True))
            # the 48-bit symbol: its first bit in byte t
            d = _bulk(Deflate(), 24800)
            hb = header_bits(S48_LL, S48_D)
            phase = (k * 18 + dd) % 8
            start = 8 * t + phase - hb  # the block's first bit
            p = start % 8
            _place(rng, d, start - p)
            assert (d.w.bit_pos() + hb + p) // 8 == t
            _sym48(d, rng, p)
            add("ring_sym48_at_%d" % t, d)
    for n in (1023, 1024, 1025, 2047, 2048, 2049, 4096) + tuple(3000 + r for r in range(16)):
        d = Deflate()
        _place(rng, d, 8 * (n - 3))
        stream, want = d.fixed([n % 251], final=True).finish()
        assert len(stream) == n
        add("stream_of_%d_bytes" % n, (stream, want))

    # ---------------- the window (32 KiB) and the flush pieces (4 KiB)
    ks = (0, 1, 2, 63, 64, 65, 257, 258)
    ll_w = flat_code([97, 256, 257, 276, 285], 286)  # lengths 3, 64 (276: 59 .. 66) and 258
    for length in (258, 3, 64):
        for dist in (32768, 32767, 32768 - 257):
            for k in ks:
                # op = -k (mod 4096) at 36864 - k, op = -k (mod 32768) at 65536 - k
                d = _filler(rng, Deflate(), 36864 - k - 1)
                d.dynamic(ll_w, flat_code([28, 29], 30), [97, (length, dist)])
                _filler(rng, d, 65536 - k - 1)
                d.fixed([98, (length, dist), 99], final=True)
                add("win_len%d_dist%d_k%d" % (length, dist, k), d)
    for dist in (1, 2, 3, 7, 8, 63, 64, 65, 127, 128, 129, 257):
        for k in ks:
            d = _filler(rng, Deflate(), 4096 - k - 1)
            d.fixed([98, (258, dist)])
            _filler(rng, d, 32768 - k - 1)
            d.fixed([99, (258, dist), 100], final=True)
            add("periodic_dist%d_k%d" % (dist, k), d)
    for at in (4096, 8192, 32768, 65536):
        d = _filler(rng, Deflate(), at - 1)
        add("literal_lands_on_%d" % at, d.fixed([77, 78], final=True))
    add("stored_crosses_4096", Deflate().fixed([1, 2, 3, (100, 3)]).stored(rng.bytes(5000)).fixed([4], final=True))
    d = _filler(rng, Deflate(), 32000).fixed([1, (5, 1)])
    add("stored_crosses_32768", d.stored(rng.bytes(2000)).fixed([(7, 2006)], final=True))
    for n in (4095, 4096, 4097, 32767, 32768, 32769, 65536):
        add("out_%d_ends_with_literal" % n, _filler(rng, Deflate(), n - 2).fixed([5, 6], final=True))
        add("out_%d_ends_with_match" % n, _filler(rng, Deflate(), n - 101).fixed([5, (100, 51)], final=True))
        add("out_%d_ends_with_stored" % n, _filler(rng, Deflate().fixed([5, (100, 1)]), n, final=True))
    add("out_200", Deflate().fixed([9, (199, 1)], final=True))  # (into a capacity of 100: no 4-KiB check on the way)

    # ---------------- streams zlib refuses
    tail = [97, 98]
    for bits in (2, 5, 15):
        add("bad_single_dist_code_%d_bits" % bits, Deflate().dynamic(ll_s, [bits], [97, (5, 1)] + tail, final=True), False)
        add("bad_single_dist_code_%d_bits_unused" % bits, Deflate().dynamic(ll_s, [0, 0, bits], [97, 98, 99], final=True), False)
    add("bad_match_without_dist_codes", Deflate().dynamic(ll_s, [0], [97, (5, None), ("raw", 0, 9)] + tail, final=True), False)
    add("bad_unused_half_of_1bit_dist", Deflate().dynamic(ll_s, [1], [97, (5, None), ("raw", 1, 1)] + tail, final=True), False)
    add("bad_unused_half_of_1bit_dist_sym15", _filler(rng, Deflate(), 300).dynamic(ll_s, [0] * 15 + [1], [97, (5, None), ("raw", 0x7F, 7)] + tail, final=True), False)
    add("bad_fixed_symbol_286", Deflate().fixed([97, ("ll", 286)] + tail, final=True), False)
    add("bad_fixed_symbol_287", Deflate().fixed([97, ("ll", 287)] + tail, final=True), False)
    add("bad_fixed_dist_30", Deflate().fixed([97, 98, (5, None), ("d", 30)] + tail, final=True), False)
    add("bad_fixed_dist_31", Deflate().fixed([97, 98, (5, None), ("d", 31)] + tail, final=True), False)
    h = _header(257, 1, _cl(s16=1, s3=2, s0=2), [(16, 0), (3, 0)] + [(0, 0)] * 255)
    add("bad_16_first", Deflate().dynamic(ll_s, [0], tail, final=True, header=h), False)
    h = auto_header(ll3, [3] * 8)
    h["syms"] = h["syms"][:-1] + [(16, 3)]  # six more threes where fewer are missing
    add("bad_run_past_the_end", Deflate().dynamic(ll3, [3] * 8, tail, final=True, header=h), False)
    h = auto_header(ll3, [3] * 8)
    h["syms"] = h["syms"][:-1] + [(18, 127)]
    add("bad_zero_run_past_the_end", Deflate().dynamic(ll3, [3] * 8, tail, final=True, header=h), False)
    ll_n = [0] * 258
    for s in (97, 98, 99, 257):
        ll_n[s] = 2
    add("bad_no_end_of_block_code", Deflate().dynamic(ll_n, [1], tail, final=True, eob=False), False)
    # a run of 138 zeros across the border takes the end of block's length with it
    syms = [(18, 97 - 11), (2, 0), (2, 0), (2, 0), (2, 0), (18, 138 - 11), (18, 37 - 11)]
    assert len(lens_from_syms(syms)) == 257 + 19
    add("bad_run18_of_138_across_border", Deflate().dynamic(ll_n, [0], tail, final=True, eob=False, header=_header(257, 19, _cl(s18=1, s2=1), syms)), False)
    # hclen 4 describes zeros only: no end of block
    add("bad_hclen4", Deflate().dynamic(ll_n, [0], tail, final=True, eob=False,
                                        header=_header(257, 1, _cl(s18=1, s0=1), [(18, 127), (18, 120 - 11)], hclen=4)), False)
    h = auto_header(ll_s, [0])
    h["cl_lens"] = [l + 1 if s == max(x for x, _ in h["syms"]) else l for s, l in enumerate(h["cl_lens"])]
    add("bad_incomplete_cl_code", Deflate().dynamic(ll_s, [0], tail, final=True, header=h), False)
    h = auto_header(ll_s, [0])
    h["cl_lens"] = [1 if l else 0 for l in h["cl_lens"]]
    add("bad_oversubscribed_cl_code", Deflate().dynamic(ll_s, [0], tail, final=True, header=h), False)
    ll_i = list(ll_s)
    ll_i[285] = 5
    add("bad_incomplete_ll_code", Deflate().dynamic(ll_i, [0], tail, final=True), False)
    ll_o = list(ll_s)
    ll_o[284] = 4
    add("bad_oversubscribed_ll_code", Deflate().dynamic(ll_o, [0], tail, final=True), False)
    add("bad_incomplete_dist_code", Deflate().dynamic(ll_s, [2, 2, 2], tail, final=True), False)
    add("bad_oversubscribed_dist_code", Deflate().dynamic(ll_s, [1, 1, 1], tail, final=True), False)
    for hlit in (287, 288):  # (a complete code that gives symbol hlit - 1 a length, so that the header says hlit)
        ll_h = flat_code([97, 98, 256, hlit - 1], 288)
        assert auto_header(ll_h, [0])["hlit"] == hlit
        add("bad_hlit_%d" % hlit, Deflate().dynamic(ll_h, [0], tail, final=True), False)
    d_h = flat_code([0, 1, 2, 30], 31)
    assert auto_header(ll_s, d_h)["hdist"] == 31
    add("bad_hdist_31", Deflate().dynamic(ll_s, d_h, tail, final=True), False)
    add("bad_block_type_3", Deflate().fixed([97]).dynamic(ll_s, [0], tail, final=True, btype=3), False)
    add("bad_len_nlen", Deflate().fixed([97]).stored(b"abcdef", final=True, nlen=6), False)
    add("bad_len_nlen_one_bit", Deflate().stored(b"abcdef", final=True, nlen=(6 ^ 0xFFFF) ^ 0x100), False)
    add("bad_distance_past_the_start", Deflate().fixed([97, 98, (3, None), ("d", 2)] + tail, final=True), False)
    add("bad_distance_past_the_start_far", Deflate().stored(rng.bytes(24576)).dynamic(ll_s, S48_D, [(3, None), ("d", 29), ("raw", 0, 13)] + tail, final=True), False)
    return cases


EOB_ONLY = "eob_only_1bit_code"  # valid for zlib, refused by both decoders as an incomplete code (by design)
_CACHE = []


def corpus():
    """[(name, stream, expected bytes or None where zlib refuses the stream)], built once"""
    if not _CACHE:
        cases = _corpus()
        ll = [0] * 257
        ll[256] = 1
        cases.append((EOB_ONLY,) + Deflate().dynamic(ll, [0], [], final=True).finish())
        cases.append((EOB_ONLY + "_between",) + Deflate().fixed([97]).dynamic(ll, [0], []).fixed([98], final=True).finish())
        assert len({c[0] for c in cases}) == len(cases)
        _CACHE.extend(cases)
    return list(_CACHE)


RANDOM_SEEDS = range(200)


def random_streams():
    """the 200 random streams of the suite, built once: [(stream, bytes)]"""
    if not _RANDOM:
        _RANDOM.extend(random_stream(s) for s in RANDOM_SEEDS)
    return list(_RANDOM)


_RANDOM = []


def golden_streams():
    """the libdeflate-made fixtures (tests/golden/deflate/NOTICE): [(name, stream, the bytes zlib inflates it to)]"""
    import os
    folder = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deflate")
    out = []
    for level in (1, 6, 9, 12):
        with open(os.path.join(folder, "fragments_150.level%d.deflate" % level), "rb") as f:
            s = f.read()
        out.append(("libdeflate_level%d" % level, s, zlib.decompress(s, -15)))
    return out


def all_streams():
    """everything the decoders are held to: the corpus, the random streams and the fixtures, as (name, stream, bytes or None)"""
    return corpus() + [("random_%d" % k, s, want) for k, (s, want) in zip(RANDOM_SEEDS, random_streams())] + golden_streams()


def write_corpus_file(path, entries):
    """the file tests/soak/inflate_corpus_check.cpp reads (little-endian u32 lengths): count, then per stream its name, its bytes,
    its kind (0 valid, 1 refused by zlib, 2 valid but the end-of-block-only code) and the expected bytes"""
    import struct
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(entries)))
        for name, stream, want in entries:
            kind = 1 if want is None else 2 if name.startswith(EOB_ONLY) else 0
            n = name.encode()
            f.write(struct.pack("<I", len(n)) + n + struct.pack("<I", len(stream)) + stream)
            f.write(struct.pack("<II", kind, len(want or b"")) + (want or b""))
