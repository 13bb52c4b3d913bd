"""Case builders for the device stages of the fused fragment pipeline (gtars_amd/csrc/fragparse.hip) at their
thresholds.  Plain Python / numpy / zlib: no GPU, no torch.

Every builder writes a folder of fragment files and a barcode map under a directory of the caller's and returns a `Case`: the
paths, the switches the case runs under, and a dict of WITNESSES -- numbers computed by a small Python model of the device
layout (line ends in the concatenated text of a batch, 64-byte lanes, 16-KiB chunks, the span of every group of 256 lines, gzip
member offsets, table capacities, sorted positions) that say where the case sits.  tests/test_fragment_edges_cpu.py asserts the
witnesses (so that an edit of a builder cannot move a case off its edge unnoticed), tests/test_gpu_fragment_edges.py runs the
cases on the device.

Which files share a batch.  The host hands the device batches of consecutive files that size themselves by thread timing.  A
case whose point is what lies TOGETHER in one batch (file borders, the sum of the table capacities) therefore starts with a lead
file of exactly 1 MiB whose barcodes are not mapped and runs with GTARS_FRAG_BATCH_MB=1 (a batch grows only while it stays below
1 MiB: the lead file is a batch of its own), GTARS_FRAG_DEVICE_THREADS=1 (the next batch is made when the device is done with
the lead file: the few small files of the case have long been read by then) and GTARS_HOST_THREADS=16.  The case's files are then
the second of two batches, and start at text offset 0 of it; the GPU test reads the number of batches from the library's timing
report (GTARS_HOST_TIMING) and insists on it."""
import gzip
import os
import struct
import zlib

import numpy as np

FP_BYTES = 64            # text bytes per lane of k_frag_lines
FP_CHUNK = 16384         # ... per workgroup
FP_TPB = 256             # lines per workgroup of k_frag_parse
PARSE_LDS = 32768        # bytes of a workgroup's lines that are staged in LDS
CRC_CHUNK = 512
CRC_GROUP = 32768
EM_TPB = 1024            # fragments per workgroup of k_frag_emit

GOLDEN_PEAKS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tokenizers", "peaks.bed")
FILLER = "."             # the sixth column's bytes; no other column holds one (gz_members corrupts only these)

LEAD_ENV = {"GTARS_HOST_THREADS": "16", "GTARS_FRAG_BATCH_MB": "1", "GTARS_FRAG_DEVICE_THREADS": "1"}
LEAD_NAME = "00lead.bed.gz"


# ----------------------------------------------------------------------------------------------------------- building blocks
def line(chrom, start, end, barcode, pad=None, support="1", eol="\n"):
    """A valid fragment line.  `pad`: the line's total length in bytes, line end included -- a sixth column of filler is
    appended to reach it (extra columns are legal: split.rs:84-98 looks at the first five)."""
    head = f"{chrom}\t{start}\t{end}\t{barcode}\t{support}"
    if pad is None:
        return head + eol
    room = pad - len(head) - len(eol)
    if room == 0:
        return head + eol
    if room < 2:
        raise ValueError(f"a line of {len(head) + len(eol)} bytes cannot be padded to {pad}")
    return head + "\t" + FILLER * (room - 1) + eol


def gz_members(text, cuts, levels=(6,), corrupt=None):
    """A multi-member gzip file: gzip.compress of the pieces of `text` (bytes) between the byte positions `cuts` (they need not
    lie on line ends), concatenated.  corrupt=(member, byte_offset): that member is the compressed form of its piece with the
    one byte changed (a filler byte: the parser never reads it), while its trailer keeps the ORIGINAL piece's CRC-32 and ISIZE
    -- a well-formed gzip file whose member `member` fails its CRC because of exactly that data byte."""
    edges = [0] + list(cuts) + [len(text)]
    assert edges == sorted(edges), "cuts must ascend and lie inside the text"
    out = b""
    for k, (a, b) in enumerate(zip(edges, edges[1:])):
        piece = text[a:b]
        level = levels[k % len(levels)]
        if corrupt is not None and corrupt[0] == k:
            at = corrupt[1]
            assert piece[at:at + 1] == FILLER.encode(), "only a filler byte may be changed"
            changed = piece[:at] + b"," + piece[at + 1:]
            out += gzip.compress(changed, level)[:-8] + struct.pack("<II", zlib.crc32(piece), len(piece))
        else:
            out += gzip.compress(piece, level)
    return out


def member_layout(lengths):
    """(off, len) of every member in its file's text"""
    off, out = 0, []
    for n in lengths:
        out.append((off, n))
        off += n
    return out


def frag_hash(key):
    """frag_hash of gtars_amd/csrc/frag_device.h: 32-bit FNV-1a with a final mix"""
    h = 2166136261
    for b in key:
        h = ((h ^ b) * 16777619) & 0xFFFFFFFF
    return h ^ (h >> 15)


def table_capacity(n):
    """slots of a file's barcode table: the smallest power of two >= 2 n + 1"""
    cap = 1
    while cap < 2 * n + 1:
        cap <<= 1
    return cap


def table_slots(barcodes):
    """{barcode: slot} of a file's table: the file's map keys are inserted in byte order, linear probing"""
    cap = table_capacity(len(barcodes))
    taken, out = set(), {}
    for bc in sorted(barcodes, key=lambda s: s.encode()):
        k = frag_hash(bc.encode()) & (cap - 1)
        while k in taken:
            k = (k + 1) & (cap - 1)
        taken.add(k)
        out[bc] = k
    return out


def device_layout(texts):
    """The model of the device's view of one batch.  `texts`: the files' (inflated) bytes in order.  The host appends a newline
    to a file that lacks one and concatenates the files without a separator."""
    texts = [t if (not t or t.endswith(b"\n")) else t + b"\n" for t in texts]
    text = b"".join(texts)
    file_off = np.concatenate([[0], np.cumsum([len(t) for t in texts])]).astype(np.int64)
    nl = np.flatnonzero(np.frombuffer(text, dtype=np.uint8) == 10).astype(np.int64)
    file_line = np.searchsorted(nl, file_off, side="left")  # line ends in front of the file's first byte
    n_files = len(texts)
    groups = []
    for first in range(0, len(nl), FP_TPB):
        last = min(first + FP_TPB, len(nl)) - 1
        span_lo = int(nl[first - 1]) + 1 if first else 0
        span_hi = int(nl[last]) + 1
        span = span_hi - (span_lo & ~15)
        f = int(np.searchsorted(file_line[:n_files], first, side="right")) - 1  # last file with file_line <= first
        one_file = f + 1 >= n_files or int(file_line[f + 1]) > last
        groups.append({"first": first, "last": last, "span_lo": span_lo, "span": span, "staged": span <= PARSE_LDS, "one_file": one_file,
                       "files": int(np.searchsorted(file_line[:n_files], last, side="right")) - f})
    return {"text": text, "n_bytes": len(text), "file_off": file_off, "newlines": nl, "file_line": file_line, "groups": groups,
            "n_chunks": (len(text) + FP_CHUNK - 1) // FP_CHUNK}


DENSE_CHROM, DENSE_ORIGIN, DENSE_STEP, DENSE_N, DENSE_FAR = "chrE", 1000, 10, 4000, 5_000_000


def dense_hits(start, end):
    """ids of a fragment on the dense universe's chromosome (write_dense_universe)"""
    lo = max(0, (start - DENSE_ORIGIN) // DENSE_STEP)
    hi = min(DENSE_N - 1, -((DENSE_ORIGIN - end) // DENSE_STEP) - 1)  # ceil((end - origin) / step) - 1
    return max(0, hi - lo + 1) if end > DENSE_ORIGIN and start < DENSE_ORIGIN + DENSE_N * DENSE_STEP else 0


def write_dense_universe(directory):
    """4000 abutting 10-bp intervals on one chromosome; nothing at DENSE_FAR and beyond"""
    path = os.path.join(str(directory), "dense.bed")
    with open(path, "w") as f:
        for i in range(DENSE_N):
            f.write(f"{DENSE_CHROM}\t{DENSE_ORIGIN + DENSE_STEP * i}\t{DENSE_ORIGIN + DENSE_STEP * (i + 1)}\n")
    return path


def read_peaks():
    return [(c, int(s), int(e)) for c, s, e in (l.split()[:3] for l in open(GOLDEN_PEAKS) if l.strip())]


class Case:
    def __init__(self, name, root):
        self.name = name
        self.dir = os.path.join(str(root), name)
        self.frags = os.path.join(self.dir, "frags")
        self.map = os.path.join(self.dir, "map.tsv")
        self.universe = GOLDEN_PEAKS
        self.env = {}          # the switches the case runs under
        self.waves = None      # batches the device route must report (None: any)
        self.error = None      # regex of the reference's message (None: a good case)
        self.oracle_error = None  # ... and of the oracle's, where the oracle restates the failing rule
        self.twin = None       # the folder of the uncorrupted twin (corrupt= cases)
        self.files = []        # names of the files of the batch the case is about, in order
        self.texts = []        # ... and their inflated bytes
        self.mapped_files = []  # names of the files that must yield tokenized fragments
        self.w = {}            # witnesses

    def path(self, name):
        return os.path.join(self.frags, name)


def _lead_text():
    return (line("chr1", 1000, 2000, "NOBODY", FP_BYTES) * (1 << 14)).encode()  # exactly 1 MiB, 16384 lines, 64 chunks


def write_case(case, files, mapping, lead=False):
    """files: [(name, inflated bytes, bytes on disk or None for plain text)]; mapping: [(stem, barcode, cluster)]"""
    os.makedirs(case.frags, exist_ok=True)
    for name, text, blob in files:
        with open(case.path(name), "wb") as f:
            f.write(text if blob is None else blob)
    if lead:
        with open(case.path(LEAD_NAME), "wb") as f:
            f.write(gzip.compress(_lead_text(), 1))
        case.env.update(LEAD_ENV)
    case.waves = 2 if lead else (1 if len(files) == 1 else None)
    with open(case.map, "w") as f:
        f.write("".join(f"{stem}+{bc}\t{cluster}\n" for stem, bc, cluster in mapping))
    case.files = [name for name, _, _ in files]
    case.texts = [text for _, text, _ in files]
    stems = {stem for stem, _, _ in mapping}
    case.mapped_files = [n for n, text, _ in files if text and n.split(".")[0] in stems]
    caps = [table_capacity(sum(1 for stem, _, _ in mapping if stem == n.split(".")[0])) for n in case.files]
    case.w["capacities"] = caps
    case.w["total_slots"] = sum(caps)
    case.w["key_bits"] = max(1, sum(caps).bit_length())
    case.w["layout"] = device_layout(case.texts)
    return case


class Gen:
    """natural fragment lines over the golden peaks: mostly mapped barcodes, some that are not mapped, some '#' lines"""

    def __init__(self, seed, mapped, unmapped=("NOPE1", "NOPE22")):
        self.rng = np.random.default_rng(seed)
        self.peaks = read_peaks()
        self.mapped, self.unmapped = list(mapped), list(unmapped)

    def fragment(self):
        c, s, e = self.peaks[int(self.rng.integers(0, len(self.peaks)))]
        return c, s + int(self.rng.integers(0, 30)), e + 3

    def natural(self, pad=None, eol="\n", barcode=None):
        r = float(self.rng.random())
        hashed = barcode is None and 0.80 < r < 0.85  # routed, never tokenized
        if barcode is None:
            barcode = self.mapped[int(self.rng.integers(0, len(self.mapped)))] if r < 0.85 or not self.unmapped else \
                self.unmapped[int(self.rng.integers(0, len(self.unmapped)))]
        for _ in range(100):  # (a pad one byte beyond the five columns has no room for "\t" + filler: another fragment fits)
            c, s, e = self.fragment()
            try:
                return line("#" + c if hashed else c, s, e, barcode, pad, eol=eol)
            except ValueError:
                pass
        raise ValueError(f"no line of {pad} bytes with barcode {barcode}")

    def fill(self, total, eol="\n"):
        """natural lines of 70 .. 130 bytes that sum to exactly `total` bytes (total > 130)"""
        out, left = [], total
        while left > 260:
            out.append(self.natural(int(self.rng.integers(70, 131)), eol))
            left -= len(out[-1])
        out.append(self.natural(left, eol))
        assert sum(len(x) for x in out) == total
        return out


BARCODES = ["BC0", "BC1", "BC2", "BC3", "BC4", "BC5", "BC6"]


def _simple_map(stems, barcodes=BARCODES, clusters=3):
    return [(stem, bc, f"k{(i + j) % clusters}") for j, stem in enumerate(stems) for i, bc in enumerate(barcodes)]


# ------------------------------------------------------------------------------------------------- a. line split geometry
def _newline_at(case, pos, crlf=False):
    """one plain-text file with a line end whose '\\n' is byte `pos` of the text (crlf: '\\r' is byte pos - 1)"""
    g = Gen(1000 + pos, BARCODES)
    if crlf:
        lines = g.fill(pos + 1 - 100) + [g.natural(100, eol="\r\n")] + g.fill(3000, eol="\r\n")
    else:
        lines = g.fill(pos + 1) + g.fill(3000)
    text = "".join(lines).encode()
    write_case(case, [("f1.bed", text, None)], _simple_map(["f1"]))
    case.w["pos"] = pos
    return case


def geometry_cases():
    cases = {}
    for pos in (64 * 5 - 1, 64 * 5, 64 * 5 + 1, FP_CHUNK - 1, FP_CHUNK, FP_CHUNK + 1):
        cases[f"a_newline_at_{pos}"] = lambda root, pos=pos: _newline_at(Case(f"a_newline_at_{pos}", root), pos)
    for pos in (64 * 7, FP_CHUNK):
        cases[f"a_crlf_split_at_{pos}"] = lambda root, pos=pos: _newline_at(Case(f"a_crlf_split_at_{pos}", root), pos, crlf=True)

    def whole_chunks(root, total):
        case = Case(f"a_text_of_{total}", root)
        text = "".join(Gen(total, BARCODES).fill(total)).encode()
        return write_case(case, [("f1.bed", text, None)], _simple_map(["f1"]))

    for total in (FP_CHUNK, 2 * FP_CHUNK):
        cases[f"a_text_of_{total}"] = lambda root, total=total: whole_chunks(root, total)

    def long_lines(root):
        case = Case("a_long_lines", root)
        g = Gen(7, BARCODES)
        # a line that covers whole lanes, then one that covers the whole second chunk (it starts in the first and ends in the third)
        lines = g.fill(5000) + [g.natural(300, barcode="BC1")] + g.fill(9000) + [g.natural(40000, barcode="BC2")] + g.fill(2000)
        return write_case(case, [("f1.bed", "".join(lines).encode(), None)], _simple_map(["f1"]))

    cases["a_long_lines"] = long_lines

    def one_line(root):
        case = Case("a_one_line_no_newline", root)
        return write_case(case, [("f1.bed", line("chr17", 7915750, 7915790, "BC3", eol="").encode(), None)], _simple_map(["f1"]))

    cases["a_one_line_no_newline"] = one_line

    def multi(name, make):
        def build(root):
            case = Case(name, root)
            files = make()
            return write_case(case, [(n, t, None) for n, t in files], _simple_map([n.split(".")[0] for n, _ in files]), lead=True)
        cases[name] = build

    def text_of(seed, total=None, n_lines=None):
        g = Gen(seed, BARCODES)
        if total is not None:
            return "".join(g.fill(total)).encode()
        return "".join(g.natural(barcode=BARCODES[k % 7] if k % 5 else None) for k in range(n_lines)).encode()

    multi("a_file_ends_on_chunk", lambda: [("f1.bed", text_of(21, total=FP_CHUNK)), ("f2.bed", text_of(22, n_lines=40))])
    multi("a_empty_file_between", lambda: [("f1.bed", text_of(23, n_lines=30)), ("f2.bed", b""), ("f3.bed", text_of(24, n_lines=30))])
    multi("a_empty_first_and_last", lambda: [("f1.bed", b""), ("f2.bed", text_of(25, n_lines=50)), ("f3.bed", b"")])
    multi("a_48_files_of_3_lines", lambda: [(f"f{k:02d}.bed", text_of(100 + k, n_lines=3)) for k in range(48)])
    for n in (255, 256, 257):
        multi(f"a_first_file_of_{n}_lines", lambda n=n: [("f1.bed", text_of(30 + n, n_lines=n)), ("f2.bed", text_of(31 + n, n_lines=20))])
    return cases


# --------------------------------------------------------------------------------------------------- b. LDS staging threshold
B_MAPPED = ["A", "ABC", "ABCD", "ABCDE", "ABCDEFGHIJKLMNOPQ"]       # 1, 3, 4, 5 and 17 bytes: the masks of the 4-byte compare
B_UNMAPPED = ["B", "ABD", "ABCE", "ABCDF", "ABCDEFGHIJKLMNOPR"]     # same lengths, the last byte differs


def _special_lines():
    """lines that exercise the parser (all good: the reference accepts them)"""
    out = []
    for bc, nb in zip(B_MAPPED, B_UNMAPPED):
        out.append(line("chr17", 7915750, 7915790, bc))
        out.append(line("chr1", "NaN", "-5", nb))           # not mapped: nothing else of the line is looked at
    out.append(line("#chr17", 7915750, 7915790, "ABC"))      # routed, never tokenized
    out.append(line("chrNope", 10, 20, "ABCD"))              # unknown chromosome: the unk id
    out.append(line("chr6", "+157381100", "+157381150", "ABCDE"))
    out.append(line("chr2", 0, 168247790, "A"))
    out.append(line("chr2", 168247750, 4294967295, "A"))
    out.append(line("chrNope", 0, 4294967295, "ABCDEFGHIJKLMNOPQ"))
    out.append(line("chr4", "0000000000000000016270170", "0000000000000000016270200", "ABC"))
    out.append(line("chr4", "0000000000000000000012", "+0000000000000000016270200", "ABCD"))
    return out


def _group_of(g, target, extra=(), last=None, n_lines=FP_TPB):
    """n_lines lines that sum to `target` bytes: the special lines, `extra`, padded natural lines, and `last` as the group's last"""
    fixed = _special_lines() + list(extra)
    tail = [last] if last is not None else []
    n_free = n_lines - len(fixed) - len(tail)
    left = target - sum(len(x) for x in fixed + tail)
    each = left // n_free
    free = [g.natural(each) for _ in range(n_free - 1)]
    free.append(g.natural(left - each * (n_free - 1)))
    # the special lines spread through the group
    lines, step = list(free), max(1, n_free // (len(fixed) + 1))
    for k, x in enumerate(fixed):
        lines.insert(min(len(lines), (k + 1) * step + k), x)
    lines += tail
    assert len(lines) == n_lines and sum(len(x) for x in lines) == target
    return lines


def _b_map(stems):
    return [(stem, bc, f"k{i % 3}") for stem in stems for i, bc in enumerate(B_MAPPED)]


def staging_cases():
    cases = {}

    def first_group(name, span, **kw):
        def build(root):
            case = Case(name, root)
            g = Gen(span, B_MAPPED, B_UNMAPPED)
            lines = _group_of(g, span, **kw) + _group_of(g, 16000)  # the second group is far under the threshold
            return write_case(case, [("f1.bed", "".join(lines).encode(), None)], _b_map(["f1"]))
        cases[name] = build

    first_group("b_span_32768", PARSE_LDS)
    first_group("b_span_32769", PARSE_LDS + 1)
    # the largest span at which a threshold of PARSE_LDS + 16 would still stage, the group's last line short and its barcode in
    # the bytes behind the buffer
    first_group("b_span_32780_barcode_last", PARSE_LDS + 12, last=line("chr17", 7915750, 7915790, "ABCDEFGHIJKLMNOPQ"))
    first_group("b_span_40000_then_under", 40000)

    def one_long_line(root):
        case = Case("b_one_line_of_33k", root)
        g = Gen(33, B_MAPPED, B_UNMAPPED)
        long_line = g.natural(33 << 10, barcode="ABCD")
        lines = _group_of(g, 16000 + len(long_line), extra=[long_line]) + _group_of(g, 16000)
        return write_case(case, [("f1.bed", "".join(lines).encode(), None)], _b_map(["f1"]))

    cases["b_one_line_of_33k"] = one_long_line

    def unaligned(name, span):
        # a short file of three lines in front: the batch's second group of 256 lines starts at a text offset that is no multiple
        # of 16, and ends so that span_hi - (span_lo & ~15) is `span`
        def build(root):
            case = Case(name, root)
            g = Gen(span + 1, B_MAPPED, B_UNMAPPED)
            short = [g.natural(35, barcode="A") for _ in range(3)]
            head = _group_of(g, 16000, n_lines=FP_TPB - 3)          # lines 3 .. 255 of the batch
            span_lo = 105 + 16000
            assert span_lo & 15 == 9
            second = _group_of(g, span - (span_lo & 15))
            files = [("f1.bed", "".join(short).encode(), None), ("f2.bed", "".join(head + second + g.fill(2000)).encode(), None)]
            return write_case(case, files, _b_map(["f1", "f2"]), lead=True)
        cases[name] = build

    unaligned("b_unaligned_span_32768", PARSE_LDS)
    unaligned("b_unaligned_span_32769", PARSE_LDS + 1)

    def failing(name, bad_line, pattern, oracle_pattern):
        def build(root):
            case = Case(name, root)
            g = Gen(len(name), B_MAPPED, B_UNMAPPED)
            lines = _group_of(g, 40000, last=bad_line) + _group_of(g, 16000)
            write_case(case, [("f1.bed", "".join(lines).encode(), None)], _b_map(["f1"]))
            case.error, case.oracle_error = pattern, oracle_pattern
            case.w["bad_line"] = FP_TPB - 1
            return case
        cases[name] = build

    failing("b_error_four_fields", "chr1\t5\t9\tABC\n", "Failed to parse fragments file at line 255: chr1\t5\t9\tABC", "Failed to parse fragments file at line 255")
    failing("b_error_end_overflow", line("chr1", 1, 4294967296, "ABCD"), "Failed to parse end position of a routed fragment", None)
    return cases


# ------------------------------------------------------------------------------------------------------------- c. CRC-32 fold
C1_LENGTHS = (0, 1, 3, 4, 5, 511, 512, 513, 1024, 32767, 32768, 32769, 32768 + 512, 65536, 65537, 3 * 32768)
C1_FILES = ((0, 1, 32769, 3, 65537, 0, 512, 5),          # a zero-length member first and in the middle
            (3, 32768, 4, 513, 65536, 1, 32768 + 512),
            (5, 1, 32767, 511, 1024, 3 * 32768, 0))      # ... and last (the BGZF end marker)


def _gz_text(seed, total):
    """`total` bytes of lines that are mostly filler (a corrupt= byte must be a filler byte)"""
    assert total > 600
    g = Gen(seed, BARCODES)
    out, left = [], total
    while left > 600:
        out.append(g.natural(int(g.rng.integers(150, 300))))
        left -= len(out[-1])
    out.append(g.natural(left))
    return "".join(out).encode()


def crc_cases():
    cases = {}

    def good(root):
        case = Case("c1_member_lengths", root)
        files = []
        for k, lengths in enumerate(C1_FILES):
            lengths = list(lengths)
            # one more member in front of the last makes every file a multiple of 4 bytes: the members' offsets mod 4 on the
            # device do not depend on which files share the batch
            lengths.insert(len(lengths) - 1, (-sum(lengths)) % 4 + 64)
            text = _gz_text(200 + k, sum(lengths))
            cuts = list(np.cumsum(lengths[:-1]))
            files.append((f"f{k + 1}.bed.gz", text, gz_members(text, cuts, levels=(1, 6, 9, 0))))
            case.w.setdefault("members", []).append(member_layout(lengths))
        return write_case(case, files, _simple_map(["f1", "f2", "f3"]))

    cases["c1_member_lengths"] = good
    return cases


# corrupt= files: (name, member lengths, corrupted member, byte of it, the start offset of that member mod 4 must not be 0)
C2_SPECS = (("c2_head_byte_unaligned", (1000, 3000), 1, 0, True),
            ("c2_last_byte_of_513", (2048, 513, 700), 1, 512, False),
            ("c2_last_byte_of_1024", (300, 1024, 700), 1, 1023, False),
            ("c2_byte_511", (5000,), 0, 511, False),
            ("c2_byte_512", (5000,), 0, 512, False),
            ("c2_last_chunk_of_first_group", (65537,), 0, 32768 - 200, False),
            ("c2_first_byte_of_second_group", (65537,), 0, 32768, False),
            ("c2_only_byte_of_third_group", (65537, 500), 0, 65536, False),
            ("c2_middle_member_of_three", (4000, 4000, 4000), 1, 2000, False))


def corrupt_cases():
    cases = {}

    def make(name, lengths, member, byte, unaligned):
        def build(root):
            case = Case(name, root)
            # a slack member in front moves the text under the cuts until the byte to change is a filler byte
            for slack in range(0, 400):
                ls = ([slack] if slack else []) + list(lengths)
                k = member + (1 if slack else 0)
                lay = member_layout(ls)
                text = _gz_text(len(name), sum(ls))
                at = lay[k][0] + byte
                if text[at:at + 1] == FILLER.encode() and (not unaligned or lay[k][0] % 4):
                    break
            else:
                raise AssertionError("no slack puts the byte on filler")
            cuts = list(np.cumsum(ls[:-1]))
            write_case(case, [("f1.bed.gz", text, gz_members(text, cuts, levels=(6, 1), corrupt=(k, byte)))], _simple_map(["f1"]))
            twin = Case(name + "_twin", root)
            write_case(twin, [("f1.bed.gz", text, gz_members(text, cuts, levels=(6, 1)))], _simple_map(["f1"]))
            case.twin = twin
            case.error = "gzip read error"
            case.w.update(members=[lay], member=k, byte=byte, at=at)
            twin.w.update(members=[lay])
            return case
        cases[name] = build

    for spec in C2_SPECS:
        make(*spec)
    return cases


# ---------------------------------------------------------------------------------------------------------- d. sort key width
def _key_width_text(seed, mapped, slots, n_lines=3000):
    """lines over a spread of the mapped barcodes -- those in the highest and lowest occupied slots among them --, with unmapped
    barcodes and '#' lines in between, every barcode again and again far apart"""
    by_slot = sorted(mapped, key=lambda b: slots[b])
    rng = np.random.default_rng(seed)
    pick = by_slot[:4] + by_slot[-4:]
    if len(by_slot) > 8:
        pick += [by_slot[int(i)] for i in rng.choice(len(by_slot), size=min(200, len(by_slot) - 8), replace=False)]
    g = Gen(seed, pick, ("NOPE1", "BC", "ZZ99999", pick[0][:-1] + "X"))
    return "".join(g.natural() for _ in range(n_lines)).encode(), pick


def key_width_cases():
    cases = {}

    def make(name, counts, n_lines=3000):
        def build(root):
            case = Case(name, root)
            files, mapping, used = [], [], []
            for k, n in enumerate(counts):
                stem = f"f{k + 1}"
                mapped = [f"BC{i:05d}" for i in range(n)]
                slots = table_slots(mapped)
                if n:
                    text, pick = _key_width_text(500 + k + len(name), mapped, slots, n_lines)
                    used.append((max(slots[b] for b in pick), max(slots.values())))
                else:
                    text = "".join(Gen(k, ["NOPE1"], ()).natural() for _ in range(200)).encode()
                    used.append((None, None))
                files.append((stem + ".bed.gz", text, gzip.compress(text, 1)))
                mapping += [(stem, bc, f"k{i % 5}") for i, bc in enumerate(mapped)]
            if not mapping:
                mapping = [("elsewhere", "BC00000", "k0")]  # (a map must have a line; no file of the case has this stem)
            write_case(case, files, mapping, lead=len(counts) > 1)
            case.w["highest_used_slot"] = used
            return case
        cases[name] = build

    make("d_slots_1", [0])
    make("d_slots_4", [1])
    make("d_slots_8_two_files", [1, 1])
    make("d_slots_128", [40])
    make("d_slots_256_two_files", [40, 50])
    make("d_slots_32768", [10000])
    make("d_slots_65536", [20000])
    return cases


# ------------------------------------------------------------------------------------ e. regrouping and the capacity refill
E_BARCODES = ["E0", "E1", "E2", "E3", "E4", "E5"]


def _emit_case(case, recs, universe):
    """recs: [(barcode, chrom, start, end, tag)] in line order.  Witnesses: the sorted position of every tokenized fragment
    (stable sort by the barcode's slot), run starts, the ids the device has to hold."""
    slots = table_slots(E_BARCODES)
    text = "".join(line(c, s, e, bc) for bc, c, s, e, _ in recs).encode()
    write_case(case, [("f1.bed", text, None)], [("f1", bc, f"k{i % 2}") for i, bc in enumerate(E_BARCODES)])
    case.universe = universe
    tok = [i for i, r in enumerate(recs) if r[0] in slots and not r[1].startswith("#")]
    order = sorted(tok, key=lambda i: slots[recs[i][0]])  # (stable)
    keys = [slots[recs[i][0]] for i in order]
    case.w["n_tokenized"] = len(order)
    case.w["run_starts"] = [j for j in range(len(order)) if j == 0 or keys[j] != keys[j - 1]]
    case.w["tagged"] = {}
    for j, i in enumerate(order):
        if recs[i][4]:
            case.w["tagged"].setdefault(recs[i][4], []).append(j)
    if universe != GOLDEN_PEAKS:
        hits = [dense_hits(recs[i][2], recs[i][3]) if recs[i][1] == DENSE_CHROM else 0 for i in order]
        case.w["hits"] = hits
        case.w["n_ids"] = sum(hits)                      # what the tokenizer returns: the guess is 2 n + 1024
        case.w["n_emitted"] = sum(max(h, 1) for h in hits)  # ... and with the unk fills
    return case


def _noise(rng, k):
    """lines that are not tokenized: an unmapped barcode, a '#' chromosome"""
    return ("NOPE", DENSE_CHROM, 1000, 1100, None) if k % 2 else ("E1", "#" + DENSE_CHROM, 1000, 1100, None)


def emit_cases(dense_bed):
    cases = {}
    by_slot = sorted(E_BARCODES, key=lambda b: table_slots(E_BARCODES)[b])
    low, second = by_slot[0], by_slot[1]

    def dense_frag(rng):
        s = DENSE_ORIGIN + 3 + int(rng.integers(0, DENSE_STEP * (DENSE_N - 20)))
        return DENSE_CHROM, s, s + 80   # 9 intervals (8 when it starts on an interval's first base)

    def counts(name, n, dense):
        def build(root):
            case = Case(name, root)
            rng = np.random.default_rng(n)
            g = Gen(n, E_BARCODES)
            recs = []
            for k in range(n):
                bc = E_BARCODES[int(rng.integers(0, 6))] if k >= 6 else E_BARCODES[k]
                recs.append((bc,) + (dense_frag(rng) if dense else g.fragment()) + (None,))
                if k % 9 == 4:
                    recs.append(_noise(rng, k))
            return _emit_case(case, recs, dense_bed if dense else GOLDEN_PEAKS)
        cases[name] = build

    for n in (1023, 1024, 1025, 2048, 2049):
        counts(f"e_dense_{n}", n, True)
        counts(f"e_sparse_{n}", n, False)

    def placed(name, n_low, special_at, special, n_other=300):
        """the barcode of the lowest slot has n_low fragments; those numbered `special_at` (line order = sorted position) are
        `special`; the other barcodes' fragments lie between them in the text"""
        def build(root):
            case = Case(name, root)
            rng = np.random.default_rng(len(name))
            recs, k_low, k_other = [], 0, 0
            while k_low < n_low or k_other < n_other:
                if k_low < n_low and (k_other >= n_other or rng.random() < n_low / (n_low + n_other)):
                    if k_low in special_at:
                        recs.append((low,) + special + ("special",))
                    else:
                        recs.append((low,) + dense_frag(rng) + (None,))
                    k_low += 1
                else:
                    recs.append((by_slot[1 + k_other % 5],) + dense_frag(rng) + ("second" if by_slot[1 + k_other % 5] == second else None,))
                    k_other += 1
                    if k_other % 7 == 0:
                        recs.append(_noise(rng, k_other))
            return _emit_case(case, recs, dense_bed)
        cases[name] = build

    far = (DENSE_CHROM, DENSE_FAR, DENSE_FAR + 80)
    placed("e_run_starts_at_1024", EM_TPB, (), far)                 # the lowest slot's run is positions 0 .. 1023
    placed("e_run_starts_at_1023", EM_TPB - 1, (), far)             # ... 0 .. 1022: the next run opens a chunk's last position
    placed("e_unk_at_1023_and_1024", 1100, (1023, 1024), far)
    placed("e_300_hits_at_1023", 1100, (1023,), (DENSE_CHROM, DENSE_ORIGIN + 5000, DENSE_ORIGIN + 8000))

    def unk_opens(root):
        # run of `low`: positions 0 .. 1023; the second slot's run opens at 1024 with a zero-hit fragment
        case = Case("e_unk_opens_run_at_1024", root)
        rng = np.random.default_rng(77)
        recs = [(second,) + far + ("special",)]
        for k in range(EM_TPB):
            recs.append((low,) + dense_frag(rng) + (None,))
            if k % 3 == 0:
                recs.append((second,) + dense_frag(rng) + (None,))
        return _emit_case(case, recs, dense_bed)

    cases["e_unk_opens_run_at_1024"] = unk_opens

    def all_unk(root):
        case = Case("e_all_unk", root)
        recs = [(E_BARCODES[k % 6], DENSE_CHROM, DENSE_FAR + 7 * k, DENSE_FAR + 7 * k + 50, None) for k in range(1500)]
        return _emit_case(case, recs, dense_bed)

    cases["e_all_unk"] = all_unk

    def one_fragment(root):
        case = Case("e_one_fragment", root)
        recs = [_noise(None, k) for k in range(40)] + [("E3", DENSE_CHROM, 2003, 2083, "special")] + [_noise(None, k) for k in range(40)]
        return _emit_case(case, recs, dense_bed)

    cases["e_one_fragment"] = one_fragment
    return cases


def all_cases(dense_bed):
    """{name: builder(root) -> Case}"""
    cases = {}
    for part in (geometry_cases(), staging_cases(), crc_cases(), corrupt_cases(), key_width_cases(), emit_cases(dense_bed)):
        cases.update(part)
    return cases


# the names, for parametrising (the builders need no universe file to be NAMED)
CASE_NAMES = sorted(all_cases(None))
