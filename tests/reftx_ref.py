"""K19 restated in plain Python, the way the reference computes it: linear scans over the exon offsets as in
gtars-refget/src/transcripts/mapper.rs:239-475, hashlib and base64 for the digests, a literal reverse-complement table
(sequence.rs:36-53), and the .reftx v2 encoder and decoder (store.rs:139-160, 389-463, 590-688).  A transcript is a dict:
accession, gene, digest (24 bytes), strand (+1 / -1), cds_start, cds_end (int or None), exons [(start, end)], mane (flags
byte).  Statuses are the library's (csrc/reftx_core.h)."""
import base64
import hashlib
import struct

OK, NOT_FOUND, NON_CODING, OUTSIDE_CDS, OUTSIDE_TRANSCRIPT, UTR5_OVERFLOW, UTR3_OVERFLOW, INVALID_OFFSET, NOT_EXONIC, BAD_KIND, BAD_EXONS = range(11)
SEQ_OK, SEQ_NOT_FOUND, SEQ_NO_SEQUENCE, SEQ_PAST_END, SEQ_BAD_EXONS = range(5)
U64 = (1 << 64) - 1
NONE = 0xFFFFFFFF


def sha512t24u(data: bytes) -> str:
    return base64.urlsafe_b64encode(hashlib.sha512(data).digest()[:24]).decode("ascii")


def digest_bytes(text: str) -> bytes:
    text = text[3:] if text.startswith("SQ.") else text
    return base64.urlsafe_b64decode(text)


def accession_of(digest: bytes) -> str:
    return "SQ." + base64.urlsafe_b64encode(digest).decode("ascii")


def make_tx(accession, digest, strand, exons, cds=(None, None), gene="", mane=0):
    return {"accession": accession, "gene": gene, "digest": bytes(digest), "strand": strand, "cds_start": cds[0], "cds_end": cds[1],
            "exons": [tuple(e) for e in exons], "mane": mane}


# ---- the container ---------------------------------------------------------------------------------------------------
def fnv1a(data: bytes) -> int:
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & U64
    return h


def encode_record(tx) -> bytes:
    acc, gene = tx["accession"].encode(), tx["gene"].encode()
    if len(acc) > 255 or len(gene) > 255:
        raise ValueError("exceeds 255-byte .reftx limit")
    out = bytes([len(acc)]) + acc + bytes([len(gene)]) + gene + tx["digest"] + struct.pack("<bB", tx["strand"], tx["mane"])
    out += struct.pack("<IIH", NONE if tx["cds_start"] is None else tx["cds_start"], NONE if tx["cds_end"] is None else tx["cds_end"],
                       len(tx["exons"]))
    for s, e in tx["exons"]:
        out += struct.pack("<II", s, e)
    return out


def encode(transcripts) -> bytes:
    order = sorted(transcripts, key=lambda t: fnv1a(t["accession"].encode()))  # (stable, like sort_by_key)
    body, index, mane = b"", [], []
    at = 40
    for tx in order:
        index.append((fnv1a(tx["accession"].encode()), at))
        if tx["mane"] & 1:
            mane.append((fnv1a(tx["gene"].upper().encode()), at))
        rec = encode_record(tx)
        body += rec
        at += len(rec)
    index_off = at
    tail = b"".join(struct.pack("<QQ", h, o) for h, o in index)
    mane_off = 0
    if mane:
        mane.sort(key=lambda e: e[0])
        mane_off = index_off + len(tail)
        tail += struct.pack("<Q", len(mane)) + b"".join(struct.pack("<QQ", h, o) for h, o in mane)
    return b"RFTX" + struct.pack("<IQQQQ", 2, len(order), index_off, mane_off, 0) + body + tail


def decode_record(data: bytes, at: int, bound: int):
    """the record at data[at:bound]; ValueError when it does not fit"""
    view = memoryview(data)[at:bound]  # (no copy: the window reaches to the index whatever the record's length)
    pos = 0

    def take(k):
        nonlocal pos
        if pos + k > len(view):
            raise ValueError("record does not fit")
        piece = bytes(view[pos:pos + k])
        pos += k
        return piece

    acc = take(take(1)[0]).decode()
    gene = take(take(1)[0]).decode()
    digest = take(24)
    strand, mane = struct.unpack("<bB", take(2))
    if strand not in (1, -1):
        raise ValueError("bad strand")
    cds_s, cds_e, n = struct.unpack("<IIH", take(10))
    exons = [struct.unpack("<II", take(8)) for _ in range(n)]
    return make_tx(acc, digest, strand, exons, (None if cds_s == NONE else cds_s, None if cds_e == NONE else cds_e), gene, mane)


def decode(data: bytes):
    """-> (transcripts in index order, has_mane_index); ValueError for anything that is not a whole v2 store"""
    if len(data) < 40:
        raise ValueError("File too small for header")
    if data[:4] != b"RFTX":
        raise ValueError("Invalid magic number: expected RFTX")
    version, count, index_off, mane_off, _ = struct.unpack("<IQQQQ", data[4:40])
    if version != 2:
        raise ValueError(f"Unsupported format version: {version}")
    if index_off < 40 or index_off + 16 * count > len(data):
        raise ValueError("the accession index does not fit")
    out = []
    for i in range(count):
        _, at = struct.unpack("<QQ", data[index_off + 16 * i:index_off + 16 * i + 16])
        if at < 40 or at > index_off:
            raise ValueError("record does not fit")
        out.append(decode_record(data, at, index_off))
    if mane_off:
        if mane_off + 8 > len(data):
            raise ValueError("the MANE index does not fit")
        (n_mane,) = struct.unpack("<Q", data[mane_off:mane_off + 8])
        if mane_off + 8 + 16 * n_mane > len(data):
            raise ValueError("the MANE index does not fit")
    return out, mane_off != 0


def lookup(transcripts, accession):
    return next((t for t in transcripts if t["accession"] == accession), None)


def lookup_mane(transcripts, gene):
    return next((t for t in transcripts if t["mane"] & 1 and t["gene"].upper() == gene.upper()), None)


# ---- the mapper: mapper.rs, scan for scan --------------------------------------------------------------------------------
def exons_ok(tx) -> bool:
    """ascending and disjoint: what the library's tables require of a transcript (status 10 otherwise)"""
    ex = tx["exons"]
    return all(s <= e for s, e in ex) and all(ex[k][1] <= ex[k + 1][0] for k in range(len(ex) - 1))


def exon_offsets(tx):
    """(tx_start, tx_end, g_start, g_end) per exon in transcript order"""
    out, pos = [], 0
    for s, e in (tx["exons"] if tx["strand"] > 0 else reversed(tx["exons"])):
        out.append((pos, pos + (e - s), s, e))
        pos += e - s
    return out


def transcript_to_genomic(tx, tx_pos, offsets):
    for ts, te, gs, ge in offsets:
        if ts <= tx_pos < te:
            return gs + (tx_pos - ts) if tx["strand"] > 0 else ge - 1 - (tx_pos - ts)
    return None


def genomic_to_transcript(tx, g_pos, offsets):
    for ts, te, gs, ge in offsets:
        if gs <= g_pos < ge:
            return ts + (g_pos - gs if tx["strand"] > 0 else ge - 1 - g_pos)
    return None


def cds_tx_bounds(tx, offsets):
    if tx["cds_start"] is None or tx["cds_end"] is None or tx["cds_end"] == 0:
        return None
    a = genomic_to_transcript(tx, tx["cds_start"], offsets)
    b = genomic_to_transcript(tx, tx["cds_end"] - 1, offsets)
    if a is None or b is None:
        return None
    return min(a, b), max(a, b) + 1


def is_exon_boundary(tx_pos, offsets, positive):
    for i, (ts, te, _, _) in enumerate(offsets):
        if positive and tx_pos + 1 == te and i + 1 < len(offsets):
            return True
        if not positive and tx_pos == ts and i > 0:
            return True
    return False


def apply_offset(tx, offsets, tx_pos, offset):
    if offset == 0:
        g = transcript_to_genomic(tx, tx_pos, offsets)
        return (OK, g) if g is not None else (OUTSIDE_TRANSCRIPT, 0)
    positive = offset > 0
    if not is_exon_boundary(tx_pos, offsets, positive):
        return INVALID_OFFSET, 0
    anchor = transcript_to_genomic(tx, tx_pos, offsets)
    g = anchor + abs(offset) if positive == (tx["strand"] > 0) else anchor - abs(offset)
    return (OK, g) if 0 <= g <= U64 else (INVALID_OFFSET, 0)


def c_to_g(tx, c_pos, offset=0, star=False):
    if tx is None:
        return NOT_FOUND, 0
    if not exons_ok(tx):
        return BAD_EXONS, 0
    offsets = exon_offsets(tx)
    bounds = cds_tx_bounds(tx, offsets)
    if bounds is None:
        return NON_CODING, 0
    lo, hi = bounds
    length = offsets[-1][1] if offsets else 0
    if star:
        if c_pos <= 0 or hi + (c_pos - 1) >= length:
            return UTR3_OVERFLOW, 0
        tx_pos = hi + (c_pos - 1)
    elif c_pos > 0:
        tx_pos = lo + c_pos - 1
        if tx_pos >= hi:
            return OUTSIDE_CDS, 0
    elif c_pos < 0:
        if -c_pos > lo:
            return UTR5_OVERFLOW, 0
        tx_pos = lo + c_pos
    else:
        return OUTSIDE_CDS, 0
    return apply_offset(tx, offsets, tx_pos, offset)


def n_to_g(tx, n_pos, offset=0):
    if tx is None:
        return NOT_FOUND, 0
    if not exons_ok(tx):
        return BAD_EXONS, 0
    offsets = exon_offsets(tx)
    length = offsets[-1][1] if offsets else 0
    if n_pos <= 0 or n_pos - 1 >= length:
        return OUTSIDE_TRANSCRIPT, 0
    return apply_offset(tx, offsets, n_pos - 1, offset)


def g_to_tx(tx, g_pos):
    if tx is None:
        return NOT_FOUND, 0
    if not exons_ok(tx):
        return BAD_EXONS, 0
    r = genomic_to_transcript(tx, g_pos, exon_offsets(tx))
    return (OK, r) if r is not None else (NOT_EXONIC, 0)


def map_rows(transcripts, rows):
    """rows of (accession, kind "c" / "n" / "g", pos, offset, star) -> (values, statuses)"""
    by_acc = {t["accession"]: t for t in transcripts}
    values, statuses = [], []
    for acc, kind, pos, offset, star in rows:
        tx = by_acc.get(acc)
        st, v = c_to_g(tx, pos, offset, star) if kind == "c" else n_to_g(tx, pos, offset) if kind == "n" else g_to_tx(tx, pos)
        values.append(v if st == OK else 0)
        statuses.append(st)
    return values, statuses


# ---- sequences -----------------------------------------------------------------------------------------------------------
COMPLEMENT = {ord("A"): ord("T"), ord("T"): ord("A"), ord("C"): ord("G"), ord("G"): ord("C"), ord("N"): ord("N"),
              ord("a"): ord("t"), ord("t"): ord("a"), ord("c"): ord("g"), ord("g"): ord("c"), ord("n"): ord("n")}


def reverse_complement(seq: bytes) -> bytes:
    return bytes(COMPLEMENT.get(b, ord("N")) for b in reversed(seq))


def refget_digests(seqs):
    """chromosome name -> sha512t24u of its upper-cased bytes"""
    return {name: sha512t24u(s.upper()) for name, s in seqs.items()}


def mature(seqs, tx):
    """(status, bytes) of one transcript over an assembly {name: bytes}: the refget store holds the sequences upper-cased
    (gtars-refget/src/fasta.rs:123), concat_regions cuts the non-empty regions out of it and reverse-complements the
    whole for a reverse-strand transcript"""
    if tx is None:
        return SEQ_NOT_FOUND, b""
    if not exons_ok(tx):
        return SEQ_BAD_EXONS, b""
    ranges = [(s, e) for s, e in tx["exons"] if s < e]
    if not ranges:
        return SEQ_OK, b""
    by_digest = {}
    for name, s in seqs.items():
        by_digest.setdefault(digest_bytes(sha512t24u(s.upper())), s.upper())
    chrom = by_digest.get(tx["digest"])
    if chrom is None:
        return SEQ_NO_SEQUENCE, b""
    if any(e > len(chrom) for _, e in ranges):
        return SEQ_PAST_END, b""
    seq = b"".join(chrom[s:e] for s, e in ranges)
    return SEQ_OK, reverse_complement(seq) if tx["strand"] < 0 else seq
