"""Plain-Python restatement of the sequence statistics of gtars-genomicdist: calc_gc_content / calc_dinucl_freq
(statistics.rs:331-483), Dinucleotide::from_bytes (models.rs:467-492), the range rule of seq_from_region (models.rs:190-210),
the FASTA reading rule of include/gtars_amd_host.h and the .fab layout (models.rs:229-412).  Test infrastructure only: the
product path never imports it, and nothing here calls the library.

A region set is a list of (chr, start, end) in set order; an assembly is a dict name -> bytes.
"""
from __future__ import annotations

import operator
import struct

DINUCL_ORDER = ["Aa", "Ac", "Ag", "At", "Ca", "Cc", "Cg", "Ct", "Ga", "Gc", "Gg", "Gt", "Ta", "Tc", "Tg", "Tt"]
# byte -> code A C G T = 0 1 2 3 in either case, 4 for every other byte; and code -> 5 * code
_CODE = bytes({65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}.get(b, 4) for b in range(256))
_TIMES5 = bytes(min(5 * b, 255) for b in range(256))
_WS = b" \t\n\v\f\r"


# ---- readers ------------------------------------------------------------------------------------------------------------
def read_fasta_records(path):
    """(name, sequence) per record in file order: the name is the header behind '>' up to the first whitespace, the sequence
    the following lines stripped of trailing whitespace and joined"""
    data = open(path, "rb").read()
    if data and data[:1] != b">":
        raise ValueError("Expected > at record start")
    recs = []
    for line in data.split(b"\n"):
        line = line.rstrip(_WS)
        if line[:1] == b">":
            head = line[1:]
            k = 0
            while k < len(head) and head[k:k + 1] not in (b" ", b"\t", b"\v", b"\f", b"\r"):
                k += 1
            recs.append([head[:k].decode(), bytearray()])
        elif line:
            recs[-1][1] += line
    return [(n, bytes(s)) for n, s in recs]


def read_fasta(path):
    """HashMap::insert per record: a repeated name keeps the last one (dict order: first appearance of the name)"""
    out = {}
    for name, seq in read_fasta_records(path):
        out[name] = seq
    return out


def pack_fab(records):
    """the .fab bytes of (name, sequence) records: magic, version 1, n, the index, the sequences back to back"""
    names = [n.encode() for n, _ in records]
    offset = 4 + 1 + 4 + sum(2 + len(n) + 8 + 8 for n in names)
    out = b"GFAB" + struct.pack("<B", 1) + struct.pack("<I", len(records))
    for n, (_, seq) in zip(names, records):
        out += struct.pack("<H", len(n)) + n + struct.pack("<Q", offset) + struct.pack("<Q", len(seq))
        offset += len(seq)
    return out + b"".join(seq for _, seq in records)


def read_fab(data):
    """name -> bytes of a .fab image; the last entry of a name wins"""
    if len(data) < 9:
        raise ValueError("too short")
    if data[:4] != b"GFAB":
        raise ValueError("bad magic bytes")
    if data[4] != 1:
        raise ValueError("unsupported version")
    (n,) = struct.unpack_from("<I", data, 5)
    pos, out = 9, {}
    for _ in range(n):
        if pos + 2 > len(data):
            raise ValueError("truncated index")
        (name_len,) = struct.unpack_from("<H", data, pos)
        pos += 2
        if pos + name_len + 16 > len(data):
            raise ValueError("truncated index entry")
        name = data[pos:pos + name_len].decode()
        pos += name_len
        offset, length = struct.unpack_from("<QQ", data, pos)
        pos += 16
        if offset + length > len(data):
            raise ValueError("beyond file boundary")
        out[name] = data[offset:offset + length]
    return out


# ---- statistics.rs:331-483 ----------------------------------------------------------------------------------------------
def iter_chroms(regions):
    """region_set.rs:399-408: chromosome names in order of first appearance"""
    seen = []
    for chr_, _, _ in regions:
        if chr_ not in seen:
            seen.append(chr_)
    return seen


def get_sequence(genome, chr_, start, end):
    if chr_ not in genome:
        raise LookupError(f"Unknown chromosome found in region set: {chr_}")
    seq = genome[chr_]
    if end <= len(seq) and start <= end:
        return seq[start:end]
    raise LookupError(f"Invalid range: start={start}, end={end} for chromosome {chr_} with length {len(seq)}")


def _rows(regions, genome, ignore_unk_chroms):
    """the (region, sequence) pairs the reference's two loops reach, in their order"""
    for chr_ in iter_chroms(regions):
        if ignore_unk_chroms and chr_ not in genome:
            continue
        for region in regions:
            if region[0] != chr_:
                continue
            try:
                seq = get_sequence(genome, *region)
            except LookupError as e:
                if ignore_unk_chroms:
                    continue
                raise RuntimeError(f"{region[0]} {region[1]} {region[2]}: {e}") from None
            yield region, seq


def gc_count(seq):
    """bytes whose to_ascii_lowercase is g or c"""
    return seq.count(b"G") + seq.count(b"C") + seq.count(b"g") + seq.count(b"c")


def calc_gc_content(regions, genome, ignore_unk_chroms=False):
    out = []
    for _, seq in _rows(regions, genome, ignore_unk_chroms):
        total = len(seq)
        out.append(gc_count(seq) / total if total > 0 else 0.0)
    return out


def dinucl_counts(seq):
    """16 counts in DINUCL_ORDER over seq.windows(2); a window with a byte outside ACGTacgt is void"""
    if len(seq) < 2:
        return [0] * 16
    codes = seq.translate(_CODE)
    # window i as 5 * code(seq[i]) + code(seq[i + 1]): 5 a + b with a, b < 4 for the 16 dinucleotides, anything else void
    windows = bytes(map(operator.add, codes[:-1].translate(_TIMES5), codes[1:]))
    return [windows.count(bytes([5 * a + b])) for a in range(4) for b in range(4)]


def calc_dinucl_counts(regions, genome, ignore_unk_chroms=False):
    """(labels, integer count rows)"""
    labels, rows = [], []
    for region, seq in _rows(regions, genome, ignore_unk_chroms):
        labels.append(f"{region[0]}_{region[1]}_{region[2]}")
        rows.append(dinucl_counts(seq))
    return labels, rows


def calc_dinucl_freq(regions, genome, raw_counts=False, ignore_unk_chroms=False):
    labels, rows = calc_dinucl_counts(regions, genome, ignore_unk_chroms)
    out = []
    for counts in rows:
        total = sum(counts)
        if raw_counts:
            out.append([float(c) for c in counts])
        elif total > 0:
            out.append([(c / total) * 100.0 for c in counts])
        else:
            out.append([0.0] * 16)
    return labels, out
