"""A plain Python / numpy restatement of gtars-genomicdist/src/signal.rs, the model the signal-matrix tests compare the
library with (not collected as a test): the TSV rules of SignalMatrix::from_tsv, the SIGM version 2 byte layout, the
fold of calc_summary_signal in AIList result order and boxplot_stats / fivenum_median.

The hits and their order come from the oracle's AIList index (``oracle.Index(..., kind=KIND_AILIST).tokenize``), which
shares nothing with the device code.  Python floats are IEEE doubles and every operation below rounds once, so
``hinge - 1.5 * iqr`` rounds twice, as the reference's does.

One divergence is pinned: a column that holds a NaN has no defined order under the reference's comparator
(``partial_cmp(..).unwrap_or(Equal)`` is not a total order there); ``sort_column`` puts NaNs last, in row order.
"""
import gzip
import math
import re
import struct

import numpy as np

import oracle

SIGM_MAGIC = 0x5349474D
SIGM_VERSION = 2
STAT_FIELDS = ("lower_whisker", "lower_hinge", "median", "upper_hinge", "upper_whisker")
NAN_BITS = 0x7FF8000000000000

_U32 = re.compile(rb"\+?[0-9]+\Z")
_F64 = re.compile(rb"([+-]?)(?:(inf|infinity|nan)|((?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?))\Z", re.I)


def bits(x) -> np.ndarray:
    """the uint64 view of f64 data"""
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def from_bits(b: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", b))[0]


# ---- SignalMatrix::from_tsv ----------------------------------------------------------------------------------------
def parse_u32(b: bytes):
    """u32::from_str: an optional '+', digits only; None on failure or overflow"""
    if not _U32.match(b):
        return None
    v = int(b)
    return v if v <= 0xFFFFFFFF else None


def parse_f64(b: bytes):
    """f64::from_str; None on failure"""
    m = _F64.match(b)
    if not m:
        return None
    sign, word, number = m.groups()
    if word is not None:
        v = from_bits(NAN_BITS) if word.lower() == b"nan" else math.inf
    else:
        v = float(number.decode("ascii"))  # correctly rounded; overflow gives inf, underflow 0.0 or a subnormal
    return -v if sign == b"-" else v


def rust_lines(data: bytes):
    """BufRead::lines: a line ends at '\\n' and loses a '\\r' in front of it; what follows the last '\\n' is a line unless empty"""
    pieces = data.split(b"\n")
    out = [p[:-1] if p.endswith(b"\r") else p for p in pieces[:-1]]
    if pieces[-1]:
        out.append(pieces[-1])
    return out


def parse_tsv(data: bytes):
    """-> (condition names, [(chr, start, end)], [[f64]]) with names as bytes; ValueError as from_tsv fails"""
    lines = rust_lines(data)
    if not lines:
        raise ValueError("Empty signal matrix file")
    header = lines[0].split(b"\t")
    if len(header) < 2:
        raise ValueError("Signal matrix must have at least 2 columns")
    cond = header[1:]
    rows, values = [], []
    for line in lines[1:]:
        fields = line.split(b"\t")
        parts = fields[0].split(b"_")
        if len(parts) != 3:
            continue
        start, end = parse_u32(parts[1]), parse_u32(parts[2])
        if start is None or end is None or len(fields) < 1 + len(cond):
            continue
        vals = [parse_f64(f) for f in fields[1:1 + len(cond)]]
        if any(v is None for v in vals):
            continue
        rows.append((parts[0], start, end))
        values.append(vals)
    if not rows:
        raise ValueError("No valid rows in signal matrix")
    return cond, rows, values


def read_tsv(path):
    with open(path, "rb") as f:
        data = f.read()
    return parse_tsv(gzip.decompress(data) if str(path).endswith(".gz") else data)


# ---- SIGM version 2 ------------------------------------------------------------------------------------------------
def sigm_bytes(cond, rows, values) -> bytes:
    """save_bin: the string table holds the chromosome names by first appearance, then the condition names it lacks"""
    table = {}
    for name in [r[0] for r in rows] + list(cond):
        table.setdefault(name, len(table))
    if len(table) > 65536:
        raise ValueError("too many strings")
    out = [struct.pack("<4I", SIGM_MAGIC, SIGM_VERSION, len(rows), len(cond)), struct.pack("<I", len(table))]
    out += [struct.pack("<I", len(s)) + s for s in table]
    out.append(struct.pack("<I", len(cond)) + b"".join(struct.pack("<H", table[c]) for c in cond))
    out.append(b"".join(struct.pack("<H", table[r[0]]) for r in rows))
    out.append(b"".join(struct.pack("<I", r[1]) for r in rows))
    out.append(b"".join(struct.pack("<I", r[2]) for r in rows))
    out.append(np.asarray(values, dtype="<f8").reshape(len(rows), len(cond)).tobytes())
    return b"".join(out)


def parse_sigm(data: bytes):
    """load_bin_from_bytes -> (cond, rows, values as an ndarray); ValueError for every malformed file"""
    pos = 0

    def take(n):
        nonlocal pos
        if pos + n > len(data):
            raise ValueError("Unexpected end of file")
        pos += n
        return data[pos - n:pos]

    def u32():
        return struct.unpack("<I", take(4))[0]

    if u32() != SIGM_MAGIC:
        raise ValueError("Invalid signal matrix file format")
    version = u32()
    if version != SIGM_VERSION:
        raise ValueError(f"Unsupported signal matrix format version {version}")
    n_regions, n_cond = u32(), u32()
    table = [take(u32()) for _ in range(u32())]
    if u32() != n_cond:
        raise ValueError("Condition name count mismatch")
    ids = struct.unpack(f"<{n_cond}H", take(2 * n_cond))
    chr_ids = struct.unpack(f"<{n_regions}H", take(2 * n_regions))
    starts = struct.unpack(f"<{n_regions}I", take(4 * n_regions))
    ends = struct.unpack(f"<{n_regions}I", take(4 * n_regions))
    values = np.frombuffer(take(8 * n_regions * n_cond), dtype="<f8").reshape(n_regions, n_cond)
    if any(i >= len(table) for i in ids + chr_ids):
        raise ValueError("string id outside the table")
    return [table[i] for i in ids], [(table[c], s, e) for c, s, e in zip(chr_ids, starts, ends)], values


# ---- boxplot_stats ---------------------------------------------------------------------------------------------------
def fivenum_median(s):
    n = len(s)
    if n == 0:
        return 0.0
    return (s[n // 2 - 1] + s[n // 2]) / 2.0 if n % 2 == 0 else s[n // 2]


def sort_column(col) -> np.ndarray:
    """the reference's stable sort (equal values, 0.0 and -0.0 among them, keep row order); NaNs last, in row order"""
    col = np.asarray(col, dtype=np.float64)
    key = np.where(col == 0.0, 0.0, col)  # one key for both zeros; numpy's sorts put NaNs last
    return col[np.argsort(key, kind="stable")]


def boxplot_stats(col):
    """(lower whisker, lower hinge, median, upper hinge, upper whisker) of a non-empty column"""
    s = sort_column(col)
    n = len(s)
    if n == 0:
        return (0.0,) * 5
    median = float(fivenum_median(s))
    mid = n // 2
    lower_hinge = float(fivenum_median(s[:mid] if n % 2 == 0 else s[:mid + 1]))
    upper_hinge = float(fivenum_median(s[mid:]))
    iqr = upper_hinge - lower_hinge
    lower_fence = lower_hinge - 1.5 * iqr
    upper_fence = upper_hinge + 1.5 * iqr
    with np.errstate(invalid="ignore"):
        inside_lo, inside_hi = np.flatnonzero(s >= lower_fence), np.flatnonzero(s <= upper_fence)
    lower_whisker = float(s[inside_lo[0]]) if len(inside_lo) else lower_hinge  # the first such value of the sorted column
    upper_whisker = float(s[inside_hi[-1]]) if len(inside_hi) else upper_hinge  # the last
    return (lower_whisker, lower_hinge, median, upper_hinge, upper_whisker)


# ---- calc_summary_signal -----------------------------------------------------------------------------------------------
def hits(m_chrom, m_start, m_end, q_chrom, q_start, q_end, n_chrom):
    """(offsets, row ids) of every query in AIList result order, from the oracle"""
    ix = oracle.Index(m_chrom, m_start, m_end, None, n_chrom=n_chrom, kind=oracle.KIND_AILIST)
    return ix.tokenize(q_chrom, q_start, q_end)


def fold(values, offsets, ids):
    """-> (indices of the queries with a hit, their folded rows): a copy of the first hit's row, every later hit's value
    replacing a smaller one (``if *val > existing[ci]``).  Vectorised over the queries, hit rank by hit rank."""
    values = np.ascontiguousarray(values, dtype=np.float64)
    off = np.asarray(offsets).astype(np.int64)
    cnt = np.diff(off)
    qidx = np.flatnonzero(cnt > 0)
    first, cnt = off[qidx], cnt[qidx]
    acc = values[np.asarray(ids)[first].astype(np.int64)].copy()
    live = np.arange(len(qidx))
    k = 1
    while True:
        live = live[cnt[live] > k]
        if not len(live):
            break
        rows = values[np.asarray(ids)[first[live] + k].astype(np.int64)]
        cur = acc[live]
        with np.errstate(invalid="ignore"):
            take = rows > cur
        cur[take] = rows[take]
        acc[live] = cur
        k += 1
    return qidx, acc


def summary(m_chrom, m_start, m_end, values, q_chrom, q_start, q_end, n_chrom):
    """-> (query indices, R x C result, C x 5 statistics -- 0 x 5 when R == 0); chromosome ids of the matrix's dictionary"""
    off, ids = hits(m_chrom, m_start, m_end, q_chrom, q_start, q_end, n_chrom)
    qidx, res = fold(values, off, ids)
    if not len(qidx):
        return qidx, res, np.zeros((0, 5))
    return qidx, res, np.array([boxplot_stats(res[:, c]) for c in range(res.shape[1])], dtype=np.float64).reshape(-1, 5)
