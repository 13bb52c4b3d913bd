"""The generated cases and the comparison helpers that tests/test_overlap_def_cpu.py (the oracle against tests/overlap_def.py) and
tests/test_gpu_overlap_def.py (the device against it) share.  Imports neither ``oracle`` nor ``gtars_amd``."""
import functools

import numpy as np

import overlap_def as od
from overlap_def import KIND_AILIST, KIND_BITS

BOTH = [KIND_BITS, KIND_AILIST]
UNK = 0xFFFFFFFF
U32_MAX = 0xFFFFFFFF
MIN_OVERLAPS = (None, 0, 1, 2, 5, 10)

# name: (seed, n intervals, nq queries, chromosomes, span, max width, law).  Laws: "uniform" -- starts uniform over the span,
# widths uniform below the maximum; "skewed" -- widths = max * u^5 (a few intervals contain hundreds of others, most are short:
# deep AIList nesting at ~600 hits per query instead of ~3 600); "heavy" -- the shape of test_ailist_heavy_nesting: 40 intervals of
# the maximum width at every 100th position, the others shorter than 20; "shifted" -- uniform, every coordinate moved to within
# span + 3 * wmax of 0xFFFFFFFF, a few ends and query ends equal to 0xFFFFFFFF and a few starts equal to 0.
CASES = {
    "small": (1, 50, 300, 1, 200, 30, "uniform"),
    "mid": (2, 10_000, 20_000, 3, 100_000, 400, "uniform"),
    "nested": (3, 10_000, 8_000, 2, 5_000, 3_000, "skewed"),
    "ties": (4, 10_000, 20_000, 40, 100, 20, "uniform"),
    "heavy": (5, 3_040, 4_097, 1, 9_000, 5_000, "heavy"),
    "shifted": (6, 10_000, 20_000, 3, 100_000, 400, "shifted"),
}
NESTED = ("nested", "heavy")


@functools.lru_cache(maxsize=None)
def case(name, nq=None):
    """-> dict of u32 arrays c, s, e, val (index rows) and qc, qs, qe, plus n_chrom.  Every case has ~10 % duplicated rows, ~3 %
    zero-length or inverted index intervals, ~5 % zero-length or inverted queries, ~4 % queries on unknown chromosome ids
    (0xFFFFFFFF and n_chrom + 5), and ~10 % queries that start at some interval's end or end at some interval's start.
    ``nq``: another number of queries on the same index (the index rows are drawn first)."""
    seed, n, nq0, n_chrom, span, wmax, law = CASES[name]
    nq = nq0 if nq is None else nq
    rng = np.random.default_rng(seed)
    c = rng.integers(0, n_chrom, n)
    s = rng.integers(0, span, n)
    if law == "skewed":
        w = 1 + (wmax * rng.random(n) ** 5).astype(np.int64)
    elif law == "heavy":
        w = rng.integers(1, 20, n)
        s[:40], w[:40] = np.arange(0, 4000, 100), wmax
    else:
        w = rng.integers(1, wmax, n)
    e = s + w
    k = rng.choice(n, int(0.03 * n), replace=False)
    e[k] = np.maximum(s[k] - rng.integers(0, 4, len(k)), 0)  # zero-length and inverted intervals
    m = int(0.1 * n)
    dst, src = rng.choice(n, m, replace=False), rng.integers(0, n, m)
    c[dst], s[dst], e[dst] = c[src], s[src], e[src]  # duplicated rows
    val = rng.permutation(n)
    top = rng.choice(n, 8, replace=False)  # (shifted: the rows that get an end of 0xFFFFFFFF / a start of 0)
    qw = 300 if law in ("skewed", "heavy") else 2 * wmax
    qc = rng.integers(0, n_chrom, nq)
    qs = rng.integers(0, span + wmax, nq)
    qe = qs + rng.integers(0, qw, nq)
    k = rng.choice(nq, nq // 10, replace=False)  # touching: the query starts at an end / ends at a start (not a hit by itself)
    i = rng.integers(0, n, len(k))
    h = len(k) // 2
    qc[k] = c[i]
    qs[k[:h]] = e[i[:h]]
    qe[k[:h]] = qs[k[:h]] + rng.integers(0, qw, h)
    qe[k[h:]] = s[i[h:]]
    qs[k[h:]] = np.maximum(qe[k[h:]] - rng.integers(0, qw, len(k) - h), 0)
    k = rng.choice(nq, nq // 20, replace=False)
    qe[k] = np.maximum(qs[k] - rng.integers(0, 4, len(k)), 0)  # zero-length and inverted queries
    k = rng.choice(nq, nq // 25, replace=False)
    qc[k] = np.where(rng.random(len(k)) < 0.5, UNK, n_chrom + 5)
    if law == "shifted":
        base = U32_MAX - (span + 3 * wmax)
        s, e, qs, qe = s + base, e + base, qs + base, qe + base
        e[top[:4]] = U32_MAX
        s[top[4:]] = 0
        qe[rng.choice(nq, 6, replace=False)] = U32_MAX
        qs[rng.choice(nq, 6, replace=False)] = 0
    assert max(int(e.max()), int(qe.max()), int(s.max()), int(qs.max())) <= U32_MAX
    u32 = lambda a: np.ascontiguousarray(a, dtype=np.uint32)
    return dict(c=u32(c), s=u32(s), e=u32(e), val=u32(val), qc=u32(qc), qs=u32(qs), qe=u32(qe), n_chrom=n_chrom)


@functools.lru_cache(maxsize=None)
def model_of(name, kind, nq=None):
    """-> (Model, Hits of the case's whole query batch): computed once, shared by every test, never modified"""
    d = case(name, nq)
    m = od.Model(d["c"], d["s"], d["e"], d["val"], n_chrom=d["n_chrom"], kind=kind)
    return m, m.query(d["qc"], d["qs"], d["qe"])


def same(got, want):
    """exact equality of arrays (or of tuples of arrays), whatever their integer types"""
    if isinstance(want, tuple):
        return len(got) == len(want) and all(same(a, b) for a, b in zip(got, want))
    return np.array_equal(np.asarray(got).astype(np.int64), np.asarray(want).astype(np.int64))


def check_layout(impl, m):
    """stored order, max_len and sub-list offsets of every chromosome; ``impl``: stored / max_len / headers by chromosome"""
    for ch in range(m.n_chrom):
        assert same(impl.stored(ch), m.stored(ch)), ch
        assert impl.max_len(ch) == m.max_len(ch), ch
        assert list(impl.headers(ch)) == m.headers(ch), ch


def check_queries(impl, h, min_overlaps=MIN_OVERLAPS, index_side=(None, 5)):
    """every call of the family on one batch against the model's Hits ``h``, exactly"""
    assert same(impl.tokenize(), h.tokenize())
    for mo in min_overlaps:
        assert same(impl.count_overlaps(mo), h.count_overlaps(mo)), mo
        assert same(impl.any_overlaps(mo), h.any_overlaps(mo)), mo
        assert same(impl.find_overlaps(mo), h.find_overlaps(mo)), mo
    for mo in index_side:
        assert same(impl.find_overlap_indices(mo), h.find_overlap_indices(mo, impl.row_vals)), mo
        assert same(impl.subset_by_overlaps(mo), h.subset_by_overlaps(mo)), mo
        assert same(impl.subset_source_indices(mo), h.subset_source_indices(mo, impl.row_vals)), mo
