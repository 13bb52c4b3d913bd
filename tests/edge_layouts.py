"""Structured region layouts whose results are known in closed form from the generator's own numpy arrays, for the
operation-level edge tests at sizes where the Python restatements are too slow to be the only reference.  Names are
zero-padded so that their bytewise order is their index order; regions come shuffled.
tests/test_primitives_ref_cpu.py checks every closed form against the restatements at small sizes.
Also the sizes and small generators that the edge tests of the three GPU files share."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np


def _names(k):
    return [f"c{i:05d}" for i in range(k)]


def covering(n, seed):
    """one chromosome; the first region by start covers all the others, which are disjoint among themselves"""
    rng = np.random.default_rng(seed)
    m = n - 1
    s = np.concatenate([[0], 10 + 10 * np.arange(m, dtype=np.int64)])
    e = np.concatenate([[10 * m + 100], s[1:] + rng.integers(1, 10, m)])
    order = rng.permutation(n)
    b = np.unique(np.concatenate([s, e]))
    z = np.zeros
    return SimpleNamespace(
        names=_names(1), chrom=z(n, dtype=np.uint32), start=s[order].astype(np.uint32), end=e[order].astype(np.uint32),
        reduce=(z(1, dtype=np.uint32), s[:1].astype(np.uint32), e[:1].astype(np.uint32)),
        cluster0=z(n, dtype=np.uint32),
        disjoin=(z(len(b) - 1, dtype=np.uint32), b[:-1].astype(np.uint32), b[1:].astype(np.uint32)))


def disjoint(n, seed, per_chrom=None, shift=0):
    """disjoint regions separated by gaps >= 1; per_chrom: sorted region k lies on chromosome (k + shift) // per_chrom,
    so with per_chrom = 2048 the segment heads sit on tile firsts (shift 0) or tile lasts (shift 1) of the sorted order"""
    rng = np.random.default_rng(seed)
    w = rng.integers(1, 51, n).astype(np.int64)
    gap = rng.integers(1, 51, n).astype(np.int64)
    s = np.cumsum(w + gap) - w
    e = s + w
    k = np.arange(n, dtype=np.int64)
    c = np.zeros(n, dtype=np.int64) if per_chrom is None else (k + shift) // per_chrom
    n_chrom = int(c[-1]) + 1
    names = _names(n_chrom)
    order = rng.permutation(n)  # input row i is sorted region order[i]
    ci = c[order]
    # neighbour distances: chromosomes in order of first appearance, each sorted by start
    _, first = np.unique(ci, return_index=True)
    appearance = np.empty(n_chrom, dtype=np.int64)
    appearance[np.argsort(first, kind="stable")] = np.arange(n_chrom)
    inner = np.flatnonzero(c[1:] == c[:-1]) + 1  # sorted regions with a predecessor on their chromosome
    nd = gap[inner][np.lexsort((inner, appearance[c[inner]]))]
    lo = np.searchsorted(c, np.arange(n_chrom), "left")
    hi = np.searchsorted(c, np.arange(n_chrom), "right")
    stats, sizes = {}, {}
    for r in range(n_chrom):
        ws = np.sort(w[lo[r]:hi[r]]).tolist()
        m = len(ws)
        median = (ws[m // 2 - 1] + ws[m // 2]) / 2.0 if m % 2 == 0 else float(ws[m // 2])
        stats[names[r]] = (m, int(s[lo[r]]), int(e[hi[r] - 1]), ws[0], ws[-1], sum(ws) / m, median)
        sizes[names[r]] = int(e[hi[r] - 1]) + 10
    size_of = np.array([sizes[nm] for nm in names], dtype=np.int64)

    def distribution(n_bins):
        """with chrom_sizes = sizes: every midpoint lies below its chromosome's size"""
        bin_size = max(int(size_of.max()) // n_bins, 1)
        rid = np.minimum((s + w // 2) // bin_size, n_bins - 1)
        key, cnt = np.unique(c * (1 << 32) + rid, return_counts=True)
        kc, kr = key >> 32, key & 0xFFFFFFFF
        start = kr * bin_size
        stop = np.where(kr == n_bins - 1, size_of[kc], np.minimum(start + bin_size, size_of[kc]))
        return [{"chr": names[a], "start": b, "end": d, "n": m, "rid": r}
                for a, b, d, m, r in zip(kc.tolist(), start.tolist(), stop.tolist(), cnt.tolist(), kr.tolist())]

    u = np.uint32
    return SimpleNamespace(
        names=names, chrom=ci.astype(u), start=s[order].astype(u), end=e[order].astype(u),
        reduce=(c.astype(u), s.astype(u), e.astype(u)), cluster0=order.astype(u), neighbor_distances=nd,
        chromosome_statistics=stats, sizes=sizes, distribution=distribution)


# ------------------------------------------------------------------------------- shared by the GPU edge tests
# sizes on the edges of a lane, a wave, a workgroup and a 2048-element tile of the sort and the scans
EDGE_SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097]
# regions of the structured layouts: the carries of the scans cross two 1024-tile chunk seams
N_SEAMS = 2 * (1 << 21) + 4099


def edge_cases():
    """(n, boundary): one chromosome (boundary None), and two chromosomes whose second begins at sorted index 2048 and
    2047 (at the middle where n is too small for either)"""
    out = []
    for n in EDGE_SIZES:
        out.append((n, None))
        for b in sorted({b for b in (2048, 2047) if b < n} or ({n // 2} if n >= 2 else set())):
            out.append((n, b))
    return out


def split_at(regs, boundary, key=lambda r: r[1]):
    """the regions of a one-chromosome set spread over two chromosomes so that, after the (chromosome, key) sort, the
    second chromosome begins at sorted index `boundary`; key: the start, or what the operation sorts by"""
    order = sorted(range(len(regs)), key=lambda i: key(regs[i]))
    out = list(regs)
    for pos, i in enumerate(order):
        out[i] = ("chr10" if pos < boundary else "chr2", regs[i][1], regs[i][2])  # "chr10" < "chr2" bytewise
    return out


def layout_set(lay):
    from gtars.models import RegionSet

    return RegionSet.from_vectors([lay.names[i] for i in lay.chrom.tolist()], lay.start, lay.end)


def wide_set(seed, n_names):
    """1 to 3 regions on each of n_names chromosomes, shuffled; the names' bytewise order is not their numeric one"""
    rng = np.random.default_rng(seed)
    c = np.repeat(np.arange(n_names), rng.integers(1, 4, n_names))
    s = rng.integers(0, 5000, len(c))
    e = s + rng.integers(0, 400, len(c))
    return [(f"k{int(c[i])}", int(s[i]), int(e[i])) for i in rng.permutation(len(c))]


def long_covers(m, n_far=300, seed=0):
    """Three sets for the folds over a list whose top-2 summary must travel a long way: set 0 is chr1:[0, B), set 1 is
    chr1:[1, B - 1) plus the m regions chr1:[10 k, 10 k + 5), set 2 the m regions chr1:[10 k + 5, 10 k + 9) plus n_far
    disjoint regions on chr2 (k = 1 .. m; B lies above every other end).  In sorted order the first two rows set m1 / s1
    (set 0's end) and m2 (set 1's long end) for the 2 m rows behind them with no head between, and the first chr2 row
    resets them.  cols: per set (chromosome index, start, end), shuffled; full / ex: the closed forms of union_all and of
    the union without each set."""
    rng = np.random.default_rng(seed)
    k = np.arange(1, m + 1, dtype=np.int64)
    top = 10 * m + 1000
    far_s = 20 * np.arange(n_far, dtype=np.int64)
    z = lambda n: np.zeros(n, dtype=np.int64)  # noqa: E731
    cols = [(z(1), z(1), np.array([top], dtype=np.int64)),
            (z(m + 1), np.concatenate([[1], 10 * k]), np.concatenate([[top - 1], 10 * k + 5])),
            (np.concatenate([z(m), z(n_far) + 1]), np.concatenate([10 * k + 5, far_s]), np.concatenate([10 * k + 9, far_s + 10]))]
    shuffled = []
    for c, s, e in cols:
        o = rng.permutation(len(c))
        shuffled.append((c[o], s[o], e[o]))
    far = [("chr2", int(s), int(s) + 10) for s in far_s]
    full = [("chr1", 0, top)] + far
    return SimpleNamespace(names=["chr1", "chr2"], cols=shuffled, full=full,
                           ex=[[("chr1", 1, top - 1)] + far, full, [("chr1", 0, top)]])
