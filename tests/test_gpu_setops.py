"""Region-set algebra on the MI355X (csrc/setops.hip) against the plain-Python restatement tests/setops_ref.py:
seeded random differentials of every operation, exact equality throughout (``==`` on the f64 metrics too)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_layouts as E  # noqa: E402
import setops_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

TOP = 0xFFFFFFFF
# first appearance differs from the bytewise order ("chr10" < "chr1_alt" < "chr2" < "chrM" < "chrX")
NAMES_A = ["chr2", "chr10", "chr1_alt", "chrX", "chrM"]
NAMES_B = ["chrX", "chr10", "chr2", "chrZ", "chr1_alt"]  # chrM only in a, chrZ only in b


def _rs(regs):
    from gtars.models import RegionSet

    return RegionSet.from_vectors([r[0] for r in regs], [r[1] for r in regs], [r[2] for r in regs])


def _tuples(rs):
    names, ids, s, e = rs.chrom_names, rs.chrom_ids, rs.starts, rs.ends
    return [(names[int(ids[i])], int(s[i]), int(e[i])) for i in range(len(rs))]


def _random_set(rng, n, names, inverted, span=20_000):
    """duplicates, nested, touching and zero-width regions, ends near 2^32 - 1; inverted: None, one name or 'all'"""
    c = rng.choice(names, n)
    s = rng.integers(0, span, n)
    w = rng.choice([0, 1, 5, 50, 400, 3000], n, p=[0.08, 0.12, 0.3, 0.3, 0.15, 0.05]) + rng.integers(0, 10, n)
    w[rng.random(n) < 0.05] = 0
    e = s + w
    top = rng.random(n) < 0.03
    s[top] = TOP - rng.integers(0, 2000, top.sum())
    e[top] = np.minimum(s[top] + rng.integers(0, 3000, top.sum()), TOP)
    regs = [(str(c[i]), int(s[i]), int(e[i])) for i in range(n)]
    # touching: a region that starts where an earlier one ends; duplicates; nested
    for k in rng.integers(0, n, n // 20):
        ch, _, en = regs[k]
        regs.append((ch, en, min(en + int(rng.integers(0, 100)), TOP)))
    regs += [regs[k] for k in rng.integers(0, len(regs), n // 20)]
    for k in rng.integers(0, n, n // 40):
        ch, st, en = regs[k]
        if en - st > 2:
            regs.append((ch, st + 1, en - 1))
    if inverted is not None:
        for k in rng.integers(0, len(regs), max(1, n // 50)):
            ch, st, _ = regs[k]
            if inverted == "all" or ch == inverted:
                regs[k] = (ch, st, max(0, st - int(rng.integers(1, 60))))
    order = rng.permutation(len(regs))
    return [regs[i] for i in order]


def _check_result_set(rs):
    assert rs.header is None
    assert all(rs.strands[i] == "*" for i in range(len(rs)))
    assert all(r.rest is None for r in rs.regions)


CASES = [(seed, inv) for seed in range(3) for inv in (None, "chr10", "all")]


def _check_every_operation(a, b):
    A, B = _rs(a), _rs(b)
    for got, want in ((A.reduce(), R.reduce(a)), (A.union(B), R.union(a, b)), (A.setdiff(B), R.setdiff(a, b)),
                      (B.setdiff(A), R.setdiff(b, a)), (A.intersect_all(B), R.intersect(a, b)),
                      (B.intersect_all(A), R.intersect(b, a))):
        _check_result_set(got)
        assert _tuples(got) == want
    assert A.jaccard(B) == R.jaccard(a, b)
    assert B.jaccard(A) == R.jaccard(b, a)
    assert A.coverage(B) == R.coverage(a, b)
    assert B.coverage(A) == R.coverage(b, a)
    assert A.overlap_coefficient(B) == R.overlap_coefficient(a, b)
    assert A.closest(B) == R.closest(a, b)
    assert B.closest(A) == R.closest(b, a)
    for gap in (0, 100, TOP):
        assert A.cluster(gap) == R.cluster(a, gap)
    assert A.get_nucleotide_length() == R.nucleotides_length(a)
    # union == reduce(concat)
    from gtars.models import RegionSetList

    assert _tuples(A.union(B)) == _tuples(RegionSetList([A, B]).concat().reduce())
    return A, B


@pytest.mark.parametrize("seed,inverted", CASES)
def test_every_operation_against_the_restatement(seed, inverted):
    rng = np.random.default_rng(1000 + seed)
    a = _random_set(rng, 3000, NAMES_A, inverted)
    b = _random_set(rng, 2000, NAMES_B, inverted)
    _check_every_operation(a, b)


# ---- sizes on the edges of a lane, a wave, a workgroup and a 2048-element tile of the sort and the scans ----------------
def _exactly(rng, n, names, inverted):
    """_random_set returns its n regions and their touching / duplicate / nested extras shuffled together: a random n of them"""
    regs = _random_set(rng, n, names, inverted)
    assert len(regs) >= n
    return regs[:n]


@pytest.mark.parametrize("n,boundary", E.edge_cases())
def test_every_operation_at_tile_edge_sizes(n, boundary):
    from gtars.models import RegionSetList

    rng = np.random.default_rng(3000 + n)
    a = _exactly(rng, n, ["chr10"], "all")
    b = _exactly(rng, n, ["chr10"], None)
    if boundary is not None:
        a, b = E.split_at(a, boundary), E.split_at(b, boundary)
        srt = sorted(a, key=lambda r: (r[0].encode(), r[1]))
        assert srt[boundary - 1][0] == "chr10" and srt[boundary][0] == "chr2"
    assert len(a) == n and len(b) == n
    A, B = _check_every_operation(a, b)
    assert RegionSetList([A, B, A]).pairwise_jaccard() == R.pairwise_jaccard([a, b, a])


def test_reduce_start_only_key_and_bytewise_names():
    regs = [("chr2", 10, 5), ("chr10", 3, 4), ("chr2", 10, 20), ("chr10", 0, 1)]
    assert _tuples(_rs(regs).reduce()) == R.reduce(regs) == [("chr10", 0, 1), ("chr10", 3, 4), ("chr2", 10, 5), ("chr2", 10, 20)]


def test_totals_wrap_modulo_2_32():
    a = [("c", 0, TOP), ("d", 0, 5)]
    b = [("c", 0, TOP), ("d", 3, 9)]
    A, B = _rs(a), _rs(b)
    assert A.jaccard(B) == R.jaccard(a, b)
    assert A.overlap_coefficient(B) == R.overlap_coefficient(a, b)
    assert A.coverage(B) == R.coverage(a, b)
    assert A.get_nucleotide_length() == 4


def test_closest_pins_the_first_of_equal_starts():
    other = [("c", 300, 310), ("c", 100, 105), ("c", 100, 200), ("c", 0, 5)]
    q = [("c", 100, 110), ("c", 150, 160), ("c", 400, 401)]
    got = _rs(q).closest(_rs(other))
    assert got == R.closest(q, other) == [(0, 1, 0), (1, 2, 0), (2, 0, 90)]


def test_empty_sets():
    from gtars.models import RegionSetList

    E, X = _rs([]), _rs([("chr1", 0, 10), ("chr2", 5, 6)])
    assert _tuples(E.reduce()) == []
    assert _tuples(E.union(X)) == [("chr1", 0, 10), ("chr2", 5, 6)]
    assert _tuples(E.setdiff(X)) == [] and _tuples(X.setdiff(E)) == _tuples(X.reduce())
    assert _tuples(X.intersect_all(E)) == []
    assert E.jaccard(E) == 0.0 and X.jaccard(E) == 0.0 and E.coverage(X) == 0.0 and X.overlap_coefficient(E) == 0.0
    assert X.closest(E) == [] and E.closest(X) == []
    assert E.cluster(5) == []
    assert RegionSetList([E, X, E]).pairwise_jaccard() == [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    assert RegionSetList([]).pairwise_jaccard() == []


def _big_set(seed, n, n_chrom=25, span=50_000_000):
    rng = np.random.default_rng(seed)
    names = [f"chr{i + 1}" for i in range(n_chrom)]
    c = rng.integers(0, n_chrom, n)
    s = rng.integers(0, span, n)
    e = s + rng.integers(0, 2000, n)
    return [(names[c[i]], int(s[i]), int(e[i])) for i in range(n)]


def test_reduce_cluster_closest_at_one_million_regions():
    a = _big_set(11, 1_000_000)
    b = _big_set(12, 200_000)
    A, B = _rs(a), _rs(b)
    assert _tuples(A.reduce()) == R.reduce(a)
    assert A.cluster(0) == R.cluster(a, 0)
    assert A.cluster(500) == R.cluster(a, 500)
    assert A.closest(B) == R.closest(a, b)


def _lola_sets():
    from gtars.models import RegionSet

    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lola_multi_db")
    paths = sorted(os.path.join(root, c, "regions", f) for c in os.listdir(root) if os.path.isdir(os.path.join(root, c))
                   for f in os.listdir(os.path.join(root, c, "regions")))
    return [RegionSet(p) for p in paths]


def test_pairwise_jaccard_lola_fixture():
    from gtars.models import RegionSetList

    sets = _lola_sets()
    assert len(sets) >= 6
    M = RegionSetList(sets).pairwise_jaccard()
    regs = [_tuples(s) for s in sets]
    assert M == R.pairwise_jaccard(regs)
    for i in range(len(sets)):
        for j in range(len(sets)):
            if i != j:
                assert M[i][j] == sets[i].reduce().jaccard(sets[j].reduce())


def test_pairwise_jaccard_with_inverted_and_empty_sets():
    from gtars.models import RegionSetList

    rng = np.random.default_rng(77)
    regs = [_random_set(rng, 400, NAMES_A if k % 2 else NAMES_B, "all" if k in (1, 4) else None) for k in range(7)]
    regs.append([])
    sets = [_rs(r) for r in regs]
    M = RegionSetList(sets).pairwise_jaccard()
    assert M == R.pairwise_jaccard(regs)
    for i in (0, 1, 4):
        for j in range(len(sets)):
            if i != j:
                assert M[i][j] == sets[i].reduce().jaccard(sets[j].reduce())


def _np_reduced_bp(rank, start, end):
    """u32 total of reduce() over numpy columns of a set without inverted regions"""
    if len(start) == 0:
        return 0
    o = np.lexsort((start, rank))
    r, s, e = rank[o], start[o].astype(np.int64), end[o].astype(np.int64)
    key = r.astype(np.int64) * (1 << 33) + e
    cm = np.maximum.accumulate(key) - r.astype(np.int64) * (1 << 33)
    head = np.ones(len(s), dtype=bool)
    head[1:] = (r[1:] != r[:-1]) | (s[1:] > cm[:-1])
    idx = np.flatnonzero(head)
    run_end = np.maximum.reduceat(e, idx)
    return int((run_end - s[idx]).sum()) & TOP


def test_pairwise_jaccard_64_synthetic_sets():
    from gtars.models import RegionSet, RegionSetList

    n_sets, n = 64, 20_000
    cols = []
    for k in range(n_sets):
        rng = np.random.default_rng(500 + k)
        rank = rng.integers(0, 25, n).astype(np.uint32)
        start = rng.integers(0, 20_000_000, n).astype(np.uint32)
        end = (start + rng.integers(0, 3000, n)).astype(np.uint32)
        cols.append((rank, start, end))
    names = [f"chr{i + 1}" for i in range(25)]
    sets = [RegionSet.from_vectors([names[i] for i in r], s, e) for r, s, e in cols]
    M = RegionSetList(sets).pairwise_jaccard()
    # bytewise rank of each name so that the numpy reduce sorts as the library does
    order = {nm: i for i, nm in enumerate(sorted(names))}
    byte_rank = np.array([order[nm] for nm in names], dtype=np.uint32)
    tot = [_np_reduced_bp(byte_rank[r], s, e) for r, s, e in cols]
    for i in range(n_sets):
        assert M[i][i] == 1.0
        for j in range(n_sets):
            if i == j:
                continue
            r = np.concatenate([byte_rank[cols[i][0]], byte_rank[cols[j][0]]])
            u = _np_reduced_bp(r, np.concatenate([cols[i][1], cols[j][1]]), np.concatenate([cols[i][2], cols[j][2]]))
            want = 0.0 if u == 0 else ((tot[i] + tot[j] - u) & TOP) / u
            assert M[i][j] == want, (i, j)
    for i, j in ((0, 1), (5, 63), (40, 7)):
        assert M[i][j] == sets[i].reduce().jaccard(sets[j].reduce())


# ---- structured layouts whose carries cross two 1024-tile chunk seams ----------------------------------------------------
def _assert_cols(rs, names, want):
    """a result set against (chromosome index into names, start, end) columns"""
    index = {nm: i for i, nm in enumerate(names)}
    res_names = np.array([index[nm] for nm in rs.chrom_names], dtype=np.uint32)
    assert len(rs) == len(want[0])
    assert np.array_equal(res_names[rs.chrom_ids] if len(rs) else np.zeros(0, dtype=np.uint32), want[0])
    assert np.array_equal(rs.starts, want[1]) and np.array_equal(rs.ends, want[2])


def test_one_region_covering_two_chunk_seams_of_others():
    """no run opens after the first region: the max-scan carries one value through every tile and both chunk seams"""
    lay = E.covering(E.N_SEAMS, seed=21)
    A = E.layout_set(lay)
    _assert_cols(A.reduce(), lay.names, lay.reduce)
    assert np.array_equal(np.asarray(A.cluster(0), dtype=np.uint32), lay.cluster0)


def _check_disjoint_layout(lay, restatement):
    A = E.layout_set(lay)
    red = A.reduce()
    _assert_cols(red, lay.names, lay.reduce)
    assert np.array_equal(np.asarray(A.cluster(0), dtype=np.uint32), lay.cluster0)
    assert len(A.setdiff(A)) == 0
    _assert_cols(A.intersect_all(A), lay.names, lay.reduce)
    assert A.jaccard(A) == 1.0
    if restatement:
        regs = [(lay.names[c], s, e) for c, s, e in zip(lay.chrom.tolist(), lay.start.tolist(), lay.end.tolist())]
        assert _tuples(red) == R.reduce(regs)
        assert A.cluster(0) == R.cluster(regs, 0)


def test_disjoint_regions_over_two_chunk_seams():
    """every region opens a run: reduce is the sorted input and cluster(0) the rank in sorted order"""
    _check_disjoint_layout(E.disjoint(E.N_SEAMS, seed=22), restatement=False)


@pytest.mark.parametrize("shift", [0, 1])
def test_chromosome_heads_on_tile_firsts_and_lasts(shift):
    """a new chromosome at every 2048-th sorted region: the segment heads sit on the first (shift 0) or the last (shift 1)
    slot of the tiles.  The shift 1 layout also runs against the Python restatement in full."""
    _check_disjoint_layout(E.disjoint(E.N_SEAMS, seed=23 + shift, per_chrom=2048, shift=shift), restatement=shift == 1)


# ---- chromosome keys of three bytes in the sort ---------------------------------------------------------------------------
def test_seventy_thousand_chromosomes():
    a, b = E.wide_set(61, 70_000), E.wide_set(62, 70_000)
    assert len({r[0] for r in a}) == 70_000 > 65_536
    A, B = _rs(a), _rs(b)
    assert _tuples(A.reduce()) == R.reduce(a)
    for gap in (0, 100):
        assert A.cluster(gap) == R.cluster(a, gap)
    assert A.closest(B) == R.closest(a, b)
    assert _tuples(A.union(B)) == R.union(a, b)


def test_pairwise_jaccard_with_more_than_65536_set_chromosome_segments():
    from gtars.models import RegionSetList

    regs = [E.wide_set(70 + k, 2000) for k in range(40)]
    assert 40 * len({r[0] for s in regs for r in s}) > 65_536
    assert RegionSetList([_rs(r) for r in regs]).pairwise_jaccard() == R.pairwise_jaccard(regs)
