"""The folds over a RegionSetList on the MI355X (csrc/setops.hip: union_all / intersect_all / union_except /
bulk_union_except) against the plain-Python restatement tests/setlist_ref.py, exact equality of the (chr, start, end) lists
throughout.  Sizes are total rows of the concatenation; the sorted-row tile of the kernels is 2,048."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_layouts as E  # noqa: E402
import setlist_ref as L  # noqa: E402
import setops_ref as R  # noqa: E402
from test_gpu_setops import NAMES_A, NAMES_B, _random_set  # noqa: E402

pytestmark = pytest.mark.gpu

TOP = 0xFFFFFFFF
TILE = 2048


def _rs(regs):
    from gtars.models import RegionSet

    return RegionSet.from_vectors([r[0] for r in regs], [r[1] for r in regs], [r[2] for r in regs])


def _tuples(rs):
    names, ids, s, e = rs.chrom_names, rs.chrom_ids, rs.starts, rs.ends
    return list(zip([names[i] for i in ids.tolist()], s.tolist(), e.tolist()))


def _rsl(sets):
    from gtars.models import RegionSetList

    return RegionSetList([_rs(s) for s in sets])


def _plain(rs):
    assert rs.header is None and all(x == "*" for x in rs.strands)
    assert all(r.rest is None for r in rs.regions[:50])
    return _tuples(rs)


def _check_all_four(sets, want=None, every_skip=True):
    """union_all, intersect_all, bulk_union_except and union_except(i) of the list against the restatement"""
    rsl = _rsl(sets)
    n = len(sets)
    full, ex = want if want is not None else L.bulk_union_except(sets)
    got_full, got_ex = rsl.bulk_union_except()
    assert _plain(got_full) == full
    assert len(got_ex) == n
    for i in range(n):
        assert _tuples(got_ex[i]) == ex[i], i
    assert _tuples(rsl.union_all()) == L.union_all(sets) == full
    assert _plain(rsl.intersect_all()) == L.intersect_all(sets)
    for i in (range(n) if every_skip else (0, n // 2, n - 1)):
        assert _tuples(rsl.union_except(i)) == ex[i], i
    assert rsl.union_except(n) is None
    return rsl


# ---- random lists ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverted", [None, "all"], ids=["plain", "inverted"])
@pytest.mark.parametrize("seed", range(3))
@pytest.mark.parametrize("n_sets", [2, 3, 5, 17])
def test_random_lists_against_the_restatement(n_sets, seed, inverted):
    rng = np.random.default_rng(7000 + 10 * n_sets + seed)
    sets = []
    for k in range(n_sets):
        names = (NAMES_A, NAMES_B, ["chrOnly%d" % k, "chr10"])[k % 3]  # some chromosomes in one set only
        sets.append(_random_set(rng, int(rng.integers(100, 400)), names, inverted))
    _check_all_four(sets)


# ---- tile edges --------------------------------------------------------------------------------------------------------
def _seam_list(n):
    """n rows on one chromosome whose sorted order is their index k (start 10 k).  Sets 0 and 1 alternate and each row
    reaches past the next two, so every union has runs of ~100 rows (rows 98 and 99 of each hundred are short: a gap
    follows).  Set 2 owns the rows on the last slot of a tile (2047, 4095) and on the first slot of the next (2048, 4096);
    the row before them reaches over both, so the run of "without set 2" that holds rows 2000 .. 2097 spans the seam."""
    own2 = {k for k in (5, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE) if k < n}
    sets = [[], [], []]
    for k in range(n):
        if k in own2:
            sets[2].append(("c", 10 * k, 10 * k + 25))
        elif k % 100 >= 98:
            sets[k % 2].append(("c", 10 * k, 10 * k + 4))
        else:
            sets[k % 2].append(("c", 10 * k, 10 * k + (45 if k + 1 in own2 else 25)))
    rng = np.random.default_rng(n)
    return [[s[i] for i in rng.permutation(len(s))] for s in sets]


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097])
def test_tile_edges_with_a_run_across_the_seam(n):
    sets = _seam_list(n)
    assert sum(len(s) for s in sets) == n
    full, ex = L.bulk_union_except(sets)
    if n > TILE:  # one run of "without set 2" holds the rows on both sides of the seam, set 2's own rows between them
        assert any(s < 10 * (TILE - 2) and e > 10 * (TILE + 1) for _, s, e in ex[2])
    _check_all_four(sets, (full, ex))


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097])
@pytest.mark.parametrize("shift", [0, 1])
def test_tile_edges_disjoint_layout_with_chromosome_heads_on_the_seam(n, shift):
    """edge_layouts.disjoint: nothing merges, chromosomes change on the first (shift 0) or the last (shift 1) slot of a
    tile; rows dealt to three sets in input order, so every result is the layout's own sorted rows without that set"""
    lay = E.disjoint(n, 100 + n + shift, per_chrom=TILE, shift=shift)
    rows = [(lay.names[c], s, e) for c, s, e in zip(lay.chrom.tolist(), lay.start.tolist(), lay.end.tolist())]
    sets = [rows[k::3] for k in range(3)]
    key = lambda r: (r[0], r[1])  # noqa: E731  (zero-padded names: bytewise order is index order)
    want = (sorted(rows, key=key), [sorted([r for j in range(3) if j != k for r in sets[j]], key=key) for k in range(3)])
    assert want[0] == list(zip([lay.names[c] for c in lay.reduce[0].tolist()], lay.reduce[1].tolist(), lay.reduce[2].tolist()))
    rsl = _check_all_four(sets, want)
    assert _tuples(rsl.intersect_all()) == []


def test_top2_carries_cross_the_second_round_of_the_tile_aggregates():
    """edge_layouts.long_covers at m = 2^20 + 1100: more than 1024 tiles, so the one workgroup that turns the tile
    aggregates into carries (k_t2_carry) takes a second round.  m1 / s1 (set 0's end) and m2 (set 1's long end) come from the
    first two sorted rows and must reach every tile, across the seam between the rounds, with no head between; the chr2
    head behind them must reset both.  Against the closed forms (tests/test_setlist_cpu.py holds them to the restatement)."""
    from gtars.models import RegionSet, RegionSetList

    lay = E.long_covers((1 << 20) + 1100)
    assert sum(len(c) for c, _, _ in lay.cols) // TILE + 1 > 1024
    rsl = RegionSetList([RegionSet.from_vectors([lay.names[i] for i in c.tolist()], s, e) for c, s, e in lay.cols])
    full, ex = rsl.bulk_union_except()
    assert _plain(full) == lay.full
    assert [_tuples(x) for x in ex] == lay.ex
    assert _tuples(rsl.union_all()) == lay.full
    for i in range(3):
        assert _tuples(rsl.union_except(i)) == lay.ex[i], i


# ---- owner logic of the scan -------------------------------------------------------------------------------------------
def test_one_set_covers_the_chromosome():
    """s1 is the covering set everywhere: only m2 decides the runs without it"""
    peaks = [("c", 100 * k, 100 * k + 30) for k in range(1, 60)]
    sets = [[("c", 0, 10_000)], peaks[0::2], peaks[1::2], [("d", 5, 6)]]
    full, ex = L.bulk_union_except(sets)
    assert full == [("c", 0, 10_000), ("d", 5, 6)] and ex[0] == peaks + [("d", 5, 6)]
    _check_all_four(sets, (full, ex))


def test_two_sets_tie_on_the_maximal_end():
    sets = [[("c", 0, 500), ("c", 600, 700)], [("c", 10, 500), ("c", 650, 700)], [("c", 400, 450), ("c", 499, 500), ("c", 500, 640)],
            [("c", 700, 700), ("c", 20, 500)]]
    _check_all_four(sets)


def test_removing_the_sole_cover_splits_a_run():
    sets = [[("c", 0, 100), ("c", 1000, 1100)], [("c", 90, 310)], [("c", 300, 400), ("c", 1100, 1200)]]
    full, ex = L.bulk_union_except(sets)
    assert full == [("c", 0, 400), ("c", 1000, 1200)]
    assert ex[1] == [("c", 0, 100), ("c", 300, 400), ("c", 1000, 1200)]
    _check_all_four(sets, (full, ex))


def test_ends_at_the_top_of_u32_and_starts_at_zero():
    sets = [[("c", 0, TOP), ("d", 0, 0)], [("c", 0, 5), ("c", TOP, TOP), ("d", 0, TOP)], [("c", TOP - 1, TOP), ("d", 0, 1), ("e", 0, TOP)],
            [("c", 7, 3), ("e", TOP, 0)]]
    _check_all_four(sets)
    _check_all_four([s[::-1] for s in sets[::-1]])


# ---- many sets ---------------------------------------------------------------------------------------------------------
def _merge_sorted(rows, skip):
    """setops_ref.reduce's merge over rows (chr, start, end, set) already in its sorted order, without set `skip`"""
    out, cur = [], None
    for c, s, e, k in rows:
        if k == skip:
            continue
        if cur is not None and cur[0] == c and s <= cur[2]:
            if e > cur[2]:
                cur[2] = e
        else:
            if cur is not None:
                out.append(tuple(cur))
            cur = [c, s, e]
    if cur is not None:
        out.append(tuple(cur))
    return out


@pytest.mark.parametrize("n_sets", [65, 257])
def test_many_sets_cross_the_wave_and_the_workgroup(n_sets):
    rng = np.random.default_rng(n_sets)
    sets = []
    for k in range(n_sets):
        if k in (0, 7, 64, n_sets - 1):
            sets.append([])  # empty sets in the list, the first and the last among them
            continue
        s = rng.integers(0, 30_000, 40)
        e = s + rng.integers(0, 40, 40)
        e[rng.random(40) < 0.05] -= 30  # a few inverted (clamped below)
        sets.append([(str(rng.choice(["chr1", "chr2", "chr10"])), int(a), int(max(b, 0))) for a, b in zip(s, e)])
    # the closed form of the restatement (tests/test_setlist_cpu.py holds it to the fold), from one stable sort of the
    # rows: the fold's 3 n unions of the growing prefix are too slow here for 257 sets
    rows = sorted(((c, a, b, k) for k, s in enumerate(sets) for c, a, b in s), key=lambda r: (r[0].encode(), r[1]))
    want = (_merge_sorted(rows, None), [_merge_sorted(rows, i) for i in range(n_sets)])
    assert want[0] == R.reduce([r for s in sets for r in s]) and want[1][1] == L.union_except_closed(sets, 1)
    if n_sets == 65:
        assert want == L.bulk_union_except(sets)
    rsl = _rsl(sets)
    got_full, got_ex = rsl.bulk_union_except()
    assert _tuples(got_full) == want[0]
    for i in range(n_sets):
        assert _tuples(got_ex[i]) == want[1][i], i
    for i in sorted({0, 1, 63, 64, 65, n_sets - 2, n_sets - 1}):
        if i < n_sets:
            assert _tuples(rsl.union_except(i)) == want[1][i], i
        else:
            assert rsl.union_except(i) is None  # skip == n (65 of 65 sets) is out of range
    assert _tuples(rsl.union_all()) == want[0]
    assert _tuples(rsl.intersect_all()) == []  # an empty set in the list
    dense = [s for s in sets if s][:20]
    assert _tuples(_rsl(dense).intersect_all()) == L.intersect_all(dense)


# ---- intersect_all -----------------------------------------------------------------------------------------------------
INTERSECT_CASES = {
    "adjacent": [[("c", 0, 10)], [("c", 10, 20)]],
    "merge_after_own_reduce": [[("c", 0, 10), ("c", 10, 20), ("c", 15, 40)], [("c", 5, 35)], [("c", 30, 32), ("c", 0, 31)]],
    "chromosome_missing_from_one": [[("c", 0, 10), ("d", 0, 10)], [("c", 5, 15), ("d", 5, 15)], [("d", 7, 30)]],
    "zero_length_inside_the_others": [[("c", 0, 100)], [("c", 50, 50)], [("c", 20, 80)]],
    "zero_length_next_to_cover": [[("c", 0, 100)], [("c", 50, 50), ("c", 60, 70)], [("c", 20, 80)]],
    "inverted_in_one_set": [[("c", 0, 50), ("c", 100, 30), ("c", 100, 200)], [("c", 10, 150)], [("c", 0, 400), ("c", 40, 20)]],
    "inverted_end_inside_an_earlier_region": [[("c", 0, 50), ("c", 60, 3)], [("c", 0, 100)], [("c", 1, 99)]],
}


@pytest.mark.parametrize("name", sorted(INTERSECT_CASES))
def test_intersect_all_cases(name):
    sets = INTERSECT_CASES[name]
    want = L.intersect_all(sets)
    if name in ("adjacent", "zero_length_inside_the_others"):
        assert want == []
    assert _plain(_rsl(sets).intersect_all()) == want
    assert _tuples(_rsl(sets[::-1]).intersect_all()) == L.intersect_all(sets[::-1])


@pytest.mark.parametrize("inverted", [None, "all"], ids=["plain", "inverted"])
def test_intersect_all_of_two_is_the_pairwise_intersect(inverted):
    rng = np.random.default_rng(99)
    a, b = _random_set(rng, 1500, NAMES_A, inverted), _random_set(rng, 1200, NAMES_B, inverted)
    A, B = _rs(a), _rs(b)
    from gtars.models import RegionSetList

    got = _tuples(RegionSetList([A, B]).intersect_all())
    assert got == _tuples(A.intersect_all(B)) == R.intersect(a, b)


# ---- pair wrappers -----------------------------------------------------------------------------------------------------
def test_pair_wrappers_equal_the_region_set_methods():
    rng = np.random.default_rng(5)
    sets = [_random_set(rng, 300, NAMES_A, "chr10"), _random_set(rng, 200, NAMES_B, None), _random_set(rng, 100, NAMES_A, None)]
    rsl = _rsl(sets)
    for i, j in ((0, 1), (1, 0), (2, 2), (0, 2)):
        a, b = rsl[i], rsl[j]
        assert _tuples(rsl.union_at(i, j)) == _tuples(a.union(b)) == L.union_at(sets, i, j)
        assert _tuples(rsl.setdiff_at(i, j)) == _tuples(a.setdiff(b)) == L.setdiff_at(sets, i, j)
        assert _tuples(rsl.pintersect_at(i, j)) == _tuples(a.pintersect(b)) == L.pintersect_at(sets, i, j)
        assert rsl.pintersect_count(i, j) == len(a.pintersect(b)) == L.pintersect_count(sets, i, j)
        assert rsl.jaccard_at(i, j) == a.jaccard(b) == L.jaccard_at(sets, i, j)
    assert rsl.union_at(0, 3) is None and rsl.jaccard_at(-1, 0) is None and rsl.region_count(2) == len(sets[2])


# ---- larger size -------------------------------------------------------------------------------------------------------
def _np_reduce_sorted(c, s, e):
    """reduce() of well-formed regions already sorted by (chromosome rank, start): a run opens where start > the running
    maximum of the ends so far (chromosomes kept apart by an offset)"""
    big = np.int64(1) << 33
    so, eo = s + c * big, e + c * big
    acc = np.maximum.accumulate(eo)
    head = so > np.concatenate([[-1], acc[:-1]])
    last = np.concatenate([head[1:], [True]])
    return c[head], s[head], acc[last] - c[last] * big


def test_64_sets_of_20k_regions():
    """union_all is the reduce of the concatenation, and every union_except(i) is exact against a numpy restatement of
    reduce over the other sets' rows (so no region of it misses all the other sets, and it covers all of them); for a
    few i the same is asked of the device's own any_overlaps"""
    from gtars.models import RegionSet, RegionSetList

    rng = np.random.default_rng(64)
    n_sets, per = 64, 20_000
    names = ["chr%d" % k for k in range(1, 9)]
    rank = np.empty(len(names), dtype=np.int64)
    rank[np.argsort(np.array([n.encode() for n in names]))] = np.arange(len(names))  # bytewise rank of each name
    cols = []
    for _ in range(n_sets):
        c = rng.integers(0, len(names), per)
        s = rng.integers(0, 40_000_000, per)
        cols.append((c, s, s + rng.integers(1, 600, per)))
    mk = lambda c, s, e: RegionSet.from_vectors([names[i] for i in c.tolist()], s, e)  # noqa: E731
    sets = [mk(*x) for x in cols]
    rsl = RegionSetList(sets)
    c, s, e = (np.concatenate([x[k] for x in cols]).astype(np.int64) for k in range(3))
    owner = np.repeat(np.arange(n_sets), per)
    o = np.lexsort((s, rank[c]))
    r_, s_, e_, owner = rank[c][o], s[o], e[o], owner[o]

    def same(got, want):
        gr = rank[np.array([names.index(n) for n in got.chrom_names])][got.chrom_ids]
        return np.array_equal(gr, want[0]) and np.array_equal(got.starts, want[1]) and np.array_equal(got.ends, want[2])

    full, ex = rsl.bulk_union_except()
    assert same(full, _np_reduce_sorted(r_, s_, e_))
    # RegionSetList.concat(), built from the same columns (concat() itself makes a Python object per region)
    concat = mk(c, s, e)
    assert _tuples(full) == _tuples(rsl.union_all()) == _tuples(concat.reduce())
    for i in range(n_sets):
        keep = owner != i
        assert same(ex[i], _np_reduce_sorted(r_[keep], s_[keep], e_[keep])), i
    for i in (0, 41):
        others = mk(c[np.repeat(np.arange(n_sets), per) != i], s[np.repeat(np.arange(n_sets), per) != i],
                    e[np.repeat(np.arange(n_sets), per) != i])
        assert all(ex[i].any_overlaps(others))  # no region misses all the other sets
        assert all(others.any_overlaps(ex[i]))  # and every row of theirs is covered
        assert _tuples(rsl.union_except(i)) == _tuples(ex[i])
    inter = rsl.intersect_all()
    assert len(inter) == 0 or all(inter.any_overlaps(sets[0]))
