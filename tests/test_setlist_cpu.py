"""The folds over a RegionSetList without a GPU: the plain-Python restatement (tests/setlist_ref.py) against the
reference's own literal cases and against brute force, the closed forms the device computes against the folds, and the
answers RegionSetList gives on the host (None, and the unreduced copies of one set) before any device call."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import setlist_ref as L  # noqa: E402
import setops_ref as R  # noqa: E402


# ---- the literal cases of gtars-genomicdist/src/region_set_list_ops.rs:303-560 (numbers retyped) -------------------------
def test_ref_union_all_literal_cases():
    assert L.union_all([[("chr1", 0, 100)], [("chr1", 50, 200)], [("chr1", 150, 300)]]) == [("chr1", 0, 300)]
    assert L.union_all([]) is None
    assert L.union_all([[("chr1", 10, 50)]]) == [("chr1", 10, 50)]


def test_ref_intersect_all_literal_cases():
    assert L.intersect_all([[("chr1", 0, 100)], [("chr1", 30, 200)], [("chr1", 60, 150)]]) == [("chr1", 60, 100)]
    assert L.intersect_all([[("chr1", 0, 50)], [("chr1", 100, 200)]]) == []  # disjoint
    assert L.intersect_all([]) is None
    # different sizes: shared coverage, not pairs by position
    assert L.intersect_all([[("chr1", 0, 100), ("chr1", 200, 300)], [("chr1", 50, 250)]]) == [
        ("chr1", 50, 100), ("chr1", 200, 250)]


def test_ref_union_except_literal_cases():
    sets = [[("chr1", 0, 100)], [("chr1", 200, 300)], [("chr1", 400, 500)]]
    assert L.union_except(sets, 1) == [("chr1", 0, 100), ("chr1", 400, 500)]
    assert L.union_except([[("chr1", 0, 100)]], 0) is None  # too small


def test_ref_bulk_union_except_literal_cases():
    a, b, c = [("chr1", 0, 100)], [("chr1", 200, 300)], [("chr1", 400, 500)]
    full, ex = L.bulk_union_except([a, b])  # n2
    assert len(full) == 2
    assert ex == [[("chr1", 200, 300)], [("chr1", 0, 100)]]
    full, ex = L.bulk_union_except([a, b, c])  # n3
    assert len(full) == 3 and len(ex) == 3
    assert ex[0] == [("chr1", 200, 300), ("chr1", 400, 500)]
    assert ex[1] == [("chr1", 0, 100), ("chr1", 400, 500)]
    assert ex[2] == [("chr1", 0, 100), ("chr1", 200, 300)]
    assert L.bulk_union_except([a]) is None and L.bulk_union_except([]) is None  # too small
    # matches union_except
    sets = [[("chr1", 0, 100), ("chr2", 50, 200)], [("chr1", 80, 180), ("chr2", 100, 300)], [("chr1", 150, 250)],
            [("chr2", 0, 150)]]
    _, ex = L.bulk_union_except(sets)
    for i in range(4):
        assert ex[i] == L.union_except(sets, i)


def test_ref_indexed_pair_literal_cases():
    a, b = [("chr1", 0, 100), ("chr1", 200, 300)], [("chr1", 50, 150), ("chr1", 250, 350)]
    assert L.pintersect_count([a, b], 0, 1) == 2
    assert L.pintersect_count([[("chr1", 0, 10)], [("chr1", 100, 200)]], 0, 1) == 1  # a zero-width region still counts
    assert L.pintersect_count([[("chr1", 0, 100)]], 0, 5) is None
    assert abs(L.jaccard_at([[("chr1", 0, 100)], [("chr1", 0, 100)]], 0, 1) - 1.0) < 1e-9
    assert abs(L.jaccard_at([[("chr1", 0, 100)], [("chr1", 200, 300)]], 0, 1)) < 1e-9
    pair = [[("chr1", 0, 100)], [("chr1", 50, 150)]]
    assert L.union_at(pair, 0, 1) == [("chr1", 0, 150)]
    assert L.setdiff_at(pair, 0, 1) == [("chr1", 0, 50)]
    sets = [[("chr1", 0, 100), ("chr1", 200, 300)], [("chr1", 50, 150)]]
    assert L.region_count(sets, 0) == 2 and L.region_count(sets, 1) == 1 and L.region_count(sets, 5) is None
    assert L.region_count(sets, -1) is None and L.union_at(pair, -1, 0) is None


def test_ref_folds_keep_the_quirks_of_the_accumulator():
    """one set, and the other set of two, come back unmerged and in their order; three or more are reduced"""
    messy = [("c", 50, 60), ("c", 0, 10), ("c", 5, 20)]
    assert L.union_all([messy]) == messy and L.intersect_all([messy]) == messy
    assert L.union_except([messy, [("c", 1, 2)]], 1) == messy
    full, ex = L.bulk_union_except([messy, [("c", 1, 2)]])
    assert full == [("c", 0, 20), ("c", 50, 60)] and ex == [[("c", 1, 2)], messy]
    assert L.union_except([messy, [("c", 1, 2)], []], 1) == [("c", 0, 20), ("c", 50, 60)]
    assert L.union_except([messy, []], 2) is None and L.union_except([messy, []], -1) is None


# ---- the restatement and the device's closed forms at larger size ----------------------------------------------------
def _random_list(rng, lo=2, hi=6, span=2000):
    """2..6 sets of 0..12 regions on one 2,000-bp chromosome (a second one now and then), with zero-length and inverted
    regions"""
    sets = []
    for _ in range(int(rng.integers(lo, hi + 1))):
        regs = []
        for _ in range(int(rng.integers(0, 13))):
            s = int(rng.integers(0, span))
            kind = rng.random()
            if kind < 0.1:
                e = s  # zero length
            elif kind < 0.2:
                e = int(rng.integers(0, s + 1))  # inverted (or zero length)
            else:
                e = min(span, s + int(rng.integers(1, 300)))
            regs.append(("chrA" if rng.random() < 0.85 else "chr9", s, e))
        sets.append(regs)
    return sets


def _covered(regs, chrom, span):
    """the numpy coverage array of reduce(regs): base p is covered when a reduced region has start <= p < end"""
    cov = np.zeros(span + 1, dtype=bool)
    for c, s, e in regs:
        if c == chrom and s < e:
            cov[s:e] = True
    return cov


def test_ref_bulk_union_except_against_brute_force():
    rng = np.random.default_rng(20240)
    span = 2000
    for _ in range(200):
        sets = _random_list(rng, span=span)
        full, ex = L.bulk_union_except(sets)
        n = len(sets)
        if n >= 3:
            assert full == R.reduce([r for s in sets for r in s])
        for i in range(n):
            assert ex[i] == L.union_except(sets, i)
            others = [r for k, s in enumerate(sets) if k != i for r in s]
            if n >= 3:
                assert ex[i] == L.union_except_closed(sets, i)
            # coverage: the bases of the result are the bases of the other sets' rows (a reduce never loses or adds one)
            for chrom in ("chrA", "chr9"):
                assert np.array_equal(_covered(ex[i], chrom, span), _covered(others, chrom, span))
            # and no two results of a reduce touch or overlap, unless an inverted row kept them apart
            if n >= 3 and all(s <= e for _, s, e in others):
                for (c0, _, e0), (c1, s1, _) in zip(ex[i], ex[i][1:]):
                    assert c0 != c1 or s1 > e0


def test_ref_intersect_all_against_brute_force_and_the_depth_sweep():
    """the fold equals the stretches that every set's reduce covers with positive length -- inverted regions included,
    which is why the device needs no sequential path for them"""
    rng = np.random.default_rng(777)
    span = 2000
    for _ in range(200):
        sets = _random_list(rng, span=span)
        got = L.intersect_all(sets)
        assert got == L.intersect_all_closed(sets)
        for chrom in ("chrA", "chr9"):
            cov = np.ones(span + 1, dtype=bool)
            for s in sets:
                cov &= _covered(R.reduce(s), chrom, span)
            assert np.array_equal(_covered(got, chrom, span), cov)
        for (c0, _, e0), (c1, s1, _) in zip(got, got[1:]):
            assert c0 != c1 or s1 > e0  # pieces never touch


# ---- what RegionSetList answers on the host ------------------------------------------------------------------------
def _rs(regs, rest=None):
    from gtars.models import Region, RegionSet

    if rest is None:
        return RegionSet.from_vectors([r[0] for r in regs], [r[1] for r in regs], [r[2] for r in regs])
    return RegionSet.from_regions([Region(c, s, e, x) for (c, s, e), x in zip(regs, rest)])


def _rows(rs):
    return [(r.chr, r.start, r.end, r.rest) for r in rs.regions]


MESSY = [("chr2", 50, 60), ("chr10", 0, 10), ("chr2", 5, 20), ("chr2", 7, 3)]
REST = ["a\t1", None, "b", "c"]


def test_empty_list_answers_none():
    from gtars.models import RegionSetList

    rsl = RegionSetList([])
    assert rsl.union_all() is None and rsl.intersect_all() is None
    assert rsl.union_except(0) is None and rsl.bulk_union_except() is None
    assert rsl.region_count(0) is None and rsl.union_at(0, 0) is None


def test_one_set_comes_back_as_it_is():
    from gtars.models import RegionSetList

    a = _rs(MESSY, REST)
    rsl = RegionSetList([a])
    want = [(c, s, e, x) for (c, s, e), x in zip(MESSY, REST)]
    for got in (rsl.union_all(), rsl.intersect_all()):
        assert got is not a and _rows(got) == want  # rows in their order, unmerged, rest kept
    assert rsl.union_except(0) is None and rsl.bulk_union_except() is None
    assert rsl.region_count(0) == 4 and rsl.region_count(1) is None


def test_two_sets_union_except_is_the_other_set_unmerged():
    from gtars.models import RegionSetList

    a, b = _rs(MESSY, REST), _rs([("chr2", 1, 2)])
    rsl = RegionSetList([a, b])
    want = [(c, s, e, x) for (c, s, e), x in zip(MESSY, REST)]
    assert _rows(rsl.union_except(1)) == want
    assert _rows(rsl.union_except(0)) == [("chr2", 1, 2, None)]
    assert rsl.union_except(2) is None  # skip == n
    assert rsl.union_except(-1) is None


def test_two_sets_bulk_union_except_on_the_host_side():
    """the excepts of two sets are copies; the full union is a device reduce"""
    import gtars_amd
    from gtars.models import RegionSetList

    a, b = _rs(MESSY, REST), _rs([("chr2", 1, 2)])
    rsl = RegionSetList([a, b])
    if gtars_amd.device_count() == 0:
        with pytest.raises(gtars_amd.NoDeviceError):
            rsl.bulk_union_except()
        return
    full, ex = rsl.bulk_union_except()
    assert [r[:3] for r in _rows(full)] == R.reduce(MESSY + [("chr2", 1, 2)])
    assert _rows(ex[0]) == [("chr2", 1, 2, None)]
    assert _rows(ex[1]) == [(c, s, e, x) for (c, s, e), x in zip(MESSY, REST)]


def test_pair_indices_out_of_range_answer_none():
    from gtars.models import RegionSetList

    a, b = _rs(MESSY), _rs([("chr2", 1, 2)])
    rsl = RegionSetList([a, b])
    for call in (rsl.pintersect_at, rsl.pintersect_count, rsl.jaccard_at, rsl.union_at, rsl.setdiff_at):
        for i, j in ((0, 2), (2, 0), (-1, 0), (0, -1), (5, 5)):
            assert call(i, j) is None
    assert rsl.region_count(-1) is None and rsl.region_count(2) is None
    assert rsl.region_count(0) == 4 and rsl.region_count(1) == 1
    # pintersect is host arithmetic: the indexed call gives what the method gives
    assert _rows(rsl.pintersect_at(0, 1)) == _rows(a.pintersect(b))
    assert rsl.pintersect_count(0, 1) == 1


FOLDS = [("union_all", lambda r: r.union_all()), ("intersect_all", lambda r: r.intersect_all()),
         ("union_except", lambda r: r.union_except(1)), ("bulk_union_except", lambda r: r.bulk_union_except())]


@pytest.mark.parametrize("name,call", FOLDS, ids=[n for n, _ in FOLDS])
def test_folds_of_three_sets_have_no_cpu_fallback(name, call):
    import gtars_amd
    from gtars.models import RegionSetList

    rsl = RegionSetList([_rs(MESSY), _rs([("chr2", 1, 2)]), _rs([("chr10", 3, 9)])])
    if gtars_amd.device_count() > 0:
        call(rsl)  # (tests/test_gpu_setlist.py checks the values)
        return
    with pytest.raises(gtars_amd.NoDeviceError):
        call(rsl)


def test_top2_scan_model_against_the_folds():
    """the row-by-row model of the device's scan (setlist_ref.bulk_union_except_top2) gives the folds' answers, and its
    operator is associative up to the choice of s1 among the sets that tie on the maximum"""
    rng = np.random.default_rng(4242)
    for _ in range(200):
        sets = _random_list(rng, lo=3)
        full, ex = L.bulk_union_except(sets)
        assert L.bulk_union_except_top2(sets) == (full, ex)
    for _ in range(300):
        rows = [(int(rng.integers(0, 6)), int(rng.integers(0, 4)), None) for _ in range(int(rng.integers(1, 12)))]
        cut = int(rng.integers(0, len(rows) + 1))
        fold = lambda xs: __import__("functools").reduce(L.t2_merge, xs, None)  # noqa: E731
        left, split = fold(rows), L.t2_merge(fold(rows[:cut]), fold(rows[cut:]))
        for i in range(5):  # the running maximum without set i is what the kernels read
            pick = lambda st: None if st is None else (st[2] if st[1] == i else st[0])  # noqa: E731
            want = max((e for e, s, _ in rows if s != i), default=None)
            assert pick(left) == want and pick(split) == want


def test_long_covers_layout_closed_forms_against_the_restatement():
    """edge_layouts.long_covers, which tests/test_gpu_setlist.py runs at 2^20 + 1100 regions per set against its closed
    forms alone: at m = 1100 the closed forms are the fold's and the top-2 model's answers"""
    import edge_layouts as E

    lay = E.long_covers(1100)
    sets = [[(lay.names[c], s, e) for c, s, e in zip(*(x.tolist() for x in col))] for col in lay.cols]
    assert [len(s) for s in sets] == [1, 1101, 1400]
    assert L.bulk_union_except(sets) == (lay.full, lay.ex)
    assert L.bulk_union_except_top2(sets) == (lay.full, lay.ex)
    assert L.union_all(sets) == lay.full
    top = lay.full[0][2]
    assert top > max(e for s in sets[1:] for _, _, e in s if e != top - 1) and len(lay.full) == 301


def test_c_abi_answers_short_lists_on_the_host():
    """the four entry points themselves: NULL handle for "None", unreduced copies for one set (the other of two), and
    GTARS_ERR_INVALID_ARG for NULL arguments -- none of it needs a device"""
    import ctypes as C

    from gtars.models import RegionSet
    from gtars_amd._lib import lib

    a, b = _rs(MESSY, REST), _rs([("chr2", 1, 2)])
    want = [(c, s, e, x) for (c, s, e), x in zip(MESSY, REST)]
    arr = lambda *sets: C.cast((C.c_void_p * max(len(sets), 1))(*[s._h for s in sets]), C.c_void_p)  # noqa: E731
    for fn in (lib.gtars_regionset_list_union_all, lib.gtars_regionset_list_intersect_all):
        h = C.c_void_p(1)
        assert fn(arr(), 0, C.byref(h)) == 0 and not h.value
        assert fn(arr(a), 1, C.byref(h)) == 0 and h.value
        assert _rows(RegionSet._from_handle(h)) == want
        assert fn(arr(a), 1, None) != 0 and fn(None, 1, C.byref(h)) != 0
    h = C.c_void_p(1)
    for n, skip in ((0, 0), (1, 0), (2, 2), (2, 7)):
        assert lib.gtars_regionset_list_union_except(arr(a, b), n, skip, C.byref(h)) == 0 and not h.value
    assert lib.gtars_regionset_list_union_except(arr(a, b), 2, 1, C.byref(h)) == 0
    assert _rows(RegionSet._from_handle(h)) == want
    h = C.c_void_p()
    assert lib.gtars_regionset_list_union_except(arr(a, b), 2, 0, C.byref(h)) == 0
    assert _rows(RegionSet._from_handle(h)) == [("chr2", 1, 2, None)]
    assert lib.gtars_regionset_list_union_except(arr(a, b), 2, 0, None) != 0
    u, ex = C.c_void_p(1), C.c_void_p(1)
    for n in (0, 1):
        assert lib.gtars_regionset_list_bulk_union_except(arr(a), n, C.byref(u), C.byref(ex)) == 0
        assert not u.value and not ex.value
    assert lib.gtars_regionset_list_bulk_union_except(arr(a, b), 2, None, C.byref(ex)) != 0
    assert lib.gtars_regionset_list_bulk_union_except(arr(a, b), 2, C.byref(u), None) != 0
