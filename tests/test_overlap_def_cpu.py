"""The overlap oracle against the definitions of tests/overlap_def.py.

Every GPU parity test of the overlap family compares the HIP path with ``oracle.Index`` (oracle/gtars_oracle.c), and that
restatement was pinned only by the reference's literal cases of at most 26 intervals.  Here (a) the numpy model answers those
literals itself, with no oracle involved, and (b) the oracle is held to the model on generated cases with duplicates, ties,
zero-length and inverted intervals and queries, unknown chromosomes, deep AIList nesting and coordinates at the top of u32.
tests/test_gpu_overlap_def.py holds the device to the same model on the same cases.
"""
import numpy as np
import pytest

import oracle
import overlap_def as od
from overlap_def import KIND_AILIST, KIND_BITS
from overlap_def_cases import BOTH, CASES, NESTED, case, check_layout, check_queries, model_of

# ------------------------------------------------------------- (a) the model against the reference's literals

AILIST_26 = [
    (0, 30), (0, 10), (0, 10), (5, 15), (5, 15), (10, 20), (10, 20), (15, 25), (15, 25), (21, 22), (22, 23),
    (20, 30), (20, 30), (25, 100), (26, 27), (27, 28), (29, 30), (30, 31), (32, 33), (50, 51), (51, 52),
    (52, 53), (53, 54), (55, 56), (60, 61), (70, 71),
]


def _model(regions, kind, vals=None):
    c, s, e = zip(*regions) if regions else ((), (), ())
    return od.Model(c, s, e, vals, n_chrom=(max(c) + 1 if c else 1), kind=kind)


def _rows(off, *cols):
    return [list(zip(*[x[int(off[i]):int(off[i + 1])].tolist() for x in cols])) for i in range(len(off) - 1)]


def test_model_ailist_26():
    # ailist.rs:550-601
    m = _model([(0, s, e) for s, e in AILIST_26], KIND_AILIST)
    assert m.headers(0) == [0, 24]
    s, e, _ = m.stored(0)
    assert list(zip(s[24:].tolist(), e[24:].tolist())) == [(0, 30), (25, 100)]  # the second sub-list
    off, fs, fe, _ = m.query([0, 0, 0], [6, 30, 101], [8, 35, 150]).find_overlaps()
    assert off.tolist() == [0, 5, 8, 8]
    assert _rows(off, fs, fe)[0] == [(5, 15), (5, 15), (0, 10), (0, 10), (0, 30)]


def test_model_bits_order_and_maxlen():
    # bits.rs:105 (stable sort by (start, end), interval.rs:18-31), bits.rs:110-119
    m = od.Model([0] * 5, [10, 10, 5, 10, 5], [30, 20, 50, 20, 50], [0, 1, 2, 3, 4], n_chrom=1, kind=KIND_BITS)
    off, ids = m.query([0], [0], [100]).tokenize()
    assert off.tolist() == [0, 5] and ids.tolist() == [2, 4, 1, 3, 0]
    assert m.stored(0)[2].tolist() == [2, 4, 1, 3, 0]
    assert m.max_len(0) == 45
    # bits.rs:194-206 restated as a build: result order (0, 5, 1) then (0, 20, 5)
    m = od.Model([0, 0, 0], [0, 6, 0], [5, 10, 20], [1, 2, 5], n_chrom=1, kind=KIND_BITS)
    off, s, e, v = m.query([0], [1], [3]).find_overlaps()
    assert _rows(off, s, e, v) == [[(0, 5, 1), (0, 20, 5)]]
    # max_len: an inverted interval counts as 0 (checked_sub(...).unwrap_or(0))
    assert od.Model([0, 0], [50, 7], [10, 9], n_chrom=1).max_len(0) == 2


@pytest.mark.parametrize("kind", BOTH)
def test_model_abcd(kind):
    # bits.rs:545-616 / ailist.rs:385-457, 489-519
    m = _model([(0, 1, 5), (0, 3, 7), (0, 6, 10), (0, 8, 12)], kind)
    assert m.chrom_len(0) == 4
    h = m.query([0, 0, 0, 0, 9], [2, 9, 13, 0, 2], [4, 11, 15, 1, 4])
    off, ids = h.tokenize()
    got = [sorted(ids[int(off[i]):int(off[i + 1])].tolist()) for i in range(5)]
    assert got == [[0, 1], [2, 3], [], [], []]
    assert h.count_overlaps().tolist() == [2, 2, 0, 0, 0]
    for qs, qe, want in [(2, 4, [0, 1]), (5, 8, [1, 2]), (9, 11, [2, 3]), (0, 15, [0, 1, 2, 3]), (7, 9, [2, 3])]:
        assert sorted(m.query([0], [qs], [qe]).tokenize()[1].tolist()) == want
    # empty index (bits.rs:607-616 / ailist.rs:447-457), single interval (ailist.rs:521-539)
    e0 = _model([], kind)
    assert e0.chrom_len(0) == 0 and e0.query([0], [1], [2]).count_overlaps().tolist() == [0]
    one = _model([(0, 5, 10)], kind)
    assert one.query([0, 0], [6, 11], [8, 15]).count_overlaps().tolist() == [1, 0]


@pytest.mark.parametrize("kind", BOTH)
def test_model_mco(kind):
    # multi_chrom_overlapper.rs:1070-1130, :878-943
    m = _model([(0, 150, 200), (0, 250, 350), (0, 500, 600)], kind)
    assert m.query([0], [100], [300]).count_overlaps().tolist() == [2]
    m = _model([(0, 150, 250)], kind)
    assert m.query([0, 0], [100, 300], [200, 400]).any_overlaps().tolist() == [True, False]
    m = _model([(0, 100, 110)], kind)
    h = m.query([0], [105], [200])
    assert h.count_overlaps(5).tolist() == [1]
    assert h.count_overlaps(6).tolist() == [0]
    assert h.any_overlaps(6).tolist() == [False]
    m = _model([(0, 100, 200)], kind)
    h = m.query([0, 99], [200, 100], [300, 200])  # half-open boundary, nonexistent chromosome
    assert h.count_overlaps().tolist() == [0, 0] and h.any_overlaps().tolist() == [False, False]
    # multi_chrom_overlapper.rs:1044-1066, indexed_region_set.rs:395-414: subset / intersect_all
    m = _model([(0, 100, 200), (0, 300, 400), (1, 500, 600)], kind)
    h = m.query([0, 1], [150, 550], [250, 650])
    assert [x.tolist() for x in h.subset_by_overlaps()] == [[0, 1], [100, 500], [200, 600]]
    assert h.subset_source_indices().tolist() == [0, 2]
    # indexed_region_set.rs:246-263: every source row sharing a hit's coordinates, sorted and de-duplicated
    m = _model([(0, 100, 200), (0, 100, 200), (0, 300, 400), (0, 100, 200)], kind)
    off, idx = m.query([0], [150], [160]).find_overlap_indices()
    assert off.tolist() == [0, 3] and idx.tolist() == [0, 1, 3]
    # the subset filter applies only when min_bp > 1 (multi_chrom_overlapper.rs:461-465)
    m = _model([(0, 100, 200), (0, 100, 200), (0, 150, 400)], kind)
    h = m.query([0], [190], [260])
    assert [x.tolist() for x in h.subset_by_overlaps(20)[1:]] == [[150], [400]]
    assert [x.tolist() for x in h.subset_by_overlaps(1)[1:]] == [[100, 150], [200, 400]]


def test_model_ailist_round_is_the_nested_loop():
    """the shifted-array round against the loop of ailist.rs:205-217, written out, on random ends with ties"""
    rng = np.random.default_rng(3)
    for m in (0, 1, 9, 10, 11, 19, 20, 21, 200):
        ends = rng.integers(0, 30, m).astype(np.int64)
        want = []
        for i in range(m):
            count = 0
            for k in range(1, 20):
                if i + k >= m:
                    break
                if ends[i] > ends[i + k]:
                    count += 1
            want.append(count >= 10)
        assert od.ailist_round(ends).tolist() == want


# ------------------------------------------------------------- (b) oracle.Index against the model


class MemoIndex(oracle.Index):
    """oracle.Index that remembers what irs_find_overlaps answered for the same arrays and min_overlap: irs_subset_by_overlaps
    asks it again for the batch that find_overlap_indices has just compared."""

    def irs_find_overlaps(self, *args):
        key = tuple(id(a) for a in args[:-1]) + (args[-1],)
        memo = self.__dict__.setdefault("_memo", {})
        if key not in memo:
            memo[key] = super().irs_find_overlaps(*args)
        return memo[key]


class OracleCalls:
    """oracle.Index under the names check_layout / check_queries use.  Its IndexedRegionSet calls answer in source rows."""

    def __init__(self, d, kind):
        self.o = MemoIndex(d["c"], d["s"], d["e"], d["val"], n_chrom=d["n_chrom"], kind=kind)
        self.q = (d["qc"], d["qs"], d["qe"])
        self.src = (d["c"], d["s"], d["e"])
        self.row_vals = np.arange(len(d["c"]))
        self.stored, self.max_len, self.headers = self.o.stored, self.o.max_len, self.o.headers

    def tokenize(self):
        return self.o.tokenize(*self.q)

    def count_overlaps(self, mo):
        return self.o.count_overlaps(*self.q, mo)

    def any_overlaps(self, mo):
        return self.o.any_overlaps(*self.q, mo)

    def find_overlaps(self, mo):
        return self.o.find_overlaps_regions(*self.q, mo)

    def find_overlap_indices(self, mo):
        return self.o.irs_find_overlaps(*self.src, *self.q, mo)

    def subset_by_overlaps(self, mo):
        return oracle.mco_subset_by_overlaps(self.o, *self.q, mo)

    def subset_source_indices(self, mo):
        return oracle.irs_subset_by_overlaps(self.o, *self.src, *self.q, mo)


@pytest.mark.parametrize("kind", BOTH)
@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_equals_the_definitions(name, kind):
    m, h = model_of(name, kind)
    impl = OracleCalls(case(name), kind)
    check_layout(impl, m)
    check_queries(impl, h)


# ------------------------------------------------------------- (c) the cases reach what they are for


def figures():
    """what the case list exercises, from the model alone"""
    f = dict(max_sublists=0, tie_neighbours=0, boundary_hits=0, touching_pairs=0, queries=0, no_hit=0, max_hits=0, hits=0)
    for name in CASES:
        d = case(name)
        ma, _ = model_of(name, KIND_AILIST)
        f["max_sublists"] = max([f["max_sublists"]] + [len(ma.headers(ch)) for ch in range(ma.n_chrom)])
        mb, h = model_of(name, KIND_BITS)
        for ch in range(mb.n_chrom):
            s, e, v = mb.stored(ch)
            f["tie_neighbours"] += int(((s[1:] == s[:-1]) & (e[1:] == e[:-1]) & (v[1:] != v[:-1])).sum())
        qs, qe, s, e = h.qs[h.q], h.qe[h.q], mb.f_start[h.pos], mb.f_end[h.pos]
        f["boundary_hits"] += int(((qs == s) | (qs == e) | (qe == s) | (qe == e)).sum())
        cnt = h.count_overlaps()
        f["queries"] += len(cnt)
        f["no_hit"] += int((cnt == 0).sum())
        f["max_hits"] = max(f["max_hits"], int(cnt.max()))
        f["hits"] += int(cnt.sum())
        # queries that touch an interval without overlapping it: qs == e_i or qe == s_i, where "<=" for "<" would add a hit
        for ch in range(mb.n_chrom):
            s, e, _ = mb.stored(ch)
            on = d["qc"] == ch
            f["touching_pairs"] += int(np.isin(d["qs"][on], e).sum() + np.isin(d["qe"][on], s).sum())
    return f


def test_cases_are_not_vacuous():
    f = figures()
    print("\noverlap_def cases:", f)
    assert f["max_sublists"] >= 4
    assert f["tie_neighbours"] >= 1000
    assert f["boundary_hits"] >= 100
    assert f["no_hit"] >= 0.02 * f["queries"] and f["max_hits"] >= 50
    assert f["touching_pairs"] >= 1000
    for name in NESTED:  # the two nested shapes are nested
        ma, _ = model_of(name, KIND_AILIST)
        assert max(len(ma.headers(ch)) for ch in range(ma.n_chrom)) >= 2, name
