"""Size edges of the engine's host-pointer entry points (OverlapIndex.* and IgdIndex.* on host arrays) against the CPU oracle,
bit-exact: empty and one-row universes, batches around the 256-byte (64-query) padding of the uploaded query columns, batches
without a single hit, and the host-side compaction of find_overlap_indices.  Everything here is tiny: what can go wrong at
these sizes is a copy of the wrong length, a column at the wrong offset or an output that is not there.
"""
import numpy as np
import pytest

import oracle
from oracle import KIND_AILIST, KIND_BITS

pytestmark = pytest.mark.gpu

BOTH = [KIND_BITS, KIND_AILIST]
NQS = (0, 1, 63, 64, 65)
MIN_OVERLAPS = (None, 2)  # has_min off / on

# (chrom, start, end) of the universes: n = 0, 1, 5 rows on 2 chromosomes
UNIVERSES = {
    0: ([], [], []),
    1: ([1], [120], [180]),
    5: ([0, 0, 1, 1, 0], [100, 150, 50, 300, 400], [200, 260, 120, 310, 480]),
}
# 6 records in 2 files on 2 chromosomes: (chrom, start, end, file, value)
IGD_DB = ([0, 0, 0, 1, 1, 1], [100, 150, 400, 50, 60, 300], [200, 260, 480, 120, 90, 310], [0, 0, 1, 1, 0, 1], [0, 1, 2, 3, 4, 5])


@pytest.fixture(scope="module")
def ga():
    import gtars_amd

    assert gtars_amd.device_count() > 0, "no MI355X visible: -m gpu tests must run on the GPU box"
    return gtars_amd


def _queries(nq, n_chrom=2, chrom=None):
    """nq queries over the span the universes cover: about half of them hit something, widths from 1 bp up; the first one
    (a batch of one is only this) hits every universe that has a row on chromosome 1"""
    rng = np.random.default_rng(1000 + nq)
    qc = rng.integers(0, n_chrom, nq).astype(np.uint32) if chrom is None else np.full(nq, chrom, dtype=np.uint32)
    qs = rng.integers(0, 520, nq).astype(np.uint32)
    qe = (qs + rng.integers(1, 150, nq)).astype(np.uint32)
    if nq and chrom is None:
        qc[0], qs[0], qe[0] = 1, 100, 190
    return qc, qs, qe


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert np.asarray(a).tolist() == np.asarray(b).tolist()


@pytest.mark.parametrize("n", sorted(UNIVERSES))
@pytest.mark.parametrize("kind", BOTH)
def test_index_entry_points_at_size_edges(ga, kind, n):
    c, s, e = UNIVERSES[n]
    g = ga.OverlapIndex(c, s, e, None, n_chrom=2, kind=kind)
    o = oracle.Index(c, s, e, None, n_chrom=2, kind=kind)
    for nq in NQS:
        qc, qs, qe = _queries(nq)
        if kind == KIND_BITS:
            want = [o.bits_count(int(a), int(b), int(d)) for a, b, d in zip(qc, qs, qe)]
            assert g.bits_count(qc, qs, qe).tolist() == want, nq
        for mo in MIN_OVERLAPS:
            assert g.count_overlaps(qc, qs, qe, mo).tolist() == o.count_overlaps(qc, qs, qe, mo).tolist(), (nq, mo)
            assert g.any_overlaps(qc, qs, qe, mo).tolist() == o.any_overlaps(qc, qs, qe, mo).tolist(), (nq, mo)
            _same(g.find_overlaps(qc, qs, qe, mo), o.find_overlaps_regions(qc, qs, qe, mo))  # offsets, starts, ends, values
            _same(g.find_overlap_indices(qc, qs, qe, mo), o.irs_find_overlaps(c, s, e, qc, qs, qe, mo))
            _same(g.subset_by_overlaps(qc, qs, qe, mo), oracle.mco_subset_by_overlaps(o, qc, qs, qe, mo))
            _same([g.subset_source_indices(qc, qs, qe, mo)], [oracle.irs_subset_by_overlaps(o, c, s, e, qc, qs, qe, mo)])


@pytest.mark.parametrize("kind", BOTH)
def test_index_batches_without_a_hit(ga, kind):
    """h = 0: every query sits on a chromosome the universe has no row on -> empty arrays, offsets all zero, nothing raises"""
    c, s, e = UNIVERSES[5]
    g = ga.OverlapIndex(c, s, e, None, n_chrom=3, kind=kind)
    o = oracle.Index(c, s, e, None, n_chrom=3, kind=kind)
    for nq in (1, 65):
        qc, qs, qe = _queries(nq, chrom=2)
        for mo in MIN_OVERLAPS:
            got = g.find_overlaps(qc, qs, qe, mo)
            _same(got, o.find_overlaps_regions(qc, qs, qe, mo))
            assert got[0].tolist() == [0] * (nq + 1) and [len(x) for x in got[1:]] == [0, 0, 0]
            off, idx = g.find_overlap_indices(qc, qs, qe, mo)
            _same((off, idx), o.irs_find_overlaps(c, s, e, qc, qs, qe, mo))
            assert off.tolist() == [0] * (nq + 1) and len(idx) == 0 and idx.dtype == np.uint32


def test_igd_batches_without_a_hit(ga):
    c, s, e, f, v = IGD_DB
    g = ga.IgdIndex(c, s, e, f, v, n_chrom=3, n_files=2)
    for nq in (1, 65):
        qc, qs, qe = _queries(nq, chrom=2)
        for mo in (1, 0):
            q, r = g.find_overlaps_regionset(qc, qs, qe, mo)
            assert len(q) == 0 and len(r) == 0 and q.dtype == np.uint32 and r.dtype == np.uint32


@pytest.mark.parametrize("kind", BOTH)
def test_find_overlap_indices_compacts_deduplicated_segments(ga, kind):
    """A universe with duplicated coordinates: rows 0-2 share one interval, row 3 is on its own.  The values name the SOURCE
    rows of a set that lists every interval once (0, 0, 0, 1), so the three hits of a query on the shared interval are one
    source row: the device's sort + unique shortens that segment (3 -> 1) and the host-side compaction moves the segments
    behind it (the offsets of the enumeration and of the result differ).  Query 1 keeps its segment whole, query 2 has one
    hit of each kind, query 3 has none.  With the default values (the rows themselves) nothing is shortened: that form is
    checked too."""
    c, s, e = [0, 0, 0, 0], [100, 100, 100, 300], [200, 200, 200, 400]
    src = ([0, 0], [100, 300], [200, 400])
    qc, qs, qe = [0, 0, 0, 0], [150, 350, 180, 220], [160, 360, 320, 290]
    for mo in MIN_OVERLAPS:
        g = ga.OverlapIndex(c, s, e, [0, 0, 0, 1], n_chrom=1, kind=kind)
        o = oracle.Index(c, s, e, [0, 0, 0, 1], n_chrom=1, kind=kind)
        hits = g.tokenize(qc, qs, qe)[0] if mo is None else None
        off, idx = g.find_overlap_indices(qc, qs, qe, mo)
        _same((off, idx), o.irs_find_overlaps(*src, qc, qs, qe, mo))
        assert off.tolist() == [0, 1, 2, 4, 4] and idx.tolist() == [0, 1, 0, 1]
        if hits is not None:
            assert hits.tolist() == [0, 3, 4, 8, 8]  # the enumeration's offsets: every segment behind the first one moves
        g = ga.OverlapIndex(c, s, e, None, n_chrom=1, kind=kind)
        o = oracle.Index(c, s, e, None, n_chrom=1, kind=kind)
        off, idx = g.find_overlap_indices(qc, qs, qe, mo)
        _same((off, idx), o.irs_find_overlaps(c, s, e, qc, qs, qe, mo))
        assert off.tolist() == [0, 3, 4, 8, 8] and idx.tolist() == [0, 1, 2, 3, 0, 1, 2, 3]


@pytest.fixture(scope="module")
def igd_pair(ga):
    c, s, e, f, v = IGD_DB
    g = ga.IgdIndex(c, s, e, f, v, n_chrom=2, n_files=2)
    o = oracle.Igd()
    o.add_arrays(c, s, e, v, f)
    o.n_files = 2
    o.finalize()
    return g, o


@pytest.mark.parametrize("nq", (0, 1, 65))
def test_igd_entry_points_at_size_edges(igd_pair, nq):
    g, o = igd_pair
    qc, qs, qe = _queries(nq)
    for mo in (1, 2):
        assert g.count_set_overlaps(qc, qs, qe, mo).tolist() == o.count_set_overlaps(qc, qs, qe, mo, n_files=2).tolist(), mo
        assert g.count_region_hits(qc, qs, qe, mo).tolist() == o.count_region_hits(qc, qs, qe, mo, n_files=2).tolist(), mo
        assert g.count_overlaps_per_query(qc, qs, qe, mo).tolist() == o.count_overlaps_per_query(qc, qs, qe, mo).tolist(), mo
        _same(g.find_overlaps_regionset(qc, qs, qe, mo), o.find_overlaps_regionset(qc, qs, qe, mo))  # same walk order


def test_igd_count_sets_with_an_empty_set(igd_pair):
    g, o = igd_pair
    full, empty = _queries(65), _queries(0)
    for binary in (False, True):
        want = (o.count_region_hits if binary else o.count_set_overlaps)(*full, 1, n_files=2)
        assert want.sum() > 0
        assert g.count_sets([full, empty], 1, binary).tolist() == [want.tolist(), [0, 0]]
        assert g.count_sets([empty, full], 1, binary).tolist() == [[0, 0], want.tolist()]
