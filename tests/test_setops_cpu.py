"""Region-set algebra without a GPU: the plain-Python restatement (tests/setops_ref.py) against the reference's own
literal cases, and the device-only methods of RegionSet / RegionSetList refusing to compute (no CPU fallback)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import setops_ref as R  # noqa: E402


def test_ref_reduce_literal_cases():
    assert R.reduce([("chr1", 0, 10), ("chr1", 5, 15), ("chr1", 20, 30)]) == [("chr1", 0, 15), ("chr1", 20, 30)]
    assert R.reduce([("chr1", 0, 10), ("chr1", 10, 20)]) == [("chr1", 0, 20)]  # adjacent regions merge
    assert R.reduce([]) == []


def test_ref_reduce_sorts_names_bytewise_and_not_by_end():
    assert R.reduce([("chr2", 0, 5), ("chr10", 0, 5)]) == [("chr10", 0, 5), ("chr2", 0, 5)]
    # [10,5) before [10,20): 10 > 5 opens a new run; the other order would merge
    assert R.reduce([("c", 10, 5), ("c", 10, 20)]) == [("c", 10, 5), ("c", 10, 20)]
    assert R.reduce([("c", 10, 20), ("c", 10, 5)]) == [("c", 10, 20)]


def test_ref_setdiff_union_literal_cases():
    assert R.setdiff([("chr1", 0, 100)], [("chr1", 30, 60)]) == [("chr1", 0, 30), ("chr1", 60, 100)]
    assert R.union([("chr1", 0, 10)], [("chr1", 5, 15)]) == [("chr1", 0, 15)]


def test_ref_jaccard_literal_cases():
    a = [("chr1", 0, 100)]
    assert R.jaccard(a, a) == 1.0
    assert R.jaccard(a, [("chr1", 200, 300)]) == 0.0
    assert R.jaccard([], []) == 0.0


def test_ref_closest_unsorted_other():
    a = [("chr1", 100, 200)]
    other = [("chr1", 500, 600), ("chr1", 210, 220), ("chr1", 0, 10)]
    assert R.closest(a, other) == [(0, 1, 10)]
    assert R.closest(a, []) == []
    assert R.closest([("chrX", 0, 1)], other) == []


def test_ref_wrapping_totals_and_cluster_saturation():
    big = [("c", 0, 0xFFFFFFFF), ("c", 0xFFFFFFFF, 0xFFFFFFFF)]
    assert R.nucleotides_length(big + [("d", 0, 2)]) == 1  # (2^32 - 1) + 2 wraps
    assert R.cluster([("c", 0, 0xFFFFFFF0), ("c", 0xFFFFFFFF, 0xFFFFFFFF)], 0xFFFFFFFF) == [0, 0]
    assert R.cluster([("c", 0, 10), ("c", 12, 20), ("d", 0, 1)], 1) == [0, 1, 2]
    assert R.cluster([("c", 0, 10), ("c", 12, 20)], 2) == [0, 0]


DEVICE_METHODS = [
    ("reduce", lambda a, b: a.reduce()),
    ("union", lambda a, b: a.union(b)),
    ("setdiff", lambda a, b: a.setdiff(b)),
    ("intersect_all", lambda a, b: a.intersect_all(b)),
    ("jaccard", lambda a, b: a.jaccard(b)),
    ("coverage", lambda a, b: a.coverage(b)),
    ("overlap_coefficient", lambda a, b: a.overlap_coefficient(b)),
    ("closest", lambda a, b: a.closest(b)),
    ("cluster", lambda a, b: a.cluster(100)),
]


@pytest.mark.parametrize("name,call", DEVICE_METHODS, ids=[n for n, _ in DEVICE_METHODS])
def test_set_algebra_has_no_cpu_fallback(name, call):
    import gtars_amd
    from gtars.models import RegionSet

    a = RegionSet.from_vectors(["chr1", "chr2"], [0, 5], [10, 50])
    b = RegionSet.from_vectors(["chr1"], [5], [20])
    if gtars_amd.device_count() > 0:
        call(a, b)  # (tests/test_gpu_setops.py checks the values)
        return
    with pytest.raises(gtars_amd.NoDeviceError):
        call(a, b)


def test_region_set_list_surface_and_no_cpu_fallback():
    import gtars_amd
    from gtars.models import RegionSet, RegionSetList

    a = RegionSet.from_vectors(["chr1", "chr2"], [0, 5], [10, 50])
    b = RegionSet.from_vectors(["chr1"], [5], [20])
    rsl = RegionSetList([a, b])
    assert len(rsl) == 2 and rsl[1] is b and rsl[-2] is a and list(rsl) == [a, b]
    assert rsl.names() is None
    with pytest.raises(IndexError):
        rsl[2]
    cat = rsl.concat()
    assert [(r.chr, r.start, r.end) for r in cat] == [("chr1", 0, 10), ("chr2", 5, 50), ("chr1", 5, 20)]
    assert a.get_nucleotide_length() == 55
    if gtars_amd.device_count() == 0:
        with pytest.raises(gtars_amd.NoDeviceError):
            rsl.pairwise_jaccard()
