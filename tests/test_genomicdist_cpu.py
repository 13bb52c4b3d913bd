"""Structural operations and region-set statistics without a GPU: the plain-Python restatement
(tests/genomicdist_ref.py) against the reference's literal cases and against its own brute-force forms, the host-side
RegionSet methods, the new import surface, and the device methods refusing to compute (no CPU fallback)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import genomicdist_ref as G  # noqa: E402

TOP = 0xFFFFFFFF
# dummy.narrowPeak of the reference's test data, chr1, as its tests list the regions (statistics.rs:503-560)
PEAKS = [("chr1", s, e) for s, e in [(5, 7), (8, 10), (11, 13), (14, 20), (16, 18), (17, 22), (25, 28), (25, 32), (27, 36)]]


def _rs(regs, strands=None):
    from gtars.models import RegionSet

    return RegionSet.from_vectors([r[0] for r in regs], [r[1] for r in regs], [r[2] for r in regs], strands)


def _tuples(rs):
    return [(r.chr, r.start, r.end) for r in rs]


def _random(rng, n, names=("chr2", "chr10", "chrX", "1", "chrM")):
    c = rng.choice(list(names), n)
    s = rng.integers(0, 300, n)
    w = rng.choice([0, 1, 3, 20, 80], n)
    e = s + w
    inv = rng.random(n) < 0.1
    e[inv] = np.maximum(s[inv] - rng.integers(1, 20, inv.sum()), 0)
    top = rng.random(n) < 0.05
    s[top] = TOP - rng.integers(0, 50, top.sum())
    e[top] = np.minimum(s[top] + rng.integers(0, 60, top.sum()), TOP)
    return [(str(c[i]), int(s[i]), int(e[i])) for i in range(n)]


# ------------------------------------------------------------------------------------------- reference literal cases
def test_ref_widths_and_neighbours_literal_cases():
    assert G.widths([("chr1", 100, 200), ("chr1", 300, 550)]) == [100, 250]
    assert G.neighbor_distances([("chr1", 100, 200), ("chr1", 300, 400), ("chr1", 500, 600)]) == [100, 100]
    assert G.neighbor_distances([("chr1", 100, 300), ("chr1", 200, 400)]) == []
    assert G.neighbor_distances([("chr1", 0, 10), ("chr2", 0, 10)]) == []
    assert G.nearest_neighbors([("chr1", 0, 10), ("chr1", 20, 30), ("chr1", 100, 110)]) == [10, 10, 70]
    assert G.nearest_neighbors([("chr1", 0, 10)]) == []
    assert G.nearest_neighbors([("chr1", 0, 10), ("chr2", 0, 10)]) == []
    assert G.neighbor_distances(PEAKS) == [1, 1, 1, 3]
    assert G.nearest_neighbors(PEAKS) == [1, 1, 1, 0, 0, 0, 0, 0, 0]


def test_ref_statistics_and_distribution_literal_cases():
    st = G.chromosome_statistics(PEAKS)["chr1"]
    assert st[:5] == (9, 5, 36, 2, 9) and st[6] == 3.0
    assert len(G.distribution(PEAKS, 5)) == 5
    d = G.distribution([("chr1", 0, 100), ("chr1", 500, 600)], 10)
    assert any(b["n"] > 0 for b in d)
    assert len(G.distribution([("chr1", 0, 1000)])) > 0
    d = G.distribution([("chr1", 0, 100), ("chr2", 200, 300)], 10, {"chr1": 1000, "chr2": 500})
    assert all(b["end"] - b["start"] == 100 for b in d if b["chr"] == "chr1")
    assert all(0 < b["end"] - b["start"] <= 100 for b in d if b["chr"] == "chr2")
    d = G.distribution([("chr1", 100, 200), ("chr1", 1200, 1300), ("chr2", 200, 300), ("chr2", 2000, 2100)], 10,
                       {"chr1": 1000, "chr2": 500})
    assert sum(b["n"] for b in d) == 2 and all(b["end"] > b["start"] and b["rid"] < 10 for b in d)
    assert G.distribution(PEAKS, 0, {"chr1": 100}) == []


def test_ref_gaps_literal_cases():
    cs = {"chr1": 100}
    assert G.gaps([("chr1", 10, 20), ("chr1", 30, 40), ("chr1", 50, 60)], cs) == [
        ("chr1", 0, 10), ("chr1", 20, 30), ("chr1", 40, 50), ("chr1", 60, 100)]
    assert G.gaps([("chr1", 0, 10), ("chr1", 20, 30)], cs) == [("chr1", 10, 20), ("chr1", 30, 100)]
    assert G.gaps([("chr1", 10, 20), ("chr1", 80, 100)], cs) == [("chr1", 0, 10), ("chr1", 20, 80)]
    assert G.gaps([("chr1", 10, 20), ("chr1", 80, 150)], cs) == [("chr1", 0, 10), ("chr1", 20, 80)]
    assert sorted(G.gaps([], {"chr1": 100, "chr2": 50})) == [("chr1", 0, 100), ("chr2", 0, 50)]
    assert all(r[0] == "chr1" for r in G.gaps([("chr1", 10, 20), ("chr2", 5, 15)], cs))
    assert [r for r in G.gaps([("chr1", 10, 20)], {"chr1": 100, "chr2": 200}) if r[0] == "chr2"] == [("chr2", 0, 200)]
    assert G.gaps([("chr1", 10, 30), ("chr1", 25, 40), ("chr1", 50, 60)], cs) == [
        ("chr1", 0, 10), ("chr1", 40, 50), ("chr1", 60, 100)]
    got = G.gaps([("chr2", 10, 20), ("chr1", 10, 20), ("chr10", 10, 20)], {"chr10": 100, "chr1": 100, "chr2": 100})
    assert list(dict.fromkeys(r[0] for r in got)) == ["chr1", "chr2", "chr10"]
    assert G.gaps([("chr1", 0, 100)], cs) == []


def test_ref_gaps_pins_names_that_share_a_key():
    # chr1 / 1 / chr+1 share key (0, 1); chrM / chrMT share (3, 0): interleaved by start, then name bytewise
    got = G.gaps([("chr1", 5, 10), ("1", 0, 3), ("chr+1", 2, 4)], {"chr1": 20, "1": 20, "chr+1": 20, "chrMT": 9, "chrM": 9,
                                                                    "chrY": 1, "chrX": 1, "chr0": 0, "chrUn": 3})
    assert got == [("1", 0, 0)][:0] + [("chr+1", 0, 2), ("chr1", 0, 5), ("1", 3, 20), ("chr+1", 4, 20), ("chr1", 10, 20),
                                       ("chrX", 0, 1), ("chrY", 0, 1), ("chrM", 0, 9), ("chrMT", 0, 9), ("chrUn", 0, 3)]
    assert G.karyotype_key("chr4294967296") == (4, 0, b"4294967296")
    assert G.karyotype_key("chr+") == (4, 0, b"+") and G.karyotype_key("chr-1") == (4, 0, b"-1")
    assert G.karyotype_key("007") == (0, 7, b"") and G.karyotype_key("chrx") == (4, 0, b"x")


def test_ref_disjoin_and_consensus_literal_cases():
    assert G.disjoin([("chr1", 0, 100), ("chr1", 50, 150)]) == [("chr1", 0, 50), ("chr1", 50, 100), ("chr1", 100, 150)]
    assert G.disjoin([("chr1", 0, 100), ("chr1", 200, 300)]) == [("chr1", 0, 100), ("chr1", 200, 300)]
    assert G.disjoin([]) == []
    # inverted and zero-width regions add boundaries, never coverage
    assert G.disjoin([("c", 0, 10), ("c", 8, 3), ("c", 5, 5), ("c", 20, 20)]) == [("c", 0, 3), ("c", 3, 5), ("c", 5, 8),
                                                                                   ("c", 8, 10)]
    assert G.consensus([[("chr1", 0, 100)], [("chr1", 50, 150)]]) == [("chr1", 0, 150, 2)]
    assert G.consensus([[("chr1", 0, 10)], [("chr1", 20, 30)]]) == [("chr1", 0, 10, 1), ("chr1", 20, 30, 1)]
    assert G.consensus([[("chr1", 0, 10)], [("chr1", 5, 15)], [("chr1", 8, 20)]]) == [("chr1", 0, 20, 3)]
    assert G.consensus([]) == []
    # a zero-width run is hit by nothing; a zero-width region does not hit its own run; an inverted one can
    assert G.consensus([[("c", 0, 0)], [("c", 0, 10)], [("c", 6, 2)]]) == [("c", 0, 10, 2)]
    assert G.consensus([[("c", 5, 5)], [("c", 0, 10)]]) == [("c", 0, 10, 2)]  # strictly inside: a hit
    assert G.consensus([[("c", 5, 5)], [("c", 7, 7)]]) == [("c", 5, 5, 0), ("c", 7, 7, 0)]


def test_ref_host_side_literal_cases():
    assert G.trim([("chr1", 0, 1000), ("chr2", 500, 2000)], {"chr1": 500, "chr2": 1500}) == [("chr1", 0, 500),
                                                                                             ("chr2", 500, 1500)]
    assert G.trim([("chr1", 0, 100), ("chrZ", 0, 100)], {"chr1": 1000}) == [("chr1", 0, 100)]
    assert G.trim([("c", 50, 10)], {"c": 40}) == [] and G.trim([("c", 50, 10)], {"c": 5}) == [("c", 5, 5)]
    assert G.promoters([("chr1", 1000, 2000)], 200, 50) == [("chr1", 800, 1050)]
    assert G.promoters([("chr1", 50, 200), ("c", TOP - 3, TOP)], 100, 10) == [("chr1", 0, 60), ("c", TOP - 103, TOP)]
    assert G.pintersect([("chr1", 0, 100)], [("chr1", 50, 200)]) == [("chr1", 50, 100)]
    assert G.pintersect([("a", 5, 10), ("a", 0, 10), ("a", 0, 3)], [("b", 0, 10), ("a", 20, 30)]) == [("a", 5, 5),
                                                                                                      ("a", 20, 20)]
    assert G.median_abs_distance([1.0, -3.0, 5.0, -7.0]) == 4.0
    assert G.median_abs_distance([42.0]) == 42.0
    assert G.median_abs_distance([]) is None
    assert G.median_abs_distance([1.0, float("nan"), 3.0]) == 2.0
    assert G.median_abs_distance([float("inf"), -2.9, 2.0 ** 63, -2.0 ** 70]) == (2.0 + 2.0 ** 63) / 2.0
    assert G.mean_region_width([("c", 0, 1), ("c", 0, 2), ("c", 0, 2)]) == 1.67
    assert G.mean_region_width([("c", 0, 1), ("c", 0, 0), ("c", 0, 0), ("c", 0, 0), ("c", 0, 0), ("c", 0, 0),
                                ("c", 0, 0), ("c", 0, 0)]) == 0.13  # 12.5 rounds half away from zero
    assert math.isnan(G.mean_region_width([]))
    assert G.get_max_end_per_chr([("a", 0, 9), ("b", 0, 5), ("a", 0, 3)]) == {"a": 3, "b": 5}
    with pytest.raises(ValueError):
        G.get_max_end_per_chr([])


# --------------------------------------------------------------------------------------- brute force vs fast form
@pytest.mark.parametrize("seed", range(6))
def test_ref_fast_forms_equal_the_brute_force(seed):
    rng = np.random.default_rng(seed)
    regs = _random(rng, 300)
    assert G.disjoin(regs) == G.disjoin_brute(regs)
    assert G.neighbor_distances(regs) == G.neighbor_distances_brute(regs)
    assert G.nearest_neighbors(regs) == G.nearest_neighbors_brute(regs)
    sets = [_random(rng, int(rng.integers(0, 60))) for _ in range(7)]
    assert G.consensus(sets) == G.consensus_brute(sets)


def test_ref_median_wraps_and_distribution_wraps():
    assert G.chromosome_statistics([("c", 0, TOP), ("c", 0, 3)])["c"][6] == 1.0  # (2^32 - 1 + 3) mod 2^32 / 2
    # midpoint start + width / 2 wraps; bin_start + bin_size wraps before the min with the chromosome end
    d = G.distribution([("c", 0, 10), ("c", TOP - 2, TOP), ("c", 10, 5)], 2)
    assert d == [{"chr": "c", "start": 0, "end": 2147483647, "n": 1, "rid": 0},
                 {"chr": "c", "start": 2147483647, "end": 4294967294, "n": 1, "rid": 1},
                 {"chr": "c", "start": 4294967294, "end": 2147483645, "n": 1, "rid": 2}]


# ------------------------------------------------------------------------------------------ host-side methods
def test_host_side_methods():
    from gtars.models import RegionSet

    a = _rs([("chr1", 0, 1000), ("chr2", 500, 2000), ("chrZ", 0, 5)], ["+", "-", "+"])
    t = a.trim({"chr1": 500, "chr2": 1500})
    assert _tuples(t) == [("chr1", 0, 500), ("chr2", 500, 1500)] and t.strands == ["*", "*"]
    p = a.promoters(600, 50)
    assert _tuples(p) == [("chr1", 0, 50), ("chr2", 0, 550), ("chrZ", 0, 50)] and p.strands == ["+", "-", "+"]
    b = _rs([("chr1", 50, 200), ("chr9", 0, 9)])
    pi = a.pintersect(b)
    assert _tuples(pi) == [("chr1", 50, 200), ("chr2", 500, 500)] and pi.strands == ["+", "-", "+"]
    c = RegionSet.from_regions(a.regions[:1]).concat(_rs([("chr3", 1, 2)], ["-"]))
    assert _tuples(c) == [("chr1", 0, 1000), ("chr3", 1, 2)] and c.strands == ["*", "-"]
    assert a.widths() == a.region_widths() == [1000, 1500, 5]
    assert _rs([("c", 5, 2)]).widths() == [TOP - 2]
    assert a.mean_region_width() == G.mean_region_width(_tuples(a))
    assert a.get_max_end_per_chr() == {"chr1": 1000, "chr2": 2000, "chrZ": 5}
    with pytest.raises(ValueError):
        _rs([]).get_max_end_per_chr()
    rng = np.random.default_rng(9)
    regs = _random(rng, 500)
    x, y = _rs(regs), _rs(regs[::-1][:300])
    sizes = {"chr2": 200, "chr10": 5000, "1": 3}
    assert _tuples(x.trim(sizes)) == G.trim(regs, sizes)
    assert _tuples(x.promoters(77, TOP)) == G.promoters(regs, 77, TOP)
    assert _tuples(x.pintersect(y)) == G.pintersect(regs, regs[::-1][:300])
    assert x.widths() == G.widths(regs)
    assert x.mean_region_width() == G.mean_region_width(regs)
    assert x.get_max_end_per_chr() == G.get_max_end_per_chr(regs)


def test_median_abs_distance_host():
    from gtars.genomic_distributions import median_abs_distance

    for v in ([1.0, -3.0, 5.0, -7.0], [42.0], [], [1.0, float("nan"), 3.0], [float("-inf"), 2.5, -2.0 ** 64, 7, -1]):
        assert median_abs_distance(v) == G.median_abs_distance(v)


def test_import_surface():
    import importlib

    import gtars
    import gtars_amd
    from gtars.genomic_distributions import consensus, median_abs_distance  # noqa: F401
    from gtars.models import ChromosomeStatistics

    assert importlib.import_module("gtars.genomic_distributions") is gtars_amd.genomic_distributions
    assert "genomic_distributions" in gtars.__all__
    for name in ("calc_gc_content", "calc_partitions", "calc_summary_signal"):
        assert not hasattr(gtars.genomic_distributions, name)
    s = ChromosomeStatistics("chr1", 2, 5, 9, 1, 3, 2.0, 2.0)
    assert (s.chromosome, s.number_of_regions, s.start_nucleotide_position, s.end_nucleotide_position,
            s.minimum_region_length, s.maximum_region_length, s.mean_region_length, s.median_region_length) == (
        "chr1", 2, 5, 9, 1, 3, 2.0, 2.0)
    with pytest.raises(AttributeError):
        s.number_of_regions = 3


DEVICE_METHODS = [
    ("disjoin", lambda a: a.disjoin()),
    ("gaps", lambda a: a.gaps({"chr1": 100})),
    ("neighbor_distances", lambda a: a.neighbor_distances()),
    ("nearest_neighbors", lambda a: a.nearest_neighbors()),
    ("distribution", lambda a: a.distribution(10)),
    ("distribution_sizes", lambda a: a.distribution(10, {"chr1": 100})),
    ("chromosome_statistics", lambda a: a.chromosome_statistics()),
    ("consensus", lambda a: __import__("gtars.genomic_distributions").genomic_distributions.consensus([a, a])),
]


@pytest.mark.parametrize("name,call", DEVICE_METHODS, ids=[n for n, _ in DEVICE_METHODS])
def test_device_methods_have_no_cpu_fallback(name, call):
    import gtars_amd

    a = _rs([("chr1", 0, 10), ("chr2", 5, 50), ("chr1", 20, 30)])
    if gtars_amd.device_count() > 0:
        call(a)  # (tests/test_gpu_genomicdist.py checks the values)
        return
    with pytest.raises(gtars_amd.NoDeviceError):
        call(a)
