"""Structural operations and region-set statistics on the MI355X (csrc/setops.hip, K9) against the plain-Python
restatement tests/genomicdist_ref.py: seeded random differentials of every device operation with exact equality, and
cross-checks that do not rest on the restatement (lola.build_restricted_universe, the device reduce and any_overlaps)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_layouts as E  # noqa: E402
import genomicdist_ref as G  # noqa: E402
import setops_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

TOP = 0xFFFFFFFF
# first appearance differs from the bytewise order; "1" shares chr1's karyotype key, chrMT shares chrM's
NAMES = ["chr2", "chr10", "chr1_alt", "chrX", "chrM", "1", "chr1", "chrMT"]


def _rs(regs):
    from gtars.models import RegionSet

    return RegionSet.from_vectors([r[0] for r in regs], [r[1] for r in regs], [r[2] for r in regs])


def _tuples(rs):
    names, ids, s, e = rs.chrom_names, rs.chrom_ids, rs.starts, rs.ends
    return [(names[int(ids[i])], int(s[i]), int(e[i])) for i in range(len(rs))]


def _random_set(rng, n, names=NAMES, inverted=True, span=20_000):
    """duplicates, nested, touching, zero-width and inverted regions, ends near 2^32 - 1"""
    c = rng.choice(names, n)
    s = rng.integers(0, span, n)
    w = rng.choice([0, 1, 5, 50, 400, 3000], n, p=[0.08, 0.12, 0.3, 0.3, 0.15, 0.05]) + rng.integers(0, 10, n)
    w[rng.random(n) < 0.05] = 0
    e = s + w
    top = rng.random(n) < 0.03
    s[top] = TOP - rng.integers(0, 2000, top.sum())
    e[top] = np.minimum(s[top] + rng.integers(0, 3000, top.sum()), TOP)
    regs = [(str(c[i]), int(s[i]), int(e[i])) for i in range(n)]
    for k in rng.integers(0, n, n // 20):  # touching
        ch, _, en = regs[k]
        regs.append((ch, en, min(en + int(rng.integers(0, 100)), TOP)))
    regs += [regs[k] for k in rng.integers(0, len(regs), n // 20)]  # duplicates
    for k in rng.integers(0, n, n // 40):  # nested
        ch, st, en = regs[k]
        if en - st > 2:
            regs.append((ch, st + 1, en - 1))
    if inverted:
        for k in rng.integers(0, len(regs), max(1, n // 50)):
            ch, st, _ = regs[k]
            regs[k] = (ch, st, max(0, st - int(rng.integers(1, 60))))
    order = rng.permutation(len(regs))
    return [regs[i] for i in order]


def _stats(rs):
    return {k: (v.number_of_regions, v.start_nucleotide_position, v.end_nucleotide_position, v.minimum_region_length,
                v.maximum_region_length, v.mean_region_length, v.median_region_length)
            for k, v in rs.chromosome_statistics().items()}


def _check_result_set(rs):
    assert rs.header is None and all(x == "*" for x in rs.strands) and all(r.rest is None for r in rs.regions)


SIZES = {"chr2": 15_000, "chr10": 30_000, "chrX": 0, "chrM": TOP, "chrMT": 7, "1": 500, "chr1": 25_000, "chrY": 99,
         "chr22": 1000}


@pytest.mark.parametrize("seed,inverted", [(s, inv) for s in range(3) for inv in (False, True)])
def test_every_operation_against_the_restatement(seed, inverted):
    from gtars.genomic_distributions import consensus

    rng = np.random.default_rng(2000 + seed)
    a = _random_set(rng, 3000, inverted=inverted)
    A = _rs(a)
    d = A.disjoin()
    _check_result_set(d)
    assert _tuples(d) == G.disjoin(a)
    g = A.gaps(SIZES)
    _check_result_set(g)
    assert _tuples(g) == G.gaps(a, SIZES)
    assert _tuples(A.gaps({})) == [] and _tuples(A.gaps({"chrQ": 10})) == [("chrQ", 0, 10)]
    assert A.neighbor_distances() == G.neighbor_distances(a)
    assert A.nearest_neighbors() == G.nearest_neighbors(a)
    for n_bins in (250, 1, 7, 0, TOP):
        assert A.distribution(n_bins) == G.distribution(a, n_bins)
        assert A.distribution(n_bins, SIZES) == G.distribution(a, n_bins, SIZES)
    assert A.distribution() == G.distribution(a)
    assert A.distribution(10, {}) == G.distribution(a, 10, {})
    assert _stats(A) == G.chromosome_statistics(a)
    sets = [_random_set(rng, int(rng.integers(1, 800)), NAMES[: 3 + k % 5], inverted) for k in range(6)] + [[]]
    want = [{"chr": c, "start": s, "end": e, "count": n} for c, s, e, n in G.consensus(sets)]
    assert consensus([_rs(s) for s in sets]) == want


def test_small_and_empty_sets():
    from gtars.genomic_distributions import consensus

    E = _rs([])
    assert _tuples(E.disjoin()) == []
    assert _tuples(E.gaps({"chr1": 100, "chr2": 0, "2": 5})) == [("chr1", 0, 100), ("2", 0, 5)]
    assert E.neighbor_distances() == [] and E.nearest_neighbors() == []
    assert E.distribution() == [] and E.distribution(5, {"chr1": 10}) == []
    assert E.chromosome_statistics() == {}
    assert consensus([]) == [] and consensus([E, E]) == []
    one = [("chr1", 10, 20)]
    assert _tuples(_rs(one).disjoin()) == [("chr1", 10, 20)]
    assert _rs(one).nearest_neighbors() == [] and _rs(one).neighbor_distances() == []
    assert consensus([_rs([("c", 5, 5)]), _rs([("c", 7, 7)])]) == [
        {"chr": "c", "start": 5, "end": 5, "count": 0}, {"chr": "c", "start": 7, "end": 7, "count": 0}]
    st = _rs([("c", 0, TOP), ("c", 0, 3)]).chromosome_statistics()["c"]
    assert st.median_region_length == 1.0 and st.mean_region_length == (TOP + 3) / 2


def _big(seed, n, n_chrom=5, span=3_000_000):
    """few chromosomes: every chromosome spans many scan tiles"""
    rng = np.random.default_rng(seed)
    names = [f"chr{i + 1}" for i in range(n_chrom)][::-1]
    c = rng.integers(0, n_chrom, n)
    s = rng.integers(0, span, n)
    e = s + rng.integers(0, 600, n)
    inv = rng.random(n) < 0.001
    e[inv] = s[inv] // 2
    return [(names[c[i]], int(s[i]), int(e[i])) for i in range(n)]


def test_disjoin_and_statistics_at_one_million_regions():
    from gtars_amd import lola

    a = _big(31, 1_000_000)
    A = _rs(a)
    got = _tuples(A.disjoin())
    assert got == G.disjoin(a)
    assert got == lola.build_restricted_universe([A])
    assert _stats(A) == G.chromosome_statistics(a)
    assert A.distribution() == G.distribution(a)
    sizes = {f"chr{i + 1}": 2_500_000 + 100_000 * i for i in range(5)}
    assert A.distribution(250, sizes) == G.distribution(a, 250, sizes)
    assert A.nearest_neighbors() == G.nearest_neighbors(a)
    assert A.neighbor_distances() == G.neighbor_distances(a)
    assert _tuples(A.gaps(sizes)) == G.gaps(a, sizes)


def test_disjoin_matches_the_lola_restatement_on_irregular_sets():
    from gtars_amd import lola

    rng = np.random.default_rng(41)
    for k in range(3):
        A = _rs(_random_set(rng, 4000))
        assert _tuples(A.disjoin()) == lola.build_restricted_universe([A])


def test_consensus_of_64_sets_against_reduce_and_any_overlaps():
    from gtars.genomic_distributions import consensus
    from gtars.models import RegionSetList

    rng = np.random.default_rng(51)
    regs = [_random_set(rng, 3000, NAMES[: 2 + k % 7], inverted=k % 3 == 0, span=200_000) for k in range(64)]
    sets = [_rs(r) for r in regs]
    got = consensus(sets)
    want = [{"chr": c, "start": s, "end": e, "count": n} for c, s, e, n in G.consensus(regs)]
    assert got == want
    union = RegionSetList(sets).concat().reduce()
    assert [(x["chr"], x["start"], x["end"]) for x in got] == _tuples(union)
    hits = np.zeros(len(union), dtype=np.int64)
    for s in sets:
        hits += np.asarray(union.any_overlaps(s), dtype=np.int64)
    assert [x["count"] for x in got] == hits.tolist()


# ---- sizes on the edges of a lane, a wave, a workgroup and a 2048-element tile ------------------------------------------
@pytest.mark.parametrize("n,boundary", E.edge_cases())
def test_every_operation_at_tile_edge_sizes(n, boundary):
    from gtars.genomic_distributions import consensus

    rng = np.random.default_rng(4000 + n)
    # (_random_set returns its n regions and their extras shuffled together: a random n of them)
    a = _random_set(rng, n, names=["chr10"])[:n]
    b = _random_set(rng, n, names=["chr10"], inverted=False)[:n]
    if boundary is not None:
        a, b = E.split_at(a, boundary), E.split_at(b, boundary)
    assert len(a) == n and len(b) == n
    A = _rs(a)
    assert _tuples(A.disjoin()) == G.disjoin(a)
    assert _tuples(A.gaps(SIZES)) == G.gaps(a, SIZES)
    assert A.neighbor_distances() == G.neighbor_distances(a)
    assert A.nearest_neighbors() == G.nearest_neighbors(a)
    for n_bins in (250, 7):
        assert A.distribution(n_bins) == G.distribution(a, n_bins)
        assert A.distribution(n_bins, SIZES) == G.distribution(a, n_bins, SIZES)
    assert _stats(A) == G.chromosome_statistics(a)
    want = [{"chr": c, "start": s, "end": e, "count": k} for c, s, e, k in G.consensus([a, b, a])]
    assert consensus([A, _rs(b), A]) == want


# ---- structured layouts whose carries cross two 1024-tile chunk seams ----------------------------------------------------
def test_disjoin_under_one_region_covering_two_chunk_seams():
    lay = E.covering(E.N_SEAMS, seed=21)
    d = E.layout_set(lay).disjoin()
    assert d.chrom_names == lay.names and len(d) == len(lay.disjoin[1])
    assert np.array_equal(d.starts, lay.disjoin[1]) and np.array_equal(d.ends, lay.disjoin[2])


def test_neighbors_statistics_and_distribution_of_disjoint_regions_over_two_chunk_seams():
    lay = E.disjoint(E.N_SEAMS, seed=22)
    A = E.layout_set(lay)
    assert np.array_equal(np.asarray(A.neighbor_distances(), dtype=np.int64), lay.neighbor_distances)
    assert _stats(A) == lay.chromosome_statistics
    for n_bins in (250, 7):
        assert A.distribution(n_bins, lay.sizes) == lay.distribution(n_bins)


@pytest.mark.parametrize("shift", [0, 1])
def test_neighbor_distances_with_chromosome_heads_on_tile_firsts_and_lasts(shift):
    lay = E.disjoint(E.N_SEAMS, seed=23 + shift, per_chrom=2048, shift=shift)
    A = E.layout_set(lay)
    assert np.array_equal(np.asarray(A.neighbor_distances(), dtype=np.int64), lay.neighbor_distances)
    assert _stats(A) == lay.chromosome_statistics


# ---- chromosome keys of three bytes in the sort ---------------------------------------------------------------------------
def test_statistics_of_seventy_thousand_chromosomes():
    a = E.wide_set(61, 70_000)
    assert len({r[0] for r in a}) == 70_000 > 65_536
    A = _rs(a)
    assert _stats(A) == G.chromosome_statistics(a)
    assert _tuples(A.disjoin()) == G.disjoin(a)
    assert A.neighbor_distances() == G.neighbor_distances(a)


def test_consensus_with_more_than_65536_set_chromosome_segments():
    from gtars.genomic_distributions import consensus

    regs = [E.wide_set(70 + k, 2000) for k in range(40)]
    want = [{"chr": c, "start": s, "end": e, "count": k} for c, s, e, k in G.consensus(regs)]
    assert consensus([_rs(r) for r in regs]) == want
