"""Every grid-stride kernel past the first trip of its loop.

grid_for (csrc/pipeline.h) and stream_grid (csrc/kernels.hip) clip a launch at 2,048 .. 65,536 workgroups and the kernels walk the
rest with `for (i = ...; i < n; i += gridDim.x * blockDim.x)`: at the suite's shapes that loop runs once.  GTARS_GRID_CAP = C
(a test switch) lowers both helpers' caps to C workgroups, so that a few hundred rows are several trips, the last one partial and
with idle workgroups.  Every family of kernels whose geometry comes from one of the helpers runs here under C = 1 and C = 3
against the family's own restatement in tests/ (never against the same call without the cap), with exact equality as in the
family's own module.

Sizes.  With `per` items per workgroup: 1, per - 1, per * C, per * C + 1 and 5 * per * C + per / 2 + 3 (`Cap.sizes`).  The
first three fit the capped grid, so nothing can clip at them: they are the cases in which the capped helper must change
nothing.  At the last two the library's entry points that launch through a helper are named per test, and EVERY call of such
an entry point must raise gtars_debug_grid_clips() -- the library handle of every gtars_amd module is replaced by a recorder
for the length of a test (`_Recorder`), so a call inside a shared checking function is held to this like one made here.  A
test whose calls do not clip fails.

The kernels with a coarse unit (thousands of rows, a chromosome, a pair of sets per lane) run the same five sizes in their unit.
Where the item count of a launch is not the input's size but a derived one -- the rows of a REDUCED set, the gaps found, the
runs of a sort, the clean pairs of a list of sets -- the test computes that count from the restatement and asserts that it
exceeds 5 * per * C: that the entry point's counter rose only says that SOME launch in it clipped.

COVERED maps every kernel of the files that use a helper to the test that runs it past its first trip
(tests/test_grid_cap_inventory_cpu.py keeps the table complete)."""
import os
import random
import sys
from contextlib import contextmanager

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

COVERED = {
    # csrc/setops.hip: reduce / union / setdiff / intersect / totals / closest / cluster
    "k_gather3": "test_set_algebra", "k_run_ids": "test_set_algebra", "k_reduce_write": "test_set_algebra",
    "k_seg_offsets": "test_set_algebra", "k_mark_inverted": "test_set_algebra", "k_sweep_par": "test_set_algebra",
    "k_closest": "test_set_algebra", "k_closest_compact": "test_set_algebra", "k_cluster_scatter": "test_set_algebra",
    "k_sweep_seq": "test_sweep_of_inverted_chromosomes_of_high_rank",
    "k_sum_widths": "test_totals_of_sets_wider_than_a_workgroup_of_the_sum",
    "k_max_width": "test_closest_and_statistics_past_64_regions_per_lane",
    "k_stat_bounds": "test_closest_and_statistics_past_64_regions_per_lane",
    "k_widths": "test_pairwise_jaccard_of_many_sets", "k_pair_finish": "test_pairwise_jaccard_of_many_sets",
    # csrc/setops.hip: disjoin, gaps, neighbours, distribution, statistics, consensus
    "k_dj_events": "test_structure_and_statistics", "k_dj_gather": "test_structure_and_statistics",
    "k_dj_pieces": "test_structure_and_statistics", "k_gaps": "test_gaps_and_bins_of_sets_that_stay_large_when_reduced",
    "k_lookup": "test_gaps_and_bins_of_sets_that_stay_large_when_reduced", "k_neighbors": "test_structure_and_statistics",
    "k_bin_keys": "test_structure_and_statistics", "k_rle_heads": "test_structure_and_statistics",
    "k_rle_write": "test_structure_and_statistics", "k_rle_counts": "test_gaps_and_bins_of_sets_that_stay_large_when_reduced",
    "k_stat_finish": "test_statistics_of_many_chromosomes", "k_gather_widths": "test_structure_and_statistics",
    "k_cons_hits": "test_structure_and_statistics", "k_cons_count": "test_structure_and_statistics",
    # csrc/setops.hip: the folds over a list of sets.  (k_fill is also the name of kernels.hip's per-query fill pass, which
    # find_overlaps and find_overlap_indices run in test_overlap_index_generic_kernels.)
    "k_fill": "test_folds_over_a_list_of_sets", "k_gather1": "test_folds_over_a_list_of_sets",
    "k_ue_finish": "test_folds_over_a_list_of_sets", "k_ue_slices": "test_bulk_union_except_of_many_sets",
    "k_ia_events": "test_folds_over_a_list_of_sets", "k_ia_pieces": "test_folds_over_a_list_of_sets",
    # csrc/annot.hip
    "k_midpoints": "test_tss_distances", "k_tss_dist": "test_tss_distances",
    # csrc/signal.hip
    "k_signal_flags": "test_signal_summary", "k_signal_rows": "test_signal_summary", "k_signal_fold": "test_signal_summary",
    "k_signal_keys": "test_signal_summary",
    # csrc/seqstats.hip
    "k_seq_pieces": "test_gc_and_dinucleotide_counts", "k_seq_count": "test_gc_and_dinucleotide_counts",
    # csrc/countmat.hip
    "k_cm_expand": "test_count_matrix", "k_cm_heads": "test_count_matrix", "k_cm_runs": "test_count_matrix",
    "k_cm_finish": "test_count_matrix",
    # csrc/partitions.hip
    "k_partitions": "test_partitions",
    # csrc/tokbatch.hip
    "k_set_lengths": "test_batched_tokenizer", "k_set_offsets": "test_batched_tokenizer", "k_set_pack": "test_batched_tokenizer",
    "k_set_pad": "test_batched_tokenizer",
    # csrc/refget.hip, csrc/byte_csr.h
    "k_refget_keys": "test_refget_digests_and_substrings", "k_refget_digest": "test_refget_digests_and_substrings",
    "k_refget_rows": "test_refget_digests_and_substrings", "k_csr_fill": "test_refget_digests_and_substrings",
    # csrc/vrs.hip
    "k_vrs_normalize": "test_vrs_alleles", "k_vrs_digest": "test_vrs_alleles", "k_vrs_lens": "test_vrs_alleles",
    "k_vrs_roll_long": "test_vrs_long_rolls",
    # csrc/reftx.hip
    "k_tx_map": "test_transcript_mapping_and_sequences", "k_tx_rows": "test_transcript_mapping_and_sequences",
    "k_tx_digest": "test_transcript_mapping_and_sequences",
    # csrc/hgvs.hip
    "k_hgvs_span": "test_hgvs_bridge", "k_hgvs_offsets": "test_hgvs_bridge", "k_hgvs_merge": "test_hgvs_bridge",
    # csrc/bam.hip
    "k_bam_decode": "test_bam_columns_and_qc", "k_bam_classify": "test_bam_columns_and_qc", "k_bam_names": "test_bam_columns_and_qc",
    "k_bam_key_init": "test_bam_columns_and_qc", "k_bam_run_heads": "test_bam_columns_and_qc", "k_bam_fix_runs": "test_bam_columns_and_qc",
    "k_bam_join": "test_bam_columns_and_qc", "k_bam_key_runs": "test_bam_columns_and_qc",
    # csrc/kernels.hip: the engine's one-thread-per-query kernels
    "k_bits_count": "test_overlap_index_generic_kernels", "k_count": "test_overlap_index_generic_kernels",
    "k_sort_unique_segments": "test_overlap_index_generic_kernels",
    "k_ailist_reorder": "test_nested_ailist_index", "k_permute_marks": "test_nested_ailist_index",
    "k_igd_count": "test_igd_small_batches", "k_igd_count_per_query": "test_igd_small_batches",
    "k_igd_fill_pairs": "test_igd_small_batches", "k_has_adjacent_equal": "test_igd_small_batches",
    "k_hist_u32": "test_histograms", "k_hist_rows": "test_histograms",
}


# ---- the switch, the counter and the recorder -------------------------------------------------------------------------------
class _Recorder:
    """Stands in for the ctypes handle of libgtars_amd.so: every gtars_* function it hands out notes, per call, by how much
    gtars_debug_grid_clips() rose across the call."""

    def __init__(self, real):
        self._real, self.log = real, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("gtars_") or name == "gtars_debug_grid_clips":
            return fn
        clips, log = self._real.gtars_debug_grid_clips, self.log

        def call(*args):
            before = clips()
            try:
                return fn(*args)
            finally:
                log.append((name, clips() - before))

        return call


class Cap:
    def __init__(self, c, rec):
        self.c, self.rec = c, rec

    def sizes(self, per=256):
        """1, per - 1 and per * C fit the capped grid; per * C + 1 is two trips, the second of one item; the last one is six,
        the sixth partial and with idle workgroups"""
        return [1, per - 1, per * self.c, per * self.c + 1, 5 * per * self.c + per // 2 + 3]

    def clips(self, n, per=256):
        return n > per * self.c

    @contextmanager
    def run(self, must_clip, *entry_points):
        """the library calls of the block; must_clip: each of `entry_points` (library functions without their gtars_ prefix) is
        called in it, and every one of their calls raises the clip counter"""
        at = len(self.rec.log)
        yield
        calls = self.rec.log[at:]
        if not must_clip:
            return
        names = {"gtars_" + e for e in entry_points}
        assert names, "a capped block names the entry points that must clip"
        seen = [(n, d) for n, d in calls if n in names]
        missing = sorted(names - {n for n, _ in seen})
        dry = sorted({n for n, d in seen if d == 0})
        assert not missing and not dry, f"not called: {missing}; called without a clipped grid: {dry}; all calls: {calls}"


def _capped(c, monkeypatch):
    import gtars  # noqa: F401  (imports every gtars_amd module the tests use: one imported later would keep the real handle)
    import gtars_amd
    import gtars_amd.engine  # noqa: F401
    import gtars_amd.refget  # noqa: F401
    import gtars_amd.uniwig  # noqa: F401

    real = gtars_amd._lib.lib
    assert gtars_amd.device_count() > 0, "no MI355X visible: -m gpu tests must run on the GPU box"
    rec = _Recorder(real)
    for name, mod in list(sys.modules.items()):
        if name.split(".")[0] == "gtars_amd" and getattr(mod, "lib", None) is real:
            monkeypatch.setattr(mod, "lib", rec)
    monkeypatch.setenv("GTARS_GRID_CAP", str(c))
    return Cap(c, rec)


@pytest.fixture(params=[1, 3], ids=["cap1", "cap3"])
def cap(request, monkeypatch):
    return _capped(request.param, monkeypatch)


@pytest.fixture
def cap1(monkeypatch):
    """for the kernels with a coarse unit (thousands of items per workgroup): one workgroup only"""
    return _capped(1, monkeypatch)


def test_the_switch_and_the_counter(monkeypatch):
    """unset, 0 and a cap above the grid: no clip is counted; the counter rises by one per clipped helper call"""
    import gtars_amd
    from gtars_amd._lib import lib

    ix = gtars_amd.OverlapIndex([0, 0], [10, 30], [20, 40], n_chrom=1)
    q = (np.zeros(600, np.uint32), np.arange(600, dtype=np.uint32), np.arange(600, dtype=np.uint32) + 5)
    want = [int(a < 20 and a + 5 > 10) + int(a < 40 and a + 5 > 30) for a in range(600)]
    for value, clipped in ((None, 0), ("0", 0), ("3", 0), ("2", 1), ("1", 1)):  # 600 queries: three workgroups
        if value is None:
            monkeypatch.delenv("GTARS_GRID_CAP", raising=False)
        else:
            monkeypatch.setenv("GTARS_GRID_CAP", value)
        before = lib.gtars_debug_grid_clips()
        assert ix.bits_count(*q).tolist() == want, value
        assert lib.gtars_debug_grid_clips() - before == clipped, value


# ---- csrc/setops.hip: the algebra ----------------------------------------------------------------------------------------
def _names(n):
    return [f"c{k:04d}" for k in range(n)]  # (bytewise order is index order: the name IS the rank)


def test_set_algebra(cap):
    import setops_ref as R
    import test_gpu_setops as SO

    calls = ("regionset_reduce", "regionset_union", "regionset_setdiff", "regionset_intersect", "regionset_jaccard",
             "regionset_coverage", "regionset_overlap_coefficient", "regionset_closest", "regionset_cluster")
    for n in cap.sizes():
        rng = np.random.default_rng(4000 + n)
        a = SO._exactly(rng, n, SO.NAMES_A, "chr10")
        b = SO._exactly(rng, n, SO.NAMES_B, None)
        with cap.run(cap.clips(n), *calls):
            SO._check_every_operation(a, b)
    # the sweeps of setdiff and intersect (k_seg_offsets, k_mark_inverted, k_sweep_par) walk the REDUCED sets, and the random
    # sets above shrink to a few dozen rows when reduced: two sets that keep every row, with inverted regions on one chromosome
    rng = np.random.default_rng(4999)
    a = _disjoint(rng, n, SO.NAMES_A)
    b = [(c, s + 3, e + 3) for c, s, e in a[: n // 2]] + _disjoint(rng, n, SO.NAMES_B)
    a += [("chrInv", 50 * k + 9, 50 * k) for k in range(5)]
    b += [("chrInv", 50 * k + 30, 50 * k + 20) for k in range(7)]
    assert min(len(R.reduce(a)), len(R.reduce(b))) > 5 * 256 * cap.c
    with cap.run(True, *calls):
        SO._check_every_operation(a, b)


def test_sweep_of_inverted_chromosomes_of_high_rank(cap):
    """k_sweep_seq: one lane per chromosome (rank), 64 per workgroup.  Inverted regions -- which send their whole chromosome
    to this kernel -- on ranks 0, 63, 64 C (the first lane of the second trip), 64 C + 1, in the fifth trip and on the last rank,
    in `a`, in `b` or in both; setdiff and intersect in both directions."""
    import setops_ref as R
    import test_gpu_setops as SO

    per = 64 * cap.c
    for n_rank in cap.sizes(64):
        names = _names(n_rank)
        rng = np.random.default_rng(600 + n_rank)
        a, b = [], []
        for r, name in enumerate(names):
            for regs in (a, b):
                for _ in range(3):
                    s = int(rng.integers(0, 400))
                    regs.append((name, s, s + int(rng.integers(1, 120))))
        dirty = sorted({r for r in (0, 63, per - 1, per, per + 1, 4 * per + 7, n_rank - 1) if r < n_rank})
        for k, r in enumerate(dirty):
            s = 100 + k
            inv = (names[r], s + 50, s)  # start > end
            if k % 3 != 1:
                a.append(inv)
            if k % 3 != 0:
                b.append((names[r], s + 90, s + 20))
        A, B = SO._rs(a), SO._rs(b)
        with cap.run(n_rank > per, "regionset_setdiff", "regionset_intersect"):
            assert SO._tuples(A.setdiff(B)) == R.setdiff(a, b)
            assert SO._tuples(B.setdiff(A)) == R.setdiff(b, a)
            assert SO._tuples(A.intersect_all(B)) == R.intersect(a, b)
            assert SO._tuples(B.intersect_all(A)) == R.intersect(b, a)
        swept = {r[0] for r in R.setdiff(a, b)} | {r[0] for r in R.intersect(a, b)}
        assert {names[r] for r in dirty if r >= per} <= swept  # the later trips' chromosomes have rows in the results


def _disjoint(rng, n, names, width=(1, 9)):
    """n regions that neither touch nor overlap, in shuffled order: reduce keeps every one"""
    c = rng.integers(0, len(names), n)
    start = 20 * rng.permutation(n)
    end = start + rng.integers(width[0], width[1], n)
    return [(names[int(c[i])], int(start[i]), int(end[i])) for i in range(n)]


def test_totals_of_sets_wider_than_a_workgroup_of_the_sum(cap1):
    """k_sum_widths: four regions per lane, 1,024 per workgroup, over the REDUCED sets (disjoint regions: nothing merges)"""
    import setops_ref as R
    import test_gpu_setops as SO

    cap = cap1
    for n in cap.sizes(1024):
        rng = np.random.default_rng(8100 + n)
        a = _disjoint(rng, n, ["x", "y", "z"])
        b = [(c, s + 3, e + 3) for c, s, e in a[: n // 5 + 1]] + _disjoint(rng, 300, ["y", "w"])
        A, B = SO._rs(a), SO._rs(b)
        assert len(R.reduce(a)) == len(a) == n  # (b, and what the two have in common, stay within one workgroup's share)
        with cap.run(n > 1024, "regionset_jaccard", "regionset_coverage", "regionset_overlap_coefficient"):
            assert A.jaccard(B) == R.jaccard(a, b) and B.jaccard(A) == R.jaccard(b, a)
            assert A.coverage(B) == R.coverage(a, b) and B.coverage(A) == R.coverage(b, a)
            assert A.overlap_coefficient(B) == R.overlap_coefficient(a, b)
        assert A.get_nucleotide_length() == R.nucleotides_length(a)


def test_closest_and_statistics_past_64_regions_per_lane(cap1):
    """k_max_width and k_stat_bounds: 64 sorted regions per lane, 16,384 per workgroup.  The widest region of a chromosome and
    its smallest start / largest end lie in a late trip's share."""
    import genomicdist_ref as G
    import setops_ref as R
    import test_gpu_genomicdist as GD
    import test_gpu_setops as SO

    cap = cap1
    names = ["m", "n", "o"]
    for n in cap.sizes(16384):
        rng = np.random.default_rng(8200 + n)
        other = _disjoint(rng, n, names, (1, 15))
        order = sorted(range(n), key=lambda i: (other[i][0], other[i][1]))
        # sorted positions in the 2nd, 4th and last trip, where the set has them
        for at, width in ((16384, 9000), (3 * 16384 + 77, 7000), (n - 2, 8000)):
            if 0 <= at < n:
                c, s, _ = other[order[at]]
                other[order[at]] = (c, s, s + width)
        q = [(names[int(rng.integers(0, 3))], int(s), int(s) + 4) for s in rng.integers(0, 20 * n, 400)]
        O, Q = SO._rs(other), SO._rs(q)
        with cap.run(n > 16384, "regionset_closest", "regionset_chromosome_statistics"):
            assert Q.closest(O) == R.closest(q, other)
            assert GD._stats(O) == G.chromosome_statistics(other)


def test_pairwise_jaccard_of_many_sets(cap):
    """k_pair_finish: one lane per pair of CLEAN sets (no inverted region once reduced; the others go another way); k_widths
    and the segment offsets over the concatenated reduced sets.  The number of pairs is a triangular number, so the sizes
    are: two sets, the longest lists of at most 255 and at most 256 C pairs, the shortest one past 256 C pairs, and the
    shortest one of five trips and a partial one."""
    import setops_ref as R
    import test_gpu_setops as SO
    from gtars.models import RegionSetList

    rng = np.random.default_rng(83)
    regs = [SO._random_set(rng, 60, ["p", "q", "r"], "all" if k % 7 == 3 else None) if k != 5 else [] for k in range(160)]
    red = [R.reduce(r) for r in regs]
    clean, pairs_of = 0, []  # pairs_of[k]: the pairs of clean sets among the first k sets
    for r in red:
        pairs_of.append(clean * (clean - 1) // 2)
        clean += all(s <= e for _, s, e in r)
    per = 256 * cap.c
    small, fits = (max(k for k in range(2, 160) if pairs_of[k] <= top) for top in (255, per))
    past, many = (min(k for k in range(2, 160) if pairs_of[k] >= low) for low in (per + 1, 5 * per + 131))
    assert 0 < pairs_of[fits] <= per < pairs_of[past] < per + 64 and 5 * per < pairs_of[many]
    for k in sorted({2, small, fits, past, many}):
        assert k != many or sum(len(r) for r in red[:k]) > 5 * per  # (k_widths: a reduced row per lane)
        with cap.run(pairs_of[k] > per, "regionset_pairwise_jaccard"):
            assert RegionSetList([SO._rs(r) for r in regs[:k]]).pairwise_jaccard() == R.pairwise_jaccard(regs[:k])


# ---- csrc/setops.hip: structure and statistics -------------------------------------------------------------------------------
def test_structure_and_statistics(cap):
    import genomicdist_ref as G
    import test_gpu_genomicdist as GD
    from gtars.genomic_distributions import consensus

    calls = ("regionset_disjoin", "regionset_gaps", "regionset_neighbor_distances", "regionset_nearest_neighbors",
             "regionset_distribution", "regionset_chromosome_statistics")
    for n in cap.sizes():
        rng = np.random.default_rng(5000 + n)
        a = GD._random_set(rng, n)[:n]
        A = GD._rs(a)
        with cap.run(cap.clips(n), *calls):
            assert GD._tuples(A.disjoin()) == G.disjoin(a)
            assert GD._tuples(A.gaps(GD.SIZES)) == G.gaps(a, GD.SIZES)
            assert A.neighbor_distances() == G.neighbor_distances(a)
            assert A.nearest_neighbors() == G.nearest_neighbors(a)
            for n_bins in (250, 7):
                assert A.distribution(n_bins) == G.distribution(a, n_bins)
                assert A.distribution(n_bins, GD.SIZES) == G.distribution(a, n_bins, GD.SIZES)
            assert GD._stats(A) == G.chromosome_statistics(a)
        sets = [GD._random_set(rng, max(n // 3, 1), GD.NAMES[: 3 + k % 5])[: max(n // 3, 1)] for k in range(4)] + [[]]
        sets[0] = a  # (k_fill: one launch per set, this one past the cap)
        want = [{"chr": c, "start": s, "end": e, "count": k} for c, s, e, k in G.consensus(sets)]
        with cap.run(cap.clips(n), "regionset_consensus"):
            assert consensus([GD._rs(s) for s in sets]) == want


def test_gaps_and_bins_of_sets_that_stay_large_when_reduced(cap):
    """both forms of k_gaps walk the REDUCED set, k_lookup the gaps found, k_rle_counts the occupied bins of a distribution:
    the random sets of the test above merge into a few hundred rows, a hundred gaps and a dozen bins.  Here no two regions
    touch, every chromosome but one (of size 0) has room for the gaps between them, one is cut short by its size, one has a
    size and no region; and with bins of one base every region's midpoint has a bin of its own."""
    import genomicdist_ref as G
    import setops_ref as R
    import test_gpu_genomicdist as GD

    names = ["chr2", "chr10", "1", "chr1", "chrM", "chrX", "chrUn"]  # (chrUn has no size: its regions are left out)
    for n in cap.sizes()[:4] + [10 * 256 * cap.c + 131]:
        rng = np.random.default_rng(5500 + n)
        a = _disjoint(rng, n, names)
        sizes = {"chr2": 40 * n, "chrY": 99, "chr10": GD.TOP, "1": 30 * n, "chrX": 0, "chr1": 20 * n + 10, "chrM": 7 * n}
        sizes_b = dict(sizes, chr10=40 * n)  # (bins of one base: the longest chromosome has as many bases as there are bins)
        want, bins, bins_b = G.gaps(a, sizes), G.distribution(a, 20 * n + 10), G.distribution(a, 40 * n, sizes_b)
        if n > 5 * 256 * cap.c:
            assert len(R.reduce(a)) == n == len(bins) and min(len(want), len(bins_b)) > 5 * 256 * cap.c
        A = GD._rs(a)
        with cap.run(cap.clips(n), "regionset_gaps", "regionset_distribution"):
            assert GD._tuples(A.gaps(sizes)) == want
            assert A.distribution(20 * n + 10) == bins
            assert A.distribution(40 * n, sizes_b) == bins_b


def test_statistics_of_many_chromosomes(cap):
    """k_stat_finish: one lane per chromosome; chromosomes of one, two and three regions, so that count, mean and both forms of
    the median are per-lane values in every trip"""
    import genomicdist_ref as G
    import test_gpu_genomicdist as GD

    for n_rank in cap.sizes():
        names = _names(n_rank)
        rng = np.random.default_rng(8400 + n_rank)
        a = [(name, int(s), int(s) + int(w)) for k, name in enumerate(names)
             for s, w in zip(rng.integers(0, 1000, 1 + k % 3), rng.integers(0, 500, 1 + k % 3))]
        random.Random(84).shuffle(a)
        with cap.run(cap.clips(n_rank), "regionset_chromosome_statistics"):
            assert GD._stats(GD._rs(a)) == G.chromosome_statistics(a)


# ---- csrc/setops.hip: the folds over a list of sets --------------------------------------------------------------------------
def test_folds_over_a_list_of_sets(cap):
    import setlist_ref as L
    import setops_ref as R
    import test_gpu_setlist as SL
    import test_gpu_setops as SO

    calls = ("regionset_list_bulk_union_except", "regionset_list_union_all", "regionset_list_intersect_all",
             "regionset_list_union_except")
    for n in cap.sizes():
        rng = np.random.default_rng(6000 + n)
        cuts = [n // 4, n // 2, 3 * n // 4]
        rows = SO._exactly(rng, n, SO.NAMES_A, "all" if n % 2 else None)
        sets = [rows[lo:hi] for lo, hi in zip([0] + cuts, cuts + [n])]
        # (union_except leaves a quarter of the rows out: at 256 C + 1 rows what is left fits the capped grid)
        with cap.run(cap.clips(n), *(calls if n > 2 * 256 * cap.c else calls[:3])):
            SL._check_all_four(sets, every_skip=False)
    # intersect_all's events (k_ia_events) are those of the REDUCED sets and k_ue_finish walks the rows of all the unions;
    # the random rows above merge into fewer than 256 C.  Four sets that keep every row: one, and three shifted copies of it,
    # so that all four have the last bases of every region in common and every union is about as long as one set.
    rng = np.random.default_rng(6999)
    base = _disjoint(rng, n // 4 + 1, SO.NAMES_A, (4, 9))
    sets = [[(c, s + k, e + k) for c, s, e in base] for k in range(4)]
    want = L.bulk_union_except(sets)
    assert sum(len(R.reduce(s)) for s in sets) > 5 * 256 * cap.c  # k_ia_events
    assert len(want[0]) + sum(len(u) for u in want[1]) > 5 * 256 * cap.c  # k_ue_finish
    assert len(L.intersect_all(sets)) == len(base)
    with cap.run(True, *calls):
        SL._check_all_four(sets, want=want, every_skip=False)


def test_bulk_union_except_of_many_sets(cap):
    """k_ue_slices: one lane per output of bulk_union_except (a union per set left out, and the union of all), plus one.
    Lists of n sets, nearly all of them empty; the few with regions sit where the trips meet, so that the unions without
    them -- other rows than their neighbours' -- are the slices of a later trip's first and last lanes."""
    import setlist_ref as L
    import test_gpu_setlist as SL

    per = 256 * cap.c
    for n in cap.sizes():
        rng = np.random.default_rng(6500 + n)
        sets = [[] for _ in range(n)]
        for at in sorted({k for k in (0, 254, 255, per - 2, per - 1, per, per + 1, 3 * per + 9, n - 2, n - 1) if 0 <= k < n}):
            sets[at] = _disjoint(rng, 3, ["chr1", "chr2"])
        if n < 2:
            continue  # (a list of one set has no union without it; the sizes from 255 on do)
        want = L.bulk_union_except(sets)
        rsl = SL._rsl(sets)
        with cap.run(n + 2 > per, "regionset_list_bulk_union_except"):  # (n + 2 slices: n + 1 outputs and the end of the last)
            got_full, got_ex = rsl.bulk_union_except()
        assert SL._plain(got_full) == want[0] and [SL._tuples(g) for g in got_ex] == want[1]
        assert len({tuple(u) for u in want[1]}) >= 3  # the unions without a set that has regions differ from the others


# ---- csrc/cov_tile.h: the coverage tile launcher ---------------------------------------------------------------------------------
# Its grid is one workgroup per tile up to 8 per CU, so a workgroup walks a second tile of its span only past 8 million
# positions.  Under the cap a track of 7 tiles + 11 positions is one span of 8 tiles (C = 1) or spans of 3, 3 and 2 tiles, the
# last one ragged (C = 3): the carry across tiles, the re-zeroed LDS tile and the event cursors that run on from tile to tile.
# (Neither file takes its geometry from grid_for / stream_grid: no COVERED entries.)
def test_coverage_tracks_of_several_tiles_per_workgroup(cap):
    """K11, all three kinds: the events of test_events_on_tile_boundaries; then 3,000 equal positions in tile 4, the second
    tile of its span under both caps, which the core track enters with a non-zero count and which takes twelve rounds of
    256 events"""
    import test_gpu_uniwig as UW

    tile, first = UW.TILE, 5
    chrom_size = first + 7 * tile + 11
    edges = []
    for k in (0, 1, 2, 5):
        edges += [first + k * tile, first + (k + 1) * tile - 1, first + (k + 1) * tile]
    start = np.array([e - 1 for e in edges], dtype=np.uint32)
    for m in (0, 3):
        p = sorted({e + m for e in edges} | {e - m - 1 for e in edges if e - m - 1 > first + m} | {first + m})
        p = np.array(p + p[:4], dtype=np.uint32)
        with cap.run(True, "uniwig_counts"):
            UW._check_tracks_vs_restatement(p - np.uint32(1), p + np.uint32(tile), chrom_size, m)
            for width in (1, tile - 1, tile, tile + 1):
                UW._check_tracks_vs_restatement(start, start + np.uint32(width), chrom_size, m)
        # the pile-up opens on the second position of the core track's tile 4 and closes 49 positions on (start and end track:
        # windows of 2 m + 1 inside their tile 4); one long row covers tiles 3 .. 5, so the core track enters tile 4 with 1
        t4 = first + 4 * tile
        s = np.concatenate([start, [t4 - tile + 7], np.full(3000, t4, dtype=np.uint32)]).astype(np.uint32)
        e = np.concatenate([start + np.uint32(9), [t4 + tile + 9], np.full(3000, t4 + 50, dtype=np.uint32)]).astype(np.uint32)
        assert int((s + 1 < t4).sum()) - int((e < t4).sum()) > 0  # the core track's count in front of tile 4
        with cap.run(True, "uniwig_counts"):
            UW._check_tracks_vs_restatement(s, e, chrom_size, m)


def test_streamed_tracks_of_several_tiles_per_workgroup(cap):
    """K24, kinds core and start: one segment of 7 tiles + 11 compacted positions with a pile of rows inside it and 300 rows
    of mixed scores that open on one position of tile 4; then, with one workgroup, device windows of two tiles, each
    entered with the count that the prefix columns give"""
    import random as _random

    import test_gpu_uniwig_stream as SW

    tile = SW.TILE
    rng = _random.Random(24)
    rows = [("chr1", 0, 7 * tile + 12, 2)] + SW._pile(rng, 400, 1, 7 * tile - 50, 45)
    rows += [("chr1", 4 * tile + 50, 4 * tile + 60 + rng.randrange(0, 30), rng.choice([1, 2, 3, 0, 1000, 65536])) for _ in range(300)]
    rows = sorted(rows, key=lambda r: r[1]) + [("chr2", 7, 20, 1)]
    # core: the long row's window is [1, 7 * tile + 11]; start (windows of 7 positions): dense up to chr1's size
    for kind, m, max_gap, sizes in (("core", 0, 0, None), ("start", 3, -1, {"chr1": 7 * tile + 11})):
        with cap.run(True, "uniwig_stream"):
            track, want = SW.check(rows, m, 1, kind, max_gap, sizes)
            if cap.c == 1:
                SW.check(rows, m, 1, kind, max_gap, sizes, max_device_bytes=2 * tile * 4)
        assert track.seg_len.tolist()[0] == 7 * tile + 11 and track.seg_first.tolist()[0] == 1
        at = 4 * tile + 50 - m  # the compacted index (position - 1) on which the 300 rows open
        assert 4 * tile <= at < 5 * tile and want[at][2] - want[at - 1][2] > 1000


# ---- csrc/annot.hip ------------------------------------------------------------------------------------------------------------
def test_tss_distances(cap, monkeypatch):
    """both forms of k_tss_dist on one index: the LDS table of the staged form is filled once per workgroup, before the loop"""
    import annot_ref as A
    import test_gpu_annot as AN
    from gtars.models import TssIndex

    names = ["chr1", "chr2", "chrX", "chrQ"]
    for n in cap.sizes():
        rng = np.random.default_rng(7000 + n)
        index = AN._tuples(*AN._random_regs(rng, n, names[:3], 50_000, (0, 3)))
        queries = AN._tuples(*AN._random_regs(rng, n, names, 52_000))
        tss = TssIndex.from_regionset(AN._rs(index))  # (its device image, and so k_midpoints, comes with the first query call)
        want_abs, want_signed = A.distances(A.build_index(index), queries)
        q = AN._rs(queries)
        for form in (None, "1"):
            if form:
                monkeypatch.setenv("GTARS_TSS_GLOBAL_SEARCH", form)
            with cap.run(cap.clips(n), "tss_index_distances"):
                assert tss.calc_tss_distances(q) == want_abs, form
                assert tss.feature_distances(q) == want_signed, form
        monkeypatch.delenv("GTARS_TSS_GLOBAL_SEARCH")


# ---- csrc/signal.hip -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cond", [1, 3, 65])
def test_signal_summary(cap, n_cond):
    """k_signal_fold: 256 / G result rows per workgroup, G = 1, 4 and 64 lanes per row for 1, 3 and 65 conditions.  One query
    per matrix row, so the result rows are the queries; a stack of SPLIT_HITS + 1 rows, folded by the whole workgroup, is hit
    by a query of the last trip."""
    import test_gpu_signal as SG
    from gtars.signal import SPLIT_HITS

    group = 1 if n_cond == 1 else 4 if n_cond == 3 else 64
    for n in sorted(set(cap.sizes(256 // group) + cap.sizes()[3:])):
        rng = np.random.default_rng(8000 + n)
        values = SG._special(rng.normal(0, 3, (n + SPLIT_HITS + 1, n_cond)), rng)
        chrs, starts, ends, _ = SG._columns(values[:n])
        top = int(ends[-1]) + 100
        chrs = chrs + ["chr1"] * (SPLIT_HITS + 1)
        starts = np.concatenate([starts, top + rng.integers(0, 40, SPLIT_HITS + 1).astype(np.uint32)])
        ends = np.concatenate([ends, top + 50 + rng.integers(0, 40, SPLIT_HITS + 1).astype(np.uint32)])
        qchrs, qs, qe = ["chr1"] * (n + 1), np.concatenate([starts[:n], [top + 45]]), np.concatenate([ends[:n], [top + 46]])
        qchrs[n // 2] = "zz"  # (a query without a row in the result: flags and rows differ from then on)
        with cap.run(n > (256 // group) * cap.c, "signal_summary"):
            got_q, _, _ = SG._check(chrs, starts, ends, values, qchrs, qs.astype(np.uint32), qe.astype(np.uint32))
        assert len(got_q) == n and got_q[-1] == n


# ---- csrc/seqstats.hip -----------------------------------------------------------------------------------------------------------
from test_gpu_seqstats import genomes, lane_settings  # noqa: E402,F401  (module-scoped assembly: FASTA and .fab)


def test_gc_and_dinucleotide_counts(cap, genomes, lane_settings):  # noqa: F811
    """k_seq_pieces: a row per lane.  k_seq_count: a 4-KiB piece per lane group, 16 (GTARS_SEQ_LANES=16) or 4 (=64) pieces per
    workgroup; rows of several pieces whose pieces fall into different trips add into one output row."""
    import test_gpu_seqstats as SQ
    from gtars_amd.seqstats import SEQ_PIECE as PIECE

    for n in cap.sizes():
        rng = random.Random(9000 + n)
        rows = []
        for k in range(n):
            name, length = (SQ.MID, 100_003) if rng.random() < 0.5 else (SQ.LONG, 2_000_000)
            w = rng.choice([0, 1, 17, 300, PIECE - 1, PIECE, 3 * PIECE + 5]) if k % 4 else 19 * PIECE + 7
            s = rng.randint(0, length - w)
            rows.append((name, s, s + w))
        with cap.run(cap.clips(n), "seqstats_gc", "seqstats_dinucl"):
            SQ._check(genomes, rows, lane_settings)
    # few rows, many pieces: only k_seq_count clips (16 C and 4 C pieces per trip); one row alone spans five trips of either
    rows = [(SQ.LONG, 9, 9 + (5 * 16 * cap.c + 9) * PIECE + 5), (SQ.MID, 3, 3 + 2 * PIECE), (SQ.MID, 0, 5)]
    assert rows[0][2] < 2_000_000
    with cap.run(True, "seqstats_gc", "seqstats_dinucl"):
        SQ._check(genomes, rows, lane_settings)


# ---- csrc/countmat.hip -----------------------------------------------------------------------------------------------------------
def test_count_matrix(cap):
    """ragged queries whose (row, peak) pairs repeat, at every size; then one hit per query with a run of eight equal pairs
    across the seam of the first two trips of the sorted hits"""
    import test_gpu_countmat as CM

    n_rows, n_cols = 40, 911
    for n in cap.sizes():
        rng = np.random.default_rng(10_000 + n)
        off = CM.ragged(n, rng)  # about n / 2 queries; few cells, so that pairs repeat; some hits and queries dropped
        ids = rng.integers(0, max(n // 12, 1), n)
        ids[rng.random(n) < 0.03] = n_cols + 1
        row = rng.integers(0, 6, len(off) - 1)
        row[rng.random(len(row)) < 0.03] = n_rows
        with cap.run(cap.clips(n), "count_matrix_csr_device"):
            CM.check(off, ids, row, n_rows, n_cols)
    # one hit per query: the run of equal pairs as built above, pair for pair
    n = 5 * 256 * cap.c + 131
    rng = np.random.default_rng(10_500)
    cells = np.sort(rng.choice(n_rows * n_cols, n, replace=False))
    seam = 256 * cap.c
    cells[seam - 4:seam + 4] = cells[seam - 4]
    cells = cells[rng.permutation(n)]
    with cap.run(True, "count_matrix_csr_device"):
        got = CM.check(np.arange(n + 1, dtype=np.uint64), cells % n_cols, cells // n_cols, n_rows, n_cols)
    assert got[3] == n - 7 and sorted(got[2].tolist())[-1] == 8


# ---- csrc/partitions.hip ---------------------------------------------------------------------------------------------------------
def test_partitions(cap):
    """k_partitions keeps a workgroup's sums in an LDS table that is zeroed once and flushed once, around the whole loop: a
    later trip adds to what the earlier ones left.  Both forms (priority assignment and bp) on free-form partitions."""
    import test_gpu_partitions as PT

    for n in cap.sizes():
        rng = np.random.default_rng(11_000 + n)

        def regs(k, names):
            s = rng.integers(0, 3000, k)
            w = rng.choice([-40, 0, 0, 5, 60, 400], k)
            return [(str(c), int(a), int(max(a + b, 0))) for c, a, b in zip(rng.choice(names, k), s, w)]

        sets = [regs(60, ["chr1", "chr2"]), regs(5, ["chr2"]), [], regs(200, ["chr1", "chr2", "chr3"])]
        with cap.run(cap.clips(n), "partitions_count"):
            PT._check_free(sets, regs(n, ["chr1", "chr2", "chr3", "chr4"]))


# ---- csrc/tokbatch.hip ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tok_world(tmp_path_factory):
    import test_gpu_tokbatch as TB

    return TB._world(TB._write_universe(tmp_path_factory.mktemp("grid_cap_tok") / "universe.bed"))


def test_batched_tokenizer(cap, tok_world):
    """n sets of 0 .. 8 ids: k_set_lengths and k_set_offsets a set per lane, k_set_pack gtars_debug_tokbatch_tile() ids per
    workgroup step (its LDS offsets are staged anew for every tile), k_set_pad a cell per lane"""
    import test_gpu_tokbatch as TB
    from gtars_amd._lib import lib

    tile = int(lib.gtars_debug_tokbatch_tile())
    for n in cap.sizes():
        rng = np.random.RandomState(n)
        lengths = rng.randint(0, 9, size=n)
        lengths[[0, n // 2, n - 1]] = 0  # (empty sets: the ids are packed, not left where the tokenizer wrote them)
        batch = TB.batch_of(TB.sets_with_lengths(lengths.tolist(), seed=n + 1))
        with cap.run(cap.clips(n), "tokenizer_encode_sets_ids", "tokenizer_encode_sets_padded"):
            want = TB.check_ragged(tok_world, batch)
            TB.check_ragged(tok_world, batch, max_length=3)
            TB.check_padded(tok_world, batch, want, side="left" if n % 2 else "right")
        if n == cap.sizes()[-1]:
            assert sum(len(r) for r in want) > 5 * tile * cap.c, "k_set_pack must walk more than five tiles per workgroup"


# ---- csrc/refget.hip, csrc/byte_csr.h ----------------------------------------------------------------------------------------------
def _refget_records(n, late):
    """n records of 0 .. 199 bytes under distinct names; the record at index `late` (behind the first trip) is 300 bytes long:
    with GTARS_REFGET_HOST_LEN = 200 it is the one row of the host tail"""
    rng = random.Random(2100 + n)
    letters = [b"ACGT", b"ACGTacgt", b"ACGTN", b"ACGTRYKM", b"acgtn", b"MEFILPQX*"]
    recs = []
    for k in range(n):
        size = rng.choice([0, 1, 15, 16, 17, rng.randrange(0, 120), rng.randrange(60, 200), rng.randrange(60, 200)])
        recs.append((f"r{k}", bytes(rng.choice(rng.choice(letters)) for _ in range(300 if k == late else size))))
    return recs


def test_refget_digests_and_substrings(cap, tmp_path, monkeypatch):
    import gtars_amd.refget as G
    import refget_ref as R
    from test_gpu_refget import _fasta_text
    from test_refget_cpu import check_collection

    monkeypatch.setenv("GTARS_REFGET_HOST_LEN", "200")
    for n in cap.sizes():
        late = 256 * cap.c + 3 if n > 256 * cap.c + 3 else n - 1
        text = _fasta_text(_refget_records(n, late))
        path = tmp_path / f"n{n}.fa"
        path.write_bytes(text)
        want = R.walk_fasta(text)
        assert want[late]["length"] == 300 and sum(w["length"] > 200 for w in want) == 1
        with cap.run(cap.clips(n - 1), "seqcol_from_fasta"):  # (the file call's image holds the n - 1 records of the device's share)
            col = G.load_fasta(str(path))
        check_collection(col, want, True)
        with cap.run(cap.clips(n), "seqcol_digest_records"):  # (the collection's full image: the long row comes back as a list)
            text_d, md5, cls = G.digest_records(col)
            assert (text_d, md5, cls.tolist()) == ([w["sha512t24u"] for w in want], [w["md5"] for w in want], [w["alphabet"] for w in want])
        # a row per record: whole, a slice, empty; failing rows (an unknown name, end < start, past the end) between them, in every trip
        store = G.RefgetStore.in_memory()
        meta, _ = store.add_sequence_collection_from_fasta(str(path))
        rows = []
        for k, w in enumerate(want):
            size = w["length"]
            rows.append([(w["name"], 0, size), (w["name"], size // 3, size - size // 4), (w["name"], 0, size), ("nope", 0, 3),
                         (w["name"], 0, size), (w["name"], 9, 3), (w["name"], size, size + 1), (w["name"], 0, 0)][k % 8 if k != late else 0])
        expect = R.region_substrings(want, *zip(*rows))
        with cap.run(cap.clips(n), "seqcol_substrings"):
            got, status = G.substrings_many(store, meta.digest, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], with_status=True)
        assert status.tolist() == [st for st, _ in expect]
        assert got == [b.decode() if st == 0 else None for st, b in expect]
        if n > 256 * cap.c:
            assert {st for st, _ in expect} == {0, 1, 2} and expect[late] == (0, want[late]["sequence"])
        if n == cap.sizes()[-1]:
            assert sum(len(b) for _, b in expect) > 5 * 2048 * cap.c, "k_csr_fill writes 2,048 bytes per workgroup and trip"


# ---- csrc/vrs.hip ------------------------------------------------------------------------------------------------------------------
from test_gpu_vrs import world as vrs_world  # noqa: E402,F401  (module-scoped: the 0.6-MB assembly as FASTA and .fab)


def _vrs_rows(seqs, where, n, seed):
    import test_gpu_vrs as VR

    good, failing = VR._kinds(seqs)
    rows = (VR._repeat_rows(where, seqs) + good + failing)[:n]
    big, rng = seqs["big"], random.Random(seed)
    while len(rows) < n:
        at = rng.randrange(0, VR.BIG_N - 40)
        kind = rng.random()
        if kind < 0.5:
            rows.append(("big", at) + VR._mnv(big, at, rng.choice([1, 1, 2, 9]), rng))
        elif kind < 0.7:
            rows.append(("big", at, big[at:at + 1], big[at:at + 1] + bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 5)))))
        elif kind < 0.9:
            rows.append(("big", at, big[at:at + rng.randint(2, 30)], big[at:at + 1]))
        else:
            rows.append(rng.choice(failing))
    rng.shuffle(rows)
    return rows


def test_vrs_alleles(cap, vrs_world):  # noqa: F811
    import test_gpu_vrs as VR

    seqs, where, _, _ = vrs_world
    for n in cap.sizes():
        rows = _vrs_rows(seqs, where, n, 1800 + n)
        with cap.run(cap.clips(n), "vrs_alleles"):
            st = VR._check(vrs_world, rows)[0]
        assert len(st) == n and (n < 300 or len(set(st)) > 3)


def test_vrs_long_rolls(cap, vrs_world, monkeypatch):  # noqa: F811
    """k_vrs_roll_long: a wave per entry of the work list, four entries per workgroup.  With the lane path's roll cut at 8 bases,
    insertions into the 1,300-base and the 1,501-base repeat leave two entries each: more than five trips' worth."""
    import test_gpu_vrs as VR

    seqs, where, _, _ = vrs_world
    monkeypatch.setenv("GTARS_VRS_ROLL_CAP", str(VR.CAP))
    every = []
    for k in range(6 * cap.c + 3):
        for name, unit in (("long", b"T"), ("longtri", b"GAT")):
            every.append(("big", where[name][0] + 40 + 29 * k, b"", unit))
    assert 2 * len(every) > 5 * 4 * cap.c
    at, size, _ = where["long"]
    # the work list has two slots per allele and the grid is sized by the slots: 1, 2 C (the slots fit the capped grid),
    # 2 C + 1 (a second trip of two slots) and all the alleles (more than five trips)
    for n in (1, 2 * cap.c, 2 * cap.c + 1, len(every)):
        rows = every[:n]
        with cap.run(2 * n > 4 * cap.c, "vrs_alleles"):
            st, ns, ne, _, _ = VR._check(vrs_world, rows)
        assert set(st) == {VR.R.OK}
        assert {(a, b) for r, a, b in zip(rows, ns, ne) if r[3] == b"T"} == {(at, at + size)}  # every roll ran to both ends of the repeat


# ---- csrc/reftx.hip ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tx_world(tmp_path_factory):
    import reftx_ref as R
    import test_gpu_reftx as TX
    from gtars_amd.seqstats import GenomeAssembly
    from test_vrs_cpu import write_fasta

    d = tmp_path_factory.mktemp("grid_cap_tx")
    write_fasta(d / "asm.fa", TX.SEQS, width=61)
    return GenomeAssembly(str(d / "asm.fa")), R.digest_bytes(R.refget_digests(TX.SEQS)["c1"])


def test_transcript_mapping_and_sequences(cap, tx_world):
    """k_tx_map a query per lane; k_tx_rows and k_tx_digest a transcript per lane (the mature sequences of EVERY transcript of a
    store of n), the fill of their bytes 2,048 per workgroup"""
    import reftx_ref as R
    import test_gpu_reftx as TX
    from gtars_amd import reftx as T
    from test_reftx_cpu import build_store, random_queries, random_transcript

    genome, c1 = tx_world
    for n in cap.sizes():
        rng = random.Random(1900 + n)
        txs = [random_transcript(rng, f"NM_G{k}.1", c1, rng.choice([60, 400, 5000])) for k in range(n)]
        store = build_store(txs)
        rows = random_queries(rng, txs, n)
        bound = T.BoundTxStore(genome, store)
        with cap.run(cap.clips(n), "txbind_map"):
            out, status = bound.map(store.indices_of([r[0] for r in rows]), ["cng".index(r[1]) for r in rows], [r[2] for r in rows],
                                    [r[3] for r in rows], [1 if r[4] else 0 for r in rows])
        assert (out.tolist(), status.tolist()) == R.map_rows(txs, rows)
        order = [R.lookup(txs, store.transcript(i).accession) for i in range(len(store))]
        want = [R.mature(TX.SEQS, tx) for tx in order]
        with cap.run(cap.clips(n), "txbind_sequences"):
            TX._check_sequences(genome, store, order, want)


# ---- csrc/hgvs.hip -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hgvs_world(tmp_path_factory):
    """one random world, 4,001 expressions and the restatement's rows for them, computed once"""
    import hgvs_ref as HR
    from gtars_amd.reftx import BoundTxStore
    from test_hgvs_cpu import make_world, random_strings

    genome, store, seqs, txs, accessions, aliases, rng = make_world(tmp_path_factory.mktemp("grid_cap_hgvs"), 27)
    strings = random_strings(rng, seqs, txs, 4001, aliases)
    return genome, BoundTxStore(genome, store), seqs, accessions, aliases, strings, HR.bridge(seqs, accessions, txs, strings, aliases)


def test_hgvs_bridge(cap, hgvs_world):
    from gtars_amd import hgvs as H
    from test_hgvs_cpu import check_batch

    genome, bound, seqs, accessions, aliases, strings, want = hgvs_world
    for n in cap.sizes():
        assert n <= len(strings)
        with cap.run(cap.clips(n), "hgvs_to_vrs"):
            got = H.hgvs_to_vrs_ids(genome, bound, strings[-n:], accessions=accessions, aliases=aliases)
        check_batch(got, want[-n:], seqs, n)
        assert n < 300 or len({w["status"] for w in want[-n:]}) > 6


# ---- csrc/bam.hip --------------------------------------------------------------------------------------------------------------------
def test_bam_columns_and_qc(cap, tmp_path):
    """records of one chromosome are one launch each of the QC's kernels: single-end files of every size; one paired file whose
    read-1 table, and so the join, is past five trips, with the paired cases of test_gpu_bam.py in front and a run of
    mitochondrial records (classified by a launch of their own) behind"""
    import bam_ref as R
    import test_gpu_bam as BM

    for n in cap.sizes():
        recs = BM.single(n)
        for i in range(0, n, 5):  # some keys twice
            recs[i]["pos"] = recs[max(i - 1, 0)]["pos"]
        with cap.run(cap.clips(n), "bam_qc", "bam_decode"):
            want = BM.check(tmp_path, BM.REFS, BM.coordinate_sorted(recs), name=f"s{n}.bam")
        assert want["total_reads"] == n
    pairs = 5 * 256 * cap.c + 131
    rng = random.Random(17)
    recs = BM.paired_records()
    for k in range(pairs):
        p1 = 6000 + rng.randrange(0, 2000)  # (few positions: many pairs share a four-tuple)
        recs += BM.pair(b"g%05d" % k, p1, p1 + rng.choice([100, 150]), tlen=rng.choice([160, -160]))
    recs += [R.rec(ref_id=2, pos=10 + i // 3, name=b"m%04d" % i) for i in range(256 * cap.c + 37)]
    with cap.run(True, "bam_qc", "bam_decode"):
        want = BM.check(tmp_path, BM.REFS, BM.coordinate_sorted(recs), name="paired.bam")
    assert want["mito_reads"] >= 256 * cap.c + 37 and want["m2"] > 0


# ---- csrc/kernels.hip: the engine -----------------------------------------------------------------------------------------------------
UNK = 0xFFFFFFFF


def _universe(rng, n, n_chrom, span, nested):
    c = rng.integers(0, n_chrom, n).astype(np.uint32)
    s = rng.integers(0, span, n).astype(np.uint32)
    w = np.where(rng.random(n) < (0.03 if nested else 0.0), rng.integers(5_000, 60_000, n), rng.integers(100, 900, n))
    return c, s, (s + w).astype(np.uint32)


def _queries(rng, nq, n_chrom, span):
    qc = rng.integers(0, n_chrom + 1, nq).astype(np.uint32)
    qc[qc == n_chrom] = UNK
    qs = rng.integers(0, span + 5_000, nq).astype(np.uint32)
    qe = (qs + np.where(rng.random(nq) < 0.05, rng.integers(2_000, 9_000, nq), rng.integers(0, 900, nq))).astype(np.uint32)
    return qc, qs, qe


def _same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert np.asarray(a).tolist() == np.asarray(b).tolist()


@pytest.mark.parametrize("kind", [0, 1], ids=["bits", "ailist"])
def test_overlap_index_generic_kernels(cap, monkeypatch, kind):
    """GTARS_NO_LDS_PATH=1: count / any / find_overlaps / find_overlap_indices on the one-thread-per-query kernels (k_count,
    k_fill, k_sort_unique_segments), with and without a minimum overlap; Bits::count (k_bits_count) whatever the path"""
    import gtars_amd
    import oracle

    rng = np.random.default_rng(300 + kind)
    n_chrom, span = 3, 400_000
    c, s, e = _universe(rng, 3000, n_chrom, span, nested=False)
    s[100:140], e[100:140], c[100:140] = s[100], e[100], c[100]  # forty copies of one interval
    src = rng.integers(0, 900, len(c)).astype(np.uint32)  # source rows named many times: sort + unique shortens segments
    g, o = gtars_amd.OverlapIndex(c, s, e, src, n_chrom=n_chrom, kind=kind), oracle.Index(c, s, e, src, n_chrom=n_chrom, kind=kind)
    monkeypatch.setenv("GTARS_NO_LDS_PATH", "1")
    for nq in cap.sizes():
        qc, qs, qe = _queries(rng, nq, n_chrom, span)
        qs[-1], qe[-1], qc[-1] = s[100], e[100], c[100]  # the last query of the last trip: the forty copies
        if kind == 0:
            with cap.run(cap.clips(nq), "bits_count"):
                assert g.bits_count(qc, qs, qe).tolist() == [o.bits_count(int(a), int(b), int(d)) if a != UNK else 0 for a, b, d in zip(qc, qs, qe)]
        for mo in (None, 30):
            with cap.run(cap.clips(nq), "count_overlaps", "any_overlaps", "find_overlaps", "find_overlap_indices"):
                assert g.count_overlaps(qc, qs, qe, mo).tolist() == o.count_overlaps(qc, qs, qe, mo).tolist(), (nq, mo)
                assert g.any_overlaps(qc, qs, qe, mo).tolist() == o.any_overlaps(qc, qs, qe, mo).tolist(), (nq, mo)
                _same(g.find_overlaps(qc, qs, qe, mo), o.find_overlaps_regions(qc, qs, qe, mo))
                got = g.find_overlap_indices(qc, qs, qe, mo)
            off, _, _, vals = o.find_overlaps_regions(qc, qs, qe, mo)  # sorted unique values per query
            uniq = [np.unique(vals[int(off[q]):int(off[q + 1])]) for q in range(nq)]
            assert got[0].tolist() == np.concatenate([[0], np.cumsum([len(u) for u in uniq])]).tolist(), (nq, mo)
            assert got[1].tolist() == np.concatenate(uniq).tolist(), (nq, mo)
        assert nq < 300 or max(len(u) for u in uniq) > 24  # (the heap-sort branch of the per-query sort)


def test_nested_ailist_index(cap, monkeypatch):
    """an AIList index with nested sub-lists: the ids of a tokenize come from the flat companion and k_ailist_reorder puts each
    query's into AIList::find order; gtars_mark_overlapped_device carries the companion's marks over to this index's stored
    (sub-list major) order with k_permute_marks, a stored position of the INDEX per lane (its size, 40 times the queries', is
    what clips).  From 255 queries on: a single query need not meet a nested interval."""
    import gtars_amd
    import oracle
    import torch
    from gtars_amd import _lib

    dev = torch.device("cuda", torch.cuda.current_device())
    monkeypatch.setenv("GTARS_AILIST_REORDER_MAX_DEPTH", "1000")
    rng = np.random.default_rng(310)
    n_chrom, span = 3, 1_500_000
    for n in cap.sizes()[1:]:
        c, s, e = _universe(rng, 40 * n, n_chrom, span, nested=True)
        v = rng.permutation(len(c)).astype(np.uint32)
        g, o = gtars_amd.OverlapIndex(c, s, e, v, n_chrom=n_chrom, kind=1), oracle.Index(c, s, e, v, n_chrom=n_chrom, kind=1)
        assert max(len(g.sublist_offsets(ch)) for ch in range(n_chrom)) > 1
        qc, qs, qe = _queries(rng, n, n_chrom, span)
        _lib.lib.gtars_prof_reset()
        _lib.lib.gtars_prof_enable(1)
        try:
            d = [torch.from_numpy(x.view(np.int32)).to(dev) for x in (qc, qs, qe)]
            mark = torch.full(((len(c) + 31) // 32,), -1, dtype=torch.int32, device=dev)  # the call zeroes it
            with cap.run(cap.clips(n), "tokenize"):
                off_g, ids_g = g.tokenize(qc, qs, qe)
            with cap.run(cap.clips(40 * n), "mark_overlapped_device"):
                g.mark_overlapped_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), len(qc), mark.data_ptr(), None,
                                         torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            facts = _lib.prof_read()
        finally:
            _lib.lib.gtars_prof_enable(0)
        assert "k_ailist_reorder" in facts, sorted(facts)
        off_o, ids_o = o.tokenize(qc, qs, qe)
        assert np.array_equal(off_g, off_o) and np.array_equal(ids_g, ids_o)
        bits = np.unpackbits(mark.cpu().numpy().view(np.uint8), bitorder="little")[: len(c)].astype(bool)
        got, base = [], 0
        for ch in range(n_chrom):
            ss, ee, _ = g.stored(ch)  # this index's stored order
            sel = bits[base:base + len(ss)]
            got += [(ch, int(a), int(b)) for a, b in zip(ss[sel], ee[sel])]
            base += len(ss)
        assert sorted(set(got)) == list(zip(*[x.tolist() for x in oracle.mco_subset_by_overlaps(o, qc, qs, qe)]))


def _igd_pair(ga, rng, n, n_files, unique):
    import oracle

    c = rng.integers(0, 2, n).astype(np.uint32)
    s = rng.integers(0, 200_000, n).astype(np.uint32)
    e = (s + rng.integers(1, 2_000, n)).astype(np.uint32)
    f = rng.integers(0, n_files, n).astype(np.uint32)
    v = rng.permutation(n).astype(np.uint32)
    if not unique:
        v[-1] = v[-2]  # the only repeated value, in the last records: k_has_adjacent_equal finds it in its last trip
    g = ga.IgdIndex(c, s, e, f, v, n_chrom=2, n_files=n_files)
    o = oracle.Igd()
    o.add_arrays(c, s, e, v, f)
    o.n_files = n_files
    o.finalize()
    return g, o


@pytest.mark.parametrize("n_files,unique", [(7, True), (7, False), (9000, True)], ids=["lds_bins", "repeated_value", "global_bins"])
def test_igd_small_batches(cap, n_files, unique):
    """batches below the sweep's crossover go to the one-thread-per-query kernels: k_igd_count (binary and per pair; LDS bins,
    flushed once behind the loop, or global ones past 8,192 files), k_igd_count_per_query and k_igd_fill_pairs (values all
    distinct or not: the database's values are looked at by k_has_adjacent_equal, a record per lane)"""
    import gtars_amd

    rng = np.random.default_rng(320 + n_files)
    g, o = _igd_pair(gtars_amd, rng, 5 * 256 * cap.c + 131, n_files, unique)
    for nq in cap.sizes():
        qc = rng.integers(0, 2, nq).astype(np.uint32)
        qs = rng.integers(0, 200_000, nq).astype(np.uint32)
        qe = (qs + rng.integers(0, 3_000, nq)).astype(np.uint32)
        for mo in (1, 40):
            with cap.run(cap.clips(nq), "igd_count", "igd_count_per_query", "igd_find_pairs"):
                assert g.count_set_overlaps(qc, qs, qe, mo).tolist() == o.count_set_overlaps(qc, qs, qe, mo, n_files=n_files).tolist(), mo
                assert g.count_region_hits(qc, qs, qe, mo).tolist() == o.count_region_hits(qc, qs, qe, mo, n_files=n_files).tolist(), mo
                assert g.count_overlaps_per_query(qc, qs, qe, mo).tolist() == o.count_overlaps_per_query(qc, qs, qe, mo).tolist(), mo
                _same(g.find_overlaps_regionset(qc, qs, qe, mo), o.find_overlaps_regionset(qc, qs, qe, mo))


def test_histograms(cap):
    """gtars_histogram_u32_device (an id per lane) and gtars_histogram_rows_device (a query per lane: its ids into its barcode's
    row of a band of the matrix) against numpy"""
    import torch
    from gtars_amd._lib import check, lib

    dev = torch.device("cuda", torch.cuda.current_device())
    put = lambda a, dt, view: torch.from_numpy(np.ascontiguousarray(a, dtype=dt).view(view)).to(dev)  # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    n_bins, n_rows, row0 = 97, 13, 4
    for n in cap.sizes():
        rng = np.random.default_rng(330 + n)
        ids = rng.integers(0, n_bins + 3, n).astype(np.uint32)  # (ids past the bins are dropped)
        bins = torch.zeros(n_bins, dtype=torch.int32, device=dev)
        with cap.run(cap.clips(n), "histogram_u32_device"):
            check(lib.gtars_histogram_u32_device(put(ids, np.uint32, np.int32).data_ptr(), n, n_bins, bins.data_ptr(), st))
        torch.cuda.synchronize()
        assert bins.cpu().numpy().tolist() == np.bincount(ids[ids < n_bins], minlength=n_bins).tolist()
        # n queries of 0 .. 4 ids, a barcode row each; rows outside the band [row0, row0 + n_rows) are dropped
        cnt = rng.integers(0, 5, n)
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint64)
        qid = rng.integers(0, n_bins + 3, int(off[-1])).astype(np.uint32)
        row = rng.integers(0, row0 + n_rows + 3, n).astype(np.uint32)
        mat = torch.zeros(n_rows * n_bins, dtype=torch.int32, device=dev)
        d_off, d_row = put(off, np.uint64, np.int64), put(row, np.uint32, np.int32)
        d_ids = put(qid if len(qid) else np.zeros(1, np.uint32), np.uint32, np.int32)
        with cap.run(cap.clips(n), "histogram_rows_device"):
            check(lib.gtars_histogram_rows_device(d_off.data_ptr(), d_ids.data_ptr(), d_row.data_ptr(), n, row0, n_rows, n_bins, mat.data_ptr(), st))
        torch.cuda.synchronize()
        want = np.zeros((n_rows, n_bins), dtype=np.int64)
        for q in range(n):
            r = int(row[q]) - row0
            if 0 <= r < n_rows:
                for i in qid[int(off[q]):int(off[q + 1])]:
                    if i < n_bins:
                        want[r, int(i)] += 1
        assert mat.cpu().numpy().reshape(n_rows, n_bins).tolist() == want.tolist()
