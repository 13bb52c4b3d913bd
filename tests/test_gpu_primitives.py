"""The three device primitives under every index build and set operation, through their test entries
(include/gtars_amd_debug.h), against numpy with exact equality:

* the stable LSD radix sort (csrc/sort.hip, device_sort_perm_ws) against np.lexsort,
* the three-phase u32 -> u64 exclusive scan (csrc/kernels.hip, launch_scan_u32_to_u64) against np.cumsum over uint64,
* the segmented max-scan (csrc/setops.hip, seg_max_pass) against tests/primitives_ref.py.

Sizes sit on the edges of a lane, a wave, a workgroup, a 2048-element tile and a 1024-tile chunk (2^21 elements: the
point from which the single-workgroup middle phase of the scan and of the max-scan loops and carries between chunks);
the sort also runs at 2048 * 8192 + 1, where its digit table passes 2^21 entries and its one-thread-per-element launches
pass 65 536 workgroups.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import primitives_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu


def _L():
    import gtars_amd._lib as L

    return L


def _assert_same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{len(bad)} of {len(want)} differ, first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}")


# ------------------------------------------------------------------------------------------------------------- sort
@pytest.mark.parametrize("n", P.SIZES)
def test_sort_sizes(n):
    rng = np.random.default_rng(100 + n % 1000)
    chrom = rng.integers(0, 5, n, dtype=np.uint64).astype(np.uint32)
    k1 = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    k1[rng.random(n) < 0.5] = 77  # ties: decided by k2, then by the input row
    k2 = rng.integers(0, 3, n, dtype=np.uint64).astype(np.uint32)
    _assert_same(_L().debug_sort_perm(chrom, k1, k2, 5), P.sort_perm_ref(chrom, k1, k2))
    _assert_same(_L().debug_sort_perm(chrom, k1, None, 5), P.sort_perm_ref(chrom, k1))


def test_sort_where_the_digit_table_takes_a_second_scan_chunk():
    n = P.SORT_DIGIT_TABLE_SIZE
    rng = np.random.default_rng(7)
    chrom = rng.integers(0, 3, n, dtype=np.uint64).astype(np.uint32)
    k1 = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    k1[rng.random(n) < 0.3] = 0xFFFFFFFF
    _assert_same(_L().debug_sort_perm(chrom, k1, None, 3), P.sort_perm_ref(chrom, k1))


@pytest.mark.parametrize("with_k2", [False, True])
@pytest.mark.parametrize("n", P.PATTERN_SIZES)
def test_sort_key_patterns(n, with_k2):
    rng = np.random.default_rng(200 + n % 1000)
    chrom = np.zeros(n, dtype=np.uint32)
    ties = rng.integers(0, 4, n, dtype=np.uint64).astype(np.uint32)
    for name, key in P.sort_key_patterns(n, rng).items():
        # the pattern as the major key (k2 breaks its ties) and as the minor key (it breaks k1's ties)
        for k1, k2 in ((key, ties if with_k2 else None), (ties, key)) if with_k2 else ((key, None),):
            try:
                _assert_same(_L().debug_sort_perm(chrom, k1, k2, 1), P.sort_perm_ref(chrom, k1, k2))
            except AssertionError as e:
                raise AssertionError(f"{name}: {e}") from None


@pytest.mark.parametrize("n_chrom", P.N_CHROMS)
@pytest.mark.parametrize("n", P.PATTERN_SIZES)
def test_sort_chromosome_key_widths(n, n_chrom):
    rng = np.random.default_rng(300 + n % 1000 + n_chrom % 97)
    chrom = P.chrom_column(n, n_chrom, rng)
    assert chrom.min() == 0 and chrom.max() == n_chrom - 1
    k1 = rng.integers(0, 50, n, dtype=np.uint64).astype(np.uint32)
    k2 = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    _assert_same(_L().debug_sort_perm(chrom, k1, None, n_chrom), P.sort_perm_ref(chrom, k1))
    _assert_same(_L().debug_sort_perm(chrom, k1, k2, n_chrom), P.sort_perm_ref(chrom, k1, k2))


# ------------------------------------------------------------------------------------------------------------- scan
@pytest.mark.parametrize("n", P.SIZES)
def test_scan_sizes(n):
    rng = np.random.default_rng(400 + n % 1000)
    for hi in (1 << 32, 3):
        counts = rng.integers(0, hi, n, dtype=np.uint64).astype(np.uint32)
        _assert_same(_L().debug_scan_u32(counts), P.scan_ref(counts))


@pytest.mark.parametrize("n", P.PATTERN_SIZES)
def test_scan_count_patterns(n):
    """one_tile_of_3e6 is the case a u32 in-tile prefix gets wrong: 2048 counts of 3 000 000 sum to 6.1e9"""
    rng = np.random.default_rng(500 + n % 1000)
    for name, counts in P.scan_count_patterns(n, rng).items():
        try:
            _assert_same(_L().debug_scan_u32(counts), P.scan_ref(counts))
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from None


# ---------------------------------------------------------------------------------------------------- segmented max
@pytest.mark.parametrize("n", P.SIZES)
def test_seg_max_sizes(n):
    rng = np.random.default_rng(600 + n % 1000)
    seg, val, start = P.seg_patterns(n, rng)["random_segments"]
    _assert_same(_L().debug_seg_max(seg, val, inclusive=True), P.seg_running_max_ref(seg, val))
    for gap in (0, 100, P.M32):
        _assert_same(_L().debug_seg_max(seg, val, start, gap, inclusive=False), P.seg_open_flags_ref(seg, val, start, gap))


@pytest.mark.parametrize("n", P.PATTERN_SIZES)
def test_seg_max_patterns(n):
    rng = np.random.default_rng(700 + n % 1000)
    for name, (seg, val, start) in P.seg_patterns(n, rng).items():
        try:
            _assert_same(_L().debug_seg_max(seg, val, inclusive=True), P.seg_running_max_ref(seg, val))
            for gap in (0, 100, P.M32):
                _assert_same(_L().debug_seg_max(seg, val, start, gap, inclusive=False),
                             P.seg_open_flags_ref(seg, val, start, gap))
        except AssertionError as e:
            raise AssertionError(f"{name}: {e}") from None


def test_seg_max_heads_on_both_chunk_seams():
    """2 * 2^21 + 2049 elements: one segment with its maximum first (no head in 2048 whole tiles, i.e. in two whole
    chunks of tile aggregates), then the same values with heads exactly on 2^21 - 1, 2^21 and 2^22"""
    n = 2 * P.CHUNK + 2049
    rng = np.random.default_rng(8)
    val = rng.integers(0, 1 << 20, n, dtype=np.uint64).astype(np.uint32)
    val[0] = P.M32 - 1
    start = rng.integers(0, (1 << 20) + 300, n, dtype=np.uint64).astype(np.uint32)
    start[::7] = P.M32
    i = np.arange(n)
    for seg in (np.zeros(n, dtype=np.uint32),
                ((i >= P.CHUNK - 1).astype(np.uint32) + (i >= P.CHUNK) + (i >= 2 * P.CHUNK)).astype(np.uint32)):
        _assert_same(_L().debug_seg_max(seg, val, inclusive=True), P.seg_running_max_ref(seg, val))
        for gap in (0, 100, P.M32):
            _assert_same(_L().debug_seg_max(seg, val, start, gap, inclusive=False), P.seg_open_flags_ref(seg, val, start, gap))
