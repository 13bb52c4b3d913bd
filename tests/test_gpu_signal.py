"""calc_summary_signal on the device (K13) against the restatement (tests/signal_ref.py): exact equality on the uint64
views of the result rows and the statistics.  The hits and their order on the reference side come from the oracle's
AIList index."""
import math
from fractions import Fraction

import numpy as np
import pytest

import signal_ref as R

pytestmark = pytest.mark.gpu

NAN = math.nan
LANE_EDGES = [1, 2, 3, 31, 32, 33, 63, 64, 65, 130]  # lane-group and stride edges of the fold kernel
# the reference's nested layout (ailist.rs:550-601): two sub-lists, (0, 30) and (25, 100) in the second
AILIST_26 = [
    (0, 30), (0, 10), (0, 10), (5, 15), (5, 15), (10, 20), (10, 20), (15, 25), (15, 25), (21, 22), (22, 23),
    (20, 30), (20, 30), (25, 100), (26, 27), (27, 28), (29, 30), (30, 31), (32, 33), (50, 51), (51, 52),
    (52, 53), (53, 54), (55, 56), (60, 61), (70, 71),
]


def _matrix(chrs, starts, ends, values, cond=None):
    from gtars.signal import SignalMatrix

    values = np.asarray(values, dtype=np.float64)
    return SignalMatrix.from_arrays(chrs, starts, ends, values, cond or [f"c{k}" for k in range(values.shape[1])])


def _ids(chrs, qchrs):
    """the matrix's dictionary (first appearance) and both name columns as its ids; a name it lacks: 0xFFFFFFFF"""
    names = {}
    m = np.array([names.setdefault(c, len(names)) for c in chrs], dtype=np.uint32)
    q = np.array([names.get(c, 0xFFFFFFFF) for c in qchrs], dtype=np.uint32)
    return m, q, len(names)


def _check(chrs, starts, ends, values, qchrs, qs, qe, sm=None):
    """the library's summary of the queries == the restatement's, bit for bit; returns the library's"""
    from gtars.models import RegionSet
    from gtars.signal import summary_arrays

    values = np.asarray(values, dtype=np.float64)
    sm = sm or _matrix(chrs, starts, ends, values)
    mc, qc, n_chrom = _ids(chrs, qchrs)
    want_q, want_v, want_s = R.summary(mc, starts, ends, values, qc, qs, qe, n_chrom)
    got_q, got_v, got_s = summary_arrays(RegionSet.from_vectors(list(qchrs), qs, qe), sm)
    assert np.array_equal(got_q, want_q)
    assert got_v.shape == want_v.shape and np.array_equal(R.bits(got_v), R.bits(want_v))
    assert got_s.shape == want_s.shape
    if len(want_q):
        # a column that holds a NaN: NaNs sort last on both sides, but which NaN an operation hands on or makes (inf - inf) is
        # the machine's choice
        exact = ~np.isnan(want_v).any(axis=0) & ~np.isnan(want_s).any(axis=1)
        assert np.array_equal(R.bits(got_s[exact]), R.bits(want_s[exact]))
        assert np.array_equal(got_s[~exact], want_s[~exact], equal_nan=True)
    return got_q, got_v, got_s


def _columns(cols):
    """a matrix of disjoint rows and one query per row: the result IS `cols` (R x C)"""
    cols = np.asarray(cols, dtype=np.float64)
    n = len(cols)
    s = np.arange(n, dtype=np.uint32) * 10
    return ["chr1"] * n, s, s + 5, cols


# ---- the reference's Python cases ------------------------------------------------------------------------------------
def test_reference_python_cases(tmp_path):
    """gtars-python/tests/test_genomicdist.py TestCalcSummarySignal"""
    from gtars.models import RegionSet
    from gtars.signal import SignalMatrix, calc_summary_signal

    p = tmp_path / "m.tsv"
    p.write_bytes(b"V1\tcond_A\tcond_B\nchr1_100_200\t0.5\t0.3\nchr1_150_250\t0.2\t0.8\nchr1_300_400\t0.9\t0.1\n")
    sm = SignalMatrix.from_tsv(p)
    out = calc_summary_signal(RegionSet.from_vectors(["chr1", "chr1"], [120, 350], [180, 380]), sm)
    assert out["condition_names"] == ["cond_A", "cond_B"]
    assert out["region_labels"] == ["chr1_120_180", "chr1_350_380"]
    assert out["signal_matrix"] == [[0.5, 0.8], [0.9, 0.1]]
    assert [d["condition"] for d in out["matrix_stats"]] == ["cond_A", "cond_B"]
    assert out["matrix_stats"][0] == {"condition": "cond_A", "lower_whisker": 0.5, "lower_hinge": 0.5, "median": 0.7,
                                      "upper_hinge": 0.9, "upper_whisker": 0.9}
    assert sm.device >= 0
    out = calc_summary_signal(RegionSet.from_vectors(["chr3"], [100], [200]), sm)
    assert out["region_labels"] == [] and out["signal_matrix"] == [] and out["matrix_stats"] == []
    # on a chromosome of the matrix, without a hit
    out = calc_summary_signal(RegionSet.from_vectors(["chr1", "chr3"], [1000, 100], [2000, 200]), sm)
    assert out["region_labels"] == [] and out["matrix_stats"] == []


def test_four_row_case():
    chrs, s, e = ["chr1", "chr1", "chr1", "chr2"], [100, 150, 300, 100], [200, 250, 400, 200]
    v = [[0.5, 0.3, 0.1], [0.2, 0.8, 0.4], [0.9, 0.1, 0.7], [0.3, 0.6, 0.2]]
    q, res, _ = _check(chrs, s, e, v, ["chr1", "chr1", "chr2"], [120, 350, 500], [180, 380, 600])
    assert q.tolist() == [0, 1] and res.tolist() == [[0.5, 0.8, 0.4], [0.9, 0.1, 0.7]]


# ---- seeded differentials ----------------------------------------------------------------------------------------------
def _special(values, rng):
    """NaNs, both zeros, infinities and many ties among the values"""
    values = np.round(values, 1)
    k = rng.random(values.shape)
    values[k < 0.03] = NAN
    values[(k >= 0.03) & (k < 0.06)] = 0.0
    values[(k >= 0.06) & (k < 0.09)] = -0.0
    values[(k >= 0.09) & (k < 0.10)] = math.inf
    values[(k >= 0.10) & (k < 0.11)] = -math.inf
    return values


def _case(n_cond, seed):
    from gtars.signal import SPLIT_HITS

    rng = np.random.default_rng(seed)
    names = [f"s{k}" for k in range(5)]
    n = 18_000
    chrs = [names[k] for k in rng.integers(0, 5, n)]
    starts = rng.integers(0, 2_000_000, n).astype(np.uint32)
    ends = starts + rng.integers(150, 501, n).astype(np.uint32)
    # stacks of rows over one position each: 1, 2, 64, 65 and SPLIT_HITS + 1 hits for a query there, ends that differ (nested)
    stacks = [(3_000_000, 1), (3_010_000, 2), (3_020_000, 64), (3_030_000, 65), (3_040_000, SPLIT_HITS + 1)]
    for pos, k in stacks:
        chrs += ["s4"] * k
        starts = np.concatenate([starts, np.full(k, pos, np.uint32) + rng.integers(0, 50, k).astype(np.uint32)])
        ends = np.concatenate([ends, np.full(k, pos + 100, np.uint32) + rng.integers(0, 5_000, k).astype(np.uint32)])
    order = rng.permutation(len(chrs))  # rows in no particular order, as a file may have them
    chrs, starts, ends = [chrs[i] for i in order], starts[order], ends[order]
    values = _special(rng.normal(0, 3, (len(chrs), n_cond)), rng)

    nq = 50_000
    qchrs = [names[k] for k in rng.integers(0, 5, nq)]
    qs = rng.integers(0, 2_000_000, nq).astype(np.uint32)
    qe = qs + rng.integers(1, 600, nq).astype(np.uint32)
    for i in rng.integers(1, nq - 1, 500):  # a chromosome the matrix lacks, zero-length and inverted queries
        qchrs[i] = "zz"
    zero, inv = rng.integers(1, nq - 1, 500), rng.integers(1, nq - 1, 500)
    qe[zero] = qs[zero]
    qe[inv] = qs[inv] - np.minimum(qs[inv], 40)
    at = [1000 + 10 * j for j in range(2 * len(stacks))]  # a point query and a wide query on every stack
    for j, (pos, _) in enumerate(stacks):
        for i, (a, b) in zip(at[2 * j:2 * j + 2], ((pos + 60, pos + 61), (pos, pos + 6_000))):
            qchrs[i], qs[i], qe[i] = "s4", a, b
    return chrs, starts, ends, values, qchrs, qs, qe, stacks


@pytest.mark.parametrize("n_cond", LANE_EDGES)
def test_seeded_differential(n_cond):
    from gtars.signal import SPLIT_HITS

    chrs, starts, ends, values, qchrs, qs, qe, stacks = _case(n_cond, 1000 + n_cond)
    sm = _matrix(chrs, starts, ends, values)
    mc, qc, n_chrom = _ids(chrs, qchrs)
    off, _ = R.hits(mc, starts, ends, qc, qs, qe, n_chrom)
    counts = set(np.diff(off.astype(np.int64)).tolist())
    assert {0, 1, 2, 64, 65, SPLIT_HITS + 1} <= counts, sorted(counts)[-8:]

    # query order: sorted by (chromosome, start), first and last queries without a hit; then shuffled
    order = sorted(range(len(qchrs)), key=lambda i: (qchrs[i], int(qs[i])))
    for name, idx in (("sorted", order), ("shuffled", np.random.default_rng(n_cond).permutation(len(qchrs)).tolist())):
        c = ["s0"] + [qchrs[i] for i in idx] + ["s4"]
        s = np.concatenate([[2_500_000], qs[idx], [9_000_000]]).astype(np.uint32)
        e = np.concatenate([[2_500_100], qe[idx], [9_000_100]]).astype(np.uint32)
        got_q, _, _ = _check(chrs, starts, ends, values, c, s, e, sm=sm)
        assert got_q[0] > 0 and got_q[-1] < len(c) - 1, name


def test_device_pointer_entry():
    import torch

    from gtars.models import RegionSet
    from gtars.signal import summary_arrays, summary_device

    chrs, starts, ends, values, qchrs, qs, qe, _ = _case(5, 7)
    sm = _matrix(chrs, starts, ends, values)
    want = summary_arrays(RegionSet.from_vectors(qchrs, qs, qe), sm)
    assert sm.chrom_names == list(dict.fromkeys(chrs))
    _, qc, _ = _ids(chrs, qchrs)
    dev = torch.device("cuda", sm.device)
    with torch.cuda.device(dev):
        d = [torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(dev) for x in (qc, qs, qe)]
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            got = summary_device(sm, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), len(qc), stream.cuda_stream)
            only = summary_device(sm, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), len(qc), stream.cuda_stream, rows=False)
    assert np.array_equal(got[0], want[0]) and len(want[0]) > 1000
    assert np.array_equal(R.bits(got[1]), R.bits(want[1])) and np.array_equal(R.bits(got[2]), R.bits(want[2]))
    assert only[0] is None and only[1] is None and only[3] == len(want[0])
    assert np.array_equal(R.bits(only[2]), R.bits(want[2]))


# ---- order sensitivity ---------------------------------------------------------------------------------------------------
def test_fold_follows_ailist_order_not_start_order():
    s, e = [a for a, _ in AILIST_26], [b for _, b in AILIST_26]
    chrs = ["chr1"] * 26
    v = np.arange(26 * 3, dtype=np.float64).reshape(26, 3) / 100.0
    # a sub-list is walked from the last start below the query's end downwards, so the query (6, 8) hits rows 4, 3 (5, 15),
    # 2, 1 (0, 10) and then 0 (0, 30) of the second sub-list: row 0 is first by start, last by AIList, and rows of equal
    # start come in descending file order
    v[0] = [NAN, -0.0, 1.0]
    v[4] = [1.0, 0.0, NAN]
    v[3] = [2.0, -0.0, 5.0]  # same coordinates as row 4, other values
    v[2] = [NAN, 0.0, 7.0]
    v[1] = [2.0, -0.0, 9.0]
    mc, qc, n_chrom = _ids(chrs, ["chr1"])
    off, ids = R.hits(mc, s, e, qc, [6], [8], n_chrom)
    assert off.tolist() == [0, 5] and ids.tolist() == [4, 3, 2, 1, 0]
    _, res, _ = _check(chrs, s, e, v, ["chr1", "chr1", "chr1"], [6, 30, 101], [8, 35, 150])
    # column 0: 1.0, then 2.0 (rows 3 and 1 tie: the earlier stays), the NaNs are ignored -- start order would give the NaN;
    # column 1: the first zero, row 4's +0.0, stays -- start order, or file order among equal starts, would give -0.0;
    # column 2: the first hit's NaN stays
    assert R.bits(res[0]).tolist() == R.bits([2.0, 0.0, NAN]).tolist()
    assert len(res) == 2


# ---- statistics ----------------------------------------------------------------------------------------------------------
def test_stats_small_columns():
    for n in range(1, 7):
        _, _, st = _check(*_columns(np.arange(1, n + 1, dtype=np.float64)[::-1].reshape(n, 1)), ["chr1"] * n, np.arange(n) * 10, np.arange(n) * 10 + 5)
        if n == 5:
            assert st.tolist() == [[1.0, 2.0, 3.0, 4.0, 5.0]]
        if n == 6:
            assert st.tolist() == [[1.0, 2.0, 3.5, 5.0, 6.0]]
    q = (["chr1"] * 6, np.arange(6) * 10, np.arange(6) * 10 + 5)
    _, _, st = _check(*_columns([[1, -100], [2, 5], [3, 4], [4, 3], [5, 2], [100, 1]]), *q)
    # 1 .. 5 and 100: the upper whisker stops at 5; -100 and 1 .. 5: hinges 1 and 4, fences -3.5 and 8.5, the lower at 1
    assert st.tolist() == [[1.0, 2.0, 3.5, 5.0, 5.0], [1.0, 1.0, 2.5, 4.0, 5.0]]


def test_stats_zero_mixes_and_a_nan_column():
    rng = np.random.default_rng(5)
    n = 41
    cols = np.zeros((n, 5))
    cols[:, 0] = rng.choice([0.0, -0.0], n)  # only zeros: every statistic is the zero the stable sort leaves at its place
    cols[:, 1] = rng.choice([0.0, -0.0, 1.0, -1.0], n)
    cols[:, 2] = rng.normal(0, 1, n)
    cols[rng.integers(0, n, 5), 2] = NAN  # NaN columns beside exact ones: a few NaNs stay behind the upper whisker,
    cols[:, 3] = rng.choice([0.0, -0.0, -2.0], n)
    cols[:, 4] = rng.normal(0, 1, n)
    cols[rng.permutation(n)[:30], 4] = NAN  # 30 of 41 reach the median and the upper hinge: the whiskers fall back to the hinges
    _, res, st = _check(*_columns(cols), ["chr1"] * n, np.arange(n) * 10, np.arange(n) * 10 + 5)
    assert np.array_equal(R.bits(res), R.bits(cols))
    assert not np.isnan(st[:4]).any() and st[2, 4] == np.nanmax(cols[:, 2])
    assert np.isnan(st[4]).tolist() == [False, False, True, True, True] and st[4, 0] == st[4, 1]


def test_stats_sorted_in_groups_of_conditions():
    """the debug hook makes 7 conditions sort in 3 groups (3 + 3 + 1)"""
    from gtars_amd._lib import lib as L

    rng = np.random.default_rng(9)
    n = 50
    cols = _special(rng.normal(0, 2, (n, 7)), rng)
    q = (["chr1"] * n, np.arange(n) * 10, np.arange(n) * 10 + 5)
    whole = _check(*_columns(cols), *q)
    before = L.gtars_debug_signal_sort_elems(3 * n)
    try:
        parts = _check(*_columns(cols), *q)
    finally:
        assert L.gtars_debug_signal_sort_elems(before) == 3 * n
    assert np.array_equal(R.bits(whole[2]), R.bits(parts[2]))


def _flip(rng, upper):
    """hinges whose fence rounds differently fused and rounded twice, and the data value at which inclusion flips"""
    while True:
        lh, iqr_src = rng.uniform(1, 2), rng.uniform(0.1, 1)
        uh = lh + iqr_src
        iqr = uh - lh
        twice = uh + 1.5 * iqr if upper else lh - 1.5 * iqr
        exact = Fraction(uh) + Fraction(3, 2) * Fraction(iqr) if upper else Fraction(lh) - Fraction(3, 2) * Fraction(iqr)
        fused = float(exact)  # int / int division: correctly rounded, what one fused multiply-add returns
        if fused != twice:
            # the value between the two fences' reach: inside one, outside the other
            return lh, uh, (max if upper else min)(fused, twice)


def test_fences_are_rounded_twice():
    rng = np.random.default_rng(11)
    cols = np.zeros((5, 2))
    lh, uh, w = _flip(rng, upper=False)
    cols[:, 0] = [w, lh, (lh + uh) / 2, uh, uh + 0.01]  # n = 5: the hinges are the second and fourth values
    lh, uh, w = _flip(rng, upper=True)
    cols[:, 1] = [lh - 0.01, lh, (lh + uh) / 2, uh, w]
    ref0, ref1 = R.boxplot_stats(cols[:, 0]), R.boxplot_stats(cols[:, 1])
    # the flip is real: exactly one of the two roundings takes the extreme value in
    fence0 = Fraction(ref0[1]) - Fraction(3, 2) * Fraction(ref0[3] - ref0[1])
    assert (cols[0, 0] >= float(fence0)) != (ref0[0] == cols[0, 0])
    fence1 = Fraction(ref1[3]) + Fraction(3, 2) * Fraction(ref1[3] - ref1[1])
    assert (cols[4, 1] <= float(fence1)) != (ref1[4] == cols[4, 1])
    _check(*_columns(cols), ["chr1"] * 5, np.arange(5) * 10, np.arange(5) * 10 + 5)
