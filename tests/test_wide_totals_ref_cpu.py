"""tests/wide_totals_ref.py against the definitional model of tests/overlap_def.py on small random inputs, and the properties the
GPU tests' shapes were chosen for (tests/test_gpu_wide_totals.py), asserted without a GPU."""
import numpy as np
import pytest

import overlap_def
import wide_totals_ref as W

TWO32 = 1 << 32


@pytest.mark.parametrize("seed", range(4))
def test_pool_counts_and_offsets_agree_with_the_definitional_model(seed):
    rng = np.random.default_rng(seed)
    n, n_pool, nq, n_chrom = 400, 60, 900, 3
    c = rng.integers(0, n_chrom, n)
    s = rng.integers(0, 5_000, n)
    e = s + rng.integers(0, 600, n)  # (zero-length intervals too)
    qc = np.where(rng.random(n_pool) < 0.1, W.UNK, rng.integers(0, n_chrom, n_pool))
    qs = rng.integers(0, 5_500, n_pool)
    qe = qs + rng.integers(0, 800, n_pool)
    pool = (qc, qs, qe)
    idx = rng.integers(0, n_pool, nq)
    files = rng.integers(0, 5, n)
    model = overlap_def.Model(c, s, e, n_chrom=n_chrom)
    hits = model.query(qc[idx], qs[idx], qe[idx])
    for mo in (None, 1, 2, 10, 300):
        counts = W.pool_counts((c, s, e), pool, mo)
        assert counts.dtype == np.int64 and counts.shape == (n_pool, 1)
        want = hits.count_overlaps(mo).astype(np.int64)
        assert np.array_equal(counts[idx, 0], want), mo
        off = W.batch_offsets(counts[:, 0], idx)
        assert off.dtype == np.int64 and np.array_equal(off[1:], np.cumsum(want)) and off[0] == 0
        per_file = W.pool_counts((c, s, e), pool, mo, files, 5)
        assert np.array_equal(per_file.sum(axis=1), counts[:, 0])
        keep = hits._keep(mo)
        f_of_hit = files[model.f_row[hits.pos[keep]]]
        assert W.batch_group_totals(per_file, idx) == np.bincount(f_of_hit, minlength=5).tolist()
        any_hit = np.zeros((nq, 5), dtype=bool)
        any_hit[hits.q[keep], f_of_hit] = True
        assert W.batch_group_totals(per_file, idx, binary=True) == any_hit.sum(axis=0).tolist()
    assert np.array_equal(hits.tokenize()[0].astype(np.int64), W.batch_offsets(W.pool_counts((c, s, e), pool)[:, 0], idx))


def test_set_lengths_and_lola_cells_on_small_values():
    off = np.array([0, 3, 3, 3, 10, 10, 12], dtype=np.int64)
    assert W.set_lengths(off, [0, 1, 3, 3, 4, 6], 0) == ([0, 3, 4, 5, 12, 14], 14, 7)
    assert W.set_lengths(off, [0, 1, 3, 3, 4, 6], 5) == ([0, 3, 4, 5, 10, 12], 12, 5)
    assert W.lola_cells([3, 9], [5, 4], 7, 20) == ([3, 9], [2, -5], [4, -2], [11, 18])


def test_the_stack_and_its_pool_are_what_they_are_named():
    for n_u, base, length, nest in ((500, 0, 1000, 0), (W.N_U, W.HIGH_BASE, W.LENGTH, W.NEST), (W.DENSE[-1], 0, W.DENSE_LENGTH, 0)):
        c, s, e = W.stacked(n_u, base, length, nest)
        assert (s == base + np.arange(n_u)).all() and (e >= s + length).all() and e.max() <= W.UNK
        assert s.max() <= base + n_u and e.min() >= base + length  # every interval contains [base + n_u, base + length)
        pool = W.query_pool(n_u, base, 24, length=length)
        counts = W.pool_counts(W.universe(n_u, base, length, nest), pool)[:, 0]
        qc, qs, qe, kind = pool
        assert len(qc) <= W.POOL_MAX and qe.max() <= W.UNK
        assert (counts[kind == 0] == n_u).all() and (kind == 0).sum() == W.N_FULL
        assert np.array_equal(counts[kind == 1], qs[kind == 1] - base + 1)
        rest = counts[kind == 2]
        assert (rest == 0).sum() >= 3 and (rest > 0).sum() >= 8 and rest.max() < 30
        assert (qc == W.UNK).sum() == 1 and {1, 2} <= set(qc.tolist())
    # nest: every NEST-th interval of the stack goes to a second AIList sub-list, the others stay in the first
    c, s, e = W.stacked(2_000, 0, 10_000, W.NEST)
    _, headers = overlap_def.ailist_layout(s, e)
    assert headers == [0, 2_000 - 2_000 // W.NEST]


@pytest.mark.parametrize("base,nest", [(0, 0), (W.HIGH_BASE, 0), (0, W.NEST)])
def test_batch_a_crosses_two_to_the_32_in_its_middle(base, nest):
    pool, counts, idx = W.case_a(base, nest)
    off = W.batch_offsets(counts, idx)
    assert len(idx) == W.NQ_A and (pool[3][idx[0::2]] == 0).all() and (pool[3][idx[1::2]] != 0).all()
    total, cross = int(off[-1]), W.first_at_or_past(off, TWO32)
    assert 7.0e9 < total < 7.6e9, total
    assert 0.5 * W.NQ_A < cross < 0.65 * W.NQ_A, cross        # a third of the batch and more lies beyond 2^32
    for tile in (1024, 2048, 4096, 8192):                       # no tile guard is involved
        assert W.max_tile_total(off, tile) < TWO32 // 8
    assert 2.0e8 < W.max_tile_total(off, 4096) < 2.4e8
    order = W.in_order(pool, idx)
    so = W.batch_offsets(counts, order)
    qc, qs, _ = (x.astype(np.int64) for x in W.queries_of(pool, order))
    assert ((np.diff(qc) > 0) | ((np.diff(qc) == 0) & (np.diff(qs) >= 0))).all() and qc[-1] == W.UNK and int(so[-1]) == total
    assert W.max_tile_total(so, 8192) == 8192 * W.N_U < TWO32  # in order the full queries lie in a row
    if base:
        assert pool[1][idx].min() < 100 and np.median(pool[1][idx]) > 1 << 31


@pytest.mark.parametrize("dense", W.DENSE)
def test_batch_b_has_one_tile_at_two_to_the_32_or_just_past_it(dense):
    pool, counts, idx = W.case_b(dense)
    t = W.heavy_tile(dense)
    assert t == {524_288: 8192, 1_048_576: 4096, 1_048_577: 4096, 2_097_152: 2048}[dense] and len(idx) == 4 * t
    off = W.batch_offsets(counts, idx)
    first = int(off[t])
    assert first == dense * t and TWO32 <= first <= TWO32 + 4096 and first - TWO32 == {1_048_577: 4096}.get(dense, 0)
    assert (np.diff(off[:t + 1]) == dense).all()
    assert dense * (t - 1) < TWO32                              # one query fewer and the tile fits
    assert (off[t + 1:] > TWO32).all() and int(off[-1]) > 2 * TWO32
    tail = W.light_tail(pool[3], counts, 5_000)
    assert counts[tail].max() <= 64 and (counts[tail] == 0).any() and (counts[tail] > 0).any()


def test_sets_of_c_hold_a_set_longer_than_two_to_the_32():
    pool, counts, idx = W.case_a()
    off = W.batch_offsets(counts, idx)
    long_sets, short_sets = W.sets_c(counts, idx)
    for so in (long_sets, short_sets):
        assert so[0] == 0 and so[-1] == W.NQ_A and (np.diff(so) >= 0).all()
    raw = [int(off[b]) - int(off[a]) for a, b in zip(long_sets[:-1], long_sets[1:])]
    assert sum(r > TWO32 for r in raw) == 1 and max(raw) > 5e9
    k = int(np.argmax(raw))
    assert all(int(off[a]) > TWO32 for a in long_sets[k + 1:-1])             # the sets behind it start beyond 2^32
    n_q = np.diff(long_sets)
    assert ((n_q > 0) & (np.array(raw) == 0)).sum() == 2 and (n_q == 0).sum() == 2  # empty sets; sets without a query
    out, total, longest = W.set_lengths(off, long_sets, 0)
    assert total == int(off[-1]) + 4 and longest == max(raw)
    out, total, longest = W.set_lengths(off, long_sets, TWO32 - 1)
    assert longest == TWO32 - 1 and total == int(off[-1]) + 4 - (max(raw) - (TWO32 - 1))
    out, total, longest = W.set_lengths(off, long_sets, 5)
    assert longest == 5 and total <= 5 * (len(long_sets) - 1)
    raw = [int(off[b]) - int(off[a]) for a, b in zip(short_sets[:-1], short_sets[1:])]
    assert max(raw) < TWO32 // 4 and int(off[short_sets[-2]]) > TWO32


def test_case_d_totals_per_file():
    uni, files, pool, counts, idx = W.case_d()
    assert len(files) == len(uni[0]) and np.bincount(files[:W.N_U]).tolist() == [10_000, 20_000, 40_000]
    assert (uni[0][files == 3] > 0).all() and (uni[0][files < 3] == 0).all() and uni[2].max() < 1 << 31
    t1 = W.batch_group_totals(counts[1], idx)
    assert t1[0] < TWO32 < t1[1] < t1[2] and 0 < t1[3] < 1 << 20, t1
    one = W.batch_group_totals(counts[1], idx[:W.NQ_D_ONE])
    assert one[1] < TWO32 < one[2] and W.batch_group_totals(counts[10], idx[:W.NQ_D_ONE])[2] == (W.NQ_D_ONE // 2) * 40_000 > TWO32, one  # (both walks)
    assert W.batch_group_totals(counts[1], idx[:W.NQ_A])[2] < TWO32  # (why the batch of (a) itself is too short here)
    t10 = W.batch_group_totals(counts[10], idx)
    assert t10[:3] == [(W.NQ_D // 2) * n for n in (10_000, 20_000, 40_000)] and t10[2] > TWO32 > t10[1], t10  # only the full queries stay
    rows = [W.batch_group_totals(counts[1], idx[a:b]) for a, b in zip(W.SETS_D[:-1], W.SETS_D[1:])]
    assert sum(max(r) > TWO32 for r in rows) == 2 and [sum(r[f] for r in rows) for f in range(4)] == t1
    binary = W.batch_group_totals(counts[1], idx, binary=True)
    assert all(b <= W.NQ_D for b in binary) and binary[0] > W.NQ_D // 2
