"""The fused tokenizer's switchable forms against the CPU oracle, bit-exact: the redo of a batch by the generic kernel after a
look-back timeout (GTARS_TEST_FORCE_LOOKBACK_TIMEOUT), the id staging of a wave on both sides of its threshold
(GTARS_TOK_STAGE), and the sorted hint (GTARS_TOK_SORTED), which is accepted and changes nothing.
Which kernel a call ran is read from the profiler's kernel names and facts, never assumed."""
import numpy as np
import pytest

from oracle import KIND_AILIST, KIND_BITS
from test_gpu_parity import UNK, VARIANTS, _pair, _tok_device, ga, sweep_cases  # noqa: F401  (ga: the module's fixture)

pytestmark = pytest.mark.gpu

SENTINEL = -7


def _profiled(ga, fn):
    """fn() with the profiler on -> (its result, {kernel name or fact: ...})"""
    _lib = ga._lib
    _lib.lib.gtars_prof_reset()
    _lib.lib.gtars_prof_enable(1)
    try:
        r = fn()
        prof = _lib.prof_read()
    finally:
        _lib.lib.gtars_prof_enable(0)
    return r, prof


def _to_device(qc, qs, qe):
    import torch

    dev = torch.device("cuda", torch.cuda.current_device())
    return [torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).to(dev) for x in (qc, qs, qe)]


def _tokenize_with_capacity(ga, g, d, cap, total, hint=0):
    """gtars_tokenize_device into an id buffer of `total + 8` sentinels of which the library may use `cap`
    -> (the CapacityError or None, H or None, offsets, the whole id buffer)"""
    import torch

    nq = d[0].numel()
    off = torch.full((nq + 1,), -1, dtype=torch.int64, device=d[0].device)
    ids = torch.full((max(total, cap) + 8,), SENTINEL, dtype=torch.int32, device=d[0].device)
    err = h = None
    try:
        h = g.tokenize_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), nq, off.data_ptr(), ids.data_ptr(), cap,
                              torch.cuda.current_stream().cuda_stream, sync=True, hint=hint)
    except ga.CapacityError as e:
        err = e
    return err, h, off.cpu().numpy().view(np.uint64), ids.cpu().numpy()


def _assert_capacity_rule(res, cap, off_o, ids_o, what):
    """the rule of gtars_tokenize_device: offsets complete whatever the capacity; a capacity below the result is CapacityError
    (naming the result's size) with the ids equal up to the capacity; nothing is written behind the capacity / the result"""
    err, h, off, ids = res
    total = len(ids_o)
    assert np.array_equal(off, off_o.astype(np.uint64)), (what, np.argwhere(off != off_o)[:3])
    if cap < total:
        assert err is not None and err.needed == total, (what, err, h)
    else:
        assert err is None and h == total, (what, err, h)
    n = min(cap, total)
    assert np.array_equal(ids[:n].view(np.uint32), ids_o[:n]), (what, np.argwhere(ids[:n].view(np.uint32) != ids_o[:n])[:3])
    assert (ids[n:] == SENTINEL).all(), (what, np.argwhere(ids[n:] != SENTINEL)[:3] + n)


# ------------------------------------------------------------------------------------------ the forced look-back timeout

LOOKBACK_SIZES = (1, 3841, 8193, 50_001)  # 1, 1, 3 and 13 tiles of 4096 queries: consecutive calls differ in tile count


@pytest.fixture(scope="module")
def lookback_inputs(ga):
    """three indexes over one disjoint universe -- Bits with ids from the position, Bits with shuffled ids, AIList with one
    sub-list per chromosome (k_tok_lds' REV form) -- and, per batch size, the queries and the oracle's answers"""
    from gtars_amd import synth

    u = synth.make_universe(20_000)
    shuffled = np.random.default_rng(77).permutation(len(u["chrom"])).astype(np.uint32)
    indexes = {"bits": _pair(ga, u["chrom"], u["start"], u["end"], None, n_chrom=synth.N_CHROM, kind=KIND_BITS),
               "bits_shuffled_ids": _pair(ga, u["chrom"], u["start"], u["end"], shuffled, n_chrom=synth.N_CHROM, kind=KIND_BITS),
               "ailist_one_sublist": _pair(ga, u["chrom"], u["start"], u["end"], shuffled, n_chrom=synth.N_CHROM, kind=KIND_AILIST)}
    batches = {}
    for nq in LOOKBACK_SIZES:
        q = synth.make_queries(u, nq, seed=nq)
        qc, qs, qe = q["chrom"].copy(), q["start"], q["end"]
        qc[::53] = UNK
        want = {name: (o.tokenize(qc, qs, qe), o.find_overlaps_regions(qc, qs, qe, 20)) for name, (_, o) in indexes.items()}
        batches[nq] = (qc, qs, qe, want)
    o = indexes["bits"][1]
    qc, qs, qe, _ = batches[8193]
    irs = {mo: o.irs_find_overlaps(u["chrom"], u["start"], u["end"], qc, qs, qe, mo) for mo in (None, 20)}
    return indexes, batches, irs


STEPS = (("default", False), ("forced", True), ("default again", False))


@pytest.mark.parametrize("name", ["bits", "bits_shuffled_ids", "ailist_one_sublist"])
def test_forced_lookback_timeout_redoes_the_batch_with_the_generic_kernel(ga, monkeypatch, lookback_inputs, name):
    """run_fused_sync (api.hip) redoes a batch with k_enum_fused when the LDS tokenizer reports a look-back timeout: the
    workspace's ScanEpoch is reset while the workspace still holds the LDS kernel's granules, and the next default call starts
    from that reset epoch on a workspace the generic kernel used last.  GTARS_TEST_FORCE_LOOKBACK_TIMEOUT replaces the status of
    a launch that SUCCEEDED, so nothing is provoked; the redo is the code production runs when another process holds CUs.

    Public entry points that reach run_fused_sync, each covered here:
      * gtars_tokenize_device / gtars_tokenize_device_ex with total_hits (OverlapIndex.tokenize_device, sync=True): the thread's
        workspace and its epoch live across calls -- three steps (default, forced, default again) on one index and one stream,
        four batch sizes per step, offsets and ids against the oracle at every step, and a capacity below the result under
        the forced timeout (CapacityError, complete offsets, ids up to the capacity, the sentinel behind it);
      * gtars_find_overlaps and the two entries that share enumerate_to_host with it (OverlapIndex.find_overlaps): min_overlap
        20 (the FILTER kernels), the payload pass runs k_tok_lds on the workspace the redo left;
      * gtars_find_overlap_indices (OverlapIndex.find_overlap_indices), with and without min_overlap, on the Bits index.
    gtars_tokenize / gtars_tokenize_into reach it only for an index the LDS kernels do NOT serve, where the hook's status is
    returned as it is (no redo exists there): not a path of this switch."""
    indexes, batches, irs = lookback_inputs
    g, _ = indexes[name]
    enum = "k_enum_fused<ailist>" if name.startswith("ailist") else "k_enum_fused<bits>"
    for step, forced in STEPS:
        if forced:
            monkeypatch.setenv("GTARS_TEST_FORCE_LOOKBACK_TIMEOUT", "1")
        for nq in LOOKBACK_SIZES:
            qc, qs, qe, want = batches[nq]
            (off_o, ids_o), fo = want[name]
            d = _to_device(qc, qs, qe)
            total = len(ids_o)
            res, prof = _profiled(ga, lambda: _tokenize_with_capacity(ga, g, d, total + 8, total))
            assert "k_tok_lds" in prof and (enum in prof) == forced, (step, nq, sorted(prof))
            _assert_capacity_rule(res, total + 8, off_o, ids_o, (name, step, nq))
            fg, prof = _profiled(ga, lambda: g.find_overlaps(qc, qs, qe, 20))
            assert "k_tok_lds" in prof and (enum in prof) == forced, (step, nq, sorted(prof))
            assert all(np.array_equal(a, b) for a, b in zip(fg, fo)), (name, step, nq, "find_overlaps")
        if forced:
            qc, qs, qe, want = batches[50_001]
            (off_o, ids_o), _ = want[name]
            cap = len(ids_o) // 2
            res, prof = _profiled(ga, lambda: _tokenize_with_capacity(ga, g, _to_device(qc, qs, qe), cap, len(ids_o)))
            assert enum in prof, sorted(prof)
            _assert_capacity_rule(res, cap, off_o, ids_o, (name, step, "capacity"))
        if name == "bits":
            qc, qs, qe, _ = batches[8193]
            for mo in (None, 20):
                (og, ig), prof = _profiled(ga, lambda: g.find_overlap_indices(qc, qs, qe, mo))
                assert (enum in prof) == forced, (step, mo, sorted(prof))
                assert np.array_equal(og, irs[mo][0]) and np.array_equal(ig, irs[mo][1]), (step, mo)
        if forced:
            monkeypatch.delenv("GTARS_TEST_FORCE_LOOKBACK_TIMEOUT")


# ------------------------------------------------------------------------------------------------ the staging threshold

STAGE_NQ = 16_384
WAVE_Q = 256  # queries of one wave and round: 64 lanes x 4 queries
# 256-query blocks of the batch and what they are in every launch geometry of VARIANTS (tiles of 2048, 4096 and 8192 queries)
STAGE_BLOCKS = {32: "first wave of a tile", 35: "a middle wave", 47: "last wave of a round", 48: "first wave of round 1 (tile 8192)",
                63: "last wave of the last tile"}
STAGES = (128, 512)


def _stage_universe():
    n = 6_000
    s = (100 * np.arange(n)).astype(np.uint32)
    return np.zeros(n, dtype=np.uint32), s, s + np.uint32(50)


def _queries_with_hits(rng, counts):
    """on the universe of _stage_universe: query i overlaps exactly counts[i] intervals"""
    a = rng.integers(0, 6_000 - 64, len(counts))
    h = np.asarray(counts)
    qs = np.where(h > 0, 100 * a + 10, 100 * a + 60)
    qe = np.where(h > 0, 100 * (a + h - 1) + 20, 100 * a + 90)
    return np.zeros(len(h), dtype=np.uint32), qs.astype(np.uint32), qe.astype(np.uint32)


@pytest.fixture(scope="module")
def stage_inputs(ga):
    """two Bits indexes over 6000 disjoint intervals (ids from the position; shuffled ids) and 30 batches of 16 384 queries: in
    each, ONE 256-query block has exactly stage - 1, stage or stage + 1 hits (one query of 20 hits, which leaves by wave-wide
    stores, the rest spread at random), every other query 0, 1 or 2 -- with the oracle's answer for both indexes"""
    c, s, e = _stage_universe()
    shuffled = np.random.default_rng(5).permutation(len(c)).astype(np.uint32)
    indexes = {"ids_from_position": _pair(ga, c, s, e, None, n_chrom=1), "shuffled_ids": _pair(ga, c, s, e, shuffled, n_chrom=1)}
    rng = np.random.default_rng(886)
    batches = []
    for block in STAGE_BLOCKS:
        for stage in STAGES:
            for total in (stage - 1, stage, stage + 1):
                counts = rng.integers(0, 3, STAGE_NQ)
                mine = np.zeros(WAVE_Q, dtype=np.int64)
                big = int(rng.integers(0, WAVE_Q))
                mine[big] = 20
                rest = rng.multinomial(total - 20, np.where(np.arange(WAVE_Q) == big, 0.0, 1.0 / (WAVE_Q - 1)))
                counts[block * WAVE_Q:(block + 1) * WAVE_Q] = mine + rest
                qc, qs, qe = _queries_with_hits(rng, counts)
                want = {}
                for name, (_, o) in indexes.items():
                    off_o, ids_o = o.tokenize(qc, qs, qe)
                    assert np.array_equal(np.diff(off_o.astype(np.int64)), counts)  # the batch is what it was built to be
                    want[name] = (off_o, ids_o)
                batches.append((block, stage, total, (qc, qs, qe), want))
    return indexes, batches


@pytest.mark.parametrize("stage_env", ["0", "128", None])
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_id_staging_on_both_sides_of_its_threshold(ga, monkeypatch, stage_inputs, variant, stage_env):
    """A wave's share of a tile (k_tok_lds): lane t of a group of GW waves holds, in round r, the four queries
    tile * TILE + r * ROUND + 4 t ... (ROUND = GW * 256, TILE = R * ROUND), so wave w of the group holds the 256 CONSECUTIVE
    queries from tile * TILE + r * ROUND + 256 w on; `wtotal` is the hit total of these 256 queries and `wave_base` the CSR
    offset of the first of them (the scan runs over the wave parts in round-major order, which is query order).  The wave's ids
    go through its LDS staging buffer iff wtotal <= stage_cap: round 0 by stage_queries / flush_queries (the flush clips at the
    caller's capacity), round 1 and every wave stage_queries refused by write_queries, where the ids are staged iff
    `cap && wtotal <= stage_cap && wave_base + wtotal <= cap`.

    stage_cap is GTARS_TOK_STAGE words (unset: 512; under 128: no staging).  Batches whose chosen 256-query block has exactly
    stage - 1, stage and stage + 1 hits for stage 128 and 512 -- the block being the first, a middle and the last wave of a tile,
    the last wave of round 0 and the first of round 1 of an 8192-query tile -- under every launch geometry, each with a caller
    capacity of wave_base + wtotal - 1, + 0 and + 1 (the third term): offsets complete, CapacityError exactly when the capacity
    is below the result, ids equal up to the capacity, the sentinel untouched behind it."""
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    if stage_env is not None:
        monkeypatch.setenv("GTARS_TOK_STAGE", stage_env)
    indexes, batches = stage_inputs
    for name, (g, _) in indexes.items():
        for block, stage, total, (qc, qs, qe), want in batches:
            off_o, ids_o = want[name]
            first = block * WAVE_Q
            wave_base, wtotal = int(off_o[first]), int(off_o[first + WAVE_Q] - off_o[first])
            assert wtotal == total and wave_base > 0
            d = _to_device(qc, qs, qe)
            for cap in (wave_base + wtotal - 1, wave_base + wtotal, wave_base + wtotal + 1):
                res, prof = _profiled(ga, lambda: _tokenize_with_capacity(ga, g, d, cap, len(ids_o)))
                assert "k_tok_lds" in prof, sorted(prof)
                _assert_capacity_rule(res, cap, off_o, ids_o, (variant, stage_env, name, STAGE_BLOCKS[block], stage, total, cap))


# ------------------------------------------------------------------------------------------------------- the sorted hint

@pytest.mark.parametrize("explicit_ids", [False, True])
def test_sorted_hint_without_the_sweep_form(ga, explicit_ids):
    """A batch given with the sorted hint goes to k_tok_lds (or, for a universe beyond its LDS key budget, to the generic kernel)
    and equals the oracle; no sweep kernel runs (the form the hint once selected was removed)."""
    rng = np.random.default_rng(17 + KIND_BITS)
    ran = set()
    for n, g, o_, (qc, qs, qe), cap_factor in sweep_cases(ga, rng, KIND_BITS, explicit_ids):
        want_off, want_ids = o_.tokenize(qc, qs, qe)
        (off, ids), prof = _profiled(ga, lambda: _tok_device(ga, g, qc, qs, qe, g.TOK_SORTED, cap_factor=cap_factor))
        assert "tok_build_sweep" not in prof and "k_tok_sweep" not in prof, sorted(prof)
        assert "k_tok_lds" in prof or "k_enum_fused<bits>" in prof, sorted(prof)
        ran |= set(prof)
        assert np.array_equal(off, want_off), (n, np.argwhere(off != want_off)[:3])
        assert np.array_equal(ids, want_ids), (n, np.argwhere(ids != want_ids)[:3])
    assert "k_tok_lds" in ran, sorted(ran)


def test_sorted_hint_changes_nothing(ga, lookback_inputs):
    """GTARS_TOK_SORTED is accepted and ignored: on every index of lookback_inputs, a call with the hint and one without record
    the same kernel names and facts, and both return the oracle's offsets and ids."""
    indexes, batches, _ = lookback_inputs
    for name, (g, _) in indexes.items():
        for nq in (3841, 50_001):
            qc, qs, qe, want = batches[nq]
            off_o, ids_o = want[name][0]
            seen = {}
            for hint in (g.TOK_SORTED, g.TOK_AUTO):
                (off, ids), prof = _profiled(ga, lambda: _tok_device(ga, g, qc, qs, qe, hint))
                assert np.array_equal(off, off_o) and np.array_equal(ids, ids_o), (name, nq, hint)
                seen[hint] = set(prof)
            assert seen[g.TOK_SORTED] == seen[g.TOK_AUTO], (name, nq, sorted(seen[g.TOK_SORTED] ^ seen[g.TOK_AUTO]))
            assert "k_tok_lds" in seen[g.TOK_AUTO], (name, nq, sorted(seen[g.TOK_AUTO]))


def test_generic_kernels_under_the_ab_switch(ga, monkeypatch, lookback_inputs):
    """GTARS_NO_LDS_PATH=1, the A/B baseline: the generic kernel (k_enum_fused) answers an index the LDS tokenizer serves, for the
    unsorted and the sorted hint; offsets and ids are the oracle's and no LDS kernel runs."""
    indexes, batches, _ = lookback_inputs
    monkeypatch.setenv("GTARS_NO_LDS_PATH", "1")
    for name, (g, _) in indexes.items():
        enum = "k_enum_fused<ailist>" if name.startswith("ailist") else "k_enum_fused<bits>"
        for nq in (3841, 50_001):
            qc, qs, qe, want = batches[nq]
            off_o, ids_o = want[name][0]
            for hint in (g.TOK_AUTO, g.TOK_SORTED):
                (off, ids), prof = _profiled(ga, lambda: _tok_device(ga, g, qc, qs, qe, hint))
                assert enum in prof and "k_tok_lds" not in prof, (name, nq, hint, sorted(prof))
                assert np.array_equal(off, off_o) and np.array_equal(ids, ids_o), (name, nq, hint)
