"""Hit totals at and past 2^32 through every count path, exact on every offset.

The library's contract is 64-bit (d_offsets, *total_hits, IGD d_hits, the offsets and *total of gtars_tokenize_sets_device are
u64) while the kernels sum in 32 bits where they can and widen at a seam: a tile's total when it is published to the chained
scan, a workgroup's IGD counters when they are handed to hits[], a set's clipped length when it is scanned.  Here those seams
carry values that need the upper word: a running total that crosses 2^32 in the middle of a batch (a), ONE tile whose hits are
exactly 2^32 or a few thousand more -- 0 or a few thousand in 32 bits -- under every launch geometry (b), region sets longer
than 2^32 ids and sets that start beyond 2^32 (c), IGD per-file totals past 2^32 (d), LOLA cells near 2^33 (e).

Every call is COUNT-ONLY (d_ids == NULL, capacity 0) on a universe of stacked intervals (tests/wide_totals_ref.py): no id is
written, the inputs are a few megabytes.  WRITING ids at offsets >= 2^32 needs an id buffer of at least 16 GiB on a shared card;
it is deliberately out of scope here.  Nothing here provokes a fault: every buffer is valid and a refusal is an error code.

The reference is the definition on a pool of <= 256 distinct queries and a lookup (wide_totals_ref.pool_counts /
batch_offsets), in int64 and Python ints; the shapes' properties are asserted on the CPU by tests/test_wide_totals_ref_cpu.py.
Which kernel a call ran is read from the profiler's kernel names and facts, never assumed; every case prints it ("PATH ...").
"""
import numpy as np
import pytest

import wide_totals_ref as W

pytestmark = pytest.mark.gpu

KIND_BITS, KIND_AILIST = 0, 1
TWO32 = 1 << 32
U32_MAX = TWO32 - 1


@pytest.fixture(scope="module")
def ga():
    import gtars_amd

    assert gtars_amd.device_count() > 0, "no MI355X visible: -m gpu tests must run on the GPU box"
    return gtars_amd


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


def _device():
    import torch

    return torch.device("cuda", torch.cuda.current_device())


def _to_device(cols):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).to(_device()) for x in cols]


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _count_only(g, d, hint=0, sync=True):
    """gtars_tokenize_device_ex without an id buffer -> (H or None, offsets int64[nq + 1] from a buffer of -1)"""
    import torch

    nq = d[0].numel()
    off = torch.full((nq + 1,), -1, dtype=torch.int64, device=d[0].device)
    h = g.tokenize_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), nq, off.data_ptr(), 0, 0, _stream(), sync=sync, hint=hint)
    torch.cuda.synchronize()
    return h, off.cpu().numpy()


def _assert_offsets(off, want, what):
    bad = np.flatnonzero(off != want)
    assert len(bad) == 0, (what, "first wrong offset at query", int(bad[0]), "got", int(off[bad[0]]), "want", int(want[bad[0]]),
                           "wrong:", len(bad), "of", len(want))


def _note(what, prof):
    """which kernels and facts the profiler saw, with the kernels' device time"""
    print("PATH", what, "->", " ".join(f"{k}[{v['total_ms']:.1f}ms]" if v["total_ms"] else k for k, v in sorted(prof.items())))


def _index(ga, uni, kind):
    c, s, e = uni
    return ga.OverlapIndex(c, s, e, None, n_chrom=3, kind=kind)


# ------------------------------------------------------------------------- (a) a running total across 2^32, every tokenizer path

# form -> (hint bits, batch in order, switches, the facts / kernels that must have run, those that must not)
def _forms_a(kind):
    enum = "k_enum_fused<ailist>" if kind == KIND_AILIST else "k_enum_fused<bits>"
    return {
        "default": (0, False, {}, ("tok_build_wide", "k_tok_lds"), (enum, "k_tok_sweep")),
        "narrow": (1, False, {}, ("tok_build_narrow", "k_tok_lds"), (enum, "k_tok_sweep")),
        "sorted": (4, True, {}, ("tok_build_wide", "k_tok_lds"), (enum, "k_tok_sweep")),
        "generic": (0, False, {"GTARS_NO_LDS_PATH": "1"}, (enum,), ("k_tok_lds", "k_tok_sweep")),
    }


@pytest.fixture(scope="module")
def indexes_a(ga):
    built = {}

    def get(kind, base=0, nest=0):
        key = (kind, base, nest)
        if key not in built:
            built[key] = _index(ga, W.universe(W.N_U, base, nest=nest), kind)
        return built[key]

    return get


def _run_a(ga, monkeypatch, g, case, form, forms, what):
    pool, counts, idx = case
    hint, ordered, env, ran, ran_not = forms[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if ordered:
        idx = W.in_order(pool, idx)
    want = W.batch_offsets(counts, idx)
    assert int(want[-1]) > TWO32 + TWO32 // 2 and W.first_at_or_past(want, TWO32) < len(idx) - 40_000  # (40 000 queries lie beyond)
    d = _to_device(W.queries_of(pool, idx))
    (h, off), prof = _profiled(ga, lambda: _count_only(g, d, hint, sync=True))
    _note((what, form, "sync"), prof)
    assert h == int(want[-1]), (what, form, h, int(want[-1]), h - int(want[-1]))
    _assert_offsets(off, want, (what, form, "sync"))
    for name in ran:
        assert name in prof, (what, form, name, sorted(prof))
    for name in ran_not:
        assert name not in prof, (what, form, name, sorted(prof))
    (h, off), prof = _profiled(ga, lambda: _count_only(g, d, hint, sync=False))
    assert h is None
    _assert_offsets(off, want, (what, form, "async"))  # (offsets[nq] is the total)
    for name in ran:
        assert name in prof, (what, form, "async", name, sorted(prof))


@pytest.mark.parametrize("form", ["default", "narrow", "sorted", "generic"])
@pytest.mark.parametrize("kind", [KIND_BITS, KIND_AILIST], ids=["bits", "ailist"])
def test_running_total_crosses_two_to_the_32(ga, monkeypatch, indexes_a, kind, form):
    """140 000 queries on a stack of 70 000: full queries (70 000 hits) at the even positions, prefix queries and a few others at
    the odd ones; 7.3e9 hits, the running total passes 2^32 near query 82 000 of 140 000, no tile holds more than 2.3e8 (none of
    the launchers' tile guards is involved).  Count-only, synchronised (*total_hits) and not (offsets[nq]); the default (wide)
    build, the narrow build, the sorted hint (accepted, no effect: k_tok_lds) on the batch in (chromosome, start) order -- there the
    70 000 full queries lie in a row -- and the generic kernel; a Bits index and an AIList index of one sub-list per chromosome (the stack's ends ascend with
    its starts: the REV forms)."""
    g = indexes_a(kind)
    if kind == KIND_AILIST:
        assert len(g.sublist_offsets(0)) == 1
    _run_a(ga, monkeypatch, g, W.case_a(), form, _forms_a(kind), ("a", "ailist" if kind else "bits"))


def test_running_total_crosses_two_to_the_32_on_a_nested_ailist_index(ga, monkeypatch, indexes_a):
    """The same batch on an AIList universe of TWO sub-lists on chromosome 0 (every 16th interval of the stack contains its
    followers): count-only it is answered by the flat companion's LDS tokenizer (run_fused: the counts do not depend on the
    order).  The route is for universes of a coverage depth below GTARS_AILIST_REORDER_MAX_DEPTH (6); the stack's depth is
    70 000, so the switch is raised.  The fact `ailist_nested_on_lds` is noted only by a call that also reorders ids; a
    count-only call shows the route by k_tok_lds having run on an index with nested sub-lists, and k_enum_fused<ailist> not."""
    monkeypatch.setenv("GTARS_AILIST_REORDER_MAX_DEPTH", "10000000")
    g = indexes_a(KIND_AILIST, nest=W.NEST)
    assert len(g.sublist_offsets(0)) == 2
    forms = {"default": (0, False, {}, ("k_tok_lds",), ("k_enum_fused<ailist>", "k_tok_sweep")),
             "narrow": (1, False, {}, ("k_tok_lds", "tok_build_narrow"), ("k_enum_fused<ailist>", "k_tok_sweep"))}
    for form in forms:
        _run_a(ga, monkeypatch, g, W.case_a(nest=W.NEST), form, forms, ("a", "nested ailist"))
    monkeypatch.delenv("GTARS_AILIST_REORDER_MAX_DEPTH")
    forms = {"default": (0, False, {}, ("k_enum_fused<ailist>",), ("k_tok_lds", "k_tok_sweep"))}  # (and without the route)
    _run_a(ga, monkeypatch, g, W.case_a(nest=W.NEST), "default", forms, ("a", "nested ailist, generic"))


@pytest.mark.parametrize("form", ["default", "narrow", "sorted", "generic"])
def test_running_total_crosses_two_to_the_32_with_coordinates_in_the_upper_half_of_u32(ga, monkeypatch, indexes_a, form):
    """the stack at base 3 000 000 000: every start, end and query coordinate but one miss is above 2^31"""
    _run_a(ga, monkeypatch, indexes_a(KIND_BITS, base=W.HIGH_BASE), W.case_a(W.HIGH_BASE), form, _forms_a(KIND_BITS), ("a", "base 3e9"))


# ------------------------------------------------------------------------------ (b) one tile at exactly 2^32 and just past it

# The fewest queries any tokenizer kernel takes as one tile: 256 lanes x 4 queries (k_enum_fused).  k_tok_lds' smallest is
# 512 lanes x 4 -- but an index it cannot serve is handed on, in the end to the generic kernel.  A batch may be REFUSED only where even 1024 queries that all hit the densest
# chromosome could pass 2^32 - 1; every other call answers exactly.
SMALLEST_TILE = 256 * 4

NARROW, WIDE, SORTED = 1, 2, 4
FORMS_B = {  # form -> (hint, switches)
    "default": (0, {}),
    "narrow r1 g1": (NARROW, {"GTARS_TOK_ROUNDS": "1", "GTARS_TOK_GROUPS": "1"}),
    "narrow r2 g1": (NARROW, {"GTARS_TOK_ROUNDS": "2", "GTARS_TOK_GROUPS": "1"}),
    "narrow r1 g2": (NARROW, {"GTARS_TOK_ROUNDS": "1", "GTARS_TOK_GROUPS": "2"}),
    "narrow r2 g2": (NARROW, {"GTARS_TOK_ROUNDS": "2", "GTARS_TOK_GROUPS": "2"}),
    "wide g1": (WIDE, {"GTARS_TOK_GROUPS": "1"}),
    "wide g2": (WIDE, {"GTARS_TOK_GROUPS": "2"}),
    "sorted": (SORTED, {}),
    "generic": (0, {"GTARS_NO_LDS_PATH": "1"}),
}
TOKENIZER_KERNELS = ("k_tok_lds", "k_enum_fused<bits>")


def _exact_or_refused(ga, g, d, hint, want, dense, what, also_async=False):
    """the offsets and the total are exact, or the call is GTARS_ERR_INVALID_ARG "too dense" where that is allowed -- never a
    wrapped result.  -> the profile"""
    try:
        (h, off), prof = _profiled(ga, lambda: _count_only(g, d, hint, sync=True))
    except ValueError as e:
        assert "too dense" in str(e), (what, str(e))
        assert dense * SMALLEST_TILE > U32_MAX, (what, "refused a batch whose smallest tile holds at most", dense * SMALLEST_TILE, "hits")
        print("PATH", what, "-> refused:", str(e))
        return None
    _note(what, prof)
    assert h == int(want[-1]), (what, h, int(want[-1]), h - int(want[-1]))
    _assert_offsets(off, want, what)
    assert sum(k in prof for k in TOKENIZER_KERNELS) == 1, (what, sorted(prof))
    if also_async:
        (_, off), _ = _profiled(ga, lambda: _count_only(g, d, hint, sync=False))
        _assert_offsets(off, want, (what, "async"))
    return prof


@pytest.fixture(scope="module")
def dense_index(ga):
    """one dense universe on the device at a time (the cases arrive grouped by `dense`)"""
    held = {}

    def get(dense, length=W.DENSE_LENGTH):
        if dense not in held:
            held.clear()
            held[dense] = _index(ga, W.universe(dense, length=length), KIND_BITS)
        return held[dense]

    return get


@pytest.fixture(scope="module")
def batches_b():
    """per dense: {in order?: (the reference's offsets, the queries on the device)} -- computed once, shared by the forms"""
    held = {}

    def get(dense):
        if dense not in held:
            held.clear()
            pool, counts, idx = W.case_b(dense)
            for ordered in (False, True):
                i = W.in_order(pool, idx) if ordered else idx
                held.setdefault(dense, {})[ordered] = (W.batch_offsets(counts, i), _to_device(W.queries_of(pool, i)))
        return held[dense]

    return get


# One run of the heavy tile costs a workgroup 1 to 3 s (4.3e9 hits walked by 1024 lanes; measured: k_tok_lds 2.2 s, the generic
# kernel 0.7 to 2.7 s), so not every form runs at every size.  Each size keeps the default, the narrow and
# the generic form, and the forms whose tile is the one that size overflows:
#   524 288 (T = 8192): the 8192-query tiles -- two rounds in one group;
#   1 048 576 (T = 4096, exactly 2^32): one round in one group (4096), which the default (wide) build takes as well;
#   1 048 577 (T = 4096, 2^32 + 4096): two rounds in one group (two steps down), the wide build with one group, and the sorted hint
#       (k_tok_lds takes the batch in order);
#   2 097 152 (T = 2048): k_tok_lds' smallest tile overflows, every form ends on the generic kernel.
# Not run: 2 rounds x 2 groups and 1 round x 2 groups (tiles of 4096 and 2048 queries: the first is the tile of `narrow r1 g1`, the
# second holds the product at every size k_tok_lds serves).
FORMS_AT = {
    524_288: ("default", "narrow r2 g1", "generic"),
    1_048_576: ("default", "narrow r1 g1", "generic"),
    1_048_577: ("default", "narrow r2 g1", "wide g1", "sorted", "generic"),
    2_097_152: ("default", "narrow r1 g1", "generic"),
}


@pytest.mark.parametrize("dense,form", [(dense, form) for dense in W.DENSE for form in FORMS_AT[dense]])
def test_one_tile_of_two_to_the_32_hits_under_every_geometry(ga, monkeypatch, dense_index, batches_b, dense, form):
    """A stack of `dense` intervals and a batch that begins with T = ceil(2^32 / dense) full queries (8192, 4096, 4096, 2048):
    a tile of T queries holds dense x T >= 2^32 hits -- 0, 0, 4096 and 0 in 32 bits -- and 3 T mixed queries follow, all of
    them beyond 2^32.  (The stack's intervals are 4 194 304 long here, so that 2 097 152 of them still share a part.)  Count-only
    under the geometries the launchers can be pushed to (FORMS_B; which of them at which size: FORMS_AT): k_tok_lds with 1 or
    2 rounds x 1 or 2 wave groups (tiles of 4096, 8192, 2048, 4096 queries; the narrow build, which alone takes two rounds), the
    wide build, the sorted hint on the batch in order (there ALL its full queries lie in a row), and the generic kernel.  The
    launchers must step the geometry down or hand the index on: offsets exact in every case."""
    g = dense_index(dense)
    t = W.heavy_tile(dense)
    batches = batches_b(dense)
    assert int(batches[False][0][t]) == dense * t >= TWO32 > dense * (t - 1)
    hint, env = FORMS_B[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want, d = batches[bool(hint & SORTED)]
    prof = _exact_or_refused(ga, g, d, hint, want, dense, ("b", dense, form), also_async=(dense, form) == (W.DENSE[0], "generic"))
    assert prof is not None  # (dense x 1024 < 2^32 for every one of these: see SMALLEST_TILE)
    if form == "generic":
        assert "k_enum_fused<bits>" in prof, sorted(prof)
    if dense * 8192 <= TWO32:  # every form can serve this index in some geometry: the forced form is the one that ran
        assert ("k_enum_fused<bits>" if form == "generic" else "k_tok_lds") in prof, (form, sorted(prof))


def test_default_geometry_steps_down_for_a_dense_tile_in_a_long_batch(ga, dense_index):
    """the heavy tile of dense = 524 288 (8192 full queries: exactly 2^32 hits) in front of CUs x 8192 light queries: at that
    length the launcher picks the two-round, 8192-query tile itself (choose_rounds) and has to step down from it"""
    import torch

    dense = W.DENSE[0]
    pool, counts, _ = W.case_b(dense)
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    t = W.heavy_tile(dense)
    full = np.flatnonzero(pool[3] == 0)
    idx = np.concatenate([full[np.arange(t) % len(full)], W.light_tail(pool[3], counts, cus * 8192)])
    assert len(idx) >= cus * 8192 + t
    want = W.batch_offsets(counts, idx)
    assert int(want[t]) == TWO32 and (want[t:] >= TWO32).all()
    g = dense_index(dense)
    d = _to_device(W.queries_of(pool, idx))
    # (the narrow build: the wide one, which a count-only call gets by default, never takes two rounds)
    prof = _exact_or_refused(ga, g, d, NARROW, want, dense, ("b", dense, "long batch", "narrow"))
    assert prof is not None and "k_tok_lds" in prof and "tok_build_narrow" in prof, sorted(prof)


def test_a_universe_no_tile_can_count_is_refused_not_wrapped(ga, monkeypatch, dense_index):
    """4 194 304 intervals on one chromosome: 1024 queries -- the smallest tile of any kernel -- can have 2^32 hits.  Every form
    either refuses ("too dense", GTARS_ERR_INVALID_ARG) or is exact (_exact_or_refused)."""
    dense = W.DENSE_REFUSED
    assert dense * SMALLEST_TILE > U32_MAX >= (dense - 1) * SMALLEST_TILE
    pool = W.query_pool(dense, n_prefix=8, length=W.DENSE_REFUSED_LENGTH)
    counts = W.pool_counts(W.universe(dense, length=W.DENSE_REFUSED_LENGTH), pool)[:, 0]
    idx = W.heavy_first_batch(pool[3], 1024, 1024)
    g = dense_index(dense, W.DENSE_REFUSED_LENGTH)
    refused = 0
    for form in ("default", "narrow r1 g2", "sorted", "generic"):
        hint, env = FORMS_B[form]
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        i = W.in_order(pool, idx) if hint & SORTED else idx
        want = W.batch_offsets(counts, i)
        refused += _exact_or_refused(ga, g, _to_device(W.queries_of(pool, i)), hint, want, dense, ("b", dense, form)) is None
        for k in env:
            monkeypatch.delenv(k)
    print("PATH refused", refused, "of 4 forms")


# -------------------------------------------------------------------------------------------------- (c) the K15 sizing pass

def _sets_sizing(ga, g, d, set_off, max_length):
    """gtars_tokenize_sets_device with d_out_ids = NULL -> (out_offsets as Python ints, total, longest)"""
    import torch

    n_sets = len(set_off) - 1
    so = torch.from_numpy(np.asarray(set_off, dtype=np.int64)).to(_device())
    out = torch.full((n_sets + 1,), -1, dtype=torch.int64, device=_device())
    total, longest = g.tokenize_sets_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[0].numel(), so.data_ptr(), n_sets,
                                            7, out.data_ptr(), 0, 0, max_length, _stream())
    torch.cuda.synchronize()
    return [int(x) for x in out.cpu().numpy().view(np.uint64)], total, longest


def test_region_sets_longer_than_two_to_the_32_ids(ga, indexes_a):
    """gtars_tokenize_sets_device as a sizing pass on the batch of (a), cut into sets of which one alone is longer than 2^32 ids
    (5.2e9), the sets behind it start beyond 2^32, two sets have queries but no hit and two have no query (the [unk] rule: 1
    id each).  out_offsets, *total and *longest against Python ints: unlimited, max_length 5, max_length 2^32 - 1 (the long
    set is clipped to 0xFFFFFFFF: the scan runs over a u32 count of all ones); a max_length of 2^32 or more is refused while a set
    is longer than it (2^32 and 5e9; no set reaches 2^40, which is answered exactly), and accepted on the same batch cut into sets
    below 2^32."""
    pool, counts, idx = W.case_a()
    off = W.batch_offsets(counts, idx)
    long_sets, short_sets = W.sets_c(counts, idx)
    g = indexes_a(KIND_BITS)
    d = _to_device(W.queries_of(pool, idx))
    for max_length in (0, 5, U32_MAX):
        (got, prof) = _profiled(ga, lambda: _sets_sizing(ga, g, d, long_sets, max_length))
        _note(("c", "long sets", max_length), prof)
        want = W.set_lengths(off, long_sets, max_length)
        assert got == want, (max_length, got, want)
    assert W.set_lengths(off, long_sets, U32_MAX)[2] == U32_MAX
    longest = W.set_lengths(off, long_sets, 0)[2]
    assert TWO32 < 5_000_000_000 < longest < 1 << 40
    for max_length in (TWO32, 5_000_000_000, 1 << 40):
        if longest > max_length:  # lengths clipped to 2^32 or more do not fit the scan's u32 counts: refused, not wrapped
            with pytest.raises(ValueError, match=r"2\^32 or more with a longer set"):
                _sets_sizing(ga, g, d, long_sets, max_length)
        else:  # (2^40: no set is that long -- nothing is clipped, the answer is that of max_length 0)
            got = _sets_sizing(ga, g, d, long_sets, max_length)
            assert got == W.set_lengths(off, long_sets, max_length) == W.set_lengths(off, long_sets, 0), (max_length, got)
        got = _sets_sizing(ga, g, d, short_sets, max_length)
        want = W.set_lengths(off, short_sets, max_length)
        assert got == want and want[1] == int(off[-1]) > TWO32, (max_length, got, want)


# ------------------------------------------------------------------------------------------ (d) IGD per-file totals past 2^32

@pytest.fixture(scope="module")
def igd_d(ga):
    uni, files, pool, counts, idx = W.case_d()
    g = ga.IgdIndex(uni[0], uni[1], uni[2], files, None, n_chrom=3, n_files=4)
    return g, pool, counts, idx


def _igd_count(g, d, min_overlap, binary):
    import torch

    hits = torch.full((4,), -1, dtype=torch.int64, device=_device())
    g.count_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[0].numel(), hits.data_ptr(), min_overlap, binary, _stream())
    torch.cuda.synchronize()
    return [int(x) for x in hits.cpu().numpy().view(np.uint64)]


IGD_ROUTES = {"default": {}, "sweep forced": {"GTARS_IGD_SWEEP_MIN": "1"},
              "sweep, no pieces view": {"GTARS_IGD_SWEEP_MIN": "1", "GTARS_IGD_NO_PIECES": "1"},
              "sweep, no pieces view, walked": {"GTARS_IGD_SWEEP_MIN": "1", "GTARS_IGD_NO_PIECES": "1", "GTARS_IGD_NO_RANK": "1"},
              "per query": {"GTARS_NO_IGD_SWEEP": "1"}}
# (in order?, min_overlap, binary).  Measured on this batch: the sweep 0.2 to 0.3 s through the view of pieces, 1.5 to 3 s in the rank
# form, 3.4 s (pairwise) and 5.2 s (binary) in the filtered walk; the per-query kernel 30 ms.  So: all eight calls per query; on the
# sweep the filtered walk once, pairwise (the binary count's totals stay below nq on every route); one call where a switch changes
# nothing (at 220 000 queries the library sweeps without being forced) or only takes the rank form away.
IGD_CALLS = [(o, mo, b) for o in (False, True) for mo in (1, 10) for b in (False, True)]
IGD_CALLS_AT = {"per query": IGD_CALLS, "sweep forced": [(False, 1, False)],
                "default": [(False, 1, False), (False, 1, True), (False, 10, False), (True, 1, False)],
                "sweep, no pieces view": [(False, 1, False), (True, 1, False)], "sweep, no pieces view, walked": [(False, 1, False)]}


@pytest.mark.parametrize("route", sorted(IGD_ROUTES))
def test_igd_per_file_totals_past_two_to_the_32(ga, monkeypatch, igd_d, route):
    """The stack of 70 000 records dealt 1 : 2 : 4 to three files, a fourth file on chromosomes 1 and 2 only, i32 coordinates; the
    batch of (a) at 220 000 queries (at 140 000 the largest file's total, 4/7 of 7.3e9, stays just below 2^32, and the filtered
    walk needs 107 375 full queries): per file 1.6e9, 3.3e9, 6.5e9 and a few thousand.  gtars_igd_count_device pairwise at
    min_overlap 1 (the MO1 forms; the rank form where the fact shows it) and 10 (the filtered walk; the one-base prefix queries
    drop out), the batch shuffled as built and in (chromosome, start) order, and the binary count of the same inputs, whose
    totals stay below nq (the two modes' counters do not mix).  Routes: as the library decides, the sweep forced, the sweep on a database without the view of pieces (the
    rank form) and the same without the rank form (whole records walked), the per-query kernel; which calls on which route:
    IGD_CALLS_AT."""
    g, pool, counts, idx = igd_d
    for k, v in IGD_ROUTES[route].items():
        monkeypatch.setenv(k, v)
    if "GTARS_IGD_NO_PIECES" in IGD_ROUTES[route]:
        # the stack's records are 1 Mbp long: min_overlap == 1 counts them through the view of pieces (the fact `igd_pieces_view`),
        # which has no rank form; without that view (the switch is read when a database is built) the records are counted whole
        uni, files = W.case_d()[:2]
        g = ga.IgdIndex(uni[0], uni[1], uni[2], files, None, n_chrom=3, n_files=4)
    idx = idx[:W.NQ_D_ONE]
    rank_ran = 0
    for ordered in (False, True):
        i = W.in_order(pool, idx) if ordered else idx
        d = _to_device(W.queries_of(pool, i))
        for mo in (1, 10):
            for binary in (False, True):
                if (ordered, mo, binary) not in IGD_CALLS_AT[route]:
                    continue
                got, prof = _profiled(ga, lambda: _igd_count(g, d, mo, binary))
                what = ("d", route, "in order" if ordered else "shuffled", "min_overlap", mo, "binary" if binary else "pairwise")
                _note(what, prof)
                want = W.batch_group_totals(counts[mo], i, binary)
                assert got == want, (what, got, want, [a - b for a, b in zip(got, want)])
                assert binary or max(want) > TWO32
                swept = any(k.startswith("k_igd_sweep") for k in prof)
                assert swept == (route != "per query"), (what, sorted(prof))
                rank_ran += "igd_sweep_rank_form" in prof
                assert any(k.startswith("k_igd_count<") for k in prof) == (route == "per query"), (what, sorted(prof))
                assert ("igd_pieces_view" in prof) == (mo == 1 and "no pieces" not in route), (what, sorted(prof))
                # the rank form: pairwise counts at min_overlap 1 on whole records -- it ran wherever it is not switched off
                assert ("igd_sweep_rank_form" in prof) == (route == "sweep, no pieces view"), (what, sorted(prof))
    print("PATH", ("d", route), "rank form ran in", rank_ran, "calls")


@pytest.mark.parametrize("binary", [False, True], ids=["pairwise", "binary"])
def test_igd_four_sets_in_one_pass_with_rows_past_two_to_the_32(ga, monkeypatch, igd_d, binary):
    """gtars_igd_count_sets_device: the batch of (d) at 320 000 queries as four sets of 150 000, 1 000, 150 000 and 19 000 queries
    that share one pass over the database (the fact `igd_sets_shared_pass`); two of the sets' rows hold a total past 2^32
    (4.5e9 in the largest file)."""
    import torch

    g, pool, counts, idx = igd_d
    monkeypatch.setenv("GTARS_IGD_SWEEP_MIN", "1")
    d = _to_device(W.queries_of(pool, idx))
    for mo in (1,):  # (the filtered walk of this batch costs 5 s: it runs once, in test_igd_per_file_totals_past_two_to_the_32)
        hits = torch.full((4 * 4,), -1, dtype=torch.int64, device=_device())

        def run():
            g.count_sets_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), W.SETS_D, hits.data_ptr(), mo, binary, _stream())
            torch.cuda.synchronize()
            return [[int(x) for x in row] for row in hits.cpu().numpy().view(np.uint64).reshape(4, 4)]

        got, prof = _profiled(ga, run)
        _note(("d", "count_sets", "min_overlap", mo, "binary" if binary else "pairwise"), prof)
        want = [W.batch_group_totals(counts[mo], idx[a:b], binary) for a, b in zip(W.SETS_D[:-1], W.SETS_D[1:])]
        assert got == want, (mo, got, want)
        assert "igd_sets_shared_pass" in prof, sorted(prof)
        if not binary and mo == 1:
            assert sum(max(r) > TWO32 for r in want) == 2


# ------------------------------------------------------------------------------------------------------------ (e) LOLA cells

def test_lola_contingency_cells_near_two_to_the_33(ga):
    """gtars_lola_contingency_device with supports and sizes near 2^33: a = user hits, b = universe hits - a, c = user size - a,
    d = universe size - a - b - c as signed 64-bit values, negative where the reference's are (enrichment.rs:214-220)."""
    import torch

    from gtars_amd._lib import check, lib

    big = 1 << 33
    user = [0, 1, U32_MAX, TWO32, TWO32 + 1, big - 1, big, big + 5, 3, big + 7]
    univ = [big, TWO32, TWO32, TWO32 - 1, big + 1, big - 1, big - 2, big + 5, 2 * big, 0]
    for user_size, universe_size in ((big - 3, 3 * big), (TWO32 + 1, big + 11), (5, big)):
        a, b, c, d = W.lola_cells(user, univ, user_size, universe_size)
        assert any(x < 0 for x in b) and any(x < 0 for x in c) and max(a) > big and max(d) > big
        assert any(x < 0 for x in d) == (universe_size < 3 * big)
        tu, tv = (torch.tensor(x, dtype=torch.int64, device=_device()) for x in (user, univ))
        out = [torch.full((len(user),), -1, dtype=torch.int64, device=_device()) for _ in range(4)]
        check(lib.gtars_lola_contingency_device(tu.data_ptr(), tv.data_ptr(), len(user), user_size, universe_size,
                                                *[o.data_ptr() for o in out], _stream()))
        torch.cuda.synchronize()
        for name, got, want in zip("abcd", out, (a, b, c, d)):
            assert got.cpu().tolist() == want, (name, user_size, universe_size, got.cpu().tolist(), want)
