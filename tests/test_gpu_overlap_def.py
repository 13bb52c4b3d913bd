"""GPU: ``gtars_amd.OverlapIndex`` against the definitions of tests/overlap_def.py -- the oracle is not in the loop.

The cases are those of tests/test_overlap_def_cpu.py (where the oracle meets the same model), both index kinds, every call of the
family, exact equality.  Then one mid-size case under every switch the parity tests use to force a kernel path, query counts at
the edges of the tokenizer's workgroup tile, and the run form of wide queries on a disjoint universe.  Which kernels a test
reached is printed from the profiling facts (``-s`` shows it) and asserted where the switch is about exactly that.
"""
import functools

import numpy as np
import pytest

import overlap_def as od
from overlap_def import KIND_AILIST, KIND_BITS
from overlap_def_cases import BOTH, CASES, NESTED, UNK, case, check_layout, check_queries, model_of

pytestmark = pytest.mark.gpu

# queries of one k_tok_lds tile as the default launch of a small batch instantiates it (launch_tokenize_lds: TPB = 1024 threads,
# 4 queries per thread; choose_rounds and choose_groups give one round and one wave group below 8192 queries per CU).  The
# library notes no fact about its tile: this constant follows the launch code by hand, and a change of that geometry has to
# move it -- the edge tests below only assert that k_tok_lds is the kernel that ran.
TILE = 1024 * 4
TILE_EDGES = (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
SHORT = dict(min_overlaps=(None, 5), index_side=(None,))  # the calls of check_queries once without and once with a filter


@pytest.fixture(scope="module")
def ga():
    import gtars_amd

    assert gtars_amd.device_count() > 0, "no MI355X visible: -m gpu tests must run on the GPU box"
    return gtars_amd


class DeviceCalls:
    """gtars_amd.OverlapIndex under the names check_layout / check_queries use.  Its IndexedRegionSet calls answer in vals."""

    row_vals = None

    def __init__(self, ga, d, kind, q=None):
        self.g = ga.OverlapIndex(d["c"], d["s"], d["e"], d["val"], n_chrom=d["n_chrom"], kind=kind)
        self.q = (d["qc"], d["qs"], d["qe"]) if q is None else q
        self.stored, self.max_len, self.headers = self.g.stored, self.g.max_len, self.g.sublist_offsets

    def tokenize(self):
        return self.g.tokenize(*self.q)

    def count_overlaps(self, mo):
        return self.g.count_overlaps(*self.q, mo)

    def any_overlaps(self, mo):
        return self.g.any_overlaps(*self.q, mo)

    def find_overlaps(self, mo):
        return self.g.find_overlaps(*self.q, mo)

    def find_overlap_indices(self, mo):
        return self.g.find_overlap_indices(*self.q, mo)

    def subset_by_overlaps(self, mo):
        return self.g.subset_by_overlaps(*self.q, mo)

    def subset_source_indices(self, mo):
        return self.g.subset_source_indices(*self.q, mo)


def with_facts(ga, f):
    """-> (f(), sorted names of the kernels and facts the library noted while f ran)"""
    L = ga._lib
    L.lib.gtars_prof_reset()
    L.lib.gtars_prof_enable(1)
    try:
        r = f()
        facts = sorted(L.prof_read())
    finally:
        L.lib.gtars_prof_enable(0)
    return r, facts


def run_case(ga, d, m, h, kind, label, **which):
    def body():
        impl = DeviceCalls(ga, d, kind, (h.qc, h.qs, h.qe))
        check_layout(impl, m)
        check_queries(impl, h, **which)

    _, facts = with_facts(ga, body)
    print(f"\n[{label}] kind={kind} n={len(d['c'])} nq={h.nq} hits={len(h.q)}: {' '.join(facts)}")
    return facts


# ------------------------------------------------------------- the cases of the CPU file, default switches


@pytest.mark.parametrize("kind", BOTH)
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_the_definitions(ga, name, kind):
    m, h = model_of(name, kind)
    assert len(h.q) <= 5_000_000
    run_case(ga, case(name), m, h, kind, name)


# ------------------------------------------------------------- a disjoint universe (ends ascend with the starts, nothing inverted)


@functools.lru_cache(maxsize=None)
def disjoint(explicit_ids=False, sizes=(1500, 1501, 1377), span=1_000_000):
    """3 chromosomes of ~1500 sorted disjoint intervals with touching neighbours and zero-length intervals: the shape the blocked
    structure serves with the run form (nothing inverted), with ids that follow from the position (val None) or explicit ones."""
    rng = np.random.default_rng(41)
    C_, S, E = [], [], []
    for c, n in enumerate(sizes):
        cuts = np.sort(rng.choice(span, 2 * n, replace=False))
        s, e = cuts[0::2].copy(), cuts[1::2].copy()
        k = rng.choice(n - 1, n // 40, replace=False)
        e[k] = s[k + 1]  # touching
        k = rng.choice(n, n // 60, replace=False)
        e[k] = s[k]  # zero-length
        C_.append(np.full(n, c)), S.append(s), E.append(e)
    c, s, e = (np.concatenate(x).astype(np.uint32) for x in (C_, S, E))
    val = rng.permutation(len(c)).astype(np.uint32) if explicit_ids else None
    return dict(c=c, s=s, e=e, val=val, n_chrom=3, span=span)


@functools.lru_cache(maxsize=None)
def disjoint_queries(nq, wide, in_order=False):
    """wide: 60 % of the queries span hundreds of intervals (a chromosome has one per ~670 bp), some a whole chromosome"""
    d = disjoint()
    rng = np.random.default_rng(43 + nq + int(wide))
    span = d["span"]
    qc = rng.integers(0, 3, nq)
    qs = rng.integers(0, span, nq)
    w = rng.integers(0, 900, nq)
    if wide:
        w = np.where(rng.random(nq) < 0.6, rng.integers(100_000, 400_000, nq), w)
    qe = qs + w
    k = rng.choice(nq, nq // 10, replace=False)  # touching: starts at some interval's end / ends at some interval's start
    i = rng.integers(0, len(d["c"]), len(k))
    qc[k], qs[k] = d["c"][i], d["e"][i]
    qe[k] = qs[k] + w[k]
    k2 = rng.choice(nq, nq // 10, replace=False)
    i = rng.integers(0, len(d["c"]), len(k2))
    qc[k2], qe[k2] = d["c"][i], d["s"][i]
    qs[k2] = np.maximum(qe[k2] - w[k2], 0)
    k = rng.choice(nq, nq // 20, replace=False)
    qe[k] = np.maximum(qs[k] - rng.integers(0, 4, len(k)), 0)  # zero-length and inverted
    if wide:
        k = rng.choice(nq, 12, replace=False)
        qs[k], qe[k] = 0, 0xFFFFFFFF  # everything on the chromosome
    k = rng.choice(nq, nq // 25, replace=False)
    qc[k] = np.where(rng.random(len(k)) < 0.5, UNK, 8)
    if in_order:
        o = np.lexsort((qs, qc))
        qc, qs, qe = qc[o], qs[o], qe[o]
    return tuple(np.ascontiguousarray(x, dtype=np.uint32) for x in (qc, qs, qe))


@functools.lru_cache(maxsize=None)
def disjoint_model(kind, explicit_ids, nq, wide, in_order=False):
    d = disjoint(explicit_ids)
    m = od.Model(d["c"], d["s"], d["e"], d["val"], n_chrom=3, kind=kind)
    return m, m.query(*disjoint_queries(nq, wide, in_order))


# ------------------------------------------------------------- every switch that forces a kernel path

# switch -> (environment, facts that must be noted on the Bits "mid" case, facts that must not).  The library notes a fact about
# the generic kernels, the build of the tokenizer and the AIList reorder, so those rows show that the switch changed the path.
# The rows that only name k_tok_lds check equality under the switch and nothing more, because no fact tells: the sampled top
# level (top_max_64), the host or device sort of the build (device_sort_*).  On this case three switches cannot change anything
# -- its universe has inverted intervals (no run form: tok_wide, tok_no_runs), explicit ids (no_affine_ids) and one-block units
# (tok_no_unit_records) -- they are here because every switch meets the mid-size case once; the universes where they do change
# the path are DISJOINT_SWITCHES and test_unit_records_on_a_universe_of_two_block_units below.
SWITCHES = {
    "generic_kernels": ({"GTARS_NO_LDS_PATH_FOR_TEST": "1"}, ["k_enum_fused<bits>", "k_count", "k_fill"], ["k_tok_lds", "k_count_lds"]),
    "top_max_64": ({"GTARS_TOP_MAX": "64"}, ["k_tok_lds"], []),
    "tok_wide": ({"GTARS_TOK_WIDE": "1"}, ["k_tok_lds"], []),
    "tok_narrow": ({"GTARS_TOK_NARROW": "1"}, ["k_tok_lds", "tok_build_narrow"], ["tok_build_wide"]),
    "tok_no_runs": ({"GTARS_TOK_NO_RUNS": "1"}, ["k_tok_lds"], ["tok_build_wide"]),
    "tok_no_unit_records": ({"GTARS_TOK_NO_UNIT_RECORDS": "1"}, ["k_tok_lds"], ["tok_unit_records"]),
    "no_affine_ids": ({"GTARS_NO_AFFINE_IDS": "1"}, ["k_tok_lds"], []),
    "ailist_no_reorder": ({"GTARS_AILIST_NO_REORDER": "1"}, ["k_tok_lds"], []),
    "ailist_reorder_any_depth": ({"GTARS_AILIST_REORDER_MAX_DEPTH": "1000000"}, ["k_tok_lds"], []),
    "device_sort_0": ({"GTARS_DEVICE_SORT": "0"}, ["k_tok_lds"], []),
    "device_sort_1": ({"GTARS_DEVICE_SORT": "1"}, ["k_tok_lds"], []),
}


@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_every_switch_meets_the_definitions(ga, monkeypatch, switch):
    """The index is built and queried under the switch: Bits on the 10 000 x 20 000 x 3 case, AIList on the two nested shapes."""
    env, must, must_not = SWITCHES[switch]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m, h = model_of("mid", KIND_BITS)
    facts = run_case(ga, case("mid"), m, h, KIND_BITS, f"{switch}: mid", **SHORT)
    assert all(f in facts for f in must) and not any(f in facts for f in must_not), facts
    for name in NESTED:
        m, h = model_of(name, KIND_AILIST)
        assert max(len(m.headers(ch)) for ch in range(m.n_chrom)) >= 2
        facts = run_case(ga, case(name), m, h, KIND_AILIST, f"{switch}: {name}", **SHORT)
        if switch == "ailist_reorder_any_depth":  # the hit set from the flat companion's LDS tokenizer, the order by k_ailist_reorder
            assert "ailist_nested_on_lds" in facts and "k_ailist_reorder" in facts, facts
        if switch in ("ailist_no_reorder", "generic_kernels"):
            assert "ailist_nested_on_lds" not in facts and "k_enum_fused<ailist>" in facts, facts


@pytest.mark.parametrize("kind", BOTH)
def test_sweep_form_on_batches_in_order(ga, kind):
    """batches sorted by (chromosome, start), once the sweep form's: k_tok_lds, forward (Bits) and reversed (a flat AIList)"""
    for explicit_ids in (False, True):
        m, h = disjoint_model(kind, explicit_ids, 6000, True, True)
        facts = run_case(ga, disjoint(explicit_ids), m, h, kind, f"in order: disjoint ids={explicit_ids}", **SHORT)
        assert "k_tok_lds" in facts and "tok_build_sweep" not in facts and "k_tok_sweep" not in facts, facts
    if kind == KIND_BITS:
        d = case("mid")
        o = np.lexsort((d["qs"], d["qc"]))
        m, _ = model_of("mid", kind)
        h = m.query(d["qc"][o], d["qs"][o], d["qe"][o])
        facts = run_case(ga, d, m, h, kind, "in order: mid", **SHORT)
        assert "k_tok_lds" in facts and "tok_build_sweep" not in facts, facts


# ------------------------------------------------------------- query counts at the tile's edges


@pytest.mark.parametrize("kind", BOTH)
@pytest.mark.parametrize("nq", TILE_EDGES)
def test_tile_edges_on_the_nested_case(ga, kind, nq):
    d = case("heavy", 2 * TILE + 1)
    m, _ = model_of("heavy", kind, 2 * TILE + 1)
    h = m.query(d["qc"][:nq], d["qs"][:nq], d["qe"][:nq])
    facts = run_case(ga, d, m, h, kind, f"tile edge {nq}: heavy", **SHORT)
    if kind == KIND_BITS:  # (the nested AIList index enumerates on the generic kernel or through its flat companion)
        assert "k_tok_lds" in facts, facts


@pytest.mark.parametrize("kind", BOTH)
@pytest.mark.parametrize("nq", TILE_EDGES)
def test_tile_edges_on_a_disjoint_universe(ga, kind, nq):
    qc, qs, qe = disjoint_queries(2 * TILE + 1, False)
    m, _ = disjoint_model(kind, False, 2 * TILE + 1, False)
    h = m.query(qc[:nq], qs[:nq], qe[:nq])
    facts = run_case(ga, disjoint(), m, h, kind, f"tile edge {nq}: disjoint", **SHORT)
    assert "k_tok_lds" in facts, facts


# ------------------------------------------------------------- the run form, and the other builds, on the disjoint universe

# switch -> (environment, explicit ids too?, facts that must be noted, facts that must not)
DISJOINT_SWITCHES = {
    "default": ({}, True, ["k_tok_lds"], []),
    "tok_wide": ({"GTARS_TOK_WIDE": "1"}, True, ["tok_build_wide"], []),
    "tok_narrow": ({"GTARS_TOK_NARROW": "1"}, True, ["tok_build_narrow"], ["tok_build_wide"]),
    "tok_no_runs": ({"GTARS_TOK_WIDE": "1", "GTARS_TOK_NO_RUNS": "1"}, False, ["tok_build_narrow"], ["tok_build_wide"]),
    "no_affine_ids": ({"GTARS_NO_AFFINE_IDS": "1", "GTARS_TOK_WIDE": "1"}, False, ["tok_build_wide"], []),
    "top_max_64": ({"GTARS_TOP_MAX": "64", "GTARS_TOK_WIDE": "1"}, False, ["tok_build_wide"], []),
    "generic_kernels": ({"GTARS_NO_LDS_PATH_FOR_TEST": "1"}, False, [], ["k_tok_lds"]),
}
# (no fact tells position-derived ids from id records, or a sampled top level from a full one: no_affine_ids and top_max_64
# check equality on a universe where the switch does change the index -- sorted input with val None, 2 190 blocks)


@pytest.mark.parametrize("kind", BOTH)
@pytest.mark.parametrize("switch", sorted(DISJOINT_SWITCHES))
def test_wide_queries_on_a_disjoint_universe(ga, monkeypatch, switch, kind):
    """queries that each span hundreds of intervals: the run form (GTARS_TOK_WIDE) and every other build of the tokenizer, with
    position-derived and explicit ids, forward (Bits) and reversed (AIList: one sub-list per chromosome)"""
    env, explicit_too, must, must_not = DISJOINT_SWITCHES[switch]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for explicit_ids in (False, True) if explicit_too else (False,):
        m, h = disjoint_model(kind, explicit_ids, 6000, True)
        if kind == KIND_AILIST:
            assert all(len(m.headers(ch)) == 1 for ch in range(3))
        assert int(np.median(h.count_overlaps()[h.count_overlaps() > 0])) >= 100 and len(h.q) <= 5_000_000
        facts = run_case(ga, disjoint(explicit_ids), m, h, kind, f"{switch}: disjoint ids={explicit_ids}", **SHORT)
        assert all(f in facts for f in must) and not any(f in facts for f in must_not), facts


# ------------------------------------------------------------- unit records

BIG = dict(sizes=(50_000, 50_001, 49_377), span=60_000_000)  # 74 690 blocks of two intervals: more than the LDS keys hold -> two-block units


@functools.lru_cache(maxsize=None)
def big_model():
    d = disjoint(False, **BIG)
    rng = np.random.default_rng(47)
    nq = 4000
    qc = rng.integers(0, 4, nq)
    qc[qc == 3] = UNK
    qs = rng.integers(0, BIG["span"], nq)
    w = np.where(rng.random(nq) < 0.2, rng.integers(0, 40_000, nq), rng.integers(0, 900, nq))  # up to ~30 intervals: past a record's eight
    k = rng.choice(nq, nq // 10, replace=False)
    i = rng.integers(0, len(d["c"]), len(k))
    qc[k], qs[k] = d["c"][i], d["e"][i]  # touching
    qe = qs + w
    k = rng.choice(nq, nq // 20, replace=False)
    qe[k] = np.maximum(qs[k] - rng.integers(0, 4, len(k)), 0)  # zero-length and inverted
    m = od.Model(d["c"], d["s"], d["e"], None, n_chrom=3, kind=KIND_BITS)
    return d, m, m.query(qc, qs, qe)


@pytest.mark.parametrize("records", ["unit", "block"])
def test_unit_records_on_a_universe_of_two_block_units(ga, monkeypatch, records):
    """149 378 sorted regions with position-derived ids: the narrow Bits tokenizer reads a 64-byte record per two-block unit
    (k_tok_lds<..., U64>), and per block under GTARS_TOK_NO_UNIT_RECORDS -- both equal the definitions, and the facts say
    that the switch changed the path"""
    monkeypatch.setenv("GTARS_TOK_NARROW", "1")
    if records == "block":
        monkeypatch.setenv("GTARS_TOK_NO_UNIT_RECORDS", "1")
    d, m, h = big_model()
    assert int(h.count_overlaps().max()) > 8
    facts = run_case(ga, d, m, h, KIND_BITS, f"{records} records: 149k regions", **SHORT)
    assert "k_tok_lds" in facts and "tok_build_narrow" in facts, facts
    if records == "unit":
        assert "tok_unit_records" in facts, facts
    else:
        assert "tok_block_records" in facts and "tok_unit_records" not in facts, facts
