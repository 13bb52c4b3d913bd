"""The cross-workgroup look-back of one-tile-per-workgroup tokenizer launches (tokenize_lds.hip, k_tok_lds<.., ONE>): the chained
look-back on eight copies of the state array, tile i reading copy i % 8 (GTARS_TOK_LOOKBACK=replicas, the default), next to the
one on the single state array that the pipelined launches use (GTARS_TOK_LOOKBACK=chain).  The copies lie in the scan workspace
behind a one-tile launch's state[], where a pipelined launch's longer state[] runs through them.  Everything is compared bit for
bit against the oracle on the 20k universe of test_gpu_tok_tail.py; which form ran is read from the profiling fact, never assumed."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from oracle import KIND_AILIST, KIND_BITS

pytestmark = pytest.mark.gpu

UNK = 0xFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096
FORMS = ("chain", "replicas")  # every value of GTARS_TOK_LOOKBACK the tree keeps
DEFAULT_FORM = "replicas"


@pytest.fixture(scope="module")
def ga():
    import gtars_amd

    assert gtars_amd.device_count() > 0, "no MI355X visible: -m gpu tests must run on the GPU box"
    return gtars_amd


class World:
    """The 20k universe, its device index and its oracle, and per batch size the queries (unknown chromosomes among them), their
    device copies and the oracle's answer: each built once, never changed."""

    def __init__(self, ga):
        from gtars_amd import synth

        self.ga, self.synth = ga, synth
        self.u = synth.make_universe(20_000)
        self.g = ga.OverlapIndex(self.u["chrom"], self.u["start"], self.u["end"], n_chrom=synth.N_CHROM)
        self.o = oracle.Index(self.u["chrom"], self.u["start"], self.u["end"], None, n_chrom=synth.N_CHROM)
        self._cases = {}

    def case(self, nq):
        import torch

        if nq not in self._cases:
            q = self.synth.make_queries(self.u, nq, seed=nq)
            qc = q["chrom"].copy()
            qc[::53] = UNK
            off_o, ids_o = self.o.tokenize(qc, q["start"], q["end"])
            d = [torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to("cuda:0") for x in (qc, q["start"], q["end"])]
            self._cases[nq] = ((qc, q["start"], q["end"]), d, off_o, ids_o)
        return self._cases[nq]

    def launch(self, nq, sync=True):
        """one gtars_tokenize_device call into fresh sentinel-filled buffers -> (H, offsets, ids)"""
        import torch

        _, d, _, ids_o = self.case(nq)
        off = torch.full((nq + 1,), -3, dtype=torch.int64, device="cuda:0")
        ids = torch.full((len(ids_o) + 8,), -7, dtype=torch.int32, device="cuda:0")
        h = self.g.tokenize_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), nq, off.data_ptr(), ids.data_ptr(), ids.numel(),
                                   torch.cuda.current_stream().cuda_stream, sync=sync)
        return h, off, ids

    def check(self, nq, what=""):
        _, _, off_o, ids_o = self.case(nq)
        h, off, ids = self.launch(nq)
        assert h == len(ids_o), (nq, what, h, len(ids_o))
        assert np.array_equal(off.cpu().numpy().view(np.uint64), off_o), (nq, what)
        assert np.array_equal(ids[:h].cpu().numpy().view(np.uint32), ids_o), (nq, what)
        assert bool((ids[h:] == -7).all()), (nq, what)


@pytest.fixture(scope="module")
def world(ga):
    return World(ga)


def _profiled(ga, fn):
    _lib = ga._lib
    _lib.lib.gtars_prof_reset()
    _lib.lib.gtars_prof_enable(1)
    try:
        r = fn()
        prof = _lib.prof_read()
    finally:
        _lib.lib.gtars_prof_enable(0)
    return r, prof


class _Env:
    """GTARS_* switches for the block, read by the library through a fresh snapshot; the old values come back afterwards"""

    def __init__(self, ga, **kv):
        self.ga, self.kv, self.old = ga, kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = os.environ.get(k)
            os.environ[k] = v
        self.ga.reload_env()

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        self.ga.reload_env()


EDGE_TILES = (1, 2, 3, 63, 64, 65, 66, 128, 129, 192, 193, 245, 255, 256)
EDGE_SIZES = [TILE * t for t in EDGE_TILES] + [n for t in (2, 65, 256) for n in (TILE * t - 1, TILE * (t - 1) + 1)]


@pytest.mark.parametrize("nq", EDGE_SIZES)
def test_tile_counts_at_the_row_and_window_edges(world, nq):
    """T tiles around the 64-granule windows of the look-back and the 256 granules of a copy: full last tiles, a last tile one
    query short and a last tile of one query."""
    _, prof = _profiled(world.ga, lambda: world.check(nq))
    if (nq + TILE - 1) // TILE <= 256:
        assert "tok_lookback_" + DEFAULT_FORM in prof, sorted(prof)


def test_workspace_growth_and_reuse(world):
    """257 tiles (the pipelined build on a 256-CU device: its state[] reaches further than a one-tile launch's), then 256 tiles in
    one-tile form on the same workspace."""
    world.check(TILE * 257, "pipelined")
    world.check(TILE * 256, "one tile per workgroup")
    world.check(TILE * 257, "pipelined again")


@pytest.mark.parametrize("form", FORMS)
def test_every_selectable_lookback_form(world, form):
    with _Env(world.ga, GTARS_TOK_LOOKBACK=form):
        for t in (3, 66, 245):
            _, prof = _profiled(world.ga, lambda: world.check(TILE * t, form))
            assert "tok_lookback_" + form in prof and prof["tok_lookback_" + form]["launches"] == 1, (form, t, sorted(prof))
            assert not [k for k in prof if k.startswith("tok_lookback_") and k != "tok_lookback_" + form], sorted(prof)


def test_stale_granules_and_epoch_wrap(world):
    """Forty launches whose tile counts cycle through 245, 7, 130, 1, 256, 64 on one workspace: every copy holds granules of
    earlier launches with more tiles and fewer.  Then 16,500 launches of two tiles, so that the 14-bit epoch wraps and the
    workspace is cleared in between, the last one checked, and 245 tiles again."""
    import torch

    cycle = (245, 7, 130, 1, 256, 64)
    for k in range(40):
        world.check(TILE * cycle[k % len(cycle)], "launch %d" % k)
    nq = 2 * TILE
    _, d, _, ids_o = world.case(nq)
    off = torch.empty(nq + 1, dtype=torch.int64, device="cuda:0")
    ids = torch.empty(len(ids_o) + 8, dtype=torch.int32, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    for _ in range(16_500):
        world.g.tokenize_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), nq, off.data_ptr(), ids.data_ptr(), ids.numel(), st, sync=False)
    world.check(nq, "after the wrap")
    world.check(TILE * 245, "after the wrap")


def test_pipelined_and_one_tile_launches_interleaved(world):
    """1.3M queries (318 tiles: the pipelined build, whose state[] runs into the first copy) and 1M queries (245 tiles, one per
    workgroup) in turn on the same workspace."""
    for k in range(3):
        world.check(1_300_000, "pipelined %d" % k)
        world.check(1_000_000, "one tile per workgroup %d" % k)


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
import gtars_amd, oracle
from gtars_amd import synth
u = synth.make_universe(20_000)
g = gtars_amd.OverlapIndex(u["chrom"], u["start"], u["end"], n_chrom=synth.N_CHROM)
o = oracle.Index(u["chrom"], u["start"], u["end"], None, n_chrom=synth.N_CHROM)
ok = True
for t in (3, 66):
    nq = 4096 * t
    q = synth.make_queries(u, nq, seed=nq)
    qc = q["chrom"].copy()
    qc[::53] = 0xFFFFFFFF
    off_o, ids_o = o.tokenize(qc, q["start"], q["end"])
    off_g, ids_g = g.tokenize(qc, q["start"], q["end"])
    ok = ok and np.array_equal(off_g, off_o) and np.array_equal(ids_g, ids_o)
print("LOOKBACK_PARITY", ok)
"""


@pytest.mark.parametrize("form", FORMS)
def test_helping_path(ga, form):
    """Spin limit 0 (own process: the switch is read once): every look-back wait counts the missing tile itself and hands the
    count on, on 3 and 66 tiles."""
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], env=dict(os.environ, GTARS_TOK_SPIN_LIMIT="0", GTARS_TOK_LOOKBACK=form),
                       capture_output=True, text=True, timeout=600)
    assert "LOOKBACK_PARITY True" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_chained_launches_start_at_the_running_total(world):
    """The host pipeline cut into three chunks of 66 tiles (GTARS_PIPE_CHUNKS): each chunk is a one-tile launch, the second and
    third with a device-resident base (d_base) that enters through tile 0's inclusive prefix, in every copy."""
    nq = 3 * 66 * TILE
    (qc, qs, qe), _, off_o, ids_o = world.case(nq)
    with _Env(world.ga, GTARS_PIPE_CHUNKS="3"):
        (off_g, ids_g), prof = _profiled(world.ga, lambda: world.g.tokenize(qc, qs, qe))
    n = prof["tok_lookback_" + DEFAULT_FORM]["launches"]  # (a batch whose ids outgrow the first buffer is run a second time)
    assert n in (3, 6) and prof["k_tok_lds"]["launches"] == n, prof
    assert np.array_equal(off_g, off_o) and np.array_equal(ids_g, ids_o)


def test_ailist_order_explicit_ids_and_min_overlap(world):
    """66 tiles on the other builds of the one-tile kernel: explicit (shuffled) ids, AIList order (a query's ids descending) and
    the min-overlap filter of 20."""
    u = world.u
    shuffled = np.random.default_rng(77).permutation(len(u["chrom"])).astype(np.uint32)
    nq = 66 * TILE
    (qc, qs, qe), _, _, _ = world.case(nq)
    n_chrom = int(u["chrom"].max()) + 1
    for val, kind in ((shuffled, KIND_BITS), (shuffled, KIND_AILIST), (None, KIND_AILIST)):
        g = world.ga.OverlapIndex(u["chrom"], u["start"], u["end"], val, n_chrom=n_chrom, kind=kind)
        o = oracle.Index(u["chrom"], u["start"], u["end"], val, n_chrom=n_chrom, kind=kind)
        off_o, ids_o = o.tokenize(qc, qs, qe)
        (off_g, ids_g), prof = _profiled(world.ga, lambda: g.tokenize(qc, qs, qe))
        assert "tok_lookback_" + DEFAULT_FORM in prof, (kind, sorted(prof))
        assert np.array_equal(off_g, off_o) and np.array_equal(ids_g, ids_o), kind
        fo = o.find_overlaps_regions(qc, qs, qe, 20)
        fg = g.find_overlaps(qc, qs, qe, 20)
        assert all(np.array_equal(a, b) for a, b in zip(fg, fo)), (kind, "min_overlap")
