"""The tail of a tokenizer launch behind its count phase (tokenize_lds.hip): wave 0's staging in front of the scan barrier
in one-tile-per-group launches, and the dense form of the offset stores (a full wave's 256 offsets as two stores of
1 KiB).  Everything is compared bit for bit against the oracle, as test_gpu_parity.py does."""
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


@pytest.fixture(scope="module")
def ga():
    import gtars_amd

    assert gtars_amd.device_count() > 0, "no MI355X visible: -m gpu tests must run on the GPU box"
    return gtars_amd


@pytest.fixture(scope="module")
def world(ga):
    """The 20k universe, its device index and its oracle: built once, never changed."""
    from gtars_amd import synth

    u = synth.make_universe(20_000)
    g = ga.OverlapIndex(u["chrom"], u["start"], u["end"], n_chrom=synth.N_CHROM)
    o = oracle.Index(u["chrom"], u["start"], u["end"], None, n_chrom=synth.N_CHROM)
    return u, g, o


def _queries(u, nq):
    from gtars_amd import synth

    q = synth.make_queries(u, nq, seed=nq)
    qc = q["chrom"].copy()
    qc[::53] = UNK
    return qc, q["start"], q["end"]


def _dev(*arrays):
    import torch

    return [torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to("cuda:0") for x in arrays]


@pytest.mark.parametrize("nq", [1, 127, 128, 129, 255, 256, 257, 4095, 4096, 4097, 4351])
def test_dense_store_edges(ga, world, nq):
    """Batch sizes around a wave's 256 queries and a tile's 4096: full waves take the dense stores, the batch's last partial wave
    the lane-by-lane ones; `offsets` 16-byte aligned and 8 bytes off (the scalar path); `ids` at element offsets 0..3."""
    import torch

    u, g, o = world
    qc, qs, qe = _queries(u, nq)
    off_o, ids_o = o.tokenize(qc, qs, qe)
    h = len(ids_o)
    d = _dev(qc, qs, qe)
    st = torch.cuda.current_stream().cuda_stream
    for off_shift in (0, 1):  # u64 elements: byte offsets 0 and 8 from a 16-byte-aligned base
        for ids_shift in (0, 1, 2, 3):
            off_buf = torch.full((nq + 4,), -3, dtype=torch.int64, device="cuda:0")
            ids_buf = torch.full((h + 16,), -7, dtype=torch.int32, device="cuda:0")
            assert off_buf.data_ptr() % 16 == 0 and ids_buf.data_ptr() % 16 == 0
            offsets, ids = off_buf[off_shift:], ids_buf[ids_shift:]
            got = g.tokenize_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), nq, offsets.data_ptr(), ids.data_ptr(), h + 8, st,
                                    sync=True)
            assert got == h, (nq, off_shift, ids_shift)
            assert np.array_equal(offsets[: nq + 1].cpu().numpy().view(np.uint64), off_o), (nq, off_shift, ids_shift)
            assert np.array_equal(ids[:h].cpu().numpy().view(np.uint32), ids_o), (nq, off_shift, ids_shift)
            assert bool((off_buf[:off_shift] == -3).all()) and bool((off_buf[off_shift + nq + 1:] == -3).all())
            assert bool((ids_buf[:ids_shift] == -7).all()) and bool((ids_buf[ids_shift + h:] == -7).all())


def test_nothing_outside_the_result_is_written(ga, world):
    """Sentinel words in front of and behind both buffers; capacities H, H - 1, one inside the first wave's ids that is no multiple
    of 4, and exactly offsets[256]: offsets complete, ids exact up to the capacity, every sentinel intact."""
    import torch

    u, g, o = world
    nq = 4351
    qc, qs, qe = _queries(u, nq)
    off_o, ids_o = o.tokenize(qc, qs, qe)
    h = len(ids_o)
    first_wave = int(off_o[256])
    inside = (first_wave // 2) | 1
    assert 0 < inside < first_wave and inside % 4 != 0
    d = _dev(qc, qs, qe)
    st = torch.cuda.current_stream().cuda_stream
    G = 64  # guard words on each side (multiples of 16 bytes: the buffers stay aligned)
    for capn in (h, h - 1, inside, first_wave):
        off_buf = torch.full((G + nq + 1 + G,), -3, dtype=torch.int64, device="cuda:0")
        ids_buf = torch.full((G + h + G,), -7, dtype=torch.int32, device="cuda:0")
        offsets, ids = off_buf[G:], ids_buf[G:]
        call = lambda: g.tokenize_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), nq, offsets.data_ptr(), ids.data_ptr(), capn,
                                         st, sync=True)
        if capn < h:
            with pytest.raises(ga.CapacityError):
                call()
        else:
            assert call() == h
        assert np.array_equal(offsets[: nq + 1].cpu().numpy().view(np.uint64), off_o), capn
        assert np.array_equal(ids[:capn].cpu().numpy().view(np.uint32), ids_o[:capn]), capn
        assert bool((ids_buf[G + capn:] == -7).all()) and bool((ids_buf[:G] == -7).all()), capn
        assert bool((off_buf[:G] == -3).all()) and bool((off_buf[G + nq + 1:] == -3).all()), capn


def _dense_case(nq, seed=77):
    """The dense single-chromosome universe of the geometries test: 30k intervals in 200 kbp (a wave's ids exceed its stage buffer)."""
    rng = np.random.default_rng(seed)
    s = np.sort(rng.integers(0, 200_000, 30_000)).astype(np.uint32)
    e = s + rng.integers(50, 400, 30_000).astype(np.uint32)
    qs = rng.integers(0, 200_000, nq).astype(np.uint32)
    qe = qs + rng.integers(1, 300, nq).astype(np.uint32)
    return np.zeros(30_000, dtype=np.uint32), s, e, np.zeros(nq, dtype=np.uint32), qs, qe


@pytest.mark.parametrize("nq", [4097, 8193])
def test_wave0_over_its_stage_buffer(ga, nq):
    """Wave 0's ids exceed the stage buffer: the early staging declines and the write phase stores the ids directly."""
    c, s, e, qc, qs, qe = _dense_case(nq)
    g = ga.OverlapIndex(c, s, e, None, n_chrom=1)
    o = oracle.Index(c, s, e, None, n_chrom=1)
    off_o, ids_o = o.tokenize(qc, qs, qe)
    off_g, ids_g = g.tokenize(qc, qs, qe)
    assert np.array_equal(off_g, off_o) and np.array_equal(ids_g, ids_o)


_CHILD = r"""
import sys, numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import gtars_amd, oracle
from gtars_amd import synth
from test_gpu_tok_tail import _dense_case
ok = True
if %r == "dense":
    for nq in (4097, 8193):
        c, s, e, qc, qs, qe = _dense_case(nq)
        g = gtars_amd.OverlapIndex(c, s, e, None, n_chrom=1)
        o = oracle.Index(c, s, e, None, n_chrom=1)
        off_o, ids_o = o.tokenize(qc, qs, qe)
        off_g, ids_g = g.tokenize(qc, qs, qe)
        ok = ok and np.array_equal(off_g, off_o) and np.array_equal(ids_g, ids_o)
u = synth.make_universe(20_000)
g = gtars_amd.OverlapIndex(u["chrom"], u["start"], u["end"], n_chrom=synth.N_CHROM)
o = oracle.Index(u["chrom"], u["start"], u["end"], None, n_chrom=synth.N_CHROM)
for nq in (4097, 50_001):
    q = synth.make_queries(u, nq, seed=nq)
    qc = q["chrom"].copy()
    qc[::53] = 0xFFFFFFFF
    off_o, ids_o = o.tokenize(qc, q["start"], q["end"])
    off_g, ids_g = g.tokenize(qc, q["start"], q["end"])
    ok = ok and np.array_equal(off_g, off_o) and np.array_equal(ids_g, ids_o)
print("TAIL_PARITY", ok)
"""


def _child(kind, **env):
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, os.path.join(ROOT, "tests"), kind)], env=dict(os.environ, **env),
                       capture_output=True, text=True, timeout=600)
    assert "TAIL_PARITY True" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_wave0_with_a_small_stage_buffer(ga):
    """The stage buffer forced to its smallest size (own process: the switch is read once): waves whose ids do not fit -- wave 0's
    early staging among them -- decline, the others stage; dense and ordinary universes."""
    _child("dense", GTARS_TOK_STAGE="128")


def test_helping_path_on_the_new_tail(ga):
    """Every look-back wait counts the missing tile itself (spin limit 0, own process) at 50,001 queries: the helping wave 0 has
    staged its ids before the scan barrier, and the help must not disturb them."""
    _child("plain", GTARS_TOK_SPIN_LIMIT="0")


def test_ailist_order_explicit_ids_and_min_overlap(ga, world):
    """nq = 4097 (one full tile and a one-query tile) on the index kinds of the geometries test: ids from the position, explicit
    (shuffled) ids, AIList order (a query's ids descending), and the min-overlap filter of 20."""
    u, _, _ = world
    rng = np.random.default_rng(77)
    shuffled = rng.permutation(len(u["chrom"])).astype(np.uint32)
    nq = 4097
    qc, qs, qe = _queries(u, nq)
    n_chrom = int(u["chrom"].max()) + 1
    for val, kind in ((None, KIND_BITS), (shuffled, KIND_BITS), (shuffled, KIND_AILIST), (None, KIND_AILIST)):
        g = ga.OverlapIndex(u["chrom"], u["start"], u["end"], val, n_chrom=n_chrom, kind=kind)
        o = oracle.Index(u["chrom"], u["start"], u["end"], val, n_chrom=n_chrom, kind=kind)
        off_o, ids_o = o.tokenize(qc, qs, qe)
        off_g, ids_g = g.tokenize(qc, qs, qe)
        assert np.array_equal(off_g, off_o) and np.array_equal(ids_g, ids_o), kind
        fo = o.find_overlaps_regions(qc, qs, qe, 20)
        fg = g.find_overlaps(qc, qs, qe, 20)
        assert all(np.array_equal(a, b) for a, b in zip(fg, fo)), (kind, "min_overlap")
