"""The batched tokenizer (csrc/tokbatch.hip, K15) against the per-set loops it replaces.

  python tools/tokbatch_bench.py [--universe 100000] [--batches 1000x10000,32x1000000] [--reps 10] [--loop-sets 64] [--json out.json]

The universe is bench.py's (synth.make_universe), a batch is B sets of synth.make_queries regions each.  Per batch, on
inputs that are resident on the device:

  batched ragged   Tokenizer.engine_index through gtars_tokenize_sets_device: one call for the batch
  batched padded   the same plus gtars_pad_sets_device at the longest set's width
  device loop      gtars_tokenize_device once per set on slices of the same resident columns (no [unk] patch, no padding)
  host loop        Tokenizer._encode_regions once per set on a prebuilt RegionSet -- what the library offered before; run on
                   the first --loop-sets sets and scaled to B (the sets are identically distributed)

Device times are HIP events around the calls (median of --reps, with min and max), wall times perf_counter around the same
calls.  The pack and pad kernels alone come from the library's profiling mode, on the batch with one set emptied so that the
pack runs, next to the tokenizer kernels of the same call.  Every result is checked in the run against the CPU oracle on a
sample of sets before anything is timed."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gtars_amd import _lib, engine, synth  # noqa: E402
from gtars.models import RegionSet  # noqa: E402
from gtars.tokenizers import Tokenizer  # noqa: E402

UNKNOWN = 0xFFFFFFFF


def timed(fn, reps):
    """(device ms by events, wall ms): medians with min and max over reps calls, after one warm-up"""
    fn()
    torch.cuda.synchronize()
    dev, wall = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        dev.append(e0.elapsed_time(e1))
    stat = lambda v: [float(np.median(v)), float(min(v)), float(max(v))]  # noqa: E731
    return stat(dev), stat(wall)


class Batch:
    def __init__(self, tok, u, n_sets, per_set, seed):
        q = synth.make_queries(u, n_sets * per_set, seed=seed)
        table = np.append(tok.chrom_ids(synth.CHROM_NAMES), np.uint32(UNKNOWN))
        self.c_u = q["chrom"]  # universe (oracle) ids
        self.c = table[np.minimum(q["chrom"], len(table) - 1)].astype(np.uint32)
        self.s, self.e = q["start"], q["end"]
        self.so = (np.arange(n_sets + 1, dtype=np.uint64) * np.uint64(per_set))
        self.B, self.n = n_sets, n_sets * per_set
        dev = torch.device("cuda", torch.cuda.current_device())
        self.d = [torch.from_numpy(a.view(np.int32)).to(dev) for a in (self.c, self.s, self.e)]
        self.d_so = torch.from_numpy(self.so.view(np.int64)).to(dev)
        self.off = torch.empty(n_sets + 1, dtype=torch.int64, device=dev)
        self.ids = torch.empty(2 * self.n + n_sets + 1024, dtype=torch.int32, device=dev)
        self.q_off = torch.empty(self.n + 1, dtype=torch.int64, device=dev)

    def with_set_emptied(self, b):
        """the same batch with set b's regions given to set b - 1: one empty set, so the pack runs"""
        other = Batch.__new__(Batch)
        other.__dict__.update(self.__dict__)
        so = self.so.copy()
        so[b] = so[b + 1]
        other.so = so
        other.d_so = torch.from_numpy(so.view(np.int64)).to(self.d_so.device)
        return other


def ragged(tok, bt, stream):
    return engine.tokenize_sets_device(tok.engine_index, bt.d[0].data_ptr(), bt.d[1].data_ptr(), bt.d[2].data_ptr(), bt.n, bt.d_so.data_ptr(),
                                       bt.B, tok.unk_token_id, bt.off.data_ptr(), bt.ids.data_ptr(), bt.ids.numel(), None, stream)


def check(tok, ref, bt, input_ids, mask, sample):
    """the batched results of the sampled sets against the oracle's Tokenizer::tokenize of each set alone"""
    off = bt.off.cpu().numpy().view(np.uint64)
    ids = bt.ids.cpu().numpy().view(np.uint32)
    W = input_ids.shape[1]
    for b in sample:
        lo, hi = int(bt.so[b]), int(bt.so[b + 1])
        _, want = ref.tokenize(bt.c_u[lo:hi], bt.s[lo:hi], bt.e[lo:hi])
        if len(want) == 0:
            want = np.array([tok.unk_token_id], dtype=np.uint32)
        got = ids[int(off[b]):int(off[b + 1])]
        assert np.array_equal(got, want), f"set {b}: ragged ids differ from the oracle"
        row, m = input_ids[b].cpu().numpy().view(np.uint32), mask[b].cpu().numpy()
        assert np.array_equal(row[:len(want)], want) and (row[len(want):] == tok.pad_token_id).all(), f"set {b}: padded row differs"
        assert m[:len(want)].all() and not m[len(want):].any() and len(row) == W, f"set {b}: mask differs"


def main():
    import oracle

    ap = argparse.ArgumentParser()
    ap.add_argument("--universe", type=int, default=100_000)
    ap.add_argument("--batches", default="1000x10000,32x1000000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--loop-sets", type=int, default=64)
    ap.add_argument("--json")
    a = ap.parse_args()
    u = synth.make_universe(a.universe)
    with tempfile.TemporaryDirectory() as d:
        ub = os.path.join(d, "universe.bed")
        with open(ub, "w") as fh:
            fh.write("".join(f"{synth.CHROM_NAMES[c]}\t{s}\t{e}\n" for c, s, e in zip(u["chrom"], u["start"], u["end"])))
        tok = Tokenizer(ub)
    ref = oracle.Index(u["chrom"], u["start"], u["end"], None, n_chrom=synth.N_CHROM)
    stream = torch.cuda.current_stream().cuda_stream
    dev = torch.device("cuda", torch.cuda.current_device())
    names = np.array(synth.CHROM_NAMES + ["chrUn_synthetic"])
    results = []
    for k, spec in enumerate(a.batches.split(",")):
        B, per = (int(x) for x in spec.split("x"))
        bt = Batch(tok, u, B, per, seed=40 + k)
        total, longest = ragged(tok, bt, stream)
        input_ids = torch.empty((B, longest), dtype=torch.int32, device=dev)
        mask = torch.empty((B, longest), dtype=torch.uint8, device=dev)

        def pad(b=bt):
            engine.pad_sets_device(b.off.data_ptr(), b.ids.data_ptr(), b.B, longest, tok.pad_token_id, input_ids.data_ptr(), mask.data_ptr(),
                                   "right", stream)

        pad()
        sample = sorted(set(np.linspace(0, B - 1, 8).astype(int).tolist()))
        check(tok, ref, bt, input_ids, mask, sample)
        # the batch with an empty set (the pack path), checked as well
        be = bt.with_set_emptied(B // 2)
        ragged(tok, be, stream)
        off_e = be.off.cpu().numpy().view(np.uint64)
        assert int(off_e[B // 2 + 1] - off_e[B // 2]) == 1 and int(be.ids[int(off_e[B // 2])]) == tok.unk_token_id, "the emptied set is not [unk]"
        lo, hi = int(be.so[B // 2 - 1]), int(be.so[B // 2])
        _, want = ref.tokenize(bt.c_u[lo:hi], bt.s[lo:hi], bt.e[lo:hi])
        assert np.array_equal(be.ids[int(off_e[B // 2 - 1]):int(off_e[B // 2])].cpu().numpy().view(np.uint32), want), "packed ids differ"
        ragged(tok, bt, stream)

        t_ragged = timed(lambda: ragged(tok, bt, stream), a.reps)
        t_padded = timed(lambda: (ragged(tok, bt, stream), pad()), a.reps)

        ix = tok.engine_index

        def device_loop():
            for b in range(B):
                lo, n = int(bt.so[b]), int(bt.so[b + 1] - bt.so[b])
                total_b = _lib.C.c_uint64()
                _lib.check(_lib.lib.gtars_tokenize_device(ix, bt.d[0].data_ptr() + 4 * lo, bt.d[1].data_ptr() + 4 * lo, bt.d[2].data_ptr() + 4 * lo,
                                                          n, bt.q_off.data_ptr(), bt.ids.data_ptr(), bt.ids.numel(), _lib.C.byref(total_b), stream))

        t_dev_loop = timed(device_loop, max(1, a.reps // 3))
        ragged(tok, bt, stream)  # (the loop overwrote the ids)

        n_loop = min(B, a.loop_sets)
        sets = [RegionSet.from_vectors(names[np.minimum(bt.c_u[int(bt.so[b]):int(bt.so[b + 1])], len(names) - 1)].tolist(),
                                       bt.s[int(bt.so[b]):int(bt.so[b + 1])], bt.e[int(bt.so[b]):int(bt.so[b + 1])]) for b in range(n_loop)]
        off = bt.off.cpu().numpy().view(np.uint64)
        first = tok._encode_regions(sets[0])
        assert np.array_equal(first, bt.ids[:int(off[1])].cpu().numpy().view(np.uint32)), "the single-set call differs from the batch"
        walls = []
        for _ in range(max(1, a.reps // 3)):
            t0 = time.perf_counter()
            for rs in sets:
                tok._encode_regions(rs)
            walls.append((time.perf_counter() - t0) * 1e3 * B / n_loop)
        host_loop = [float(np.median(walls)), float(min(walls)), float(max(walls))]

        # the kernels alone
        _lib.lib.gtars_prof_enable(1)
        try:
            _lib.lib.gtars_prof_reset()
            ragged(tok, be, stream)
            engine.pad_sets_device(be.off.data_ptr(), be.ids.data_ptr(), B, longest, tok.pad_token_id, input_ids.data_ptr(), mask.data_ptr(),
                                   "right", stream)
            prof = _lib.prof_read()
        finally:
            _lib.lib.gtars_prof_enable(0)
        ms = {k: v["total_ms"] for k, v in prof.items()}
        tok_ms = sum(v for k, v in ms.items() if not k.startswith("k_set_") and not k.startswith("scan"))
        row = {"sets": B, "regions_per_set": per, "ids": total, "longest": longest, "checks": "ok",
               "batched_ragged_device_ms": t_ragged[0], "batched_ragged_wall_ms": t_ragged[1],
               "batched_padded_device_ms": t_padded[0], "batched_padded_wall_ms": t_padded[1],
               "device_loop_device_ms": t_dev_loop[0], "device_loop_wall_ms": t_dev_loop[1],
               "host_loop_wall_ms_scaled": host_loop, "host_loop_sets_run": n_loop,
               "kernels_ms": ms, "tokenize_kernels_ms": tok_ms,
               "pack_fraction_of_tokenize": ms.get("k_set_pack", 0.0) / tok_ms if tok_ms else None,
               "pad_fraction_of_tokenize": ms.get("k_set_pad", 0.0) / tok_ms if tok_ms else None}
        results.append(row)
        print(json.dumps(row), flush=True)
        del bt, be, input_ids, mask
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
