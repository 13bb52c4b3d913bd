"""The streaming uniwig (csrc/uniwig_stream.hip, K24) on the device: k_sw_tile and the plan kernels by HIP events, the
achieved HBM fraction, the library call, a 16-thread numpy baseline and K11's k_cov_tile on the same rows, in one run.

  python tools/uniwig_stream_bench.py [--rows 1000000,10000000] [--reps 10] [--smoothsize 25] [--json profiles/uniwig_stream_bench.json]

Cases, all on hg38-shaped synthetic peaks (gtars_amd.synth.make_universe: sorted, karyotype order) with a score in
1 .. 1000 per row, start track at --smoothsize:
  sparse_<n>     max_gap 0, for every n of --rows
  gap100_<n0>    max_gap 100, the first n of --rows
  dense_chr1     max_gap -1 on the chr1 rows of the first n, chr1's size given
Per case: the rows are made resident, a StreamPlan is built --reps + 1 times with the library's profiling scopes on (every
launch between its own two HIP events; the median per scope name, k_sw_tile excluded, is "plan"), then the whole compacted
output is produced by one k_sw_tile launch chain --reps + 1 times between two HIP events (median).  HBM fraction of
k_sw_tile: (4 L out + 24 n in) / t / 8.0e12, L the compacted length, n the rows (an open and a close per row, each a u64
key and a u32 weight).  The library call is stream_counts on host columns, end to end.  The numpy baseline computes the
same output per chromosome (prefix maxima, segments, weighted bincount, cumsum) on 16 threads; the device's output is
compared with it, every position of every case.  K11: k_cov_tile's start track of the same rows with unit scores, every
chromosome to its full size (the dense path has no sparse form), through counts_device.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import gtars_amd.uniwig as U  # noqa: E402
from gtars_amd import _lib, synth  # noqa: E402

HBM_PEAK = 8.0e12


def numpy_run(start, score, size, m, max_gap):
    """one chromosome run of the start track -> (segment firsts, segment lengths, counts u32)"""
    c = start.astype(np.int64) + 1
    ws, we = np.maximum(1, c - m), c + m
    M, binc = np.maximum.accumulate(ws), np.maximum.accumulate(we)
    bx = np.r_[0, binc[:-1]]
    flag = np.zeros(len(ws), dtype=bool)
    flag[0] = True
    if max_gap >= 0:
        flag |= (M > bx + 1) & (M - bx - 1 > max_gap)
    seg = np.cumsum(flag) - 1
    heads = np.flatnonzero(flag)
    tails = np.r_[heads[1:] - 1, len(ws) - 1]
    first = M[heads] if max_gap >= 0 else np.ones(1, dtype=np.int64)
    last = binc[tails] if max_gap >= 0 else np.maximum(binc[tails], size)
    length = last + 1 - first
    off = np.r_[0, np.cumsum(length)]
    live = (score > 0) & (we >= M)
    w = np.where(live, score, 0).astype(np.float64)  # (exact below 2^53)
    A = off[seg] + M - first[seg]
    E = off[seg] + np.where(live, we + 1, M) - first[seg]
    total = int(off[-1])
    d = np.bincount(A, weights=w, minlength=total + 1) - np.bincount(E, weights=w, minlength=total + 1)
    return first, length, (np.cumsum(d[:total]).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)


def numpy_baseline(rows, score, sizes, m, max_gap):
    bounds = np.r_[0, np.flatnonzero(np.diff(rows["chrom"].astype(np.int64)) != 0) + 1, len(rows["chrom"])]

    def one(k):
        lo, hi = int(bounds[k]), int(bounds[k + 1])
        return numpy_run(rows["start"][lo:hi], score[lo:hi], int(sizes[int(rows["chrom"][lo])]), m, max_gap)

    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        parts = list(ex.map(one, range(len(bounds) - 1)))
    ms = (time.perf_counter() - t0) * 1e3
    return ms, np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts])


def median_scopes(samples):
    names = sorted({k for s in samples for k in s})
    return {k: float(np.median([s.get(k, {"total_ms": 0.0})["total_ms"] for s in samples])) for k in names}


def run_case(label, rows, score, m, max_gap, with_sizes, reps, dev):
    n = len(rows["chrom"])
    sizes = synth.CHROM_SIZES if with_sizes else np.zeros(synth.N_CHROM, dtype=np.int64)
    d = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).to(dev) for x in (rows["chrom"], rows["start"], rows["end"], score)]
    ptrs = [t.data_ptr() for t in d]
    plan = U.StreamPlan(*ptrs, n, sizes.astype(np.uint32), m, "start", max_gap)  # warm-up
    total = plan.total
    # the plan, scope by scope
    _lib.lib.gtars_prof_enable(1)
    samples = []
    for _ in range(reps + 1):
        plan.close()
        _lib.lib.gtars_prof_reset()
        plan = U.StreamPlan(*ptrs, n, sizes.astype(np.uint32), m, "start", max_gap)
        samples.append(_lib.prof_read())
    _lib.lib.gtars_prof_enable(0)
    scopes = median_scopes(samples[1:])
    plan_ms = sum(v for k, v in scopes.items() if k != "k_sw_tile")
    # k_sw_tile over the whole compacted output
    out = torch.empty(total + 16, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    times = []
    for _ in range(reps + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        plan.counts_device(0, total, out.data_ptr(), stream)
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    tile_ms = float(np.median(times[1:]))
    got = out[:total].cpu().numpy().view(np.uint32)
    # the numpy baseline, and the check of every position and segment
    base_ms, first, length, want = numpy_baseline(rows, score, sizes, m, max_gap)
    assert total == len(want), (label, total, len(want))
    assert np.array_equal(got, want), label
    keep = plan.seg_len > 0
    assert np.array_equal(plan.seg_first[keep], first.astype(np.uint32)) and np.array_equal(plan.seg_len[keep], length.astype(np.uint32)), label
    n_seg = int(keep.sum())
    plan.close()
    del out
    # the library call, host columns in, counts out
    cols = ((synth.CHROM_NAMES, rows["chrom"].astype(np.uint32)), rows["start"], rows["end"], score)
    size_map = dict(zip(synth.CHROM_NAMES, (int(s) for s in sizes))) if with_sizes else None
    t = time.perf_counter()
    track = U.stream_counts(cols, size_map, m, 1, "start", max_gap)
    lib_ms = (time.perf_counter() - t) * 1e3
    assert np.array_equal(track.counts, want), label
    del track
    return {"case": label, "rows": n, "max_gap": max_gap, "smoothsize": m, "segments": n_seg, "compacted_positions": total,
            "k_sw_tile_ms_median": tile_ms, "k_sw_tile_ms_min": float(min(times[1:])),
            "k_sw_tile_hbm_fraction": (4 * total + 24 * n) / (tile_ms * 1e-3) / HBM_PEAK, "plan_ms_median_sum_of_scopes": plan_ms,
            "plan_scopes_ms_median": scopes, "library_call_ms": lib_ms, "numpy_16_threads_ms": base_ms, "reps": reps,
            "checked": "every position and segment against the numpy baseline"}


def k11_same_rows(rows, m, reps, dev):
    """k_cov_tile's start track of the same rows, unit scores, every chromosome to its size"""
    plan = []
    for c in range(synth.N_CHROM):
        sel = rows["chrom"] == c
        if not sel.any():
            continue
        s1 = np.sort(rows["start"][sel].astype(np.uint32) + np.uint32(1))
        first, length = U.track_extent("start", s1, None, int(synth.CHROM_SIZES[c]), m)
        plan.append((torch.from_numpy(s1.view(np.int32)).to(dev), len(s1), first, length))
    out = torch.empty(max(p[3] for p in plan) + 16, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    times = []
    for _ in range(reps + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for d_s, n, first, length in plan:
            U.counts_device("start", d_s.data_ptr(), 0, n, m, first, length, out.data_ptr(), stream)
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    return {"k_cov_tile_ms_median": float(np.median(times[1:])), "positions": int(sum(p[3] for p in plan)), "chromosomes": len(plan)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--smoothsize", type=int, default=25)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    results = {"device": torch.cuda.get_device_name(0), "smoothsize": a.smoothsize, "cases": []}

    def emit(res):
        results["cases"].append(res)
        print(json.dumps(res), flush=True)
        if a.json:  # (written case by case: a run that is cut short leaves what it has)
            with open(a.json, "w") as fh:
                json.dump(results, fh, indent=1)

    sets = []
    for n in (int(x) for x in a.rows.split(",")):
        rows = synth.make_universe(n)
        score = (1 + synth.splitmix_stream(24, len(rows["chrom"])) % np.uint64(1000)).astype(np.uint32)
        sets.append((n, rows, score))
        res = run_case(f"sparse_{n}", rows, score, a.smoothsize, 0, False, a.reps, dev)
        res["k11_same_rows_unit_scores"] = k11_same_rows(rows, a.smoothsize, a.reps, dev)
        emit(res)
    n, rows, score = sets[0]
    emit(run_case(f"gap100_{n}", rows, score, a.smoothsize, 100, False, a.reps, dev))
    sel = rows["chrom"] == 0
    chr1 = {k: v[sel] for k, v in rows.items()}
    emit(run_case("dense_chr1", chr1, score[sel], a.smoothsize, -1, True, a.reps, dev))


if __name__ == "__main__":
    main()
