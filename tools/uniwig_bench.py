"""Coverage tracks (csrc/uniwig.hip, K11) on the device: kernel time, achieved HBM fraction, the library call, the
bedGraph path, and a 16-thread numpy baseline, on hg38-shaped synthetic sets.

  python tools/uniwig_bench.py [--rows 100000,1000000,10000000] [--reps 10] [--smoothsize 25] [--json out.json]

Per set (gtars_amd.synth.make_universe rows, and a pile-up set: the 1e6 set with 1 % of its rows inside one 10 kbp
window of chr1): the start, end and core tracks of every chromosome at --smoothsize, launched through the device entry
(sorted columns resident, one output buffer), timed by HIP events after a warm-up, median of --reps; the HBM fraction
(4 L tracks + 8 n tracks) / t / 8.0e12 with L the genome's reported positions and n the rows.  Every track of every
chromosome is checked on the device against bincount + cumsum of the same events (torch), and the tracks of the two
smallest chromosomes on the host against the closed form by np.searchsorted.  The whole library call
(start_end_counts: columns in, sort, track, counts out) and the bedGraph path (compress_counts: only the runs come back)
are timed on chr1.  The numpy baseline (bincount + cumsum per chromosome, 16 threads) runs on the 1e6 set in the same run.
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
from gtars_amd import synth  # noqa: E402

HBM_PEAK = 8.0e12


def chromosomes(rows):
    """-> [(name, size, sorted start + 1, sorted end)] of the chromosomes that have rows"""
    out = []
    for c in range(synth.N_CHROM):
        sel = rows["chrom"] == c
        if sel.any():
            out.append((synth.CHROM_NAMES[c], int(synth.CHROM_SIZES[c]), np.sort(rows["start"][sel].astype(np.uint32) + np.uint32(1)),
                        np.sort(rows["end"][sel].astype(np.uint32))))
    return out


def track_args(kind, s1, e, m):
    """-> (opens column, closes column or None, smoothsize, window opens a, window closes e) of a track"""
    if kind == "core":
        return s1, e, 0, s1.astype(np.int64), e.astype(np.int64)
    p = s1 if kind == "start" else e
    return p, None, m, np.maximum(1, p.astype(np.int64) - m), p.astype(np.int64) + m + 1


def closed_form_host(a, e, first, length):
    pos = np.arange(first, first + length, dtype=np.int64)
    return (np.searchsorted(a, pos, side="right") - np.searchsorted(e, pos, side="right")).astype(np.uint32)


def numpy_baseline(chroms, m):
    def one(job):
        (_, size, s1, e), kind = job
        _, _, _, a, c = track_args(kind, s1, e, m)
        first, last = int(a[0]), max(size, int(a[-1]) - 1)
        d = np.bincount(a - first, minlength=last - first + 2)[:last - first + 1].astype(np.int32)
        c = c[c <= last] - first
        d -= np.bincount(c, minlength=last - first + 1).astype(np.int32)
        return np.cumsum(d, dtype=np.int32).astype(np.uint32)[-1]

    jobs = [(ch, k) for ch in chroms for k in ("start", "end", "core")]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(one, jobs))
    return (time.perf_counter() - t0) * 1e3


def run_set(label, rows, m, reps, dev):
    chroms = chromosomes(rows)
    n = sum(len(c[2]) for c in chroms)
    cols = [(torch.from_numpy(s1.view(np.int32)).to(dev), torch.from_numpy(e.view(np.int32)).to(dev)) for _, _, s1, e in chroms]
    plan, total_len = [], 0
    for (name, size, s1, e), (d_s, d_e) in zip(chroms, cols):
        for kind in ("start", "end", "core"):
            o, c, mm, a, ee = track_args(kind, s1, e, m)
            first, length = U.track_extent(kind, o, c, size, mm)
            d_o = d_s if o is s1 else d_e
            plan.append((name, kind, d_o, d_e if c is not None else None, len(s1), mm, first, length, a, ee))
            total_len += length
    out = torch.empty(max(p[7] for p in plan) + 16, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def launch(p):
        U.counts_device(p[1], p[2].data_ptr(), p[3].data_ptr() if p[3] is not None else 0, p[4], p[5], p[6], p[7], out.data_ptr(), stream)

    # correctness: every track on the device against bincount + cumsum, the two smallest chromosomes on the host
    small = sorted({p[0] for p in plan}, key=lambda nme: synth.CHROM_SIZES[synth.CHROM_NAMES.index(nme)])[:2]
    for p in plan:
        launch(p)
        first, length = p[6], p[7]
        a = torch.from_numpy(p[8] - first).to(dev)
        e = torch.from_numpy(p[9][p[9] < first + length] - first).to(dev)
        d = torch.bincount(a, minlength=length)[:length] - torch.bincount(e, minlength=length)[:length]
        want = torch.cumsum(d, 0).to(torch.int32)
        assert torch.equal(out[:length], want), (label, p[0], p[1])
        if p[0] in small:
            assert np.array_equal(out[:length].cpu().numpy().view(np.uint32), closed_form_host(p[8], p[9], first, length)), (label, p[0], p[1])
        del a, e, d, want
    torch.cuda.synchronize()
    times = []
    for _ in range(reps + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for p in plan:
            launch(p)
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    ms = float(np.median(times[1:]))
    bytes_moved = 4 * total_len + 8 * n * 3
    res = {"set": label, "rows": n, "chromosomes": len(chroms), "tracks": 3, "positions_all_tracks": total_len,
           "kernel_ms_median": ms, "kernel_ms_min": float(min(times[1:])), "reps": reps,
           "hbm_fraction": bytes_moved / (ms * 1e-3) / HBM_PEAK, "checked_on_device": len(plan), "checked_on_host": small}
    # the library call and the bedGraph path on chr1
    name, size, s1, e = chroms[0]
    U.start_end_counts(s1, size, m)
    t = time.perf_counter()
    counts, _ = U.start_end_counts(s1, size, m)
    res["library_call_chr1_start_ms"] = (time.perf_counter() - t) * 1e3
    res["library_call_chr1_rows"] = len(s1)
    del counts
    t = time.perf_counter()
    runs = U.compress_counts("start", s1, None, size, m, max(0, int(s1[0]) - m))
    res["bedgraph_chr1_start_ms"] = (time.perf_counter() - t) * 1e3
    res["bedgraph_chr1_runs"] = len(runs[0])
    return res, chroms


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", default="100000,1000000,10000000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--smoothsize", type=int, default=25)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    results = {"device": torch.cuda.get_device_name(0), "smoothsize": a.smoothsize, "sets": []}
    for n in (int(x) for x in a.rows.split(",")):
        rows = synth.make_universe(n)
        res, chroms = run_set(f"hg38_{n}", rows, a.smoothsize, a.reps, dev)
        if n == 1_000_000:
            res["numpy_16_threads_ms"] = numpy_baseline(chroms, a.smoothsize)
            pile = {k: v.copy() for k, v in rows.items()}
            idx = np.flatnonzero(pile["chrom"] == 0)[:: max(1, (pile["chrom"] == 0).sum() // (n // 100))][: n // 100]
            rng = np.random.default_rng(1)
            pile["start"][idx] = (50_000_000 + rng.integers(0, 10_000, len(idx))).astype(pile["start"].dtype)
            pile["end"][idx] = pile["start"][idx] + 150
            results["sets"].append(res)
            print(json.dumps(res), flush=True)
            res, _ = run_set(f"pileup_{n}", pile, a.smoothsize, a.reps, dev)
        results["sets"].append(res)
        print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
