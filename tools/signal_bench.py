"""calc_summary_signal (csrc/signal.hip, K13) on the device: time of the fold kernel and of the whole device entry,
achieved HBM fraction, the library call, and a 16-thread numpy baseline, on a synthetic hg38-shaped signal matrix.

  python tools/signal_bench.py [--rows 1000000] [--conds 16,74,256] [--reps 10] [--json out.json]

The matrix: --rows regions of 150-500 bp spread over the 25 chromosomes of tests/golden/hg38.chrom.sizes (chr1 .. chr22,
X, Y, M) in proportion to their sizes, disjoint, in shuffled row order, random values, built with
SignalMatrix.from_arrays.  Three query sets: 1e5 peaks and 1e6 peaks of 200-800 bp, 1e4 regions of 0.1-1 Mbp.  Per
condition count and set: the device entry on resident query columns without the download of the result rows, timed by
HIP events after a warm-up, median of --reps -- it holds the two tokenizer passes, the compaction, the fold, the sorts
and the statistics; the fold kernel alone from the library's per-kernel events (median of --reps); HBM fraction of the
fold = hits x conditions x 8 bytes / t / 8.0e12.  Every output is checked in the run against a torch restatement: the
rows are disjoint, so a query's hits are one run of the position-sorted rows, found by searchsorted and folded by a
running maximum; the statistics come from torch.sort and the same unfused arithmetic.  The library call
(summary_arrays: region set in, arrays out) is timed on its own.  The numpy baseline (searchsorted and a maximum over
row slices, 16 threads) runs on the first --baseline-rows queries of a set.
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

import gtars_amd  # noqa: E402
from gtars_amd import _lib  # noqa: E402
from gtars_amd.models import RegionSet  # noqa: E402
from gtars_amd.signal import SignalMatrix, summary_arrays, summary_device  # noqa: E402

HBM_PEAK = 8.0e12


def chrom_sizes():
    path = os.path.join(ROOT, "tests", "golden", "hg38.chrom.sizes")
    rows = [line.split() for line in open(path) if line.strip()]
    keep = {f"chr{k}" for k in list(range(1, 23)) + ["X", "Y", "M"]}
    return [(n, int(s)) for n, s in rows if n in keep]


def make_rows(sizes, n, seed=7):
    """n disjoint regions of 150-500 bp: per chromosome sorted random slots of its length / count, one region in each"""
    rng = np.random.default_rng(seed)
    lens = np.array([s for _, s in sizes], dtype=np.int64)
    per = np.maximum((n * lens / lens.sum()).astype(np.int64), 1)
    per[0] += n - per.sum()
    chrom, start, end = [], [], []
    for c, k in enumerate(per):
        slot = lens[c] // k
        w = np.minimum(rng.integers(150, 501, k), max(slot - 1, 1))
        s = np.arange(k, dtype=np.int64) * slot + (rng.random(k) * (slot - w)).astype(np.int64)
        chrom.append(np.full(k, c, np.uint32)), start.append(s), end.append(s + w)
    chrom, start, end = np.concatenate(chrom), np.concatenate(start).astype(np.uint32), np.concatenate(end).astype(np.uint32)
    order = rng.permutation(len(chrom))
    return chrom[order], start[order], end[order]


def make_queries(sizes, n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    lens = np.array([s for _, s in sizes], dtype=np.int64)
    ok = np.flatnonzero(lens > hi)
    c = ok[rng.choice(len(ok), n, p=lens[ok] / lens[ok].sum())]
    w = rng.integers(lo, hi + 1, n)
    s = (rng.random(n) * (lens[c] - w)).astype(np.int64)
    return c.astype(np.uint32), s.astype(np.uint32), (s + w).astype(np.uint32)


class Truth:
    """the rows sorted by (chromosome, start) on the device: a query's hits are the run [lo, hi) of them"""

    def __init__(self, chrom, start, end, values, dev):
        order = np.lexsort((start, chrom))
        self.dev = dev
        key = chrom[order].astype(np.int64) << 32
        self.start_key = torch.from_numpy(key | start[order]).to(dev)
        self.end_key = torch.from_numpy(key | end[order]).to(dev)  # disjoint rows: the ends ascend with the starts
        self.values = torch.from_numpy(values[order]).to(dev)

    def runs(self, qc, qs, qe):
        k = torch.from_numpy(qc.astype(np.int64) << 32).to(self.dev)
        s, e = (torch.from_numpy(x.astype(np.int64)).to(self.dev) for x in (qs, qe))
        lo = torch.searchsorted(self.end_key, k | s, right=True)  # first row with end > q.start
        hi = torch.searchsorted(self.start_key, k | e, right=False)  # first row with start >= q.end
        return lo, torch.maximum(hi, lo)

    def summary(self, qc, qs, qe):
        lo, hi = self.runs(qc, qs, qe)
        qidx = torch.nonzero(hi > lo).flatten()
        lo, cnt = lo[qidx], (hi - lo)[qidx]
        acc = self.values[lo].clone()
        live = torch.arange(len(qidx), device=self.dev)
        for k in range(1, int(cnt.max().item()) if len(qidx) else 0):
            live = live[cnt[live] > k]
            acc[live] = torch.maximum(acc[live], self.values[lo[live] + k])
        return qidx, acc, int(cnt.sum().item())

    @staticmethod
    def stats(res):
        s, _ = torch.sort(res, dim=0)
        n = s.shape[0]

        def median(a, b):
            k = b - a
            return (s[a + k // 2 - 1] + s[a + k // 2]) / 2.0 if k % 2 == 0 else s[a + k // 2]

        mid = n // 2
        med, lh, uh = median(0, n), median(0, mid if n % 2 == 0 else mid + 1), median(mid, n)
        iqr = uh - lh
        t = iqr * 1.5
        lf, uf = lh - t, uh + t
        big = torch.full_like(s, float("inf"))
        lw = torch.where(s >= lf, s, big).min(dim=0).values
        uw = torch.where(s <= uf, s, -big).max(dim=0).values
        return torch.stack([lw, lh, med, uh, uw], dim=1)


def numpy_baseline(chrom, start, end, values, q, rows, threads=16):
    order = np.lexsort((start, chrom))
    key = chrom[order].astype(np.int64) << 32
    sk, ek, v = key | start[order], key | end[order], values[order]
    qc, qs, qe = (x[:rows] for x in q)
    k = qc.astype(np.int64) << 32

    def work(part):
        lo = np.searchsorted(ek, k[part] | qs[part], side="right")
        hi = np.searchsorted(sk, k[part] | qe[part], side="left")
        return [v[a:b].max(axis=0) for a, b in zip(lo, hi) if b > a]

    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:
        n = sum(len(r) for r in ex.map(work, np.array_split(np.arange(len(qc)), threads)))
    return time.perf_counter() - t0, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--conds", default="16,74,256")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--baseline-rows", type=int, default=100_000)
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available() and gtars_amd.device_count() > 0, "signal_bench needs an MI355X"
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    sizes = chrom_sizes()
    chrom, start, end = make_rows(sizes, a.rows)
    sets = {"peaks_1e5": make_queries(sizes, 100_000, 200, 800, 3), "peaks_1e6": make_queries(sizes, 1_000_000, 200, 800, 4),
            "wide_1e4": make_queries(sizes, 10_000, 100_000, 1_000_000, 5)}
    names = [n for n, _ in sizes]
    out = []
    for nc in [int(x) for x in a.conds.split(",")]:
        values = np.random.default_rng(nc).random((len(chrom), nc))
        sm = SignalMatrix.from_arrays([names[c] for c in chrom], start, end, values, [f"c{k}" for k in range(nc)])
        assert sm.chrom_names == list(dict.fromkeys(names[c] for c in chrom))
        to_matrix = np.array([sm.chrom_names.index(n) for n in names], dtype=np.uint32)
        truth = Truth(chrom, start, end, values, dev)
        for name, (qc, qs, qe) in sets.items():
            d = [torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(dev) for x in (to_matrix[qc], qs, qe)]
            args = (sm, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), len(qc), torch.cuda.current_stream().cuda_stream)
            t0 = time.perf_counter()
            qidx, res, stats = summary_device(*args)  # (the first call of a matrix builds its device image)
            first = time.perf_counter() - t0
            want_q, want_res, hits = truth.summary(qc, qs, qe)
            assert np.array_equal(qidx, want_q.cpu().numpy()), (nc, name, "rows")
            assert np.array_equal(res.view(np.uint64), want_res.cpu().numpy().view(np.uint64)), (nc, name, "fold")
            assert np.array_equal(stats.view(np.uint64), truth.stats(want_res).cpu().numpy().view(np.uint64)), (nc, name, "stats")
            times = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                summary_device(*args, rows=False)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1) * 1e-3)
            folds = []
            _lib.lib.gtars_prof_enable(1)
            for _ in range(a.reps):
                _lib.lib.gtars_prof_reset()
                summary_device(*args, rows=False)
                folds.append(_lib.prof_read()["k_signal_fold"]["total_ms"] * 1e-3)
            _lib.lib.gtars_prof_enable(0)
            rs = RegionSet.from_vectors([names[c] for c in qc], qs, qe)
            t0 = time.perf_counter()
            summary_arrays(rs, sm)
            call = time.perf_counter() - t0
            rows = min(a.baseline_rows, len(qc))
            base_t, base_n = numpy_baseline(chrom, start, end, values, (qc, qs, qe), rows)
            fold, entry = float(np.median(folds)), float(np.median(times))
            row = {"conditions": nc, "set": name, "queries": len(qc), "result_rows": len(qidx), "hits": hits, "fold_ms": fold * 1e3,
                   "fold_hbm_fraction": hits * nc * 8 / fold / HBM_PEAK, "entry_ms": entry * 1e3, "first_call_ms": first * 1e3,
                   "library_call_ms": call * 1e3, "numpy16_ms": base_t * 1e3, "numpy16_queries": rows, "numpy16_result_rows": base_n,
                   "checked": True}
            print(json.dumps(row), flush=True)
            out.append(row)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
