"""GC content and dinucleotide counts (csrc/seqstats.hip, K12) on the device: kernel time and achieved HBM fraction for
both modes and both lane groupings, the library call, the one-off upload of the assembly, and a 16-thread numpy baseline,
on a synthetic hg38-shaped assembly.

  python tools/seqstats_bench.py [--scale 1.0] [--reps 10] [--lanes 16,64] [--json out.json]

The assembly: the 25 chromosomes of tests/golden/hg38.chrom.sizes (chr1 .. chr22, X, Y, M) at --scale times their size,
random ACGT with soft-masked (lower-case) stretches on 40 % of the bytes and runs of N, written as a .fab file and loaded
with BinaryGenomeAssembly.  Three region sets: 1e6 peaks of 200-800 bp, 1e5 regions of 0.1-2 Mbp, and a mix of a tenth
of each.  Per set, mode and lane grouping (GTARS_SEQ_LANES, reloaded between runs): the device entry on resident columns,
timed by HIP events after a warm-up, median of --reps; HBM fraction = (sum of region bytes + output bytes) / t / 8.0e12.
The device entry's time holds the piece count, its scan and one stream drain besides the counting kernel.  Every output
is checked in the run against per-chromosome prefix sums made with torch from the same bytes.  The library call
(calc_gc_content / calc_dinucl_freq: columns in, floats out) and the upload (the first counting call) are timed on their
own.  The numpy baseline (a byte table and bincount over slices, 16 threads) runs on the first --baseline-rows rows of a
set and is reported with the bytes it covered.
"""
from __future__ import annotations

import argparse
import json
import os
import struct
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import gtars_amd  # noqa: E402
import gtars_amd.seqstats as GD  # noqa: E402
from gtars_amd.models import RegionSet  # noqa: E402
from gtars_amd.seqstats import BinaryGenomeAssembly  # noqa: E402

HBM_PEAK = 8.0e12
CODE = np.full(256, 4, dtype=np.uint8)  # byte -> A C G T = 0 .. 3, anything else 4
for _k, _b in enumerate(b"ACGT"):
    CODE[_b] = CODE[_b + 32] = _k
IS_GC = np.zeros(256, dtype=np.uint8)
IS_GC[[ord(c) for c in "GCgc"]] = 1


def chrom_sizes(scale):
    path = os.path.join(ROOT, "tests", "golden", "hg38.chrom.sizes")
    rows = [line.split() for line in open(path) if line.strip()]
    keep = {f"chr{k}" for k in list(range(1, 23)) + ["X", "Y", "M"]}
    return [(n, max(int(int(s) * scale), 16_569)) for n, s in rows if n in keep]


def make_assembly(sizes, seed=7):
    rng = np.random.default_rng(seed)
    upper, lower = np.frombuffer(b"ACGT", np.uint8), np.frombuffer(b"acgt", np.uint8)
    seqs = []
    for _, n in sizes:
        s = upper[rng.integers(0, 4, n, dtype=np.uint8)]
        # soft-masked stretches of ~5 kbp on 40 % of the chromosome, N runs of ~50 kbp on 2 %
        for frac, length, fill in ((0.4, 5000, None), (0.02, 50_000, ord("N"))):
            for at in rng.integers(0, max(n - length, 1), max(int(n * frac / length), 1)):
                if fill is None:
                    s[at:at + length] |= 0x20
                else:
                    s[at:at + length] = fill
        seqs.append(s)
    return seqs


def write_fab(path, sizes, seqs):
    head = 9 + sum(2 + len(n) + 16 for n, _ in sizes)
    with open(path, "wb") as f:
        f.write(b"GFAB\x01" + struct.pack("<I", len(sizes)))
        at = head
        for (n, _), s in zip(sizes, seqs):
            f.write(struct.pack("<H", len(n)) + n.encode() + struct.pack("<QQ", at, len(s)))
            at += len(s)
        for s in seqs:
            f.write(s.tobytes())


def make_sets(sizes, seed=3):
    rng = np.random.default_rng(seed)
    lens = np.array([n for _, n in sizes], dtype=np.int64)

    def draw(n, lo, hi):
        ok = np.flatnonzero(lens > hi)
        c = ok[rng.choice(len(ok), n, p=lens[ok] / lens[ok].sum())]
        w = rng.integers(lo, hi + 1, n)
        s = (rng.random(n) * (lens[c] - w)).astype(np.int64)
        return c.astype(np.uint32), s.astype(np.uint32), (s + w).astype(np.uint32)

    peaks, longs = draw(1_000_000, 200, 800), draw(100_000, 100_000, 2_000_000)
    pick_p, pick_l = rng.permutation(1_000_000)[:100_000], rng.permutation(100_000)[:10_000]
    mix = [np.concatenate([p[pick_p], l[pick_l]]) for p, l in zip(peaks, longs)]
    order = rng.permutation(len(mix[0]))
    return {"peaks_1e6": peaks, "long_1e5": longs, "mix_1.1e5": tuple(m[order] for m in mix)}


class Truth:
    """per-chromosome exclusive prefix sums on the device: GC bytes, and valid windows per dinucleotide"""

    def __init__(self, seqs, dev):
        self.dev = dev
        self.code = [torch.from_numpy(CODE[s]).to(dev) for s in seqs]
        self.gc = [torch.from_numpy(IS_GC[s]).to(dev) for s in seqs]

    @staticmethod
    def _prefix(flags):
        p = torch.zeros(len(flags) + 1, dtype=torch.int32, device=flags.device)
        torch.cumsum(flags, 0, dtype=torch.int32, out=p[1:])
        return p

    def counts(self, chrom, start, end, mode):
        n = len(chrom)
        out = torch.zeros((n, 1 if mode == "gc" else 16), dtype=torch.int32, device=self.dev)
        c_t, s_t, e_t = (torch.from_numpy(x.astype(np.int64)).to(self.dev) for x in (chrom, start, end))
        for c in np.unique(chrom).tolist():
            rows = torch.nonzero(c_t == c).flatten()
            s, e = s_t[rows], e_t[rows]
            if mode == "gc":
                p = self._prefix(self.gc[c])
                out[rows, 0] = p[e] - p[s]
                continue
            code = self.code[c]
            pair = code[:-1].to(torch.int16) * 5 + code[1:].to(torch.int16)  # window i
            last = torch.clamp(e - 1, min=0)
            last = torch.maximum(last, s)  # windows [s, e - 1)
            for a in range(4):
                for b in range(4):
                    p = self._prefix(pair == 5 * a + b)
                    out[rows, 4 * a + b] = p[last] - p[s]
                    del p
        return out


def numpy_baseline(seqs, chrom, start, end, mode):
    def one(lo_hi):
        acc = 0
        for i in range(*lo_hi):
            seg = seqs[chrom[i]][start[i]:end[i]]
            if mode == "gc":
                acc += int(IS_GC[seg].sum())
            else:
                code = CODE[seg]
                pair = code[:-1] * 5 + code[1:]
                acc += int(np.bincount(pair, minlength=25)[0])
        return acc

    n = len(chrom)
    cuts = [(k * n // 16, (k + 1) * n // 16) for k in range(16)]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(one, cuts))
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--lanes", default="16,64")
    ap.add_argument("--baseline-rows", type=int, default=100_000)
    ap.add_argument("--baseline-long-rows", type=int, default=200)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    sizes = chrom_sizes(a.scale)
    t = time.perf_counter()
    seqs = make_assembly(sizes)
    total = int(sum(len(s) for s in seqs))
    results = {"device": torch.cuda.get_device_name(0), "scale": a.scale, "assembly_bytes": total, "piece_bytes": GD.SEQ_PIECE,
               "make_assembly_s": time.perf_counter() - t, "sets": []}
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "synthetic.fab")
        write_fab(path, sizes, seqs)
        t = time.perf_counter()
        g = BinaryGenomeAssembly(path)
        results["load_fab_s"] = time.perf_counter() - t
    names = g.chrom_names
    assert names == [n for n, _ in sizes]
    # the upload: the first counting call builds the device image
    one = RegionSet.from_vectors([names[0]], [0], [100])
    t = time.perf_counter()
    GD.calc_gc_content(one, g)
    results["upload_s"] = time.perf_counter() - t
    results["upload_GBps"] = total / results["upload_s"] / 1e9
    print(json.dumps({k: v for k, v in results.items() if k != "sets"}), flush=True)
    truth = Truth(seqs, dev)
    stream = torch.cuda.current_stream().cuda_stream
    for label, (chrom, start, end) in make_sets(sizes).items():
        n = len(chrom)
        region_bytes = int((end.astype(np.int64) - start).sum())
        cols = [torch.from_numpy(x.view(np.int32)).to(dev) for x in (chrom, start, end)]
        res = {"set": label, "rows": n, "region_bytes": region_bytes, "median_width": float(np.median(end - start))}
        for mode in ("gc", "dinucl"):
            width = 1 if mode == "gc" else 16
            want = truth.counts(chrom, start, end, mode)
            out = torch.empty(n * width, dtype=torch.int32, device=dev)
            for lanes in a.lanes.split(","):
                os.environ["GTARS_SEQ_LANES"] = lanes
                gtars_amd.reload_env()
                out.fill_(-1)
                times = []
                for _ in range(a.reps + 1):
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    GD.counts_device(g, mode, cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), n, out.data_ptr(), stream)
                    t1.record()
                    torch.cuda.synchronize()
                    times.append(t0.elapsed_time(t1))
                assert torch.equal(out.view(n, width), want), (label, mode, lanes)
                ms = float(np.median(times[1:]))
                res[f"{mode}_lanes{lanes}_ms_median"] = ms
                res[f"{mode}_lanes{lanes}_ms_min"] = float(min(times[1:]))
                res[f"{mode}_lanes{lanes}_hbm_fraction"] = (region_bytes + 4 * n * width) / (ms * 1e-3) / HBM_PEAK
            del want, out
        os.environ.pop("GTARS_SEQ_LANES", None)
        gtars_amd.reload_env()
        res["checked"] = "every row, both modes, every lane grouping"
        # the library call: names and columns in, floats out (a tenth of the rows of the long set: its host part is per row)
        rs = RegionSet.from_vectors([names[c] for c in chrom.tolist()], start, end)
        for mode, call in (("gc", GD.calc_gc_content), ("dinucl", GD.calc_dinucl_freq)):
            call(rs, g)
            t = time.perf_counter()
            call(rs, g)
            res[f"library_call_{mode}_ms"] = (time.perf_counter() - t) * 1e3
        k = min(n, a.baseline_long_rows if label.startswith("long") else a.baseline_rows)
        for mode in ("gc", "dinucl"):
            res[f"numpy_16_threads_{mode}_ms"] = numpy_baseline(seqs, chrom[:k], start[:k], end[:k], mode)
        res["numpy_rows"] = k
        res["numpy_region_bytes"] = int((end[:k].astype(np.int64) - start[:k]).sum())
        results["sets"].append(res)
        print(json.dumps(res), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
