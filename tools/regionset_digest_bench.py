"""RegionSet identifiers and BED text on the device (csrc/bed_text.hip, K25): kernel times, the device entry on resident
columns, the list call from Python, the library's host path on 16 threads and the hashlib restatement on a sample; the
GTARS_BED_DIGEST_HOST_LEN sweep; to_bed's text on the device against host formatting.  Every output is compared in the run.

  python tools/regionset_digest_bench.py [--sets 2000,200] [--rows 50000] [--text-rows 10000000] [--reps 10] [--json out.json]

The batch: --sets sets of --rows hg38-shaped regions each (synth.make_universe; 50 distinct universes, set k = universe k % 50
with its starts and ends moved up by k, so every set hashes differently), one names table of 25 chromosomes.
  * kernels: k_bed_widths, k_bed_fill and k_bed_md5 from the library's profiling scopes (HIP events), median of --reps runs
    of the device entry; the entry itself by wall time around a synchronised call, median of --reps.
  * the list call RegionSetList.identifiers() by wall time (it gathers the handles' columns, uploads, runs and downloads),
    and identifiers(on_host=True, threads=16): median of 3.
  * the restatement (tests/bed_text_ref.py) on the first --sample sets, scaled to the batch by rows.
  * the host-tail sweep on the smallest batch: GTARS_BED_DIGEST_HOST_LEN at half, once and twice the batch's median stream
    length and far above it, the device entry by wall time.
  * to_bed's text of 1e4 .. --text-rows rows: RegionSet._bed_text on the device (fill plus download) and on the host threads.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import bed_text_ref as R  # noqa: E402
import gtars_amd  # noqa: E402
from gtars_amd import _lib, synth  # noqa: E402
from gtars_amd._lib import check, lib  # noqa: E402
from gtars_amd.models import RegionSet, RegionSetList  # noqa: E402

DEV = torch.device("cuda:0")


def make_batch(n_sets, rows):
    base = [synth.make_universe(rows, seed=100 + k) for k in range(min(n_sets, 50))]
    cols = []
    for k in range(n_sets):
        u = base[k % len(base)]
        cols.append((u["chrom"].astype(np.uint32), (u["start"] + k).astype(np.uint32), (u["end"] + k).astype(np.uint32)))
    return cols


def wall(fn, reps):
    times, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), out


class Resident:
    """the batch as resident columns of gtars_bed_digests_device"""

    def __init__(self, cols):
        self.n = len(cols)
        self.set_off = np.concatenate([[0], np.cumsum([len(c[0]) for c in cols])]).astype(np.uint64)
        up = lambda k: torch.from_numpy(np.concatenate([c[k] for c in cols]).view(np.int32)).to(DEV)  # noqa: E731
        self.chrom, self.start, self.end = up(0), up(1), up(2)
        names = [n.encode() for n in synth.CHROM_NAMES]
        self.n_names = len(names)
        self.name_off = torch.from_numpy(np.cumsum([0] + [len(n) for n in names]).astype(np.int64)).to(DEV)
        self.names = torch.from_numpy(np.frombuffer(b"".join(names), dtype=np.uint8).copy()).to(DEV)
        self.out = torch.zeros(16 * self.n + 8, dtype=torch.uint8, device=DEV)

    def run(self, n_sets=None):
        n = self.n if n_sets is None else n_sets
        check(lib.gtars_bed_digests_device(self.set_off.ctypes.data, n, self.chrom.data_ptr(), self.start.data_ptr(), self.end.data_ptr(),
                                           self.name_off.data_ptr(), self.names.data_ptr(), self.n_names, None, None, None, 0,
                                           self.out.data_ptr(), torch.cuda.current_stream().cuda_stream))
        raw = self.out.cpu().numpy().tobytes()
        return [raw[16 * i:16 * i + 16].hex() for i in range(n)]


def kernel_medians(res, reps):
    per = {}
    lib.gtars_prof_enable(1)
    try:
        for _ in range(reps):
            lib.gtars_prof_reset()
            res.run()
            for name, v in _lib.prof_read().items():
                if name.startswith("k_bed_"):
                    per.setdefault(name, []).append(v["total_ms"])
    finally:
        lib.gtars_prof_enable(0)
        lib.gtars_prof_reset()
    return {k: statistics.median(v) for k, v in per.items()}


def bench_batch(n_sets, rows, reps, sample):
    cols = make_batch(n_sets, rows)
    names = list(synth.CHROM_NAMES)
    t0 = time.perf_counter()
    sets = [RegionSet.from_vectors([names[c] for c in ch], s, e) for ch, s, e in cols]
    build_s = time.perf_counter() - t0
    lst = RegionSetList(sets)
    res = Resident(cols)
    want = res.run()  # (warm-up; compared below)
    entry_ms, got = wall(res.run, reps)
    assert got == want
    kernels = kernel_medians(res, reps)
    list_ms, got = wall(lst.identifiers, 3)
    assert got == want, "the list call and the device entry differ"
    host_ms, got = wall(lambda: lst.identifiers(on_host=True, threads=16), 3)
    assert got == want, "the host path and the device entry differ"
    t0 = time.perf_counter()
    for k in range(min(sample, n_sets)):
        ch, s, e = cols[k]
        assert R.identifier([(names[c], int(a), int(b), None) for c, a, b in zip(ch, s, e)]) == want[k], k
    ref_ms = (time.perf_counter() - t0) * 1e3 * n_sets / max(1, min(sample, n_sets))
    text_bytes = sum(len(",".join(map(str, c[1]))) + len(",".join(map(str, c[2]))) for c in cols[:1]) * n_sets  # (starts + ends, about)
    out = {"sets": n_sets, "rows_per_set": rows, "handles_built_s": round(build_s, 2), "device_entry_ms": entry_ms, "kernels_ms": kernels,
           "list_call_device_ms": list_ms, "list_call_host16_ms": host_ms, "restatement_scaled_ms": ref_ms,
           "start_end_text_bytes_about": text_bytes, "compared": "entry == list call == host path == restatement sample"}
    return out, res, want, cols


def sweep_host_len(res, want, cols):
    lens = sorted(len(",".join(map(str, c[k]))) for c in cols[:50] for k in (1, 2)) + sorted(len(",".join(synth.CHROM_NAMES[i] for i in c[0])) for c in cols[:50])
    med = int(statistics.median(lens))
    rows = []
    for value in (med // 2, med, 2 * med, 1 << 39, None):
        if value is None:
            os.environ.pop("GTARS_BED_DIGEST_HOST_LEN", None)
        else:
            os.environ["GTARS_BED_DIGEST_HOST_LEN"] = str(value)
        gtars_amd.reload_env()
        ms, got = wall(res.run, 3)
        assert got == want, value
        rows.append({"GTARS_BED_DIGEST_HOST_LEN": value if value is not None else "unset (rule of the batch)", "device_entry_ms": ms})
    return {"median_stream_bytes": med, "runs": rows}


def bench_text(max_rows):
    u = synth.make_universe(max_rows, seed=9)
    names = list(synth.CHROM_NAMES)
    out = []
    n = 10_000
    while n <= max_rows:
        rs = RegionSet.from_vectors([names[c] for c in u["chrom"][:n]], u["start"][:n], u["end"][:n])
        reps = 3 if n >= 1_000_000 else 5
        rs._bed_text(False)  # warm-up
        dev_ms, a = wall(lambda: rs._bed_text(False), reps)
        host_ms, b = wall(lambda: rs._bed_text(True), reps)
        assert a == b, n
        if n <= 100_000:
            assert a == R.bed_text([(names[c], int(s), int(e), None) for c, s, e in zip(u["chrom"][:n], u["start"][:n], u["end"][:n])])
        out.append({"rows": n, "text_bytes": len(a), "device_ms": dev_ms, "host_ms": host_ms})
        n *= 10
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="2000,200")
    ap.add_argument("--rows", type=int, default=50_000)
    ap.add_argument("--text-rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sample", type=int, default=4)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert gtars_amd.device_count() > 0
    result = {"device": torch.cuda.get_device_name(0), "batches": []}
    shapes = sorted({int(x) for x in a.sets.split(",")}, reverse=True)
    for n_sets in shapes:
        out, res, want, cols = bench_batch(n_sets, a.rows, a.reps, a.sample)
        result["batches"].append(out)
        print(json.dumps(out), flush=True)
        if n_sets == shapes[-1]:
            result["host_len_sweep"] = sweep_host_len(res, want, cols)
            print(json.dumps(result["host_len_sweep"]), flush=True)
        del res, cols
        torch.cuda.empty_cache()
    result["bed_text"] = bench_text(a.text_rows)
    print(json.dumps(result["bed_text"]), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
