#!/usr/bin/env python3
"""Host-side costs of an IGD handle (profiles/igd_handle): wall time of IgdIndex(...) at 5e4 records (the host-sort arm of
gtars_igd_build) and at 5e6 (the device-sort arm), one warm-up and five timed builds each, and the first binary count with
min_overlap == 1 on a fresh 5e6-record handle -- the call that builds pme_file -- next to the second call on the same
handle, five fresh handles.  One JSON line.  GTARS_AMD_LIB selects the library (A/B runs).
usage: python tools/igd_handle_bench.py"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import gtars_amd
from gtars_amd import synth

F = 100


def build(db):
    t = time.perf_counter()
    g = gtars_amd.IgdIndex(db["chrom"], db["start"], db["end"], db["file"], db["value"], n_chrom=synth.N_CHROM, n_files=F)
    return g, (time.perf_counter() - t) * 1e3


def summary(ms):
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "all_ms": [round(x, 3) for x in ms]}


def main():
    torch.cuda.set_device(0)
    out = {"lib": os.environ.get("GTARS_AMD_LIB", "tree")}
    dbs = {}
    for n in (50_000, 5_000_000):
        db = synth.make_igd_db(n, F, seed=6)
        db["value"] = np.arange(n, dtype=np.int32)
        dbs[n] = db
        build(db)[0].close()  # warm-up
        ms = []
        for _ in range(5):
            g, t = build(db)
            ms.append(t)
            g.close()
        out[f"build_{n}"] = summary(ms)
    q = synth.make_background_queries(100_000, seed=5)
    first, second = [], []
    for _ in range(5):
        g, _t = build(dbs[5_000_000])
        torch.cuda.synchronize()
        for into in (first, second):
            t = time.perf_counter()
            hits = g.count_region_hits(q["chrom"], q["start"], q["end"], 1)
            into.append((time.perf_counter() - t) * 1e3)
        out["binary_hits"] = int(hits.sum())
        g.close()
    out["first_binary_count_5000000"] = summary(first)
    out["second_binary_count_5000000"] = summary(second)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
