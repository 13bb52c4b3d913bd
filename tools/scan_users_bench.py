"""The calls that run the scan skeleton of csrc/scan.h (k_sm_*, k_scan_*, k_pme_scan*) and the top-2 scan (k_t2_*), timed
or laid out for a kernel trace.  What profiles/scan_skeleton/README.md was measured with.

  python tools/scan_users_bench.py [--reps 7]        # wall time of each library call: median and best of --reps, one JSON line
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/scan_users_bench.py --reps 1
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/scan_users_bench.py --igd

Shapes are those of tools/setops_bench.py (reduce / cluster of 10M synth.py regions, the folds of 64 sets x 200k regions)
plus a u32 -> u64 scan of 50M counts; --igd makes one binary count (min_overlap 1) of 1M queries on the config-3 database
of tools/igd_bench.py, which builds pme_file once.  GTARS_AMD_LIB selects the library, so two builds can be run in turn.
Results are not checked here: tools/setops_bench.py and the tests do that.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--igd", action="store_true")
    a = ap.parse_args()
    import gtars_amd
    from gtars_amd import synth
    from gtars_amd._lib import check, debug_scan_u32, lib, ptr

    res = {"lib": os.environ.get("GTARS_AMD_LIB", "tree")}
    if a.igd:
        db, q = synth.make_igd_db(50_000_000, 1000), synth.make_background_queries(1_000_000)
        g = gtars_amd.IgdIndex(db["chrom"], db["start"], db["end"], db["file"], None, n_chrom=synth.N_CHROM, n_files=1000)
        res["records"] = len(g)
        res["binary_hits"] = int(np.asarray(g.count_region_hits(q["chrom"], q["start"], q["end"], 1)).sum())
        print(json.dumps(res), flush=True)
        return
    from gtars.models import RegionSetList
    from setops_bench import make_set

    def times(fn):
        fn()  # warm-up
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.median(ts)), 3), round(min(ts), 3)

    u = synth.make_universe(100_000)
    _, A = make_set(10_000_000, 91, u)
    h = C.c_void_p()
    ids = np.zeros(len(A), dtype=np.uint32)

    def do_reduce():
        check(lib.gtars_regionset_reduce(A._h, C.byref(h)))
        lib.gtars_regionset_free(h)

    res["reduce_10M_ms"] = times(do_reduce)
    res["cluster_10M_ms"] = times(lambda: check(lib.gtars_regionset_cluster(A._h, 0, ptr(ids))))
    del A
    counts = np.random.default_rng(3).integers(0, 50, 50_000_000).astype(np.uint32)
    res["scan_u32_50M_ms"] = times(lambda: debug_scan_u32(counts))
    del counts
    rsl = RegionSetList([make_set(200_000, 5000 + 7 * k, u)[1] for k in range(64)])
    res["union_all_b_ms"] = times(rsl.union_all)
    res["intersect_all_b_ms"] = times(rsl.intersect_all)
    res["bulk_union_except_b_ms"] = times(rsl.bulk_union_except)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
