"""Region-set algebra (csrc/setops.hip) on the device vs the plain-Python restatement (tests/setops_ref.py).

  python tools/setops_bench.py [--sets 200] [--set-regions 50000] [--big 10000000] [--reps 3] [--json out.json]

Device figures are wall times of one library call (host columns in, host results out, the stream drained), the best of
--reps after a warm-up call.  pairwise_jaccard runs on --sets x --set-regions synth.py query sets; reduce / closest / cluster
on --big synth.py regions (closest against a quarter as many).  The CPU restatement is pure Python: it is timed on a
smaller share of the same work (--cpu-big regions, --cpu-sets sets) and its results are compared with the device's there;
at full size the device results are checked against numpy restatements (reduce, cluster) and sampled pairs.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import setops_ref as R  # noqa: E402

from gtars_amd import synth  # noqa: E402
from gtars_amd._lib import check, lib, ptr  # noqa: E402
from gtars.models import RegionSet, RegionSetList  # noqa: E402

TOP = 0xFFFFFFFF


def make_set(n, seed, universe):
    q = synth.make_queries(universe, n, seed=seed, unknown_per_mille=0)
    names = np.array(synth.CHROM_NAMES, dtype=object)[q["chrom"]]
    return q, RegionSet.from_vectors(list(names), q["start"], q["end"])


def best_of(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3


def np_reduce(rank, start, end):
    o = np.lexsort((start, rank))
    r, s, e = rank[o], start[o].astype(np.int64), end[o].astype(np.int64)
    key = r.astype(np.int64) * (1 << 33) + e
    cm = np.maximum.accumulate(key) - r.astype(np.int64) * (1 << 33)
    head = np.ones(len(s), dtype=bool)
    head[1:] = (r[1:] != r[:-1]) | (s[1:] > cm[:-1])
    idx = np.flatnonzero(head)
    return r[idx], s[idx], np.maximum.reduceat(e, idx)


def byte_rank(chrom):
    order = {nm: i for i, nm in enumerate(sorted(synth.CHROM_NAMES))}
    lut = np.array([order[nm] for nm in synth.CHROM_NAMES], dtype=np.uint32)
    return lut[chrom]


def tuples(q, n=None):
    n = len(q["chrom"]) if n is None else n
    return [(synth.CHROM_NAMES[int(q["chrom"][i])], int(q["start"][i]), int(q["end"][i])) for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=200)
    ap.add_argument("--set-regions", type=int, default=50_000)
    ap.add_argument("--big", type=int, default=10_000_000)
    ap.add_argument("--cpu-big", type=int, default=1_000_000)
    ap.add_argument("--cpu-sets", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = {"device": {}, "cpu_restatement": {}, "checks": {}}
    u = synth.make_universe(100_000)

    # ---- pairwise Jaccard
    cols, sets = [], []
    for k in range(a.sets):
        q, rs = make_set(a.set_regions, 1000 + 7 * k, u)
        cols.append(q)
        sets.append(rs)
    rsl = RegionSetList(sets)
    n = len(sets)
    out = np.zeros((n, n))
    handles = (C.c_void_p * n)(*[s._h for s in sets])
    res["device"]["pairwise_jaccard_ms"] = best_of(
        lambda: check(lib.gtars_regionset_pairwise_jaccard(C.cast(handles, C.c_void_p), n, ptr(out))), a.reps)
    res["device"]["pairwise_jaccard_shape"] = f"{n} sets x {a.set_regions} regions"
    M = np.array(rsl.pairwise_jaccard())
    assert np.array_equal(M, out)
    tot = [int((lambda r: (r[2] - r[1]).sum())(np_reduce(byte_rank(c["chrom"]), c["start"], c["end"]))) & TOP for c in cols]
    rng = np.random.default_rng(0)
    for i, j in rng.integers(0, n, (64, 2)):
        if i == j:
            assert M[i, j] == 1.0
            continue
        ci, cj = cols[i], cols[j]
        _, s, e = np_reduce(np.concatenate([byte_rank(ci["chrom"]), byte_rank(cj["chrom"])]),
                            np.concatenate([ci["start"], cj["start"]]), np.concatenate([ci["end"], cj["end"]]))
        un = int((e - s).sum()) & TOP
        want = 0.0 if un == 0 else ((tot[i] + tot[j] - un) & TOP) / un
        assert M[i, j] == want, (i, j)
    res["checks"]["pairwise_sampled_pairs"] = 64
    m = min(a.cpu_sets, n)
    regs = [tuples(c) for c in cols[:m]]
    t0 = time.perf_counter()
    Mc = R.pairwise_jaccard(regs)
    res["cpu_restatement"]["pairwise_jaccard_ms"] = (time.perf_counter() - t0) * 1e3
    res["cpu_restatement"]["pairwise_jaccard_shape"] = f"{m} sets x {a.set_regions} regions"
    assert Mc == M[:m, :m].tolist()
    del sets, rsl, handles

    # ---- reduce / cluster / closest at --big
    qa, A = make_set(a.big, 91, u)
    qb, B = make_set(a.big // 4, 92, u)
    nA = len(A)
    h = C.c_void_p()

    def do_reduce():
        check(lib.gtars_regionset_reduce(A._h, C.byref(h)))
        lib.gtars_regionset_free(h)

    ids = np.zeros(nA, dtype=np.uint32)

    def do_cluster():
        check(lib.gtars_regionset_cluster(A._h, 0, ptr(ids)))

    def do_closest():
        ps, po, pd, cnt = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        check(lib.gtars_regionset_closest(A._h, B._h, C.byref(ps), C.byref(po), C.byref(pd), C.byref(cnt)))
        for p in (ps, po, pd):
            lib.gtars_free(p)

    for name, fn in (("reduce", do_reduce), ("cluster", do_cluster), ("closest", do_closest)):
        res["device"][f"{name}_ms"] = best_of(fn, a.reps)
    res["device"]["big_shape"] = f"{nA} regions (closest: vs {len(B)})"
    # checks at full size: reduce and cluster against numpy
    _, s, e = np_reduce(byte_rank(qa["chrom"]), qa["start"], qa["end"])
    red = A.reduce()
    assert np.array_equal(red.starts, s.astype(np.uint32)) and np.array_equal(red.ends, e.astype(np.uint32))
    cl = np.array(A.cluster(0), dtype=np.int64)
    want = np.empty(nA, dtype=np.int64)
    o3 = np.lexsort((qa["end"], qa["start"], byte_rank(qa["chrom"])))
    r3, s3, e3 = byte_rank(qa["chrom"])[o3], qa["start"][o3].astype(np.int64), qa["end"][o3].astype(np.int64)
    cm = np.maximum.accumulate(r3.astype(np.int64) * (1 << 33) + e3) - r3.astype(np.int64) * (1 << 33)
    h3 = np.ones(nA, dtype=bool)
    h3[1:] = (r3[1:] != r3[:-1]) | (s3[1:] > cm[:-1])
    want[o3] = np.cumsum(h3) - 1
    assert np.array_equal(cl, want)
    res["checks"]["reduce_cluster_full_size"] = True
    # CPU restatement on --cpu-big of the same regions, compared with the device there
    k = min(a.cpu_big, nA)
    sa, sb = tuples(qa, k), tuples(qb, k // 4)
    As, Bs = RegionSet.from_vectors([t[0] for t in sa], [t[1] for t in sa], [t[2] for t in sa]), \
        RegionSet.from_vectors([t[0] for t in sb], [t[1] for t in sb], [t[2] for t in sb])
    for name, cpu, dev in (("reduce", lambda: R.reduce(sa), lambda: [(r.chr, r.start, r.end) for r in As.reduce()]),
                           ("cluster", lambda: R.cluster(sa, 0), lambda: As.cluster(0)),
                           ("closest", lambda: R.closest(sa, sb), lambda: As.closest(Bs))):
        t0 = time.perf_counter()
        want = cpu()
        res["cpu_restatement"][f"{name}_ms"] = (time.perf_counter() - t0) * 1e3
        assert dev() == want, name
    res["cpu_restatement"]["big_shape"] = f"{k} regions (closest: vs {k // 4})"
    res["checks"]["cpu_vs_device_equal"] = True
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
