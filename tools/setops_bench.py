"""Region-set algebra (csrc/setops.hip) on the device vs the plain-Python restatement (tests/setops_ref.py).

  python tools/setops_bench.py [--sets 200] [--set-regions 50000] [--big 10000000] [--reps 3] [--json out.json]
                               [--fold-sets 64] [--fold-set-regions 200000] [--only folds|algebra]

Device figures are wall times of one library call (host columns in, host results out, the stream drained), the best of
--reps after a warm-up call.  pairwise_jaccard runs on --sets x --set-regions synth.py query sets; reduce / closest / cluster
on --big synth.py regions (closest against a quarter as many).  The CPU restatement is pure Python: it is timed on a
smaller share of the same work (--cpu-big regions, --cpu-sets sets) and its results are compared with the device's there;
at full size the device results are checked against numpy restatements (reduce, cluster) and sampled pairs.

The folds over a list (RegionSetList.union_all / intersect_all / bulk_union_except) run on the --sets x --set-regions sets
and on --fold-sets x --fold-set-regions.  Each is timed (one call, results as RegionSets on the host) next to the same
answer from a Python fold of RegionSet.union / RegionSet.intersect_all through the library, in the same process: N - 1
calls for union_all and intersect_all, the prefix / suffix scheme of 3 N unions for bulk_union_except.  Every device
output must equal the fold's, union_all must equal a numpy reduce of the concatenation, and sampled union_except(i) must
equal a numpy reduce of the other sets' rows, overlap every row of theirs and have no region that misses them all
(any_overlaps).  The JSON is rewritten after every stage, so a run that is cut short leaves what it measured.
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


def same_set(a, b):
    return a.chrom_names == b.chrom_names and all(np.array_equal(x, y) for x, y in
                                                  ((a.chrom_ids, b.chrom_ids), (a.starts, b.starts), (a.ends, b.ends)))


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def fold_union_all(sets):
    acc = sets[0]
    for s in sets[1:]:
        acc = acc.union(s)
    return acc


def fold_intersect_all(sets):
    acc = sets[0]
    for s in sets[1:]:
        acc = acc.intersect_all(s)
    return acc


def fold_bulk_union_except(sets):
    """the prefix / suffix scheme: about 3 N unions of growing sets"""
    n = len(sets)
    prefix = [sets[0]]
    for i in range(1, n):
        prefix.append(prefix[-1].union(sets[i]))
    suffix = [None] * n
    suffix[n - 1] = sets[n - 1]
    for i in range(n - 2, -1, -1):
        suffix[i] = sets[i].union(suffix[i + 1])
    ex = [suffix[1]] + [prefix[i - 1].union(suffix[i + 1]) for i in range(1, n - 1)] + [prefix[n - 2]]
    return prefix[n - 1], ex


def bench_folds(res, tag, cols, sets, reps, flush):
    """union_all / intersect_all / bulk_union_except of one list: device call vs Python fold, every output checked"""
    rsl = RegionSetList(sets)
    n, shape = len(sets), f"{len(sets)} sets x {len(sets[0])} regions"
    dev, fold, chk = res["device"], res["library_fold"], res["checks"]
    rank = np.concatenate([byte_rank(c["chrom"]) for c in cols]).astype(np.int64)
    start, end = (np.concatenate([c[k] for c in cols]).astype(np.int64) for k in ("start", "end"))
    owner = np.repeat(np.arange(n), [len(c["chrom"]) for c in cols])
    o = np.lexsort((start, rank))
    rank, start, end, owner = rank[o], start[o], end[o], owner[o]
    names_sorted = sorted(synth.CHROM_NAMES)

    def equals_numpy(got, keep):
        r, s, e = np_reduce(rank[keep], start[keep], end[keep])  # (rows already sorted: the lexsort is stable)
        gr = np.array([names_sorted.index(nm) for nm in got.chrom_names], dtype=np.int64)[got.chrom_ids]
        return np.array_equal(gr, r) and np.array_equal(got.starts, s) and np.array_equal(got.ends, e)

    # union_all
    dev[f"union_all_ms_{tag}"] = best_of(rsl.union_all, reps)
    want, fold[f"union_all_ms_{tag}"] = timed(lambda: fold_union_all(sets))
    got = rsl.union_all()
    assert same_set(got, want) and equals_numpy(got, np.ones(len(owner), dtype=bool))
    chk[f"union_all_{tag}"] = f"{len(got)} regions == fold == numpy reduce"
    flush()
    # intersect_all
    dev[f"intersect_all_ms_{tag}"] = best_of(rsl.intersect_all, reps)
    want, fold[f"intersect_all_ms_{tag}"] = timed(lambda: fold_intersect_all(sets))
    got = rsl.intersect_all()
    assert same_set(got, want)
    assert len(got) == 0 or all(all(got.any_overlaps(s)) for s in sets[:: max(1, n // 4)])
    chk[f"intersect_all_{tag}"] = f"{len(got)} regions == fold, each inside every sampled set"
    flush()
    del got, want
    # bulk_union_except
    dev[f"bulk_union_except_ms_{tag}"] = best_of(rsl.bulk_union_except, max(1, reps - 1))
    full, ex = rsl.bulk_union_except()
    (wfull, wex), fold[f"bulk_union_except_ms_{tag}"] = timed(lambda: fold_bulk_union_except(sets))
    assert same_set(full, wfull) and all(same_set(g, w) for g, w in zip(ex, wex))
    del wfull, wex
    sample = sorted({0, n // 3, n - 1})
    for i in sample:
        assert equals_numpy(ex[i], owner != i), i
        keep = np.flatnonzero(owner != i)
        others = RegionSet.from_vectors([names_sorted[r] for r in rank[keep].tolist()], start[keep], end[keep])
        assert all(ex[i].any_overlaps(others)) and all(others.any_overlaps(ex[i])), i
    chk[f"bulk_union_except_{tag}"] = (f"{n} sets of {min(map(len, ex))}..{max(map(len, ex))} regions == fold; {sample} == numpy "
                                       "reduce of the other sets, any_overlaps both ways")
    for k in ("device", "library_fold"):
        res[k][f"folds_shape_{tag}"] = shape
    flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=200)
    ap.add_argument("--set-regions", type=int, default=50_000)
    ap.add_argument("--big", type=int, default=10_000_000)
    ap.add_argument("--cpu-big", type=int, default=1_000_000)
    ap.add_argument("--cpu-sets", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--fold-sets", type=int, default=64)
    ap.add_argument("--fold-set-regions", type=int, default=200_000)
    ap.add_argument("--only", choices=("folds", "algebra"), default=None)
    a = ap.parse_args()
    res = {"device": {}, "cpu_restatement": {}, "library_fold": {}, "checks": {}}
    u = synth.make_universe(100_000)

    def flush():
        if a.json:
            with open(a.json, "w") as f:
                json.dump(res, f, indent=1)

    if a.only != "algebra":
        # ---- folds over a list: the pairwise shape, then --fold-sets x --fold-set-regions
        for tag, n_sets, per, seed in (("a", a.sets, a.set_regions, 1000), ("b", a.fold_sets, a.fold_set_regions, 5000)):
            made = [make_set(per, seed + 7 * k, u) for k in range(n_sets)]
            bench_folds(res, tag, [q for q, _ in made], [rs for _, rs in made], a.reps, flush)
            del made
    if a.only == "folds":
        print(json.dumps(res))
        flush()
        return

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
    flush()


if __name__ == "__main__":
    main()
