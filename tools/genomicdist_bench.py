"""Structural operations and region-set statistics (csrc/setops.hip, K9) on the device vs the plain-Python restatement
(tests/genomicdist_ref.py).

  python tools/genomicdist_bench.py [--big 10000000] [--sets 64] [--set-regions 200000] [--reps 3] [--json out.json]

Device figures are wall times of one library call (host columns in, host results out, the stream drained), the best of
--reps after a warm-up call: disjoin / chromosome_statistics / distribution / nearest_neighbors on --big synth.py regions,
consensus of --sets x --set-regions.  Every device output is checked: at full size against numpy restatements (consensus:
its union against the device reduce of the concatenation and its counts against the sum of the device any_overlaps over
the sets).  The pure-Python restatement is timed on a share of the same work (--cpu-big regions, --cpu-sets sets) and
compared with the device there.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import genomicdist_ref as G  # noqa: E402

from gtars_amd import synth  # noqa: E402
from gtars.genomic_distributions import consensus  # noqa: E402
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


def byte_rank(chrom):
    order = {nm: i for i, nm in enumerate(sorted(synth.CHROM_NAMES))}
    return np.array([order[nm] for nm in synth.CHROM_NAMES], dtype=np.int64)[chrom]


def rank_cols(rs):
    """a device result's chromosome column as bytewise ranks"""
    order = {nm: i for i, nm in enumerate(sorted(synth.CHROM_NAMES))}
    lut = np.array([order[nm] for nm in rs.chrom_names], dtype=np.int64)
    return lut[rs.chrom_ids] if len(rs) else np.zeros(0, dtype=np.int64)


def np_disjoin(rank, start, end):
    s, e = start.astype(np.int64), end.astype(np.int64)
    wf = (s < e).astype(np.int64)
    key = np.concatenate([rank * (1 << 32) + s, rank * (1 << 32) + e])
    delta = np.concatenate([wf, -wf])
    uk, inv = np.unique(key, return_inverse=True)
    depth = np.cumsum(np.bincount(inv, weights=delta, minlength=len(uk)).astype(np.int64))
    rk, pos = uk >> 32, uk & TOP
    keep = np.flatnonzero((rk[1:] == rk[:-1]) & (depth[:-1] > 0))
    return rk[keep], pos[keep], pos[keep + 1]


def np_stats(rank, start, end, n_rank):
    w = (end.astype(np.int64) - start.astype(np.int64)) & TOP
    o = np.lexsort((w, rank))
    ws, rs = w[o], rank[o]
    cnt = np.bincount(rank, minlength=n_rank)
    off = np.concatenate([[0], np.cumsum(cnt)])
    out = {}
    for r in np.flatnonzero(cnt):
        lo, c = off[r], cnt[r]
        seg = ws[lo:lo + c]
        med = float((int(seg[c // 2 - 1]) + int(seg[c // 2])) & TOP) / 2.0 if c % 2 == 0 else float(seg[c // 2])
        m = rank == r
        out[int(r)] = (int(c), int(start[m].min()), int(end[m].max()), int(seg[0]), int(seg[-1]),
                       float(int(seg.sum())) / c, med)
    return out


def np_nearest(chrom, start, end):
    _, first = np.unique(chrom, return_index=True)
    fa = np.empty(chrom.max() + 1, dtype=np.int64)
    fa[chrom[np.sort(first)]] = np.arange(len(first))
    r = fa[chrom]
    o = np.lexsort((end, start, r))
    r, s, e = r[o], start[o].astype(np.int64), end[o].astype(np.int64)
    same = r[1:] == r[:-1]
    d = np.where(same, np.maximum(s[1:] - e[:-1], 0), -1)
    left = np.concatenate([[-1], d])
    right = np.concatenate([d, [-1]])
    both = (left >= 0) & (right >= 0)
    val = np.where(both, np.minimum(left, right), np.maximum(left, right))
    return val[(left >= 0) | (right >= 0)]


def np_distribution(q, rs, n_bins):
    rank = byte_rank(q["chrom"])
    s, e = q["start"].astype(np.int64), q["end"].astype(np.int64)
    mid = (s + (((e - s) & TOP) // 2)) & TOP
    me = rs.get_max_end_per_chr()
    order = sorted(synth.CHROM_NAMES)
    lim = np.array([me.get(nm, 0) for nm in order], dtype=np.int64)
    bs = max(int(lim.max()) // n_bins, 1)
    rid = mid // bs
    key, cnt = np.unique(rank * (1 << 32) + rid, return_counts=True)
    kr, kid = key >> 32, key & TOP
    st = kid * bs
    return [{"chr": order[kr[i]], "start": int(st[i]), "end": int(min((st[i] + bs) & TOP, lim[kr[i]])), "n": int(cnt[i]),
             "rid": int(kid[i])} for i in range(len(key))]


def tuples(q, n=None):
    n = len(q["chrom"]) if n is None else n
    return [(synth.CHROM_NAMES[int(q["chrom"][i])], int(q["start"][i]), int(q["end"][i])) for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", type=int, default=10_000_000)
    ap.add_argument("--sets", type=int, default=64)
    ap.add_argument("--set-regions", type=int, default=200_000)
    ap.add_argument("--cpu-big", type=int, default=1_000_000)
    ap.add_argument("--cpu-sets", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    res = {"device": {}, "cpu_restatement": {}, "checks": {}}
    u = synth.make_universe(100_000)

    # ---- disjoin / chromosome_statistics / distribution / nearest_neighbors at --big
    q, A = make_set(a.big, 91, u)
    out = {}
    for name, fn in (("disjoin", A.disjoin), ("chromosome_statistics", A.chromosome_statistics),
                     ("distribution", A.distribution), ("nearest_neighbors", A.nearest_neighbors)):
        res["device"][f"{name}_ms"] = best_of(lambda: out.__setitem__(name, fn()), a.reps)
    res["device"]["big_shape"] = f"{len(A)} regions"
    rank = byte_rank(q["chrom"])
    rk, s, e = np_disjoin(rank, q["start"], q["end"])
    d = out["disjoin"]
    assert np.array_equal(rank_cols(d), rk) and np.array_equal(d.starts, s) and np.array_equal(d.ends, e)
    res["checks"]["disjoin_pieces"] = len(d)
    order = sorted(synth.CHROM_NAMES)
    want = np_stats(rank, q["start"], q["end"], len(order))
    got = {order.index(k): (v.number_of_regions, v.start_nucleotide_position, v.end_nucleotide_position,
                            v.minimum_region_length, v.maximum_region_length, v.mean_region_length, v.median_region_length)
           for k, v in out["chromosome_statistics"].items()}
    assert got == want
    assert out["distribution"] == np_distribution(q, A, 250)
    assert np.array_equal(np.asarray(out["nearest_neighbors"], dtype=np.int64), np_nearest(q["chrom"], q["start"], q["end"]))
    res["checks"]["big_full_size_numpy"] = True

    # ---- consensus of --sets x --set-regions
    cols, sets = [], []
    for k in range(a.sets):
        qk, rk_ = make_set(a.set_regions, 1000 + 7 * k, u)
        cols.append(qk)
        sets.append(rk_)
    cons = {}
    res["device"]["consensus_ms"] = best_of(lambda: cons.__setitem__("v", consensus(sets)), a.reps)
    res["device"]["consensus_shape"] = f"{a.sets} sets x {a.set_regions} regions"
    union = RegionSetList(sets).concat().reduce()
    got = cons["v"]
    assert [(x["chr"], x["start"], x["end"]) for x in got] == [(r.chr, r.start, r.end) for r in union]
    hits = np.zeros(len(union), dtype=np.int64)
    for st in sets:
        hits += np.asarray(union.any_overlaps(st), dtype=np.int64)
    assert [x["count"] for x in got] == hits.tolist()
    res["checks"]["consensus_vs_reduce_and_any_overlaps"] = len(got)

    # ---- the CPU restatement on a share of the same work, compared with the device there
    k = min(a.cpu_big, len(A))
    sa = tuples(q, k)
    As = RegionSet.from_vectors([t[0] for t in sa], [t[1] for t in sa], [t[2] for t in sa])
    stats = lambda rs: {c: (v.number_of_regions, v.start_nucleotide_position, v.end_nucleotide_position,  # noqa: E731
                            v.minimum_region_length, v.maximum_region_length, v.mean_region_length,
                            v.median_region_length) for c, v in rs.chromosome_statistics().items()}
    for name, cpu, dev in (("disjoin", lambda: G.disjoin(sa), lambda: [(r.chr, r.start, r.end) for r in As.disjoin()]),
                           ("chromosome_statistics", lambda: G.chromosome_statistics(sa), lambda: stats(As)),
                           ("distribution", lambda: G.distribution(sa), As.distribution),
                           ("nearest_neighbors", lambda: G.nearest_neighbors(sa), As.nearest_neighbors)):
        t0 = time.perf_counter()
        want = cpu()
        res["cpu_restatement"][f"{name}_ms"] = (time.perf_counter() - t0) * 1e3
        assert dev() == want, name
    res["cpu_restatement"]["big_shape"] = f"{k} regions"
    m = min(a.cpu_sets, a.sets)
    regs = [tuples(c) for c in cols[:m]]
    t0 = time.perf_counter()
    want = G.consensus(regs)
    res["cpu_restatement"]["consensus_ms"] = (time.perf_counter() - t0) * 1e3
    res["cpu_restatement"]["consensus_shape"] = f"{m} sets x {a.set_regions} regions"
    assert [(x["chr"], x["start"], x["end"], x["count"]) for x in consensus(sets[:m])] == want
    res["checks"]["cpu_vs_device_equal"] = True
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
