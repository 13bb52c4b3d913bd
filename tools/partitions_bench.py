"""calc_partitions (csrc/partitions.hip, K14) on the device against a composition of what the library had before it.

  python tools/partitions_bench.py [--genes 60000] [--exons 300000] [--queries 1000000,10000000] [--reps 10] [--json out.json]

A GENCODE-shaped synthetic GTF (tools/annot_bench.py writes it; exon minus CDS gives no UTRs there, so the list is
promoterCore / promoterProx / exon / intron) and hg38-shaped queries, BED-sorted and shuffled, in both modes.  Times are
device times by HIP events (the library's profiling mode), the median of --reps single calls with min and max:

  fused        k_partitions, one launch
  composition  priority: P calls of RegionSet.any_overlaps (the counting kernels only: index builds and sorts left
               out), then first hit in numpy; bp: no device composition exists, the check is torch prefix sums on the host

Every output is checked in the run: priority counts and per-region assignments against the any_overlaps composition, bp
counts against F(qe) - F(qs) over torch cumulative sums of each partition's sorted starts and ends."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import annot_bench as AB  # noqa: E402

from gtars_amd import _lib  # noqa: E402
from gtars.models import RegionSet  # noqa: E402
from gtars.partitions import PartitionList, calc_partitions, partition_assignments  # noqa: E402

U32 = 0xFFFFFFFF
QUERY_KERNELS = ("k_count", "k_bits_count")  # what an any_overlaps call runs against a built index


def profiled(fn, reps, pick):
    """per-call device ms of the profiling entries pick(name) accepts: (median, min, max, names seen)"""
    fn()
    _lib.lib.gtars_prof_enable(1)
    ms, seen = [], set()
    try:
        for _ in range(reps):
            _lib.lib.gtars_prof_reset()
            fn()
            p = _lib.prof_read()
            seen |= {k for k in p if pick(k)}
            ms.append(sum(v["total_ms"] for k, v in p.items() if pick(k)))
    finally:
        _lib.lib.gtars_prof_enable(0)
    assert seen, "no profiling entry matched: the time would read 0 ms and mean nothing"
    return float(np.median(ms)), min(ms), max(ms), sorted(seen)


def bp_by_prefix_sums(sets, names, qc, qs, qe):
    """per partition sum over queries of F(qe) - F(qs), F(x) = sum min(e, x) - sum min(s, x), in torch on the host"""
    import torch

    out = []
    tq = {k: torch.from_numpy(v.astype(np.int64)) for k, v in (("s", qs), ("e", qe))}
    for rs in sets:
        pn = rs.chrom_names
        pid, ps, pe = rs.chrom_ids, rs.starts.astype(np.int64), rs.ends.astype(np.int64)
        total = 0
        for code, nm in enumerate(names):
            if nm not in pn:
                continue
            sel = torch.from_numpy(np.flatnonzero(qc == code))
            rows = pid == pn.index(nm)
            if not len(sel) or not rows.any():
                continue
            f = {}
            for key, col in (("s", ps[rows]), ("e", pe[rows])):
                srt = torch.sort(torch.from_numpy(col)).values
                pre = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(srt, 0)])
                for x in ("s", "e"):
                    v = tq[x][sel]
                    j = torch.searchsorted(srt, v)
                    f[key, x] = pre[j] + (len(srt) - j) * v
            total += int(((f["e", "e"] - f["s", "e"]) - (f["e", "s"] - f["s", "s"])).sum())
        out.append(total & U32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=60000)
    ap.add_argument("--exons", type=int, default=300000)
    ap.add_argument("--queries", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json")
    a = ap.parse_args()
    rng = np.random.default_rng(14)
    with tempfile.TemporaryDirectory() as d:
        gtf = os.path.join(d, "synthetic.gtf")
        AB.write_gtf(gtf, a.genes, a.exons, rng)
        pl = PartitionList.from_gtf(gtf, 100, 2000, False, True)
    names = pl.partition_names()
    sets = [pl.partition(n) for n in names]
    print(f"partition list: " + ", ".join(f"{n} {len(s)}" for n, s in zip(names, sets)), flush=True)
    results = []
    for nq in (int(x) for x in a.queries.split(",")):
        qnames = ["chr" + c for c, _ in AB.CHROMS]
        c, s, e = AB.make_queries(nq, rng, qnames)
        order = np.lexsort((s, c))
        for label, idx in (("sorted", order), ("shuffled", rng.permutation(nq))):
            qc, qs, qe = c[idx], s[idx], e[idx]
            q = RegionSet.from_vectors([qnames[k] for k in qc], qs, qe)
            # priority: fused against P any_overlaps calls and a first hit in numpy
            flags = np.stack([np.asarray(q.any_overlaps(rs), dtype=bool) for rs in sets])
            want = np.where(flags.any(0), flags.argmax(0), len(sets))
            got = partition_assignments(q, pl)
            r = calc_partitions(q, pl)
            assert np.array_equal(got, want), "priority assignments differ from the any_overlaps composition"
            assert r["count"] == np.bincount(want, minlength=len(sets) + 1).tolist() and r["total"] == nq
            fused = profiled(lambda: calc_partitions(q, pl), a.reps, lambda k: k == "partitions_priority_kernel")
            comp = profiled(lambda: [q.any_overlaps(rs) for rs in sets], a.reps, lambda k: k.startswith(QUERY_KERNELS))
            # bp: fused against torch prefix sums
            rb = calc_partitions(q, pl, True)
            wb = bp_by_prefix_sums(sets, qnames, qc, qs, qe)
            tot = int(((qe - qs) & U32).sum()) & U32
            assert rb["count"][:-1] == wb and rb["total"] == tot and rb["count"][-1] == max(tot - (sum(wb) & U32), 0), "bp counts differ"
            fused_bp = profiled(lambda: calc_partitions(q, pl, True), a.reps, lambda k: k == "partitions_bp_kernel")
            row = {"queries": nq, "order": label, "checks": "ok",
                   "priority_fused_ms": fused[:3], "priority_composition_ms": comp[:3], "composition_kernels": comp[3],
                   "bp_fused_ms": fused_bp[:3]}
            results.append(row)
            print(f"{nq:>9} {label:<8} priority fused {fused[0]:.3f} ms [{fused[1]:.3f}, {fused[2]:.3f}]   "
                  f"composition {comp[0]:.3f} ms [{comp[1]:.3f}, {comp[2]:.3f}] ({'+'.join(comp[3])})   "
                  f"bp fused {fused_bp[0]:.3f} ms [{fused_bp[1]:.3f}, {fused_bp[2]:.3f}]   checks ok", flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
