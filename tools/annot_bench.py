"""TSS / feature distances and GTF gene models (csrc/annot.hip, K10) on the device vs the plain-Python restatement
(tests/annot_ref.py).

  python tools/annot_bench.py [--genes 60000] [--exons 1500000] [--queries 10000000] [--features 1000000] [--reps 3]
                              [--cpu-queries 200000] [--json out.json]

Measures, on a GENCODE-shaped synthetic GTF (--genes gene rows, --exons exon rows, 25 hg38-sized chromosomes): the
host parse (GeneModel.from_gtf's reader) and the two stranded reduces on the device; the build of the TSS index of the
reduced genes; --queries regions against that TSS index and against a --features index, BED-sorted and shuffled: the
device time of the distance kernel by HIP events (profiling mode), the library call (columns in, both result vectors
out) and the Python calls calc_tss_distances / feature_distances (lists included).  Wall times are the best of --reps
after a warm-up.  Every output is checked: the reader against the restatement's parser, the reduces against its
stranded reduce, the distances at full size against a numpy restatement and on --cpu-queries against the restatement
itself, which is timed there.  The search forms (LDS-staged sampled keys / global memory only) are A/B'd in the run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import annot_ref as A  # noqa: E402

from gtars_amd import _lib  # noqa: E402
from gtars_amd import models as M  # noqa: E402
from gtars.models import GenomicDistAnnotation, RegionSet, TssIndex  # noqa: E402

U32 = 0xFFFFFFFF
I64_MAX = (1 << 63) - 1
CHROMS = [(f"{k}", n) for k, n in zip(list(range(1, 23)) + ["X", "Y", "MT"],
                                       [248956422, 242193529, 198295559, 190214555, 181538259, 170805979, 159345973,
                                        145138636, 138394717, 133797422, 135086622, 133275309, 114364328, 107043718,
                                        101991189, 90338345, 83257441, 80373285, 58617616, 64444167, 46709983, 50818468,
                                        156040895, 57227415, 16569])]


def best_of(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3


def write_gtf(path, n_genes, n_exons, rng):
    w = np.array([n for _, n in CHROMS], dtype=np.float64)
    gc = rng.choice(len(CHROMS), n_genes, p=w / w.sum())
    # (MT is shorter than the 200 kb margin: a gene drawn there starts at 1)
    gs = np.maximum((rng.random(n_genes) * (np.array([n for _, n in CHROMS])[gc] - 200_000)).astype(np.int64), 0) + 1
    glen = rng.integers(500, 150_000, n_genes)
    gst = rng.choice(np.array(["+", "-"]), n_genes)
    pc = rng.random(n_genes) < 0.35
    per = rng.multinomial(n_exons, np.ones(n_genes) / n_genes)
    lines = ["#!genome-build synthetic"]
    names = [c for c, _ in CHROMS]
    eg = np.repeat(np.arange(n_genes), per)
    off = rng.random(n_exons) * glen[eg]
    es = gs[eg] + off.astype(np.int64)
    ee = es + rng.integers(50, 400, n_exons)
    for g in range(n_genes):
        bio = 'gene_type "protein_coding"' if pc[g] else 'gene_type "lncRNA"'
        attr = f'gene_id "ENSG{g:011d}.1"; {bio}; gene_name "G{g}";'
        lines.append(f"{names[gc[g]]}\tHAVANA\tgene\t{gs[g]}\t{gs[g] + glen[g]}\t.\t{gst[g]}\t.\t{attr}")
    k = 0
    for g in range(n_genes):
        bio = 'gene_type "protein_coding"' if pc[g] else 'gene_type "lncRNA"'
        pre = f"{names[gc[g]]}\tHAVANA\texon\t"
        post = f"\t.\t{gst[g]}\t.\tgene_id \"ENSG{g:011d}.1\"; transcript_id \"ENST{g:011d}.1\"; {bio};"
        for _ in range(per[g]):
            lines.append(f"{pre}{es[k]}\t{ee[k]}{post}")
            k += 1
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def make_queries(n, rng, names):
    sizes = dict(CHROMS)
    c = rng.integers(0, len(names), n)
    lim = np.array([sizes.get(nm.replace("chr", ""), 10_000_000) for nm in names], dtype=np.int64)
    s = (rng.random(n) * (lim[c] - 2000)).astype(np.int64)
    e = s + rng.integers(100, 1000, n)
    return c, s, e


def np_distances(index_c, index_mid, names, qc, qs, qe):
    """numpy restatement: first-appearance grouping, lower bound per chromosome, the upstream neighbour on a tie"""
    rank = np.full(len(names), -1, dtype=np.int64)
    _, first = np.unique(qc, return_index=True)
    for r, code in enumerate(qc[np.sort(first)]):
        rank[code] = r
    order = np.argsort(rank[qc], kind="stable")
    t = (qs + ((qe - qs) & U32) // 2) & U32
    ab = np.full(len(qc), U32, dtype=np.int64)
    sg = np.full(len(qc), I64_MAX, dtype=np.int64)
    present = set(index_c.tolist())
    for code, nm in enumerate(names):
        sel = qc == code
        mids = np.sort(index_mid[index_c == nm]) if nm in present else None
        if mids is None or not sel.any():
            continue
        tt = t[sel]
        p = np.searchsorted(mids, tt, "left")
        has_r = p < len(mids)
        has_l = p > 0
        r = np.where(has_r, mids[np.minimum(p, len(mids) - 1)], 0) - tt
        l_ = tt - np.where(has_l, mids[np.maximum(p - 1, 0)], 0)
        take_l = has_l & (~has_r | (l_ <= r))
        a = np.where(take_l, l_, r)
        s_ = np.where(take_l, -l_, r)
        exact = has_r & (r == 0)
        ab[sel] = np.where(exact, 0, a)
        sg[sel] = np.where(exact, 0, s_)
    return ab[order], sg[order]


def kernel_ms(fn, reps):
    fn()
    _lib.lib.gtars_prof_enable(1)
    _lib.lib.gtars_prof_reset()
    for _ in range(reps):
        fn()
    p = _lib.prof_read()
    _lib.lib.gtars_prof_enable(0)
    e = p.get("tss_distance_kernel", {"total_ms": float("nan"), "launches": 1})
    return e["total_ms"] / max(e["launches"], 1)


def set_form(global_search: bool):
    if global_search:
        os.environ["GTARS_TSS_GLOBAL_SEARCH"] = "1"
    else:
        os.environ.pop("GTARS_TSS_GLOBAL_SEARCH", None)
    _lib.reload_env()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genes", type=int, default=60_000)
    ap.add_argument("--exons", type=int, default=1_500_000)
    ap.add_argument("--queries", type=int, default=10_000_000)
    ap.add_argument("--features", type=int, default=1_000_000)
    ap.add_argument("--cpu-queries", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(1)
    res = {"genes_rows": a.genes, "exon_rows": a.exons, "queries": a.queries, "features": a.features}
    tmp = tempfile.mkdtemp()
    gtf = os.path.join(tmp, "gencode_like.gtf")
    write_gtf(gtf, a.genes, a.exons, rng)
    res["gtf_mb"] = round(os.path.getsize(gtf) / 1e6, 1)

    # --- load: host parse, device reduces
    res["gtf_parse_ms"] = best_of(lambda: M._read_gtf(gtf, False, True), a.reps)
    rows, strand, feature = M._read_gtf(gtf, False, True)
    red = {}

    def reduce_both():
        red["g"] = M._stranded_reduce(rows, strand, feature == 0)
        red["e"] = M._stranded_reduce(rows, strand, feature == 1)

    res["stranded_reduce_ms"] = best_of(reduce_both, a.reps)
    res["from_gtf_ms"] = best_of(lambda: GenomicDistAnnotation.from_gtf(gtf, False, True), a.reps)
    t0 = time.perf_counter()
    ref_rows = A.read_gtf(gtf, False, True)
    res["python_parse_ms"] = (time.perf_counter() - t0) * 1e3
    names, ids, s, e = rows.chrom_names, rows.chrom_ids, rows.starts, rows.ends
    assert len(ref_rows) == len(rows)
    assert [r[1] for r in ref_rows] == s.tolist() and [r[2] for r in ref_rows] == e.tolist()
    assert [r[0] for r in ref_rows] == [names[i] for i in ids.tolist()]
    assert [r[3] for r in ref_rows] == strand.tolist() and [r[4] for r in ref_rows] == feature.tolist()
    t0 = time.perf_counter()
    genes, exons = A.gene_model(ref_rows)
    res["python_reduce_ms"] = (time.perf_counter() - t0) * 1e3
    for part, want in ((red["g"], genes), (red["e"], exons)):
        rs = part.regions
        nm, ii, ss, ee = rs.chrom_names, rs.chrom_ids, rs.starts, rs.ends
        got = [(nm[int(ii[k])], int(ss[k]), int(ee[k]), int(part.strands[k])) for k in range(len(rs))]
        assert got == want
    res["n_genes"], res["n_exons"] = len(genes), len(exons)

    # --- indexes
    gda = GenomicDistAnnotation.from_gtf(gtf, False, True)
    tss_regs = A.tss_regions(genes)
    frng = np.random.default_rng(2)
    fc, fs, fe = make_queries(a.features, frng, [f"chr{c}" for c, _ in CHROMS])
    fnames = np.array([f"chr{c}" for c, _ in CHROMS], dtype=object)
    feat_rs = RegionSet.from_vectors(list(fnames[fc]), fs, fe)
    build = []
    for _ in range(a.reps):
        t = gda.tss_index()
        one = RegionSet.from_vectors(["chr1"], [5], [6])
        t0 = time.perf_counter()
        t._distances(one)
        build.append((time.perf_counter() - t0) * 1e3)
    res["tss_index_build_ms"] = min(build)
    build = []
    for _ in range(a.reps):
        t = TssIndex.from_regionset(feat_rs)
        one = RegionSet.from_vectors(["chr1"], [5], [6])
        t0 = time.perf_counter()
        t._distances(one)
        build.append((time.perf_counter() - t0) * 1e3)
    res["feature_index_build_ms"] = min(build)
    indexes = {
        "tss": (gda.tss_index(), np.array([r[0] for r in tss_regs], dtype=object), np.array([r[1] for r in tss_regs], dtype=np.int64)),
        "features": (TssIndex.from_regionset(feat_rs), fnames[fc], ((fs + ((fe - fs) & U32) // 2) & U32).astype(np.int64)),
    }

    # --- queries: BED-sorted (a file, read as the reference reads it) and shuffled (from_vectors, interleaved)
    qnames = [f"chr{c}" for c, _ in CHROMS] + ["chrUn_1"]
    qc, qs, qe = make_queries(a.queries, np.random.default_rng(3), qnames)
    qn = np.array(qnames, dtype=object)
    bed = os.path.join(tmp, "q.bed")
    byte_rank = np.argsort(np.argsort([nm.encode() for nm in qnames], kind="stable"))
    o = np.lexsort((qs, byte_rank[qc]))
    with open(bed, "w") as f:
        for k in o:
            f.write(f"{qnames[qc[k]]}\t{qs[k]}\t{qe[k]}\n")
    sorted_rs = RegionSet(bed)
    shuffled_rs = RegionSet.from_vectors(list(qn[qc]), qs, qe)
    queries = {"sorted": (sorted_rs, qc[o], qs[o], qe[o]), "shuffled": (shuffled_rs, qc, qs, qe)}

    for iname, (ix, ic, imid) in indexes.items():
        for qname, (rs, c, s_, e_) in queries.items():
            key = f"{iname}_{qname}"
            ab, sg = ix._distances(rs)
            want_ab, want_sg = np_distances(ic, imid, qnames, c, s_, e_)
            assert np.array_equal(ab.astype(np.int64), want_ab) and np.array_equal(sg, want_sg), key
            r = {}
            forms = {}
            for rnd in range(2):  # the two search forms, alternating
                for gs in (False, True):
                    set_form(gs)
                    forms.setdefault("global" if gs else "lds", []).append(kernel_ms(lambda: ix._distances(rs), a.reps))
            set_form(False)
            r["kernel_ms_lds"] = min(forms["lds"])
            r["kernel_ms_global"] = min(forms["global"])
            r["call_ms"] = best_of(lambda: ix._distances(rs), a.reps)
            r["calc_tss_distances_ms"] = best_of(lambda: ix.calc_tss_distances(rs), 1)
            r["feature_distances_ms"] = best_of(lambda: ix.feature_distances(rs), 1)
            res[key] = r
            print(key, r, flush=True)

    # --- the restatement on a share of the same work (the sorted set's head: BED order)
    n = min(a.cpu_queries, a.queries)
    sub = [(qnames[c], int(s_), int(e_)) for c, s_, e_ in zip(queries["shuffled"][1][:n], queries["shuffled"][2][:n],
                                                                queries["shuffled"][3][:n])]
    idx = A.build_index(tss_regs)
    t0 = time.perf_counter()
    want = A.distances(idx, sub)
    res["python_distances_ms_at_cpu_queries"] = (time.perf_counter() - t0) * 1e3
    res["cpu_queries"] = n
    sub_rs = RegionSet.from_vectors([r[0] for r in sub], [r[1] for r in sub], [r[2] for r in sub])
    ix = indexes["tss"][0]
    assert ix.calc_tss_distances(sub_rs) == want[0] and ix.feature_distances(sub_rs) == want[1]
    res["device_call_ms_at_cpu_queries"] = best_of(lambda: ix._distances(sub_rs), a.reps)
    print(json.dumps(res))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
