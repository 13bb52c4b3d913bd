"""VRS allele identifiers (csrc/vrs.hip, K18) on the device: per-kernel times, the device entry on resident columns, the
column call and the file call, against the library's own host path on 16 threads and the plain-Python restatement, on
the synthetic hg38-shaped assembly of tools/seqstats_bench.py.

  python tools/vrs_bench.py [--scale 1.0] [--alleles 10000000] [--reps 10] [--json profiles/vrs_bench.json]

The alleles: 88 % SNVs at random places, 12 % insertions and deletions of one unit inside homopolymers and short tandem
repeats (units of 1 to 3 bases, 8 to 40 units) planted into the assembly, in (chromosome, position) order as a VCF has
them; the same alleles as a VCF file, one ALT per line with a short INFO field, indels in VCF's anchored form.
Per-kernel times come from the library's profiling scopes (HIP events around every launch), median of --reps calls after a warm-up; the entries by wall time,
median of --reps.  Baselines, in the same run: the library's host path (on_host) on 16 threads over all alleles, and
tests/vrs_ref.py on the first --sample alleles.  Checks, in the run: the device's statuses, intervals and digests equal the
host path's for every allele, the restatement's on the sample, and the file call's identifiers equal the column call's.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import gtars_amd  # noqa: E402
import vrs_ref  # noqa: E402
from gtars_amd import _lib  # noqa: E402
from gtars_amd import vrs as V  # noqa: E402
from gtars_amd.seqstats import BinaryGenomeAssembly  # noqa: E402
from seqstats_bench import chrom_sizes, make_assembly, write_fab  # noqa: E402

SLOT = 8  # pool bytes per allele: REF in the first four, ALT in the last four


def make_alleles(sizes, seqs, n, seed=5):
    """plants the repeats into seqs and -> columns (chrom, start, pool, ref_off, ref_len, alt_off, alt_len) in file order"""
    rng = np.random.default_rng(seed)
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    chrom = np.sort(rng.choice(len(seqs), n, p=lens / lens.sum())).astype(np.uint32)
    start = np.zeros(n, dtype=np.uint64)
    pool = np.zeros(n * SLOT, dtype=np.uint8)
    ref_len, alt_len = np.ones(n, dtype=np.uint32), np.ones(n, dtype=np.uint32)
    letters = np.frombuffer(b"ACGT", np.uint8)
    for c in range(len(seqs)):
        rows = np.flatnonzero(chrom == c)
        if not len(rows):
            continue
        s = seqs[c]
        pos = np.sort(rng.integers(64, len(s) - 256, len(rows)))
        indel = rng.random(len(rows)) < 0.12
        unit_len = rng.integers(1, 4, len(rows))
        units = rng.integers(8, 41, len(rows))
        # plant the repeats (later ones may overwrite earlier ones: the alleles are cut from the final bytes below)
        for k in np.flatnonzero(indel):
            u = letters[rng.integers(0, 4, unit_len[k])]
            if unit_len[k] > 1 and (u == u[0]).all():
                u[-1] = letters[(np.flatnonzero(letters == u[0])[0] + 1) % 4]
            s[pos[k]:pos[k] + unit_len[k] * units[k]] = np.tile(u, units[k])
        start[rows] = pos
        base = rows.astype(np.int64) * SLOT
        ref0 = s[pos] & 0xDF
        ref0[ref0 == ord("N")] = ord("A")
        # SNV: REF as the assembly has it (upper-cased), ALT the next letter
        pool[base] = np.where(s[pos] & 0xDF == ord("N"), s[pos], ref0)
        code = np.searchsorted(letters, ref0)
        pool[base + 4] = letters[(code + 1) % 4]
        for k in np.flatnonzero(indel):
            ul = int(unit_len[k])
            at, b = int(pos[k]) + ul * int(rng.integers(0, units[k] - 1)), int(base[k])
            unit = s[at:at + ul] & 0xDF
            start[rows[k]] = at
            if rng.random() < 0.5:  # insertion of one unit, anchored VCF style on the base before
                ref_len[rows[k]], alt_len[rows[k]] = 0, ul
                pool[b + 4:b + 4 + ul] = unit
            else:
                ref_len[rows[k]], alt_len[rows[k]] = ul, 0
                pool[b:b + ul] = unit
    ref_off = (np.arange(n, dtype=np.uint64) * SLOT).astype(np.uint32)
    # REF must equal the final bytes (a later repeat may have overwritten an SNV's base)
    snv = (ref_len == 1) & (alt_len == 1)
    for c in range(len(seqs)):
        rows = np.flatnonzero((chrom == c) & snv)
        b = seqs[c][start[rows].astype(np.int64)]
        pool[rows.astype(np.int64) * SLOT] = b
        code = np.searchsorted(letters, np.where(np.isin(b & 0xDF, letters), b & 0xDF, ord("A")))
        pool[rows.astype(np.int64) * SLOT + 4] = letters[(code + 1) % 4]
    return chrom, start, pool, ref_off, ref_len, ref_off + 4, alt_len


def write_vcf(path, names, seqs, cols):
    """one ALT per line; insertions and deletions in VCF's anchored form (the base before, then REF / ALT): trimming takes the
    anchor off again, so the file's alleles normalize to the columns' identifiers"""
    chrom, start, pool, ref_off, ref_len, alt_off, alt_len = cols
    text = pool.tobytes()
    with open(path, "wb") as f:
        f.write(b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for lo in range(0, len(chrom), 200_000):
            hi = min(lo + 200_000, len(chrom))
            lines = []
            for i in range(lo, hi):
                r = text[ref_off[i]:ref_off[i] + ref_len[i]]
                a = text[alt_off[i]:alt_off[i] + alt_len[i]]
                pos = int(start[i])
                if not r or not a:
                    pos -= 1
                    anchor = bytes([int(seqs[chrom[i]][pos]) & 0xDF])
                    r, a = anchor + r, anchor + a
                lines.append(b"%s\t%d\t.\t%s\t%s\t.\tPASS\tAC=1;AF=0.001\n" % (names[chrom[i]], pos + 1, r, a))
            f.write(b"".join(lines))


def median_wall(fn, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--alleles", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available() and gtars_amd.device_count() > 0, "vrs_bench needs an MI355X"
    dev = torch.device("cuda", torch.cuda.current_device())
    n = args.alleles
    sizes = chrom_sizes(args.scale)
    seqs = make_assembly(sizes)
    cols = make_alleles(sizes, seqs, n)
    chrom, start, pool, ref_off, ref_len, alt_off, alt_len = cols
    out = {"device": torch.cuda.get_device_name(0), "scale": args.scale, "alleles": n, "reps": args.reps,
           "assembly_bytes": int(sum(len(s) for s in seqs))}
    with tempfile.TemporaryDirectory() as tmp:
        fab = os.path.join(tmp, "asm.fab")
        write_fab(fab, sizes, seqs)
        g = BinaryGenomeAssembly(fab)
        names = [nm.encode() for nm in g.chrom_names]
        t0 = time.perf_counter()
        acc = g.refget_digests()
        out["refget_digests_s"] = time.perf_counter() - t0

        def host_call():
            status, ns, ne = np.zeros(n, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
            dig = np.zeros(32 * n, np.uint8)
            _lib.check(_lib.lib.gtars_vrs_alleles(g._h, None, _lib.ptr(chrom), _lib.ptr(start), _lib.ptr(pool), pool.size, _lib.ptr(ref_off),
                                                  _lib.ptr(ref_len), _lib.ptr(alt_off), _lib.ptr(alt_len), n, host_call.on_host,
                                                  args.host_threads, _lib.ptr(status), _lib.ptr(ns), _lib.ptr(ne), _lib.ptr(dig), None, None))
            return status, ns, ne, dig

        # the baseline: the library's host path
        host_call.on_host = 1
        t0 = time.perf_counter()
        h_status, h_ns, h_ne, h_dig = host_call()
        out["host_path_s"] = time.perf_counter() - t0
        out["host_path_threads"] = args.host_threads
        out["host_path_alleles_per_s"] = n / out["host_path_s"]
        assert (h_status == 0).all(), np.bincount(h_status)
        out["rolled_alleles"] = int(((h_ne - h_ns) > 4).sum())

        # the column call (host columns in, host columns out; the first one uploads the assembly)
        host_call.on_host = 0
        t0 = time.perf_counter()
        d_status, d_ns, d_ne, d_dig = host_call()
        out["first_column_call_s"] = time.perf_counter() - t0
        assert (d_status == h_status).all() and (d_ns == h_ns).all() and (d_ne == h_ne).all() and (d_dig == h_dig).all()
        out["column_call_s"] = median_wall(host_call, max(3, args.reps // 3))
        out["column_call_alleles_per_s"] = n / out["column_call_s"]

        # the restatement on a sample
        k = min(args.sample, n)
        text = pool.tobytes()
        rows = [(g.chrom_names[chrom[i]], int(start[i]), text[ref_off[i]:ref_off[i] + ref_len[i]], text[alt_off[i]:alt_off[i] + alt_len[i]])
                for i in range(k)]
        by_name = {nm: seqs[c].tobytes() for c, nm in enumerate(g.chrom_names) if nm in {r[0] for r in rows}}
        t0 = time.perf_counter()
        r_st, r_ns, r_ne, _, r_ids = vrs_ref.alleles(by_name, acc, rows)
        out["python_restatement_alleles_per_s"] = k / (time.perf_counter() - t0)
        raw = d_dig.tobytes()
        assert r_ids == ["ga4gh:VA." + raw[32 * i:32 * i + 32].decode() for i in range(k)]
        assert r_ns == d_ns[:k].tolist() and r_ne == d_ne[:k].tolist()

        # the device entry on resident columns, and the kernels inside it
        t = [torch.from_numpy(a.view(dt)).to(dev) for a, dt in ((chrom, np.int32), (start, np.int64), (pool, np.uint8), (ref_off, np.int32),
                                                                 (ref_len, np.int32), (alt_off, np.int32), (alt_len, np.int32))]
        o_status = torch.zeros(n, dtype=torch.uint8, device=dev)
        o_ns, o_ne = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
        o_dig = torch.zeros(32 * n, dtype=torch.uint8, device=dev)

        def device_entry():
            V.ids_device(g, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), pool.size, t[3].data_ptr(), t[4].data_ptr(), t[5].data_ptr(),
                         t[6].data_ptr(), n, o_status.data_ptr(), o_ns.data_ptr(), o_ne.data_ptr(), o_dig.data_ptr(),
                         torch.cuda.current_stream().cuda_stream)

        device_entry()
        assert (o_dig.cpu().numpy() == h_dig).all() and (o_ns.cpu().numpy().view(np.uint64) == h_ns).all()
        out["device_entry_s"] = median_wall(device_entry, args.reps)
        out["device_entry_alleles_per_s"] = n / out["device_entry_s"]
        _lib.lib.gtars_prof_enable(1)
        per_kernel = {}
        for _ in range(args.reps):
            _lib.lib.gtars_prof_reset()
            device_entry()
            for name, v in _lib.prof_read().items():
                if name.startswith("k_vrs"):
                    per_kernel.setdefault(name, []).append(v["total_ms"])
        _lib.lib.gtars_prof_enable(0)
        out["kernel_ms_median"] = {name: statistics.median(v) for name, v in per_kernel.items()}
        if "k_vrs_digest" in out["kernel_ms_median"]:
            out["digest_kernel_alleles_per_s"] = n / (out["kernel_ms_median"]["k_vrs_digest"] * 1e-3)

        # the file call
        vcf = os.path.join(tmp, "alleles.vcf")
        write_vcf(vcf, names, seqs, cols)
        out["vcf_bytes"] = os.path.getsize(vcf)
        t0 = time.perf_counter()
        res = V.compute_vrs_ids(vcf, g)
        out["file_call_s"] = time.perf_counter() - t0
        assert len(res) == n, (len(res), n)
        assert res.vrs_id == ["ga4gh:VA." + raw[32 * i:32 * i + 32].decode() for i in range(n)]
        out["file_call_alleles"] = len(res)
        out["file_call_alleles_per_s"] = len(res) / out["file_call_s"]
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
