"""BAM to fragments (csrc/bam.hip + csrc/bam_frag.cpp, K26): where bam_to_fragments spends a call, next to compute_bam_qc on
the same file.

  python tools/bam_frag_bench.py [--reads 20000000] [--reps 10] [--warmup 2] [--threads 16] [--json out.json]

The synthetic coordinate-sorted paired-end BAM of tools/bamqc_bench.py (about 10 % of the pairs repeat another pair's position
and template length), every record extended with a CB:Z tag: one of 10000 barcodes of 18 bytes, a function of the pair's
position and length, so that both mates carry the same barcode and a repeated pair repeats it.

  wall             bam_to_fragments(path, plain text output), open included: median of --reps after --warmup (min, max)
  host stages      read + block table + header, inflate on the host threads, the record walk (gtars_bam_last_stages)
  device stages    the new kernels and sorts from the library's profiling mode, median of 3 profiled calls
  qc               compute_bam_qc on the same file in the same run, and the ratio of the two walls: both calls share the read,
                   the inflate and the walk, so the QC call is the yardstick for what the fragment call adds
  restatement      tests/bam_frag_ref.py's fragments_ref on the small file, reads per second

Checked in the run: every row, barcode and statistic of a small file of the same shape against the restatement; on the large
file records = the reasons + kept_pairs and the sum of the count column = kept_pairs."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bamqc_bench as Q  # noqa: E402

N_BARCODES, CB_LEN = 10_000, 18
AUX_LEN = 3 + CB_LEN + 1
REC = np.dtype(Q.REC.descr + [("aux", "u1", AUX_LEN)])
REASONS = ("unplaced", "flag", "mapq", "mate_ref", "not_leftmost", "too_long", "no_barcode", "empty")


def barcode_table(seed: int = 23) -> np.ndarray:
    """[N_BARCODES, AUX_LEN] bytes: CB Z, sixteen letters, "-1", NUL"""
    rng = np.random.default_rng(seed)
    t = np.zeros((N_BARCODES, AUX_LEN), dtype=np.uint8)
    t[:, :3] = np.frombuffer(b"CBZ", dtype=np.uint8)
    t[:, 3:3 + CB_LEN - 2] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, (N_BARCODES, CB_LEN - 2))]
    t[:, 3 + CB_LEN - 2:3 + CB_LEN] = np.frombuffer(b"-1", dtype=np.uint8)
    return t


def make_records(refs, n_reads: int, seed: int = 17) -> np.ndarray:
    base = Q.make_records(refs, n_reads, seed)
    r = np.zeros(len(base), dtype=REC)
    for name in Q.REC.names:
        r[name] = base[name]
    r["block_size"] = REC.itemsize - 4
    tlen = base["tlen"].astype(np.int64)
    pos1 = np.where(tlen > 0, base["pos"].astype(np.int64), base["pos"].astype(np.int64) + tlen + Q.L_SEQ)  # the leftmost mate's position
    key = (pos1 * 2654435761 + np.abs(tlen) * 40503 + base["ref_id"].astype(np.int64) * 7919) % N_BARCODES
    r["aux"] = barcode_table()[key]
    return r


def frag_dict(stats):
    return {k: int(v) for k, v in stats.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--json")
    a = ap.parse_args()

    import gtars_amd
    from gtars_amd import _lib, bam, synth

    assert gtars_amd.device_count() > 0, "bam_frag_bench needs an MI355X"
    import bam_frag_ref as F

    refs = [(n, int(s)) for n, s in synth.HG38]
    procs = max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "16"))))
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "fragments.tsv")
        # ---- a small file of the same shape: every row against the restatement
        small = os.path.join(tmp, "small.bam")
        Q.write_bam(small, refs, make_records(refs, 20_000, seed=5), 1)
        s_refs, s_recs = F.read_bam(small)
        t0 = time.perf_counter()
        rows, barcodes, want, text = F.fragments_ref(s_refs, s_recs)
        ref_s = time.perf_counter() - t0
        with bam.BamFile(small) as b:
            fr = b.fragments(threads=a.threads, max_window_bytes=1 << 20)
        got_rows = list(zip(fr.ref.tolist(), fr.start.tolist(), fr.end.tolist(), fr.barcode.tolist(), fr.count.tolist()))
        assert got_rows == rows and fr.barcodes == [x.decode() for x in barcodes] and fr.stats == want, (fr.stats, want)
        assert bam.bam_to_fragments(small, out, threads=a.threads) == want and open(out, "rb").read() == text
        assert want["fragments"] < want["kept_pairs"] and want["barcodes"] > 1000
        print(f"[bam_frag_bench] 20000 reads against fragments_ref: ok {want}", flush=True)

        # ---- the large file
        t0 = time.perf_counter()
        recs = make_records(refs, a.reads)
        path = os.path.join(tmp, "large.bam")
        n_stream = Q.write_bam(path, refs, recs, procs)
        n_reads = len(recs)
        del recs
        gen_s = time.perf_counter() - t0
        n_file = os.path.getsize(path)
        print(f"[bam_frag_bench] {n_reads} reads written in {gen_s:.1f} s: {n_file / 1e6:.1f} MB, {n_stream / 1e6:.1f} MB inflated", flush=True)

        def call():
            return bam.bam_to_fragments(path, out, threads=a.threads)

        def qc():
            return bam.compute_bam_qc(path, threads=a.threads)

        stats = frag_dict(call())
        assert stats["records"] == n_reads == sum(stats[k] for k in REASONS) + stats["kept_pairs"], stats
        with bam.BamFile(path) as b:
            fr = b.fragments(threads=a.threads)
        assert int(fr.count.astype(np.uint64).sum()) == stats["kept_pairs"] and len(fr) == stats["fragments"] == sum(1 for _ in open(out, "rb"))
        del fr
        n_text = os.path.getsize(out)
        print(f"[bam_frag_bench] the statistics identities hold: ok {stats}", flush=True)

        def timed(fn, stages):
            for _ in range(a.warmup):
                fn()
            walls = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                fn()
                walls.append((time.perf_counter() - t0) * 1e3)
                for k, v in bam.last_stages().items():
                    stages.setdefault(k, []).append(v * 1e3 if k.endswith("_s") else v)
            return walls

        stages, qc_stages = {}, {}
        walls = timed(call, stages)
        qc_walls = timed(qc, qc_stages)
        per_kernel = {}
        _lib.lib.gtars_prof_enable(1)
        try:
            for _ in range(3):
                _lib.lib.gtars_prof_reset()
                call()
                for k, v in _lib.prof_read().items():
                    per_kernel.setdefault(k, []).append(v["total_ms"])
        finally:
            _lib.lib.gtars_prof_enable(0)
            _lib.lib.gtars_prof_reset()

    def host(st):
        return {k.replace("_s", "_ms"): Q.stat(v) for k, v in st.items() if k.endswith("_s")}

    wall, qc_wall = Q.stat(walls), Q.stat(qc_walls)
    row = {"reads": n_reads, "file_bytes": n_file, "inflated_bytes": n_stream, "text_bytes": n_text, "generation_s": gen_s, "threads": a.threads,
           "checks": "ok", "stats": stats, "windows": int(stages["windows"][0]), "wall_ms": wall, "host_stages_ms": host(stages),
           "device_stages_ms": {k: Q.stat(v) for k, v in sorted(per_kernel.items())}, "qc_wall_ms": qc_wall, "qc_host_stages_ms": host(qc_stages),
           "fragments_over_qc": wall[0] / qc_wall[0], "reads_per_s": n_reads / (wall[0] / 1e3),
           "restatement_reads_per_s": 20_000 / ref_s}
    print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
