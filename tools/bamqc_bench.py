"""BAM QC (csrc/bam.cpp + csrc/bam.hip, K17): where compute_bam_qc spends a call.

  python tools/bamqc_bench.py [--reads 20000000] [--reps 10] [--warmup 2] [--threads 16] [--json out.json]

One synthetic coordinate-sorted paired-end BAM: --reads records (half as many pairs) over the hg38 reference names, about 5 % of
them on chrM and about 10 % of the pairs repeating another pair's four-tuple; the records are built with numpy and the BGZF
blocks are compressed by a pool of at most 16 processes.

  wall             compute_bam_qc(path), open included: median of --reps after --warmup (min, max)
  host stages      read + block table + header, inflate on the host threads, the record walk (gtars_bam_last_stages; the inflate
                   of window k + 1 runs while window k is on the device)
  device stages    host-to-device copies, k_bam_decode, the per-window QC step and the per-chromosome join and key counts, from the
                   library's profiling mode (HIP events around each), median of 3 profiled calls

Checked in the run: a small file of the same shape against tests/bam_ref.py's restatement of bamqc.rs, and the large file against
itself under GTARS_BAM_NAME_HASH_BITS=16."""
from __future__ import annotations

import argparse
import json
import multiprocessing
import os
import struct
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BLOCK = 0xFF00
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
L_SEQ, NAME_LEN = 50, 11  # "f0000000000": one name per pair
REC = np.dtype([("block_size", "<u4"), ("ref_id", "<i4"), ("pos", "<i4"), ("l_read_name", "u1"), ("mapq", "u1"), ("bin", "<u2"),
                ("n_cigar", "<u2"), ("flag", "<u2"), ("l_seq", "<i4"), ("next_ref", "<i4"), ("next_pos", "<i4"), ("tlen", "<i4"),
                ("name", "S%d" % (NAME_LEN + 1)), ("cigar", "<u4"), ("seq", "u1", (L_SEQ + 1) // 2), ("qual", "u1", L_SEQ)])


def stat(v):
    return [float(np.median(v)), float(min(v)), float(max(v))]


def bgzf_block(data: bytes) -> bytes:
    co = zlib.compressobj(1, zlib.DEFLATED, -15)
    comp = co.compress(data) + co.flush()
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def header(refs) -> bytes:
    out = b"BAM\1" + struct.pack("<i", 0) + struct.pack("<i", len(refs))
    for name, length in refs:
        nm = name.encode() + b"\0"
        out += struct.pack("<i", len(nm)) + nm + struct.pack("<i", int(length))
    return out


def make_records(refs, n_reads: int, seed: int = 17) -> np.ndarray:
    """coordinate-sorted paired-end records: pairs spread over the references by length, chrM at 5 %"""
    rng = np.random.default_rng(seed)
    n_pairs = n_reads // 2
    sizes = np.array([s for _, s in refs], dtype=np.float64)
    mito = [i for i, (n, _) in enumerate(refs) if n == "chrM"]
    share = sizes / sizes[[i for i in range(len(refs)) if i not in mito]].sum() * 0.95
    share[mito] = 0.05
    counts = np.floor(share * n_pairs).astype(np.int64)
    counts[0] += n_pairs - counts.sum()
    out, first = [], 0
    for c, k in enumerate(counts.tolist()):
        if not k:
            continue
        size = int(refs[c][1])
        pos1 = rng.integers(0, max(size - 1000, 1), k)
        insert = rng.integers(100, 400, k)
        dup = rng.random(k) < 0.10  # these pairs repeat another pair's tuple
        src = rng.integers(0, k, k)
        pos1 = np.where(dup, pos1[src], pos1)
        insert = np.where(dup, insert[src], insert)
        r = np.zeros(2 * k, dtype=REC)
        r["block_size"] = REC.itemsize - 4
        r["ref_id"] = c
        r["next_ref"] = c
        r["l_read_name"] = NAME_LEN + 1
        r["mapq"] = 60
        r["bin"] = 4680
        r["n_cigar"] = 1
        r["l_seq"] = L_SEQ
        r["cigar"] = L_SEQ << 4
        r["seq"] = 0x12
        r["qual"] = 30
        ids = first + np.arange(k, dtype=np.int64)
        text = np.zeros((k, NAME_LEN + 1), dtype=np.uint8)  # "f" + ten digits + NUL
        text[:, 0] = ord("f")
        text[:, 1:NAME_LEN] = (ids[:, None] // 10 ** np.arange(NAME_LEN - 2, -1, -1, dtype=np.int64)) % 10 + ord("0")
        names = text.view("S%d" % (NAME_LEN + 1)).reshape(k)
        a, b = r[:k], r[k:]
        a["pos"], b["pos"] = pos1, pos1 + insert - L_SEQ
        a["next_pos"], b["next_pos"] = b["pos"], a["pos"]
        a["tlen"], b["tlen"] = insert, -insert
        a["flag"], b["flag"] = 0x1 | 0x2 | 0x40 | 0x20, 0x1 | 0x2 | 0x80 | 0x10
        dupflag = rng.random(k) < 0.03
        a["flag"] |= np.where(dupflag, 0x400, 0).astype(np.uint16)
        a["name"], b["name"] = names, names
        out.append(r[np.argsort(r["pos"], kind="stable")])
        first += k
    return np.concatenate(out) if out else np.zeros(0, dtype=REC)


def write_bam(path: str, refs, records: np.ndarray, procs: int) -> int:
    stream = header(refs) + records.tobytes()
    chunks = [stream[i:i + BLOCK] for i in range(0, len(stream), BLOCK)]
    with open(path, "wb") as f:
        if procs > 1 and len(chunks) > 64:
            with multiprocessing.Pool(procs) as pool:
                for blk in pool.imap(bgzf_block, chunks, chunksize=64):
                    f.write(blk)
        else:
            for c in chunks:
                f.write(bgzf_block(c))
        f.write(EOF_BLOCK)
    return len(stream)


def as_dict(r):
    return {k: getattr(r, k) for k in ("total_reads", "distinct", "m1", "m2", "dups", "mito_reads", "nrf", "pbc1", "pbc2")}


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

    assert gtars_amd.device_count() > 0, "bamqc_bench needs an MI355X"
    import bam_ref

    refs = list(synth.HG38)
    procs = max(1, min(16, int(os.environ.get("OMP_NUM_THREADS", "16"))))
    with tempfile.TemporaryDirectory() as tmp:
        # ---- a small file of the same shape against the restatement
        small = os.path.join(tmp, "small.bam")
        write_bam(small, refs, make_records(refs, 20_000, seed=5), 1)
        want = bam_ref.bam_qc_ref_file(small)
        got = as_dict(bam.compute_bam_qc(small, threads=a.threads, max_window_bytes=1 << 20))
        assert got == want, (got, want)
        print(f"[bamqc_bench] 20000 reads against bam_qc_ref: ok {got}", flush=True)

        # ---- the large file
        t0 = time.perf_counter()
        recs = make_records(refs, a.reads)
        path = os.path.join(tmp, "large.bam")
        n_stream = write_bam(path, refs, recs, procs)
        n_reads = len(recs)
        del recs
        gen_s = time.perf_counter() - t0
        n_file = os.path.getsize(path)
        print(f"[bamqc_bench] {n_reads} reads written in {gen_s:.1f} s: {n_file / 1e6:.1f} MB, {n_stream / 1e6:.1f} MB inflated", flush=True)

        def call():
            return bam.compute_bam_qc(path, threads=a.threads)

        res = as_dict(call())
        os.environ["GTARS_BAM_NAME_HASH_BITS"] = "16"
        _lib.reload_env()
        try:
            res16 = as_dict(call())
        finally:
            del os.environ["GTARS_BAM_NAME_HASH_BITS"]
            _lib.reload_env()
        assert res16 == res, (res16, res)
        print(f"[bamqc_bench] the same result with 16 hash bits: ok {res}", flush=True)

        for _ in range(a.warmup):
            call()
        walls, stages = [], {}
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            walls.append((time.perf_counter() - t0) * 1e3)
            for k, v in bam.last_stages().items():
                stages.setdefault(k, []).append(v * 1e3 if k.endswith("_s") else v)
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

    host = {k.replace("_s", "_ms"): stat(v) for k, v in stages.items() if k.endswith("_s")}
    row = {"reads": n_reads, "file_bytes": n_file, "inflated_bytes": n_stream, "generation_s": gen_s, "threads": a.threads, "checks": "ok",
           "result": res, "windows": int(stages["windows"][0]), "wall_ms": stat(walls), "host_stages_ms": host,
           "device_stages_ms": {k: stat(v) for k, v in sorted(per_kernel.items())},
           "reads_per_s": n_reads / (stat(walls)[0] / 1e3), "inflated_GB_per_s": n_stream / 1e9 / (stat(walls)[0] / 1e3)}
    print(json.dumps(row), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
