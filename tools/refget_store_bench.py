"""The refget store's encoded mode (csrc/refget_pack.hip, K22) on the device: k_refget_pack over a many-record FASTA and an
hg38-shaped assembly, the packed substring fill next to the raw one on the same 1e6 peaks, and opening a store from disk
against reading the FASTA again.

  python tools/refget_store_bench.py [--records 200000] [--scale 0.25] [--peaks 1000000] [--reps 10] [--json profiles/refget_store_bench.json]

The inputs are those of tools/refget_bench.py: --records records with RefSeq-like mature-mRNA lengths, and the synthetic
hg38-shaped assembly of tools/seqstats_bench.py at --scale (a quarter of hg38's lengths by default).  Per-kernel times come
from the library's profiling scopes (HIP events around every launch), median of --reps calls after a warm-up call;
k_refget_fill (the raw image, K21's kernel) and k_refget_fill_packed run on the same peaks in the same run.  open_local plus the
first region call and load_fasta plus the first region call are wall times of one cold call each.  Checks, in the run: the
device pack equals the host path's image byte for byte, every packed substring and every whole-record decode equals the raw
image's upper-cased bytes (the inputs hold A C G T N in both cases only, which every table maps back to itself).
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import gtars_amd  # noqa: E402
from gtars_amd import refget as G  # noqa: E402
from refget_bench import write_assembly, write_records  # noqa: E402
from reftx_bench import kernel_medians, make_transcripts, median_wall  # noqa: E402
from seqstats_bench import chrom_sizes, make_assembly  # noqa: E402


def note(text):
    print(f"[refget_store_bench] {text}", file=sys.stderr, flush=True)


def raw_image_bytes(lengths):
    """K12's layout: every record at a 16-byte-aligned offset, 16 .. 31 zero bytes behind it"""
    return int(sum((int(n) + 16 + 15) & ~15 for n in lengths))


def pack_case(handle, lengths, reps, threads):
    """k_refget_pack over a loaded collection -> (the pack, its figures); checked against the host path and the raw image"""
    n = len(handle)
    classes = G.digest_records(handle)[2]
    pack = G._Pack.from_handle(handle, classes)  # (warm-up: builds the raw image too)
    host = G._Pack.from_handle(handle, classes, on_host=True, threads=threads)
    assert pack.image_bytes == host.image_bytes
    for i in range(0, n, max(1, n // 2000)):
        assert pack.record(i, 16) == host.record(i, 16), i
    total = int(np.sum(lengths))
    ms = kernel_medians(lambda: G._Pack.from_handle(handle, classes), reps, "k_refget_pack")["k_refget_pack"]
    rows = np.arange(n, dtype=np.uint32)
    _, off, blob = handle.substrings(rows, np.zeros(n, np.uint64), np.asarray(lengths, np.uint64), False)
    d_off, d_blob = pack.decode_records()
    assert (d_off == off).all() and d_blob == blob
    return pack, {"text_bytes": total, "records": n, "classes": {str(c): int((classes == c).sum()) for c in np.unique(classes)},
                  "k_refget_pack_ms": ms, "k_refget_pack_GBps_of_text": total / (ms * 1e-3) / 1e9,
                  "raw_image_bytes": raw_image_bytes(lengths), "packed_image_bytes": pack.image_bytes,
                  "host_pack_s": median_wall(lambda: G._Pack.from_handle(handle, classes, on_host=True, threads=threads), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=200_000)
    ap.add_argument("--long", type=int, default=8)
    ap.add_argument("--scale", type=float, default=0.25)
    ap.add_argument("--peaks", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available() and gtars_amd.device_count() > 0, "refget_store_bench needs an MI355X"
    out = {"device": torch.cuda.get_device_name(0), "scale": args.scale, "peaks": args.peaks, "reps": args.reps,
           "host_path_threads": args.host_threads}
    with tempfile.TemporaryDirectory() as tmp:
        # ---- the many-record FASTA ----
        lengths = make_transcripts(np.array([250_000_000] * 4, dtype=np.int64), args.records, args.long)[6]
        fa = os.path.join(tmp, "many.fa")
        write_records(fa, lengths)
        many = G._Handle.from_path(fa, G.KEEP_BYTES | G.NO_DIGESTS, args.host_threads)
        pack, out["many"] = pack_case(many, lengths, args.reps, args.host_threads)
        note(f"many records: {out['many']}")
        del many, pack

        # ---- the hg38-shaped assembly ----
        sizes = chrom_sizes(args.scale)
        seqs = make_assembly(sizes)
        asm = os.path.join(tmp, "asm.fa")
        write_assembly(asm, sizes, seqs)
        lens = np.array([len(s) for s in seqs], dtype=np.int64)
        del seqs
        a = G._Handle.from_path(asm, G.KEEP_BYTES | G.NO_DIGESTS, args.host_threads)
        pack, out["assembly"] = pack_case(a, lens, args.reps, args.host_threads)
        note(f"assembly: {out['assembly']}")

        # ---- substrings of the same peaks from both images ----
        rng = np.random.default_rng(5)
        rows = rng.choice(len(lens), args.peaks, p=lens / lens.sum()).astype(np.uint32)
        width = rng.integers(200, 801, args.peaks)
        start = (rng.random(args.peaks) * np.maximum(lens[rows] - width, 1)).astype(np.uint64)
        end = np.minimum(start + width.astype(np.uint64), lens[rows].astype(np.uint64))
        r_st, r_off, r_blob = a.substrings(rows, start, end, False)
        p_st, p_off, p_blob = pack.substrings(rows, start, end, False)
        assert not r_st.any() and (p_st == r_st).all() and (p_off == r_off).all() and p_blob == r_blob
        h_st, h_off, h_blob = pack.substrings(rows, start, end, True, args.host_threads)
        assert (h_off == r_off).all() and h_blob == r_blob
        reps = max(3, args.reps)
        raw_ms = kernel_medians(lambda: a.substrings(rows, start, end, False), reps, "k_refget")
        packed_ms = kernel_medians(lambda: pack.substrings(rows, start, end, False), reps, "k_refget")
        out["substrings"] = {"bytes": len(r_blob), "raw_kernel_ms": raw_ms, "packed_kernel_ms": packed_ms,
                             "k_refget_fill_GBps_written": len(r_blob) / (raw_ms["k_refget_fill"] * 1e-3) / 1e9,
                             "k_refget_fill_packed_GBps_written": len(r_blob) / (packed_ms["k_refget_fill_packed"] * 1e-3) / 1e9,
                             "raw_column_call_s": median_wall(lambda: a.substrings(rows, start, end, False), 3),
                             "packed_column_call_s": median_wall(lambda: pack.substrings(rows, start, end, False), 3)}
        note(f"substrings: {out['substrings']}")
        del a, pack

        # ---- a store on disk against the FASTA ----
        root = os.path.join(tmp, "store")
        t0 = time.perf_counter()
        store = G.RefgetStore.on_disk(root)
        meta, _ = store.add_sequence_collection_from_fasta(asm)
        out["store_build_s"] = time.perf_counter() - t0
        out["store_seq_file_bytes"] = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(os.path.join(root, "sequences")) for f in fs)
        del store
        names = [n for n, _ in sizes]
        k = min(args.peaks, 100_000)
        chroms = [names[r] for r in rows[:k]]
        s_k, e_k = start[:k].tolist(), end[:k].tolist()
        t0 = time.perf_counter()
        opened = G.RefgetStore.open_local(root)
        got = G.substrings_many(opened, meta.digest, chroms, s_k, e_k)
        out["open_local_plus_first_region_call_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        memory = G.RefgetStore.in_memory()
        memory.add_sequence_collection(G.load_fasta(asm))
        want = G.substrings_many(memory, meta.digest, chroms, s_k, e_k)
        out["load_fasta_plus_first_region_call_s"] = time.perf_counter() - t0
        assert got == want and got[0] == r_blob[int(r_off[0]):int(r_off[1])].decode()
        out["first_region_call_rows"] = k
    print(json.dumps(out))
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
