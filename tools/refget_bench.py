"""Refget (csrc/refget.hip, K21) on the device: the digests of a many-record FASTA and of an hg38-shaped assembly, and
substrings of 1e6 peaks, per kernel and per entry, against the library's own host path on 16 threads.

  python tools/refget_bench.py [--records 200000] [--scale 1.0] [--peaks 1000000] [--reps 10] [--json profiles/refget_bench.json]

The many-record FASTA: --records records with the RefSeq-like mature-mRNA lengths of tools/reftx_bench.py (a few of 100 to
150 kb among them), random bases with some soft-masked, one line per record.  The assembly: the synthetic hg38-shaped one of
tools/seqstats_bench.py at --scale.  Per-kernel times come from the library's profiling scopes (HIP events around every
launch), median of --reps calls after a warm-up; the entries by wall time, median of --reps.  The run repeats at
GTARS_REFGET_HOST_LEN 16384, 65536 and 2^20.  Checks, in the run: every digest, MD5, class and collection digest of the
device path equals the host path's, every substring and status too.
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

import torch  # noqa: E402

import gtars_amd  # noqa: E402
from gtars_amd import _lib  # noqa: E402
from gtars_amd import refget as G  # noqa: E402
from reftx_bench import kernel_medians, make_transcripts, median_wall  # noqa: E402
from seqstats_bench import chrom_sizes, make_assembly  # noqa: E402


def write_records(path, lengths, seed=21):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGTACGTACGTACGTacgtN", np.uint8)
    with open(path, "wb") as f:
        for k, n in enumerate(lengths):
            f.write(b">NM_%07d.1 record %d\n" % (k, k))
            f.write(letters[rng.integers(0, len(letters), int(n))].tobytes())
            f.write(b"\n")


def write_assembly(path, sizes, seqs):
    with open(path, "wb") as f:
        for (name, _), s in zip(sizes, seqs):
            f.write(b">" + name.encode() + b"\n")
            f.write(s.tobytes())
            f.write(b"\n")


def note(text):
    print(f"[refget_bench] {text}", file=sys.stderr, flush=True)


def set_host_len(value):
    if value is None:
        os.environ.pop("GTARS_REFGET_HOST_LEN", None)
    else:
        os.environ["GTARS_REFGET_HOST_LEN"] = str(value)
    _lib.reload_env()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=200_000)
    ap.add_argument("--long", type=int, default=8)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--peaks", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available() and gtars_amd.device_count() > 0, "refget_bench needs an MI355X"
    dev = torch.device("cuda", torch.cuda.current_device())
    nt = args.records
    out = {"device": torch.cuda.get_device_name(0), "records": nt, "scale": args.scale, "peaks": args.peaks, "reps": args.reps,
           "host_path_threads": args.host_threads, "default_host_len": int(_lib.lib.gtars_refget_host_len())}
    stream = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    with tempfile.TemporaryDirectory() as tmp:
        # ---- the many-record FASTA ----
        lengths = make_transcripts(np.array([250_000_000] * 4, dtype=np.int64), nt, args.long)[6]
        fa = os.path.join(tmp, "many.fa")
        write_records(fa, lengths)
        note("the many-record FASTA is written")
        total = int(lengths.sum())
        out["many_bytes"], out["many_longest"], out["many_file_bytes"] = total, int(lengths.max()), os.path.getsize(fa)
        t0 = time.perf_counter()
        host = G._Handle.from_path(fa, G.KEEP_BYTES | G.ON_HOST, args.host_threads)
        out["many_load_fasta_host_path_s"] = time.perf_counter() - t0
        want = G.digest_records(host, on_host=True, threads=args.host_threads)
        out["many_host_path_digest_s"] = median_wall(lambda: G.digest_records(host, on_host=True, threads=args.host_threads), 3)
        out["many_host_path_GBps"] = total / out["many_host_path_digest_s"] / 1e9
        n = len(host)
        o_dig = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
        o_md5 = torch.zeros(16 * n, dtype=torch.uint8, device=dev)
        o_cls = torch.zeros(n, dtype=torch.uint8, device=dev)

        def entry():
            G.digests_device(host, o_dig.data_ptr(), o_md5.data_ptr(), o_cls.data_ptr(), stream())

        def check_entry():
            raw, m = o_dig.cpu().numpy().tobytes(), o_md5.cpu().numpy().tobytes()
            assert [raw[32 * i:32 * i + 32].decode() for i in range(n)] == want[0]
            assert [m[16 * i:16 * i + 16].hex() for i in range(n)] == want[1]
            assert (o_cls.cpu().numpy() == want[2]).all()

        t0 = time.perf_counter()
        entry()
        out["many_first_device_entry_s"] = time.perf_counter() - t0  # (builds the full image)
        check_entry()
        by_host_len = {}
        for thr in (16384, 65536, 1 << 20):
            set_host_len(thr)
            o_dig.zero_(), o_md5.zero_(), o_cls.zero_()
            entry()
            check_entry()
            row = {"records_on_host": int((lengths > thr).sum()), "bytes_on_host": int(lengths[lengths > thr].sum()),
                   "device_entry_s": median_wall(entry, args.reps), "kernel_ms": kernel_medians(entry, args.reps, "k_refget")}
            row["k_refget_digest_GBps"] = (total - row["bytes_on_host"]) / (row["kernel_ms"]["k_refget_digest"] * 1e-3) / 1e9
            row["device_entry_GBps"] = total / row["device_entry_s"] / 1e9

            def from_file():
                return G._Handle.from_path(fa, 0, args.host_threads)

            h = from_file()
            assert h.digests() == host.digests()
            assert [h.record(i, False).metadata.md5 for i in range(0, n, max(1, n // 500))] == want[1][::max(1, n // 500)]
            row["digest_fasta_library_s"] = median_wall(from_file, 3)
            by_host_len[str(thr)] = row
            note(f"host_len {thr}: {row}")
        set_host_len(None)
        out["many_by_host_len"] = by_host_len
        t0 = time.perf_counter()
        col = G.digest_fasta(fa)
        out["many_digest_fasta_python_s"] = time.perf_counter() - t0
        assert col.digest == host.digests()[0]
        del host, col

        # ---- the hg38-shaped assembly ----
        sizes = chrom_sizes(args.scale)
        seqs = make_assembly(sizes)
        asm = os.path.join(tmp, "asm.fa")
        write_assembly(asm, sizes, seqs)
        note("the assembly is written")
        out["assembly_bytes"] = int(sum(len(s) for s in seqs))
        t0 = time.perf_counter()
        a_host = G._Handle.from_path(asm, G.KEEP_BYTES | G.ON_HOST, args.host_threads)
        out["assembly_load_fasta_host_path_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        a_dev = G._Handle.from_path(asm, 0, args.host_threads)
        out["assembly_digest_fasta_library_s"] = time.perf_counter() - t0
        assert a_dev.digests() == a_host.digests()
        note("the assembly is digested")
        out["assembly_records_on_host"] = int(sum(len(s) > out["default_host_len"] for s in seqs))
        # ---- substrings ----
        rng = np.random.default_rng(5)
        lens = np.array([len(s) for s in seqs], dtype=np.int64)
        rows = rng.choice(len(lens), args.peaks, p=lens / lens.sum()).astype(np.uint32)
        width = rng.integers(200, 801, args.peaks)
        start = (rng.random(args.peaks) * np.maximum(lens[rows] - width, 1)).astype(np.uint64)
        end = np.minimum(start + width.astype(np.uint64), lens[rows].astype(np.uint64))
        t0 = time.perf_counter()
        h_st, h_off, h_blob = a_host.substrings(rows, start, end, True, args.host_threads)
        out["substrings_host_path_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        d_st, d_off, d_blob = a_host.substrings(rows, start, end, False)
        out["substrings_first_column_call_s"] = time.perf_counter() - t0  # (builds the image)
        assert (d_st == h_st).all() and (d_off == h_off).all() and d_blob == h_blob and not h_st.any()
        out["substrings_bytes"] = len(d_blob)
        out["substrings_column_call_s"] = median_wall(lambda: a_host.substrings(rows, start, end, False), max(3, args.reps // 3))
        out["substrings_kernel_ms"] = kernel_medians(lambda: a_host.substrings(rows, start, end, False), max(3, args.reps // 3), "k_refget")
        cols = [torch.from_numpy(a.view(dt)).to(dev) for a, dt in ((rows, np.int32), (start, np.int64), (end, np.int64))]
        o_st = torch.zeros(args.peaks, dtype=torch.uint8, device=dev)
        o_off = torch.zeros(args.peaks + 1, dtype=torch.int64, device=dev)
        o_bytes = torch.zeros(len(d_blob) + 8, dtype=torch.uint8, device=dev)

        def sub_entry():
            return G.substrings_device(a_host, cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), args.peaks, o_st.data_ptr(),
                                       o_off.data_ptr(), o_bytes.data_ptr(), len(d_blob), stream())

        assert sub_entry() == len(d_blob) and o_bytes.cpu().numpy().tobytes()[:len(d_blob)] == h_blob
        out["substrings_device_entry_s"] = median_wall(sub_entry, args.reps)
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
