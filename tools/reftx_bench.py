"""Transcripts (csrc/reftx.hip, K19) on the device: coordinate mapping, the digests of every transcript's mature mRNA and
the sequences themselves, per kernel and per entry, against the library's own host path on 16 threads and the
plain-Python restatement, on the synthetic hg38-shaped assembly of tools/seqstats_bench.py.

  python tools/reftx_bench.py [--scale 1.0] [--transcripts 200000] [--queries 10000000] [--reps 10] [--json profiles/reftx_bench.json]

The transcripts: RefSeq-like exon counts (1 to 80, mean about 10), exon lengths around 150 bases with a longer last exon,
introns of a few kilobases, 85 % coding, both strands, and --long transcripts of 100 to 150 kb (they are what
GTARS_TX_HOST_LEN hands to the host threads).  The queries: 70 % c. (some in the UTRs, some c.*N, a tenth with an intronic
offset), 20 % n., 10 % genomic positions inside the transcript's span.
Per-kernel times come from the library's profiling scopes (HIP events around every launch), median of --reps calls after
a warm-up; the entries by wall time, median of --reps.  Baselines, in the same run: the library's host path (on_host) on
16 threads over everything, and tests/reftx_ref.py on the first --sample rows.  Checks, in the run: the device's values,
statuses, digests and sequences equal the host path's for every row, the restatement's on the sample.
"""
from __future__ import annotations

import argparse
import ctypes as C
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
import reftx_ref  # noqa: E402
from gtars_amd import _lib  # noqa: E402
from gtars_amd import reftx as T  # noqa: E402
from gtars_amd.seqstats import BinaryGenomeAssembly  # noqa: E402
from seqstats_bench import chrom_sizes, make_assembly, write_fab  # noqa: E402


def make_transcripts(lens, n, n_long, seed=19):
    """-> per transcript: chromosome, strand, cds (0xFFFFFFFF: none), exon offsets; flat (start, end) pairs"""
    rng = np.random.default_rng(seed)
    n_exons = np.clip(rng.geometric(0.1, n), 1, 80).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(n_exons)])
    total = int(off[-1])
    ex_len = np.clip(rng.lognormal(5.0, 0.6, total), 20, 5000).astype(np.int64)
    ex_len[off[1:] - 1] += rng.integers(300, 3000, n)          # the last exon carries the 3' UTR
    for t in range(min(n_long, n)):                            # a few transcripts above 100 kb
        ex_len[off[t]:off[t + 1]] = rng.integers(100_000, 150_000) // n_exons[t] + 1
    intron = np.clip(rng.lognormal(7.3, 1.0, total), 50, 60_000).astype(np.int64)
    intron[off[:-1]] = 0
    rel_end = np.cumsum(ex_len + intron)
    base = np.repeat(rel_end[off[:-1]] - ex_len[off[:-1]], n_exons)  # (the first exon's own start in the running sum)
    rel_end -= base
    rel_start = rel_end - ex_len
    span = rel_end[off[1:] - 1]
    chrom = rng.choice(len(lens), n, p=lens / lens.sum())
    room = lens[chrom] - span - 64
    small = room < 1
    chrom[small] = int(np.argmax(lens))                        # the longest chromosome holds every transcript
    room = lens[chrom] - span - 64
    assert (room >= 1).all()
    origin = (rng.random(n) * room).astype(np.int64) + 32
    starts = (rel_start + np.repeat(origin, n_exons)).astype(np.uint32)
    ends = (rel_end + np.repeat(origin, n_exons)).astype(np.uint32)
    strand = np.where(rng.random(n) < 0.5, 1, -1).astype(np.int32)
    coding = rng.random(n) < 0.85
    cds_s = np.where(coding, starts[off[:-1]] + (ex_len[off[:-1]] // 3), 0xFFFFFFFF).astype(np.uint32)
    cds_e = np.where(coding, ends[off[1:] - 1] - (ex_len[off[1:] - 1] // 3), 0xFFFFFFFF).astype(np.uint32)
    pairs = np.empty(2 * total, dtype=np.uint32)
    pairs[0::2], pairs[1::2] = starts, ends
    tx_len = np.add.reduceat(ex_len, off[:-1])
    return chrom, strand, cds_s, cds_e, off, pairs, tx_len


def build_store(path, g, tr):
    chrom, strand, cds_s, cds_e, off, pairs, _ = tr
    digests = g.refget_digests()
    acc_of = [("SQ." + digests[name]).encode() for name in g.chrom_names]
    b = T.TxStoreBuilder()
    add, h, base = _lib.lib.gtars_txbuilder_add, b._h, pairs.ctypes.data
    names = [b"NM_%07d.%d" % (t, 1 + t % 9) for t in range(len(chrom))]
    for t in range(len(chrom)):
        _lib.check(add(h, names[t], b"GENE%d" % (t // 3), acc_of[chrom[t]], int(strand[t]), int(cds_s[t]), int(cds_e[t]), 1 if t % 3 == 0 else 0,
                       C.c_void_p(base + 8 * int(off[t])), int(off[t + 1] - off[t])))
    b.build(path)
    return [nm.decode() for nm in names]


def make_queries(tr, to_store, n, seed=7):
    chrom, strand, cds_s, cds_e, off, pairs, tx_len = tr
    rng = np.random.default_rng(seed)
    t = rng.integers(0, len(chrom), n)
    kind = rng.choice(np.array([0, 1, 2], dtype=np.uint8), n, p=[0.7, 0.2, 0.1])
    length = tx_len[t]
    pos = (rng.random(n) * (length + 100)).astype(np.int64) - 50          # c.: UTRs, the CDS and a little beyond
    npos = (rng.random(n) * (length + 2)).astype(np.int64)
    lo, hi = pairs[2 * off[t]].astype(np.int64), pairs[2 * off[t + 1] - 1].astype(np.int64)
    gpos = lo + (rng.random(n) * (hi - lo)).astype(np.int64)
    pos = np.where(kind == 1, npos, np.where(kind == 2, gpos, pos))
    offset = np.where((rng.random(n) < 0.1) & (kind != 2), rng.integers(-20, 21, n), 0).astype(np.int64)
    star = ((rng.random(n) < 0.1) & (kind == 0)).astype(np.uint8)
    tx = to_store[t].astype(np.uint32)
    tx[rng.random(n) < 0.001] = 0xFFFFFFFF                                 # unknown accessions
    return tx, kind, pos, offset, star, t


def median_wall(fn, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def kernel_medians(fn, reps, prefix="k_tx"):
    _lib.lib.gtars_prof_enable(1)
    per = {}
    for _ in range(reps):
        _lib.lib.gtars_prof_reset()
        fn()
        for name, v in _lib.prof_read().items():
            if name.startswith(prefix):
                per.setdefault(name, []).append(v["total_ms"])
    _lib.lib.gtars_prof_enable(0)
    return {name: statistics.median(v) for name, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--transcripts", type=int, default=200_000)
    ap.add_argument("--long", type=int, default=8)
    ap.add_argument("--queries", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--sequences", type=int, default=200_000, help="transcripts whose sequences are filled (a byte CSR of about 3.5 kB each)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available() and gtars_amd.device_count() > 0, "reftx_bench needs an MI355X"
    dev = torch.device("cuda", torch.cuda.current_device())
    nt, nq = args.transcripts, args.queries
    sizes = chrom_sizes(args.scale)
    seqs = make_assembly(sizes)
    out = {"device": torch.cuda.get_device_name(0), "scale": args.scale, "transcripts": nt, "queries": nq, "reps": args.reps,
           "assembly_bytes": int(sum(len(s) for s in seqs)), "host_path_threads": args.host_threads}
    with tempfile.TemporaryDirectory() as tmp:
        fab = os.path.join(tmp, "asm.fab")
        write_fab(fab, sizes, seqs)
        g = BinaryGenomeAssembly(fab)
        tr = make_transcripts(np.array([len(s) for s in seqs], dtype=np.int64), nt, args.long)
        t0 = time.perf_counter()
        names = build_store(os.path.join(tmp, "tx.reftx"), g, tr)
        out["build_store_s"] = time.perf_counter() - t0
        out["store_bytes"] = os.path.getsize(os.path.join(tmp, "tx.reftx"))
        t0 = time.perf_counter()
        store = T.ReadonlyTxStore.open(os.path.join(tmp, "tx.reftx"))
        out["open_store_s"] = time.perf_counter() - t0
        out["exons"], out["mature_bytes"], out["longest_transcript"] = int(tr[4][-1]), int(tr[6].sum()), int(tr[6].max())
        to_store = store.indices_of(names)
        t0 = time.perf_counter()
        bound = T.BoundTxStore(g, store)
        out["bind_s"] = time.perf_counter() - t0

        # ---- mapping ----
        tx, kind, pos, offset, star, t_of = make_queries(tr, to_store, nq)
        t0 = time.perf_counter()
        h_val, h_st = bound.map(tx, kind, pos, offset, star, on_host=True, threads=args.host_threads)
        out["map_host_path_s"] = time.perf_counter() - t0
        out["map_status_counts"] = np.bincount(h_st, minlength=11).tolist()
        t0 = time.perf_counter()
        d_val, d_st = bound.map(tx, kind, pos, offset, star)
        out["map_first_column_call_s"] = time.perf_counter() - t0
        assert (d_val == h_val).all() and (d_st == h_st).all()
        out["map_column_call_s"] = median_wall(lambda: bound.map(tx, kind, pos, offset, star), max(3, args.reps // 3))
        k = min(args.sample, nq)
        txs, _ = reftx_ref.decode(open(os.path.join(tmp, "tx.reftx"), "rb").read()) if nt <= 250_000 else (None, None)
        if txs is not None:
            rows = [(txs[tx[i]]["accession"] if tx[i] != 0xFFFFFFFF else "NM_NOPE.1", "cng"[kind[i]], int(pos[i]), int(offset[i]), bool(star[i]))
                    for i in range(k)]
            t0 = time.perf_counter()
            want = reftx_ref.map_rows(txs, rows)
            out["map_python_restatement_queries_per_s"] = k / (time.perf_counter() - t0)
            assert want == (d_val[:k].tolist(), d_st[:k].tolist())
        cols = [torch.from_numpy(a.view(dt)).to(dev) for a, dt in ((tx, np.int32), (kind, np.uint8), (pos, np.int64), (offset, np.int64),
                                                                    (star, np.uint8))]
        o_val, o_st = torch.zeros(nq, dtype=torch.int64, device=dev), torch.zeros(nq, dtype=torch.uint8, device=dev)

        def map_entry():
            bound.map_device(*(c.data_ptr() for c in cols), nq, o_val.data_ptr(), o_st.data_ptr(), torch.cuda.current_stream().cuda_stream)

        map_entry()
        assert (o_val.cpu().numpy().view(np.uint64) == h_val).all() and (o_st.cpu().numpy() == h_st).all()
        out["map_device_entry_s"] = median_wall(map_entry, args.reps)
        out["map_kernel_ms_median"] = kernel_medians(map_entry, args.reps)
        m = min(nq, 1_000_000)
        accs = [names[i] for i in t_of[:m]]
        mapper = T.CoordinateMapper(store, g)
        t0 = time.perf_counter()
        mapper.n_to_g_many(accs, pos[:m])
        out["map_python_call_1e6_s"] = (time.perf_counter() - t0) * (1_000_000 / m)

        # ---- digests ----
        idx = np.arange(nt, dtype=np.uint32)
        t0 = time.perf_counter()
        hs_st, hs_dig, _ = bound.sequences(idx, want_sequences=False, on_host=True, threads=args.host_threads)
        out["digest_host_path_s"] = time.perf_counter() - t0
        d_idx = torch.from_numpy(idx.view(np.int32)).to(dev)
        o_sst, o_dig = torch.zeros(nt, dtype=torch.uint8, device=dev), torch.zeros(32 * nt, dtype=torch.uint8, device=dev)

        def digest_entry():
            bound.digests_device(d_idx.data_ptr(), nt, o_sst.data_ptr(), o_dig.data_ptr(), torch.cuda.current_stream().cuda_stream)

        digest_entry()
        raw = o_dig.cpu().numpy().tobytes()
        assert (o_sst.cpu().numpy() == hs_st).all() and (hs_st == 0).all()
        assert [raw[32 * i:32 * i + 32].decode() for i in range(nt)] == hs_dig
        out["digest_device_entry_s"] = median_wall(digest_entry, args.reps)
        out["digest_kernel_ms_median"] = kernel_medians(digest_entry, args.reps)
        # the host tail's threshold: the same call with more and fewer transcripts left to the host threads
        by_host_len = {}
        for thr in (4096, 16384, 32768, 65536, 1 << 20):
            os.environ["GTARS_TX_HOST_LEN"] = str(thr)
            _lib.reload_env()
            o_dig.zero_()
            digest_entry()
            assert o_dig.cpu().numpy().tobytes() == raw
            by_host_len[str(thr)] = {"device_entry_s": median_wall(digest_entry, max(3, args.reps // 2)), "transcripts_on_host": int((tr[6] > thr).sum()),
                                     "k_tx_digest_ms": kernel_medians(digest_entry, 3).get("k_tx_digest")}
        del os.environ["GTARS_TX_HOST_LEN"]
        _lib.reload_env()
        out["digest_by_host_len"] = by_host_len
        t0 = time.perf_counter()
        ids = T.transcript_accessions(g, bound)
        out["transcript_accessions_python_s"] = time.perf_counter() - t0
        assert len(ids) == nt

        # ---- sequences ----
        ns = min(args.sequences, nt)
        t0 = time.perf_counter()
        _, _, h_seqs = bound.sequences(idx[:ns], want_digests=False, on_host=True, threads=args.host_threads)
        out["sequences_host_path_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        _, _, d_seqs = bound.sequences(idx[:ns], want_digests=False)
        out["sequences_column_call_s"] = time.perf_counter() - t0
        assert d_seqs == h_seqs
        out["sequences_transcripts"], out["sequences_bytes"] = ns, sum(len(s) for s in d_seqs)
        out["sequences_kernel_ms_median"] = kernel_medians(lambda: bound.sequences(idx[:ns], want_digests=False), max(3, args.reps // 3))
        if txs is not None:
            by_name = {nm: s.tobytes() for nm, s in zip(g.chrom_names, seqs)}
            digests = g.refget_digests()
            by_digest = {reftx_ref.digest_bytes(digests[nm]): by_name[nm] for nm in g.chrom_names}
            t0 = time.perf_counter()
            for i in range(min(args.sample, ns) // 10):  # (the restatement's own chromosome lookup hashes the assembly: cut here)
                txr = txs[i]
                chrom_seq = by_digest[txr["digest"]]
                seq = b"".join(chrom_seq[s:e] for s, e in txr["exons"]).upper()
                seq = reftx_ref.reverse_complement(seq) if txr["strand"] < 0 else seq
                assert seq == d_seqs[i] and reftx_ref.sha512t24u(seq) == hs_dig[i]
            out["sequences_python_restatement_checked"] = min(args.sample, ns) // 10
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
