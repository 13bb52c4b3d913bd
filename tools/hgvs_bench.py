"""HGVS expressions to VRS identifiers (csrc/hgvs.hip on top of csrc/reftx.hip and csrc/vrs.hip, K20) on the device: per
kernel, per entry and for the Python call, against the library's own host path on 16 threads and the plain-Python
restatement, on the synthetic hg38-shaped assembly and store of tools/reftx_bench.py.

  python tools/hgvs_bench.py [--scale 1.0] [--transcripts 200000] [--strings 10000000] [--reps 5] [--json profiles/hgvs_bench.json]
                             [--tx-json profiles/hgvs_tx_bench.json]

The expressions: 60 % c., 15 % n., 25 % g.; 60 % SNVs with the assembly's base as REF, the rest deletions, duplications,
insertions and delins of 1 to 3 bases (none that starts on an N: the assembly's gaps), half of the g. indels inside CAG repeats
planted every 100 kb; both strands; a tenth of
the transcript rows with an intronic offset behind the first exon; one in a thousand with an unknown accession, one in a
thousand through a gene symbol.
Per-kernel times come from the library's profiling scopes (HIP events around every launch), median of --reps calls after a
warm-up.  The Python call is split into host parse + accession lookup (gtars_hgvs_resolve), the upload of the resolved
columns, and the device entry on resident columns.  Baselines, in the same run: the library's host path (on_host) on 16
threads over everything, and tests/hgvs_ref.py on the first --sample rows.  Checks, in the run: every status, detail,
interval and identifier of the device equals the host path's, and the restatement's on the sample.

The transcript-anchored bridge (csrc/hgvs_tx.hip, K23) runs in the same run on the exonic c. / n. rows of the same
expressions: per kernel, the device entry on resident columns, the library's host path on 16 threads, the genome-anchored
device entry on the same rows (the ratio never mixes runs) and the share of the entry taken by the mRNA image's fill and
digests; every output of the device is checked against the host path.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
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
import hgvs_ref  # noqa: E402
import reftx_ref  # noqa: E402
from gtars_amd import _lib  # noqa: E402
from gtars_amd import hgvs as H  # noqa: E402
from gtars_amd import reftx as T  # noqa: E402
from gtars_amd.seqstats import BinaryGenomeAssembly  # noqa: E402
from reftx_bench import build_store, kernel_medians, make_transcripts, median_wall  # noqa: E402
from seqstats_bench import chrom_sizes, make_assembly, write_fab  # noqa: E402

REPEAT_EVERY, REPEAT_AT, REPEAT = 100_000, 1_000, np.frombuffer(b"CAG" * 30, np.uint8)
COMPLEMENT = np.arange(256, dtype=np.uint8)
for a, b in zip(b"ACGTacgt", b"TGCAtgca"):
    COMPLEMENT[a] = b


def plant_repeats(seqs):
    for s in seqs:
        for at in range(REPEAT_AT, len(s) - len(REPEAT) - 1, REPEAT_EVERY):
            s[at:at + len(REPEAT)] = REPEAT


def make_strings(seqs, names, chrom_names, tr, to_store, bound, n, threads, seed=20):
    """n expressions over the store and the assembly, as str"""
    chrom, strand, cds_s, cds_e, off, pairs, tx_len = tr
    rng = np.random.default_rng(seed)
    nt = len(chrom)
    t = rng.integers(0, nt, n)
    kind = rng.choice(np.array([0, 1, 2]), n, p=[0.6, 0.15, 0.25])  # c n g
    noncoding = cds_s[t] == 0xFFFFFFFF
    kind[(kind == 0) & noncoding] = 1
    # the CDS in transcript coordinates, through the library's own mapper
    coding = np.flatnonzero(cds_s != 0xFFFFFFFF)
    lo_hi = np.zeros((nt, 2), dtype=np.int64)
    for col, g in ((0, cds_s[coding].astype(np.int64)), (1, cds_e[coding].astype(np.int64) - 1)):
        v, st = bound.map(to_store[coding], np.full(len(coding), 2, np.uint8), g, on_host=True, threads=threads)
        assert (st == 0).all()
        lo_hi[coding, col] = v.astype(np.int64)
    cds_lo, cds_hi = lo_hi.min(axis=1), lo_hi.max(axis=1) + 1
    # a transcript position, or the last base of the first exon (transcript order) with an offset into the intron
    first_exon = np.where(strand > 0, off[:-1], off[1:] - 1)
    first_len = (pairs[2 * first_exon + 1] - pairs[2 * first_exon]).astype(np.int64)
    many = (off[1:] - off[:-1]) > 1
    p = (rng.random(n) * np.maximum(tx_len[t] - 3, 1)).astype(np.int64)
    intronic = (rng.random(n) < 0.1) & many[t] & (kind != 2)
    p = np.where(intronic, first_len[t] - 1, p)
    offset = np.where(intronic, rng.integers(1, 21, n), 0).astype(np.int64)
    width = np.where(intronic, 1, rng.integers(1, 4, n))  # bases of a range
    edit = rng.choice(np.array([0, 1, 2, 3, 4]), n, p=[0.6, 0.12, 0.12, 0.08, 0.08])  # sub del dup ins delins
    # g. rows: anywhere, or inside a planted repeat for half of the indels
    lens = np.array([len(s) for s in seqs], dtype=np.int64)
    gc = rng.choice(len(seqs), n, p=lens / lens.sum())
    gp = (rng.random(n) * (lens[gc] - 8)).astype(np.int64)
    planted = (edit != 0) & (rng.random(n) < 0.5) & (lens[gc] > REPEAT_EVERY + REPEAT_AT)
    slot = (rng.random(n) * np.maximum((lens[gc] - len(REPEAT) - 1 - REPEAT_AT) // REPEAT_EVERY, 1)).astype(np.int64)
    gp = np.where(planted, REPEAT_AT + slot * REPEAT_EVERY + rng.integers(3, 60, n), gp)
    # the genomic position of every transcript row's first base, for the REF of an SNV
    rows = np.flatnonzero(kind != 2)
    g_pos, g_st = bound.map(to_store[t[rows]], np.ones(len(rows), np.uint8), p[rows] + 1, offset[rows], on_host=True, threads=threads)
    ref = np.full(n, ord("A"), dtype=np.uint8)
    for c in range(len(seqs)):
        sel = np.flatnonzero((kind == 2) & (gc == c))
        ref[sel] = seqs[c][gp[sel]]
        tsel = rows[(chrom[t[rows]] == c) & (g_st == 0)]
        where = g_pos[(chrom[t[rows]] == c) & (g_st == 0)].astype(np.int64)
        ok = where < lens[c]
        base = seqs[c][where[ok]]
        ref[tsel[ok]] = np.where(strand[t[tsel[ok]]] > 0, base, COMPLEMENT[base])
    ref &= 0xDF  # upper case
    edit = np.where(ref == ord("N"), 0, edit)  # no indels inside the assembly's 50-kb N runs: each would roll through the whole run
    alt = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n, 3))]
    code = np.zeros(256, dtype=np.int64)
    code[list(b"ACGT")] = [0, 1, 2, 3]
    alt[:, 0] = np.frombuffer(b"ACGT", np.uint8)[(code[ref] + rng.integers(1, 4, n)) % 4]  # an SNV's ALT differs from its REF
    unknown, by_gene = rng.random(n) < 0.001, rng.random(n) < 0.001
    out = []
    for i in range(n):
        k = kind[i]
        if k == 2:
            head = f"{chrom_names[gc[i]]}:g."
            a, b = str(gp[i] + 1), str(gp[i] + width[i])
        else:
            ti = t[i]
            acc = "NM_NOPE.1" if unknown[i] else (f"GENE{ti // 3}" if by_gene[i] and ti % 3 == 0 else names[ti])
            q = int(p[i])
            if k == 1:
                a, b = str(q + 1), str(q + width[i])
            else:
                def c_pos(x, lo=int(cds_lo[ti]), hi=int(cds_hi[ti])):
                    return str(x - lo) if x < lo else ("*" + str(x - hi + 1) if x >= hi else str(x - lo + 1))
                a, b = c_pos(q), c_pos(q + int(width[i]) - 1)
            if offset[i]:
                a += "+%d" % offset[i]
            head = f"{acc}:{'cn'[k]}."
        e = edit[i]
        letters = alt[i].tobytes().decode()
        if e == 0:
            out.append(f"{head}{a}{chr(ref[i])}>{letters[0]}")
        elif e == 3:
            out.append(f"{head}{a}_{b}ins{letters}" if width[i] == 2 and not offset[i] else f"{head}{a}ins{letters[:2]}")
        else:
            loc = a if width[i] == 1 else f"{a}_{b}"
            out.append(head + loc + ("del" if e == 1 else "dup" if e == 2 else "delins" + letters))
    return out


def say(text):
    print(f"[hgvs_bench] {text}", file=sys.stderr, flush=True)


def transcript_section(g, bound, strings, cols, text, off, threads, reps, dev):
    """K23 (csrc/hgvs_tx.hip) on the exonic c. / n. rows of the run's own expressions: the library's host path on `threads`
    threads, the device entry on resident columns with its per-kernel times, and -- on the same rows, in the same run -- the
    genome-anchored device entry it is compared with.  Every status, detail, interval, identifier and anchor of the device
    is checked against the host path."""
    keep = np.flatnonzero(((cols["kind"] == 1) | (cols["kind"] == 2)) & (cols["off1"] == 0) & (cols["off2"] == 0) & (cols["pre"] == 0))
    n = int(keep.size)
    sec = {"rows": n}
    if not n:
        return sec
    # the kept rows as a batch of their own: text and offsets, then the resolved columns
    lens = (off[1:] - off[:-1])[keep].astype(np.int64)
    sub_off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens).astype(np.uint64)])
    idx = np.repeat(off[:-1][keep].astype(np.int64) - sub_off[:-1].astype(np.int64), lens) + np.arange(int(sub_off[-1]), dtype=np.int64)
    sub_text = text[idx].copy()
    sub = {name: np.zeros(n, dtype=dt) for name, dt in H.COLUMN_DTYPES}
    c = H._CColumns(**{name: sub[name].ctypes.data for name, _ in H.COLUMN_DTYPES})
    _lib.check(_lib.lib.gtars_hgvs_resolve(bound._h, _lib.ptr(sub_text), _lib.ptr(sub_off), n, None, None, None, 0, threads, C.byref(c)))
    sub["text"] = sub_text

    def outputs():
        return (np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint64),
                np.zeros(n, np.uint64), np.zeros(32 * n, np.uint8), np.zeros(32 * n, np.uint8))

    def to_tx(on_host, res):
        _lib.check(_lib.lib.gtars_hgvs_to_transcript_vrs(bound._h, _lib.ptr(sub_text), _lib.ptr(sub_off), n, 1 if on_host else 0, threads,
                                                         *(_lib.ptr(a) for a in res)))

    host = outputs()
    t0 = time.perf_counter()
    to_tx(True, host)
    sec["host_path_s"], sec["host_path_threads"] = time.perf_counter() - t0, threads
    sec["status_counts"] = np.bincount(host[0], minlength=12).tolist()
    got = outputs()
    to_tx(False, got)
    for a, b in zip(got, host):
        assert (a == b).all()
    sec["library_call_s"] = median_wall(lambda: to_tx(False, got), max(2, reps // 2))
    signed = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64, np.dtype(np.int64): np.int64}
    resident = {name: torch.from_numpy(a.view(signed[a.dtype])).to(dev) for name, a in sub.items()}
    ptrs = {k: v.data_ptr() for k, v in resident.items()}
    o_st, o_de, o_wa = (torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(3))
    o_tx = torch.zeros(n, dtype=torch.int32, device=dev)
    o_ns, o_ne = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    o_dig, o_anc = torch.zeros(32 * n, dtype=torch.uint8, device=dev), torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def tx_entry():
        H.transcript_ids_device(g, bound, ptrs, sub_text.size, n, o_st.data_ptr(), o_de.data_ptr(), o_wa.data_ptr(), o_tx.data_ptr(),
                                o_ns.data_ptr(), o_ne.data_ptr(), o_dig.data_ptr(), o_anc.data_ptr(), stream)

    def genome_entry():
        H.ids_device(g, bound, ptrs, sub_text.size, n, o_st.data_ptr(), o_de.data_ptr(), o_wa.data_ptr(), o_tx.data_ptr(), o_ns.data_ptr(),
                     o_ne.data_ptr(), o_dig.data_ptr(), stream)

    tx_entry()
    for t, h in zip((o_st, o_de, o_wa, o_tx, o_ns, o_ne, o_dig, o_anc), host):
        assert (t.cpu().numpy().view(h.dtype) == h).all()
    sec["device_entry_s"] = median_wall(tx_entry, reps)
    kernels = {}
    for prefix in ("k_hgvs_tx", "k_tx_", "k_vrs"):
        kernels.update(kernel_medians(tx_entry, reps, prefix))
    sec["kernel_ms_median"] = kernels
    genome_entry()
    sec["genome_entry_same_rows_s"] = median_wall(genome_entry, reps)
    sec["ratio_to_genome_entry"] = sec["device_entry_s"] / sec["genome_entry_same_rows_s"]
    sec["image_fill_and_digest_share"] = (kernels.get("k_hgvs_tx_image", 0.0) + kernels.get("k_tx_digest", 0.0)) / (1e3 * sec["device_entry_s"])
    sec["host_over_device_entry"] = sec["host_path_s"] / sec["device_entry_s"]
    return sec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--transcripts", type=int, default=200_000)
    ap.add_argument("--strings", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=2000)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--json", default=None)
    ap.add_argument("--tx-json", default=None, help="the transcript-anchored section on its own (profiles/hgvs_tx_bench.json)")
    args = ap.parse_args()
    assert torch.cuda.is_available() and gtars_amd.device_count() > 0, "hgvs_bench needs an MI355X"
    dev = torch.device("cuda", torch.cuda.current_device())
    nt, n, threads = args.transcripts, args.strings, args.host_threads
    sizes = chrom_sizes(args.scale)
    seqs = make_assembly(sizes)
    plant_repeats(seqs)
    say("assembly made")
    out = {"device": torch.cuda.get_device_name(0), "scale": args.scale, "transcripts": nt, "strings": n, "reps": args.reps,
           "assembly_bytes": int(sum(len(s) for s in seqs)), "host_path_threads": threads}
    with tempfile.TemporaryDirectory() as tmp:
        fab = os.path.join(tmp, "asm.fab")
        write_fab(fab, sizes, seqs)
        g = BinaryGenomeAssembly(fab)
        tr = make_transcripts(np.array([len(s) for s in seqs], dtype=np.int64), nt, 0)
        names = build_store(os.path.join(tmp, "tx.reftx"), g, tr)
        store = T.ReadonlyTxStore.open(os.path.join(tmp, "tx.reftx"))
        to_store = store.indices_of(names)
        bound = T.BoundTxStore(g, store)
        say("store bound")
        t0 = time.perf_counter()
        strings = make_strings(seqs, names, g.chrom_names, tr, to_store, bound, n, threads)
        out["make_strings_s"] = time.perf_counter() - t0
        text, off, _ = H._blob(strings)
        text = text.copy()  # (writable: torch wraps it for the upload)
        out["text_bytes"] = int(text.size)
        say("strings made")

        def outputs():
            return (np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint64),
                    np.zeros(n, np.uint64), np.zeros(32 * n, np.uint8))

        def to_vrs(on_host, res):
            _lib.check(_lib.lib.gtars_hgvs_to_vrs(bound._h, _lib.ptr(text), _lib.ptr(off), n, None, None, None, 0, None, 1 if on_host else 0, threads,
                                                  *(_lib.ptr(a) for a in res)))

        host = outputs()
        t0 = time.perf_counter()
        to_vrs(True, host)
        out["host_path_s"] = time.perf_counter() - t0
        out["status_counts"] = np.bincount(host[0], minlength=12).tolist()
        say("host path done")
        dev_res = outputs()
        t0 = time.perf_counter()
        to_vrs(False, dev_res)
        out["first_library_call_s"] = time.perf_counter() - t0
        for a, b in zip(dev_res, host):  # every row: status, detail, warnings, chromosome, interval, identifier
            assert (a == b).all()
        out["library_call_s"] = median_wall(lambda: to_vrs(False, dev_res), max(2, args.reps // 2))
        t0 = time.perf_counter()
        r = H.hgvs_to_vrs_ids(g, bound, strings)
        out["python_call_s"] = time.perf_counter() - t0
        assert (r["statuses"] == host[0]).all()
        say("library and Python calls done")

        # the split of the call: parse + lookup on the host threads, the upload, the device entry on resident columns
        cols = {name: np.zeros(n, dtype=dt) for name, dt in H.COLUMN_DTYPES}
        c = H._CColumns(**{name: cols[name].ctypes.data for name, _ in H.COLUMN_DTYPES})

        def resolve():
            _lib.check(_lib.lib.gtars_hgvs_resolve(bound._h, _lib.ptr(text), _lib.ptr(off), n, None, None, None, 0, threads, C.byref(c)))

        out["parse_and_lookup_s"] = median_wall(resolve, max(2, args.reps // 2))
        cols["text"] = text
        signed = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64, np.dtype(np.int64): np.int64}
        resident = {}

        def upload():
            for name, a in cols.items():
                resident[name] = torch.from_numpy(a.view(signed[a.dtype])).to(dev)

        out["upload_s"] = median_wall(upload, max(2, args.reps // 2))
        o_st, o_de, o_wa = (torch.zeros(n, dtype=torch.uint8, device=dev) for _ in range(3))
        o_ch = torch.zeros(n, dtype=torch.int32, device=dev)
        o_ns, o_ne = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
        o_dig = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
        ptrs = {k: v.data_ptr() for k, v in resident.items()}

        def entry():
            H.ids_device(g, bound, ptrs, text.size, n, o_st.data_ptr(), o_de.data_ptr(), o_wa.data_ptr(), o_ch.data_ptr(), o_ns.data_ptr(),
                         o_ne.data_ptr(), o_dig.data_ptr(), torch.cuda.current_stream().cuda_stream)

        entry()
        assert (o_st.cpu().numpy() == host[0]).all() and (o_dig.cpu().numpy() == host[6]).all()
        assert (o_ns.cpu().numpy().view(np.uint64) == host[4]).all() and (o_ne.cpu().numpy().view(np.uint64) == host[5]).all()
        out["device_entry_s"] = median_wall(entry, args.reps)
        out["kernel_ms_median"] = {**kernel_medians(entry, args.reps, "k_hgvs"), **kernel_medians(entry, args.reps, "k_vrs")}

        say("device entry done")
        out["transcript_anchored"] = transcript_section(g, bound, strings, cols, text, off, threads, args.reps, dev)
        say("transcript-anchored section done")
        # the restatement on a sample
        k = min(args.sample, n)
        if nt <= 250_000:
            txs, _ = reftx_ref.decode(open(os.path.join(tmp, "tx.reftx"), "rb").read())
            by_name = {nm: s.tobytes() for nm, s in zip(g.chrom_names, seqs)}
            hgvs_ref._OWN[id(by_name)] = (by_name, g.refget_digests())  # (the library's digests: hashing 3 GB in Python is not the point)
            t0 = time.perf_counter()
            want = hgvs_ref.bridge(by_name, g.refget_digests(), txs, strings[:k])
            out["python_restatement_strings_per_s"] = k / (time.perf_counter() - t0)
            raw = host[6].tobytes()
            for i, w in enumerate(want):
                assert (w["status"], w["detail"], w["start"], w["end"]) == (host[0][i], host[1][i], host[4][i], host[5][i]), strings[i]
                assert w["id"] == ("ga4gh:VA." + raw[32 * i:32 * i + 32].decode() if host[0][i] == 0 else None), strings[i]
            out["python_restatement_checked"] = k
    line = json.dumps(out)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    if args.tx_json:
        head = {k: out[k] for k in ("device", "scale", "transcripts", "strings", "reps", "assembly_bytes")}
        with open(args.tx_json, "w") as f:
            f.write(json.dumps({**head, "genome_device_entry_all_rows_s": out["device_entry_s"], **out["transcript_anchored"]}, indent=1) + "\n")


if __name__ == "__main__":
    main()
