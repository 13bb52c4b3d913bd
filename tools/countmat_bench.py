"""The sparse count matrix (csrc/countmat.hip, K16) against the dense-band dict path it stands next to.

  python tools/countmat_bench.py [--universe 100000] [--fragments 2000000] [--barcodes 10000] [--reps 10] [--dict-reps 3] [--json out.json]

One synthetic single-cell sample: --fragments position-sorted fragments of --barcodes barcodes (synth.write_config5_inputs)
against bench.py's universe of --universe regions, written in sorted order so that a peak's index is its line.

  csr build        gtars_count_matrix_csr_device on the resident hits of one tokenization: HIP events around the call and wall time,
                   median of --reps (min, max); its three kernels, the sort and the scan alone from the library's profiling mode
                   (HIP events around each launch), median of --reps profiled calls
  band step        the matrix step of barcode_scoring_from_fragments on the same resident hits: bands of BAND_CELLS cells filled by
                   gtars_histogram_rows_device, copied to the host, searched with np.nonzero, entered into the dict (wall time)
  end to end       barcode_count_matrix(file) and barcode_scoring_from_fragments(file), parse and tokenization included (wall
                   time, median of --dict-reps), and SparseCounts.to_dict() on top of the former

The two results are compared in the run (to_dict() == the dict) before anything is timed."""
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

import torch  # noqa: E402

from gtars_amd import _lib, scoring, synth  # noqa: E402


def stat(v):
    return [float(np.median(v)), float(min(v)), float(max(v))]


def wall_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return stat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--universe", type=int, default=100_000)
    ap.add_argument("--fragments", type=int, default=2_000_000)
    ap.add_argument("--barcodes", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dict-reps", type=int, default=3)
    ap.add_argument("--json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "countmat_bench needs an MI355X"
    u = synth.make_universe(a.universe)
    with tempfile.TemporaryDirectory() as tmp:
        fd = synth.write_config5_inputs(tmp, u, 1, a.fragments, 5, barcodes=a.barcodes)[1]
        frag = os.path.join(fd, sorted(os.listdir(fd))[0])
        rows = sorted(zip((synth.CHROM_NAMES[c] for c in u["chrom"]), u["start"].tolist(), u["end"].tolist()))
        cons_path = os.path.join(tmp, "consensus_sorted.bed")
        with open(cons_path, "w") as fh:
            fh.write("".join(f"{c}\t{s}\t{e}\n" for c, s, e in rows))
        cons = scoring.ConsensusSet(cons_path)
        n_peaks = len(cons)
        print(f"[countmat_bench] inputs written: {a.fragments} fragments, {a.barcodes} barcodes, {n_peaks} peaks", flush=True)

        # ---- both results, compared
        m = scoring.barcode_count_matrix(frag, cons)
        print(f"[countmat_bench] csr: {m.shape[0]} x {m.shape[1]}, nnz {m.nnz}", flush=True)
        old = scoring.barcode_scoring_from_fragments(frag, cons)
        assert m.to_dict() == old, "the CSR matrix and the dict form differ"
        print("[countmat_bench] to_dict() == barcode_scoring_from_fragments: ok", flush=True)

        # ---- the matrix step alone, on resident hits
        c, s, e, b, barcodes = scoring._read_fragments(frag, cons)
        order = sorted(range(len(barcodes)), key=lambda i: barcodes[i].encode())
        rank = np.empty(len(barcodes), dtype=np.uint32)
        rank[order] = np.arange(len(barcodes), dtype=np.uint32)
        dev = torch.device("cuda", torch.cuda.current_device())
        stream = torch.cuda.current_stream().cuda_stream
        d = [torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to(dev) for x in (c, s, e, rank[b])]
        nq, n_rows = len(c), len(barcodes)
        offsets = torch.empty(nq + 1, dtype=torch.int64, device=dev)
        ids = torch.empty(4 * nq + 1024, dtype=torch.int32, device=dev)
        h = cons.index.tokenize_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), nq, offsets.data_ptr(), ids.data_ptr(), ids.numel(),
                                       stream, sync=True)
        indptr = torch.empty(n_rows + 1, dtype=torch.int64, device=dev)
        indices = torch.empty(h, dtype=torch.int32, device=dev)
        data = torch.empty(h, dtype=torch.int32, device=dev)

        def csr():
            return scoring.count_matrix_csr_device(offsets.data_ptr(), ids.data_ptr(), d[3].data_ptr(), nq, n_rows, n_peaks, indptr.data_ptr(),
                                                   indices.data_ptr(), data.data_ptr(), h, stream)

        nnz = csr()
        assert nnz == m.nnz and np.array_equal(indices[:nnz].cpu().numpy(), m.indices) and np.array_equal(data[:nnz].cpu().numpy(), m.data)
        dev_ms, walls = [], []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            csr()
            e1.record()
            e1.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
            dev_ms.append(e0.elapsed_time(e1))
        per_kernel = {}
        _lib.lib.gtars_prof_enable(1)
        try:
            for _ in range(a.reps):
                _lib.lib.gtars_prof_reset()
                csr()
                for k, v in _lib.prof_read().items():
                    per_kernel.setdefault(k, []).append(v["total_ms"])
        finally:
            _lib.lib.gtars_prof_enable(0)
            _lib.lib.gtars_prof_reset()
        kernels = {k: stat(v) for k, v in per_kernel.items()}

        def band_step():
            out = {}
            rows_per = max(1, min(n_rows, scoring.BAND_CELLS // n_peaks))
            band = torch.empty((rows_per, n_peaks), dtype=torch.int32, device=dev)
            for row0 in range(0, n_rows, rows_per):
                nr = min(rows_per, n_rows - row0)
                band.zero_()
                _lib.check(_lib.lib.gtars_histogram_rows_device(offsets.data_ptr(), ids.data_ptr(), d[3].data_ptr(), nq, row0, nr, n_peaks,
                                                                band.data_ptr(), stream))
                mm = band[:nr].cpu().numpy().view(np.uint32)
                r, k = np.nonzero(mm)
                for ri, ki, v in zip(r.tolist(), k.tolist(), mm[r, k].tolist()):
                    out.setdefault(row0 + ri, {})[ki] = v
            return out

        got = band_step()
        assert sum(len(r) for r in got.values()) == nnz
        t_band = wall_ms(band_step, a.dict_reps)
        print(f"[countmat_bench] matrix step: csr {stat(dev_ms)[0]:.3f} ms (events), band {t_band[0]:.1f} ms (wall)", flush=True)

        # ---- end to end, from the file
        t_new = wall_ms(lambda: scoring.barcode_count_matrix(frag, cons), a.dict_reps)
        t_new_dev = wall_ms(lambda: scoring.barcode_count_matrix(frag, cons, device=True), a.dict_reps)
        t_to_dict = wall_ms(m.to_dict, a.dict_reps)
        t_old = wall_ms(lambda: scoring.barcode_scoring_from_fragments(frag, cons), a.dict_reps)

    row = {"fragments": a.fragments, "barcodes": n_rows, "peaks": n_peaks, "hits": h, "nnz": nnz, "checks": "ok",
           "dense_cells": n_rows * n_peaks, "bands": -(-n_rows // max(1, min(n_rows, scoring.BAND_CELLS // n_peaks))),
           "csr_build_device_ms": stat(dev_ms), "csr_build_wall_ms": stat(walls), "csr_kernels_ms": kernels,
           "band_step_wall_ms": t_band, "band_over_csr_matrix_step": t_band[0] / stat(walls)[0],
           "barcode_count_matrix_wall_ms": t_new, "barcode_count_matrix_device_true_wall_ms": t_new_dev, "to_dict_wall_ms": t_to_dict,
           "barcode_scoring_from_fragments_wall_ms": t_old, "dict_over_csr_end_to_end": t_old[0] / t_new[0]}
    print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(row, f, indent=1)


if __name__ == "__main__":
    main()
