"""Genome assemblies and the two sequence statistics of gtars-genomicdist: ``GenomeAssembly`` (plain FASTA),
``BinaryGenomeAssembly`` (.fab) and ``write_fab`` (gtars-genomicdist/src/models.rs:145-413,
gtars-python/src/models/genome_assembly.rs), ``calc_gc_content`` and ``calc_dinucl_freq`` (statistics.rs:331-483,
gtars-python/src/genomic_distributions/tools.rs:8-70).

The reference has the classes in ``gtars.models`` and the functions in ``gtars.genomic_distributions``.  Here they live
in this module (``gtars.seqstats`` under the reference's import root): the suite pins both of those modules as having no
``GenomeAssembly`` / ``BinaryGenomeAssembly`` / ``calc_gc_content`` (tests/test_annot_cpu.py,
tests/test_genomicdist_cpu.py), and the group stays in one place rather than split across three.  Signatures, return
values and errors are the reference's.

An assembly holds a genome's sequences on the host and, from the first counting call on, as one packed buffer on the
device that was current then (csrc/seqstats.hip).  Integer counts per region come back from
the device; the divisions are the library's host f64 arithmetic in the reference's order of operations, so the values
are the reference's bit for bit.  Output rows follow the reference's loops: chromosomes in order of first appearance in
the set, set order within one.  ``counts_device`` is the device-pointer entry for callers whose columns are on the GPU
already.

There is no CPU fallback: without a device a counting call that has rows to count raises NoDeviceError.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional

from . import _lib
from ._lib import check, dec, lib
from .models import RegionSet, _take

SEQ_PIECE = int(lib.gtars_seqstats_piece_bytes())  # bytes of a region one work item of the counting kernels covers
DINUCLEOTIDES = ["Aa", "Ac", "Ag", "At", "Ca", "Cc", "Cg", "Ct", "Ga", "Gc", "Gg", "Gt", "Ta", "Tc", "Tg", "Tt"]
SEQ_MODES = {"gc": 0, "dinucl": 1}


def _value_error(fn, *args):
    """the library call, every failure as the ValueError the reference's constructors raise"""
    try:
        check(fn(*args))
    except (OSError, _lib.GtarsError) as e:
        raise ValueError(str(e)) from None


def _runtime_error(fn, *args):
    """the library call, every failure as the RuntimeError the reference's anyhow errors become"""
    try:
        check(fn(*args))
    except (ValueError, OSError) as e:
        raise RuntimeError(str(e)) from None


def _u64(x) -> int:
    if not 0 <= int(x) < 1 << 64:
        raise OverflowError("position must fit in u64")
    return int(x)


class _Assembly:
    """what the two assembly classes share: the handle, its accessors, the lazily built device image"""

    _open = None

    def __init__(self, path):
        self._h = None
        h = C.c_void_p()
        _value_error(type(self)._open, os.fspath(path).encode("utf-8"), C.byref(h))
        self._h = h

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib.gtars_assembly_free(self._h)
                self._h = None
        except Exception:
            pass

    def __len__(self) -> int:
        return int(lib.gtars_assembly_n_chrom(self._h))

    @property
    def chrom_names(self) -> List[str]:
        """chromosome names by assembly id (order of first appearance in the file)"""
        return [dec(lib.gtars_assembly_chrom_name(self._h, i)) for i in range(len(self))]

    @property
    def chrom_sizes(self) -> Dict[str, int]:
        return {dec(lib.gtars_assembly_chrom_name(self._h, i)): int(lib.gtars_assembly_chrom_len(self._h, i))
                for i in range(len(self))}

    def contains_chr(self, name: str) -> bool:
        return bool(lib.gtars_assembly_contains(self._h, str(name).encode("utf-8")))

    def sequence(self, chr: str, start: int, end: int) -> bytes:
        """the bytes [start, end) of a chromosome as the file has them; ValueError unless end <= length and start <= end"""
        p = C.c_void_p()
        check(lib.gtars_assembly_sequence(self._h, str(chr).encode("utf-8"), _u64(start), _u64(end), C.byref(p)))
        return C.string_at(p, int(end) - int(start))

    def refget_digests(self, threads: int = 0) -> Dict[str, str]:
        """chromosome name -> sha512t24u of its upper-cased bytes (the GA4GH refget digest, without "SQ."): computed once per
        assembly, one chromosome per host task, and kept on the handle; what ``gtars.vrs`` names a chromosome by"""
        p = C.c_void_p()
        check(lib.gtars_assembly_refget_digests(self._h, int(threads), C.byref(p)))
        names = self.chrom_names
        blob = C.string_at(p, 33 * len(names))
        return {name: blob[33 * k:33 * k + 32].decode("ascii") for k, name in enumerate(names)}

    @property
    def device(self) -> int:
        """the device that holds the packed image; -1 until the first counting call"""
        return int(lib.gtars_assembly_device(self._h))

    def __repr__(self) -> str:
        return f"{type(self).__name__} with {len(self)} chromosomes."


class GenomeAssembly(_Assembly):
    """GenomeAssembly(path) -- a plain FASTA file read into memory (models.rs:145-215).  Names end at the first whitespace
    of the header, sequences keep their bytes (no case folding), a repeated name keeps the last record."""

    _open = lib.gtars_assembly_from_fasta


class BinaryGenomeAssembly(_Assembly):
    """BinaryGenomeAssembly(path) -- a .fab binary FASTA file (models.rs:229-318), see ``write_fab``."""

    _open = lib.gtars_assembly_from_fab


def write_fab(fasta_path, out_path) -> None:
    """BinaryGenomeAssembly::write_from_fasta (models.rs:357-412): every record of the FASTA file, in file order, as .fab.
    The reference's Python package does not expose it."""
    _value_error(lib.gtars_fab_write_from_fasta, os.fspath(fasta_path).encode("utf-8"), os.fspath(out_path).encode("utf-8"))


def _genome_handle(genome):
    if not isinstance(genome, _Assembly):
        raise RuntimeError("genome must be a GenomeAssembly or BinaryGenomeAssembly")
    return genome._h


def calc_gc_content(rs: RegionSet, genome, ignore_unk_chroms: Optional[bool] = False) -> List[float]:
    """GC fraction of every region: bytes that are G, C, g or c over the region's width (N counts in the width), 0.0 for an
    empty region.  With ``ignore_unk_chroms`` chromosomes the assembly lacks and out-of-range regions are skipped;
    without it the first one raises RuntimeError (statistics.rs:331-383)."""
    h = _genome_handle(genome)
    p, n = C.c_void_p(), C.c_uint64()
    _runtime_error(lib.gtars_seqstats_gc, h, rs._h, 1 if ignore_unk_chroms else 0, C.byref(p), C.byref(n))
    return _take(p, C.c_double, n.value)


def calc_dinucl_freq(rs: RegionSet, genome, raw_counts: bool = False, ignore_unk_chroms: bool = False) -> dict:
    """per-region dinucleotide frequencies: {"region_labels": chr_start_end per row, "dinucleotides": "Aa" .. "Tt",
    "frequencies": one row of 16 per region -- counts as floats (``raw_counts``) or percentages of the region's valid
    windows, a zero row when it has none} (statistics.rs:426-483, tools.rs:42-70)"""
    h = _genome_handle(genome)
    pi, pf, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
    _runtime_error(lib.gtars_seqstats_dinucl, h, rs._h, 1 if raw_counts else 0, 1 if ignore_unk_chroms else 0, C.byref(pi),
                   C.byref(pf), C.byref(n))
    rows = _take(pi, C.c_uint64, n.value)
    flat = _take(pf, C.c_double, n.value * 16)
    names, ids, s, e = rs.chrom_names, rs.chrom_ids.tolist(), rs.starts.tolist(), rs.ends.tolist()
    return {
        "region_labels": [f"{names[ids[i]]}_{s[i]}_{e[i]}" for i in rows],
        "dinucleotides": list(DINUCLEOTIDES),
        "frequencies": [flat[16 * k:16 * k + 16] for k in range(n.value)],
    }


def counts_device(genome, mode: str, d_chrom: int, d_start: int, d_end: int, n: int, d_out: int, stream: int = 0) -> None:
    """integer counts of n device rows (device pointers; chromosome ids of the assembly, every row start <= end <= length)
    into d_out -- n u32 for mode "gc", n * 16 for "dinucl" -- queued on ``stream``, which is drained before the call
    returns"""
    check(lib.gtars_seqstats_counts_device(_genome_handle(genome), C.c_void_p(d_chrom), C.c_void_p(d_start), C.c_void_p(d_end),
                                           int(n), SEQ_MODES[mode], C.c_void_p(d_out), C.c_void_p(stream)))
