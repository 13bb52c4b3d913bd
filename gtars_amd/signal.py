"""Signal matrices of gtars-genomicdist: ``SignalMatrix`` (gtars-genomicdist/src/signal.rs:33-354,
gtars-python/src/models/signal_matrix.rs) and ``calc_summary_signal`` (signal.rs:356-526,
gtars-python/src/genomic_distributions/tools.rs:120-155).

The reference has the class in ``gtars.models`` and the function in ``gtars.genomic_distributions``.  Here they live in
this module (``gtars.signal`` under the reference's import root), like the assemblies of ``gtars.seqstats``: the suite
pins both of those modules as having no ``SignalMatrix`` / ``calc_summary_signal`` (tests/test_annot_cpu.py,
tests/test_genomicdist_cpu.py).  Signatures, return values and errors are the reference's.

A matrix holds its rows and values on the host and, from the first summary on, as an overlap index plus the row-major
values on the device that was current then (csrc/signal.hip).  The per-query fold and the
boxplot statistics come back from the device bit for bit as the reference computes them; a result column that holds a
NaN has no defined statistics in the reference and sorts its NaNs last here.  ``summary_arrays`` is the same call
without Python lists, ``summary_device`` the device-pointer entry for callers whose query columns are on the GPU.

There is no CPU fallback: without a device a summary whose queries share a chromosome with the matrix raises
NoDeviceError.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import check, cstr_array, dec, lib, ptr
from .models import RegionSet

STAT_FIELDS = ("lower_whisker", "lower_hinge", "median", "upper_hinge", "upper_whisker")
SPLIT_HITS = int(lib.gtars_debug_signal_split_hits())  # a query with more hits is folded by a whole workgroup


def _value_error(fn, *args):
    """the library call, every failure as the ValueError the reference's constructors raise"""
    try:
        check(fn(*args))
    except (OSError, _lib.GtarsError) as e:
        raise ValueError(str(e)) from None


def _array(p: C.c_void_p, ctype, dtype, n: int) -> np.ndarray:
    """a library-allocated array as an ndarray of its own, freed"""
    try:
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(n,)).astype(dtype, copy=True) if n else np.zeros(0, dtype)
    finally:
        if p.value:
            lib.gtars_free(p)


class SignalMatrix:
    """a region x condition matrix of f64, rows in file order (never sorted, duplicates kept)"""

    def __init__(self, *args, **kwargs):
        raise TypeError("SignalMatrix has no constructor: use SignalMatrix.from_tsv, load_bin or from_arrays")

    @classmethod
    def _open(cls, fn, *args) -> "SignalMatrix":
        self = cls.__new__(cls)
        self._h = None
        h = C.c_void_p()
        _value_error(fn, *args, C.byref(h))
        self._h = h
        return self

    @staticmethod
    def from_tsv(path) -> "SignalMatrix":
        """a TSV file (".gz" by extension): header ``id<TAB>condition...``, rows ``chr_start_end<TAB>value...``; rows that
        do not parse are skipped, a file without a valid row is a ValueError (signal.rs:73-164)"""
        return SignalMatrix._open(lib.gtars_signal_from_tsv, os.fspath(path).encode("utf-8"))

    @staticmethod
    def load_bin(path) -> "SignalMatrix":
        """a packed SIGM version 2 file (signal.rs:239-354)"""
        return SignalMatrix._open(lib.gtars_signal_load_bin, os.fspath(path).encode("utf-8"))

    @staticmethod
    def from_arrays(chrs: Sequence[str], starts, ends, values, condition_names: Sequence[str]) -> "SignalMatrix":
        """rows (chrs[i], starts[i], ends[i]) with values[i, :], one column per condition name.  Additive."""
        chrs, cond = list(chrs), [str(c) for c in condition_names]
        s, e = np.ascontiguousarray(starts, dtype=np.uint32), np.ascontiguousarray(ends, dtype=np.uint32)
        v = np.ascontiguousarray(values, dtype=np.float64)
        if len(s) != len(chrs) or len(e) != len(chrs):
            raise ValueError("chrs, starts, and ends must have the same length")
        if v.size != len(chrs) * len(cond) or (v.ndim == 2 and v.shape != (len(chrs), len(cond))):
            raise ValueError("values must hold one row per region and one column per condition")
        names: dict = {}
        ids = np.fromiter((names.setdefault(str(c), len(names)) for c in chrs), dtype=np.uint32, count=len(chrs))
        narr, _keep1 = cstr_array(list(names))
        carr, _keep2 = cstr_array(cond)
        return SignalMatrix._open(lib.gtars_signal_from_arrays, C.cast(narr, C.c_void_p), len(names), ptr(ids), ptr(s), ptr(e),
                                  len(chrs), ptr(v), C.cast(carr, C.c_void_p), len(cond))

    def save_bin(self, path) -> None:
        """the matrix as a packed SIGM version 2 file (signal.rs:170-236).  The reference's Python package does not
        expose it."""
        _value_error(lib.gtars_signal_save_bin, self._h, os.fspath(path).encode("utf-8"))

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib.gtars_signal_free(self._h)
                self._h = None
        except Exception:
            pass

    @property
    def condition_names(self) -> List[str]:
        return [dec(lib.gtars_signal_condition_name(self._h, i)) for i in range(self.n_conditions)]

    @property
    def n_conditions(self) -> int:
        return int(lib.gtars_signal_n_conditions(self._h))

    @property
    def n_regions(self) -> int:
        return int(lib.gtars_signal_n_regions(self._h))

    def __len__(self) -> int:
        return self.n_regions

    def __repr__(self) -> str:
        return f"SignalMatrix(n_regions={self.n_regions}, n_conditions={self.n_conditions})"

    # -- the rows, additive ------------------------------------------------------------------------------------------
    @property
    def chrom_names(self) -> List[str]:
        """chromosome names by matrix id (order of first appearance among the rows)"""
        return [dec(lib.gtars_signal_chrom_name(self._h, i)) for i in range(int(lib.gtars_signal_n_chrom(self._h)))]

    def _col(self, fn, ctype, n) -> np.ndarray:
        return np.ctypeslib.as_array(C.cast(fn(self._h), C.POINTER(ctype)), shape=(n,)).copy()

    @property
    def chrom_ids(self) -> np.ndarray:
        return self._col(lib.gtars_signal_chrom_ids, C.c_uint32, self.n_regions)

    @property
    def starts(self) -> np.ndarray:
        return self._col(lib.gtars_signal_starts, C.c_uint32, self.n_regions)

    @property
    def ends(self) -> np.ndarray:
        return self._col(lib.gtars_signal_ends, C.c_uint32, self.n_regions)

    @property
    def values(self) -> np.ndarray:
        """the n_regions x n_conditions values"""
        return self._col(lib.gtars_signal_values, C.c_double, self.n_regions * self.n_conditions).reshape(self.n_regions, self.n_conditions)

    @property
    def device(self) -> int:
        """the device that holds the matrix and its overlap index; -1 until the first summary"""
        return int(lib.gtars_signal_device(self._h))


def _handle(signal_matrix):
    if not isinstance(signal_matrix, SignalMatrix):
        raise TypeError("signal_matrix must be a SignalMatrix")
    return signal_matrix._h


def _results(pq, pv, ps, n_rows: int, n_cond: int, rows: bool = True) -> Tuple[Optional[np.ndarray], Optional[np.ndarray], np.ndarray]:
    qidx = _array(pq, C.c_uint32, np.int64, n_rows) if rows else None
    values = _array(pv, C.c_double, np.float64, n_rows * n_cond).reshape(n_rows, n_cond) if rows else None
    stats = _array(ps, C.c_double, np.float64, n_cond * 5 if n_rows else 0).reshape(-1, 5)
    return qidx, values, stats


def summary_arrays(rs: RegionSet, signal_matrix: SignalMatrix) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """calc_summary_signal as arrays: the indices (rows of ``rs``) of the R queries that overlap a row of the matrix, in
    query order; the R x n_conditions result; the n_conditions x 5 statistics in the order of ``STAT_FIELDS`` (0 x 5
    when R == 0).  Additive."""
    h = _handle(signal_matrix)
    pq, pv, ps, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    check(lib.gtars_signal_summary(h, rs._h, C.byref(pq), C.byref(pv), C.byref(ps), C.byref(n)))
    return _results(pq, pv, ps, n.value, signal_matrix.n_conditions)


def calc_summary_signal(rs: RegionSet, signal_matrix: SignalMatrix) -> dict:
    """for every region of ``rs`` that overlaps a row of the matrix, per condition the maximum over the overlapping rows,
    and Tukey boxplot statistics of every condition's column: {"condition_names", "region_labels": chr_start_end per
    result row, "signal_matrix": one list per result row, "matrix_stats": one dict {condition, lower_whisker,
    lower_hinge, median, upper_hinge, upper_whisker} per condition -- none when nothing overlapped}"""
    qidx, values, stats = summary_arrays(rs, signal_matrix)
    cond = signal_matrix.condition_names
    names, ids, s, e = rs.chrom_names, rs.chrom_ids.tolist(), rs.starts.tolist(), rs.ends.tolist()
    return {
        "condition_names": cond,
        "region_labels": [f"{names[ids[i]]}_{s[i]}_{e[i]}" for i in qidx.tolist()],
        "signal_matrix": values.tolist(),
        "matrix_stats": [dict([("condition", cond[c])] + list(zip(STAT_FIELDS, row))) for c, row in enumerate(stats.tolist())],
    }


def summary_device(signal_matrix: SignalMatrix, d_chrom: int, d_start: int, d_end: int, n: int, stream: int = 0, rows: bool = True):
    """the summary of n device rows (device pointers; d_chrom: chromosome ids of the matrix, any other value gives no
    hits), queued on ``stream``, which is drained before the call returns.  Returns what ``summary_arrays`` returns;
    with ``rows=False`` the result rows stay on the device and (None, None, stats, R) comes back."""
    h = _handle(signal_matrix)
    pq, pv, ps, cnt = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    check(lib.gtars_signal_summary_device(h, C.c_void_p(d_chrom), C.c_void_p(d_start), C.c_void_p(d_end), int(n), C.c_void_p(stream),
                                          C.byref(pq) if rows else None, C.byref(pv) if rows else None, C.byref(ps), C.byref(cnt)))
    out = _results(pq, pv, ps, cnt.value, signal_matrix.n_conditions, rows)
    return out if rows else out + (int(cnt.value),)
