"""BAM input and BAM QC (K17; gtars-uniwig/src/reading.rs:279-319, bamqc.rs).

``BamFile`` opens a coordinate-sorted BAM through the library's own BGZF reader: the block table, the header, the
inflated bytes (host threads) and the records' columns (decoded on the device).  ``compute_bam_qc`` is the reference's
library-complexity QC -- NRF, PBC1, PBC2, duplicate and mitochondrial rate -- computed on the device from the decoded
records; ``run_bam_qc`` / ``write_bam_qc_tsv`` write the reference's TSV.  No ``.bai`` is needed or read.  Without a
device the calls that decode records raise NoDeviceError: there is no host fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from decimal import Decimal
from typing import Dict, List, Optional, TextIO, Tuple

import numpy as np

from ._lib import check, dec, lib, take_array

COLUMNS = ("ref_id", "start", "end", "flag", "mapq", "l_seq", "tlen")
TSV_HEADER = ("Total_read_pairs\tDistinct_read_pairs\tOne_read_pair\tTwo_read_pairs\tDuplicate_rate\tMitochondria_reads\t"
              "Mitochondria_rate\tNRF\tPBC1\tPBC2")


class _QcResult(C.Structure):
    _fields_ = [(k, C.c_uint64) for k in ("total_reads", "distinct", "m1", "m2", "dups", "mito_reads")] + \
               [(k, C.c_double) for k in ("nrf", "pbc1", "pbc2")]


@dataclass
class BamQcResult:
    """bamqc.rs:21-50"""
    total_reads: int = 0
    distinct: int = 0
    m1: int = 0
    m2: int = 0
    dups: int = 0
    mito_reads: int = 0
    nrf: float = 0.0
    pbc1: float = 0.0
    pbc2: float = 0.0

    def mito_rate(self) -> float:
        return 0.0 if self.total_reads == 0 else self.mito_reads / self.total_reads

    def dup_rate(self) -> float:
        return 0.0 if self.total_reads == 0 else self.dups / self.total_reads


class BamFile:
    """An open BAM file: header, BGZF block table, inflated bytes, record offsets and decoded columns."""

    def __init__(self, path: str):
        self.path = str(path)
        self._h = C.c_void_p()
        check(lib.gtars_bam_open(self.path.encode(), C.byref(self._h)))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            lib.gtars_bam_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # (interpreter shutdown: the module's globals may be gone)
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def header_text(self) -> str:
        return dec(lib.gtars_bam_header_text(self._h))

    @property
    def references(self) -> List[Tuple[str, int]]:
        """(name, length) in header order"""
        return [(dec(lib.gtars_bam_ref_name(self._h, i)), int(lib.gtars_bam_ref_len(self._h, i))) for i in range(lib.gtars_bam_n_ref(self._h))]

    @property
    def n_blocks(self) -> int:
        return int(lib.gtars_bam_n_blocks(self._h))

    @property
    def n_bytes(self) -> int:
        """inflated"""
        return int(lib.gtars_bam_n_bytes(self._h))

    @property
    def first_record(self) -> int:
        """offset of the first record in the inflated stream"""
        return int(lib.gtars_bam_first_record(self._h))

    def block_table(self) -> Dict[str, np.ndarray]:
        """per BGZF block: offset and size in the file, ISIZE, CRC-32, offset in the inflated stream"""
        n = self.n_blocks
        t = {"coff": np.zeros(n, np.uint64), "csize": np.zeros(n, np.uint32), "isize": np.zeros(n, np.uint32), "crc": np.zeros(n, np.uint32),
             "uoff": np.zeros(n, np.uint64)}
        check(lib.gtars_bam_block_table(self._h, *(C.c_void_p(a.ctypes.data) for a in t.values())))
        return t

    def inflate(self, block0: int = 0, block1: Optional[int] = None, threads: int = 0) -> bytes:
        """the inflated bytes of blocks [block0, block1), every block's length and CRC-32 checked"""
        block1 = self.n_blocks if block1 is None else block1
        t = self.block_table()
        end = self.n_bytes if block1 >= self.n_blocks else int(t["uoff"][block1])
        begin = self.n_bytes if block0 >= self.n_blocks else int(t["uoff"][block0])
        buf = np.zeros(max(end - begin, 0), np.uint8)
        check(lib.gtars_bam_inflate(self._h, block0, block1, C.c_void_p(buf.ctypes.data), buf.size, threads))
        return buf.tobytes()

    def record_offsets(self, data: Optional[bytes] = None, begin: Optional[int] = None, final: bool = True) -> np.ndarray:
        """offsets of the records' block_size fields in `data` (default: the whole inflated file, from the first record)"""
        if data is None:
            data, begin = self.inflate(), self.first_record if begin is None else begin
        begin = 0 if begin is None else begin
        p, n, used = C.c_void_p(), C.c_uint64(), C.c_uint64()
        check(lib.gtars_bam_record_offsets(self._h, data, len(data), begin, 1 if final else 0, C.byref(p), C.byref(n), C.byref(used)))
        self.consumed = int(used.value)
        return take_array(p, int(n.value), C.c_uint64, np.uint64)

    def columns(self, first: int = 0, count: Optional[int] = None, threads: int = 0, max_window_bytes: Optional[int] = None) -> Dict[str, np.ndarray]:
        """records [first, first + count) decoded on the device: ref_id, start (0-based), end (start + the CIGAR's reference
        span), flag, mapq, l_seq, tlen -- int32 arrays"""
        p, n = C.c_void_p(), C.c_uint64()
        check(lib.gtars_bam_decode(self._h, first, (1 << 64) - 1 if count is None else count, max_window_bytes or 0, threads, C.byref(p), C.byref(n)))
        flat = take_array(p, 7 * int(n.value), C.c_int32, np.int32)
        return {k: flat[i * n.value:(i + 1) * n.value] for i, k in enumerate(COLUMNS)}

    def qc(self, threads: int = 1, max_window_bytes: Optional[int] = None) -> BamQcResult:
        r = _QcResult()
        check(lib.gtars_bam_qc(self._h, max_window_bytes or 0, threads, C.byref(r)))
        return BamQcResult(*(getattr(r, k) for k, _ in _QcResult._fields_))


def read_bam_header(path: str) -> List[str]:
    """reading.rs:279-319: the reference names, in header order"""
    with BamFile(path) as b:
        return [name for name, _ in b.references]


def compute_bam_qc(path: str, threads: int = 1, max_window_bytes: Optional[int] = None) -> BamQcResult:
    """bamqc.rs:165-319 (compute_bam_qc and compute_bam_qc_parallel give the same numbers).  threads: host threads that
    inflate, capped by the library's budget; max_window_bytes: inflated bytes per device window (default 256 MiB)."""
    with BamFile(path) as b:
        return b.qc(threads, max_window_bytes)


def last_stages() -> Dict[str, float]:
    """where the calling thread's last compute_bam_qc / columns() spent its host time"""
    out = (C.c_double * 6)()
    lib.gtars_bam_last_stages(C.cast(out, C.c_void_p))
    return {"open_s": out[0], "inflate_s": out[1], "walk_s": out[2], "windows": int(out[3]), "records": int(out[4]), "call_s": out[5]}


def format_f64(x: float) -> str:
    """a float as Rust's `{}` prints an f64: the shortest digits that round-trip, never an exponent, an integral value
    without a fraction"""
    if math.isnan(x):
        return "NaN"
    if math.isinf(x):
        return "inf" if x > 0 else "-inf"
    s = format(Decimal(repr(float(x))), "f")
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    return "-0" if s in ("-", "-0") else s


def write_bam_qc_tsv(result: BamQcResult, out: TextIO) -> None:
    """bamqc.rs:321-341"""
    r = result
    out.write(TSV_HEADER + "\n")
    out.write("\t".join([str(r.total_reads), str(r.distinct), str(r.m1), str(r.m2), format_f64(r.dup_rate()), str(r.mito_reads),
                         format_f64(r.mito_rate()), format_f64(r.nrf), format_f64(r.pbc1), format_f64(r.pbc2)]) + "\n")


def run_bam_qc(path: str, output: str, threads: int = 1) -> BamQcResult:
    """bamqc.rs:343-349"""
    result = compute_bam_qc(path, threads)
    with open(output, "w") as fh:
        write_bam_qc_tsv(result, fh)
    return result
