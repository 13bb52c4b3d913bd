"""BAM input and BAM QC (K17; gtars-uniwig/src/reading.rs:279-319, bamqc.rs).

``BamFile`` opens a coordinate-sorted BAM through the library's own BGZF reader: the block table, the header, the
inflated bytes (host threads) and the records' columns (decoded on the device).  ``compute_bam_qc`` is the reference's
library-complexity QC -- NRF, PBC1, PBC2, duplicate and mitochondrial rate -- computed on the device from the decoded
records; ``run_bam_qc`` / ``write_bam_qc_tsv`` write the reference's TSV.  ``BamFile.fragments`` / ``bam_to_fragments`` (K26,
this library's own) turn a paired-end BAM into the deduplicated fragments of a 10x-style fragment file -- filters, barcode tag,
Tn5 shift, sort and dedup on the device.  No ``.bai`` is needed or read.  Without a device the calls that decode records
raise NoDeviceError: there is no host fallback.
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

    def fragments(self, barcode_tag: Optional[str] = "CB", min_mapq: int = 30, max_fragment_length: int = 2000,
                  shift: Tuple[int, int] = (4, -5), require_flags: int = 0x3, exclude_flags: int = 0xB0C, sample: str = "bulk",
                  threads: int = 0, max_window_bytes: Optional[int] = None) -> "BamFragments":
        """The deduplicated fragments of a coordinate-sorted paired-end BAM (K26): the leftmost mate of
        every pair that passes the filters gives (start, end) = (pos + shift[0], pos + tlen + shift[1]), clamped to the
        reference; equal (reference, start, end, barcode) tuples collapse into one row with their multiplicity as count.
        barcode_tag=None: no tag is read and every pair carries `sample`."""
        p = _frag_params(barcode_tag, min_mapq, max_fragment_length, shift, require_flags, exclude_flags, sample)
        h = C.c_void_p()
        check(lib.gtars_bam_fragments(self._h, C.byref(p), max_window_bytes or 0, threads, C.byref(h)))
        try:
            return BamFragments._take(h, self.references)
        finally:
            lib.gtars_bam_frags_free(h)


def read_bam_header(path: str) -> List[str]:
    """reading.rs:279-319: the reference names, in header order"""
    with BamFile(path) as b:
        return [name for name, _ in b.references]


def compute_bam_qc(path: str, threads: int = 1, max_window_bytes: Optional[int] = None) -> BamQcResult:
    """bamqc.rs:165-319 (compute_bam_qc and compute_bam_qc_parallel give the same numbers).  threads: host threads that
    inflate, capped by the library's budget; max_window_bytes: inflated bytes per device window (default 256 MiB)."""
    with BamFile(path) as b:
        return b.qc(threads, max_window_bytes)


FRAG_STATS = ("records", "unplaced", "flag", "mapq", "mate_ref", "not_leftmost", "too_long", "no_barcode", "empty", "kept_pairs", "fragments",
              "barcodes")


class _FragParams(C.Structure):
    _fields_ = [("barcode_tag", C.c_char * 2), ("use_barcode_tag", C.c_int32), ("sample", C.c_char_p), ("min_mapq", C.c_int32),
                ("max_fragment_length", C.c_int64), ("shift_left", C.c_int32), ("shift_right", C.c_int32), ("require_flags", C.c_uint32),
                ("exclude_flags", C.c_uint32)]


def _frag_params(barcode_tag, min_mapq, max_fragment_length, shift, require_flags, exclude_flags, sample) -> _FragParams:
    """the parameter block of gtars_bam_fragments; ValueError for what the call refuses, before any device work"""
    p = _FragParams()
    if barcode_tag is not None:
        tag = barcode_tag.encode() if isinstance(barcode_tag, str) else bytes(barcode_tag)
        if len(tag) != 2 or 0 in tag:
            raise ValueError(f"barcode_tag must be two bytes, not {barcode_tag!r}")
        p.barcode_tag, p.use_barcode_tag = tag, 1
    else:
        if not isinstance(sample, str) or not sample or any(c.isspace() for c in sample):
            raise ValueError(f"sample must not be empty and must hold no white space, not {sample!r}")
        p.use_barcode_tag = 0
    p.sample = (sample if isinstance(sample, str) else "").encode()
    if min_mapq < 0:
        raise ValueError("min_mapq must not be negative")
    if max_fragment_length < 1:
        raise ValueError("max_fragment_length must be at least 1")
    shift = tuple(int(s) for s in shift)
    if len(shift) != 2 or any(abs(s) >= 1 << 31 for s in shift):
        raise ValueError("shift must be two 32-bit integers")
    if not 0 <= require_flags <= 0xFFFF or not 0 <= exclude_flags <= 0xFFFF:
        raise ValueError("require_flags and exclude_flags are 16-bit flag masks")
    p.min_mapq, p.max_fragment_length = min(int(min_mapq), 256), min(int(max_fragment_length), (1 << 62))
    p.shift_left, p.shift_right = shift
    p.require_flags, p.exclude_flags = int(require_flags), int(exclude_flags)
    return p


def _frag_stats(h) -> Dict[str, int]:
    out = (C.c_uint64 * len(FRAG_STATS))()
    lib.gtars_bam_frags_stats(h, C.cast(out, C.c_void_p))
    return {k: int(out[i]) for i, k in enumerate(FRAG_STATS)}


class BamFragments:
    """The rows of BamFile.fragments in (ref, start, end, barcode) order: numpy columns ``ref`` (int32, the header's reference
    ids), ``start``, ``end``, ``barcode`` (ids into ``barcodes``) and ``count`` (uint32); ``barcodes`` in id order (the byte
    order of the distinct barcodes); ``references`` as (name, length); ``stats``."""

    def __init__(self, ref, start, end, barcode, count, barcodes: List[str], references: List[Tuple[str, int]], stats: Dict[str, int]):
        self.ref, self.start, self.end, self.barcode, self.count = ref, start, end, barcode, count
        self.barcodes, self.references, self.stats = barcodes, references, stats

    @classmethod
    def _take(cls, h, references) -> "BamFragments":
        n = int(lib.gtars_bam_frags_len(h))

        def col(fn, ctype, dtype):
            p = fn(h)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(n,)).copy() if n and p else np.zeros(0, dtype)

        names = []
        for i in range(int(lib.gtars_bam_frags_n_barcodes(h))):
            ln = C.c_uint64()
            names.append(C.string_at(lib.gtars_bam_frags_barcode_name(h, i, C.byref(ln)), ln.value).decode("utf-8", "replace"))
        return cls(col(lib.gtars_bam_frags_ref, C.c_int32, np.int32), col(lib.gtars_bam_frags_start, C.c_uint32, np.uint32),
                   col(lib.gtars_bam_frags_end, C.c_uint32, np.uint32), col(lib.gtars_bam_frags_barcode, C.c_uint32, np.uint32),
                   col(lib.gtars_bam_frags_count, C.c_uint32, np.uint32), names, list(references), _frag_stats(h))

    def __len__(self) -> int:
        return len(self.ref)

    def write(self, path) -> None:
        """``chrom\\tstart\\tend\\tbarcode\\tcount`` per row; one gzip member when the path ends in ``.gz``"""
        refs = (C.c_char_p * max(len(self.references), 1))(*[name.encode() for name, _ in self.references])
        bcs = (C.c_char_p * max(len(self.barcodes), 1))(*[b.encode() for b in self.barcodes])
        cols = [np.ascontiguousarray(self.ref, np.int32)] + [np.ascontiguousarray(c, np.uint32) for c in (self.start, self.end, self.barcode, self.count)]
        check(lib.gtars_fragments_write_text(str(path).encode(), C.cast(refs, C.c_void_p), len(self.references), C.cast(bcs, C.c_void_p),
                                             len(self.barcodes), *(C.c_void_p(c.ctypes.data) for c in cols), len(self)))


def bam_to_fragments(bam_path: str, out_path: str, threads: int = 0, max_window_bytes: Optional[int] = None, **kw) -> Dict[str, int]:
    """BamFile.fragments(**kw) of the file at bam_path written to out_path (the rows never become Python objects); returns the
    statistics"""
    names = ("barcode_tag", "min_mapq", "max_fragment_length", "shift", "require_flags", "exclude_flags", "sample")
    dflt = dict(zip(names, ("CB", 30, 2000, (4, -5), 0x3, 0xB0C, "bulk")))
    unknown = set(kw) - set(names)
    if unknown:
        raise TypeError(f"bam_to_fragments: unexpected arguments {sorted(unknown)}")
    p = _frag_params(*(kw.get(k, dflt[k]) for k in names))
    with BamFile(bam_path) as b:
        h = C.c_void_p()
        check(lib.gtars_bam_fragments(b._h, C.byref(p), max_window_bytes or 0, threads, C.byref(h)))
        try:
            check(lib.gtars_bam_frags_write(h, b._h, str(out_path).encode()))
            return _frag_stats(h)
        finally:
            lib.gtars_bam_frags_free(h)


def last_stages() -> Dict[str, float]:
    """where the calling thread's last compute_bam_qc / columns() / fragments() spent its host time"""
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
