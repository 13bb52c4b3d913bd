"""Coverage tracks of a BED file on the device (gtars-uniwig, BED input): ``*_start``, ``*_end`` and ``*_core`` per-base
counts written as wig, bedGraph or npy.  The reference's Python package has no such module; this one lives under
``gtars_amd`` only.

What is computed: with unit scores and step 1 the reference's sweeps (counting.rs:32-290) are

    count(pos) = #{a_i <= pos} - #{e_i <= pos}        pos = a_0 .. max(chrom_size, a_{n-1} - 1)

over sorted window opens ``a`` and closes ``e``: ``a = max(1, p - m)``, ``e = p + m + 1`` for the start and the end track
(``p`` = start + 1 resp. end of the rows, ``m`` = smoothsize), ``a = start + 1``, ``e = end`` for the core track.  Outside
that domain the sweeps' results depend on their queue handling and are no coverage tracks, so ``stepsize != 1``, scored
input and a zero-length row on the core track raise ValueError.  BAM input and bigWig output are not provided.

The streaming uniwig (gtars-uniwig/src/stream.rs, ``gtars uniwig --streaming``) is the second half
of the module: ``stream_counts``, ``uniwig_streaming``, ``read_chrom_sizes``, ``write_records_as_wig`` /
``write_records_as_bedgraph``.  It adds every row's score (column 5) instead of 1, emits only the positions that carry
data, fills gaps of at most ``max_gap`` positions with zeros (-1: fully dense, 0: sparse), honours a step size, takes rows
in any order and drops nothing that the chrom.sizes file lacks.  The whole file is one chain of launches on the device.

There is no CPU fallback: without a device every compute call raises NoDeviceError.
"""
from __future__ import annotations

import ctypes as C
import enum
import json
import os
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np

from ._lib import as_u32, check, lib, ptr, take_u32
from .bam import read_bam_header  # noqa: F401  (reading.rs:279-319 lives beside the BED readers)

KINDS = {"start": 0, "end": 1, "core": 2}
WIG_CHUNK = 1 << 22  # entries formatted per call of the C++ writer


class Chromosome:
    """utils.rs:15-19 with unit scores: name, ``starts`` (start + 1) and ``ends``, each sorted on its own"""

    __slots__ = ("chrom", "starts", "ends")

    def __init__(self, chrom: str, starts: np.ndarray, ends: np.ndarray):
        self.chrom, self.starts, self.ends = chrom, starts, ends

    def __repr__(self):
        return f"Chromosome({self.chrom!r}, n={len(self.starts)})"


def read_chromosomes(path: str) -> List[Chromosome]:
    """create_chrom_vec_default_score (reading.rs:17-101) over the C++ BED reader (plain or .gz): one Chromosome per RUN of
    consecutive equal names in file order (a name that comes back later starts a new one), start + 1 and end of every row,
    the two columns sorted independently of each other."""
    from .cli import read_bed3_lines

    names, cid, starts, ends = read_bed3_lines(str(path))
    out: List[Chromosome] = []
    if not len(cid):
        return out
    # names are compared trimmed (reading.rs:55, 62): ids of names that differ in blanks only fall together
    names = [nme.strip() for nme in names]
    canon = np.fromiter((names.index(nme) for nme in names), dtype=np.int64, count=len(names))
    cid = canon[cid]
    cuts = np.flatnonzero(np.diff(cid) != 0) + 1
    lo = 0
    for hi in list(cuts) + [len(cid)]:
        s = np.sort(starts[lo:hi].astype(np.uint32) + np.uint32(1))
        e = np.sort(ends[lo:hi])
        out.append(Chromosome(names[int(cid[lo])], s, e))
        lo = int(hi)
    return out


def read_chromosome_sizes(path: str) -> Dict[str, int]:
    """read_chromosome_sizes (reading.rs:226-275): ``.sizes`` files split on blanks, ``.bed`` / ``.narrowPeak`` files take
    column 3; any other extension is refused as there"""
    ext = os.path.splitext(str(path))[1]
    sizes: Dict[str, int] = {}
    with open(path) as fh:
        for line in fh.read().splitlines():
            if ext in (".bed", ".narrowPeak"):
                it = line.split("\t")
                sizes[it[0]] = int(it[2])
            elif ext == ".sizes":
                it = line.split()
                sizes[it[0]] = int(it[1])
            else:
                raise ValueError(f"Unsupported file type: {path}")
    return sizes


def _domain(stepsize: int = 1, score: bool = False):
    if stepsize != 1:
        raise ValueError(f"stepsize {stepsize} is not provided: only stepsize 1 is a coverage track (gtars_amd.uniwig)")
    if score:
        raise ValueError("scored input (create_chrom_vec_scores) is not provided (gtars_amd.uniwig)")


def _columns(kind: str, opens, closes):
    if kind not in KINDS:
        raise ValueError(f"unknown count type {kind!r}: start, end or core")
    o = as_u32(opens)
    c = None
    if kind == "core":
        c = as_u32(closes)
        if len(c) != len(o):
            raise ValueError("starts and ends must have the same length")
    return o, c


def _track(kind: str, opens, closes, chrom_size: int, smoothsize: int, max_device_bytes: int = 0):
    o, c = _columns(kind, opens, closes)
    first, n = C.c_uint64(), C.c_uint64()
    out = C.c_void_p()
    check(lib.gtars_uniwig_counts(ptr(o), ptr(c) if c is not None else None, len(o), int(chrom_size), int(smoothsize), KINDS[kind],
                                  int(max_device_bytes), C.byref(first), C.byref(out), C.byref(n)))
    return take_u32(out, n.value), int(first.value)


def start_end_counts(positions, chrom_size: int, smoothsize: int, stepsize: int = 1, max_device_bytes: int = 0
                     ) -> Tuple[np.ndarray, int]:
    """start_end_counts (counting.rs:32-158) of ``positions`` (start + 1 or end of the rows, any order):
    -> (counts u32, first reported position).  ``max_device_bytes``: the track is produced in position windows of at most
    that many bytes on the device (0: the library's default)."""
    _domain(stepsize)
    return _track("start", positions, None, chrom_size, smoothsize, max_device_bytes)


def core_counts(starts, ends, chrom_size: int, stepsize: int = 1, max_device_bytes: int = 0) -> Tuple[np.ndarray, int]:
    """core_counts (counting.rs:167-290) of the rows ``(starts[i], ends[i])``, starts being start + 1 as in the reference's
    Chromosome: -> (counts u32, first reported position).  ValueError when some ``ends[i] < starts[i]`` (a zero-length row)."""
    _domain(stepsize)
    return _track("core", starts, ends, chrom_size, 0, max_device_bytes)


def track_extent(kind: str, opens, closes, chrom_size: int, smoothsize: int) -> Tuple[int, int]:
    """-> (first position, number of entries) of a track, on the host"""
    o, c = _columns(kind, opens, closes)
    first, n = C.c_uint64(), C.c_uint64()
    check(lib.gtars_uniwig_extent(ptr(o), ptr(c) if c is not None else None, len(o), int(chrom_size), int(smoothsize), KINDS[kind],
                                  C.byref(first), C.byref(n)))
    return int(first.value), int(n.value)


def counts_device(kind: str, d_opens: int, d_closes: int, n: int, smoothsize: int, window_first: int, window_len: int,
                  d_counts: int, stream: int = 0) -> None:
    """positions ``window_first .. window_first + window_len - 1`` of a track into device memory, queued on ``stream``.
    ``d_opens`` / ``d_closes`` (0 unless core): device pointers of ASCENDING u32 columns; ``d_counts``: 16-byte aligned."""
    if kind not in KINDS:
        raise ValueError(f"unknown count type {kind!r}: start, end or core")
    check(lib.gtars_uniwig_counts_device(C.c_void_p(d_opens), C.c_void_p(d_closes or 0), int(n), int(smoothsize), KINDS[kind],
                                         int(window_first), int(window_len), C.c_void_p(d_counts), C.c_void_p(stream or 0)))


def compress_counts(kind: str, opens, closes, chrom_size: int, smoothsize: int, start_position: int
                    ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """compress_counts (utils.rs:40-81) of a track, made on the device: -> (starts, ends, counts) u32, the runs beginning
    at ``start_position`` and advancing by one per entry, the closing run included"""
    o, c = _columns(kind, opens, closes)
    s, e, k = C.c_void_p(), C.c_void_p(), C.c_void_p()
    n = C.c_uint64()
    check(lib.gtars_uniwig_runs(ptr(o), ptr(c) if c is not None else None, len(o), int(chrom_size), int(smoothsize), KINDS[kind],
                                int(start_position), C.byref(s), C.byref(e), C.byref(k), C.byref(n)))
    return take_u32(s, n.value), take_u32(e, n.value), take_u32(k, n.value)


def nonzero_counts(kind: str, opens, closes, chrom_size: int, smoothsize: int, start_position: int
                   ) -> Tuple[np.ndarray, np.ndarray]:
    """the lines of write_to_wig_file_variable (writing.rs:149-179): (start_position + k, count) of the non-zero entries
    among the first ``chrom_size`` entries of a track, made on the device"""
    o, c = _columns(kind, opens, closes)
    p, k = C.c_void_p(), C.c_void_p()
    n = C.c_uint64()
    check(lib.gtars_uniwig_nonzero(ptr(o), ptr(c) if c is not None else None, len(o), int(chrom_size), int(smoothsize), KINDS[kind],
                                   int(start_position), C.byref(p), C.byref(k), C.byref(n)))
    return take_u32(p, n.value), take_u32(k, n.value)


# ---- writers (writing.rs:13-214); the text is formatted by the compiled host layer ---------------------------------------
def _take_text(text: C.c_void_p, n: C.c_uint64) -> bytes:
    try:
        return C.string_at(text, n.value)
    finally:
        lib.gtars_free(text)


def _mkparent(filename: str) -> None:
    parent = os.path.dirname(filename)
    if parent:
        os.makedirs(parent, exist_ok=True)


def write_to_wig_file(counts, filename: str, chromname: str, start_position: int, stepsize: int, chrom_size: int) -> None:
    """fixedStep header, then at most ``chrom_size`` ENTRIES (writing.rs:113-146); appends"""
    counts = as_u32(counts)[: int(chrom_size)]
    _mkparent(filename)
    with open(filename, "ab") as fh:
        fh.write(f"fixedStep chrom={chromname} start={start_position} step={stepsize}\n".encode())
        for lo in range(0, len(counts), WIG_CHUNK):
            part = counts[lo:lo + WIG_CHUNK]
            text, n = C.c_void_p(), C.c_uint64()
            check(lib.gtars_uniwig_format_counts(ptr(part), len(part), C.byref(text), C.byref(n)))
            fh.write(_take_text(text, n))


def write_to_wig_file_variable(positions, counts, filename: str, chromname: str) -> None:
    """variableStep header, then ``position<TAB>count`` of the pairs of nonzero_counts (writing.rs:149-179); appends"""
    positions, counts = as_u32(positions), as_u32(counts)
    _mkparent(filename)
    with open(filename, "ab") as fh:
        fh.write(f"variableStep chrom={chromname}\n".encode())
        for lo in range(0, len(counts), WIG_CHUNK):
            a, b = positions[lo:lo + WIG_CHUNK], counts[lo:lo + WIG_CHUNK]
            text, n = C.c_void_p(), C.c_uint64()
            check(lib.gtars_uniwig_format_pairs(ptr(a), ptr(b), len(a), C.byref(text), C.byref(n)))
            fh.write(_take_text(text, n))


def write_to_bed_graph_file(count_info, filename: str, chromname: str) -> None:
    """``chrom<TAB>start<TAB>end<TAB>count`` per run (writing.rs:182-214); appends"""
    s, e, k = (as_u32(x) for x in count_info)
    if not (len(s) == len(e) == len(k)):
        raise ValueError("count info vectors are not equal!")
    _mkparent(filename)
    with open(filename, "ab") as fh:
        for lo in range(0, len(s), WIG_CHUNK):
            a, b, c = s[lo:lo + WIG_CHUNK], e[lo:lo + WIG_CHUNK], k[lo:lo + WIG_CHUNK]
            text, n = C.c_void_p(), C.c_uint64()
            check(lib.gtars_uniwig_format_bedgraph(chromname.encode(), ptr(a), ptr(b), ptr(c), len(a), C.byref(text), C.byref(n)))
            fh.write(_take_text(text, n))


def write_to_npy_file(counts, filename: str, chromname: str, start_position: int, stepsize: int, metafilename: str) -> None:
    """a version 1.0 ``.npy`` of ``<u4`` and one fixedStep header line appended to the metadata file (writing.rs:13-59)"""
    counts = as_u32(counts)
    _mkparent(metafilename)
    header = "{'descr': '<u4', 'fortran_order': False, 'shape': (%d,), }" % len(counts)
    header += " " * ((64 - (10 + len(header) + 1) % 64) % 64) + "\n"
    with open(filename, "wb") as fh:
        fh.write(b"\x93NUMPY\x01\x00" + len(header).to_bytes(2, "little") + header.encode("latin1"))
        fh.write(counts.astype("<u4", copy=False).tobytes())
    with open(metafilename, "a") as fh:
        fh.write(f"fixedStep chrom={chromname} start={start_position} step={stepsize}\n")


def write_combined_files(location: str, output_type: str, prefix: str, chromosomes: Sequence[Chromosome]) -> None:
    """the per-chromosome files appended to ``{prefix}_{location}.{ext}`` in chromosome order and deleted
    (writing.rs:63-110)"""
    combined = f"{prefix}_{location}.{output_type}"
    _mkparent(combined)
    with open(combined, "ab") as out:
        inputs = [f for f in (f"{prefix}{c.chrom}_{location}.{output_type}" for c in chromosomes) if os.path.exists(f)]
        for f in inputs:
            with open(f, "rb") as fh:
                while True:
                    block = fh.read(1 << 24)
                    if not block:
                        break
                    out.write(block)
            os.remove(f)


def uniwig(bed: str, chrom_sizes: str, smoothsize: int, stepsize: int = 1, count_types: Sequence[str] = ("start", "end", "core"),
           output_prefix: str = "", output_type: str = "wig", wig_variable: bool = False, score: bool = False) -> List[str]:
    """uniwig_main (lib.rs:50-581) for one BED file: the same files under the same names.  -> the chromosomes processed.

    * chromosomes the sizes file does not name are dropped (get_final_chromosomes, utils.rs:252-281);
    * ``smoothsize == 0``: lib.rs:135 counts and writes nothing per chromosome, so the combined wig / bedGraph files come out
      empty and the npy metadata holds the sizes only -- mirrored as it is;
    * start positions per track and format as at each call site: wig ``max(1, p0 - m)`` for start and end, ``max(1, s0)``
      for core (lib.rs:163-183, 289-309, 397-406); bedGraph and npy ``max(0, p0 - m)`` for start, ``max(1, e0 - m)`` for end,
      ``s0`` for core (lib.rs:194-197, 215-218, 266-270, 322-326, 375-378, 421-424);
    * count types other than start / end / core are skipped (lib.rs:449);
    * npy: ``{prefix}{chrom}_{type}.npy`` and ``{prefix}npy_meta.json`` (lib.rs:476-532; the reference's key order in that
      file is a HashMap's, here the keys are in processing order).
    """
    _domain(stepsize, score)
    smoothsize = int(smoothsize)
    if output_type in ("bw", "bigwig", "bigWig"):
        raise ValueError("bigWig output is not provided (gtars_amd.uniwig): write bedGraph")
    if output_type == "bedgraph":
        output_type = "bedGraph"  # lib.rs:110-112
    if output_type not in ("wig", "bedGraph", "npy"):
        raise ValueError(f"unknown output type {output_type!r}: wig, bedGraph or npy")
    sizes = read_chromosome_sizes(chrom_sizes)
    final = [c for c in read_chromosomes(bed) if c.chrom in sizes]
    prefix = str(output_prefix)
    for c in final:
        size = sizes[c.chrom]
        p0, e0 = int(c.starts[0]), int(c.ends[0])
        for kind in count_types:
            if smoothsize == 0 or kind not in KINDS:
                continue
            opens, closes, m = (c.ends, None, smoothsize) if kind == "end" else (c.starts, c.ends if kind == "core" else None,
                                                                                 smoothsize if kind == "start" else 0)
            lead = e0 if kind == "end" else p0
            file_name = f"{prefix}{c.chrom}_{kind}.{output_type}"
            if output_type == "wig":
                wig_start = max(1, lead - m)
                if wig_variable:
                    pos, cnt = nonzero_counts(kind, opens, closes, size, m, wig_start)
                    write_to_wig_file_variable(pos, cnt, file_name, c.chrom)
                else:
                    counts, _ = _track(kind, opens, closes, size, m)
                    write_to_wig_file(counts, file_name, c.chrom, wig_start, stepsize, size)
            else:
                start_position = max(1, lead - m) if kind == "end" else max(0, lead - m)
                if output_type == "bedGraph":
                    write_to_bed_graph_file(compress_counts(kind, opens, closes, size, m, start_position), file_name, c.chrom)
                else:
                    counts, _ = _track(kind, opens, closes, size, m)
                    write_to_npy_file(counts, file_name, c.chrom, start_position, stepsize, f"{prefix}{kind}.meta")
    if output_type in ("wig", "bedGraph"):
        for kind in count_types:
            write_combined_files(kind, output_type, prefix, final)
    else:
        meta: Dict[str, Dict[str, int]] = {c.chrom: {"stepsize": stepsize, "reported_chrom_size": sizes[c.chrom]} for c in final}
        for kind in count_types:
            temp = f"{prefix}{kind}.meta"
            if os.path.exists(temp):
                with open(temp) as fh:
                    for line in fh.read().splitlines():
                        parts = line.split()
                        if len(parts) >= 3 and parts[1].split("=")[1] in meta:
                            meta[parts[1].split("=")[1]][kind] = int(parts[2].split("=")[1])
                os.remove(temp)
        with open(f"{prefix}npy_meta.json", "w") as fh:
            fh.write(json.dumps(meta, indent=2))
    return [c.chrom for c in final]


# ---- the streaming uniwig (stream.rs; K24) -------------------------------------------------------------------------------
class CountType(enum.Enum):
    """stream.rs:16-21"""
    Start = "start"
    End = "end"
    Core = "core"


class OutputFormat(enum.Enum):
    """stream.rs:23-27"""
    Wig = "wig"
    BedGraph = "bedgraph"


I32_MAX = (1 << 31) - 1
STREAM_TEXT_CHUNK = 1 << 20  # values formatted per call of the C++ writers


def _count_type(count_type) -> CountType:
    if isinstance(count_type, CountType):
        return count_type
    try:
        return CountType(str(count_type).lower())
    except ValueError:
        raise ValueError(f"unknown count type {count_type!r}: start, end or core") from None


def _output_format(output_format) -> OutputFormat:
    if isinstance(output_format, OutputFormat):
        return output_format
    key = str(output_format).lower()
    if key in ("bedgraph", "bg"):
        return OutputFormat.BedGraph
    if key == "wig":
        return OutputFormat.Wig
    raise ValueError(f"unknown output format {output_format!r}: wig or bedgraph")


def _read_all(src) -> bytes:
    """a path, bytes, or a binary file object -> its bytes"""
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src)
    if isinstance(src, (str, os.PathLike)):
        with open(src, "rb") as fh:
            return fh.read()
    data = src.read()
    if isinstance(data, str):
        raise TypeError("the input must be a binary file object")
    return data


def read_chrom_sizes(source) -> Dict[str, int]:
    """read_chrom_sizes (stream.rs:473-495) of a path, bytes or a binary file object: ``name<TAB>size`` per line, split on
    TABS only, ``#`` and blank lines skipped, the size a u32; a name that comes again overwrites.  Not
    ``read_chromosome_sizes``, which is the batch path's reader."""
    text = _read_all(source).decode("utf-8")
    sizes: Dict[str, int] = {}
    for line in text.split("\n"):
        if line.endswith("\r"):
            line = line[:-1]
        trimmed = line.strip(_RUST_WS)
        if not trimmed or trimmed.startswith("#"):
            continue
        fields = trimmed.split("\t")
        if len(fields) < 2:
            raise ValueError(f"chrom.sizes line has fewer than 2 fields: '{trimmed}'")
        digits = fields[1][1:] if fields[1][:1] == "+" else fields[1]
        if fields[1] == "":
            raise ValueError(f"Cannot parse size '{fields[1]}': cannot parse integer from empty string")
        if not digits or any(c not in "0123456789" for c in digits):
            raise ValueError(f"Cannot parse size '{fields[1]}': invalid digit found in string")
        if int(digits) > 0xFFFFFFFF:
            raise ValueError(f"Cannot parse size '{fields[1]}': number too large to fit in target type")
        sizes[fields[0]] = int(digits)
    return sizes


# char::is_whitespace
_RUST_WS = ("\t\n\x0b\x0c\r \x85\xa0\u1680\u2000\u2001\u2002\u2003\u2004\u2005\u2006\u2007\u2008\u2009\u200a\u2028\u2029"
            "\u202f\u205f\u3000")


def parse_stream_bed(source) -> Tuple[List[str], np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """the rows of a BED file as the streaming processor reads them (parse_bed_line, stream.rs:57-112; the C++ parser of
    csrc/uniwig_stream_parse.h): a path, bytes or a binary file object, plain or gzip (first member only) ->
    (chromosome names in first-seen order, chromosome id, start i32, end i32, score u32 per row).  ValueError with the
    reference's message for a bad line; no row is returned then."""
    h = C.c_void_p()
    if isinstance(source, (str, os.PathLike)):
        check(lib.gtars_uniwig_stream_parse(os.fspath(source).encode(), None, 0, C.byref(h)))
    else:
        data = _read_all(source)
        check(lib.gtars_uniwig_stream_parse(None, data, len(data), C.byref(h)))
    try:
        n = int(lib.gtars_uniwig_rows_len(h))
        names = [lib.gtars_uniwig_rows_chrom_name(h, i).decode("utf-8") for i in range(lib.gtars_uniwig_rows_n_chrom(h))]
        cols = [C.c_void_p() for _ in range(4)]
        check(lib.gtars_uniwig_rows_columns(h, *[C.byref(c) for c in cols]))
        out = []
        for c, (ct, dt) in zip(cols, ((C.c_uint32, np.uint32), (C.c_int32, np.int32), (C.c_int32, np.int32), (C.c_uint32, np.uint32))):
            out.append(np.ctypeslib.as_array(C.cast(c, C.POINTER(ct)), shape=(n,)).astype(dt, copy=True) if n else np.zeros(0, dtype=dt))
        return (names, *out)
    finally:
        lib.gtars_uniwig_rows_free(h)


class StreamTrack:
    """What the streaming processor emits for one file and one count type.

    ``chroms``: chromosome names, first-seen order.  ``seg_chrom`` / ``seg_first`` / ``seg_len``: the segments in output
    order -- index into ``chroms``, first position (1-based) and number of positions at step 1; a segment is a stretch of
    consecutive positions of one chromosome run.  ``counts``: the u32 counts of the KEPT positions
    (``(pos - 1) % step == 0``), segment after segment."""

    __slots__ = ("chroms", "seg_chrom", "seg_first", "seg_len", "counts", "step")

    def __init__(self, chroms, seg_chrom, seg_first, seg_len, counts, step):
        self.chroms, self.seg_chrom, self.seg_first, self.seg_len, self.counts, self.step = chroms, seg_chrom, seg_first, seg_len, counts, step

    def __repr__(self):
        return f"StreamTrack(segments={len(self.seg_first)}, counts={len(self.counts)}, step={self.step})"

    def segment_slices(self) -> Iterator[Tuple[str, int, int, int]]:
        """(chrom, first kept position, lo, hi): ``counts[lo:hi]`` are the segment's kept positions, ``step`` apart"""
        lo = 0
        st = self.step
        for c, f, ln in zip(self.seg_chrom.tolist(), self.seg_first.tolist(), self.seg_len.tolist()):
            q0 = (f - 1 + st - 1) // st
            q1 = (f + ln - 2) // st
            k = max(q1 - q0 + 1, 0)
            if k:
                yield self.chroms[c], q0 * st + 1, lo, lo + k
            lo += k

    def records(self) -> Iterator[Tuple[str, int, int]]:
        """(chrom, position, count) as the reference's CountRecords, in its order"""
        for chrom, first, lo, hi in self.segment_slices():
            for k, v in enumerate(self.counts[lo:hi].tolist()):
                yield chrom, first + k * self.step, v


def _stream_columns(bed_or_columns):
    if isinstance(bed_or_columns, (tuple, list)) and len(bed_or_columns) in (3, 4) and not isinstance(bed_or_columns[0], (str, bytes)):
        chroms, start, end = bed_or_columns[:3]
        if isinstance(chroms, tuple) and len(chroms) == 2 and isinstance(chroms[1], np.ndarray):
            names, cid = [str(c) for c in chroms[0]], as_u32(chroms[1])  # (names, index into them per row)
            if len(cid) and int(cid.max()) >= len(names):
                raise ValueError("a chromosome index is not below the number of names")
        else:
            ids: Dict[str, int] = {}
            cid = np.fromiter((ids.setdefault(str(c), len(ids)) for c in chroms), dtype=np.uint32, count=len(chroms))
            names = list(ids)
        start, end = np.asarray(start, dtype=np.int64), np.asarray(end, dtype=np.int64)
        score = np.ones(len(cid), dtype=np.int64) if len(bed_or_columns) == 3 else np.asarray(bed_or_columns[3], dtype=np.int64)
        if not (len(start) == len(end) == len(score) == len(cid)):
            raise ValueError("the columns must have the same length")
        score = np.maximum(score, 0)  # (negative scores count 0, stream.rs:101)
        return names, cid, start, end, score
    names, cid, start, end, score = parse_stream_bed(bed_or_columns)
    return names, cid, start.astype(np.int64), end.astype(np.int64), score.astype(np.int64)


def _stream_args(smooth_size: int, step_size: int, max_gap: int):
    smooth_size, step_size, max_gap = int(smooth_size), int(step_size), int(max_gap)
    if not 0 <= smooth_size <= 0x3FFFFFFF:
        raise ValueError(f"smooth size {smooth_size} is out of range")
    if not -I32_MAX <= step_size <= I32_MAX:
        raise ValueError(f"step size {step_size} is out of range")
    step = abs(step_size) if abs(step_size) > 1 else 1  # (stream.rs:274: step <= 1 keeps all; % truncates, so the sign is immaterial)
    if not -(1 << 63) <= max_gap < (1 << 63):
        raise ValueError(f"max_gap {max_gap} does not fit an i64")
    return smooth_size, step, max_gap


def _checked_rows(cid, start, end, score, smooth_size: int):
    """the rules of the issue: 0 <= start, 0 <= end, end + m + 1 <= 2^31 - 1 (and the same for start); names the first row"""
    limit = I32_MAX - smooth_size - 1
    bad = (start < 0) | (end < 0) | (start > limit) | (end > limit) | (score > I32_MAX)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f"uniwig stream: row {i} (start {int(start[i])}, end {int(end[i])}, score {int(score[i])}) is out of range: "
                         f"0 <= start, 0 <= end, end + smooth_size + 1 <= 2^31 - 1 and score <= 2^31 - 1 are required")
    return as_u32(cid), start.astype(np.uint32), end.astype(np.uint32), score.astype(np.uint32)


def _sizes_by_id(names: Sequence[str], chrom_sizes) -> np.ndarray:
    if chrom_sizes is None:
        chrom_sizes = {}
    elif not isinstance(chrom_sizes, dict):
        chrom_sizes = read_chrom_sizes(chrom_sizes)
    # `chrom_size as i32 + 1` (stream.rs:349) is not positive from 2^31 - 1 on: such a size extends nothing, like no size
    return np.fromiter((s if 0 < (s := int(chrom_sizes.get(nme, 0))) < I32_MAX else 0 for nme in names), dtype=np.uint32,
                       count=len(names))


def stream_counts(bed_or_columns, chrom_sizes=None, smooth_size: int = 0, step_size: int = 1, count_type="start", max_gap: int = 0,
                  max_device_bytes: int = 0) -> StreamTrack:
    """UniwigStreamProcessor (stream.rs:124-382) over a whole file, on the device.

    ``bed_or_columns``: a BED path, bytes or binary file object (plain or gzip), or columns ``(chroms, starts, ends[,
    scores])`` with one chromosome NAME per row -- or ``chroms = (names, ndarray of indices into names)`` -- rows in file
    order (no order is required).  ``chrom_sizes``: a dict, a
    chrom.sizes path / bytes / file object, or None; it matters only with ``max_gap < 0``.  ``max_gap``: 0 sparse, N > 0
    fills gaps of at most N positions with zeros, -1 fully dense (from position 1 to the chromosome's size).  Counts past
    2^32 - 1 wrap (the reference's release build).  ``max_device_bytes``: the counts leave the device in pieces of at
    most that many bytes (0: the library's default).  ValueError for rows outside the reference's i32 arithmetic."""
    ct = _count_type(count_type)
    smooth_size, step, max_gap = _stream_args(smooth_size, step_size, max_gap)
    names, cid, start, end, score = _stream_columns(bed_or_columns)
    cid, start, end, score = _checked_rows(cid, start, end, score, smooth_size)
    sizes = _sizes_by_id(names, chrom_sizes)
    sc, sf, sl, cnt = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    n_seg, n_cnt = C.c_uint64(), C.c_uint64()
    check(lib.gtars_uniwig_stream(ptr(cid), ptr(start), ptr(end), ptr(score), len(cid), ptr(sizes), len(sizes), smooth_size, step,
                                  KINDS[ct.value], max_gap, int(max_device_bytes), C.byref(sc), C.byref(sf), C.byref(sl), C.byref(n_seg),
                                  C.byref(cnt), C.byref(n_cnt)))
    return StreamTrack(names, take_u32(sc, n_seg.value), take_u32(sf, n_seg.value), take_u32(sl, n_seg.value), take_u32(cnt, n_cnt.value),
                       step)


class StreamPlan:
    """The plan of device-resident rows: the segment table on the host, the event columns on the device.
    ``seg_chrom`` (chromosome ID), ``seg_first``, ``seg_len`` and ``seg_off`` (n + 1 offsets into the compacted counts, the
    last one their total) keep segments of length 0.  ``counts_device`` queues one window of the step-1 counts."""

    def __init__(self, d_cid: int, d_start: int, d_end: int, d_score: int, n: int, sizes_by_id=None, smooth_size: int = 0,
                 count_type="start", max_gap: int = 0):
        ct = _count_type(count_type)
        smooth_size, _, max_gap = _stream_args(smooth_size, 1, max_gap)
        sizes = as_u32(sizes_by_id if sizes_by_id is not None else [])
        self._h = C.c_void_p()
        check(lib.gtars_uniwig_stream_plan_device(C.c_void_p(d_cid), C.c_void_p(d_start), C.c_void_p(d_end), C.c_void_p(d_score), int(n),
                                                  ptr(sizes), len(sizes), smooth_size, KINDS[ct.value], max_gap, C.byref(self._h)))
        k = int(lib.gtars_uniwig_plan_segments(self._h))
        self.total = int(lib.gtars_uniwig_plan_total(self._h))
        self.seg_chrom, self.seg_first, self.seg_len = (np.zeros(k, dtype=np.uint32) for _ in range(3))
        self.seg_off = np.zeros(k + 1, dtype=np.uint64)
        check(lib.gtars_uniwig_plan_table(self._h, ptr(self.seg_chrom), ptr(self.seg_first), ptr(self.seg_len), ptr(self.seg_off)))

    def counts_device(self, window_first: int, window_len: int, d_counts: int, stream: int = 0) -> None:
        """compacted positions ``window_first .. window_first + window_len - 1`` into device memory (16-byte aligned),
        queued on ``stream``"""
        check(lib.gtars_uniwig_stream_device(self._h, int(window_first), int(window_len), C.c_void_p(d_counts), C.c_void_p(stream or 0)))

    def close(self) -> None:
        if self._h:
            lib.gtars_uniwig_plan_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        self.close()


class _WigState:
    """WigWriter (stream.rs:389-438): a header whenever the chromosome changes or ``position != last + 1``; the text says
    ``step=1`` whatever the step is"""

    def __init__(self):
        self.chrom: Optional[str] = None
        self.last: Optional[int] = None

    def need_header(self, chrom: str, position: int) -> bool:
        return self.chrom is None or self.chrom != chrom or self.last is None or position != self.last + 1


def _write_track(track: StreamTrack, out, fmt: OutputFormat) -> None:
    wig = _WigState()
    for chrom, first, lo, hi in track.segment_slices():
        if fmt is OutputFormat.BedGraph:
            for a in range(lo, hi, STREAM_TEXT_CHUNK):
                part = track.counts[a:min(hi, a + STREAM_TEXT_CHUNK)]
                text, n = C.c_void_p(), C.c_uint64()
                check(lib.gtars_uniwig_format_bedgraph_bases(chrom.encode(), first + (a - lo) * track.step, track.step, ptr(part),
                                                             len(part), C.byref(text), C.byref(n)))
                out.write(_take_text(text, n))
        elif track.step == 1:
            if wig.need_header(chrom, first):
                out.write(f"fixedStep chrom={chrom} start={first} step=1\n".encode())
            for a in range(lo, hi, STREAM_TEXT_CHUNK):
                part = track.counts[a:min(hi, a + STREAM_TEXT_CHUNK)]
                text, n = C.c_void_p(), C.c_uint64()
                check(lib.gtars_uniwig_format_counts(ptr(part), len(part), C.byref(text), C.byref(n)))
                out.write(_take_text(text, n))
            wig.chrom, wig.last = chrom, first + (hi - lo) - 1
        else:
            # kept positions are `step` apart, so every value gets its header (a position is never its predecessor + 1)
            head = f"fixedStep chrom={chrom} start=".encode()
            for a in range(lo, hi, STREAM_TEXT_CHUNK):
                b = min(hi, a + STREAM_TEXT_CHUNK)
                pos = first + (a - lo) * track.step
                out.write(b"".join(head + b"%d step=1\n%d\n" % (pos + k * track.step, v) for k, v in enumerate(track.counts[a:b].tolist())))
            wig.chrom, wig.last = chrom, first + (hi - lo - 1) * track.step


def write_records_as_wig(out, records) -> None:
    """write_records_as_wig (stream.rs:442-447): ``(chrom, position, count)`` records as fixedStep wig into a binary file
    object"""
    wig = _WigState()
    for chrom, position, count in records:
        if wig.need_header(chrom, position):
            out.write(f"fixedStep chrom={chrom} start={position} step=1\n".encode())
            wig.chrom = chrom
        out.write(b"%d\n" % count)
        wig.last = position


def write_records_as_bedgraph(out, records) -> None:
    """write_records_as_bedgraph (stream.rs:450-466): ``chrom<TAB>pos-1<TAB>pos<TAB>count`` per record"""
    for chrom, position, count in records:
        out.write(f"{chrom}\t{position - 1}\t{position}\t{count}\n".encode())


def uniwig_streaming(input, output, chrom_sizes=None, smooth_size: int = 0, step_size: int = 1, count_type="start",
                     output_format="wig", max_gap: int = 0, max_device_bytes: int = 0) -> StreamTrack:
    """uniwig_streaming (stream.rs:548-596): ``input`` is a BED path, bytes or a binary file object, plain or gzip;
    ``output`` a path (created or truncated) or a binary file object.  The whole input is parsed and counted before the
    first byte is written: a bad line fails the call and nothing is written (the reference has written the lines in front
    of it by then).  -> the track that was written."""
    fmt = _output_format(output_format)
    track = stream_counts(input, chrom_sizes, smooth_size, step_size, count_type, max_gap, max_device_bytes)
    if isinstance(output, (str, os.PathLike)):
        with open(output, "wb") as fh:
            _write_track(track, fh, fmt)
    else:
        _write_track(track, output, fmt)
    return track
