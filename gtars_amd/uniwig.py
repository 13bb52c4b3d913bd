"""Coverage tracks of a BED file on the device (gtars-uniwig, BED input): ``*_start``, ``*_end`` and ``*_core`` per-base
counts written as wig, bedGraph or npy.  The reference's Python package has no such module; this one lives under
``gtars_amd`` only.

What is computed: with unit scores and step 1 the reference's sweeps (counting.rs:32-290) are

    count(pos) = #{a_i <= pos} - #{e_i <= pos}        pos = a_0 .. max(chrom_size, a_{n-1} - 1)

over sorted window opens ``a`` and closes ``e``: ``a = max(1, p - m)``, ``e = p + m + 1`` for the start and the end track
(``p`` = start + 1 resp. end of the rows, ``m`` = smoothsize), ``a = start + 1``, ``e = end`` for the core track.  Outside
that domain the sweeps' results depend on their queue handling and are no coverage tracks, so ``stepsize != 1``, scored
input and a zero-length row on the core track raise ValueError.  BAM input and bigWig output are not provided.

There is no CPU fallback: without a device every compute call raises NoDeviceError.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Dict, List, Sequence, Tuple

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
