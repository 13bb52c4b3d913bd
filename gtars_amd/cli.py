"""Text front ends of the two CLI commands that sit directly on the hot path:

  python -m gtars_amd overlaprs --universe U.bed[.gz] --query Q.bed[.gz] [--backend bits|ailist]
      gtars-cli/src/overlaprs/handlers.rs:21-157: one line  chr<TAB>hit.start<TAB>hit.end  per hit, queries in file
      order, hits in the backend's find order (Bits: stored order; AIList: sub-list major, descending), queries on
      chromosomes the universe does not have are skipped.
  python -m gtars_amd igd create --output DIR --filelist DIR|list.txt|- [--dbname igd_database]
  python -m gtars_amd igd search --database DB.igd --query Q.bed[.gz]
      gtars-cli/src/igd/handlers.rs:11-98: the legacy TSV  index / number of regions / number of hits / File_name  for
      the files with hits, then  Total: N.
  python -m gtars_amd uniwig --file F.bed[.gz] --chromref G.chrom.sizes --smoothsize M --stepsize 1 --fileheader PREFIX
                             [--outputtype wig|bedGraph|npy] [--counttype all|start|end|core] [--wigstep fixed|variable]
      gtars-cli/src/uniwig/cli.rs:38-178, handlers.rs:48-160 for BED input: the coverage tracks of gtars_amd.uniwig.  BAM
      input (--filetype bam) and bigWig output (--outputtype bw) are not provided and exit with a message.
  python -m gtars_amd uniwig --streaming [--file F.bed[.gz]|-] [--chromref G.chrom.sizes] --smoothsize M --stepsize S
                             [--counttype start|end|core|all] [--outputtype wig|bedgraph|bg] [--dense N] [--stdout]
                             [--fileheader PREFIX]
      gtars-cli/src/uniwig/handlers.rs:162-274: the streaming uniwig of gtars_amd.uniwig (scores, sparse output, gap
      filling, any step).  Input from a file or stdin, output to PREFIX_{start,end,core}.wig|bedgraph or stdout.
  python -m gtars_amd uniwig bamqc --input X.bam --output Y.tsv [--threads N]
      gtars-cli/src/uniwig/cli.rs, gtars-uniwig/src/bamqc.rs: the library-complexity QC of a coordinate-sorted BAM as a TSV.
  python -m gtars_amd bam fragments --bam X.bam --output Y.tsv[.gz] [--barcode-tag CB | --no-barcode NAME] [--min-mapq N]
                                    [--max-length N] [--shift A,B]
      this library's own: the deduplicated fragments of a coordinate-sorted paired-end BAM as a
      10x-style fragment file; prints the statistics as key<TAB>value lines.

Same rules as the reference: fields are split on TAB only, coordinates must parse as u32 (``+5`` is accepted, blanks and
signs are not), every line counts (no header skipping in overlaprs).  The whole query file is ONE batch on the device.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Sequence, TextIO, Tuple

import numpy as np

from ._lib import KIND_AILIST, KIND_BITS, UNKNOWN_CHROM


def read_bed3_lines(path: str) -> Tuple[List[str], np.ndarray, np.ndarray, np.ndarray]:
    """chr / start / end of EVERY line, in file order (handlers.rs:64-92, 123-139), through the C++ chunked reader
    (gtars_bed3_lines_read): -> (chromosome names in first-seen order, chromosome id per line, starts, ends)."""
    import ctypes as C

    from . import _lib

    h = C.c_void_p()
    if _lib.lib.gtars_bed3_lines_read(str(path).encode(), C.byref(h)) != 0:
        raise ValueError(_lib.last_error())
    try:
        n = int(_lib.lib.gtars_fragments_len(h))

        def col(fn):
            if not n:
                return np.zeros(0, dtype=np.uint32)
            return np.ctypeslib.as_array(C.cast(fn(h), C.POINTER(C.c_uint32)), shape=(n,)).copy()

        names = [_lib.lib.gtars_fragments_chrom_name(h, i).decode() for i in range(_lib.lib.gtars_fragments_n_chrom(h))]
        return names, col(_lib.lib.gtars_fragments_chrom_ids), col(_lib.lib.gtars_fragments_starts), col(_lib.lib.gtars_fragments_ends)
    finally:
        _lib.lib.gtars_fragments_free(h)


HIT_CHUNK = 1 << 20  # hit lines formatted per call of the C++ writer


def run_overlaprs(universe: str, query: str, backend: str = "bits", out: TextIO = sys.stdout) -> int:
    """-> number of hit lines written.  Text in and out go through the C++ host layer (chunked in-place parse, hit lines formatted
    and written a million at a time); the whole query file is one device batch in between -- so a malformed line anywhere in the
    query file fails the run BEFORE any hit line is written (the reference streams line by line, handlers.rs:114-155, and has
    written the hits of the lines in front of the bad one: INTEGRATION.md)."""
    import ctypes as C

    from . import _lib
    from .engine import OverlapIndex

    if backend not in ("bits", "ailist"):
        raise ValueError(f"Invalid backend type: {backend}. Valid options are 'bits' or 'ailist'")
    names, cid, us, ue = read_bed3_lines(universe)
    ix = OverlapIndex(cid, us, ue, None, n_chrom=len(names), kind=KIND_AILIST if backend == "ailist" else KIND_BITS)
    q_names, q_cid, qs, qe = read_bed3_lines(query)
    # the query file's chromosome ids -> the universe's (chromosomes the universe does not have are skipped)
    uid = {nme: i for i, nme in enumerate(names)}
    relabel = np.fromiter((uid.get(nme, UNKNOWN_CHROM) for nme in q_names), dtype=np.uint32, count=len(q_names))
    qc = relabel[q_cid] if len(q_cid) else np.zeros(0, dtype=np.uint32)
    offsets, hs, he, _ = ix.find_overlaps(qc, qs, qe)
    n = int(len(hs))
    if n:
        # formatted and written in chunks of HIT_CHUNK hits (one C++ buffer and one bytes object per chunk, straight to the
        # stream's binary layer when it has one): a 1e9-hit run needs tens of MB of text in flight, not tens of GB
        counts = np.diff(offsets.astype(np.int64))
        arr = (C.c_char_p * len(names))(*[nme.encode() for nme in names])
        hs, he = np.ascontiguousarray(hs), np.ascontiguousarray(he)
        sink = getattr(out, "buffer", None)
        if sink is not None:
            out.flush()
        q_lo = 0
        for lo in range(0, n, HIT_CHUNK):
            hi = min(n, lo + HIT_CHUNK)
            # the queries whose hits [lo, hi) belong to: offsets is their CSR
            q_hi = int(np.searchsorted(offsets, hi, side="left"))
            q_first = max(int(np.searchsorted(offsets, lo, side="right")) - 1, 0)
            rep = counts[q_first:q_hi].copy()
            rep[0] -= lo - int(offsets[q_first])
            rep[-1] -= int(offsets[q_hi]) - hi
            hit_chrom = np.ascontiguousarray(np.repeat(qc[q_first:q_hi], rep), dtype=np.uint32)
            text, ln = C.c_void_p(), C.c_uint64()
            _lib.check(_lib.lib.gtars_format_hit_lines(C.cast(arr, C.c_void_p), _lib.ptr(hit_chrom), _lib.ptr(hs[lo:hi]), _lib.ptr(he[lo:hi]),
                                                       hi - lo, C.byref(text), C.byref(ln)))
            try:
                data = C.string_at(text, ln.value)
            finally:
                _lib.lib.gtars_free(text)
            if sink is not None:
                sink.write(data)
            else:
                out.write(data.decode())
            q_lo = q_hi
        if sink is not None:
            sink.flush()
    return n


def resolve_bed_paths(filelist: str, stdin: TextIO = sys.stdin) -> List[str]:
    """handlers.rs:17-52: a .txt list, "-" / "stdin", or a directory of .bed / .gz files (sorted)."""
    if filelist.endswith(".txt"):
        with open(filelist) as fh:
            return [p.strip() for p in fh if p.strip()]
    if filelist in ("-", "stdin"):
        return [p.strip() for p in stdin if p.strip()]
    paths = [os.path.join(filelist, n) for n in os.listdir(filelist)
             if n.rsplit(".", 1)[-1] in ("bed", "gz") and "." in n and os.path.isfile(os.path.join(filelist, n))]
    return sorted(paths)


def run_igd_create(output: str, filelist: str, dbname: str = "igd_database", stdin: TextIO = sys.stdin) -> str:
    from .igd import Igd

    db = Igd.from_bed_files(resolve_bed_paths(filelist, stdin))
    path = os.path.join(output, f"{dbname}.igd")
    db.save(path)
    return path


def run_igd_search(database: str, query: str, out: TextIO = sys.stdout) -> int:
    """-> total number of hits."""
    from .igd import Igd
    from .models import RegionSet

    db = Igd.from_igd_file(database)
    hits = db.count_set_overlaps(RegionSet(query), 1)
    out.write("index\t number of regions\t number of hits\t File_name\n")
    for i, fi in enumerate(db.file_info):
        if int(hits[i]) > 0:
            out.write(f"{i}\t{fi.num_regions}\t{int(hits[i])}\t{fi.filename}\n")
    total = int(np.asarray(hits, dtype=np.uint64).sum())
    out.write(f"Total: {total}\n")
    return total


COUNT_TYPES = {"start": ("start",), "end": ("end",), "core": ("core",)}  # anything else: all three (handlers.rs:93-113)


def run_uniwig(a) -> int:
    """handlers.rs:48-160 for the BED path.  -> exit status"""
    if a.filetype.lower() == "bam":
        sys.stderr.write("uniwig: --filetype bam is not provided by gtars_amd (BED and narrowPeak input only)\n")
        return 2
    if a.outputtype in ("bw", "bigwig", "bigWig"):
        sys.stderr.write("uniwig: --outputtype bw is not provided by gtars_amd (write bedGraph and convert it)\n")
        return 2
    if a.filetype.lower() not in ("bed", "narrowpeak"):
        sys.stderr.write(f"uniwig: unknown file type {a.filetype!r}\n")
        return 2
    if a.counttype == "shift":
        sys.stderr.write("uniwig: --counttype shift belongs to the BAM workflow, which is not provided by gtars_amd\n")
        return 2
    from .uniwig import uniwig

    uniwig(a.file, a.chromref, a.smoothsize, stepsize=a.stepsize, count_types=COUNT_TYPES.get(a.counttype, ("start", "end", "core")),
           output_prefix=a.fileheader, output_type=a.outputtype, wig_variable=a.wigstep == "variable", score=a.score)
    return 0


STREAM_COUNT_TYPES = {"all": ("start", "end", "core"), "start": ("start",), "end": ("end",), "core": ("core",)}


def run_uniwig_streaming(a, stdin=None, stdout=None) -> int:
    """run_uniwig_streaming (handlers.rs:162-274).  -> exit status.  ``stdin`` / ``stdout``: binary file objects (the
    process's own by default)."""
    from .uniwig import read_chrom_sizes, uniwig_streaming

    chrom_sizes = read_chrom_sizes(a.chromref) if a.chromref else {}
    labels = STREAM_COUNT_TYPES.get(a.counttype)
    if labels is None:
        sys.stderr.write(f"Error: unknown count type '{a.counttype}' for streaming mode\n")
        return 1
    if a.smoothsize is None or a.stepsize is None:
        sys.stderr.write("uniwig: --smoothsize and --stepsize are required\n")
        return 2
    if a.outputtype == "wig":
        extension = "wig"
    elif a.outputtype in ("bedgraph", "bg"):
        extension = "bedgraph"
    else:
        sys.stderr.write(f"Error: output type '{a.outputtype}' not supported in streaming mode (use wig or bedgraph)\n")
        return 1
    if not a.stdout and a.fileheader is None:
        sys.stderr.write("uniwig: --fileheader required for file output in streaming mode\n")
        return 2
    if a.file is None or a.file == "-":
        # read once, whatever the number of count types (the reference buffers stdin only when there are several)
        source = (stdin if stdin is not None else sys.stdin.buffer).read()
    else:
        source = a.file
    sink = stdout if stdout is not None else getattr(sys.stdout, "buffer", sys.stdout)
    for label in labels:
        if a.stdout:
            if len(labels) > 1:
                sink.write(f"# count_type={label}\n".encode())
            uniwig_streaming(source, sink, chrom_sizes, a.smoothsize, a.stepsize, label, extension, a.dense)
            sink.flush()
        else:
            uniwig_streaming(source, f"{a.fileheader}_{label}.{extension}", chrom_sizes, a.smoothsize, a.stepsize, label, extension,
                             a.dense)
    return 0


def bamqc_parser() -> argparse.ArgumentParser:
    q = argparse.ArgumentParser(prog="python -m gtars_amd uniwig bamqc", description="Library-complexity QC of a coordinate-sorted BAM file")
    q.add_argument("--input", "-i", required=True, help="Path to the BAM file")
    q.add_argument("--output", "-o", required=True, help="Path of the TSV to write")
    q.add_argument("--threads", "-t", type=int, default=1, help="Host threads that inflate")
    return q


def bam_fragments_parser() -> argparse.ArgumentParser:
    q = argparse.ArgumentParser(prog="python -m gtars_amd bam fragments",
                                description="Deduplicated fragments (chrom, start, end, barcode, count) of a coordinate-sorted paired-end BAM file")
    q.add_argument("--bam", required=True, help="Path to the BAM file")
    q.add_argument("--output", "-o", required=True, help="Path of the fragment file to write (.gz: one gzip member)")
    g = q.add_mutually_exclusive_group()
    g.add_argument("--barcode-tag", default="CB", help="Aux tag (type Z) that holds the cell barcode (default CB)")
    g.add_argument("--no-barcode", metavar="NAME", help="Read no tag: every pair belongs to the sample NAME")
    q.add_argument("--min-mapq", type=int, default=30)
    q.add_argument("--max-length", type=int, default=2000, help="Longest template length kept")
    q.add_argument("--shift", default="4,-5", help="Tn5 shift of the two ends, A,B (default 4,-5)")
    q.add_argument("--threads", "-t", type=int, default=0, help="Host threads that inflate (0: the library's budget)")
    return q


def run_bam_fragments(a, out: TextIO = None) -> int:
    from .bam import bam_to_fragments

    out = sys.stdout if out is None else out
    try:
        shift = tuple(int(x) for x in a.shift.split(","))
        if len(shift) != 2:
            raise ValueError
    except ValueError:
        sys.stderr.write(f"bam fragments: --shift takes two integers A,B, not {a.shift!r}\n")
        return 2
    kw = dict(barcode_tag=None, sample=a.no_barcode) if a.no_barcode is not None else dict(barcode_tag=a.barcode_tag)
    stats = bam_to_fragments(a.bam, a.output, threads=a.threads, min_mapq=a.min_mapq, max_fragment_length=a.max_length, shift=shift, **kw)
    for k, v in stats.items():
        out.write(f"{k}\t{v}\n")
    return 0


def main(argv: Sequence[str] = None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if argv[:2] == ["bam", "fragments"]:
        return run_bam_fragments(bam_fragments_parser().parse_args(argv[2:]))
    # `uniwig bamqc` is a command of its own under uniwig: uniwig's own options are all required, so it cannot be one of them
    if argv[:2] == ["uniwig", "bamqc"]:
        a = bamqc_parser().parse_args(argv[2:])
        from .bam import run_bam_qc

        run_bam_qc(a.input, a.output, a.threads)
        return 0
    ap = argparse.ArgumentParser(prog="python -m gtars_amd", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    o = sub.add_parser("overlaprs", help="Find overlaps between a query file and a universe file")
    o.add_argument("--query", "-q", required=True)
    o.add_argument("--universe", "-u", required=True)
    o.add_argument("--backend", "-b", default="bits")
    g = sub.add_parser("igd", help="Create or search an integrated genome database (IGD)")
    gs = g.add_subparsers(dest="igd_cmd", required=True)
    c = gs.add_parser("create")
    c.add_argument("--output", required=True)
    c.add_argument("--filelist", required=True)
    c.add_argument("--dbname", default="igd_database")
    s = gs.add_parser("search")
    s.add_argument("--database", "-d", required=True)
    s.add_argument("--query", "-q", required=True)
    w = sub.add_parser("uniwig", help="Create accumulation files from a BED file")
    w.add_argument("--file", "-f", help="Path to the combined bed file we want to transform ('-' or absent with --streaming: stdin)")
    w.add_argument("--filetype", "-t", default="bed", help="Input file type, 'bed' or 'narrowpeak'")
    w.add_argument("--chromref", "-c", help="Path to chromreference (optional with --streaming)")
    w.add_argument("--smoothsize", "-m", type=int, help="Integer value for smoothing")
    w.add_argument("--stepsize", "-s", type=int, help="Integer value for stepsize")
    w.add_argument("--fileheader", "-l", help="Name of the file")
    w.add_argument("--outputtype", "-y", default="wig", help="Output as wig, bedGraph or npy")
    w.add_argument("--counttype", "-u", default="all", help="Select to only output start, end, or core. Defaults to all.")
    w.add_argument("--score", "-o", action="store_true", help="Count via score (not provided)")
    w.add_argument("--wigstep", "-w", default="fixed", help="'fixed' (every position) or 'variable' (non-zero only)")
    w.add_argument("--streaming", action="store_true", help="Use the streaming processor (scores, sparse output, BED only)")
    w.add_argument("--dense", type=int, default=0,
                   help="Streaming: widest gap to fill with zeros. 0 = sparse, -1 = fully dense, N = fill gaps <= N (default 0)")
    w.add_argument("--stdout", action="store_true", help="Streaming: write to stdout instead of files")
    a = ap.parse_args(argv)
    if a.cmd == "uniwig":
        if a.streaming:
            return run_uniwig_streaming(a)
        # the batch path needs them all, as before the streaming mode made them optional
        missing = [f"--{k}" for k in ("file", "chromref", "smoothsize", "stepsize", "fileheader") if getattr(a, k) is None]
        if missing:
            w.error("the following arguments are required: " + ", ".join(missing))
        return run_uniwig(a)
    if a.cmd == "overlaprs":
        run_overlaprs(a.universe, a.query, a.backend)
    elif a.igd_cmd == "create":
        run_igd_create(a.output, a.filelist, a.dbname)
    else:
        run_igd_search(a.database, a.query)
    return 0
