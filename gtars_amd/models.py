"""``gtars.models`` mirror: ``Region``, ``RegionSet`` and ``RegionSetList``.

Signature-compatible with the reference's pyo3 classes
(gtars-python/src/models/region.rs, gtars-python/src/models/region_set.rs:69-478)
for the part of the surface that sits on the overlap hot path: construction
(path / from_regions / from_vectors), iteration, and the overlap operations
``count_overlaps / any_overlaps / find_overlaps / subset_by_overlaps`` which
index ``other`` on the GPU (IndexedRegionSet::new -> AIList by default) and
query ``self``.  BED parsing + sorting is done by the C++ host layer.

The set algebra of region_set.rs:369-494 (reduce / union / setdiff / intersect_all, jaccard / coverage /
overlap_coefficient, closest, cluster) and ``RegionSetList.pairwise_jaccard`` (region_set_list.rs:74-84) run
on the GPU (csrc/setops.hip); results are bit-exact against the reference's semantics, ``closest`` with
one pinned choice the reference leaves open (the walk starts at the first of several ``other`` regions that
share the query's start).

The structural operations and statistics of region_set.rs:288-531 are here too: ``disjoin``, ``gaps``,
``neighbor_distances``, ``nearest_neighbors``, ``distribution`` and ``chromosome_statistics`` (returning
``ChromosomeStatistics``) run on the GPU (csrc/setops.hip, K9); ``trim``, ``promoters``, ``pintersect``, ``concat``,
``widths`` / ``region_widths``, ``mean_region_width`` and ``get_max_end_per_chr`` are elementwise host arithmetic.
``gaps`` pins the order the reference leaves open among names that share a karyotype key (start, then name bytewise).

What names a set and writes it back out is here as well (region_set.rs:240-330, region_set_list.rs:85-98; csrc/bed_text.cpp
and bed_text.hip, K25): ``RegionSet.identifier`` (the BEDbase bed digest, cached), ``file_digest``, ``to_bed``, ``to_bed_gz``
and ``sort``, ``RegionSetList.identifier()`` and the additive batch calls ``RegionSetList.identifiers()`` / ``file_digests()``.
One set is three sequential MD5 streams and stays on the host threads; a list hashes every stream of every set as one lane
of a device kernel (``on_host=True`` keeps it on the host), and ``to_bed`` formats large sets on the device.

The annotation side of the reference's ``gtars.models`` (gtars-python/src/models/{tss_index,gene_model,gda}.rs) is here
too: ``TssIndex`` (distances to the nearest TSS / feature midpoint on the GPU, csrc/annot.hip, K10), ``GeneModel`` and
``GenomicDistAnnotation`` (a GTF read by host threads; genes, exons and the two UTR sets each merged by a strand-aware
reduce on the GPU).  ``PartitionList`` and what classifies against it live in ``gtars.partitions``
(``PartitionList.from_annotation`` stands for ``GenomicDistAnnotation.partition_list``); ``GenomicDistAnnotation.load_bin`` /
``save_bin`` are not provided; ``GenomeAssembly`` / ``BinaryGenomeAssembly`` live
in ``gtars.seqstats`` and ``SignalMatrix`` in ``gtars.signal``.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import KIND_AILIST, check, cstr_array, dec, lib, ptr, take_u32

_U32_MAX = 0xFFFFFFFF


class Region:
    """gtars.models.Region(chr, start, end, rest) -- region.rs:11-17 of gtars-python/src/models."""

    __slots__ = ("chr", "start", "end", "rest")

    def __init__(self, chr: str, start: int, end: int, rest: Optional[str] = None):
        if not (0 <= int(start) <= 0xFFFFFFFF and 0 <= int(end) <= 0xFFFFFFFF):
            raise OverflowError("start/end must fit in u32")
        self.chr = str(chr)
        self.start = int(start)
        self.end = int(end)
        self.rest = rest

    def __repr__(self) -> str:
        return f"Region -> {self.chr} {self.start} {self.end}"

    def __str__(self) -> str:
        return f"{self.chr}\t{self.start}\t{self.end}" + (f"\t{self.rest}" if self.rest is not None else "")

    def __len__(self) -> int:
        return self.end - self.start

    def __eq__(self, other) -> bool:
        if not isinstance(other, Region):
            return NotImplemented
        return self.chr == other.chr and self.start == other.start and self.end == other.end

    def __ne__(self, other) -> bool:
        r = self.__eq__(other)
        return r if r is NotImplemented else not r

    def __hash__(self):
        return hash((self.chr, self.start, self.end, self.rest))


class RegionSet:
    """gtars.models.RegionSet -- a BED file (parsed + sorted by (chr, start)) or an in-memory list."""

    def __init__(self, path):
        p = str(path)
        h = C.c_void_p()
        st = lib.gtars_regionset_from_bed(p.encode(), C.byref(h))
        if st != 0:
            # PyRegionSet::py_new maps every error to RuntimeError (region_set.rs:79-84)
            raise RuntimeError(_lib.last_error())
        self._h = h
        self.path = p
        self._strands: Optional[List[str]] = None
        self._curr = 0

    # -- alternate constructors ------------------------------------------------
    @classmethod
    def _from_handle(cls, h, strands=None) -> "RegionSet":
        self = cls.__new__(cls)
        self._h = h
        self.path = None
        self._strands = strands
        self._curr = 0
        return self

    @classmethod
    def from_regions(cls, regions: Sequence[Region], strands: Optional[Sequence[str]] = None) -> "RegionSet":
        regions = list(regions)
        if strands is not None and len(strands) != len(regions):
            raise ValueError(f"strands length ({len(strands)}) must match regions length ({len(regions)})")
        return cls._from_columns([r.chr for r in regions], [r.start for r in regions], [r.end for r in regions],
                                 [r.rest for r in regions], strands)

    @classmethod
    def from_vectors(cls, chrs: Sequence[str], starts: Sequence[int], ends: Sequence[int],
                     strands: Optional[Sequence[str]] = None) -> "RegionSet":
        if len(starts) != len(chrs) or len(ends) != len(chrs):
            raise ValueError("chrs, starts, and ends must have the same length")
        if strands is not None and len(strands) != len(chrs):
            raise ValueError(f"strands length ({len(strands)}) must match regions length ({len(chrs)})")
        return cls._from_columns(list(chrs), starts, ends, None, strands)

    @classmethod
    def _from_columns(cls, chrs, starts, ends, rest, strands) -> "RegionSet":
        n = len(chrs)
        s = np.ascontiguousarray(starts, dtype=np.uint32)
        e = np.ascontiguousarray(ends, dtype=np.uint32)
        carr, _keep1 = cstr_array(chrs)
        rarr, _keep2 = (cstr_array(rest) if rest is not None else (None, None))
        h = C.c_void_p()
        check(lib.gtars_regionset_from_arrays(C.cast(carr, C.c_void_p), ptr(s), ptr(e),
                                              C.cast(rarr, C.c_void_p) if rarr is not None else None, n, C.byref(h)))
        return cls._from_handle(h, list(strands) if strands is not None else None)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib.gtars_regionset_free(self._h)
                self._h = None
        except Exception:
            pass

    # -- columns -----------------------------------------------------------------
    def __len__(self) -> int:
        return int(lib.gtars_regionset_len(self._h))

    def _col(self, fn) -> np.ndarray:
        n = len(self)
        if n == 0:
            return np.zeros(0, dtype=np.uint32)
        p = fn(self._h)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n,)).copy()

    @property
    def starts(self) -> np.ndarray:
        return self._col(lib.gtars_regionset_starts)

    @property
    def ends(self) -> np.ndarray:
        return self._col(lib.gtars_regionset_ends)

    @property
    def chrom_names(self) -> List[str]:
        return [dec(lib.gtars_regionset_chrom_name(self._h, i)) for i in range(lib.gtars_regionset_n_chrom(self._h))]

    @property
    def chrom_ids(self) -> np.ndarray:
        return self._col(lib.gtars_regionset_chrom_ids)

    @property
    def header(self) -> Optional[str]:
        return dec(lib.gtars_regionset_header(self._h))

    @property
    def strands(self) -> List[str]:
        return list(self._strands) if self._strands is not None else ["*"] * len(self)

    def __getitem__(self, i: int) -> Region:
        n = len(self)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError("Index out of bounds")
        names = self.chrom_names
        c = int(self.chrom_ids[i])
        return Region(names[c], int(self.starts[i]), int(self.ends[i]), dec(lib.gtars_regionset_rest(self._h, i)))

    @property
    def regions(self) -> List[Region]:
        names, ids, s, e = self.chrom_names, self.chrom_ids, self.starts, self.ends
        return [Region(names[int(ids[i])], int(s[i]), int(e[i]), dec(lib.gtars_regionset_rest(self._h, i)))
                for i in range(len(self))]

    def __iter__(self):
        return iter(self.regions)

    def __repr__(self) -> str:
        return f"RegionSet with {len(self)} regions."

    # -- what names the set and writes it back out (gtars-python/src/models/region_set.rs:136-200; csrc/bed_text.cpp, K25) --
    # Rows are taken in the set's order: a set read from a file is sorted by (chr, start), one built from regions or
    # vectors is not until sort() is called.  One set is three sequential MD5 streams: these run on the host threads.
    def _digest(self, fn) -> str:
        out = C.create_string_buffer(33)
        check(fn(self._h, out))
        return out.value.decode()

    @property
    def identifier(self) -> str:
        """the BEDbase bed digest: md5 of "c,s,e" over the md5s of the joined chromosome names, starts and ends (cached)"""
        if getattr(self, "_identifier", None) is None:
            self._identifier = self._digest(lib.gtars_regionset_identifier)
        return self._identifier

    @property
    def file_digest(self) -> str:
        """md5 of the BED text ``to_bed`` writes"""
        return self._digest(lib.gtars_regionset_file_digest)

    def to_bed(self, path) -> None:
        """one line per region, rest included; parent directories are created, an existing file is replaced.  The text is
        formatted on the host threads; GTARS_BED_TEXT_DEVICE_ROWS names the rows from which the GPU formats it instead
        (unset: never -- with its upload and download the device path measured no faster up to 1e7 rows)."""
        check(lib.gtars_regionset_write_bed(self._h, os.fspath(path).encode(), 0))

    def to_bed_gz(self, path) -> None:
        """the bytes of ``to_bed`` as one gzip member at the best compression level"""
        check(lib.gtars_regionset_write_bed(self._h, os.fspath(path).encode(), 1))

    def _bed_text(self, on_host: bool) -> bytes:
        """the BED text, formatted on the host threads or on the device"""
        p, n = C.c_void_p(), C.c_uint64()
        check(lib.gtars_regionset_bed_text(self._h, int(bool(on_host)), C.byref(p), C.byref(n)))
        try:
            return C.string_at(p, n.value)
        finally:
            lib.gtars_free(p)

    def sort(self) -> None:
        """stable, in place, by (chr bytewise, start): the order of a set read from a file; rest and strands move with
        their rows"""
        if self._strands is not None and len(self):
            names = [nm.encode() for nm in self.chrom_names]
            rank = np.argsort(np.argsort(np.array(names, dtype=object), kind="stable"), kind="stable")
            order = np.lexsort((self.starts, rank[self.chrom_ids]))
            self._strands = [self._strands[i] for i in order]
        check(lib.gtars_regionset_sort(self._h))
        self._identifier = None

    # -- overlap operations (gtars-python/src/models/region_set.rs:445-478) ---------
    def count_overlaps(self, other: "RegionSet") -> List[int]:
        out = np.zeros(len(self), dtype=np.uint32)
        check(lib.gtars_regionset_count_overlaps(self._h, other._h, KIND_AILIST, 0, 0, ptr(out)))
        return [int(x) for x in out]

    def any_overlaps(self, other: "RegionSet") -> List[bool]:
        out = np.zeros(len(self), dtype=np.uint8)
        check(lib.gtars_regionset_any_overlaps(self._h, other._h, KIND_AILIST, 0, 0, ptr(out)))
        return [bool(x) for x in out]

    def find_overlaps(self, other: "RegionSet") -> List[List[int]]:
        n = len(self)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        p, cnt = C.c_void_p(), C.c_uint64()
        check(lib.gtars_regionset_find_overlaps(self._h, other._h, KIND_AILIST, 0, 0, ptr(offsets), C.byref(p), C.byref(cnt)))
        idx = take_u32(p, cnt.value)
        return [[int(v) for v in idx[int(offsets[i]):int(offsets[i + 1])]] for i in range(n)]

    def subset_by_overlaps(self, other: "RegionSet") -> "RegionSet":
        counts = self.count_overlaps(other)
        regs = self.regions
        return RegionSet.from_regions([r for r, c in zip(regs, counts) if c > 0])

    # -- set algebra (gtars-python/src/models/region_set.rs:369-494) -------------------
    # Results are new sets with no rest, no header and strand "*" (PyRegionSet::from_regionset).
    def _result(self, fn, *args) -> "RegionSet":
        h = C.c_void_p()
        check(fn(self._h, *args, C.byref(h)))
        return RegionSet._from_handle(h)

    def reduce(self) -> "RegionSet":
        return self._result(lib.gtars_regionset_reduce)

    def union(self, other: "RegionSet") -> "RegionSet":
        return self._result(lib.gtars_regionset_union, other._h)

    def setdiff(self, other: "RegionSet") -> "RegionSet":
        return self._result(lib.gtars_regionset_setdiff, other._h)

    def intersect_all(self, other: "RegionSet") -> "RegionSet":
        return self._result(lib.gtars_regionset_intersect, other._h)

    def _metric(self, fn, other: "RegionSet") -> float:
        out = C.c_double()
        check(fn(self._h, other._h, C.byref(out)))
        return out.value

    def jaccard(self, other: "RegionSet") -> float:
        return self._metric(lib.gtars_regionset_jaccard, other)

    def coverage(self, other: "RegionSet") -> float:
        return self._metric(lib.gtars_regionset_coverage, other)

    def overlap_coefficient(self, other: "RegionSet") -> float:
        return self._metric(lib.gtars_regionset_overlap_coefficient, other)

    def get_nucleotide_length(self) -> int:
        """nucleotides_length(): the u32 sum of (u32)(end - start), wrapping as the reference's release build does"""
        w = (self.ends - self.starts).astype(np.uint32)
        return int(w.sum(dtype=np.uint64)) & _U32_MAX

    def closest(self, other: "RegionSet") -> List[Tuple[int, int, int]]:
        ps, po, pd = C.c_void_p(), C.c_void_p(), C.c_void_p()
        n = C.c_uint64()
        check(lib.gtars_regionset_closest(self._h, other._h, C.byref(ps), C.byref(po), C.byref(pd), C.byref(n)))
        cols = []
        for p, t in ((ps, C.c_uint64), (po, C.c_uint64), (pd, C.c_int64)):
            try:
                cols.append(np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), shape=(n.value,)).tolist() if n.value else [])
            finally:
                if p.value:
                    lib.gtars_free(p)
        return list(zip(*cols))

    def cluster(self, max_gap: int = 0) -> List[int]:
        if not 0 <= int(max_gap) <= _U32_MAX:
            raise OverflowError("max_gap must fit in u32")
        out = np.zeros(len(self), dtype=np.uint32)
        check(lib.gtars_regionset_cluster(self._h, int(max_gap), ptr(out)))
        return out.tolist()

    # -- structural operations and statistics (gtars-python/src/models/region_set.rs:288-531) ----------------------
    # disjoin / gaps / neighbor_distances / nearest_neighbors / distribution / chromosome_statistics run on the GPU
    # (csrc/setops.hip, K9); the elementwise ones below are O(n) numpy over the host columns.
    def disjoin(self) -> "RegionSet":
        """every boundary a boundary of the result: the covered pieces, sorted by (chr, start), strand "*" """
        return self._result(lib.gtars_regionset_disjoin)

    def gaps(self, chrom_sizes: Dict[str, int]) -> "RegionSet":
        """the uncovered stretches of the chromosomes in chrom_sizes, in karyotypic order (region_set.rs:786-878)"""
        arr, sizes, _keep, n = _sizes(chrom_sizes)
        return self._result(lib.gtars_regionset_gaps, C.cast(arr, C.c_void_p), ptr(sizes), n)

    def neighbor_distances(self) -> List[int]:
        p, n = C.c_void_p(), C.c_uint64()
        check(lib.gtars_regionset_neighbor_distances(self._h, C.byref(p), C.byref(n)))
        return _take(p, C.c_int64, n.value)

    def nearest_neighbors(self) -> List[int]:
        p, n = C.c_void_p(), C.c_uint64()
        check(lib.gtars_regionset_nearest_neighbors(self._h, C.byref(p), C.byref(n)))
        return _take(p, C.c_uint32, n.value)

    def distribution(self, n_bins: int = 250, chrom_sizes: Optional[Dict[str, int]] = None) -> List[dict]:
        """regions per bin of their midpoint: dicts {chr, start, end, n, rid} sorted by (chr, start)"""
        n_bins = _u32(n_bins, "n_bins")
        if chrom_sizes is None:
            arr, sizes, _keep, n, has = None, np.zeros(0, dtype=np.uint32), None, 0, 0
        else:
            (arr, sizes, _keep, n), has = _sizes(chrom_sizes), 1
        p, m = C.c_void_p(), C.c_uint64()
        check(lib.gtars_regionset_distribution(self._h, n_bins, has, C.cast(arr, C.c_void_p) if arr is not None else None,
                                               ptr(sizes), n, C.byref(p), C.byref(m)))
        rows = _take(p, C.c_uint32, 5 * m.value)
        names = self.chrom_names
        return [{"chr": names[rows[k]], "start": rows[k + 1], "end": rows[k + 2], "n": rows[k + 3], "rid": rows[k + 4]}
                for k in range(0, len(rows), 5)]

    def chromosome_statistics(self) -> Dict[str, "ChromosomeStatistics"]:
        pr, pf, m = C.c_void_p(), C.c_void_p(), C.c_uint64()
        check(lib.gtars_regionset_chromosome_statistics(self._h, C.byref(pr), C.byref(pf), C.byref(m)))
        rows, f = _take(pr, C.c_uint32, 6 * m.value), _take(pf, C.c_double, 2 * m.value)
        names = self.chrom_names
        out: Dict[str, ChromosomeStatistics] = {}
        for k in range(m.value):
            c, cnt, lo, hi, wmin, wmax = rows[6 * k:6 * k + 6]
            out[names[c]] = ChromosomeStatistics(names[c], cnt, lo, hi, wmin, wmax, f[2 * k], f[2 * k + 1])
        return out

    def trim(self, chrom_sizes: Dict[str, int]) -> "RegionSet":
        """regions clamped to their chromosome's size; unsized chromosomes and clamped start > end dropped; strand lost"""
        names, ids = self.chrom_names, self.chrom_ids
        size = np.array([_u32(chrom_sizes.get(nm, 0), "chromosome size") for nm in names], dtype=np.uint32)
        known = np.array([nm in chrom_sizes for nm in names], dtype=bool)
        cs = size[ids] if len(ids) else np.zeros(0, dtype=np.uint32)
        s, e = np.minimum(self.starts, cs), np.minimum(self.ends, cs)
        keep = (known[ids] if len(ids) else np.zeros(0, dtype=bool)) & (s <= e)
        return RegionSet.from_vectors([names[i] for i in ids[keep]], s[keep], e[keep])

    def promoters(self, upstream: int, downstream: int) -> "RegionSet":
        """[start - upstream, start + downstream), saturating in u32; strand kept"""
        up, down = _u32(upstream, "upstream"), _u32(downstream, "downstream")
        s = self.starts.astype(np.int64)
        names, ids = self.chrom_names, self.chrom_ids
        return RegionSet._from_columns([names[i] for i in ids], np.maximum(s - up, 0), np.minimum(s + down, _U32_MAX), None,
                                       self.strands)

    def pintersect(self, other: "RegionSet") -> "RegionSet":
        """pairwise by position over the shorter length: [max start, min end), empty at max start when the two do not
        overlap, at self's start when the chromosomes differ; self's strands"""
        n = min(len(self), len(other))
        an, bn = self.chrom_names, other.chrom_names
        ac = [an[i] for i in self.chrom_ids[:n]]
        bc = [bn[i] for i in other.chrom_ids[:n]]
        a_s, a_e, b_s, b_e = self.starts[:n], self.ends[:n], other.starts[:n], other.ends[:n]
        same = np.array([x == y for x, y in zip(ac, bc)], dtype=bool)
        s = np.maximum(a_s, b_s)
        e = np.minimum(a_e, b_e)
        e = np.where(s >= e, s, e)
        s, e = np.where(same, s, a_s), np.where(same, e, a_s)
        return RegionSet._from_columns(ac, s, e, None, self.strands)

    def concat(self, other: "RegionSet") -> "RegionSet":
        """self's regions then other's, rest kept, strand lists concatenated"""
        regs = self.regions + other.regions
        return RegionSet._from_columns([r.chr for r in regs], [r.start for r in regs], [r.end for r in regs],
                                       [r.rest for r in regs], self.strands + other.strands)

    def widths(self) -> List[int]:
        return ((self.ends - self.starts).astype(np.uint32)).tolist()

    def region_widths(self) -> List[int]:
        return self.widths()

    def mean_region_width(self) -> float:
        """wrapping u32 sum of the widths / count, rounded to 2 decimals (half away from zero); nan when empty"""
        n = len(self)
        if n == 0:
            return float("nan")
        v = (self.get_nucleotide_length() / n) * 100.0
        r = math.floor(v)
        return (r + 1.0 if v - r >= 0.5 else float(r)) / 100.0

    def get_max_end_per_chr(self) -> Dict[str, int]:
        """per chromosome, the largest end of its LAST contiguous run in set order (region_set.rs:584-606)"""
        n = len(self)
        if n == 0:
            raise ValueError("get_max_end_per_chr: empty region set")
        ids, e = self.chrom_ids, self.ends
        heads = np.flatnonzero(np.r_[True, ids[1:] != ids[:-1]])
        run_max = np.maximum.reduceat(e, heads)
        names = self.chrom_names
        return {names[int(ids[h])]: int(m) for h, m in zip(heads, run_max)}


class ChromosomeStatistics:
    """gtars.models.ChromosomeStatistics -- one chromosome's entry of ``RegionSet.chromosome_statistics()``, read-only
    (gtars-python/src/models/region_set.rs:13-24, 531-573)."""

    __slots__ = ("_v",)
    _FIELDS = ("chromosome", "number_of_regions", "start_nucleotide_position", "end_nucleotide_position",
               "minimum_region_length", "maximum_region_length", "mean_region_length", "median_region_length")

    def __init__(self, chromosome, number_of_regions, start_nucleotide_position, end_nucleotide_position,
                 minimum_region_length, maximum_region_length, mean_region_length, median_region_length):
        object.__setattr__(self, "_v", (str(chromosome), int(number_of_regions), int(start_nucleotide_position),
                                        int(end_nucleotide_position), int(minimum_region_length),
                                        int(maximum_region_length), float(mean_region_length),
                                        float(median_region_length)))

    def __setattr__(self, name, value):
        raise AttributeError(f"attribute '{name}' of 'ChromosomeStatistics' objects is not writable")

    def __eq__(self, other) -> bool:
        return isinstance(other, ChromosomeStatistics) and self._v == other._v

    def __hash__(self):
        return hash(self._v)

    def __repr__(self) -> str:
        return "ChromosomeStatistics(" + ", ".join(f"{k}={v!r}" for k, v in zip(self._FIELDS, self._v)) + ")"


def _field(i):
    return property(lambda self: self._v[i])


for _i, _name in enumerate(ChromosomeStatistics._FIELDS):
    setattr(ChromosomeStatistics, _name, _field(_i))
del _i, _name


def _u32(x, what: str) -> int:
    if not 0 <= int(x) <= _U32_MAX:
        raise OverflowError(f"{what} must fit in u32")
    return int(x)


def _sizes(chrom_sizes) -> Tuple[object, np.ndarray, list, int]:
    """chrom_sizes (a dict name -> u32) as the parallel arrays the C ABI takes"""
    names = [str(k) for k in chrom_sizes]
    sizes = np.array([_u32(chrom_sizes[k], "chromosome size") for k in chrom_sizes], dtype=np.uint32)
    arr, keep = cstr_array(names)
    return arr, sizes, keep, len(names)


def _take(p: C.c_void_p, ctype, n: int) -> list:
    """a library-allocated array as a list, freed"""
    try:
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(n,)).tolist() if n else []
    finally:
        if p.value:
            lib.gtars_free(p)


class RegionSetList:
    """gtars.models.RegionSetList -- an ordered collection of RegionSets (gtars-python/src/models/region_set_list.rs)."""

    def __init__(self, sets: Iterable[RegionSet]):
        self._sets: List[RegionSet] = list(sets)

    def __len__(self) -> int:
        return len(self._sets)

    def __getitem__(self, index: int) -> RegionSet:
        n = len(self._sets)
        i = index + n if index < 0 else index
        if not 0 <= i < n:
            raise IndexError(f"Index {index} out of range for RegionSetList of length {n}")
        return self._sets[i]

    def __iter__(self):
        return iter(list(self._sets))

    def __repr__(self) -> str:
        return f"RegionSetList with {len(self)} region sets."

    def concat(self) -> RegionSet:
        """every set's regions one after the other, in list order (no merging)"""
        return RegionSet.from_regions([r for s in self._sets for r in s.regions])

    def names(self) -> Optional[List[str]]:
        return None

    # -- digests (region_set_list.rs:85-98; csrc/bed_text.hip, K25) ------------------------------------------------
    # A list is the device's case: every stream of every set -- names, starts, ends, or the BED text -- is one lane of
    # k_bed_md5.  on_host=True runs the same text on `threads` host threads (0: all of them).
    def _digests(self, what: int, on_host: bool, threads: int) -> List[str]:
        n = len(self._sets)
        out = C.create_string_buffer(32 * n + 1)
        check(lib.gtars_regionset_list_digests(self._handles(), n, what, int(bool(on_host)), _u32(threads, "threads"), out))
        return [out.raw[32 * i:32 * i + 32].decode() for i in range(n)]

    def identifiers(self, on_host: bool = False, threads: int = 0) -> List[str]:
        """every member's ``identifier``, in list order"""
        return self._digests(0, on_host, threads)

    def file_digests(self, on_host: bool = False, threads: int = 0) -> List[str]:
        """every member's ``file_digest``, in list order"""
        return self._digests(1, on_host, threads)

    def identifier(self, on_host: bool = False, threads: int = 0) -> str:
        """md5 of the members' identifiers, sorted as strings and concatenated"""
        out = C.create_string_buffer(33)
        check(lib.gtars_regionset_list_identifier(self._handles(), len(self._sets), int(bool(on_host)), _u32(threads, "threads"), out))
        return out.value.decode()

    def pairwise_jaccard(self) -> List[List[float]]:
        """N x N: M[i][j] = reduce(S_i).jaccard(reduce(S_j)), 1.0 on the diagonal; all pairs in one device pass"""
        n = len(self._sets)
        out = np.zeros((n, n), dtype=np.float64)
        handles = (C.c_void_p * max(n, 1))(*[s._h for s in self._sets])
        check(lib.gtars_regionset_pairwise_jaccard(C.cast(handles, C.c_void_p), n, ptr(out)))
        return out.tolist()

    # -- RegionSetListOps (gtars-genomicdist/src/region_set_list_ops.rs:53-182) ------------------------------------
    # The folds run on the GPU (csrc/setops.hip): one upload and one sort of the concatenation.  What the reference
    # answers without a union -- None, and the clones it returns for one set (or for the other set of two) -- is
    # answered here on the host, before any device call.
    def _pair(self, i: int, j: int) -> Optional[Tuple[RegionSet, RegionSet]]:
        """the reference's indices are usize: a negative index is out of range"""
        n = len(self._sets)
        return (self._sets[i], self._sets[j]) if 0 <= i < n and 0 <= j < n else None

    def _handles(self):
        return C.cast((C.c_void_p * max(len(self._sets), 1))(*[s._h for s in self._sets]), C.c_void_p)

    @staticmethod
    def _clone(s: RegionSet) -> RegionSet:
        """the set as it is: rows in their order, unmerged, rest and strands kept"""
        regs = s.regions
        return RegionSet._from_columns([r.chr for r in regs], [r.start for r in regs], [r.end for r in regs],
                                       [r.rest for r in regs], s._strands)

    def pintersect_at(self, i: int, j: int) -> Optional[RegionSet]:
        p = self._pair(i, j)
        return None if p is None else p[0].pintersect(p[1])

    def pintersect_count(self, i: int, j: int) -> Optional[int]:
        r = self.pintersect_at(i, j)
        return None if r is None else len(r)

    def jaccard_at(self, i: int, j: int) -> Optional[float]:
        p = self._pair(i, j)
        return None if p is None else p[0].jaccard(p[1])

    def union_at(self, i: int, j: int) -> Optional[RegionSet]:
        p = self._pair(i, j)
        return None if p is None else p[0].union(p[1])

    def setdiff_at(self, i: int, j: int) -> Optional[RegionSet]:
        p = self._pair(i, j)
        return None if p is None else p[0].setdiff(p[1])

    def region_count(self, i: int) -> Optional[int]:
        return len(self._sets[i]) if 0 <= i < len(self._sets) else None

    def _fold(self, fn) -> Optional[RegionSet]:
        n = len(self._sets)
        if n == 0:
            return None
        if n == 1:
            return self._clone(self._sets[0])
        h = C.c_void_p()
        check(fn(self._handles(), n, C.byref(h)))
        return RegionSet._from_handle(h)

    def union_all(self) -> Optional[RegionSet]:
        """reduce of the concatenation of every set; one set: that set, unmerged; no set: None"""
        return self._fold(lib.gtars_regionset_list_union_all)

    def intersect_all(self) -> Optional[RegionSet]:
        """the left fold of intersect: what every set's own reduce covers; one set: that set, unmerged; no set: None"""
        return self._fold(lib.gtars_regionset_list_intersect_all)

    def union_except(self, skip: int) -> Optional[RegionSet]:
        """reduce of the concatenation of every set but ``skip``; of two sets: the other one, unmerged"""
        n = len(self._sets)
        if n < 2 or not 0 <= skip < n:
            return None
        if n == 2:
            return self._clone(self._sets[1 - skip])
        h = C.c_void_p()
        check(lib.gtars_regionset_list_union_except(self._handles(), n, skip, C.byref(h)))
        return RegionSet._from_handle(h)

    def bulk_union_except(self) -> Optional[Tuple[RegionSet, List[RegionSet]]]:
        """(union_all(), [union_except(i) for every i]) from one upload, one sort and one scan on the device"""
        n = len(self._sets)
        if n < 2:
            return None
        if n == 2:
            return self.union_all(), [self._clone(self._sets[1]), self._clone(self._sets[0])]
        h, arr = C.c_void_p(), C.c_void_p()
        check(lib.gtars_regionset_list_bulk_union_except(self._handles(), n, C.byref(h), C.byref(arr)))
        try:
            hs = C.cast(arr, C.POINTER(C.c_void_p))
            return RegionSet._from_handle(h), [RegionSet._from_handle(C.c_void_p(hs[i])) for i in range(n)]
        finally:
            lib.gtars_free(arr)


# ---------------------------------------------------------------------------------------------------------------------
# TSS / feature distances and gene models (gtars-genomicdist/src/models.rs:516-690, partitions.rs:123-340,
# stranded_region_set.rs:84-135; gtars-python/src/models/{tss_index,gene_model,gda}.rs)
_I64_MAX = (1 << 63) - 1
_GTF_GENE, _GTF_EXON = 0, 1  # feature codes of gtars_gtf_read
_MINUS = 1  # strand codes: 0 '+', 1 '-', 2 unstranded


class TssIndex:
    """gtars.models.TssIndex -- the midpoints start + width / 2 (wrapping u32) of a region set, sorted per chromosome.

    Construction and ``len`` stay on the host; the device index is built at the first distance call, on the device
    current then, and every later call runs there.  Both distance calls return one value per query region, chromosomes
    in order of first appearance in the query and set order within one (for a set read from a BED file: set order)."""

    def __init__(self, path):
        try:
            rs = RegionSet(str(path))
        except Exception:
            # TssIndex::try_from(path) maps every read error to TSSContentError, whose message drops the cause
            raise ValueError("No TSS's found for region. Double-check your index!") from None
        self._h = None
        self._attach(rs)

    @staticmethod
    def from_regionset(rs: RegionSet) -> "TssIndex":
        self = TssIndex.__new__(TssIndex)
        self._h = None
        self._attach(rs)
        return self

    def _attach(self, rs: RegionSet) -> None:
        h = C.c_void_p()
        check(lib.gtars_tss_index_from_regionset(rs._h, C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib.gtars_tss_index_free(self._h)
                self._h = None
        except Exception:
            pass

    def __len__(self) -> int:
        return int(lib.gtars_tss_index_len(self._h))

    def __repr__(self) -> str:
        return f"RegionSet with {len(self)} regions."

    __str__ = __repr__

    def _distances(self, rs: RegionSet) -> Tuple[np.ndarray, np.ndarray]:
        n = len(rs)
        out_abs = np.empty(n, dtype=np.uint32)
        out_signed = np.empty(n, dtype=np.int64)
        check(lib.gtars_tss_index_distances(self._h, rs._h, ptr(out_abs), ptr(out_signed)))
        return out_abs, out_signed

    def calc_tss_distances(self, rs: RegionSet) -> List[int]:
        """distance to the nearest midpoint (0 on an exact hit); 4294967295 on a chromosome the index lacks"""
        return self._distances(rs)[0].tolist()

    def feature_distances(self, rs: RegionSet) -> List[Optional[float]]:
        """nearest midpoint - query midpoint as a float, the upstream one on a tie; None on a chromosome the index lacks"""
        d = self._distances(rs)[1]
        missing = d == _I64_MAX
        vals = d.astype(np.float64).tolist()
        if missing.any():
            for k in np.flatnonzero(missing).tolist():
                vals[k] = None
        return vals


class _Stranded:
    """a strand-aware reduced region set: (chr bytewise, strand, start) order, strand codes 0 '+', 1 '-', 2 other"""

    __slots__ = ("regions", "strands")

    def __init__(self, regions: RegionSet, strands: np.ndarray):
        self.regions = regions
        self.strands = strands

    def __len__(self) -> int:
        return len(self.strands)


def _stranded_reduce(rows: RegionSet, strand: np.ndarray, keep: np.ndarray) -> _Stranded:
    h, p = C.c_void_p(), C.c_void_p()
    keep = np.ascontiguousarray(keep, dtype=np.uint8)
    check(lib.gtars_regionset_stranded_reduce(rows._h, ptr(strand), ptr(keep), C.byref(h), C.byref(p)))
    out = RegionSet._from_handle(h)
    try:
        n = len(out)
        s = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n,)).copy() if n else np.zeros(0, np.uint8)
    finally:
        if p.value:
            lib.gtars_free(p)
    return _Stranded(out, s)


def _read_gtf(path, filter_protein_coding: bool, convert_ensembl_ucsc: bool):
    h, ps, pf = C.c_void_p(), C.c_void_p(), C.c_void_p()
    st = lib.gtars_gtf_read(str(path).encode(), int(bool(filter_protein_coding)), int(bool(convert_ensembl_ucsc)),
                            C.byref(h), C.byref(ps), C.byref(pf))
    if st != 0:
        raise ValueError(_lib.last_error())  # GeneModel::from_gtf: every error is a ValueError (gene_model.rs)
    rows = RegionSet._from_handle(h)
    n = len(rows)
    cols = []
    for p in (ps, pf):
        try:
            cols.append(np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n,)).copy() if n else np.zeros(0, np.uint8))
        finally:
            if p.value:
                lib.gtars_free(p)
    return rows, cols[0], cols[1]


def _stranded_setdiff(a: _Stranded, b: _Stranded) -> _Stranded:
    """a minus b, each row cut only by rows of its own strand code (stranded_region_set.rs:138-217)"""
    h, p = C.c_void_p(), C.c_void_p()
    check(lib.gtars_regionset_stranded_setdiff(a.regions._h, ptr(a.strands), b.regions._h, ptr(b.strands), C.byref(h), C.byref(p)))
    return _Stranded(RegionSet._from_handle(h), np.array(_take(p, C.c_uint8, int(lib.gtars_regionset_len(h))), dtype=np.uint8))


def _reduce_all(rows: RegionSet, strand: np.ndarray) -> _Stranded:
    return _stranded_reduce(rows, np.ascontiguousarray(strand, dtype=np.uint8), np.ones(len(rows), dtype=np.uint8))


def _read_gtf_utrs(path, filter_protein_coding: bool, convert_ensembl_ucsc: bool):
    h, ps, pk = C.c_void_p(), C.c_void_p(), C.c_void_p()
    st = lib.gtars_gtf_read_utrs(str(path).encode(), int(bool(filter_protein_coding)), int(bool(convert_ensembl_ucsc)),
                                 C.byref(h), C.byref(ps), C.byref(pk))
    if st != 0:
        raise ValueError(_lib.last_error())
    rows = RegionSet._from_handle(h)
    n = len(rows)
    return rows, np.array(_take(ps, C.c_uint8, n), dtype=np.uint8), np.array(_take(pk, C.c_uint8, n), dtype=np.uint8)


def _bed_stranded(path, what: str) -> _Stranded:
    """a BED file with the strand of column 6 (the third field of ``rest``; unstranded without one), stranded-reduced"""
    try:
        rs = RegionSet(str(path))
    except Exception as e:
        raise ValueError(f"Loading {what}: {e}") from None
    code = np.full(len(rs), 2, dtype=np.uint8)
    for i in range(len(rs)):
        rest = dec(lib.gtars_regionset_rest(rs._h, i))
        f = rest.split("\t") if rest is not None else []
        if len(f) >= 3:
            code[i] = {"+": 0, "-": 1}.get(f[2][:1], 2)
    return _reduce_all(rs, code)


class GeneModel:
    """gtars.models.GeneModel -- genes, exons and the two UTR sets of a gene model, each merged by a strand-aware reduce.

    ``from_gtf`` reads the GTF on host threads (a malformed number or a line that is not UTF-8 raises ``ValueError``
    before any device work) and reduces on the GPU.  ``three_utr`` / ``five_utr`` are ``None`` when the model has no
    such rows: typed rows, else ``UTR`` rows classified against their transcript's CDS, else exon minus CDS."""

    def __init__(self, *args, **kwargs):
        raise TypeError("No constructor defined for GeneModel")

    @staticmethod
    def _of(genes: _Stranded, exons: _Stranded, three: Optional[_Stranded], five: Optional[_Stranded]) -> "GeneModel":
        self = GeneModel.__new__(GeneModel)
        self._genes, self._exons = genes, exons
        self._three_utr = three if three is not None and len(three) else None
        self._five_utr = five if five is not None and len(five) else None
        return self

    @staticmethod
    def from_gtf(path: str, filter_protein_coding: bool = True, convert_ensembl_ucsc: bool = True) -> "GeneModel":
        rows, strand, feature = _read_gtf(path, filter_protein_coding, convert_ensembl_ucsc)
        utr, ustrand, kind = _read_gtf_utrs(path, filter_protein_coding, convert_ensembl_ucsc)
        three, five = (_stranded_reduce(utr, ustrand, kind == k) if (kind == k).any() else None for k in (0, 1))
        return GeneModel._of(_stranded_reduce(rows, strand, feature == _GTF_GENE), _stranded_reduce(rows, strand, feature == _GTF_EXON),
                             three, five)

    @staticmethod
    def from_bed_files(genes: str, exons: str, three_utr: Optional[str] = None, five_utr: Optional[str] = None) -> "GeneModel":
        """partitions.rs:63-101: every file stranded-reduced, an empty UTR set is None"""
        return GeneModel._of(_bed_stranded(genes, "genes"), _bed_stranded(exons, "exons"),
                             _bed_stranded(three_utr, "3'UTR") if three_utr is not None else None,
                             _bed_stranded(five_utr, "5'UTR") if five_utr is not None else None)

    @property
    def n_genes(self) -> int:
        return len(self._genes)

    @property
    def n_exons(self) -> int:
        return len(self._exons)

    @property
    def three_utr(self) -> Optional[RegionSet]:
        return self._three_utr.regions if self._three_utr is not None else None

    @property
    def five_utr(self) -> Optional[RegionSet]:
        return self._five_utr.regions if self._five_utr is not None else None

    def __repr__(self) -> str:
        return f"GeneModel(n_genes={self.n_genes}, n_exons={self.n_exons})"


class GenomicDistAnnotation:
    """gtars.models.GenomicDistAnnotation -- a GeneModel and the TSS index of its genes."""

    def __init__(self, *args, **kwargs):
        raise TypeError("No constructor defined for GenomicDistAnnotation")

    @staticmethod
    def from_gtf(path: str, filter_protein_coding: bool = True, convert_ensembl_ucsc: bool = True) -> "GenomicDistAnnotation":
        self = GenomicDistAnnotation.__new__(GenomicDistAnnotation)
        self._model = GeneModel.from_gtf(path, filter_protein_coding, convert_ensembl_ucsc)
        return self

    def gene_model(self) -> GeneModel:
        return self._model

    def tss_index(self) -> TssIndex:
        """one TSS per reduced gene: [end - 1, end) (saturating) on the minus strand, [start, start + 1) otherwise"""
        g = self._model._genes
        rs = g.regions
        s, e = rs.starts, rs.ends
        p = np.where(g.strands == _MINUS, np.maximum(e, 1) - 1, s).astype(np.uint32)
        names = np.array(rs.chrom_names, dtype=object)
        ids = rs.chrom_ids
        chrs = names[ids].tolist() if len(ids) else []
        return TssIndex.from_regionset(RegionSet.from_vectors(chrs, p, p + np.uint32(1)))

    def __repr__(self) -> str:
        return f"GenomicDistAnnotation(n_genes={self._model.n_genes}, n_exons={self._model.n_exons})"
