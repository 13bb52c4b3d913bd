"""``gtars.partitions`` (additive): genomic partitions -- ``PartitionList``, ``calc_partitions`` and ``calc_expected_partitions``,
which the reference keeps in ``gtars.models`` and ``gtars.genomic_distributions`` (gtars-python/src/models/partition_list.rs,
gda.rs, genomic_distributions/tools.rs:72-118; gtars-genomicdist/src/partitions.rs:363-784).  They sit in a module of their own
as ``gtars.seqstats`` and ``gtars.signal`` do.  ``PartitionList.from_annotation(gda, ...)`` stands for the reference's
``GenomicDistAnnotation.partition_list(...)``.

The list is built from the strand-aware reduce and setdiff on the GPU; ``calc_partitions`` classifies the regions against it
on the GPU (csrc/partitions.hip, K14): one lane per region, two binary searches per partition for the priority counts,
prefix sums of the sorted starts and ends for the bp counts.  ``partition_assignments`` returns the per-region bucket behind
the priority counts.  ``calc_expected_partitions`` adds the reference's own chi-square arithmetic, f64 on the host
(csrc/partitions.cpp).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import numpy as np

from ._lib import check, cstr_array, dec, lib, ptr
from .models import (_MINUS, _U32_MAX, GeneModel, GenomicDistAnnotation, RegionSet, _reduce_all, _Stranded, _stranded_setdiff,
                     _u32)


def _promoters(g: _Stranded, upstream: int, chrom_sizes: Optional[Dict[str, int]]) -> _Stranded:
    """reduce(trim(promoters(upstream, 0))), all strand-aware (stranded_region_set.rs:16-80): [end, end + upstream) on the
    minus strand, [start - upstream, start) otherwise, saturating in u32; with sizes, rows of a sized chromosome are
    clamped to it and dropped when nothing is left, rows of any other chromosome stay as they are"""
    rs = g.regions
    s, e = rs.starts.astype(np.int64), rs.ends.astype(np.int64)
    minus = g.strands == _MINUS
    ps = np.where(minus, e, np.maximum(s - upstream, 0))
    pe = np.where(minus, np.minimum(e + upstream, _U32_MAX), s)
    names, ids = rs.chrom_names, rs.chrom_ids
    keep = np.ones(len(ps), dtype=bool)
    if chrom_sizes is not None and len(ps):
        size = np.array([_u32(chrom_sizes.get(nm, 0), "chromosome size") for nm in names], dtype=np.int64)[ids]
        known = np.array([nm in chrom_sizes for nm in names], dtype=bool)[ids]
        ps, pe = np.where(known, np.minimum(ps, size), ps), np.where(known, np.minimum(pe, size), pe)
        keep = ~known | (ps < pe)
    rows = RegionSet.from_vectors([names[i] for i in ids[keep]], ps[keep], pe[keep])
    return _reduce_all(rows, g.strands[keep])


class PartitionList:
    """gtars.partitions.PartitionList -- the ordered, named partitions of a gene model (genome_partition_list,
    partitions.rs:410-483): promoterCore, promoterProx, threeUTR and fiveUTR when the model has them, exon, intron.  The
    order is the priority ``calc_partitions`` resolves overlaps by."""

    def __init__(self, *args, **kwargs):
        raise TypeError("No constructor defined for PartitionList")

    @staticmethod
    def _from_sets(names: Sequence[str], sets: Sequence[RegionSet]) -> "PartitionList":
        self = PartitionList.__new__(PartitionList)
        self._h = None
        arr, _keep = cstr_array(list(names))
        handles = (C.c_void_p * max(len(sets), 1))(*[s._h for s in sets])
        h = C.c_void_p()
        check(lib.gtars_partition_list_from_sets(C.cast(arr, C.c_void_p), C.cast(handles, C.c_void_p), len(sets), C.byref(h)))
        self._h = h
        return self

    @staticmethod
    def from_gene_model(gene_model: GeneModel, core_prom: int, prox_prom: int,
                        chrom_sizes: Optional[Dict[str, int]] = None) -> "PartitionList":
        core_prom, prox_prom = _u32(core_prom, "core_prom"), _u32(prox_prom, "prox_prom")
        m = gene_model
        core = _promoters(m._genes, core_prom, chrom_sizes)
        prox = _stranded_setdiff(_promoters(m._genes, prox_prom, chrom_sizes), core)
        three, five = m._three_utr, m._five_utr
        parts = [("promoterCore", core), ("promoterProx", prox)]
        if three is not None:
            parts.append(("threeUTR", three))
        if five is not None:
            parts.append(("fiveUTR", _stranded_setdiff(five, three) if three is not None else five))
        exon, intron = m._exons, m._genes
        for utr in (three, five):
            if utr is not None:
                exon, intron = _stranded_setdiff(exon, utr), _stranded_setdiff(intron, utr)
        parts += [("exon", exon), ("intron", _stranded_setdiff(intron, m._exons))]
        return PartitionList._from_sets([n for n, _ in parts], [p.regions for _, p in parts])

    @staticmethod
    def from_annotation(annotation: GenomicDistAnnotation, core_prom: int, prox_prom: int,
                        chrom_sizes: Optional[Dict[str, int]] = None) -> "PartitionList":
        """the reference's ``GenomicDistAnnotation.partition_list(core_prom, prox_prom, chrom_sizes)``"""
        return PartitionList.from_gene_model(annotation.gene_model(), core_prom, prox_prom, chrom_sizes)

    @staticmethod
    def from_gtf(path: str, core_prom: int, prox_prom: int, filter_protein_coding: bool = True, convert_ensembl_ucsc: bool = True,
                 chrom_sizes: Optional[Dict[str, int]] = None) -> "PartitionList":
        return PartitionList.from_gene_model(GeneModel.from_gtf(path, filter_protein_coding, convert_ensembl_ucsc), core_prom,
                                             prox_prom, chrom_sizes)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib.gtars_partition_list_free(self._h)
                self._h = None
        except Exception:
            pass

    def partition_names(self) -> List[str]:
        return [dec(lib.gtars_partition_list_name(self._h, i)) for i in range(len(self))]

    def partition(self, name: str) -> RegionSet:
        """the rows of the partition called ``name`` (the first of that name), strands dropped"""
        h = C.c_void_p()
        check(lib.gtars_partition_list_set(self._h, self.partition_names().index(name), C.byref(h)))
        return RegionSet._from_handle(h)

    @property
    def chrom_names(self) -> List[str]:
        """the list's chromosome dictionary: the ids the device-pointer entry takes"""
        return [dec(lib.gtars_partition_list_chrom_name(self._h, i)) for i in range(lib.gtars_partition_list_n_chrom(self._h))]

    @property
    def device(self) -> int:
        """the device that holds the index, -1 before the first ``calc_partitions``"""
        return int(lib.gtars_partition_list_device(self._h))

    def __len__(self) -> int:
        return int(lib.gtars_partition_list_len(self._h))

    def __repr__(self) -> str:
        return "PartitionList(partitions=[" + ", ".join(f'"{n}"' for n in self.partition_names()) + "])"


def _count(rs: RegionSet, partition_list: PartitionList, bp: bool, assign: Optional[np.ndarray] = None):
    counts = np.zeros(len(partition_list) + 1, dtype=np.uint32)
    total = C.c_uint32()
    check(lib.gtars_partitions_count(partition_list._h, rs._h, int(bp), ptr(counts), C.byref(total),
                                     ptr(assign) if assign is not None else None))
    return counts, total.value


def calc_partitions(rs: RegionSet, partition_list: PartitionList, bp_proportion: bool = False) -> dict:
    """{"partition": [..names, "intergenic"], "count": [...], "total": n} (partitions.rs:493-592): every region counted for
    the first partition it overlaps in list order, or with ``bp_proportion`` the overlapping base pairs per partition (a
    region adds to every partition it overlaps) and the rest of the regions' widths as intergenic, all in wrapping u32"""
    counts, total = _count(rs, partition_list, bool(bp_proportion))
    return {"partition": partition_list.partition_names() + ["intergenic"], "count": counts.tolist(), "total": total}


def partition_assignments(rs: RegionSet, partition_list: PartitionList) -> np.ndarray:
    """per region of ``rs``, in its order, the index of the partition ``calc_partitions`` counts it for (u8);
    ``len(partition_list)`` is intergenic"""
    out = np.zeros(len(rs), dtype=np.uint8)
    _count(rs, partition_list, False, out)
    return out


def calc_expected_partitions(rs: RegionSet, partition_list: PartitionList, chrom_sizes: Dict[str, int],
                             bp_proportion: bool = False) -> dict:
    """{"partition", "observed", "expected", "log10OE", "pvalue"} (partitions.rs:598-784): expected = the partition's share
    of the genome (raw sum of its rows' widths over the sum of ``chrom_sizes``) times the total; intergenic takes what the
    partitions leave of the genome"""
    counts, total = _count(rs, partition_list, bool(bp_proportion))
    n = len(partition_list)
    sizes = np.zeros(n, dtype=np.uint64)
    check(lib.gtars_partition_list_sizes(partition_list._h, ptr(sizes)))
    genome = sum(_u32(v, "chromosome size") for v in chrom_sizes.values())
    exp, oe, pv = (np.zeros(n + 1, dtype=np.float64) for _ in range(3))
    check(lib.gtars_partition_expected(ptr(counts), ptr(sizes), n, total, genome, ptr(exp), ptr(oe), ptr(pv)))
    return {"partition": partition_list.partition_names() + ["intergenic"], "observed": counts.astype(np.float64).tolist(),
            "expected": exp.tolist(), "log10OE": oe.tolist(), "pvalue": pv.tolist()}


def partitions_count_device(partition_list: PartitionList, d_chrom: int, d_start: int, d_end: int, n: int, stream: int = 0,
                            bp_proportion: bool = False, d_assign: int = 0):
    """``calc_partitions`` for ``n`` regions whose u32 columns are on the index's device already (additive): ``d_chrom`` holds
    ids of ``partition_list.chrom_names`` (any other value: no hit), ``stream`` is a hipStream_t of that device, ``d_assign``
    an optional device pointer to ``n`` bytes for the per-region buckets.  -> (counts as u32 array, total)"""
    counts = np.zeros(len(partition_list) + 1, dtype=np.uint32)
    total = C.c_uint32()
    check(lib.gtars_partitions_count_device(partition_list._h, C.c_void_p(d_chrom), C.c_void_p(d_start), C.c_void_p(d_end), int(n),
                                            int(bool(bp_proportion)), C.c_void_p(stream), ptr(counts), C.byref(total),
                                            C.c_void_p(d_assign) if d_assign else None))
    return counts, total.value
