"""``gtars`` -- drop-in import namespace over gtars_amd.

The reference's Python package registers its sub-modules in sys.modules (gtars-python/src/lib.rs:27-104), so user
code reads ``from gtars.tokenizers import Tokenizer``, ``from gtars.models import RegionSet``,
``from gtars.utils import read_tokens_from_gtok``, ``from gtars.lola import RegionDB, run_lola``.  This package makes
those imports resolve to the MI355X implementation (gtars_amd.*) without edits to the calling code.
``gtars.genomic_distributions`` provides ``consensus`` and ``median_abs_distance``, the functions of that module that need
nothing beyond region sets.  The one sub-module that is not provided under this name is refget: importing ``gtars.refget``
raises ModuleNotFoundError, not a silent stub; the module lives in ``gtars_amd.refget`` (registering the alias is a follow-up).
``gtars.igd``, ``gtars.scoring`` and ``gtars.fragsplit`` are additive (the
reference exposes those crates through Rust / the CLI only).  ``gtars.seqstats`` is additive too: it holds
``GenomeAssembly``, ``BinaryGenomeAssembly``, ``calc_gc_content`` and ``calc_dinucl_freq``, which the reference keeps in
``gtars.models`` and ``gtars.genomic_distributions``; ``gtars.signal`` likewise holds ``SignalMatrix`` and
``calc_summary_signal``, and ``gtars.partitions`` holds ``PartitionList``, ``calc_partitions`` and ``calc_expected_partitions``.
``gtars.bam`` holds ``BamFile``, ``read_bam_header`` and the BAM QC of ``gtars uniwig bamqc`` (``compute_bam_qc``, ``run_bam_qc``,
``write_bam_qc_tsv``) and, this library's own, ``BamFile.fragments`` / ``bam_to_fragments``.
``gtars.vrs`` holds the reference's four functions (``vrs_digest``, ``vrs_id``, ``normalize_allele``,
``location_digest``) and the batch calls on top of the device kernels (``normalize_alleles``, ``vrs_ids``, ``compute_vrs_ids``);
its ``hgvs`` sub-module (``gtars.vrs.hgvs``, also ``gtars.hgvs``) holds the reference's HGVS parser classes, ``parse_hgvs``,
``HgvsError`` and ``hgvs_to_vrs_id`` over an assembly and a transcript store, and, additive, the batch bridge on the device
(``hgvs_to_vrs_ids``), and the transcript-anchored bridge (``hgvs_to_transcript_vrs_id``, ``hgvs_to_transcript_allele``, the batch
``hgvs_to_transcript_vrs_ids``; ``gtars.vrs.transcript_vrs_ids`` for alleles given on transcripts).  ``gtars.reftx`` holds the reference's transcript classes (``TxStoreBuilder``,
``ReadonlyTxStore``, ``CoordinateMapper``, ``Transcript``, ``Exon``, ``ManeStatus``, ``Strand``, ``MappingError``, ``TxStoreError``) and, additive,
the batch mapping calls and the spliced mRNA of every transcript on the device (``mature_mrna``, ``mature_mrnas``,
``transcript_accessions``); ``ReftxProvider`` is not provided.
"""
import sys as _sys

import gtars_amd as _impl
from gtars_amd import bam, fragsplit, genomic_distributions, igd, lola, models, partitions, scoring, seqstats, signal, tokenizers, utils, vrs, reftx, hgvs  # noqa: F401

for _name in ("bam", "tokenizers", "models", "utils", "lola", "igd", "scoring", "fragsplit", "genomic_distributions", "seqstats", "signal", "partitions", "vrs", "reftx", "hgvs"):
    _sys.modules[f"{__name__}.{_name}"] = getattr(_sys.modules[__name__], _name)

_sys.modules[f"{__name__}.vrs.hgvs"] = hgvs  # (gtars-python/src/vrs/mod.rs registers the sub-module under vrs)

__version__ = _impl.__version__
__all__ = ["bam", "tokenizers", "models", "utils", "lola", "igd", "scoring", "fragsplit", "genomic_distributions", "seqstats", "signal", "partitions", "vrs", "reftx", "hgvs"]
