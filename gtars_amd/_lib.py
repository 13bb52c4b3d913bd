"""ctypes binding of libgtars_amd.so (the C ABI in include/gtars_amd.h).

There is no fallback: if the shared library is missing this module raises at
import time, and every compute call fails with GTARS_ERR_NO_DEVICE when no
MI355X is visible.  The CPU oracle under ``oracle/`` is never imported here.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GTARS_AMD_LIB") or os.path.join(_HERE, "libgtars_amd.so")

GTARS_OK = 0
ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_CAPACITY, ERR_IO, ERR_PARSE, ERR_EMPTY, ERR_CONFIG, ERR_INTERNAL = range(1, 10)

KIND_BITS = 0
KIND_AILIST = 1
PAD_RIGHT = 0
PAD_LEFT = 1
UNKNOWN_CHROM = 0xFFFFFFFF


class GtarsError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"[gtars_amd status {status}] {message}")
        self.status = status
        self.message = message


class NoDeviceError(GtarsError):
    pass


class CapacityError(GtarsError):
    @property
    def needed(self) -> int:
        """the element count the library asked for ("... need N")"""
        import re

        m = re.search(r"need (\d+)", self.message)
        return int(m.group(1)) if m else 0


if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
        "(hipcc --offload-arch=gfx950).  gtars_amd has no CPU fallback."
    )

# One process must hold ONE HIP runtime.  PyTorch wheels bundle their own libamdhip64.so.7; if this library
# pulled in /opt/rocm's copy first, torch would later fail with "No HIP GPUs are available".  Importing torch
# first makes the dynamic linker resolve our NEEDED libamdhip64.so.7 to the copy torch already mapped.
if os.environ.get("GTARS_AMD_NO_TORCH") != "1":
    try:
        import torch  # noqa: F401
    except ImportError:  # torch is plumbing (device buffers, torch.distributed), not a hard dependency
        pass

lib = C.CDLL(LIB_PATH)

vp, u32, u64, i32, i64 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32, C.c_int64
pp = C.POINTER(C.c_void_p)
pu64 = C.POINTER(C.c_uint64)

_SIG = {
    "gtars_last_error": (C.c_char_p, []),
    "gtars_version": (C.c_char_p, []),
    "gtars_device_count": (C.c_int, []),
    "gtars_free": (None, [vp]),
    "gtars_index_build": (C.c_int, [vp, vp, vp, vp, u64, u32, C.c_int, pp]),
    "gtars_index_free": (None, [vp]),
    "gtars_index_len": (u64, [vp]),
    "gtars_index_n_chrom": (u32, [vp]),
    "gtars_index_kind": (C.c_int, [vp]),
    "gtars_index_device": (C.c_int, [vp]),
    "gtars_index_chrom_len": (u64, [vp, u32]),
    "gtars_index_stored": (C.c_int, [vp, u32, vp, vp, vp]),
    "gtars_index_insert": (C.c_int, [vp, u32, u32, u32, u32, vp]),
    "gtars_index_seek": (C.c_int, [vp, u32, u32, u32, vp, vp, u64, vp]),
    "gtars_index_max_len": (u32, [vp, u32]),
    "gtars_index_n_sublists": (u64, [vp, u32]),
    "gtars_index_sublist_offsets": (C.c_int, [vp, u32, vp]),
    "gtars_tokenize_device": (C.c_int, [vp, vp, vp, vp, u64, vp, vp, u64, pu64, vp]),
    "gtars_fill_device": (C.c_int, [vp, vp, vp, vp, u64, vp, vp, vp]),
    "gtars_fill_device_n": (C.c_int, [vp, vp, vp, vp, u64, vp, vp, u64, vp]),
    "gtars_tokenize_device_ex": (C.c_int, [vp, vp, vp, vp, u64, vp, vp, u64, pu64, vp, C.c_int]),
    "gtars_tokenize_sets_device": (C.c_int, [vp, vp, vp, vp, u64, vp, u64, u32, u64, vp, vp, u64, pu64, pu64, vp]),
    "gtars_pad_sets_device": (C.c_int, [vp, vp, u64, u64, u32, C.c_int, vp, vp, vp]),
    "gtars_histogram_u32_device": (C.c_int, [vp, u64, u32, vp, vp]),
    "gtars_histogram_rows_device": (C.c_int, [vp, vp, vp, u64, u32, u32, u32, vp, vp]),
    "gtars_count_matrix_csr_device": (C.c_int, [vp, vp, vp, u64, u32, u32, vp, vp, vp, u64, pu64, vp]),
    "gtars_tokenize": (C.c_int, [vp, vp, vp, vp, u64, vp, pp, pu64]),
    "gtars_tokenize_into": (C.c_int, [vp, vp, vp, vp, u64, vp, vp, u64, pu64]),
    "gtars_count_overlaps_device": (C.c_int, [vp, vp, vp, vp, u64, C.c_int, i32, vp, vp]),
    "gtars_count_overlaps": (C.c_int, [vp, vp, vp, vp, u64, C.c_int, i32, vp]),
    "gtars_bits_count_device": (C.c_int, [vp, vp, vp, vp, u64, vp, vp]),
    "gtars_bits_count": (C.c_int, [vp, vp, vp, vp, u64, vp]),
    "gtars_any_overlaps": (C.c_int, [vp, vp, vp, vp, u64, C.c_int, i32, vp]),
    "gtars_find_overlaps": (C.c_int, [vp, vp, vp, vp, u64, C.c_int, i32, vp, pp, pp, pp, pu64]),
    "gtars_find_overlap_indices": (C.c_int, [vp, vp, vp, vp, u64, C.c_int, i32, vp, pp, pu64]),
    "gtars_subset_by_overlaps": (C.c_int, [vp, vp, vp, vp, u64, C.c_int, i32, pp, pp, pp, pu64]),
    "gtars_subset_source_indices": (C.c_int, [vp, vp, vp, vp, u64, C.c_int, i32, pp, pu64]),
    "gtars_mark_overlapped_device": (C.c_int, [vp, vp, vp, vp, u64, C.c_int, i32, vp, vp]),
    "gtars_igd_build": (C.c_int, [vp, vp, vp, vp, vp, u64, u32, u32, pp]),
    "gtars_igd_free": (None, [vp]),
    "gtars_igd_len": (u64, [vp]),
    "gtars_igd_n_files": (u32, [vp]),
    "gtars_igd_device": (C.c_int, [vp]),
    "gtars_igd_total_records": (u64, [vp, i32]),
    "gtars_igd_export": (C.c_int, [vp, vp, vp, vp, vp, vp]),
    "gtars_igd_count_device": (C.c_int, [vp, vp, vp, vp, u64, i32, C.c_int, vp, vp]),
    "gtars_igd_count": (C.c_int, [vp, vp, vp, vp, u64, i32, C.c_int, vp]),
    "gtars_igd_count_sets_device": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint32, i32, C.c_int, vp, vp]),
    "gtars_igd_count_sets": (C.c_int, [vp, vp, vp, vp, vp, C.c_uint32, i32, C.c_int, vp]),
    "gtars_igd_count_per_query": (C.c_int, [vp, vp, vp, vp, u64, i32, vp]),
    "gtars_igd_find_pairs": (C.c_int, [vp, vp, vp, vp, u64, i32, pp, pp, pu64]),
    "gtars_lola_contingency_device": (C.c_int, [vp, vp, u64, i64, i64, vp, vp, vp, vp, vp]),
    "gtars_refget_digests_device": (C.c_int, [vp, vp, vp, vp, vp]),
    "gtars_refget_substrings_device": (C.c_int, [vp, vp, vp, vp, u64, vp, vp, vp, u64, pu64, vp]),
    "gtars_refget_packed_substrings_device": (C.c_int, [vp, vp, vp, vp, u64, vp, vp, vp, u64, pu64, vp]),
    "gtars_bed_digests_device": (C.c_int, [vp, u64, vp, vp, vp, vp, vp, u32, vp, vp, vp, C.c_int, vp, vp]),
    "gtars_prof_enable": (None, [C.c_int]),
    "gtars_prof_reset": (None, []),
    "gtars_prof_read": (C.c_int, [vp, vp, vp, C.c_int]),
}

pvp = C.POINTER(C.c_void_p)


class FragmentTokens(C.Structure):
    _fields_ = [
        ("n_barcodes", C.c_uint64),
        ("barcodes", C.POINTER(C.c_char_p)),
        ("offsets", C.POINTER(C.c_uint64)),
        ("ids", C.POINTER(C.c_uint32)),
    ]


cstr = C.c_char_p
# include/gtars_amd_host.h
_HOST_SIG = {
    "gtars_regionset_from_bed": (C.c_int, [cstr, pp]),
    "gtars_regionset_from_arrays": (C.c_int, [vp, vp, vp, vp, u64, pp]),
    "gtars_regionset_free": (None, [vp]),
    "gtars_regionset_dense_ids": (C.c_int, [vp, pp, vp]),
    "gtars_regionset_len": (u64, [vp]),
    "gtars_regionset_header": (cstr, [vp]),
    "gtars_regionset_n_chrom": (u32, [vp]),
    "gtars_regionset_chrom_name": (cstr, [vp, u32]),
    "gtars_regionset_chrom_ids": (vp, [vp]),
    "gtars_regionset_starts": (vp, [vp]),
    "gtars_regionset_ends": (vp, [vp]),
    "gtars_regionset_rest": (cstr, [vp, u64]),
    "gtars_regionset_count_overlaps": (C.c_int, [vp, vp, C.c_int, C.c_int, i32, vp]),
    "gtars_regionset_any_overlaps": (C.c_int, [vp, vp, C.c_int, C.c_int, i32, vp]),
    "gtars_regionset_find_overlaps": (C.c_int, [vp, vp, C.c_int, C.c_int, i32, vp, pp, pu64]),
    "gtars_regionset_reduce": (C.c_int, [vp, pp]),
    "gtars_regionset_union": (C.c_int, [vp, vp, pp]),
    "gtars_regionset_setdiff": (C.c_int, [vp, vp, pp]),
    "gtars_regionset_intersect": (C.c_int, [vp, vp, pp]),
    "gtars_regionset_jaccard": (C.c_int, [vp, vp, vp]),
    "gtars_regionset_coverage": (C.c_int, [vp, vp, vp]),
    "gtars_regionset_overlap_coefficient": (C.c_int, [vp, vp, vp]),
    "gtars_regionset_closest": (C.c_int, [vp, vp, pp, pp, pp, pu64]),
    "gtars_regionset_cluster": (C.c_int, [vp, u32, vp]),
    "gtars_regionset_pairwise_jaccard": (C.c_int, [vp, u64, vp]),
    "gtars_regionset_list_union_all": (C.c_int, [vp, u64, pp]),
    "gtars_regionset_list_intersect_all": (C.c_int, [vp, u64, pp]),
    "gtars_regionset_list_union_except": (C.c_int, [vp, u64, u64, pp]),
    "gtars_regionset_list_bulk_union_except": (C.c_int, [vp, u64, pp, pp]),
    "gtars_regionset_identifier": (C.c_int, [vp, vp]),
    "gtars_regionset_file_digest": (C.c_int, [vp, vp]),
    "gtars_regionset_bed_text": (C.c_int, [vp, C.c_int, pp, pu64]),
    "gtars_regionset_write_bed": (C.c_int, [vp, cstr, C.c_int]),
    "gtars_regionset_sort": (C.c_int, [vp]),
    "gtars_regionset_list_digests": (C.c_int, [vp, u64, C.c_int, C.c_int, u32, vp]),
    "gtars_regionset_list_identifier": (C.c_int, [vp, u64, C.c_int, u32, vp]),
    "gtars_regionset_disjoin": (C.c_int, [vp, pp]),
    "gtars_regionset_gaps": (C.c_int, [vp, vp, vp, u64, pp]),
    "gtars_regionset_consensus": (C.c_int, [vp, u64, pp, pp]),
    "gtars_regionset_neighbor_distances": (C.c_int, [vp, pp, pu64]),
    "gtars_regionset_nearest_neighbors": (C.c_int, [vp, pp, pu64]),
    "gtars_regionset_distribution": (C.c_int, [vp, u32, C.c_int, vp, vp, u64, pp, pu64]),
    "gtars_regionset_chromosome_statistics": (C.c_int, [vp, pp, pp, pu64]),
    "gtars_gtf_read": (C.c_int, [cstr, C.c_int, C.c_int, pp, pp, pp]),
    "gtars_regionset_stranded_reduce": (C.c_int, [vp, vp, vp, pp, pp]),
    "gtars_regionset_stranded_setdiff": (C.c_int, [vp, vp, vp, vp, pp, pp]),
    "gtars_gtf_read_utrs": (C.c_int, [cstr, C.c_int, C.c_int, pp, pp, pp]),
    "gtars_tss_index_from_regionset": (C.c_int, [vp, pp]),
    "gtars_tss_index_free": (None, [vp]),
    "gtars_tss_index_len": (u64, [vp]),
    "gtars_tss_index_device": (C.c_int, [vp]),
    "gtars_tss_index_distances": (C.c_int, [vp, vp, vp, vp]),
    "gtars_partition_list_from_sets": (C.c_int, [vp, vp, u32, pp]),
    "gtars_partition_list_free": (None, [vp]),
    "gtars_partition_list_len": (u32, [vp]),
    "gtars_partition_list_name": (cstr, [vp, u32]),
    "gtars_partition_list_n_chrom": (u32, [vp]),
    "gtars_partition_list_chrom_name": (cstr, [vp, u32]),
    "gtars_partition_list_set": (C.c_int, [vp, u32, pp]),
    "gtars_partition_list_sizes": (C.c_int, [vp, vp]),
    "gtars_partition_list_device": (C.c_int, [vp]),
    "gtars_partitions_count": (C.c_int, [vp, vp, C.c_int, vp, vp, vp]),
    "gtars_partitions_count_device": (C.c_int, [vp, vp, vp, vp, u64, C.c_int, vp, vp, vp, vp]),
    "gtars_partition_expected": (C.c_int, [vp, vp, u32, u32, u64, vp, vp, vp]),
    "gtars_uniwig_counts": (C.c_int, [vp, vp, u64, u32, u32, C.c_int, u64, pu64, pp, pu64]),
    "gtars_uniwig_extent": (C.c_int, [vp, vp, u64, u32, u32, C.c_int, pu64, pu64]),
    "gtars_uniwig_counts_device": (C.c_int, [vp, vp, u64, u32, C.c_int, u64, u64, vp, vp]),
    "gtars_uniwig_runs": (C.c_int, [vp, vp, u64, u32, u32, C.c_int, u32, pp, pp, pp, pu64]),
    "gtars_uniwig_nonzero": (C.c_int, [vp, vp, u64, u32, u32, C.c_int, u32, pp, pp, pu64]),
    "gtars_uniwig_format_counts": (C.c_int, [vp, u64, pp, pu64]),
    "gtars_uniwig_format_pairs": (C.c_int, [vp, vp, u64, pp, pu64]),
    "gtars_uniwig_format_bedgraph": (C.c_int, [cstr, vp, vp, vp, u64, pp, pu64]),
    "gtars_uniwig_stream_parse": (C.c_int, [cstr, vp, u64, pp]),
    "gtars_uniwig_rows_free": (None, [vp]),
    "gtars_uniwig_rows_len": (u64, [vp]),
    "gtars_uniwig_rows_n_chrom": (u32, [vp]),
    "gtars_uniwig_rows_chrom_name": (cstr, [vp, u32]),
    "gtars_uniwig_rows_columns": (C.c_int, [vp, pp, pp, pp, pp]),
    "gtars_uniwig_stream": (C.c_int, [vp, vp, vp, vp, u64, vp, u32, u32, u32, C.c_int, i64, u64, pp, pp, pp, pu64, pp, pu64]),
    "gtars_uniwig_stream_plan_device": (C.c_int, [vp, vp, vp, vp, u64, vp, u32, u32, C.c_int, i64, pp]),
    "gtars_uniwig_plan_free": (None, [vp]),
    "gtars_uniwig_plan_segments": (u64, [vp]),
    "gtars_uniwig_plan_total": (u64, [vp]),
    "gtars_uniwig_plan_table": (C.c_int, [vp, vp, vp, vp, vp]),
    "gtars_uniwig_stream_device": (C.c_int, [vp, u64, u64, vp, vp]),
    "gtars_uniwig_format_bedgraph_bases": (C.c_int, [cstr, u32, u32, vp, u64, pp, pu64]),
    "gtars_assembly_from_fasta": (C.c_int, [cstr, pp]),
    "gtars_assembly_from_fab": (C.c_int, [cstr, pp]),
    "gtars_fab_write_from_fasta": (C.c_int, [cstr, cstr]),
    "gtars_assembly_free": (None, [vp]),
    "gtars_assembly_n_chrom": (u32, [vp]),
    "gtars_assembly_chrom_name": (cstr, [vp, u32]),
    "gtars_assembly_chrom_len": (u64, [vp, u32]),
    "gtars_assembly_contains": (C.c_int, [vp, cstr]),
    "gtars_assembly_sequence": (C.c_int, [vp, cstr, u64, u64, pp]),
    "gtars_assembly_device": (C.c_int, [vp]),
    "gtars_seqstats_piece_bytes": (u32, []),
    "gtars_seqstats_counts_device": (C.c_int, [vp, vp, vp, vp, u64, C.c_int, vp, vp]),
    "gtars_seqstats_gc": (C.c_int, [vp, vp, C.c_int, pp, pu64]),
    "gtars_seqstats_dinucl": (C.c_int, [vp, vp, C.c_int, C.c_int, pp, pp, pu64]),
    "gtars_signal_from_tsv": (C.c_int, [cstr, pp]),
    "gtars_signal_load_bin": (C.c_int, [cstr, pp]),
    "gtars_signal_save_bin": (C.c_int, [vp, cstr]),
    "gtars_signal_from_arrays": (C.c_int, [vp, u32, vp, vp, vp, u64, vp, vp, u32, pp]),
    "gtars_signal_free": (None, [vp]),
    "gtars_signal_n_regions": (u64, [vp]),
    "gtars_signal_n_conditions": (u32, [vp]),
    "gtars_signal_condition_name": (cstr, [vp, u32]),
    "gtars_signal_n_chrom": (u32, [vp]),
    "gtars_signal_chrom_name": (cstr, [vp, u32]),
    "gtars_signal_chrom_ids": (vp, [vp]),
    "gtars_signal_starts": (vp, [vp]),
    "gtars_signal_ends": (vp, [vp]),
    "gtars_signal_values": (vp, [vp]),
    "gtars_signal_device": (C.c_int, [vp]),
    "gtars_signal_summary": (C.c_int, [vp, vp, pp, pp, pp, pu64]),
    "gtars_signal_summary_device": (C.c_int, [vp, vp, vp, vp, u64, vp, pp, pp, pp, pu64]),
    "gtars_tokenizer_from_auto": (C.c_int, [cstr, pp]),
    "gtars_tokenizer_from_config": (C.c_int, [cstr, pp]),
    "gtars_tokenizer_from_bed": (C.c_int, [cstr, pp]),
    "gtars_tokenizer_free": (None, [vp]),
    "gtars_tokenizer_vocab_size": (u64, [vp]),
    "gtars_tokenizer_kind": (C.c_int, [vp]),
    "gtars_tokenizer_id_to_token": (cstr, [vp, u32]),
    "gtars_tokenizer_token_to_id": (i64, [vp, cstr]),
    "gtars_tokenizer_vocab_token": (cstr, [vp, u64, C.POINTER(C.c_uint32)]),
    "gtars_tokenizer_special_token": (cstr, [vp, C.c_int]),
    "gtars_tokenizer_region_name": (cstr, [vp, cstr]),
    "gtars_tokenizer_region_score": (C.c_double, [vp, cstr]),
    "gtars_tokenizer_chrom_id": (i64, [vp, cstr]),
    "gtars_tokenizer_n_chrom": (u32, [vp]),
    "gtars_tokenizer_chrom_name": (cstr, [vp, u32]),
    "gtars_tokenizer_index": (vp, [vp]),
    "gtars_tokenizer_encode_regionset": (C.c_int, [vp, vp, pp, pu64]),
    "gtars_tokenizer_encode_arrays": (C.c_int, [vp, vp, vp, vp, u64, pp, pu64]),
    "gtars_tokenizer_encode_ids": (C.c_int, [vp, vp, vp, vp, u64, vp, pp, pu64]),
    "gtars_tokenizer_encode_sets": (C.c_int, [vp, vp, u64, u64, pp, pp, pu64]),
    "gtars_tokenizer_encode_sets_ids": (C.c_int, [vp, vp, vp, vp, u64, vp, u64, u64, pp, pp, pu64]),
    "gtars_tokenizer_encode_sets_padded": (C.c_int, [vp, vp, vp, vp, u64, vp, u64, u64, u64, C.c_int, pp, pp, pu64]),
    "gtars_tokenizer_tokenize_fragment_file": (C.c_int, [vp, cstr, C.POINTER(C.POINTER(FragmentTokens))]),
    "gtars_fragment_tokens_free": (None, [C.POINTER(FragmentTokens)]),
    "gtars_fragment_tokens_barcodes_joined": (C.c_int, [C.POINTER(FragmentTokens), pp, pu64]),
    "gtars_barcode_map_from_file": (C.c_int, [cstr, pp]),
    "gtars_barcode_map_free": (None, [vp]),
    "gtars_barcode_map_len": (u64, [vp]),
    "gtars_barcode_map_n_clusters": (u32, [vp]),
    "gtars_barcode_map_cluster_label": (C.c_char_p, [vp, u32]),
    "gtars_barcode_map_lookup": (C.c_char_p, [vp, cstr]),
    "gtars_fragsplit": (C.c_int, [cstr, vp, cstr, pu64, pu64]),
    "gtars_fragsplit_tokenize": (C.c_int, [vp, cstr, vp, C.POINTER(C.POINTER(C.POINTER(FragmentTokens))), pu64]),
    "gtars_fragsplit_tokenize_files": (C.c_int, [vp, vp, u64, vp, C.POINTER(C.POINTER(C.POINTER(FragmentTokens))), pu64]),
    "gtars_host_threads": (u32, [u32]),
    "gtars_read_file": (C.c_int, [cstr, pp, pu64]),
    "gtars_fragsplit_last_stages": (None, [vp]),
    "gtars_fragsplit_last_inflate": (None, [vp]),
    "gtars_bgzf_members": (C.c_int, [vp, u64, u64, vp, vp, vp, vp, vp, vp, vp]),
    "gtars_gtok_write": (C.c_int, [cstr, vp, u64]),
    "gtars_gtok_read": (C.c_int, [cstr, pp, pu64]),
    "gtars_fragments_read": (C.c_int, [cstr, pp]),
    "gtars_fragments_read_strict": (C.c_int, [cstr, pp]),
    "gtars_bed3_lines_read": (C.c_int, [cstr, pp]),
    "gtars_format_hit_lines": (C.c_int, [vp, vp, vp, vp, u64, pp, pu64]),
    "gtars_fragments_free": (None, [vp]),
    "gtars_fragments_len": (u64, [vp]),
    "gtars_fragments_n_chrom": (u32, [vp]),
    "gtars_fragments_n_barcodes": (u32, [vp]),
    "gtars_fragments_chrom_name": (cstr, [vp, u32]),
    "gtars_fragments_barcode_name": (cstr, [vp, u32]),
    "gtars_fragments_chrom_ids": (vp, [vp]),
    "gtars_fragments_starts": (vp, [vp]),
    "gtars_fragments_ends": (vp, [vp]),
    "gtars_fragments_barcode_ids": (vp, [vp]),
    "gtars_igddb_from_bed_files": (C.c_int, [vp, u64, pp]),
    "gtars_igddb_from_bed_dir": (C.c_int, [cstr, pp]),
    "gtars_igddb_free": (None, [vp]),
    "gtars_igddb_n_files": (u32, [vp]),
    "gtars_igddb_n_contigs": (u32, [vp]),
    "gtars_igddb_file_name": (cstr, [vp, u32]),
    "gtars_igddb_file_num_regions": (u32, [vp, u32]),
    "gtars_igddb_file_avg_width": (C.c_double, [vp, u32]),
    "gtars_igddb_chrom_id": (i64, [vp, cstr]),
    "gtars_igddb_chrom_name": (cstr, [vp, u32]),
    "gtars_igddb_engine": (vp, [vp]),
    "gtars_igddb_count_regionset": (C.c_int, [vp, vp, i32, C.c_int, vp]),
    "gtars_igddb_from_arrays": (C.c_int, [vp, u32, vp, vp, vp, vp, vp, u64, vp, vp, vp, u32, pp]),
    "gtars_igddb_save": (C.c_int, [vp, cstr, i32]),
    "gtars_igddb_load": (C.c_int, [cstr, pp, C.POINTER(C.c_int32)]),
    "gtars_lola_stats": (C.c_int, [vp, vp, vp, vp, u64, u64, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "gtars_lola_rank": (C.c_int, [vp, vp, vp, u64, vp, vp, vp, vp, vp]),
    "gtars_lola_fdr": (C.c_int, [vp, vp, u64, vp]),
    "gtars_lola_fisher_pvalue": (C.c_double, [u64, u64, u64, u64, C.c_int]),
    "gtars_lola_odds_ratio": (C.c_double, [u64, u64, u64, u64]),
    "gtars_bam_open": (C.c_int, [cstr, pp]),
    "gtars_bam_close": (None, [vp]),
    "gtars_bam_header_text": (cstr, [vp]),
    "gtars_bam_n_ref": (u32, [vp]),
    "gtars_bam_ref_name": (cstr, [vp, u32]),
    "gtars_bam_ref_len": (u32, [vp, u32]),
    "gtars_bam_n_blocks": (u64, [vp]),
    "gtars_bam_n_bytes": (u64, [vp]),
    "gtars_bam_first_record": (u64, [vp]),
    "gtars_bam_block_table": (C.c_int, [vp, vp, vp, vp, vp, vp]),
    "gtars_bam_inflate": (C.c_int, [vp, u64, u64, vp, u64, u32]),
    "gtars_bam_record_offsets": (C.c_int, [vp, vp, u64, u64, C.c_int, pp, pu64, pu64]),
    "gtars_bam_decode": (C.c_int, [vp, u64, u64, u64, u32, pp, pu64]),
    "gtars_bam_qc": (C.c_int, [vp, u64, u32, vp]),
    "gtars_bam_last_stages": (None, [vp]),
    "gtars_bam_frag_params_default": (None, [vp]),
    "gtars_bam_fragments": (C.c_int, [vp, vp, u64, u32, pp]),
    "gtars_bam_frags_len": (u64, [vp]),
    "gtars_bam_frags_ref": (vp, [vp]),
    "gtars_bam_frags_start": (vp, [vp]),
    "gtars_bam_frags_end": (vp, [vp]),
    "gtars_bam_frags_barcode": (vp, [vp]),
    "gtars_bam_frags_count": (vp, [vp]),
    "gtars_bam_frags_n_barcodes": (u64, [vp]),
    "gtars_bam_frags_barcode_name": (vp, [vp, u64, pu64]),
    "gtars_bam_frags_stats": (None, [vp, vp]),
    "gtars_bam_frags_write": (C.c_int, [vp, vp, cstr]),
    "gtars_bam_frags_free": (None, [vp]),
    "gtars_fragments_write_text": (C.c_int, [cstr, vp, u32, vp, u64, vp, vp, vp, vp, vp, u64]),
    "gtars_sha512t24u": (C.c_int, [vp, u64, vp]),
    "gtars_vrs_location_digest": (C.c_int, [cstr, u64, u64, vp]),
    "gtars_vrs_allele_digest": (C.c_int, [cstr, u64, u64, vp, u64, vp]),
    "gtars_vrs_normalize": (C.c_int, [vp, u64, u64, vp, u64, vp, u64, pu64, pu64, pp, pu64]),
    "gtars_assembly_refget_digests": (C.c_int, [vp, u32, pp]),
    "gtars_vrs_alleles": (C.c_int, [vp, vp, vp, vp, vp, u64, vp, vp, vp, vp, u64, C.c_int, u32, vp, vp, vp, vp, pp, pp]),
    "gtars_vrs_ids_device": (C.c_int, [vp, vp, vp, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp, vp, vp, vp]),
    "gtars_vcf_read_alleles": (C.c_int, [vp, cstr, vp, u32, pp]),
    "gtars_vrs_from_vcf": (C.c_int, [vp, cstr, vp, C.c_int, u32, pp]),
    "gtars_vrs_results_free": (None, [vp]),
    "gtars_vrs_results_len": (u64, [vp]),
    "gtars_vrs_results_columns": (C.c_int, [vp, pp, pp, pp, pu64, pp, pp, pp, pp, pp]),
    "gtars_txbuilder_new": (C.c_int, [pp]),
    "gtars_txbuilder_free": (None, [vp]),
    "gtars_txbuilder_len": (u64, [vp]),
    "gtars_txbuilder_add": (C.c_int, [vp, cstr, cstr, cstr, C.c_int, u32, u32, u32, vp, u64]),
    "gtars_txbuilder_add_chrom_mapping": (C.c_int, [vp, cstr, cstr]),
    "gtars_txbuilder_add_mane": (C.c_int, [vp, cstr, u32]),
    "gtars_txbuilder_add_cdot": (C.c_int, [vp, cstr, cstr, cstr, i64, u32, u32, vp, u64, C.POINTER(C.c_int)]),
    "gtars_txbuilder_bytes": (C.c_int, [vp, pp, pu64]),
    "gtars_txbuilder_build": (C.c_int, [vp, cstr]),
    "gtars_txstore_open": (C.c_int, [cstr, pp]),
    "gtars_txstore_from_bytes": (C.c_int, [vp, u64, pp]),
    "gtars_txstore_free": (None, [vp]),
    "gtars_txstore_len": (u64, [vp]),
    "gtars_txstore_has_mane": (C.c_int, [vp]),
    "gtars_txstore_lookup": (i64, [vp, cstr]),
    "gtars_txstore_lookup_mane": (i64, [vp, cstr]),
    "gtars_txstore_lookup_many": (C.c_int, [vp, vp, vp, u64, u32, vp]),
    "gtars_txstore_record": (C.c_int, [vp, u64, pp, pp, vp, C.POINTER(C.c_int), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32),
                                       C.POINTER(u32), pp, pu64]),
    "gtars_txstore_map": (C.c_int, [vp, vp, vp, vp, vp, vp, u64, u32, vp, vp]),
    "gtars_txbind_new": (C.c_int, [vp, vp, u32, pp]),
    "gtars_txbind_free": (None, [vp]),
    "gtars_txbind_map": (C.c_int, [vp, vp, vp, vp, vp, vp, u64, C.c_int, u32, vp, vp]),
    "gtars_txbind_sequences": (C.c_int, [vp, vp, u64, C.c_int, u32, vp, vp, pp, pp]),
    "gtars_tx_map_device": (C.c_int, [vp, vp, vp, vp, vp, vp, u64, vp, vp, vp]),
    "gtars_tx_digests_device": (C.c_int, [vp, vp, u64, vp, vp, vp]),
    "gtars_hgvs_status_name": (cstr, [u32]),
    "gtars_hgvs_parse": (C.c_int, [vp, u64, vp, vp, pu64, vp, u64]),
    "gtars_hgvs_looks_like_gene_symbol": (C.c_int, [cstr]),
    "gtars_hgvs_resolve": (C.c_int, [vp, vp, vp, u64, vp, vp, vp, u64, u32, vp]),
    "gtars_hgvs_to_vrs": (C.c_int, [vp, vp, vp, u64, vp, vp, vp, u64, vp, C.c_int, u32, vp, vp, vp, vp, vp, vp, vp]),
    "gtars_hgvs_ids_device": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "gtars_hgvs_to_transcript_vrs": (C.c_int, [vp, vp, vp, u64, C.c_int, u32, vp, vp, vp, vp, vp, vp, vp, vp]),
    "gtars_hgvs_transcript_ids_device": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "gtars_vrs_transcript_ids": (C.c_int, [vp, vp, vp, vp, u64, vp, vp, vp, vp, u64, C.c_int, u32, vp, vp, vp, vp, vp]),
    "gtars_md5": (C.c_int, [vp, u64, vp]),
    "gtars_refget_alphabet": (C.c_int, [vp, u64]),
    "gtars_refget_class_table": (None, [vp]),
    "gtars_refget_host_len": (u32, []),
    "gtars_seqcol_from_fasta": (C.c_int, [cstr, C.c_int, u32, pp]),
    "gtars_seqcol_from_fasta_bytes": (C.c_int, [vp, u64, C.c_int, u32, pp]),
    "gtars_seqcol_free": (None, [vp]),
    "gtars_seqcol_len": (u64, [vp]),
    "gtars_seqcol_is_gzip": (C.c_int, [vp]),
    "gtars_seqcol_assembly": (vp, [vp]),
    "gtars_seqcol_record": (C.c_int, [vp, u64, pp, pp, pu64, C.POINTER(C.c_int), pu64, C.POINTER(u32), C.POINTER(u32), vp, vp,
                                      C.POINTER(C.c_int), pp]),
    "gtars_seqcol_digests": (C.c_int, [vp, vp]),
    "gtars_seqcol_substrings": (C.c_int, [vp, vp, vp, vp, u64, C.c_int, u32, vp, pp, pp]),
    "gtars_seqcol_digest_records": (C.c_int, [vp, C.c_int, u32, vp, vp, vp]),
    "gtars_refget_bits": (u32, [C.c_int]),
    "gtars_refget_encode": (C.c_int, [vp, u64, C.c_int, vp, u64, pu64]),
    "gtars_refget_decode": (C.c_int, [vp, u64, u64, u64, u64, C.c_int, vp]),
    "gtars_refget_byte_range": (None, [u64, u64, u32, pu64, pu64]),
    "gtars_seqpack_from_seqcol": (C.c_int, [vp, vp, C.c_int, u32, pp]),
    "gtars_seqpack_from_files": (C.c_int, [vp, vp, vp, u64, u32, pp]),
    "gtars_seqpack_from_buffers": (C.c_int, [vp, vp, vp, vp, u64, pp]),
    "gtars_seqpack_free": (None, [vp]),
    "gtars_seqpack_len": (u64, [vp]),
    "gtars_seqpack_device": (C.c_int, [vp]),
    "gtars_seqpack_image_bytes": (u64, [vp]),
    "gtars_seqpack_record": (C.c_int, [vp, u64, pp, pu64, pu64, C.POINTER(C.c_int)]),
    "gtars_seqpack_write_files": (C.c_int, [vp, vp, u32]),
    "gtars_seqpack_substrings": (C.c_int, [vp, vp, vp, vp, u64, C.c_int, u32, vp, pp, pp]),
    "gtars_seqpack_decode_records": (C.c_int, [vp, C.c_int, u32, pp, pp]),
    "gtars_seqcol_from_seq_files": (C.c_int, [vp, vp, u64, u32, pp]),
    "gtars_seqcol_from_buffers": (C.c_int, [vp, vp, u64, pp]),
    "gtars_seqcol_write_files": (C.c_int, [vp, vp, u32]),
}

# include/gtars_amd_debug.h: test / A-B / diagnostics hooks, not part of the drop-in boundary
_DEBUG_SIG = {
    "gtars_debug_occupy_device": (C.c_int, [vp, u32, u32, u32]),
    "gtars_debug_reload_env": (None, []),
    "gtars_debug_set_handle_device": (C.c_int, [vp, C.c_int, C.c_int]),
    "gtars_debug_set_assembly_device": (C.c_int, [vp, C.c_int]),
    "gtars_debug_inflate_streams": (C.c_int, [vp, vp, vp, vp, vp, vp, u32, vp, vp, vp, vp]),
    "gtars_debug_inflate_members": (C.c_int, [vp, vp, vp, vp, vp, vp, u32, vp, vp, vp, u32, vp]),
    "gtars_debug_sort_perm": (C.c_int, [vp, vp, vp, u64, u32, vp]),
    "gtars_debug_scan_u32": (C.c_int, [vp, u64, vp]),
    "gtars_debug_seg_max": (C.c_int, [vp, vp, vp, u64, u32, C.c_int, vp]),
    "gtars_debug_signal_sort_elems": (u32, [u32]),
    "gtars_debug_signal_split_hits": (u32, []),
    "gtars_debug_tokbatch_tile": (u32, []),
    "gtars_debug_grid_clips": (u64, []),
    "gtars_debug_seq_stage_blocks": (u64, []),
}

# every symbol the headers declare must resolve -- fail loudly otherwise (GTARS_AMD_LIB_OLDER=1, A/B tooling only: an older
# build loaded through GTARS_AMD_LIB may lack the newest entry points; calling one of those then fails at the call)
_older = bool(os.environ.get("GTARS_AMD_LIB")) and os.environ.get("GTARS_AMD_LIB_OLDER") == "1"
for _table in (_SIG, _HOST_SIG, _DEBUG_SIG):
    for _name, (_res, _args) in _table.items():
        if _older and not hasattr(lib, _name):
            continue
        _fn = getattr(lib, _name)
        _fn.restype = _res
        _fn.argtypes = _args

EXPORTED_SYMBOLS = tuple(_SIG)
EXPORTED_HOST_SYMBOLS = tuple(_HOST_SIG)
EXPORTED_DEBUG_SYMBOLS = tuple(_DEBUG_SIG)


def cstr_array(strings):
    """list[str] -> (char*[] ctypes array, keepalive)."""
    enc = [s.encode("utf-8") if s is not None else None for s in strings]
    arr = (C.c_char_p * max(len(enc), 1))(*enc)
    return arr, enc


def dec(b):
    return None if b is None else b.decode("utf-8", "replace")


def last_error() -> str:
    return (lib.gtars_last_error() or b"").decode("utf-8", "replace")


def check(status: int):
    if status == GTARS_OK:
        return
    msg = last_error()
    if status == ERR_NO_DEVICE:
        raise NoDeviceError(status, msg)
    if status == ERR_CAPACITY:
        raise CapacityError(status, msg)
    if status == ERR_IO:
        raise FileNotFoundError(msg)
    if status in (ERR_PARSE, ERR_EMPTY, ERR_CONFIG, ERR_INVALID_ARG):
        raise ValueError(msg)
    raise GtarsError(status, msg)


def device_count() -> int:
    return int(lib.gtars_device_count())


def as_u32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint32)


def ptr(a: np.ndarray):
    return C.c_void_p(a.ctypes.data) if a.size else C.c_void_p(0)


def take_u32(p: C.c_void_p, n: int) -> np.ndarray:
    """Copy a library-allocated u32 array into numpy and free it."""
    try:
        if n == 0 or not p.value:
            return np.zeros(0, dtype=np.uint32)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n,)).copy()
    finally:
        if p.value:
            lib.gtars_free(p)


def take_array(p: C.c_void_p, n: int, ctype, dtype) -> np.ndarray:
    """Copy a library-allocated array of n elements into numpy and free it."""
    try:
        if n == 0 or not p.value:
            return np.zeros(0, dtype=dtype)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(n,)).copy()
    finally:
        if p.value:
            lib.gtars_free(p)


def prof_read():
    cap = 64
    names = (C.c_char_p * cap)()
    ms = (C.c_double * cap)()
    launches = (C.c_uint64 * cap)()
    n = lib.gtars_prof_read(C.cast(names, vp), C.cast(ms, vp), C.cast(launches, vp), cap)
    return {names[i].decode(): {"total_ms": ms[i], "launches": int(launches[i])} for i in range(min(n, cap))}


def reload_env() -> None:
    """The library reads its GTARS_* switches ONCE, into a snapshot taken at first use; a process that changes one afterwards
    (tests, A/B harnesses) calls this to make the library take a new snapshot.  No library call may be in flight."""
    lib.gtars_debug_reload_env()


# -- the device primitives through their test entries (include/gtars_amd_debug.h) --------------------------------------
def debug_sort_perm(chrom, k1, k2, n_chrom: int) -> np.ndarray:
    """perm such that (chrom, k1, [k2], input row) ascends, from the device radix sort"""
    chrom, k1 = as_u32(chrom), as_u32(k1)
    k2 = None if k2 is None else as_u32(k2)
    if len(k1) != len(chrom) or (k2 is not None and len(k2) != len(chrom)):
        raise ValueError("key columns must have the same length")
    perm = np.zeros(len(chrom), dtype=np.uint32)
    check(lib.gtars_debug_sort_perm(ptr(chrom), ptr(k1), ptr(k2) if k2 is not None else None, len(chrom), int(n_chrom), ptr(perm)))
    return perm


def debug_scan_u32(counts) -> np.ndarray:
    """n + 1 exclusive u64 offsets of n u32 counts, from the device's three-phase scan"""
    counts = as_u32(counts)
    out = np.zeros(len(counts) + 1, dtype=np.uint64)
    check(lib.gtars_debug_scan_u32(ptr(counts), len(counts), ptr(out)))
    return out


def debug_seg_max(seg, val, start=None, gap: int = 0, inclusive: bool = True) -> np.ndarray:
    """the segmented max-scan: the running maximum since the segment head (inclusive), or the run-opening flags"""
    seg, val = as_u32(seg), as_u32(val)
    start = None if start is None else as_u32(start)
    if len(val) != len(seg) or (start is not None and len(start) != len(seg)):
        raise ValueError("columns must have the same length")
    out = np.zeros(len(seg), dtype=np.uint32)
    check(lib.gtars_debug_seg_max(ptr(seg), ptr(val), ptr(start) if start is not None else None, len(seg), int(gap),
                                  1 if inclusive else 0, ptr(out)))
    return out
