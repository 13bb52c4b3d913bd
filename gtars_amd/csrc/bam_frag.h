// bam_frag.h -- K26 between its device pipeline (bam.hip) and its host layer (bam_frag.cpp): the result
// handle and the fragment text.  No HIP types here.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/gtars_amd_host.h"

// what gtars_bam_fragments returns: the collapsed rows in (ref, start, end, barcode) order, all on the host
struct gtars_bam_frags {
    std::vector<int32_t> ref;
    std::vector<uint32_t> start, end, barcode, count;
    std::vector<std::string> barcodes;  // in id order: the byte order of the distinct barcodes
    uint64_t stats[GTARS_BAM_FRAG_N_STATS] = {};
};

namespace gtars {

// `chrom \t start \t end \t barcode \t count \n` per row; numbers by the decimal formatting of bed_text_core.h, the rows cut
// over `threads` host threads.  ref and barcode must name entries of the two tables (GTARS_ERR_INVALID_ARG otherwise).
gtars_status bam_frag_text(const std::vector<std::string> &ref_names, const std::vector<std::string> &barcodes, const int32_t *ref,
                           const uint32_t *start, const uint32_t *end, const uint32_t *barcode, const uint32_t *count, uint64_t n, unsigned threads,
                           std::string &text);

}  // namespace gtars
