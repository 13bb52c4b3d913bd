// annot.h -- internal interface of annot.hip (K10: distances to the nearest TSS / feature midpoint) for the host layer.
// Plain C++: host.cpp includes it without the HIP headers.  Chromosomes are the index set's dictionary ids; the host maps
// a query's chromosome ids onto them.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/gtars_amd.h"

namespace gtars {

// the sorted midpoints of an index set on one device, segment c = the midpoints of chromosome id c
struct TssDevice;

// TssIndex::from_region_set (gtars-genomicdist/src/models.rs:533-549), on the current device: midpoints
// start + (u32)(end - start) / 2 (wrapping), sorted by (chromosome, midpoint), duplicates kept.  chrom[i] < n_chrom.
gtars_status tss_build(const uint32_t *chrom, const uint32_t *start, const uint32_t *end, uint64_t n, uint32_t n_chrom,
                       TssDevice **out);
void tss_free(TssDevice *t);
int tss_device(const TssDevice *t);

// calc_tss_distances / calc_feature_distances (models.rs:588-690), both in one pass, on the index's device.
// seg_of[c]: the index chromosome of query chromosome id c, or UINT32_MAX (absent: u32::MAX / INT64_MAX).
// grouped: the query's chromosome ids never decrease, so input order is output order; otherwise the results come in a
// stable order by chromosome id (the ids are first-appearance ranks).  out_abs / out_signed: nq entries each.
gtars_status tss_distances(const TssDevice *t, const uint32_t *q_chrom, const uint32_t *q_start, const uint32_t *q_end,
                           uint64_t nq, const std::vector<uint32_t> &seg_of, bool grouped, uint32_t *out_abs,
                           int64_t *out_signed);

}  // namespace gtars
