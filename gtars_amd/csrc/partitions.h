// partitions.h -- internal interface of partitions.hip (K14: classifying query regions into genomic partitions) for the
// host layer.  Plain C++: partitions.cpp includes it without the HIP headers.  Chromosomes are ids of the partition
// list's dictionary; the host maps a query's chromosome ids onto them.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/gtars_amd.h"

namespace gtars {

constexpr uint32_t PART_MAX = 255;  // partitions of a list: an assignment is a u8 and the list's length is "intergenic"

// the rows of every partition of a list on one device, segment (p, c) = the rows of partition p on chromosome id c
struct PartDevice;

// One partition's rows as host columns, chrom[i] < n_chrom
struct PartCols {
    const uint32_t *chrom, *start, *end;
    uint64_t n;
};

// On the current device: per segment the starts sorted (with each row's own end next to it), the ends sorted on their
// own, and a u64 exclusive prefix sum of either.  Rows with start > end are kept apart in a side list.
gtars_status part_build(const std::vector<PartCols> &parts, uint32_t n_chrom, PartDevice **out);
void part_free(PartDevice *d);
int part_device(const PartDevice *d);

// calc_partitions (gtars-genomicdist/src/partitions.rs:506-592) over n query rows, on the index's device.
// seg_of[c]: the list chromosome of query chromosome id c, or UINT32_MAX (absent: no partition hits).
//   bp == false: out[p] = queries whose first hit partition (list order) is p, out[P] = queries without a hit;
//                assign (optional, n entries): that bucket per query, in input order
//   bp == true:  out[p] = sum over the queries and the rows of p they hit of the overlap width, out[P] = sum of the
//                queries' (u32)(end - start); assign must be null
// All sums are u64: the reference's u32 wrap is the caller's.
gtars_status part_count(const PartDevice *d, const uint32_t *q_chrom, const uint32_t *q_start, const uint32_t *q_end, uint64_t n,
                        const std::vector<uint32_t> &seg_of, bool bp, uint64_t *out, uint8_t *assign);
// the same for n device rows whose chromosome ids are the list's (any id >= n_chrom: absent), queued on `stream` of the
// current device, which must be the index's; d_assign (optional) is a device pointer.  The stream is drained.
gtars_status part_count_device(const PartDevice *d, const uint32_t *d_chrom, const uint32_t *d_start, const uint32_t *d_end,
                               uint64_t n, bool bp, uint64_t *out, uint8_t *d_assign, void *stream);

}  // namespace gtars
