// setops.h -- internal interface of setops.hip (K8: region-set algebra on the device) for the host layer.
// Plain C++: host.cpp includes it without the HIP headers.  Every set is given as host columns (rank, start, end):
// `rank` is the chromosome's position in the bytewise order of the names the call involves, so that sorting by rank
// is sorting by name as the reference does (gtars-core/src/models/region_set.rs:502-505).
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/gtars_amd.h"

namespace gtars {

struct SetCols {
    const uint32_t *rank;
    const uint32_t *start;
    const uint32_t *end;
    uint64_t n;
};

struct SetOut {
    std::vector<uint32_t> rank, start, end;
};

// reduce(): stable sort by (rank, start), merge while next.start <= current.end
gtars_status setops_reduce(const SetCols &a, uint32_t n_rank, SetOut &out);
// IntervalSetOps::setdiff / intersect (region_set.rs:1229-1370): both sets reduced, one sweep per chromosome of `a`
gtars_status setops_setdiff(const SetCols &a, const SetCols &b, uint32_t n_rank, SetOut &out);
gtars_status setops_intersect(const SetCols &a, const SetCols &b, uint32_t n_rank, SetOut &out);
// the bp totals behind jaccard / coverage / overlap_coefficient (region_set.rs:1383-1415), each a wrapping u32 sum of
// (u32)(end - start): reduce(a), reduce(b), reduce(concat(a, b)), setdiff(a, b).  `want_diff`: compute diff_bp too.
struct SetTotals {
    uint32_t a_bp = 0, b_bp = 0, union_bp = 0, diff_bp = 0;
};
gtars_status setops_totals(const SetCols &a, const SetCols &b, uint32_t n_rank, bool want_diff, SetTotals &out);
// RegionSet::closest (region_set.rs:1132-1225); a.rank == UINT32_MAX: chromosome absent from `other`
gtars_status setops_closest(const SetCols &a, const SetCols &other, uint32_t n_rank, std::vector<uint32_t> &self_idx,
                            std::vector<uint32_t> &other_idx, std::vector<int64_t> &dist);
// RegionSet::cluster (region_set.rs:1093-1129): ids in input order
gtars_status setops_cluster(const SetCols &a, uint32_t n_rank, uint32_t max_gap, uint32_t *ids);
// RegionSetList::pairwise_jaccard: out[i * n + j] == reduce(S_i).jaccard(reduce(S_j)), 1.0 on the diagonal
gtars_status setops_pairwise_jaccard(const std::vector<SetCols> &sets, uint32_t n_rank, double *out);

}  // namespace gtars
