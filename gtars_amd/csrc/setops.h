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

// RegionSetListOps (gtars-genomicdist/src/region_set_list_ops.rs:103-181) for lists of >= 2 sets; the host layer answers
// the shorter ones.  union_except: reduce of the concatenation of every set but `skip` (skip >= sets.size(): of all).
gtars_status setops_list_union_all(const std::vector<SetCols> &sets, uint32_t n_rank, SetOut &out);
gtars_status setops_list_union_except(const std::vector<SetCols> &sets, uint32_t n_rank, uint64_t skip, SetOut &out);
// uni = reduce(concat), except[i] = reduce(concat without set i), all from one sort and one top-2-by-owner scan
gtars_status setops_list_bulk_union_except(const std::vector<SetCols> &sets, uint32_t n_rank, SetOut &uni, std::vector<SetOut> &except);
// the left fold of intersect: the stretches of positive length that every set's own reduce covers
gtars_status setops_list_intersect_all(const std::vector<SetCols> &sets, uint32_t n_rank, SetOut &out);

// GTARS_ERR_NO_DEVICE unless a device is visible (common.h)
gtars_status require_device();

// ---- K9: structural operations and region-set statistics (gtars-genomicdist) -----------------------------------------
// RegionSet::disjoin (region_set.rs:1051-1090): pieces between consecutive boundaries (every start and end) of a
// chromosome that some well-formed region (start < end) covers, in (rank, start) order
gtars_status setops_disjoin(const SetCols &a, uint32_t n_rank, SetOut &out);
// RegionSet::gaps (region_set.rs:786-878).  size[r]: chromosome size of rank r, 0 where it is absent or 0 (nothing is
// emitted for it); group[r] < n_group: its karyotype key's position among the keys.  Out: (group, start, rank) order.
gtars_status setops_gaps(const SetCols &a, uint32_t n_rank, const std::vector<uint32_t> &size, const std::vector<uint32_t> &group,
                         uint32_t n_group, SetOut &out);
// consensus (gtars-genomicdist/src/consensus.rs:29-68): reduce of the concatenation, and for each run the number of
// sets with a region that hits it (start < run.end && run.start < end)
gtars_status setops_consensus(const std::vector<SetCols> &sets, uint32_t n_rank, SetOut &uni, std::vector<uint32_t> &count);
// calc_neighbor_distances / calc_nearest_neighbors (statistics.rs:258-316); rank: first appearance in the set
gtars_status setops_neighbor_distances(const SetCols &a, uint32_t n_rank, std::vector<int64_t> &out);
gtars_status setops_nearest_neighbors(const SetCols &a, uint32_t n_rank, std::vector<uint32_t> &out);
// region_distribution_with_bins / _with_chrom_sizes (statistics.rs:143-256): regions counted per (rank, rid) of their
// midpoint.  with_sizes: limit[r] is the chromosome size (0: absent), regions with midpoint >= it are skipped and rid is
// clamped to n_bins - 1.  Out: the occupied (rank, rid) keys in ascending order and their counts.
gtars_status setops_distribution(const SetCols &a, uint32_t n_rank, uint32_t n_bins, uint32_t bin_size, bool with_sizes,
                                 const std::vector<uint32_t> &limit, std::vector<uint32_t> &rank, std::vector<uint32_t> &rid,
                                 std::vector<uint32_t> &count);
// chromosome_statistics (statistics.rs:88-141), one entry per rank; count == 0: the rank holds no region
struct ChromStat {
    uint32_t count, min_start, max_end, min_width, max_width;
    double mean, median;
};
gtars_status setops_chrom_stats(const SetCols &a, uint32_t n_rank, std::vector<ChromStat> &out);

}  // namespace gtars
