// setops.hip -- K8: region-set algebra on the device (gtars-core/src/models/region_set.rs:675-1420,
// gtars-genomicdist/src/region_set_list_ops.rs:20-45): reduce / union, setdiff / intersect, the bp totals behind
// jaccard / coverage / overlap_coefficient, closest, cluster, the pairwise Jaccard matrix of a list of sets, and the folds
// over a list (union_all, intersect_all, union_except, bulk_union_except).
//
// Building blocks, all on the calling thread's current device and its null stream (drained on every exit):
//   * the stable radix sort of sort.hip: (rank, start) for reduce and closest, (rank, start, end) for cluster;
//   * a segmented max-scan of the ends over u32 (tile aggregates, one workgroup scanning them, a re-scan per tile).
//     A run (reduce) or cluster opens where start > (exclusive running max of end over the chromosome) [+ max_gap,
//     saturating]: every earlier run ended before the start that closed it, so this is the reference's sequential
//     rule.  The run's end is a second max-scan, segmented by run (a run of one inverted region ends below the ends
//     of earlier runs, so the chromosome-wide maximum is not it);
//   * count / exclusive scan / write (CSR) for the sweeps, one lane per region of `a` with two binary searches.  A
//     reduced set without inverted regions (start > end) has strictly increasing starts and ends, and there the
//     reference's monotone b_idx is the lower bound on end.  A chromosome where either reduced set still holds an
//     inverted region is swept by one lane, exactly as the reference does;
//   * pairwise Jaccard: all sets reduced in one pass (segments = set x chromosome), per-set prefix sums of widths, and
//     for a pair the covered bp of S_j before p as one binary search: |S_i & S_j| = sum over x in S_i of
//     F_j(x.end) - F_j(x.start).  One work list of (smaller set, other set, chunk) items covers every pair.
//   * folds over a list (region_set_list_ops.rs:103-181; the second part of K8, after K9 in this file): union_all and
//     union_except(i) are one reduce of the concatenation (without set i); bulk_union_except gives the union of all and
//     every union_except(i) from one upload, one sort and one segmented scan whose value is the top two ends by owner
//     (m1, the set s1 that attains it, m2 over the other sets): the running maximum without set i is s1 == i ? m2 : m1,
//     reduce's rule is applied with it, and one workgroup per tile of sorted rows counts, then writes, the runs of every
//     output set (a compare, a ballot and a popcount per set and 64 rows).  intersect_all reduces every set in one pass
//     (segment = set x chromosome), drops the reduced regions with start >= end and sweeps the open / close events
//     sorted by (rank, position): a stretch is emitted where the depth is the number of sets.  This is the reference's
//     left fold exactly, inverted regions included, and needs no sequential path: in sweep_intersect_chr a region with
//     start >= end yields no piece on either side (max(starts) >= min(ends)), it never hides a later region from the
//     sweep (a's starts ascend, and a b region is skipped only once its end is at or below the current start), and the
//     well-formed regions of a reduced set keep gaps >= 1 (each opened past every earlier end), so every step's result
//     is sorted, separated and its own reduce;
// Widths and totals are the reference's release-build u32 values: (u32)(end - start), summed modulo 2^32 (u64 on the
// device, truncated), and the intersection is a_bp + b_bp - union_bp in wrapping u32.
// K9 (the second half of the file) builds disjoin, gaps, consensus and the region-set statistics of gtars-genomicdist
// from the same blocks; DESIGN.md §3 K9.
#include <algorithm>
#include <limits>
#include <vector>

#include "common.h"
#include "../../include/gtars_amd_debug.h"
#include "pipeline.h"
#include "scan.h"
#include "setops.h"

namespace gtars {
namespace {

constexpr int SO_TPB = 256;
constexpr int SO_IPT = 8;
constexpr u32 SO_TILE = SO_TPB * SO_IPT;
constexpr u32 SO_PAIR_CHUNK = 2048;  // regions of the smaller set per work item of the pairwise kernel
constexpr u32 SO_MAX_N = 0xFFFFF000u;
enum { SWEEP_SETDIFF = 0, SWEEP_INTERSECT = 1 };

// ---------------------------------------------------------------------------------------------- segmented max-scan
using SMax = SegMax<u32>;  // f: a segment head lies in the span; v: max of the values since the last head
__device__ __forceinline__ u32 is_head(const u32 *__restrict__ seg, u64 i) { return i == 0 || seg[i] != seg[i - 1]; }

// a thread's SO_IPT elements folded in order; elements past n are the identity
__device__ __forceinline__ SMax::T sm_thread(const u32 *__restrict__ seg, const u32 *__restrict__ val, u32 n, u64 base) {
    SMax::T acc = SMax::identity();
#pragma unroll
    for (int k = 0; k < SO_IPT; ++k)
        if (base + k < n) acc = SMax::op(acc, SMax::T{is_head(seg, base + k), val[base + k]});
    return acc;
}

__global__ void __launch_bounds__(SO_TPB)
k_sm_tiles(const u32 *__restrict__ seg, const u32 *__restrict__ val, u32 n, SMax::T *__restrict__ agg) {
    __shared__ SMax::T lds[SO_TPB / 64];
    const u64 base = (u64)blockIdx.x * SO_TILE + (u64)threadIdx.x * SO_IPT;
    SMax::T excl, total;
    (void)block_scan<SMax, SO_TPB>(sm_thread(seg, val, n, base), lds, excl, total);
    if (threadIdx.x == 0) agg[blockIdx.x] = total;
}

// tile aggregates -> exclusive carries, in place (one workgroup)
__global__ void __launch_bounds__(1024) k_sm_carry(SMax::T *__restrict__ agg, u32 n_tiles) {
    __shared__ SMax::T lds[1024 / 64];
    (void)carry_walk<SMax>(agg, n_tiles, lds);
}

// INCL: out[i] = max of val over [segment head, i].  Else: out[i] = 1 where i opens a run: a head, or
// start[i] > sat(max of val over [head, i) + gap).
template <bool INCL>
__global__ void __launch_bounds__(SO_TPB)
k_sm_apply(const u32 *__restrict__ seg, const u32 *__restrict__ val, const u32 *__restrict__ start, u32 n,
           const SMax::T *__restrict__ carry, u32 gap, u32 *__restrict__ out) {
    __shared__ SMax::T lds[SO_TPB / 64];
    const u64 base = (u64)blockIdx.x * SO_TILE + (u64)threadIdx.x * SO_IPT;
    SMax::T excl, total;
    (void)block_scan<SMax, SO_TPB>(sm_thread(seg, val, n, base), lds, excl, total);
    SMax::T run = SMax::op(carry[blockIdx.x], excl);
#pragma unroll
    for (int k = 0; k < SO_IPT; ++k) {
        const u64 i = base + k;
        if (i >= n) break;
        const SMax::T x{is_head(seg, i), val[i]};
        if (INCL) {
            run = SMax::op(run, x);
            out[i] = run.v;
        } else {
            const u32 lim = run.v > 0xFFFFFFFFu - gap ? 0xFFFFFFFFu : run.v + gap;  // saturating_add
            out[i] = (x.f || start[i] > lim) ? 1u : 0u;
            run = SMax::op(run, x);
        }
    }
}

gtars_status seg_max_pass(StreamFrame &fr, bool incl, const u32 *seg, const u32 *val, const u32 *start, u32 n, u32 gap, u32 *out) {
    if (!n) return GTARS_OK;
    hipStream_t st = fr.st;
    const u32 tiles = (n + SO_TILE - 1) / SO_TILE;
    SMax::T *agg = nullptr;
    GT_TRY(fr.alloc(&agg, tiles));
    hipLaunchKernelGGL(k_sm_tiles, dim3(tiles), dim3(SO_TPB), 0, st, seg, val, n, agg);
    hipLaunchKernelGGL(k_sm_carry, dim3(1), dim3(1024), 0, st, agg, tiles);
    if (incl)
        hipLaunchKernelGGL(k_sm_apply<true>, dim3(tiles), dim3(SO_TPB), 0, st, seg, val, start, n, agg, gap, out);
    else
        hipLaunchKernelGGL(k_sm_apply<false>, dim3(tiles), dim3(SO_TPB), 0, st, seg, val, start, n, agg, gap, out);
    GT_HIP(hipGetLastError());
    return GTARS_OK;
}

// ------------------------------------------------------------------------------------------------ small kernels
__global__ void k_gather3(const u32 *__restrict__ perm, u32 n, const u32 *__restrict__ a, const u32 *__restrict__ b,
                          const u32 *__restrict__ c, u32 *__restrict__ oa, u32 *__restrict__ ob, u32 *__restrict__ oc) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u32 p = perm[i];
        oa[i] = a[p];
        ob[i] = b[p];
        oc[i] = c[p];
    }
}

__global__ void k_run_ids(const u32 *__restrict__ flag, const u64 *__restrict__ off, u32 n, u32 *__restrict__ rid) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
        rid[i] = (u32)(off[i] + flag[i] - 1);
}

__global__ void k_reduce_write(const u32 *__restrict__ seg, const u32 *__restrict__ start, const u32 *__restrict__ flag,
                               const u32 *__restrict__ rid, const u32 *__restrict__ run_max, u32 n, u32 *__restrict__ oseg,
                               u32 *__restrict__ ostart, u32 *__restrict__ oend) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u32 r = rid[i];
        if (flag[i]) {
            oseg[r] = seg[i];
            ostart[r] = start[i];
        }
        if (i + 1 == n || rid[i + 1] != r) oend[r] = run_max[i];
    }
}

// off[r] = first position with seg >= r, r in [0, n_seg]; seg sorted ascending, every value < n_seg
__global__ void k_seg_offsets(const u32 *__restrict__ seg, u32 n, u32 n_seg, u32 *__restrict__ off) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (u64)gridDim.x * blockDim.x) {
        const u64 lo = i == 0 ? 0 : (u64)seg[i - 1] + 1;
        const u64 hi = i == n ? n_seg : seg[i];
        for (u64 r = lo; r <= hi; ++r) off[r] = (u32)i;
    }
}

// dirty[seg / div] = 1 for every inverted region (start > end)
__global__ void k_mark_inverted(const u32 *__restrict__ seg, const u32 *__restrict__ start, const u32 *__restrict__ end, u32 n,
                                u32 div, u32 *__restrict__ dirty) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
        if (start[i] > end[i]) dirty[seg[i] / div] = 1u;
}

// sum of (u32)(end - start) in u64
__global__ void k_sum_widths(const u32 *__restrict__ start, const u32 *__restrict__ end, u32 n, u64 *__restrict__ acc) {
    u64 s = 0;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) s += (u32)(end[i] - start[i]);
    s = wave_reduce_sum_u64(s);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd((unsigned long long *)acc, (unsigned long long)s);
}

__global__ void k_widths(const u32 *__restrict__ start, const u32 *__restrict__ end, u32 n, u32 *__restrict__ w) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) w[i] = end[i] - start[i];
}

// ------------------------------------------------------------------------------------------------------- reduce
struct DevSet {
    u32 *seg = nullptr, *start = nullptr, *end = nullptr;
    u32 n = 0;
};

// what a reduce leaves behind for callers that work on the members of the runs: the sort permutation, the sorted
// columns and each sorted region's run (an index into the reduced set)
struct ReduceWork {
    u32 *perm = nullptr, *sseg = nullptr, *sstart = nullptr, *send = nullptr, *rid = nullptr;
};

// a set of n rows whose three columns belong to the frame
gtars_status alloc_set(StreamFrame &fr, u64 n, DevSet &s) {
    s.n = (u32)n;
    GT_TRY(fr.alloc(&s.seg, n));
    GT_TRY(fr.alloc(&s.start, n));
    return fr.alloc(&s.end, n);
}

gtars_status upload_set(StreamFrame &fr, const SetCols &a, DevSet &s) {
    s.n = (u32)a.n;
    GT_TRY(fr.upload(&s.seg, a.rank, a.n));
    GT_TRY(fr.upload(&s.start, a.start, a.n));
    return fr.upload(&s.end, a.end, a.n);
}

// the rows of n_sets host sets one after the other in one device set
gtars_status upload_concat(StreamFrame &fr, const SetCols *sets, size_t n_sets, DevSet &out) {
    u64 n = 0;
    for (size_t k = 0; k < n_sets; ++k) n += sets[k].n;
    GT_TRY(alloc_set(fr, n, out));
    u64 at = 0;
    for (size_t k = 0; k < n_sets; ++k) {
        const SetCols &s = sets[k];
        GT_TRY(fr.upload_to(out.seg + at, s.rank, s.n));
        GT_TRY(fr.upload_to(out.start + at, s.start, s.n));
        GT_TRY(fr.upload_to(out.end + at, s.end, s.n));
        at += s.n;
    }
    return GTARS_OK;
}

// queued, not drained: `out` holds the rows after fr.drain()
gtars_status download(StreamFrame &fr, const DevSet &d, SetOut &out) {
    GT_TRY(fr.download(out.rank, d.seg, d.n));
    GT_TRY(fr.download(out.start, d.start, d.n));
    return fr.download(out.end, d.end, d.n);
}

// the rows of `in` stably sorted by (key_seg, start[, key2]) and gathered, key_seg < n_seg; *perm (optional): the order
gtars_status sorted_set(StreamFrame &fr, const DevSet &in, const u32 *key_seg, const u32 *key2, u32 n_seg, DevSet &out,
                        u32 **perm = nullptr) {
    u32 *p;
    GT_TRY(sort_perm(fr, key_seg, in.start, key2, in.n, n_seg, &p));
    GT_TRY(alloc_set(fr, in.n, out));
    hipLaunchKernelGGL(k_gather3, dim3(grid_for(in.n)), dim3(256), 0, fr.st, p, in.n, in.seg, in.start, in.end, out.seg, out.start,
                       out.end);
    GT_HIP(hipGetLastError());
    if (perm) *perm = p;
    return GTARS_OK;
}

// reduce() of the device regions `in` (unsorted) whose segment keys are < n_seg
gtars_status dev_reduce(StreamFrame &fr, const DevSet &in, u32 n_seg, DevSet &out, ReduceWork *work = nullptr) {
    out = DevSet();
    if (work) *work = ReduceWork();
    const u32 n = in.n;
    if (!n) return GTARS_OK;
    hipStream_t st = fr.st;
    DevSet S;
    u32 *perm, *flag, *rid, *rmax;
    GT_TRY(sorted_set(fr, in, in.seg, nullptr, n_seg, S, &perm));  // (segment, start), ties in input order
    GT_TRY(fr.alloc(&flag, n));
    GT_TRY(seg_max_pass(fr, false, S.seg, S.end, S.start, n, 0, flag));
    u64 *off, m = 0;
    GT_TRY(scan_total(fr, flag, n, &off, &m));
    GT_TRY(fr.alloc(&rid, n));
    hipLaunchKernelGGL(k_run_ids, dim3(grid_for(n)), dim3(256), 0, st, flag, off, n, rid);
    GT_TRY(fr.alloc(&rmax, n));
    GT_TRY(seg_max_pass(fr, true, rid, S.end, nullptr, n, 0, rmax));
    GT_TRY(alloc_set(fr, m, out));
    hipLaunchKernelGGL(k_reduce_write, dim3(grid_for(n)), dim3(256), 0, st, S.seg, S.start, flag, rid, rmax, n, out.seg, out.start,
                       out.end);
    GT_HIP(hipGetLastError());
    if (work) *work = ReduceWork{perm, S.seg, S.start, S.end, rid};
    return GTARS_OK;
}

gtars_status check_sizes(u64 n, u32 n_rank) {
    if (n > SO_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "region set too large for the device set operations (" + std::to_string(n) + " regions)");
    if (n_rank > 0x7FFFFFFFu) return fail(GTARS_ERR_INVALID_ARG, "too many chromosomes");
    return require_device();
}

gtars_status reduce_cols(StreamFrame &fr, const SetCols &a, u32 n_rank, DevSet &out) {
    DevSet in;
    GT_TRY(upload_set(fr, a, in));
    return dev_reduce(fr, in, n_rank, out);
}

// ------------------------------------------------------------------------------------------- setdiff / intersect
template <int MODE, bool WRITE>
__device__ __forceinline__ void emit(u32 &c, u64 o, u32 r, u32 s, u32 e, u32 *oseg, u32 *os, u32 *oe) {
    if (WRITE) {
        oseg[o + c] = r;
        os[o + c] = s;
        oe[o + c] = e;
    }
    ++c;
}

// one lane per region of reduced `a` on a chromosome where neither reduced set holds an inverted region
template <int MODE, bool WRITE>
__global__ void k_sweep_par(const u32 *__restrict__ aseg, const u32 *__restrict__ as, const u32 *__restrict__ ae, u32 na,
                            const u32 *__restrict__ bs, const u32 *__restrict__ be, const u32 *__restrict__ boff,
                            const u32 *__restrict__ dirty, u32 *__restrict__ cnt, const u64 *__restrict__ off, u32 *__restrict__ oseg,
                            u32 *__restrict__ os, u32 *__restrict__ oe) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < na; i += (u64)gridDim.x * blockDim.x) {
        const u32 r = aseg[i];
        if (dirty[r]) continue;
        const u32 s = as[i], e = ae[i], lo = boff[r], hi = boff[r + 1];
        const u32 j0 = first_gt(be, lo, hi, s);  // the sweep's b_idx: first b with end > a.start
        const u32 j1 = first_ge(bs, j0, hi, e);  // the first b with start >= a.end ends the inner loop
        const u64 o = WRITE ? off[i] : 0;
        u32 c = 0;
        if (MODE == SWEEP_SETDIFF) {
            u32 pos = s;
            for (u32 j = j0; j < j1 && pos < e; ++j) {
                if (bs[j] > pos) emit<MODE, WRITE>(c, o, r, pos, bs[j], oseg, os, oe);
                pos = max(pos, be[j]);
            }
            if (pos < e) emit<MODE, WRITE>(c, o, r, pos, e, oseg, os, oe);
        } else {
            for (u32 j = j0; j < j1; ++j) {
                const u32 ps = max(s, bs[j]), pe = min(e, be[j]);
                if (ps < pe) emit<MODE, WRITE>(c, o, r, ps, pe, oseg, os, oe);
            }
        }
        if (!WRITE) cnt[i] = c;
    }
}

// one lane per chromosome that holds an inverted region: sweep_setdiff_chr / sweep_intersect_chr as they stand
template <int MODE, bool WRITE>
__global__ void k_sweep_seq(const u32 *__restrict__ as, const u32 *__restrict__ ae, const u32 *__restrict__ aoff,
                            const u32 *__restrict__ bs, const u32 *__restrict__ be, const u32 *__restrict__ boff, u32 n_rank,
                            const u32 *__restrict__ dirty, u32 *__restrict__ cnt, const u64 *__restrict__ off, u32 *__restrict__ oseg,
                            u32 *__restrict__ os, u32 *__restrict__ oe) {
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n_rank; r += (u64)gridDim.x * blockDim.x) {
        if (!dirty[r]) continue;
        const u32 blo = boff[r], bhi = boff[r + 1];
        u32 b_idx = blo;
        for (u32 i = aoff[r]; i < aoff[r + 1]; ++i) {
            const u32 s = as[i], e = ae[i];
            while (b_idx < bhi && be[b_idx] <= s) ++b_idx;
            const u64 o = WRITE ? off[i] : 0;
            u32 c = 0;
            if (MODE == SWEEP_SETDIFF) {
                u32 pos = s;
                for (u32 j = b_idx; j < bhi && bs[j] < e && pos < e; ++j) {
                    if (bs[j] > pos) emit<MODE, WRITE>(c, o, (u32)r, pos, bs[j], oseg, os, oe);
                    pos = max(pos, be[j]);
                }
                if (pos < e) emit<MODE, WRITE>(c, o, (u32)r, pos, e, oseg, os, oe);
            } else {
                for (u32 j = b_idx; j < bhi && bs[j] < e; ++j) {
                    const u32 ps = max(s, bs[j]), pe = min(e, be[j]);
                    if (ps < pe) emit<MODE, WRITE>(c, o, (u32)r, ps, pe, oseg, os, oe);
                }
            }
            if (!WRITE) cnt[i] = c;
        }
    }
}

template <int MODE>
gtars_status dev_sweep(StreamFrame &fr, const DevSet &A, const DevSet &B, u32 n_rank, DevSet &out) {
    out = DevSet();
    if (!A.n) return GTARS_OK;
    hipStream_t st = fr.st;
    u32 *aoff, *boff, *dirty, *cnt;
    GT_TRY(fr.alloc(&aoff, (size_t)n_rank + 1));
    GT_TRY(fr.alloc(&boff, (size_t)n_rank + 1));
    GT_TRY(fr.alloc(&dirty, n_rank));
    hipLaunchKernelGGL(k_seg_offsets, dim3(grid_for((u64)A.n + 1)), dim3(256), 0, st, A.seg, A.n, n_rank, aoff);
    hipLaunchKernelGGL(k_seg_offsets, dim3(grid_for((u64)B.n + 1)), dim3(256), 0, st, B.seg, B.n, n_rank, boff);
    GT_HIP(hipMemsetAsync(dirty, 0, (size_t)std::max<u32>(n_rank, 1) * 4, st));
    hipLaunchKernelGGL(k_mark_inverted, dim3(grid_for(A.n)), dim3(256), 0, st, A.seg, A.start, A.end, A.n, 1u, dirty);
    if (B.n) hipLaunchKernelGGL(k_mark_inverted, dim3(grid_for(B.n)), dim3(256), 0, st, B.seg, B.start, B.end, B.n, 1u, dirty);
    GT_TRY(fr.alloc(&cnt, A.n));
    hipLaunchKernelGGL((k_sweep_par<MODE, false>), dim3(grid_for(A.n)), dim3(256), 0, st, A.seg, A.start, A.end, A.n, B.start, B.end,
                       boff, dirty, cnt, nullptr, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL((k_sweep_seq<MODE, false>), dim3(grid_for(n_rank, 64)), dim3(64), 0, st, A.start, A.end, aoff, B.start, B.end,
                       boff, n_rank, dirty, cnt, nullptr, nullptr, nullptr, nullptr);
    u64 *off, m = 0;
    GT_TRY(scan_total(fr, cnt, A.n, &off, &m));
    if (m > SO_MAX_N) return fail(GTARS_ERR_CAPACITY, "set operation result too large: need " + std::to_string(m));
    GT_TRY(alloc_set(fr, m, out));
    hipLaunchKernelGGL((k_sweep_par<MODE, true>), dim3(grid_for(A.n)), dim3(256), 0, st, A.seg, A.start, A.end, A.n, B.start, B.end,
                       boff, dirty, nullptr, off, out.seg, out.start, out.end);
    hipLaunchKernelGGL((k_sweep_seq<MODE, true>), dim3(grid_for(n_rank, 64)), dim3(64), 0, st, A.start, A.end, aoff, B.start, B.end,
                       boff, n_rank, dirty, nullptr, off, out.seg, out.start, out.end);
    GT_HIP(hipGetLastError());
    return GTARS_OK;
}

template <int MODE>
gtars_status two_set(const SetCols &a, const SetCols &b, u32 n_rank, SetOut &res) {
    GT_TRY(check_sizes(a.n + b.n, n_rank));
    StreamFrame fr(nullptr);
    DevSet A, B, R;
    GT_TRY(reduce_cols(fr, a, n_rank, A));
    GT_TRY(reduce_cols(fr, b, n_rank, B));
    GT_TRY(dev_sweep<MODE>(fr, A, B, n_rank, R));
    GT_TRY(download(fr, R, res));
    return fr.drain();
}

// ------------------------------------------------------------------------------------------------------ closest
// max over the chromosome of the wrapping width end - start (sorted by rank: a lane flushes on a rank change)
__global__ void k_max_width(const u32 *__restrict__ seg, const u32 *__restrict__ start, const u32 *__restrict__ end, u32 n,
                            u32 *__restrict__ maxw) {
    constexpr u32 PER = 64;
    for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t * PER < n; t += (u64)gridDim.x * blockDim.x) {
        const u64 i1 = std::min<u64>(n, (t + 1) * PER);
        u32 r = seg[t * PER], m = 0;
        for (u64 i = t * PER; i < i1; ++i) {
            if (seg[i] != r) {
                atomicMax(&maxw[r], m);
                r = seg[i];
                m = 0;
            }
            m = max(m, end[i] - start[i]);
        }
        atomicMax(&maxw[r], m);
    }
}

// RegionSet::closest for one region of self: the reference's interleaved walk (right, then left, per step) from the
// insertion point.  The insertion point is the FIRST candidate whose start equals the query's start (lower bound):
// binary_search_by_key leaves the index unspecified among equal keys, this library pins it.
__global__ void k_closest(const u32 *__restrict__ qr, const u32 *__restrict__ qs, const u32 *__restrict__ qe, u32 nq,
                          const u32 *__restrict__ cs, const u32 *__restrict__ ce, const u32 *__restrict__ cperm,
                          const u32 *__restrict__ coff, const u32 *__restrict__ maxw, u32 n_rank, u32 *__restrict__ found,
                          u32 *__restrict__ best_idx, i64 *__restrict__ best_d) {
    for (u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (u64)gridDim.x * blockDim.x) {
        const u32 r = qr[q];
        const u32 lo = r < n_rank ? coff[r] : 0, hi = r < n_rank ? coff[r + 1] : 0;
        if (lo >= hi) {
            found[q] = 0;
            continue;
        }
        const i64 as = qs[q], ae = qe[q];
        const u32 n_c = hi - lo;
        const u32 ins = first_ge(cs, lo, hi, qs[q]) - lo;
        const i64 mw = maxw[r];
        u32 bi = 0;
        i64 best = std::numeric_limits<i64>::max();
        bool left_done = ins == 0, right_done = ins >= n_c;
        u32 li = ins > 0 ? ins - 1 : 0, ri = ins;
        auto gap = [&](u32 j) -> i64 {
            const i64 bs = cs[lo + j], be = ce[lo + j];
            if (as < be && bs < ae) return 0;
            if (be <= as) return as - be;
            return bs - ae;
        };
        auto iabs = [](i64 x) { return x < 0 ? -x : x; };
        while (!left_done || !right_done) {
            if (!right_done) {
                const i64 d = gap(ri);
                if (iabs(d) < iabs(best)) {
                    best = d;
                    bi = ri;
                }
                if (best == 0) break;
                const i64 bstart = cs[lo + ri];
                ++ri;
                if (ri >= n_c || bstart - ae > iabs(best)) right_done = true;
            }
            if (!left_done) {
                const i64 d = gap(li);
                if (iabs(d) < iabs(best)) {
                    best = d;
                    bi = li;
                }
                if (best == 0) break;
                if (li == 0 || as - (i64)cs[lo + li] > iabs(best) + mw) left_done = true;
                else --li;
            }
        }
        found[q] = 1;
        best_idx[q] = cperm[lo + bi];
        best_d[q] = best;
    }
}

__global__ void k_closest_compact(const u32 *__restrict__ found, const u64 *__restrict__ off, const u32 *__restrict__ bidx,
                                  const i64 *__restrict__ bd, u32 nq, u32 *__restrict__ o_self, u32 *__restrict__ o_other,
                                  i64 *__restrict__ o_d) {
    for (u64 q = (u64)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (u64)gridDim.x * blockDim.x) {
        if (!found[q]) continue;
        const u64 o = off[q];
        o_self[o] = (u32)q;
        o_other[o] = bidx[q];
        o_d[o] = bd[q];
    }
}

// ------------------------------------------------------------------------------------------------------ cluster
__global__ void k_cluster_scatter(const u32 *__restrict__ perm, const u32 *__restrict__ flag, const u64 *__restrict__ off, u32 n,
                                  u32 *__restrict__ ids) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
        ids[perm[i]] = (u32)(off[i] + flag[i] - 1);
}

// ------------------------------------------------------------------------------------------------ pairwise Jaccard
// item: {smaller set s, other set t, first region of s (relative), pair index}.  Covered bp of t on segment c before p:
// G(p) = P[k] - (end[k-1] - p if region k-1 of the segment reaches past p), k = first region of the segment with start >= p.
__global__ void __launch_bounds__(256)
k_pair_inter(const uint4 *__restrict__ items, const u32 *__restrict__ seg, const u32 *__restrict__ start, const u32 *__restrict__ end,
             const u64 *__restrict__ P, const u32 *__restrict__ set_off, const u32 *__restrict__ seg_off, u32 n_rank,
             u64 *__restrict__ inter) {
    const uint4 it = items[blockIdx.x];
    const u32 s = it.x, t = it.y;
    const u32 i0 = set_off[s] + it.z, i1 = min(set_off[s + 1], i0 + SO_PAIR_CHUNK);
    u64 acc = 0;
    for (u32 i = i0 + threadIdx.x; i < i1; i += 256) {
        const u32 c = seg[i] - s * n_rank + t * n_rank;
        const u32 lo = seg_off[c], hi = seg_off[c + 1];
        if (lo == hi) continue;
        const u32 xs = start[i], xe = end[i];
        const u32 ks = first_ge(start, lo, hi, xs);
        const u32 ke = first_ge(start, ks, hi, xe);
        const u64 gs = P[ks] - ((ks > lo && end[ks - 1] > xs) ? (u64)(end[ks - 1] - xs) : 0);
        const u64 ge = P[ke] - ((ke > lo && end[ke - 1] > xe) ? (u64)(end[ke - 1] - xe) : 0);
        acc += ge - gs;
    }
    acc = wave_reduce_sum_u64(acc);
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd((unsigned long long *)&inter[it.w], (unsigned long long)acc);
}

__global__ void k_pair_finish(const uint2 *__restrict__ pairs, u32 n_pairs, const u64 *__restrict__ inter, const u64 *__restrict__ P,
                              const u32 *__restrict__ set_off, u32 n_sets, double *__restrict__ M) {
    for (u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += (u64)gridDim.x * blockDim.x) {
        const u32 i = pairs[p].x, j = pairs[p].y;
        const u32 a = (u32)(P[set_off[i + 1]] - P[set_off[i]]), b = (u32)(P[set_off[j + 1]] - P[set_off[j]]);
        const u32 uni = a + b - (u32)inter[p];
        const double v = uni == 0 ? 0.0 : (double)(u32)(a + b - uni) / (double)uni;
        M[(u64)i * n_sets + j] = v;
        M[(u64)j * n_sets + i] = v;
    }
}

double jaccard_of(const SetTotals &t) {
    if (t.union_bp == 0) return 0.0;
    const u32 inter = t.a_bp + t.b_bp - t.union_bp;
    return (double)inter / (double)t.union_bp;
}

}  // namespace

// ======================================================================================================= entries
gtars_status setops_reduce(const SetCols &a, uint32_t n_rank, SetOut &res) {
    GT_TRY(check_sizes(a.n, n_rank));
    StreamFrame fr(nullptr);
    DevSet R;
    GT_TRY(reduce_cols(fr, a, n_rank, R));
    GT_TRY(download(fr, R, res));
    return fr.drain();
}

gtars_status setops_setdiff(const SetCols &a, const SetCols &b, uint32_t n_rank, SetOut &res) {
    return two_set<SWEEP_SETDIFF>(a, b, n_rank, res);
}

gtars_status setops_intersect(const SetCols &a, const SetCols &b, uint32_t n_rank, SetOut &res) {
    return two_set<SWEEP_INTERSECT>(a, b, n_rank, res);
}

gtars_status setops_totals(const SetCols &a, const SetCols &b, uint32_t n_rank, bool want_diff, SetTotals &out) {
    GT_TRY(check_sizes(a.n + b.n, n_rank));
    StreamFrame fr(nullptr);
    hipStream_t st = fr.st;
    // a and b side by side: reduce(a), reduce(b) and reduce(concat(a, b)) from the same columns
    const SetCols parts[2] = {a, b};
    DevSet C, A, B, U, D;
    GT_TRY(upload_concat(fr, parts, 2, C));
    GT_TRY(dev_reduce(fr, DevSet{C.seg, C.start, C.end, (u32)a.n}, n_rank, A));
    GT_TRY(dev_reduce(fr, DevSet{C.seg + a.n, C.start + a.n, C.end + a.n, (u32)b.n}, n_rank, B));
    GT_TRY(dev_reduce(fr, C, n_rank, U));
    if (want_diff) GT_TRY(dev_sweep<SWEEP_SETDIFF>(fr, A, B, n_rank, D));
    u64 *acc;
    GT_TRY(fr.alloc(&acc, 4));
    GT_HIP(hipMemsetAsync(acc, 0, 4 * sizeof(u64), st));
    const DevSet *sets[4] = {&A, &B, &U, &D};
    for (int k = 0; k < 4; ++k)
        if (sets[k]->n)
            hipLaunchKernelGGL(k_sum_widths, dim3(grid_for(sets[k]->n, 1024)), dim3(256), 0, st, sets[k]->start, sets[k]->end,
                               sets[k]->n, acc + k);
    GT_HIP(hipGetLastError());
    u64 h[4];
    GT_TRY(fr.download(h, acc, 4));
    GT_TRY(fr.drain());
    out.a_bp = (u32)h[0];
    out.b_bp = (u32)h[1];
    out.union_bp = (u32)h[2];
    out.diff_bp = (u32)h[3];
    return GTARS_OK;
}

gtars_status setops_closest(const SetCols &a, const SetCols &other, uint32_t n_rank, std::vector<uint32_t> &self_idx,
                            std::vector<uint32_t> &other_idx, std::vector<int64_t> &dist) {
    self_idx.clear();
    other_idx.clear();
    dist.clear();
    GT_TRY(check_sizes(std::max(a.n, other.n), n_rank));
    if (!other.n || !a.n) return GTARS_OK;
    StreamFrame fr(nullptr);
    hipStream_t st = fr.st;
    const u32 no = (u32)other.n, nq = (u32)a.n;
    // candidates: `other` stably sorted by (chromosome, start)
    DevSet O, C, Q;
    u32 *perm, *coff, *maxw;
    GT_TRY(upload_set(fr, other, O));
    GT_TRY(sorted_set(fr, O, O.seg, nullptr, n_rank, C, &perm));
    GT_TRY(fr.alloc(&coff, (size_t)n_rank + 1));
    hipLaunchKernelGGL(k_seg_offsets, dim3(grid_for((u64)no + 1)), dim3(256), 0, st, C.seg, no, n_rank, coff);
    GT_TRY(fr.alloc(&maxw, n_rank));
    GT_HIP(hipMemsetAsync(maxw, 0, (size_t)std::max<u32>(n_rank, 1) * 4, st));
    hipLaunchKernelGGL(k_max_width, dim3(grid_for((no + 63) / 64)), dim3(256), 0, st, C.seg, C.start, C.end, no, maxw);
    u32 *found, *bidx;
    i64 *bd;
    GT_TRY(upload_set(fr, a, Q));
    GT_TRY(fr.alloc(&found, nq));
    GT_TRY(fr.alloc(&bidx, nq));
    GT_TRY(fr.alloc(&bd, nq));
    hipLaunchKernelGGL(k_closest, dim3(grid_for(nq)), dim3(256), 0, st, Q.seg, Q.start, Q.end, nq, C.start, C.end, perm, coff, maxw, n_rank,
                       found, bidx, bd);
    GT_HIP(hipGetLastError());
    u64 *off, m = 0;
    GT_TRY(scan_total(fr, found, nq, &off, &m));
    u32 *o_self, *o_other;
    i64 *o_d;
    GT_TRY(fr.alloc(&o_self, m));
    GT_TRY(fr.alloc(&o_other, m));
    GT_TRY(fr.alloc(&o_d, m));
    hipLaunchKernelGGL(k_closest_compact, dim3(grid_for(nq)), dim3(256), 0, st, found, off, bidx, bd, nq, o_self, o_other, o_d);
    GT_HIP(hipGetLastError());
    GT_TRY(fr.download(self_idx, o_self, m));
    GT_TRY(fr.download(other_idx, o_other, m));
    GT_TRY(fr.download(dist, o_d, m));
    return fr.drain();
}

gtars_status setops_cluster(const SetCols &a, uint32_t n_rank, uint32_t max_gap, uint32_t *ids) {
    GT_TRY(check_sizes(a.n, n_rank));
    if (!a.n) return GTARS_OK;
    StreamFrame fr(nullptr);
    const u32 n = (u32)a.n;
    DevSet A, S;
    u32 *perm, *flag, *d_ids;
    GT_TRY(upload_set(fr, a, A));
    GT_TRY(sorted_set(fr, A, A.seg, A.end, n_rank, S, &perm));  // (chromosome, start, end)
    GT_TRY(fr.alloc(&flag, n));
    GT_TRY(seg_max_pass(fr, false, S.seg, S.end, S.start, n, max_gap, flag));
    u64 *off, m = 0;
    GT_TRY(scan_total(fr, flag, n, &off, &m));
    GT_TRY(fr.alloc(&d_ids, n));
    hipLaunchKernelGGL(k_cluster_scatter, dim3(grid_for(n)), dim3(256), 0, fr.st, perm, flag, off, n, d_ids);
    GT_HIP(hipGetLastError());
    GT_TRY(fr.download(ids, d_ids, n));
    return fr.drain();
}

gtars_status setops_pairwise_jaccard(const std::vector<SetCols> &sets, uint32_t n_rank, double *out) {
    const u64 n_sets = sets.size();
    u64 n = 0;
    for (const SetCols &s : sets) n += s.n;
    GT_TRY(check_sizes(n, n_rank));
    if (!n_sets) return GTARS_OK;
    const u64 n_seg64 = n_sets * std::max<u32>(n_rank, 1);
    if (n_seg64 > 0x7FFFFFFFull || n_sets > 0xFFFFFFull) return fail(GTARS_ERR_INVALID_ARG, "too many sets x chromosomes for one pairwise call");
    const u32 n_seg = (u32)n_seg64, nr = std::max<u32>(n_rank, 1);
    for (u64 i = 0; i < n_sets; ++i)
        for (u64 j = 0; j < n_sets; ++j) out[i * n_sets + j] = i == j ? 1.0 : 0.0;
    if (!n) return GTARS_OK;  // every off-diagonal pair has union 0
    StreamFrame fr(nullptr);
    hipStream_t st = fr.st;
    // every set reduced in one pass: segment = set * n_rank + chromosome rank, built set by set between the copies
    std::vector<u32> hseg(n);
    DevSet C, R;
    C.n = (u32)n;
    GT_TRY(fr.alloc(&C.start, n));
    GT_TRY(fr.alloc(&C.end, n));
    u64 at = 0;
    for (u64 k = 0; k < n_sets; ++k) {
        const SetCols &s = sets[k];
        for (u64 i = 0; i < s.n; ++i) hseg[at + i] = (u32)k * nr + s.rank[i];
        GT_TRY(fr.upload_to(C.start + at, s.start, s.n));
        GT_TRY(fr.upload_to(C.end + at, s.end, s.n));
        at += s.n;
    }
    GT_TRY(fr.upload(&C.seg, hseg.data(), n));
    GT_TRY(dev_reduce(fr, C, n_seg, R));
    u32 *seg_off, *dirty, *w, *d_set_off;
    GT_TRY(fr.alloc(&seg_off, (size_t)n_seg + 1));
    hipLaunchKernelGGL(k_seg_offsets, dim3(grid_for((u64)R.n + 1)), dim3(256), 0, st, R.seg, R.n, n_seg, seg_off);
    GT_TRY(fr.alloc(&dirty, n_sets));
    GT_HIP(hipMemsetAsync(dirty, 0, n_sets * 4, st));
    hipLaunchKernelGGL(k_mark_inverted, dim3(grid_for(R.n)), dim3(256), 0, st, R.seg, R.start, R.end, R.n, nr, dirty);
    GT_TRY(fr.alloc(&w, R.n));
    hipLaunchKernelGGL(k_widths, dim3(grid_for(R.n)), dim3(256), 0, st, R.start, R.end, R.n, w);
    u64 *P, total = 0;
    GT_TRY(scan_total(fr, w, R.n, &P, &total));
    std::vector<u32> h_seg_off, h_dirty, set_off(n_sets + 1);
    GT_TRY(fr.download(h_seg_off, seg_off, (size_t)n_seg + 1));
    GT_TRY(fr.download(h_dirty, dirty, n_sets));
    GT_TRY(fr.drain());
    for (u64 k = 0; k <= n_sets; ++k) set_off[k] = h_seg_off[k * nr];
    GT_TRY(fr.upload(&d_set_off, set_off.data(), set_off.size()));
    // work list over the pairs of clean sets (no inverted region after reduce)
    std::vector<uint2> pairs;
    std::vector<uint4> items;
    std::vector<std::pair<u32, u32>> dirty_pairs;
    for (u32 i = 0; i < n_sets; ++i)
        for (u32 j = i + 1; j < n_sets; ++j) {
            if (h_dirty[i] || h_dirty[j]) {
                dirty_pairs.emplace_back(i, j);
                continue;
            }
            const u32 p = (u32)pairs.size();
            pairs.push_back(make_uint2(i, j));
            const u32 ni = set_off[i + 1] - set_off[i], nj = set_off[j + 1] - set_off[j];
            const u32 s = ni <= nj ? i : j, t = ni <= nj ? j : i, ns = std::min(ni, nj);
            for (u32 c = 0; c < ns; c += SO_PAIR_CHUNK) items.push_back(make_uint4(s, t, c, p));
        }
    if (!pairs.empty()) {
        uint2 *d_pairs;
        uint4 *d_items;
        u64 *inter;
        double *dM;
        GT_TRY(fr.upload(&d_pairs, pairs.data(), pairs.size()));
        GT_TRY(fr.alloc(&inter, pairs.size()));
        GT_HIP(hipMemsetAsync(inter, 0, pairs.size() * 8, st));
        if (!items.empty()) {
            GT_TRY(fr.upload(&d_items, items.data(), items.size()));
            for (size_t b = 0; b < items.size(); b += (1u << 20)) {  // grids of at most 2^20 workgroups
                const size_t nb = std::min<size_t>(items.size() - b, 1u << 20);
                hipLaunchKernelGGL(k_pair_inter, dim3((unsigned)nb), dim3(256), 0, st, d_items + b, R.seg, R.start, R.end, P, d_set_off,
                                   seg_off, nr, inter);
            }
        }
        GT_TRY(fr.alloc(&dM, n_sets * n_sets));
        GT_TRY(fr.upload_to(dM, out, n_sets * n_sets));
        hipLaunchKernelGGL(k_pair_finish, dim3(grid_for(pairs.size())), dim3(256), 0, st, d_pairs, (u32)pairs.size(), inter, P, d_set_off,
                           (u32)n_sets, dM);
        GT_HIP(hipGetLastError());
        GT_TRY(fr.download(out, dM, n_sets * n_sets));
        GT_TRY(fr.drain());
    }
    if (!dirty_pairs.empty()) {
        // a set that keeps an inverted region: the two-set path on the reduced sets, both orders
        SetOut h;
        GT_TRY(download(fr, R, h));
        GT_TRY(fr.drain());
        for (u32 k = 0; k < R.n; ++k) h.rank[k] %= nr;
        auto cols = [&](u32 k) { return SetCols{h.rank.data() + set_off[k], h.start.data() + set_off[k], h.end.data() + set_off[k],
                                                (u64)(set_off[k + 1] - set_off[k])}; };
        for (const auto &pr : dirty_pairs) {
            SetTotals t1, t2;
            GT_TRY(setops_totals(cols(pr.first), cols(pr.second), n_rank, false, t1));
            GT_TRY(setops_totals(cols(pr.second), cols(pr.first), n_rank, false, t2));
            out[(u64)pr.first * n_sets + pr.second] = jaccard_of(t1);
            out[(u64)pr.second * n_sets + pr.first] = jaccard_of(t2);
        }
    }
    return GTARS_OK;
}


// ================================================================= K9: structural operations and region-set statistics
// disjoin, gaps, consensus, neighbour distances, the midpoint distribution and the per-chromosome statistics of
// gtars-core's RegionSet and gtars-genomicdist, on the same blocks as K8: the stable radix sort, the segmented max-scan
// of reduce, and count / scan / write compaction.
namespace {

__global__ void k_fill(u32 *__restrict__ p, u32 n, u32 v) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) p[i] = v;
}

// out[i] = table[idx[i]]
__global__ void k_lookup(const u32 *__restrict__ idx, u32 n, const u32 *__restrict__ table, u32 *__restrict__ out) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) out[i] = table[idx[i]];
}

// ------------------------------------------------------------------------------------------------------- disjoin
// events 2i and 2i + 1: the start and the end of region i
__global__ void k_dj_events(const u32 *__restrict__ rank, const u32 *__restrict__ start, const u32 *__restrict__ end, u32 n,
                            u32 *__restrict__ ev_rank, u32 *__restrict__ ev_pos) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        ev_rank[2 * i] = ev_rank[2 * i + 1] = rank[i];
        ev_pos[2 * i] = start[i];
        ev_pos[2 * i + 1] = end[i];
    }
}

// sorted events; opens / closes: the event is the start / end of a well-formed region (start < end).  Inverted and
// zero-width regions add boundaries and no depth.
__global__ void k_dj_gather(const u32 *__restrict__ perm, u32 m, const u32 *__restrict__ ev_rank, const u32 *__restrict__ ev_pos,
                            const u32 *__restrict__ start, const u32 *__restrict__ end, u32 *__restrict__ srank, u32 *__restrict__ spos,
                            u32 *__restrict__ opens, u32 *__restrict__ closes) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (u64)gridDim.x * blockDim.x) {
        const u32 p = perm[j], i = p >> 1;
        const u32 wf = start[i] < end[i];
        srank[j] = ev_rank[p];
        spos[j] = ev_pos[p];
        opens[j] = wf & ~p & 1u;
        closes[j] = wf & p & 1u;
    }
}

// piece [pos[j], pos[j + 1]) when j is the last event at its position, the next event is on the same chromosome, and the
// depth after j (opens minus closes so far: every chromosome's own events cancel) is positive.  WRITE: emit it at off[j].
template <bool WRITE>
__global__ void k_dj_pieces(const u32 *__restrict__ srank, const u32 *__restrict__ spos, const u64 *__restrict__ co,
                            const u64 *__restrict__ cc, u32 m, u32 *__restrict__ keep, const u64 *__restrict__ off,
                            u32 *__restrict__ orank, u32 *__restrict__ ostart, u32 *__restrict__ oend) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (u64)gridDim.x * blockDim.x) {
        const bool k = j + 1 < m && srank[j + 1] == srank[j] && spos[j + 1] != spos[j] && co[j + 1] > cc[j + 1];
        if (!WRITE) {
            keep[j] = k;
        } else if (k) {
            const u64 o = off[j];
            orank[o] = srank[j];
            ostart[o] = spos[j];
            oend[o] = spos[j + 1];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- gaps
// per reduced run i of a chromosome with size cs > 0: the leading gap (first run) or the gap after the previous run,
// then the trailing gap (last run), each clipped as RegionSet::gaps clips it
template <bool WRITE>
__global__ void k_gaps(const u32 *__restrict__ seg, const u32 *__restrict__ start, const u32 *__restrict__ end, u32 n,
                       const u32 *__restrict__ size, u32 *__restrict__ cnt, const u64 *__restrict__ off, u32 *__restrict__ oseg,
                       u32 *__restrict__ os, u32 *__restrict__ oe) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u32 r = seg[i], cs = size[r];
        const bool first = i == 0 || seg[i - 1] != r, last = i + 1 == n || seg[i + 1] != r;
        const u64 o = WRITE ? off[i] : 0;
        u32 c = 0;
        if (cs) {
            if (first) {
                if (start[i] > 0) emit<0, WRITE>(c, o, r, 0, min(start[i], cs), oseg, os, oe);
            } else {
                const u32 gs = end[i - 1], ge = start[i];
                if (gs < ge && min(gs, cs) < min(ge, cs)) emit<0, WRITE>(c, o, r, min(gs, cs), min(ge, cs), oseg, os, oe);
            }
            if (last && end[i] < cs) emit<0, WRITE>(c, o, r, end[i], cs, oseg, os, oe);
        }
        if (!WRITE) cnt[i] = c;
    }
}

// ----------------------------------------------------------------------------------------------------- consensus
// a sorted region hits its own run when start < run.end && run.start < end (the AIList rule); set' = its set, or
// n_sets when it does not hit
__global__ void k_cons_hits(const u32 *__restrict__ perm, const u32 *__restrict__ set, const u32 *__restrict__ sstart,
                            const u32 *__restrict__ send, const u32 *__restrict__ rid, const u32 *__restrict__ ustart,
                            const u32 *__restrict__ uend, u32 n, u32 n_sets, u32 *__restrict__ hit_set) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (u64)gridDim.x * blockDim.x) {
        const u32 r = rid[j];
        hit_set[j] = (sstart[j] < uend[r] && ustart[r] < send[j]) ? set[perm[j]] : n_sets;
    }
}

// rows sorted by (run, set'): one count per distinct hitting set of a run
__global__ void k_cons_count(const u32 *__restrict__ perm, const u32 *__restrict__ rid, const u32 *__restrict__ hit_set, u32 n,
                             u32 n_sets, u32 *__restrict__ count) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (u64)gridDim.x * blockDim.x) {
        const u32 p = perm[j], s = hit_set[p];
        if (s == n_sets) continue;
        if (j > 0) {
            const u32 q = perm[j - 1];
            if (rid[q] == rid[p] && hit_set[q] == s) continue;
        }
        atomicAdd(&count[rid[p]], 1u);
    }
}

// ----------------------------------------------------------------------------------------------------- neighbours
// rows sorted by (first-appearance rank, start, end).  NEAREST: every region of a chromosome with >= 2 regions, the
// smaller of its gaps to the left and right neighbour clamped at 0.  Else: every gap next.start - prev.end > 0.
template <bool NEAREST, bool WRITE>
__global__ void k_neighbors(const u32 *__restrict__ seg, const u32 *__restrict__ start, const u32 *__restrict__ end, u32 n,
                            u32 *__restrict__ keep, const u64 *__restrict__ off, i64 *__restrict__ odist, u32 *__restrict__ onear) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (u64)gridDim.x * blockDim.x) {
        const bool has_r = j + 1 < n && seg[j + 1] == seg[j];
        const i64 dr = has_r ? (i64)start[j + 1] - (i64)end[j] : 0;
        if (NEAREST) {
            const bool has_l = j > 0 && seg[j - 1] == seg[j];
            const bool k = has_l || has_r;
            if (!WRITE) {
                keep[j] = k;
            } else if (k) {
                const i64 dl = has_l ? (i64)start[j] - (i64)end[j - 1] : 0;
                const u32 cl = dl > 0 ? (u32)dl : 0u, cr = dr > 0 ? (u32)dr : 0u;
                onear[off[j]] = !has_l ? cr : !has_r ? cl : min(cl, cr);
            }
        } else {
            const bool k = has_r && dr > 0;
            if (!WRITE) keep[j] = k;
            else if (k) odist[off[j]] = dr;
        }
    }
}

// -------------------------------------------------------------------------------------------------- distribution
// key of region i: (rank, rid) of its midpoint start + (u32)(end - start) / 2 (wrapping); rank n_rank: not counted
__global__ void k_bin_keys(const u32 *__restrict__ rank, const u32 *__restrict__ start, const u32 *__restrict__ end, u32 n,
                           u32 n_rank, u32 n_bins, u32 bin_size, int with_sizes, const u32 *__restrict__ limit,
                           u32 *__restrict__ krank, u32 *__restrict__ krid) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u32 r = rank[i], mid = start[i] + (end[i] - start[i]) / 2u;
        u32 rid = mid / bin_size, kr = r;
        if (with_sizes) {
            if (mid >= limit[r]) kr = n_rank;
            rid = min(rid, n_bins - 1u);
        }
        krank[i] = kr;
        krid[i] = rid;
    }
}

// head[j]: row j (sorted by key) is counted and opens a key
__global__ void k_rle_heads(const u32 *__restrict__ perm, const u32 *__restrict__ krank, const u32 *__restrict__ krid, u32 n,
                            u32 n_rank, u32 *__restrict__ head) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (u64)gridDim.x * blockDim.x) {
        const u32 p = perm[j];
        bool h = krank[p] < n_rank;
        if (h && j > 0) {
            const u32 q = perm[j - 1];
            h = krank[q] != krank[p] || krid[q] != krid[p];
        }
        head[j] = h;
    }
}

// key o = (rank, rid) opens at row pos[o]; pos[m] = the number of counted rows (they sort first)
__global__ void k_rle_write(const u32 *__restrict__ perm, const u32 *__restrict__ krank, const u32 *__restrict__ krid,
                            const u32 *__restrict__ head, const u64 *__restrict__ off, u32 n, u32 n_rank, u32 m,
                            u32 *__restrict__ orank, u32 *__restrict__ orid, u32 *__restrict__ pos) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (u64)gridDim.x * blockDim.x) {
        const u32 p = perm[j];
        if (head[j]) {
            const u64 o = off[j];
            orank[o] = krank[p];
            orid[o] = krid[p];
            pos[o] = (u32)j;
        }
        if (krank[p] < n_rank && (j + 1 == n || krank[perm[j + 1]] == n_rank)) pos[m] = (u32)(j + 1);
    }
}

__global__ void k_rle_counts(const u32 *__restrict__ pos, u32 m, u32 *__restrict__ count) {
    for (u64 o = (u64)blockIdx.x * blockDim.x + threadIdx.x; o < m; o += (u64)gridDim.x * blockDim.x) count[o] = pos[o + 1] - pos[o];
}

// ---------------------------------------------------------------------------------------------- chromosome stats
// rows sorted by (rank, width): per lane 64 consecutive rows, flushed to the rank's min start / max end / width sum
// whenever the rank changes
__global__ void k_stat_bounds(const u32 *__restrict__ seg, const u32 *__restrict__ start, const u32 *__restrict__ end, u32 n,
                              u32 *__restrict__ min_start, u32 *__restrict__ max_end, u64 *__restrict__ wsum) {
    constexpr u32 PER = 64;
    for (u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x; t * PER < n; t += (u64)gridDim.x * blockDim.x) {
        const u64 i1 = std::min<u64>(n, (t + 1) * PER);
        u32 r = seg[t * PER], lo = 0xFFFFFFFFu, hi = 0;
        u64 sum = 0;
        for (u64 i = t * PER; i < i1; ++i) {
            if (seg[i] != r) {
                atomicMin(&min_start[r], lo);
                atomicMax(&max_end[r], hi);
                atomicAdd((unsigned long long *)&wsum[r], (unsigned long long)sum);
                r = seg[i];
                lo = 0xFFFFFFFFu, hi = 0, sum = 0;
            }
            lo = min(lo, start[i]);
            hi = max(hi, end[i]);
            sum += (u32)(end[i] - start[i]);
        }
        atomicMin(&min_start[r], lo);
        atomicMax(&max_end[r], hi);
        atomicAdd((unsigned long long *)&wsum[r], (unsigned long long)sum);
    }
}

// one lane per rank: count, min / max width at the segment's ends, mean = u64 sum / count, median from the middle
// widths (an even count adds the two in wrapping u32 before the division, as the reference's release build does)
__global__ void k_stat_finish(const u32 *__restrict__ off, const u32 *__restrict__ w, const u64 *__restrict__ wsum, u32 n_rank,
                              u32 *__restrict__ count, u32 *__restrict__ min_w, u32 *__restrict__ max_w, double *__restrict__ mean,
                              double *__restrict__ median) {
    for (u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x; r < n_rank; r += (u64)gridDim.x * blockDim.x) {
        const u32 lo = off[r], c = off[r + 1] - lo;
        count[r] = c;
        if (!c) continue;
        min_w[r] = w[lo];
        max_w[r] = w[lo + c - 1];
        mean[r] = (double)wsum[r] / (double)c;
        median[r] = (c & 1) ? (double)w[lo + c / 2] : (double)(u32)(w[lo + c / 2 - 1] + w[lo + c / 2]) / 2.0;
    }
}

// sorted rows of (rank, start, end) and their widths
__global__ void k_gather_widths(const u32 *__restrict__ perm, u32 n, const u32 *__restrict__ seg, const u32 *__restrict__ start,
                                const u32 *__restrict__ end, u32 *__restrict__ sseg, u32 *__restrict__ ss, u32 *__restrict__ se,
                                u32 *__restrict__ sw) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u32 p = perm[i];
        sseg[i] = seg[p];
        ss[i] = start[p];
        se[i] = end[p];
        sw[i] = end[p] - start[p];
    }
}

}  // namespace

gtars_status setops_disjoin(const SetCols &a, uint32_t n_rank, SetOut &res) {
    GT_TRY(check_sizes(2 * a.n, n_rank));
    res = SetOut();
    if (!a.n) return GTARS_OK;
    StreamFrame fr(nullptr);
    hipStream_t st = fr.st;
    const u32 n = (u32)a.n, m = 2 * n;
    DevSet A, R;
    u32 *ev_rank, *ev_pos, *perm, *srank, *spos, *opens, *closes, *keep;
    GT_TRY(upload_set(fr, a, A));
    GT_TRY(fr.alloc(&ev_rank, m));
    GT_TRY(fr.alloc(&ev_pos, m));
    hipLaunchKernelGGL(k_dj_events, dim3(grid_for(n)), dim3(256), 0, st, A.seg, A.start, A.end, n, ev_rank, ev_pos);
    GT_TRY(sort_perm(fr, ev_rank, ev_pos, nullptr, m, n_rank, &perm));
    GT_TRY(fr.alloc(&srank, m));
    GT_TRY(fr.alloc(&spos, m));
    GT_TRY(fr.alloc(&opens, m));
    GT_TRY(fr.alloc(&closes, m));
    hipLaunchKernelGGL(k_dj_gather, dim3(grid_for(m)), dim3(256), 0, st, perm, m, ev_rank, ev_pos, A.start, A.end, srank, spos, opens,
                       closes);
    u64 *co, *cc, *off, t = 0, k = 0;
    GT_TRY(scan_total(fr, opens, m, &co, &t));
    GT_TRY(scan_total(fr, closes, m, &cc, &t));
    GT_TRY(fr.alloc(&keep, m));
    hipLaunchKernelGGL(k_dj_pieces<false>, dim3(grid_for(m)), dim3(256), 0, st, srank, spos, co, cc, m, keep, nullptr, nullptr, nullptr,
                       nullptr);
    GT_TRY(scan_total(fr, keep, m, &off, &k));
    GT_TRY(alloc_set(fr, k, R));
    hipLaunchKernelGGL(k_dj_pieces<true>, dim3(grid_for(m)), dim3(256), 0, st, srank, spos, co, cc, m, nullptr, off, R.seg, R.start,
                       R.end);
    GT_HIP(hipGetLastError());
    GT_TRY(download(fr, R, res));
    return fr.drain();
}

gtars_status setops_gaps(const SetCols &a, uint32_t n_rank, const std::vector<uint32_t> &size, const std::vector<uint32_t> &group,
                         uint32_t n_group, SetOut &res) {
    GT_TRY(check_sizes(a.n + n_rank, n_rank));
    if (size.size() != n_rank || group.size() != n_rank) return fail(GTARS_ERR_INTERNAL, "gaps: per-rank tables of the wrong size");
    res = SetOut();
    StreamFrame fr(nullptr);
    hipStream_t st = fr.st;
    DevSet R;
    GT_TRY(reduce_cols(fr, a, n_rank, R));
    // full-chromosome gaps: ranks with a size that hold no region
    std::vector<u32> has(n_rank, 0);
    for (u64 i = 0; i < a.n; ++i) has[a.rank[i]] = 1;
    std::vector<u32> fr_rank, fr_end;
    for (u32 r = 0; r < n_rank; ++r)
        if (size[r] && !has[r]) fr_rank.push_back(r), fr_end.push_back(size[r]);
    const u32 nf = (u32)fr_rank.size();
    u32 *d_size, *cnt = nullptr;
    GT_TRY(fr.upload(&d_size, size.data(), n_rank));
    u64 *off = nullptr, m = 0;
    if (R.n) {
        GT_TRY(fr.alloc(&cnt, R.n));
        hipLaunchKernelGGL(k_gaps<false>, dim3(grid_for(R.n)), dim3(256), 0, st, R.seg, R.start, R.end, R.n, d_size, cnt, nullptr, nullptr,
                           nullptr, nullptr);
        GT_TRY(scan_total(fr, cnt, R.n, &off, &m));
    }
    const u64 total = m + nf;
    if (total > SO_MAX_N) return fail(GTARS_ERR_CAPACITY, "gaps result too large: need " + std::to_string(total));
    if (!total) return GTARS_OK;
    const u32 g = (u32)total;
    DevSet G, O;
    u32 *ggroup, *d_group;
    GT_TRY(alloc_set(fr, g, G));
    if (R.n)
        hipLaunchKernelGGL(k_gaps<true>, dim3(grid_for(R.n)), dim3(256), 0, st, R.seg, R.start, R.end, R.n, d_size, nullptr, off, G.seg,
                           G.start, G.end);
    GT_TRY(fr.upload_to(G.seg + m, fr_rank.data(), nf));
    if (nf) GT_HIP(hipMemsetAsync(G.start + m, 0, (size_t)nf * 4, st));
    GT_TRY(fr.upload_to(G.end + m, fr_end.data(), nf));
    // karyotypic order: (key, start), names of one key bytewise (rank order)
    GT_TRY(fr.upload(&d_group, group.data(), n_rank));
    GT_TRY(fr.alloc(&ggroup, g));
    hipLaunchKernelGGL(k_lookup, dim3(grid_for(g)), dim3(256), 0, st, G.seg, g, d_group, ggroup);
    GT_TRY(sorted_set(fr, G, ggroup, G.seg, std::max<u32>(n_group, 1), O));
    GT_TRY(download(fr, O, res));
    return fr.drain();
}

gtars_status setops_consensus(const std::vector<SetCols> &sets, uint32_t n_rank, SetOut &uni, std::vector<uint32_t> &count) {
    u64 n = 0;
    for (const SetCols &s : sets) n += s.n;
    GT_TRY(check_sizes(n, n_rank));
    uni = SetOut();
    count.clear();
    if (sets.size() >= 0xFFFFFFFFull) return fail(GTARS_ERR_INVALID_ARG, "too many region sets");
    if (!n) return GTARS_OK;
    const u32 n_sets = (u32)sets.size();
    StreamFrame fr(nullptr);
    hipStream_t st = fr.st;
    // the concatenation, with each row's set
    DevSet C, U;
    u32 *set;
    GT_TRY(upload_concat(fr, sets.data(), n_sets, C));
    GT_TRY(fr.alloc(&set, n));
    u64 at = 0;
    for (u32 k = 0; k < n_sets; ++k) {
        if (sets[k].n) hipLaunchKernelGGL(k_fill, dim3(grid_for(sets[k].n)), dim3(256), 0, st, set + at, (u32)sets[k].n, k);
        at += sets[k].n;
    }
    ReduceWork w;
    GT_TRY(dev_reduce(fr, C, n_rank, U, &w));
    // a region can only hit its own run: a later run starts past every end of the earlier ones
    u32 *hit_set, *perm, *d_count;
    GT_TRY(fr.alloc(&hit_set, n));
    hipLaunchKernelGGL(k_cons_hits, dim3(grid_for(n)), dim3(256), 0, st, w.perm, set, w.sstart, w.send, w.rid, U.start, U.end, (u32)n,
                       n_sets, hit_set);
    GT_TRY(sort_perm(fr, w.rid, hit_set, nullptr, (u32)n, U.n, &perm));
    GT_TRY(fr.alloc(&d_count, U.n));
    GT_HIP(hipMemsetAsync(d_count, 0, (size_t)U.n * 4, st));
    hipLaunchKernelGGL(k_cons_count, dim3(grid_for(n)), dim3(256), 0, st, perm, w.rid, hit_set, (u32)n, n_sets, d_count);
    GT_HIP(hipGetLastError());
    GT_TRY(fr.download(count, d_count, U.n));
    GT_TRY(download(fr, U, uni));
    return fr.drain();
}

template <bool NEAREST, class T>
gtars_status neighbors(const SetCols &a, uint32_t n_rank, std::vector<T> &res) {
    GT_TRY(check_sizes(a.n, n_rank));
    res.clear();
    if (a.n < 2) return GTARS_OK;
    StreamFrame fr(nullptr);
    hipStream_t st = fr.st;
    DevSet A, S;
    GT_TRY(upload_set(fr, a, A));
    GT_TRY(sorted_set(fr, A, A.seg, A.end, n_rank, S));
    u32 *keep;
    GT_TRY(fr.alloc(&keep, S.n));
    hipLaunchKernelGGL((k_neighbors<NEAREST, false>), dim3(grid_for(S.n)), dim3(256), 0, st, S.seg, S.start, S.end, S.n, keep, nullptr,
                       nullptr, nullptr);
    u64 *off, m = 0;
    GT_TRY(scan_total(fr, keep, S.n, &off, &m));
    T *out;
    GT_TRY(fr.alloc(&out, m));
    hipLaunchKernelGGL((k_neighbors<NEAREST, true>), dim3(grid_for(S.n)), dim3(256), 0, st, S.seg, S.start, S.end, S.n, nullptr, off,
                       (i64 *)out, (u32 *)out);
    GT_HIP(hipGetLastError());
    GT_TRY(fr.download(res, out, m));
    return fr.drain();
}

gtars_status setops_neighbor_distances(const SetCols &a, uint32_t n_rank, std::vector<int64_t> &out) {
    return neighbors<false>(a, n_rank, out);
}

gtars_status setops_nearest_neighbors(const SetCols &a, uint32_t n_rank, std::vector<uint32_t> &out) {
    return neighbors<true>(a, n_rank, out);
}

gtars_status setops_distribution(const SetCols &a, uint32_t n_rank, uint32_t n_bins, uint32_t bin_size, bool with_sizes,
                                 const std::vector<uint32_t> &limit, std::vector<uint32_t> &rank, std::vector<uint32_t> &rid,
                                 std::vector<uint32_t> &count) {
    GT_TRY(check_sizes(a.n, n_rank + 1));
    rank.clear();
    rid.clear();
    count.clear();
    if (!bin_size || (with_sizes && !n_bins) || limit.size() != n_rank) return fail(GTARS_ERR_INTERNAL, "distribution: bad bin layout");
    if (!a.n) return GTARS_OK;
    StreamFrame fr(nullptr);
    hipStream_t st = fr.st;
    const u32 n = (u32)a.n;
    DevSet A;
    u32 *d_limit, *krank, *krid, *perm, *head;
    GT_TRY(upload_set(fr, a, A));
    GT_TRY(fr.upload(&d_limit, limit.data(), std::max<u32>(n_rank, 1)));
    GT_TRY(fr.alloc(&krank, n));
    GT_TRY(fr.alloc(&krid, n));
    hipLaunchKernelGGL(k_bin_keys, dim3(grid_for(n)), dim3(256), 0, st, A.seg, A.start, A.end, n, n_rank, n_bins, bin_size,
                       (int)with_sizes, d_limit, krank, krid);
    GT_TRY(sort_perm(fr, krank, krid, nullptr, n, n_rank + 1, &perm));
    GT_TRY(fr.alloc(&head, n));
    hipLaunchKernelGGL(k_rle_heads, dim3(grid_for(n)), dim3(256), 0, st, perm, krank, krid, n, n_rank, head);
    u64 *off, m = 0;
    GT_TRY(scan_total(fr, head, n, &off, &m));
    if (!m) return GTARS_OK;
    u32 *orank, *orid, *pos, *cnt;
    GT_TRY(fr.alloc(&orank, m));
    GT_TRY(fr.alloc(&orid, m));
    GT_TRY(fr.alloc(&pos, m + 1));
    GT_TRY(fr.alloc(&cnt, m));
    hipLaunchKernelGGL(k_rle_write, dim3(grid_for(n)), dim3(256), 0, st, perm, krank, krid, head, off, n, n_rank, (u32)m, orank, orid, pos);
    hipLaunchKernelGGL(k_rle_counts, dim3(grid_for(m)), dim3(256), 0, st, pos, (u32)m, cnt);
    GT_HIP(hipGetLastError());
    GT_TRY(fr.download(rank, orank, m));
    GT_TRY(fr.download(rid, orid, m));
    GT_TRY(fr.download(count, cnt, m));
    return fr.drain();
}

gtars_status setops_chrom_stats(const SetCols &a, uint32_t n_rank, std::vector<ChromStat> &out) {
    GT_TRY(check_sizes(a.n, n_rank));
    out.assign(n_rank, ChromStat{0, 0, 0, 0, 0, 0.0, 0.0});
    if (!a.n) return GTARS_OK;
    StreamFrame fr(nullptr);
    hipStream_t st = fr.st;
    const u32 n = (u32)a.n, nr = std::max<u32>(n_rank, 1);
    DevSet A, S;
    u32 *w, *perm, *sw, *off, *min_s, *max_e, *cnt, *min_w, *max_w;
    u64 *wsum;
    double *mean, *median;
    GT_TRY(upload_set(fr, a, A));
    GT_TRY(fr.alloc(&w, n));
    hipLaunchKernelGGL(k_widths, dim3(grid_for(n)), dim3(256), 0, st, A.start, A.end, n, w);
    GT_TRY(sort_perm(fr, A.seg, w, nullptr, n, n_rank, &perm));  // (rank, width)
    GT_TRY(alloc_set(fr, n, S));
    GT_TRY(fr.alloc(&sw, n));
    hipLaunchKernelGGL(k_gather_widths, dim3(grid_for(n)), dim3(256), 0, st, perm, n, A.seg, A.start, A.end, S.seg, S.start, S.end, sw);
    GT_TRY(fr.alloc(&off, (size_t)nr + 1));
    hipLaunchKernelGGL(k_seg_offsets, dim3(grid_for((u64)n + 1)), dim3(256), 0, st, S.seg, n, n_rank, off);
    GT_TRY(fr.alloc(&min_s, nr));
    GT_TRY(fr.alloc(&max_e, nr));
    GT_TRY(fr.alloc(&wsum, nr));
    GT_HIP(hipMemsetAsync(min_s, 0xFF, (size_t)nr * 4, st));
    GT_HIP(hipMemsetAsync(max_e, 0, (size_t)nr * 4, st));
    GT_HIP(hipMemsetAsync(wsum, 0, (size_t)nr * 8, st));
    hipLaunchKernelGGL(k_stat_bounds, dim3(grid_for((n + 63) / 64)), dim3(256), 0, st, S.seg, S.start, S.end, n, min_s, max_e, wsum);
    GT_TRY(fr.alloc(&cnt, nr));
    GT_TRY(fr.alloc(&min_w, nr));
    GT_TRY(fr.alloc(&max_w, nr));
    GT_TRY(fr.alloc(&mean, nr));
    GT_TRY(fr.alloc(&median, nr));
    hipLaunchKernelGGL(k_stat_finish, dim3(grid_for(n_rank)), dim3(256), 0, st, off, sw, wsum, n_rank, cnt, min_w, max_w, mean, median);
    GT_HIP(hipGetLastError());
    std::vector<u32> h_cnt, h_min_s, h_max_e, h_min_w, h_max_w;
    std::vector<double> h_mean, h_median;
    GT_TRY(fr.download(h_cnt, cnt, n_rank));
    GT_TRY(fr.download(h_min_s, min_s, n_rank));
    GT_TRY(fr.download(h_max_e, max_e, n_rank));
    GT_TRY(fr.download(h_min_w, min_w, n_rank));
    GT_TRY(fr.download(h_max_w, max_w, n_rank));
    GT_TRY(fr.download(h_mean, mean, n_rank));
    GT_TRY(fr.download(h_median, median, n_rank));
    GT_TRY(fr.drain());
    for (u32 r = 0; r < n_rank; ++r)
        if (h_cnt[r]) out[r] = ChromStat{h_cnt[r], h_min_s[r], h_max_e[r], h_min_w[r], h_max_w[r], h_mean[r], h_median[r]};
    return GTARS_OK;
}

// ============================================================ K8, second part: folds over a list of sets (RegionSetListOps)
// union_all / union_except / bulk_union_except / intersect_all of gtars-genomicdist/src/region_set_list_ops.rs:103-181 for
// lists of >= 2 sets (the host layer answers the shorter lists, which the reference returns as unreduced copies).
// DESIGN.md §3 K8 "Folds over a list".
namespace {

// ------------------------------------------------------------------------------- top-2-by-owner segmented max-scan
// The summary of a span of rows (end, set): m1 = the largest end, s1 = a set that attains it, m2 = the largest end among
// the rows of every other set.  The running maximum without set i is then s1 == i ? m2 : m1.  Each maximum has a valid
// bit of its own: an end of 0xFFFFFFFF is a value, not "none yet".
struct T2 {
    u32 f;  // T2_V1 | T2_V2 | T2_HEAD
    u32 m1, s1, m2;
};
constexpr u32 T2_V1 = 1u, T2_V2 = 2u, T2_HEAD = 4u;  // m1 valid, m2 valid, a segment head lies in the span
constexpr u32 T2_CHR = 4u;                           // in a stored row: the row opens a chromosome (or is the row past the end)
constexpr u32 T2_CLS_SHIFT = 3;                      // in a stored row: 0 no head, 1 head for every set but its own, 2 head for s1 only

__device__ __forceinline__ T2 t2_op(T2 a, T2 b) {
    if (b.f & T2_HEAD) return b;
    if (!(b.f & T2_V1)) return a;
    const u32 head = a.f & T2_HEAD;
    if (!(a.f & T2_V1)) return T2{b.f | head, b.m1, b.s1, b.m2};
    if (a.s1 == b.s1) {
        const u32 v2 = (a.f | b.f) & T2_V2;
        const u32 m2 = (a.f & b.f & T2_V2) ? max(a.m2, b.m2) : (a.f & T2_V2) ? a.m2 : b.m2;
        return T2{T2_V1 | v2 | head, max(a.m1, b.m1), a.s1, m2};
    }
    const bool bw = b.m1 > a.m1;  // the larger m1 wins; the loser's m1 is the largest end of its span, and not the winner's set
    const T2 w = bw ? b : a, l = bw ? a : b;
    return T2{T2_V1 | T2_V2 | head, w.m1, w.s1, (w.f & T2_V2) ? max(w.m2, l.m1) : l.m1};
}
__device__ __forceinline__ uint4 t2_pack(T2 a) { return make_uint4(a.f, a.m1, a.s1, a.m2); }
__device__ __forceinline__ T2 t2_unpack(uint4 x) { return T2{x.x, x.y, x.z, x.w}; }
__device__ __forceinline__ T2 t2_row(const u32 *__restrict__ seg, const u32 *__restrict__ end, const u32 *__restrict__ set, u64 i) {
    return T2{T2_V1 | (is_head(seg, i) ? T2_HEAD : 0u), end[i], set[i], 0u};
}

// Inclusive scan across the workgroup through LDS (Hillis-Steele); lds[t] holds thread t's inclusive value afterwards.
// Kept beside scan.h's block_scan: on the shuffle form k_t2_apply measured 3 % slower (profiles/scan_skeleton).
template <int TPB>
__device__ __forceinline__ T2 t2_block_incl(T2 x, uint4 *lds) {
    const int t = threadIdx.x;
    lds[t] = t2_pack(x);
    __syncthreads();
    for (int d = 1; d < TPB; d <<= 1) {
        T2 y = x;
        if (t >= d) y = t2_op(t2_unpack(lds[t - d]), x);
        __syncthreads();
        lds[t] = t2_pack(y);
        x = y;
        __syncthreads();
    }
    return x;
}

// a thread's SO_IPT rows folded in order; rows past n are the identity
__device__ __forceinline__ T2 t2_thread(const u32 *__restrict__ seg, const u32 *__restrict__ end, const u32 *__restrict__ set, u32 n,
                                        u64 base) {
    T2 acc{0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < SO_IPT; ++k)
        if (base + k < n) acc = t2_op(acc, t2_row(seg, end, set, base + k));
    return acc;
}

__global__ void __launch_bounds__(SO_TPB)
k_t2_tiles(const u32 *__restrict__ seg, const u32 *__restrict__ end, const u32 *__restrict__ set, u32 n, uint4 *__restrict__ agg) {
    __shared__ uint4 lds[SO_TPB];
    const u64 base = (u64)blockIdx.x * SO_TILE + (u64)threadIdx.x * SO_IPT;
    const T2 acc = t2_block_incl<SO_TPB>(t2_thread(seg, end, set, n, base), lds);
    if (threadIdx.x == SO_TPB - 1) agg[blockIdx.x] = t2_pack(acc);
}

// tile aggregates -> exclusive carries, in place (one workgroup)
__global__ void __launch_bounds__(1024) k_t2_carry(uint4 *__restrict__ agg, u32 n_tiles) {
    __shared__ uint4 lds[1024];
    T2 run{0, 0, 0, 0};
    for (u32 b = 0; b < n_tiles; b += 1024) {
        const u32 t = b + threadIdx.x;
        const T2 x = t < n_tiles ? t2_unpack(agg[t]) : T2{0, 0, 0, 0};
        (void)t2_block_incl<1024>(x, lds);
        const T2 ex = threadIdx.x ? t2_op(run, t2_unpack(lds[threadIdx.x - 1])) : run;
        const T2 last = t2_unpack(lds[1023]);
        __syncthreads();
        if (t < n_tiles) agg[t] = t2_pack(ex);
        run = t2_op(run, last);
    }
}

// rows[k], k in [0, n]: the summary of the rows from the head of row k - 1's chromosome to row k - 1, whether row k opens
// a chromosome (row n, past the end, does), and for which sets row k opens a run of "the union without that set":
// reduce()'s rule start > (running max of end over the chromosome so far) with the maximum taken without the set.
// m2 <= m1, so a row past m1 is a head for every set but its own, and a row in (m2, m1] for s1 alone.
__global__ void __launch_bounds__(SO_TPB)
k_t2_apply(const u32 *__restrict__ seg, const u32 *__restrict__ start, const u32 *__restrict__ end, const u32 *__restrict__ set, u32 n,
           const uint4 *__restrict__ carry, uint4 *__restrict__ rows) {
    __shared__ uint4 lds[SO_TPB];
    const u64 base = (u64)blockIdx.x * SO_TILE + (u64)threadIdx.x * SO_IPT;
    (void)t2_block_incl<SO_TPB>(t2_thread(seg, end, set, n, base), lds);
    T2 run = t2_unpack(carry[blockIdx.x]);
    if (threadIdx.x) run = t2_op(run, t2_unpack(lds[threadIdx.x - 1]));
#pragma unroll
    for (int k = 0; k < SO_IPT; ++k) {
        const u64 i = base + k;
        if (i > n) break;
        const bool chr = i == n || is_head(seg, i);
        u32 cls = 0;
        if (i < n) {
            const u32 s = start[i];
            if (chr || !(run.f & T2_V1) || s > run.m1) cls = 1;
            else if (set[i] != run.s1 && (!(run.f & T2_V2) || s > run.m2)) cls = 2;
        }
        rows[i] = make_uint4((run.f & (T2_V1 | T2_V2)) | (chr ? T2_CHR : 0u) | (cls << T2_CLS_SHIFT), run.m1, run.s1, run.m2);
        if (i < n) run = t2_op(run, t2_row(seg, end, set, i));
    }
}

__global__ void k_gather1(const u32 *__restrict__ perm, u32 n, const u32 *__restrict__ a, u32 *__restrict__ oa) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) oa[i] = a[perm[i]];
}

// One workgroup per tile of the sorted rows [0, n]; each wave takes the output sets i = wave, wave + 4, ... < n_out (set
// n_out - 1 owns no row: the union of all) and walks the tile 64 rows at a time: a compare, a ballot and a popcount per
// step.  !WRITE: cnt[i * tiles + tile] = the heads of set i in the tile.  WRITE: head number p of set i (off: the
// exclusive scan of cnt, so set i's runs are one slice of the output) gets its rank, start and own end, and the row
// that ends run p - 1 -- the next head of the chromosome, or the row that opens the next chromosome -- writes the running
// maximum without i up to it into oclose[p - 1].  k_ue_finish picks between the two ends.
template <bool WRITE>
__global__ void __launch_bounds__(SO_TPB)
k_ue_emit(const uint4 *__restrict__ rows, const u32 *__restrict__ sset, const u32 *__restrict__ seg, const u32 *__restrict__ start,
          const u32 *__restrict__ end, u32 n, u32 n_out, u32 tiles, u32 *__restrict__ cnt, const u64 *__restrict__ off,
          u32 *__restrict__ oseg, u32 *__restrict__ ostart, u32 *__restrict__ oend, u32 *__restrict__ oclose) {
    __shared__ u32 l_f[SO_TILE], l_m1[SO_TILE], l_s1[SO_TILE], l_m2[SO_TILE], l_own[SO_TILE];
    const u64 t0 = (u64)blockIdx.x * SO_TILE;
    for (u32 j = threadIdx.x; j < SO_TILE; j += SO_TPB) {
        const u64 k = t0 + j;
        const uint4 e = k <= n ? rows[k] : make_uint4(0, 0, 0, 0);
        l_f[j] = e.x;
        l_m1[j] = e.y;
        l_s1[j] = e.z;
        l_m2[j] = e.w;
        l_own[j] = k < n ? sset[k] : 0xFFFFFFFFu;
    }
    __syncthreads();
    const u32 lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u32 live = (u32)min((u64)SO_TILE, (u64)n + 1 - t0), chunks = (live + 63) / 64;
    for (u32 i = wave; i < n_out; i += SO_TPB / 64) {
        const u64 base = WRITE ? off[(u64)i * tiles + blockIdx.x] : 0;
        u32 c = 0;
        for (u32 ch = 0; ch < chunks; ++ch) {
            const u32 j = ch * 64 + lane;
            const u32 f = l_f[j], s1 = l_s1[j], cls = (f >> T2_CLS_SHIFT) & 3u;
            const bool head = (cls == 1 && l_own[j] != i) || (cls == 2 && s1 == i);
            const u64 b = __ballot(head);
            if (WRITE) {
                const u64 p = base + c + __popcll(b & ((1ull << lane) - 1ull));
                if (head) {
                    const u64 k = t0 + j;
                    oseg[p] = seg[k];
                    ostart[p] = start[k];
                    oend[p] = end[k];
                }
                if ((head || (f & T2_CHR)) && (f & (s1 == i ? T2_V2 : T2_V1))) oclose[p - 1] = s1 == i ? l_m2[j] : l_m1[j];
            }
            c += (u32)__popcll(b);
        }
        if (!WRITE && lane == 0) cnt[(u64)i * tiles + blockIdx.x] = c;
    }
}

// A run whose head is inverted (start > end) has one row and ends at its own end; every other run ends at the running
// maximum at its last row (the earlier runs of the chromosome ended below its start).
__global__ void k_ue_finish(const u32 *__restrict__ ostart, u32 *__restrict__ oend, const u32 *__restrict__ oclose, u64 m) {
    for (u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x; p < m; p += (u64)gridDim.x * blockDim.x)
        if (ostart[p] <= oend[p]) oend[p] = oclose[p];
}

// out[i] = off[i * tiles], i in [0, n_out]
__global__ void k_ue_slices(const u64 *__restrict__ off, u32 tiles, u32 n_out, u64 *__restrict__ out) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i <= n_out; i += (u64)gridDim.x * blockDim.x) out[i] = off[i * tiles];
}

// ------------------------------------------------------------------------------------------------- intersect_all
// events 2i and 2i + 1: the start and the end of reduced region i (segment = set * nr + rank).  A region that is not
// well-formed (start >= end) never yields a piece of an intersect sweep: its events go to the rank past the last.
__global__ void k_ia_events(const u32 *__restrict__ seg, const u32 *__restrict__ start, const u32 *__restrict__ end, u32 n, u32 nr,
                            u32 *__restrict__ ev_rank, u32 *__restrict__ ev_pos) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        ev_rank[2 * i] = ev_rank[2 * i + 1] = start[i] < end[i] ? seg[i] % nr : nr;
        ev_pos[2 * i] = start[i];
        ev_pos[2 * i + 1] = end[i];
    }
}

// piece [pos[j], pos[j + 1]) when j is the last event at its position, the next event is on the same chromosome and
// every set covers the stretch: the depth after j (opens minus closes so far) is n_sets
template <bool WRITE>
__global__ void k_ia_pieces(const u32 *__restrict__ srank, const u32 *__restrict__ spos, const u64 *__restrict__ co,
                            const u64 *__restrict__ cc, u32 m, u32 nr, u64 n_sets, u32 *__restrict__ keep,
                            const u64 *__restrict__ off, u32 *__restrict__ orank, u32 *__restrict__ ostart, u32 *__restrict__ oend) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < m; j += (u64)gridDim.x * blockDim.x) {
        const bool k = j + 1 < m && srank[j] < nr && srank[j + 1] == srank[j] && spos[j + 1] != spos[j] &&
                       co[j + 1] - cc[j + 1] == n_sets;
        if (!WRITE) {
            keep[j] = k;
        } else if (k) {
            const u64 o = off[j];
            orank[o] = srank[j];
            ostart[o] = spos[j];
            oend[o] = spos[j + 1];
        }
    }
}

// the concatenation of the sets but `skip` (none: sets.size()) on the device, and its size checked
gtars_status list_concat(StreamFrame &fr, const std::vector<SetCols> &sets, size_t skip, DevSet &C) {
    std::vector<SetCols> parts;
    for (size_t k = 0; k < sets.size(); ++k)
        if (k != skip) parts.push_back(sets[k]);
    return upload_concat(fr, parts.data(), parts.size(), C);
}

u64 list_rows(const std::vector<SetCols> &sets) {
    u64 n = 0;
    for (const SetCols &s : sets) n += s.n;
    return n;
}

}  // namespace

gtars_status setops_list_union_except(const std::vector<SetCols> &sets, uint32_t n_rank, uint64_t skip, SetOut &res) {
    res = SetOut();
    const u64 n = list_rows(sets) - (skip < sets.size() ? sets[skip].n : 0);
    GT_TRY(check_sizes(n, n_rank));
    if (!n) return GTARS_OK;
    StreamFrame fr(nullptr);
    DevSet C, R;
    GT_TRY(list_concat(fr, sets, skip, C));
    GT_TRY(dev_reduce(fr, C, n_rank, R));
    GT_TRY(download(fr, R, res));
    return fr.drain();
}

gtars_status setops_list_union_all(const std::vector<SetCols> &sets, uint32_t n_rank, SetOut &res) {
    return setops_list_union_except(sets, n_rank, sets.size(), res);
}

gtars_status setops_list_bulk_union_except(const std::vector<SetCols> &sets, uint32_t n_rank, SetOut &uni, std::vector<SetOut> &except) {
    const u64 n64 = list_rows(sets), n_sets = sets.size();
    uni = SetOut();
    except.assign(n_sets, SetOut());
    GT_TRY(check_sizes(n64, n_rank));
    // one row of counts per output set (every set, and the union of all) and tile of the rows [0, n]
    const u64 tiles64 = n64 / SO_TILE + 1;
    if ((n_sets + 1) * tiles64 > SO_MAX_N)
        return fail(GTARS_ERR_INVALID_ARG, "too many region sets x regions for one bulk_union_except call (" + std::to_string(n_sets) +
                                               " sets, " + std::to_string(n64) + " regions)");
    if (!n64) return GTARS_OK;
    const u32 n = (u32)n64, tiles = (u32)tiles64, n_out = (u32)n_sets + 1;
    StreamFrame fr(nullptr);
    hipStream_t st = fr.st;
    // the concatenation with each row's set, sorted once by (rank, start)
    DevSet C, S;
    u32 *set, *sset, *perm;
    GT_TRY(upload_concat(fr, sets.data(), n_sets, C));
    GT_TRY(fr.alloc(&set, n));
    u64 at = 0;
    for (u32 k = 0; k < n_sets; ++k) {
        if (sets[k].n) hipLaunchKernelGGL(k_fill, dim3(grid_for(sets[k].n)), dim3(256), 0, st, set + at, (u32)sets[k].n, k);
        at += sets[k].n;
    }
    GT_TRY(sorted_set(fr, C, C.seg, nullptr, n_rank, S, &perm));
    GT_TRY(fr.alloc(&sset, n));
    hipLaunchKernelGGL(k_gather1, dim3(grid_for(n)), dim3(256), 0, st, perm, n, set, sset);
    // the top-2 scan, left per row
    uint4 *agg, *rows;
    GT_TRY(fr.alloc(&agg, tiles));
    GT_TRY(fr.alloc(&rows, (size_t)n + 1));
    hipLaunchKernelGGL(k_t2_tiles, dim3(tiles), dim3(SO_TPB), 0, st, S.seg, S.end, sset, n, agg);
    hipLaunchKernelGGL(k_t2_carry, dim3(1), dim3(1024), 0, st, agg, tiles);
    hipLaunchKernelGGL(k_t2_apply, dim3(tiles), dim3(SO_TPB), 0, st, S.seg, S.start, S.end, sset, n, agg, rows);
    // count / scan / write, every output set in one launch
    u32 *cnt;
    const u64 n_cnt = (u64)n_out * tiles;
    GT_TRY(fr.alloc(&cnt, n_cnt));
    hipLaunchKernelGGL(k_ue_emit<false>, dim3(tiles), dim3(SO_TPB), 0, st, rows, sset, S.seg, S.start, S.end, n, n_out, tiles, cnt, nullptr,
                       nullptr, nullptr, nullptr, nullptr);
    GT_HIP(hipGetLastError());
    u64 *off, m = 0, *d_slice;
    GT_TRY(scan_total(fr, cnt, n_cnt, &off, &m));
    if (m > SO_MAX_N) return fail(GTARS_ERR_CAPACITY, "bulk_union_except result too large: need " + std::to_string(m) + " regions");
    u32 *oseg, *ostart, *oend, *oclose;
    GT_TRY(fr.alloc(&oseg, m));
    GT_TRY(fr.alloc(&ostart, m));
    GT_TRY(fr.alloc(&oend, m));
    GT_TRY(fr.alloc(&oclose, m));
    hipLaunchKernelGGL(k_ue_emit<true>, dim3(tiles), dim3(SO_TPB), 0, st, rows, sset, S.seg, S.start, S.end, n, n_out, tiles, nullptr, off,
                       oseg, ostart, oend, oclose);
    hipLaunchKernelGGL(k_ue_finish, dim3(grid_for(m)), dim3(256), 0, st, ostart, oend, oclose, m);
    GT_TRY(fr.alloc(&d_slice, (size_t)n_out + 1));
    hipLaunchKernelGGL(k_ue_slices, dim3(grid_for((u64)n_out + 1)), dim3(256), 0, st, off, tiles, n_out, d_slice);
    GT_HIP(hipGetLastError());
    std::vector<u64> slice;
    GT_TRY(fr.download(slice, d_slice, (size_t)n_out + 1));
    GT_TRY(fr.drain());
    for (u32 i = 0; i < n_out; ++i) {
        SetOut &o = i < n_sets ? except[i] : uni;
        const u64 lo = slice[i], k = slice[i + 1] - lo;
        GT_TRY(fr.download(o.rank, oseg + lo, k));
        GT_TRY(fr.download(o.start, ostart + lo, k));
        GT_TRY(fr.download(o.end, oend + lo, k));
    }
    return fr.drain();
}

gtars_status setops_list_intersect_all(const std::vector<SetCols> &sets, uint32_t n_rank, SetOut &res) {
    const u64 n = list_rows(sets), n_sets = sets.size();
    res = SetOut();
    GT_TRY(check_sizes(2 * n, n_rank));
    const u32 nr = std::max<u32>(n_rank, 1);
    if (n_sets * nr > 0x7FFFFFFFull) return fail(GTARS_ERR_INVALID_ARG, "too many sets x chromosomes for one intersect_all call");
    for (const SetCols &s : sets)
        if (!s.n) return GTARS_OK;  // nothing is in an empty set
    if (!n_sets) return GTARS_OK;
    StreamFrame fr(nullptr);
    hipStream_t st = fr.st;
    // every set reduced in one pass: segment = set * nr + chromosome rank, as the pairwise matrix does
    std::vector<u32> hseg(n);
    DevSet C, R, O;
    C.n = (u32)n;
    GT_TRY(fr.alloc(&C.start, n));
    GT_TRY(fr.alloc(&C.end, n));
    u64 at = 0;
    for (u64 k = 0; k < n_sets; ++k) {
        const SetCols &s = sets[k];
        for (u64 i = 0; i < s.n; ++i) hseg[at + i] = (u32)k * nr + s.rank[i];
        GT_TRY(fr.upload_to(C.start + at, s.start, s.n));
        GT_TRY(fr.upload_to(C.end + at, s.end, s.n));
        at += s.n;
    }
    GT_TRY(fr.upload(&C.seg, hseg.data(), n));
    GT_TRY(dev_reduce(fr, C, (u32)(n_sets * nr), R));
    // the open / close events of the well-formed reduced regions by (rank, position), and the depth along them
    const u32 m = 2 * R.n;
    u32 *ev_rank, *ev_pos, *perm, *srank, *spos, *opens, *closes, *keep;
    GT_TRY(fr.alloc(&ev_rank, m));
    GT_TRY(fr.alloc(&ev_pos, m));
    hipLaunchKernelGGL(k_ia_events, dim3(grid_for(R.n)), dim3(256), 0, st, R.seg, R.start, R.end, R.n, nr, ev_rank, ev_pos);
    GT_TRY(sort_perm(fr, ev_rank, ev_pos, nullptr, m, nr + 1, &perm));
    GT_TRY(fr.alloc(&srank, m));
    GT_TRY(fr.alloc(&spos, m));
    GT_TRY(fr.alloc(&opens, m));
    GT_TRY(fr.alloc(&closes, m));
    hipLaunchKernelGGL(k_dj_gather, dim3(grid_for(m)), dim3(256), 0, st, perm, m, ev_rank, ev_pos, R.start, R.end, srank, spos, opens,
                       closes);
    u64 *co, *cc, *off, t = 0, k = 0;
    GT_TRY(scan_total(fr, opens, m, &co, &t));
    GT_TRY(scan_total(fr, closes, m, &cc, &t));
    GT_TRY(fr.alloc(&keep, m));
    hipLaunchKernelGGL(k_ia_pieces<false>, dim3(grid_for(m)), dim3(256), 0, st, srank, spos, co, cc, m, nr, n_sets, keep, nullptr, nullptr,
                       nullptr, nullptr);
    GT_TRY(scan_total(fr, keep, m, &off, &k));
    GT_TRY(alloc_set(fr, k, O));
    hipLaunchKernelGGL(k_ia_pieces<true>, dim3(grid_for(m)), dim3(256), 0, st, srank, spos, co, cc, m, nr, n_sets, nullptr, off, O.seg,
                       O.start, O.end);
    GT_HIP(hipGetLastError());
    GT_TRY(download(fr, O, res));
    return fr.drain();
}

}  // namespace gtars

// test entry (include/gtars_amd_debug.h): host buffers in and out around seg_max_pass, both forms
extern "C" gtars_status gtars_debug_seg_max(const uint32_t *seg, const uint32_t *val, const uint32_t *start, uint64_t n, uint32_t gap,
                                            int inclusive, uint32_t *out) {
    using namespace gtars;
    return guarded([&]() -> gtars_status {
        if (n && (!seg || !val || !out || (!inclusive && !start))) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        GT_TRY(check_sizes(n, 0));
        if (!n) return GTARS_OK;
        StreamFrame fr(nullptr);
        u32 *d_seg, *d_val, *d_start = nullptr, *d_out;
        GT_TRY(fr.upload(&d_seg, seg, (size_t)n));
        GT_TRY(fr.upload(&d_val, val, (size_t)n));
        if (!inclusive) GT_TRY(fr.upload(&d_start, start, (size_t)n));
        GT_TRY(fr.alloc(&d_out, (size_t)n));
        GT_TRY(seg_max_pass(fr, inclusive != 0, d_seg, d_val, d_start, (u32)n, gap, d_out));
        GT_TRY(fr.download(out, d_out, (size_t)n));
        return fr.drain();
    });
}
