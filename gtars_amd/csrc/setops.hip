// setops.hip -- K8: region-set algebra on the device (gtars-core/src/models/region_set.rs:675-1420,
// gtars-genomicdist/src/region_set_list_ops.rs:20-45): reduce / union, setdiff / intersect, the bp totals behind
// jaccard / coverage / overlap_coefficient, closest, cluster, and the pairwise Jaccard matrix of a list of sets.
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
// Widths and totals are the reference's release-build u32 values: (u32)(end - start), summed modulo 2^32 (u64 on the
// device, truncated), and the intersection is a_bp + b_bp - union_bp in wrapping u32.
#include <algorithm>
#include <limits>
#include <vector>

#include "common.h"
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

inline unsigned grid_for(u64 n, u32 per = 256) { return (unsigned)std::min<u64>(std::max<u64>(1, (n + per - 1) / per), 1u << 16); }

// ---------------------------------------------------------------------------------------------- segmented max-scan
struct SM {
    u32 f, v;  // f: a segment head lies in the span; v: max of the values since the last head
};
__device__ __forceinline__ SM sm_op(SM a, SM b) { return SM{a.f | b.f, b.f ? b.v : max(a.v, b.v)}; }
__device__ __forceinline__ u64 sm_pack(SM a) { return ((u64)a.f << 32) | a.v; }
__device__ __forceinline__ SM sm_unpack(u64 x) { return SM{(u32)(x >> 32), (u32)x}; }
__device__ __forceinline__ u32 is_head(const u32 *__restrict__ seg, u64 i) { return i == 0 || seg[i] != seg[i - 1]; }

// inclusive scan across the workgroup; lds[t] holds thread t's inclusive value afterwards
template <int TPB>
__device__ __forceinline__ SM block_incl(SM x, u64 *lds) {
    const int t = threadIdx.x;
    lds[t] = sm_pack(x);
    __syncthreads();
    for (int d = 1; d < TPB; d <<= 1) {
        SM y = x;
        if (t >= d) y = sm_op(sm_unpack(lds[t - d]), x);
        __syncthreads();
        lds[t] = sm_pack(y);
        x = y;
        __syncthreads();
    }
    return x;
}

__global__ void __launch_bounds__(SO_TPB)
k_sm_tiles(const u32 *__restrict__ seg, const u32 *__restrict__ val, u32 n, u64 *__restrict__ agg) {
    __shared__ u64 lds[SO_TPB];
    const u64 base = (u64)blockIdx.x * SO_TILE + (u64)threadIdx.x * SO_IPT;
    SM acc{0, 0};
#pragma unroll
    for (int k = 0; k < SO_IPT; ++k)
        if (base + k < n) acc = sm_op(acc, SM{is_head(seg, base + k), val[base + k]});
    acc = block_incl<SO_TPB>(acc, lds);
    if (threadIdx.x == SO_TPB - 1) agg[blockIdx.x] = sm_pack(acc);
}

// tile aggregates -> exclusive carries, in place (one workgroup)
__global__ void __launch_bounds__(1024) k_sm_carry(u64 *__restrict__ agg, u32 n_tiles) {
    __shared__ u64 lds[1024];
    SM run{0, 0};
    for (u32 b = 0; b < n_tiles; b += 1024) {
        const u32 t = b + threadIdx.x;
        const SM x = t < n_tiles ? sm_unpack(agg[t]) : SM{0, 0};
        (void)block_incl<1024>(x, lds);
        const SM ex = threadIdx.x ? sm_op(run, sm_unpack(lds[threadIdx.x - 1])) : run;
        const SM last = sm_unpack(lds[1023]);
        __syncthreads();
        if (t < n_tiles) agg[t] = sm_pack(ex);
        run = sm_op(run, last);
    }
}

// INCL: out[i] = max of val over [segment head, i].  Else: out[i] = 1 where i opens a run: a head, or
// start[i] > sat(max of val over [head, i) + gap).
template <bool INCL>
__global__ void __launch_bounds__(SO_TPB)
k_sm_apply(const u32 *__restrict__ seg, const u32 *__restrict__ val, const u32 *__restrict__ start, u32 n,
           const u64 *__restrict__ carry, u32 gap, u32 *__restrict__ out) {
    __shared__ u64 lds[SO_TPB];
    const u64 base = (u64)blockIdx.x * SO_TILE + (u64)threadIdx.x * SO_IPT;
    SM acc{0, 0};
#pragma unroll
    for (int k = 0; k < SO_IPT; ++k)
        if (base + k < n) acc = sm_op(acc, SM{is_head(seg, base + k), val[base + k]});
    (void)block_incl<SO_TPB>(acc, lds);
    SM run = sm_unpack(carry[blockIdx.x]);
    if (threadIdx.x) run = sm_op(run, sm_unpack(lds[threadIdx.x - 1]));
#pragma unroll
    for (int k = 0; k < SO_IPT; ++k) {
        const u64 i = base + k;
        if (i >= n) break;
        const SM x{is_head(seg, i), val[i]};
        if (INCL) {
            run = sm_op(run, x);
            out[i] = run.v;
        } else {
            const u32 lim = run.v > 0xFFFFFFFFu - gap ? 0xFFFFFFFFu : run.v + gap;  // saturating_add
            out[i] = (x.f || start[i] > lim) ? 1u : 0u;
            run = sm_op(run, x);
        }
    }
}

gtars_status seg_max_pass(bool incl, const u32 *seg, const u32 *val, const u32 *start, u32 n, u32 gap, u32 *out, StreamFrame &fr,
                          hipStream_t st) {
    if (!n) return GTARS_OK;
    const u32 tiles = (n + SO_TILE - 1) / SO_TILE;
    u64 *agg = nullptr;
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

// exclusive scan of u32 flags / counts; returns the total
gtars_status scan_counts(const u32 *cnt, u32 n, u64 **off, u64 *total, StreamFrame &fr, hipStream_t st) {
    GT_TRY(fr.alloc(off, (size_t)n + 1));
    void *ws = nullptr;
    const size_t wsb = scan_ws_bytes(n);
    GT_TRY(fr.alloc((u8 **)&ws, wsb));
    GT_TRY(launch_scan_u32_to_u64(cnt, n, *off, ws, wsb, st));
    GT_HIP(hipMemcpyAsync(total, *off + n, sizeof(u64), hipMemcpyDeviceToHost, st));
    GT_HIP(hipStreamSynchronize(st));
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

__device__ __forceinline__ u32 first_gt(const u32 *__restrict__ x, u32 lo, u32 hi, u32 key) {
    while (lo < hi) {
        const u32 m = lo + ((hi - lo) >> 1);
        if (x[m] > key) hi = m;
        else lo = m + 1;
    }
    return lo;
}
__device__ __forceinline__ u32 first_ge(const u32 *__restrict__ x, u32 lo, u32 hi, u32 key) {
    while (lo < hi) {
        const u32 m = lo + ((hi - lo) >> 1);
        if (x[m] >= key) hi = m;
        else lo = m + 1;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------------------- reduce
struct DevSet {
    u32 *seg = nullptr, *start = nullptr, *end = nullptr;
    u32 n = 0;
};

// reduce() of n device regions (unsorted) whose segment keys are < n_seg
gtars_status dev_reduce(const u32 *seg, const u32 *start, const u32 *end, u32 n, u32 n_seg, StreamFrame &fr, hipStream_t st, DevSet &out) {
    out = DevSet();
    if (!n) return GTARS_OK;
    u32 *perm, *sseg, *sstart, *send, *flag, *rid, *rmax;
    GT_TRY(fr.alloc(&perm, n));
    const size_t sb = device_sort_perm_ws_bytes(n);
    u8 *scratch;
    GT_TRY(fr.alloc(&scratch, sb));
    GT_TRY(device_sort_perm_ws(seg, start, nullptr, n, n_seg, perm, scratch, sb, st));  // (segment, start), ties in input order
    GT_TRY(fr.alloc(&sseg, n));
    GT_TRY(fr.alloc(&sstart, n));
    GT_TRY(fr.alloc(&send, n));
    hipLaunchKernelGGL(k_gather3, dim3(grid_for(n)), dim3(256), 0, st, perm, n, seg, start, end, sseg, sstart, send);
    GT_TRY(fr.alloc(&flag, n));
    GT_TRY(seg_max_pass(false, sseg, send, sstart, n, 0, flag, fr, st));
    u64 *off, m = 0;
    GT_TRY(scan_counts(flag, n, &off, &m, fr, st));
    GT_TRY(fr.alloc(&rid, n));
    hipLaunchKernelGGL(k_run_ids, dim3(grid_for(n)), dim3(256), 0, st, flag, off, n, rid);
    GT_TRY(fr.alloc(&rmax, n));
    GT_TRY(seg_max_pass(true, rid, send, nullptr, n, 0, rmax, fr, st));
    out.n = (u32)m;
    GT_TRY(fr.alloc(&out.seg, m));
    GT_TRY(fr.alloc(&out.start, m));
    GT_TRY(fr.alloc(&out.end, m));
    hipLaunchKernelGGL(k_reduce_write, dim3(grid_for(n)), dim3(256), 0, st, sseg, sstart, flag, rid, rmax, n, out.seg, out.start,
                       out.end);
    GT_HIP(hipGetLastError());
    return GTARS_OK;
}

gtars_status upload_set(const SetCols &a, StreamFrame &fr, hipStream_t st, u32 **seg, u32 **start, u32 **end) {
    GT_TRY(fr.upload(seg, a.rank, a.n, st));
    GT_TRY(fr.upload(start, a.start, a.n, st));
    return fr.upload(end, a.end, a.n, st);
}

gtars_status download(const DevSet &d, hipStream_t st, SetOut &out) {
    out.rank.resize(d.n);
    out.start.resize(d.n);
    out.end.resize(d.n);
    if (d.n) {
        GT_HIP(hipMemcpyAsync(out.rank.data(), d.seg, (size_t)d.n * 4, hipMemcpyDeviceToHost, st));
        GT_HIP(hipMemcpyAsync(out.start.data(), d.start, (size_t)d.n * 4, hipMemcpyDeviceToHost, st));
        GT_HIP(hipMemcpyAsync(out.end.data(), d.end, (size_t)d.n * 4, hipMemcpyDeviceToHost, st));
    }
    GT_HIP(hipStreamSynchronize(st));
    return GTARS_OK;
}

gtars_status check_sizes(u64 n, u32 n_rank) {
    if (n > SO_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "region set too large for the device set operations (" + std::to_string(n) + " regions)");
    if (n_rank > 0x7FFFFFFFu) return fail(GTARS_ERR_INVALID_ARG, "too many chromosomes");
    return require_device();
}

gtars_status reduce_cols(const SetCols &a, u32 n_rank, StreamFrame &fr, hipStream_t st, DevSet &out) {
    u32 *seg, *start, *end;
    GT_TRY(upload_set(a, fr, st, &seg, &start, &end));
    return dev_reduce(seg, start, end, (u32)a.n, n_rank, fr, st, out);
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
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rank || !dirty[r]) return;
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

template <int MODE>
gtars_status dev_sweep(const DevSet &A, const DevSet &B, u32 n_rank, StreamFrame &fr, hipStream_t st, DevSet &out) {
    out = DevSet();
    if (!A.n) return GTARS_OK;
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
    GT_TRY(scan_counts(cnt, A.n, &off, &m, fr, st));
    if (m > SO_MAX_N) return fail(GTARS_ERR_CAPACITY, "set operation result too large: need " + std::to_string(m));
    out.n = (u32)m;
    GT_TRY(fr.alloc(&out.seg, m));
    GT_TRY(fr.alloc(&out.start, m));
    GT_TRY(fr.alloc(&out.end, m));
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
    hipStream_t st = nullptr;
    StreamFrame fr(st);
    DevSet A, B, R;
    GT_TRY(reduce_cols(a, n_rank, fr, st, A));
    GT_TRY(reduce_cols(b, n_rank, fr, st, B));
    GT_TRY(dev_sweep<MODE>(A, B, n_rank, fr, st, R));
    return download(R, st, res);
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
    hipStream_t st = nullptr;
    StreamFrame fr(st);
    DevSet R;
    GT_TRY(reduce_cols(a, n_rank, fr, st, R));
    return download(R, st, res);
}

gtars_status setops_setdiff(const SetCols &a, const SetCols &b, uint32_t n_rank, SetOut &res) {
    return two_set<SWEEP_SETDIFF>(a, b, n_rank, res);
}

gtars_status setops_intersect(const SetCols &a, const SetCols &b, uint32_t n_rank, SetOut &res) {
    return two_set<SWEEP_INTERSECT>(a, b, n_rank, res);
}

gtars_status setops_totals(const SetCols &a, const SetCols &b, uint32_t n_rank, bool want_diff, SetTotals &out) {
    GT_TRY(check_sizes(a.n + b.n, n_rank));
    hipStream_t st = nullptr;
    StreamFrame fr(st);
    // a and b side by side: reduce(a), reduce(b) and reduce(concat(a, b)) from the same columns
    const u64 n = a.n + b.n;
    u32 *seg, *start, *end;
    GT_TRY(fr.alloc(&seg, n));
    GT_TRY(fr.alloc(&start, n));
    GT_TRY(fr.alloc(&end, n));
    const SetCols *parts[2] = {&a, &b};
    u64 at = 0;
    for (const SetCols *p : parts) {
        if (p->n) {
            GT_HIP(hipMemcpyAsync(seg + at, p->rank, p->n * 4, hipMemcpyHostToDevice, st));
            GT_HIP(hipMemcpyAsync(start + at, p->start, p->n * 4, hipMemcpyHostToDevice, st));
            GT_HIP(hipMemcpyAsync(end + at, p->end, p->n * 4, hipMemcpyHostToDevice, st));
        }
        at += p->n;
    }
    DevSet A, B, U, D;
    GT_TRY(dev_reduce(seg, start, end, (u32)a.n, n_rank, fr, st, A));
    GT_TRY(dev_reduce(seg + a.n, start + a.n, end + a.n, (u32)b.n, n_rank, fr, st, B));
    GT_TRY(dev_reduce(seg, start, end, (u32)n, n_rank, fr, st, U));
    if (want_diff) GT_TRY(dev_sweep<SWEEP_SETDIFF>(A, B, n_rank, fr, st, D));
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
    GT_HIP(hipMemcpyAsync(h, acc, sizeof h, hipMemcpyDeviceToHost, st));
    GT_HIP(hipStreamSynchronize(st));
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
    hipStream_t st = nullptr;
    StreamFrame fr(st);
    const u32 no = (u32)other.n, nq = (u32)a.n;
    // candidates: `other` stably sorted by (chromosome, start)
    u32 *oseg, *ostart, *oend, *perm, *cseg, *cs, *ce, *coff, *maxw;
    GT_TRY(upload_set(other, fr, st, &oseg, &ostart, &oend));
    GT_TRY(fr.alloc(&perm, no));
    const size_t sb = device_sort_perm_ws_bytes(no);
    u8 *scratch;
    GT_TRY(fr.alloc(&scratch, sb));
    GT_TRY(device_sort_perm_ws(oseg, ostart, nullptr, no, n_rank, perm, scratch, sb, st));
    GT_TRY(fr.alloc(&cseg, no));
    GT_TRY(fr.alloc(&cs, no));
    GT_TRY(fr.alloc(&ce, no));
    hipLaunchKernelGGL(k_gather3, dim3(grid_for(no)), dim3(256), 0, st, perm, no, oseg, ostart, oend, cseg, cs, ce);
    GT_TRY(fr.alloc(&coff, (size_t)n_rank + 1));
    hipLaunchKernelGGL(k_seg_offsets, dim3(grid_for((u64)no + 1)), dim3(256), 0, st, cseg, no, n_rank, coff);
    GT_TRY(fr.alloc(&maxw, n_rank));
    GT_HIP(hipMemsetAsync(maxw, 0, (size_t)std::max<u32>(n_rank, 1) * 4, st));
    hipLaunchKernelGGL(k_max_width, dim3(grid_for((no + 63) / 64)), dim3(256), 0, st, cseg, cs, ce, no, maxw);
    u32 *qr, *qs, *qe, *found, *bidx;
    i64 *bd;
    GT_TRY(upload_set(a, fr, st, &qr, &qs, &qe));
    GT_TRY(fr.alloc(&found, nq));
    GT_TRY(fr.alloc(&bidx, nq));
    GT_TRY(fr.alloc(&bd, nq));
    hipLaunchKernelGGL(k_closest, dim3(grid_for(nq)), dim3(256), 0, st, qr, qs, qe, nq, cs, ce, perm, coff, maxw, n_rank, found, bidx, bd);
    GT_HIP(hipGetLastError());
    u64 *off, m = 0;
    GT_TRY(scan_counts(found, nq, &off, &m, fr, st));
    u32 *o_self, *o_other;
    i64 *o_d;
    GT_TRY(fr.alloc(&o_self, m));
    GT_TRY(fr.alloc(&o_other, m));
    GT_TRY(fr.alloc(&o_d, m));
    hipLaunchKernelGGL(k_closest_compact, dim3(grid_for(nq)), dim3(256), 0, st, found, off, bidx, bd, nq, o_self, o_other, o_d);
    GT_HIP(hipGetLastError());
    self_idx.resize(m);
    other_idx.resize(m);
    dist.resize(m);
    if (m) {
        GT_HIP(hipMemcpyAsync(self_idx.data(), o_self, m * 4, hipMemcpyDeviceToHost, st));
        GT_HIP(hipMemcpyAsync(other_idx.data(), o_other, m * 4, hipMemcpyDeviceToHost, st));
        GT_HIP(hipMemcpyAsync(dist.data(), o_d, m * 8, hipMemcpyDeviceToHost, st));
    }
    GT_HIP(hipStreamSynchronize(st));
    return GTARS_OK;
}

gtars_status setops_cluster(const SetCols &a, uint32_t n_rank, uint32_t max_gap, uint32_t *ids) {
    GT_TRY(check_sizes(a.n, n_rank));
    if (!a.n) return GTARS_OK;
    hipStream_t st = nullptr;
    StreamFrame fr(st);
    const u32 n = (u32)a.n;
    u32 *seg, *start, *end, *perm, *sseg, *sstart, *send, *flag, *d_ids;
    GT_TRY(upload_set(a, fr, st, &seg, &start, &end));
    GT_TRY(fr.alloc(&perm, n));
    const size_t sb = device_sort_perm_ws_bytes(n);
    u8 *scratch;
    GT_TRY(fr.alloc(&scratch, sb));
    GT_TRY(device_sort_perm_ws(seg, start, end, n, n_rank, perm, scratch, sb, st));  // (chromosome, start, end)
    GT_TRY(fr.alloc(&sseg, n));
    GT_TRY(fr.alloc(&sstart, n));
    GT_TRY(fr.alloc(&send, n));
    hipLaunchKernelGGL(k_gather3, dim3(grid_for(n)), dim3(256), 0, st, perm, n, seg, start, end, sseg, sstart, send);
    GT_TRY(fr.alloc(&flag, n));
    GT_TRY(seg_max_pass(false, sseg, send, sstart, n, max_gap, flag, fr, st));
    u64 *off, m = 0;
    GT_TRY(scan_counts(flag, n, &off, &m, fr, st));
    GT_TRY(fr.alloc(&d_ids, n));
    hipLaunchKernelGGL(k_cluster_scatter, dim3(grid_for(n)), dim3(256), 0, st, perm, flag, off, n, d_ids);
    GT_HIP(hipGetLastError());
    GT_HIP(hipMemcpyAsync(ids, d_ids, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    GT_HIP(hipStreamSynchronize(st));
    return GTARS_OK;
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
    hipStream_t st = nullptr;
    StreamFrame fr(st);
    // every set reduced in one pass: segment = set * n_rank + chromosome rank
    std::vector<u32> hseg(n);
    u32 *seg, *start, *end;
    GT_TRY(fr.alloc(&start, n));
    GT_TRY(fr.alloc(&end, n));
    u64 at = 0;
    for (u64 k = 0; k < n_sets; ++k) {
        const SetCols &s = sets[k];
        for (u64 i = 0; i < s.n; ++i) hseg[at + i] = (u32)k * nr + s.rank[i];
        if (s.n) {
            GT_HIP(hipMemcpyAsync(start + at, s.start, s.n * 4, hipMemcpyHostToDevice, st));
            GT_HIP(hipMemcpyAsync(end + at, s.end, s.n * 4, hipMemcpyHostToDevice, st));
        }
        at += s.n;
    }
    GT_TRY(fr.upload(&seg, hseg.data(), n, st));
    DevSet R;
    GT_TRY(dev_reduce(seg, start, end, (u32)n, n_seg, fr, st, R));
    u32 *seg_off, *dirty, *w, *d_set_off;
    GT_TRY(fr.alloc(&seg_off, (size_t)n_seg + 1));
    hipLaunchKernelGGL(k_seg_offsets, dim3(grid_for((u64)R.n + 1)), dim3(256), 0, st, R.seg, R.n, n_seg, seg_off);
    GT_TRY(fr.alloc(&dirty, n_sets));
    GT_HIP(hipMemsetAsync(dirty, 0, n_sets * 4, st));
    hipLaunchKernelGGL(k_mark_inverted, dim3(grid_for(R.n)), dim3(256), 0, st, R.seg, R.start, R.end, R.n, nr, dirty);
    GT_TRY(fr.alloc(&w, R.n));
    hipLaunchKernelGGL(k_widths, dim3(grid_for(R.n)), dim3(256), 0, st, R.start, R.end, R.n, w);
    u64 *P, total = 0;
    GT_TRY(scan_counts(w, R.n, &P, &total, fr, st));
    std::vector<u32> h_seg_off((size_t)n_seg + 1), h_dirty(n_sets), set_off(n_sets + 1);
    GT_HIP(hipMemcpyAsync(h_seg_off.data(), seg_off, h_seg_off.size() * 4, hipMemcpyDeviceToHost, st));
    GT_HIP(hipMemcpyAsync(h_dirty.data(), dirty, n_sets * 4, hipMemcpyDeviceToHost, st));
    GT_HIP(hipStreamSynchronize(st));
    for (u64 k = 0; k <= n_sets; ++k) set_off[k] = h_seg_off[k * nr];
    GT_TRY(fr.upload(&d_set_off, set_off.data(), set_off.size(), st));
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
        GT_TRY(fr.upload(&d_pairs, pairs.data(), pairs.size(), st));
        GT_TRY(fr.alloc(&inter, pairs.size()));
        GT_HIP(hipMemsetAsync(inter, 0, pairs.size() * 8, st));
        if (!items.empty()) {
            GT_TRY(fr.upload(&d_items, items.data(), items.size(), st));
            for (size_t b = 0; b < items.size(); b += (1u << 20)) {  // grids of at most 2^20 workgroups
                const size_t nb = std::min<size_t>(items.size() - b, 1u << 20);
                hipLaunchKernelGGL(k_pair_inter, dim3((unsigned)nb), dim3(256), 0, st, d_items + b, R.seg, R.start, R.end, P, d_set_off,
                                   seg_off, nr, inter);
            }
        }
        GT_TRY(fr.alloc(&dM, n_sets * n_sets));
        GT_HIP(hipMemcpyAsync(dM, out, n_sets * n_sets * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_pair_finish, dim3(grid_for(pairs.size())), dim3(256), 0, st, d_pairs, (u32)pairs.size(), inter, P, d_set_off,
                           (u32)n_sets, dM);
        GT_HIP(hipGetLastError());
        GT_HIP(hipMemcpyAsync(out, dM, n_sets * n_sets * 8, hipMemcpyDeviceToHost, st));
        GT_HIP(hipStreamSynchronize(st));
    }
    if (!dirty_pairs.empty()) {
        // a set that keeps an inverted region: the two-set path on the reduced sets, both orders
        SetOut h;
        GT_TRY(download(R, st, h));
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

}  // namespace gtars
