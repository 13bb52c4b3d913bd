// uniwig_stream.hip -- K24: the streaming uniwig on the device (gtars-uniwig/src/stream.rs: UniwigStreamProcessor).
//
// The reference is a stateful line-by-line processor over a deque.  For any input order it reduces to the closed form of
// uniwig_stream.h (tests/uniwig_stream_ref.py restates the processor statement by statement, tests/test_uniwig_stream_cpu.py
// holds the two against each other).  The whole file goes through ONE chain of launches, whose length does not depend on
// the number of chromosome runs:
//
//   1. k_sw_window: one lane per row -> ws, we, the keep flag of the core track, the first row out of range.  Dropped core
//      rows are compacted out (scan_total, k_sw_compact).
//   2. the plan.  k_sw_plan_tiles / _carry / _apply: the segmented inclusive maximum of ws (M) and the exclusive one of
//      we (B) over the runs -- SegMax over block_scan and carry_walk of scan.h -- and from them the segment head flags;
//      their scan numbers the segments.  k_sw_seg_fill / k_sw_seg_len: the segment table (chromosome, first position,
//      length), the dense-mode lead and tail included; the scan of the lengths is every segment's offset in the
//      compacted output.  A later segment of a run begins behind every earlier window of the run, so the run's running
//      maximum of we at a segment's last row is the segment's last position.
//   3. events in compacted coordinates.  open_i = off[seg] + (M_i - first[seg]) ascends as the rows stand;
//      close_i = off[seg] + (we_i + 1 - first[seg]) is sorted with sort_perm by (segment, we + 1) -- the order by
//      (run, we + 1), as a run's segments ascend -- and the scores go along.  A row that adds nothing (score 0, or
//      we_i < M_i) keeps its place in both columns with weight 0 and closes where it opens.  Exclusive prefix sums of the
//      weights in both orders (scan_total; read modulo 2^32).
//   4. k_sw_tile: the coverage tile skeleton of cov_tile.h, which K11's k_cov_tile shares, over the compacted index space
//      with the event source SwSrc -- u64 keys, a weight per event, so a span is entered with
//      prefix_open[ia] - prefix_close[ie] and a run of equal keys inside a wave adds the SUM of its weights.
//      A close one past its segment's end lands on the next segment's first slot, where the count has to drop anyway.
//   5. step > 1: the window is computed at step 1 and k_sw_decimate keeps the positions with (pos - 1) % step == 0.
#include <algorithm>
#include <cstdlib>
#include <memory>
#include <vector>

#include "common.h"
#include "cov_tile.h"
#include "pipeline.h"
#include "scan.h"
#include "uniwig.h"
#include "uniwig_stream.h"

namespace gtars {

struct SwPlan {
    u64 n = 0;                               // rows that are left after the core track's drop
    std::vector<u32> seg_cid, seg_first, seg_len;
    std::vector<u64> seg_off;                // n_seg + 1
    DevBuf<u64> A, E, PA, PE, d_seg_off;     // opens, closes (ascending), exclusive weight sums (n + 1)
    DevBuf<u32> SA, SE, d_seg_first;         // weights in open and in close order
    int device = -1;
};

namespace {

constexpr u32 SW_NO_ROW = 0xFFFFFFFFu;  // k_sw_window found no row out of range
constexpr int PL_TPB = 256;
constexpr int PL_IPT = 8;
constexpr u32 PL_TILE = PL_TPB * PL_IPT;

using SMax = SegMax<u32>;

__device__ __forceinline__ u32 sw_is_head(const u32 *__restrict__ cid, u64 i) { return i == 0 || cid[i] != cid[i - 1]; }

// ---- 1. windows ---------------------------------------------------------------------------------------------------------
__global__ void k_sw_window(const u32 *__restrict__ cid, const u32 *__restrict__ start, const u32 *__restrict__ end,
                            const u32 *__restrict__ score, u64 n, u32 n_chrom, u32 m, int kind, u32 *__restrict__ ws,
                            u32 *__restrict__ we, u32 *__restrict__ keep, u32 *__restrict__ bad) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;  // (exactly ceil(n / 256) workgroups: sw_blocks)
    if (i >= n) return;
    const u64 s = start[i], e = end[i];
    const u64 limit = 0x7FFFFFFFull - m - 1;
    if (s > limit || e > limit || score[i] > 0x7FFFFFFFu || cid[i] >= n_chrom) {
        atomicMin(bad, (u32)i);
        ws[i] = 1, we[i] = 1, keep[i] = 0;
        return;
    }
    i64 a, b;
    if (kind == GTARS_UNIWIG_CORE) {
        a = (i64)s + 1, b = (i64)e - 1;
    } else {
        const i64 c = kind == GTARS_UNIWIG_START ? (i64)s + 1 : (i64)e;
        a = max((i64)1, c - (i64)m), b = c + (i64)m;
    }
    const bool k = b >= a || kind != GTARS_UNIWIG_CORE;
    ws[i] = (u32)a;
    we[i] = k ? (u32)b : 0u;
    keep[i] = k ? 1u : 0u;
}

__global__ void k_sw_compact(const u32 *__restrict__ keep, const u64 *__restrict__ off, u64 n, const u32 *__restrict__ cid,
                             const u32 *__restrict__ ws, const u32 *__restrict__ we, const u32 *__restrict__ sc,
                             u32 *__restrict__ ocid, u32 *__restrict__ ows, u32 *__restrict__ owe, u32 *__restrict__ osc) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;  // (exactly ceil(n / 256) workgroups: sw_blocks)
    if (i >= n) return;
    if (!keep[i]) return;
    const u64 o = off[i];
    ocid[o] = cid[i], ows[o] = ws[i], owe[o] = we[i], osc[o] = sc[i];
}

// ---- 2. the plan ----------------------------------------------------------------------------------------------------------
// a thread's PL_IPT rows folded in order; rows past n are the identity
__device__ __forceinline__ void pl_thread(const u32 *__restrict__ cid, const u32 *__restrict__ ws, const u32 *__restrict__ we, u32 n,
                                          u64 base, SMax::T &w, SMax::T &e) {
    w = e = SMax::identity();
#pragma unroll
    for (int k = 0; k < PL_IPT; ++k)
        if (base + k < n) {
            const u32 h = sw_is_head(cid, base + k);
            w = SMax::op(w, SMax::T{h, ws[base + k]});
            e = SMax::op(e, SMax::T{h, we[base + k]});
        }
}

__global__ void __launch_bounds__(PL_TPB)
k_sw_plan_tiles(const u32 *__restrict__ cid, const u32 *__restrict__ ws, const u32 *__restrict__ we, u32 n, SMax::T *__restrict__ agg_w,
                SMax::T *__restrict__ agg_e) {
    __shared__ SMax::T lds[PL_TPB / 64];
    const u64 base = (u64)blockIdx.x * PL_TILE + (u64)threadIdx.x * PL_IPT;
    SMax::T w, e, excl, tot_w, tot_e;
    pl_thread(cid, ws, we, n, base, w, e);
    (void)block_scan<SMax, PL_TPB>(w, lds, excl, tot_w);
    (void)block_scan<SMax, PL_TPB>(e, lds, excl, tot_e);
    if (threadIdx.x == 0) agg_w[blockIdx.x] = tot_w, agg_e[blockIdx.x] = tot_e;
}

__global__ void __launch_bounds__(1024) k_sw_plan_carry(SMax::T *__restrict__ agg_w, SMax::T *__restrict__ agg_e, u32 n_tiles) {
    __shared__ SMax::T lds[1024 / 64];
    (void)carry_walk<SMax>(agg_w, n_tiles, lds);
    (void)carry_walk<SMax>(agg_e, n_tiles, lds);
}

// M[i]: the run's inclusive maximum of ws; binc[i]: its inclusive maximum of we; flag[i]: row i opens a segment
__global__ void __launch_bounds__(PL_TPB)
k_sw_plan_apply(const u32 *__restrict__ cid, const u32 *__restrict__ ws, const u32 *__restrict__ we, u32 n,
                const SMax::T *__restrict__ carry_w, const SMax::T *__restrict__ carry_e, int dense, u64 max_gap, u32 *__restrict__ M,
                u32 *__restrict__ binc, u32 *__restrict__ flag) {
    __shared__ SMax::T lds[PL_TPB / 64];
    const u64 base = (u64)blockIdx.x * PL_TILE + (u64)threadIdx.x * PL_IPT;
    SMax::T w, e, ex_w, ex_e, tot;
    pl_thread(cid, ws, we, n, base, w, e);
    (void)block_scan<SMax, PL_TPB>(w, lds, ex_w, tot);
    (void)block_scan<SMax, PL_TPB>(e, lds, ex_e, tot);
    SMax::T run_w = SMax::op(carry_w[blockIdx.x], ex_w), run_e = SMax::op(carry_e[blockIdx.x], ex_e);
#pragma unroll
    for (int k = 0; k < PL_IPT; ++k) {
        const u64 i = base + k;
        if (i >= n) break;
        const u32 h = sw_is_head(cid, i);
        const u64 b = run_e.v;  // the exclusive maximum of we (of the run in front for a head, which does not look at it)
        run_w = SMax::op(run_w, SMax::T{h, ws[i]});
        run_e = SMax::op(run_e, SMax::T{h, we[i]});
        const u64 mi = run_w.v;
        const bool open = h || (mi > b + 1 && !dense && mi - b - 1 > max_gap);
        M[i] = run_w.v;
        binc[i] = run_e.v;
        flag[i] = open ? 1u : 0u;
    }
}

// seg[i]; the head row writes its segment's chromosome and first position, the last row its last position
__global__ void k_sw_seg_fill(const u32 *__restrict__ cid, const u32 *__restrict__ M, const u32 *__restrict__ binc,
                              const u32 *__restrict__ flag, const u64 *__restrict__ soff, u64 n, int dense,
                              const u32 *__restrict__ sizes, u32 *__restrict__ seg, u32 *__restrict__ seg_cid, u32 *__restrict__ seg_first,
                              u32 *__restrict__ seg_last) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;  // (exactly ceil(n / 256) workgroups: sw_blocks)
    if (i >= n) return;
    const u32 s = (u32)(soff[i] + flag[i] - 1);
    seg[i] = s;
    if (flag[i]) {
        seg_cid[s] = cid[i];
        seg_first[s] = dense ? 1u : M[i];
    }
    if (i + 1 == n || flag[i + 1]) {
        u32 last = binc[i];
        if (dense) last = max(last, sizes[cid[i]]);  // (0 for a chromosome without a size)
        seg_last[s] = last;
    }
}

__global__ void k_sw_seg_len(const u32 *__restrict__ first, const u32 *__restrict__ last, u64 n_seg, u32 *__restrict__ len) {
    const u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;  // (exactly ceil(n_seg / 256) workgroups: sw_blocks)
    if (s >= n_seg) return;
    len[s] = last[s] + 1u >= first[s] ? last[s] + 1u - first[s] : 0u;
}

// ---- 3. events ------------------------------------------------------------------------------------------------------------
__global__ void k_sw_events(const u32 *__restrict__ seg, const u32 *__restrict__ M, const u32 *__restrict__ we,
                            const u32 *__restrict__ sc, const u32 *__restrict__ seg_first, const u64 *__restrict__ seg_off, u64 n,
                            u64 *__restrict__ A, u32 *__restrict__ SA, u32 *__restrict__ ckey) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;  // (exactly ceil(n / 256) workgroups: sw_blocks)
    if (i >= n) return;
    const u32 s = seg[i], mi = M[i];
    const bool live = sc[i] != 0 && we[i] >= mi;
    A[i] = seg_off[s] + (mi - seg_first[s]);
    SA[i] = live ? sc[i] : 0u;
    ckey[i] = live ? we[i] + 1u : mi;
}

__global__ void k_sw_closes(const u32 *__restrict__ perm, const u32 *__restrict__ seg, const u32 *__restrict__ ckey,
                            const u32 *__restrict__ SA, const u32 *__restrict__ seg_first, const u64 *__restrict__ seg_off, u64 n,
                            u64 *__restrict__ E, u32 *__restrict__ SE) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;  // (exactly ceil(n / 256) workgroups: sw_blocks)
    if (j >= n) return;
    const u32 p = perm[j], s = seg[p];
    E[j] = seg_off[s] + (ckey[p] - seg_first[s]);
    SE[j] = SA[p];
}

// ---- 4. the tile kernel ---------------------------------------------------------------------------------------------------
// K24's event source over the compacted index space: u64 keys, a u32 weight per event, the exclusive weight sums of both
// columns (read modulo 2^32)
struct SwSrc {
    const u64 *__restrict__ A, *__restrict__ E;
    const u32 *__restrict__ SA, *__restrict__ SE;
    const u64 *__restrict__ PA, *__restrict__ PE;
    u32 n;
    static constexpr bool WEIGHTED = true;

    // the first index whose value is >= pos
    __device__ __forceinline__ u32 lower_bound(const u64 *__restrict__ x, u64 pos) const {
        u32 lo = 0, hi = n;
        while (lo < hi) {
            const u32 mid = lo + ((hi - lo) >> 1);
            if (x[mid] >= pos) hi = mid;
            else lo = mid + 1;
        }
        return lo;
    }
    __device__ __forceinline__ u32 first_open(u64 pos) const { return lower_bound(A, pos); }
    __device__ __forceinline__ u32 first_close(u64 pos) const { return lower_bound(E, pos); }
    __device__ __forceinline__ u32 entering(u32 ia, u32 ie) const { return (u32)PA[ia] - (u32)PE[ie]; }

    __device__ __forceinline__ void open(u64 i, u64 t0, u64 t1, u32 &key, u32 &w) const {
        const u64 v = A[i];
        if (v >= t0 && v < t1) key = (u32)(v - t0), w = SA[i];
    }
    __device__ __forceinline__ void close(u64 i, u64 t0, u64 t1, u32 &key, u32 &w) const {
        const u64 v = E[i];
        if (v >= t0 && v < t1) key = (u32)(v - t0), w = SE[i];
    }
};

// compacted positions w0 + [0, len) into out[0, len); out is 16-byte aligned, span a multiple of COV_TILE
__global__ void __launch_bounds__(COV_TPB)
k_sw_tile(const u64 *__restrict__ A, const u64 *__restrict__ E, const u32 *__restrict__ SA, const u32 *__restrict__ SE,
          const u64 *__restrict__ PA, const u64 *__restrict__ PE, u32 n, u64 w0, u64 len, u64 span, u32 *__restrict__ out) {
    cov_tile_body(SwSrc{A, E, SA, SE, PA, PE, n}, w0, len, span, out);
}

// ---- 5. step > 1 ----------------------------------------------------------------------------------------------------------
// in[0, len): compacted positions w0 + [0, len) at step 1.  The position behind compacted index x is
// first[s] + (x - off[s]) for the segment s with off[s] <= x < off[s + 1]; the kept ones go to out[kept index - k0],
// koff[s] being the number of kept positions in front of segment s.
__global__ void k_sw_decimate(const u32 *__restrict__ in, u64 w0, u64 len, const u64 *__restrict__ off, const u32 *__restrict__ first,
                              const u64 *__restrict__ koff, u32 n_seg, u32 step, u64 k0, u32 *__restrict__ out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;  // (exactly ceil(len / 256) workgroups: sw_blocks)
    if (i >= len) return;
    const u64 x = w0 + i;
    u32 lo = 0, hi = n_seg;  // the first segment with off > x, minus one
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (off[mid] > x) hi = mid;
        else lo = mid + 1;
    }
    const u32 s = lo - 1;
    const u64 f = first[s], q = f - 1 + (x - off[s]);  // q = pos - 1
    if (q % step) return;
    out[koff[s] + (q / step - (f - 1 + step - 1) / step) - k0] = in[i];
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// one thread per element, no loop in the kernels: n is at most 2^32, the grid at most 2^24 workgroups
unsigned sw_blocks(u64 n) { return (unsigned)std::max<u64>(1, (n + 255) / 256); }

gtars_status launch_sw(const SwPlan &p, u64 w_first, u64 w_len, u32 *d_out, hipStream_t st) {
    return cov_tile_launch("k_sw_tile", "uniwig stream", k_sw_tile, st, w_first, w_len, d_out, p.A.p, p.E.p, p.SA.p, p.SE.p, p.PA.p, p.PE.p,
                           (u32)p.n);
}

// positions of [first, first + len) with (pos - 1) % step == 0
u64 sw_kept_in(u64 first, u64 len, u64 step) {
    if (!len) return 0;
    const u64 lo = (first - 1 + step - 1) / step, hi = (first + len - 2) / step;
    return hi >= lo ? hi - lo + 1 : 0;
}

gtars_status build_plan(SwPlan &p, const u32 *cid, const u32 *start, const u32 *end, const u32 *score, u64 n_rows, int on_device,
                        const u32 *sizes, u32 n_chrom, u32 m, int kind, i64 max_gap) {
    p.seg_off.assign(1, 0);
    if (!n_rows) return GTARS_OK;
    StreamFrame fr(nullptr);
    hipStream_t st = fr.st;
    const u64 n0 = n_rows;
    const u32 *d_cid = cid, *d_start = start, *d_end = end, *d_sc = score;
    if (!on_device) {
        u32 *c, *s, *e, *w;
        GT_TRY(fr.upload(&c, cid, (size_t)n0));
        GT_TRY(fr.upload(&s, start, (size_t)n0));
        GT_TRY(fr.upload(&e, end, (size_t)n0));
        GT_TRY(fr.upload(&w, score, (size_t)n0));
        d_cid = c, d_start = s, d_end = e, d_sc = w;
    }
    std::vector<u32> no_sizes(std::max<u32>(n_chrom, 1), 0u);
    u32 *d_sizes;
    GT_TRY(fr.upload(&d_sizes, sizes ? sizes : no_sizes.data(), (size_t)std::max<u32>(n_chrom, 1)));
    // 1. windows
    u32 *ws, *we, *keep, *bad;
    GT_TRY(fr.alloc(&ws, (size_t)n0));
    GT_TRY(fr.alloc(&we, (size_t)n0));
    GT_TRY(fr.alloc(&keep, (size_t)n0));
    GT_TRY(fr.alloc(&bad, 1));
    GT_HIP(hipMemsetAsync(bad, 0xFF, sizeof(u32), st));
    {
        ProfScope ps("k_sw_window", st);
        hipLaunchKernelGGL(k_sw_window, dim3(sw_blocks(n0)), dim3(256), 0, st, d_cid, d_start, d_end, d_sc, n0, n_chrom, m, kind, ws, we, keep,
                           bad);
        GT_HIP(hipGetLastError());
    }
    u32 h_bad = SW_NO_ROW;
    GT_TRY(fr.download(&h_bad, bad, 1));
    u64 n = n0;
    if (kind == GTARS_UNIWIG_CORE) {
        u64 *koff;
        GT_TRY(scan_total(fr, keep, n0, &koff, &n));
        if (h_bad == SW_NO_ROW && n != n0 && n) {
            u32 *c2, *ws2, *we2, *sc2;
            GT_TRY(fr.alloc(&c2, (size_t)n));
            GT_TRY(fr.alloc(&ws2, (size_t)n));
            GT_TRY(fr.alloc(&we2, (size_t)n));
            GT_TRY(fr.alloc(&sc2, (size_t)n));
            ProfScope ps("k_sw_compact", st);
            hipLaunchKernelGGL(k_sw_compact, dim3(sw_blocks(n0)), dim3(256), 0, st, keep, koff, n0, d_cid, ws, we, d_sc, c2, ws2, we2, sc2);
            GT_HIP(hipGetLastError());
            d_cid = c2, ws = ws2, we = we2, d_sc = sc2;
        }
    } else {
        GT_TRY(fr.drain());
    }
    if (h_bad != SW_NO_ROW)
        return fail(GTARS_ERR_INVALID_ARG, "uniwig stream: row " + std::to_string(h_bad) +
                                               " is out of range (start, end and end + smoothsize + 1 must fit an i32, the score "
                                               "an i32, the chromosome id the size table)");
    p.n = n;
    if (!n) return GTARS_OK;
    // 2. the plan
    const u32 n32 = (u32)n;
    const u32 tiles = (n32 + PL_TILE - 1) / PL_TILE;
    const int dense = max_gap < 0;
    SMax::T *agg_w, *agg_e;
    u32 *M, *binc, *flag, *seg;
    GT_TRY(fr.alloc(&agg_w, tiles));
    GT_TRY(fr.alloc(&agg_e, tiles));
    GT_TRY(fr.alloc(&M, (size_t)n));
    GT_TRY(fr.alloc(&binc, (size_t)n));
    GT_TRY(fr.alloc(&flag, (size_t)n));
    GT_TRY(fr.alloc(&seg, (size_t)n));
    {
        ProfScope ps("k_sw_plan", st);
        hipLaunchKernelGGL(k_sw_plan_tiles, dim3(tiles), dim3(PL_TPB), 0, st, d_cid, ws, we, n32, agg_w, agg_e);
        hipLaunchKernelGGL(k_sw_plan_carry, dim3(1), dim3(1024), 0, st, agg_w, agg_e, tiles);
        hipLaunchKernelGGL(k_sw_plan_apply, dim3(tiles), dim3(PL_TPB), 0, st, d_cid, ws, we, n32, agg_w, agg_e, dense,
                           (u64)(dense ? 0 : max_gap), M, binc, flag);
        GT_HIP(hipGetLastError());
    }
    u64 *soff, n_seg = 0;
    GT_TRY(scan_total(fr, flag, n, &soff, &n_seg));
    u32 *seg_cid, *seg_last, *seg_len;
    GT_TRY(fr.alloc(&seg_cid, (size_t)n_seg));
    GT_TRY(fr.alloc(&seg_last, (size_t)n_seg));
    GT_TRY(fr.alloc(&seg_len, (size_t)n_seg));
    GT_TRY(p.d_seg_first.alloc((size_t)n_seg));
    {
        ProfScope ps("k_sw_segments", st);
        hipLaunchKernelGGL(k_sw_seg_fill, dim3(sw_blocks(n)), dim3(256), 0, st, d_cid, M, binc, flag, soff, n, dense, d_sizes, seg, seg_cid,
                           p.d_seg_first.p, seg_last);
        hipLaunchKernelGGL(k_sw_seg_len, dim3(sw_blocks(n_seg)), dim3(256), 0, st, p.d_seg_first.p, seg_last, n_seg, seg_len);
        GT_HIP(hipGetLastError());
    }
    u64 *seg_off, total = 0;
    GT_TRY(scan_total(fr, seg_len, n_seg, &seg_off, &total));
    // 3. events
    u32 *ckey, *perm;
    GT_TRY(fr.alloc(&ckey, (size_t)n));
    GT_TRY(p.A.alloc((size_t)n));
    GT_TRY(p.E.alloc((size_t)n));
    GT_TRY(p.SA.alloc((size_t)n));
    GT_TRY(p.SE.alloc((size_t)n));
    GT_TRY(p.PA.alloc((size_t)n + 1));
    GT_TRY(p.PE.alloc((size_t)n + 1));
    GT_TRY(p.d_seg_off.alloc((size_t)n_seg + 1));
    {
        ProfScope ps("k_sw_events", st);
        hipLaunchKernelGGL(k_sw_events, dim3(sw_blocks(n)), dim3(256), 0, st, seg, M, we, d_sc, p.d_seg_first.p, seg_off, n, p.A.p, p.SA.p,
                           ckey);
        GT_HIP(hipGetLastError());
    }
    GT_TRY(sort_perm(fr, seg, ckey, nullptr, n32, (u32)n_seg, &perm));
    {
        ProfScope ps("k_sw_closes", st);
        hipLaunchKernelGGL(k_sw_closes, dim3(sw_blocks(n)), dim3(256), 0, st, perm, seg, ckey, p.SA.p, p.d_seg_first.p, seg_off, n, p.E.p,
                           p.SE.p);
        GT_HIP(hipGetLastError());
    }
    u64 *pa, *pe, sum = 0;
    GT_TRY(scan_total(fr, p.SA.p, n, &pa, &sum));
    GT_TRY(scan_total(fr, p.SE.p, n, &pe, &sum));
    GT_HIP(hipMemcpyAsync(p.PA.p, pa, (n + 1) * sizeof(u64), hipMemcpyDeviceToDevice, st));
    GT_HIP(hipMemcpyAsync(p.PE.p, pe, (n + 1) * sizeof(u64), hipMemcpyDeviceToDevice, st));
    GT_HIP(hipMemcpyAsync(p.d_seg_off.p, seg_off, (n_seg + 1) * sizeof(u64), hipMemcpyDeviceToDevice, st));
    // the table on the host
    GT_TRY(fr.download(p.seg_cid, seg_cid, (size_t)n_seg));
    GT_TRY(fr.download(p.seg_first, p.d_seg_first.p, (size_t)n_seg));
    GT_TRY(fr.download(p.seg_len, seg_len, (size_t)n_seg));
    GT_TRY(fr.download(p.seg_off, seg_off, (size_t)n_seg + 1));
    return fr.drain();
}

}  // namespace

gtars_status uniwig_stream_plan(const uint32_t *cid, const uint32_t *start, const uint32_t *end, const uint32_t *score, uint64_t n,
                                int on_device, const uint32_t *sizes_by_cid, uint32_t n_chrom, uint32_t smoothsize, int kind,
                                int64_t max_gap, SwPlan **plan) {
    *plan = nullptr;
    if (kind != GTARS_UNIWIG_START && kind != GTARS_UNIWIG_END && kind != GTARS_UNIWIG_CORE)
        return fail(GTARS_ERR_INVALID_ARG, "uniwig stream: unknown track kind " + std::to_string(kind));
    if (n > COV_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "uniwig stream: too many rows (" + std::to_string(n) + ")");
    if (smoothsize > 0x3FFFFFFFu) return fail(GTARS_ERR_INVALID_ARG, "uniwig stream: smooth size out of the i32 range");
    if (n && (!cid || !start || !end || !score)) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    if (n_chrom && !sizes_by_cid) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    for (u32 c = 0; c < n_chrom; ++c)
        if (sizes_by_cid[c] > 0x7FFFFFFEu) return fail(GTARS_ERR_INVALID_ARG, "uniwig stream: chromosome size out of the i32 range");
    GT_TRY(require_device());
    std::unique_ptr<SwPlan> p(new SwPlan());
    GT_HIP(hipGetDevice(&p->device));
    GT_TRY(build_plan(*p, cid, start, end, score, n, on_device, sizes_by_cid, n_chrom, smoothsize, kind, max_gap));
    *plan = p.release();
    return GTARS_OK;
}

void uniwig_stream_plan_free(SwPlan *plan) { delete plan; }
uint64_t uniwig_stream_plan_segments(const SwPlan *plan) { return plan ? plan->seg_cid.size() : 0; }
uint64_t uniwig_stream_plan_total(const SwPlan *plan) { return plan ? plan->seg_off.back() : 0; }

gtars_status uniwig_stream_plan_table(const SwPlan *plan, uint32_t *seg_cid, uint32_t *seg_first, uint32_t *seg_len, uint64_t *seg_off) {
    if (!plan) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    const size_t k = plan->seg_cid.size();
    if (seg_cid) std::copy(plan->seg_cid.begin(), plan->seg_cid.end(), seg_cid);
    if (seg_first) std::copy(plan->seg_first.begin(), plan->seg_first.end(), seg_first);
    if (seg_len) std::copy(plan->seg_len.begin(), plan->seg_len.end(), seg_len);
    if (seg_off) std::copy(plan->seg_off.begin(), plan->seg_off.begin() + k + 1, seg_off);
    return GTARS_OK;
}

gtars_status uniwig_stream_device(const SwPlan *plan, uint64_t window_first, uint64_t window_len, uint32_t *d_counts, void *stream) {
    if (!plan || (window_len && !d_counts)) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    const u64 total = plan->seg_off.back();
    if (window_first > total || window_len > total - window_first)
        return fail(GTARS_ERR_INVALID_ARG, "uniwig stream: window out of the compacted range");
    GT_TRY(require_device());
    GT_TRY(require_handle_device(plan->device));
    return launch_sw(*plan, window_first, window_len, d_counts, (hipStream_t)stream);
}

gtars_status uniwig_stream(const uint32_t *cid, const uint32_t *start, const uint32_t *end, const uint32_t *score, uint64_t n,
                           const uint32_t *sizes_by_cid, uint32_t n_chrom, uint32_t smoothsize, uint32_t step, int kind,
                           int64_t max_gap, uint64_t max_device_bytes, uint32_t **seg_cid, uint32_t **seg_first,
                           uint32_t **seg_len, uint64_t *n_seg, uint32_t **counts, uint64_t *n_counts) {
    *seg_cid = *seg_first = *seg_len = *counts = nullptr, *n_seg = *n_counts = 0;
    if (step > 0x7FFFFFFFu) return fail(GTARS_ERR_INVALID_ARG, "uniwig stream: step size out of the i32 range");
    if (step == 0) step = 1;  // (step_size <= 1 keeps every position, stream.rs:274)
    SwPlan *raw = nullptr;
    GT_TRY(uniwig_stream_plan(cid, start, end, score, n, 0, sizes_by_cid, n_chrom, smoothsize, kind, max_gap, &raw));
    std::unique_ptr<SwPlan> p(raw);
    const u64 k = p->seg_cid.size(), total = p->seg_off.back();
    // kept positions in front of every segment
    std::vector<u64> koff(k + 1, 0);
    for (u64 s = 0; s < k; ++s) koff[s + 1] = koff[s] + sw_kept_in(p->seg_first[s], p->seg_len[s], step);
    const u64 n_kept = koff[k];
    auto kept_before = [&](u64 x) -> u64 {  // x: a compacted index
        if (x >= total) return n_kept;
        const u64 s = (u64)(std::upper_bound(p->seg_off.begin(), p->seg_off.begin() + k + 1, x) - p->seg_off.begin()) - 1;
        return koff[s] + sw_kept_in(p->seg_first[s], x - p->seg_off[s], step);
    };
    MallocArray<u32> h;
    if (!h.alloc(n_kept)) return fail(GTARS_ERR_INTERNAL, "out of host memory");
    if (total) {
        const u64 window = cov_window(max_device_bytes, total);
        StreamFrame fr(nullptr);
        u32 *d, *dk = nullptr;
        u64 *d_koff = nullptr;
        GT_TRY(fr.alloc(&d, (size_t)window));
        if (step > 1) {
            GT_TRY(fr.alloc(&dk, (size_t)window));
            GT_TRY(fr.upload(&d_koff, koff.data(), (size_t)k + 1));
        }
        for (u64 w = 0; w < total; w += window) {
            const u64 wl = std::min(window, total - w);
            GT_TRY(launch_sw(*p, w, wl, d, fr.st));
            if (step == 1) {
                GT_TRY(fr.download(h.p + w, d, wl));
                continue;
            }
            const u64 k0 = kept_before(w), k1 = kept_before(w + wl);
            ProfScope ps("k_sw_decimate", fr.st);
            hipLaunchKernelGGL(k_sw_decimate, dim3(sw_blocks(wl)), dim3(256), 0, fr.st, d, w, wl, p->d_seg_off.p, p->d_seg_first.p, d_koff,
                               (u32)k, step, k0, dk);
            GT_HIP(hipGetLastError());
            GT_TRY(fr.download(h.p + k0, dk, k1 - k0));
        }
        GT_TRY(fr.drain());
    }
    // the table without its empty segments
    u64 live = 0;
    for (u64 s = 0; s < k; ++s) live += p->seg_len[s] != 0;
    MallocArray<u32> oc, of, ol;
    if (!oc.alloc(live) || !of.alloc(live) || !ol.alloc(live)) return fail(GTARS_ERR_INTERNAL, "out of host memory");
    for (u64 s = 0, j = 0; s < k; ++s)
        if (p->seg_len[s]) oc.p[j] = p->seg_cid[s], of.p[j] = p->seg_first[s], ol.p[j] = p->seg_len[s], ++j;
    *seg_cid = oc.release(), *seg_first = of.release(), *seg_len = ol.release(), *n_seg = live;
    *counts = h.release();
    *n_counts = n_kept;
    return GTARS_OK;
}

}  // namespace gtars
