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
//   4. k_sw_tile, the weighted form of K11's k_cov_tile over the compacted index space: a workgroup owns a span, finds
//      the first open and the first close at or behind it by binary search, enters with prefix_open[ia] - prefix_close[ie],
//      streams the events into the LDS difference tile (a run of equal keys inside a wave adds the SUM of its weights with
//      one LDS atomic: a segmented sum over the wave from one DPP scan and one shuffle), scans and stores as K11 does.
//      A close one past its segment's end lands on the next segment's first slot, where the count has to drop anyway.
//   5. step > 1: the window is computed at step 1 and k_sw_decimate keeps the positions with (pos - 1) % step == 0.
#include <algorithm>
#include <cstdlib>
#include <memory>
#include <vector>

#include "common.h"
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

constexpr int SW_TPB = 256;
constexpr u32 SW_PER = 16;                  // consecutive positions per thread in the scan
constexpr u32 SW_TILE = SW_TPB * SW_PER;    // 4096 positions: 16 KiB of counts
constexpr u32 SW_LDS_WORDS = SW_TILE + SW_TILE / SW_PER * 4;  // the padded 80-byte stride of K11
constexpr u32 SW_WG_PER_CU = 8;
constexpr u64 SW_MAX_N = 0xFFFFF000u;
constexpr u64 SW_DEFAULT_WINDOW = 1ull << 28;
constexpr u32 SW_NONE = 0xFFFFFFFFu;
constexpr int PL_TPB = 256;
constexpr int PL_IPT = 8;
constexpr u32 PL_TILE = PL_TPB * PL_IPT;

using SMax = SegMax<u32>;

__device__ __forceinline__ u32 sw_phys(u32 i) { return i + ((i >> 4) << 2); }
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
// the first index whose value is >= pos
__device__ __forceinline__ u32 sw_lower_bound(const u64 *__restrict__ x, u32 n, u64 pos) {
    u32 lo = 0, hi = n;
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        if (x[mid] >= pos) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// adds the weights of the wave's events into the difference tile (negated for closes); key = the event's offset in the
// tile, SW_NONE for a lane without one.  The keys of a wave ascend, so equal keys are neighbours: the last lane of a run adds
// the run's sum, the wave's inclusive sum at that lane minus the exclusive one at the run's first lane.  Every lane of the
// wave calls this.
__device__ __forceinline__ void sw_add_runs(u32 *__restrict__ d, u32 key, u32 w, bool negate, int lane) {
    const u32 prev = __shfl_up(key, 1, 64), next = __shfl_down(key, 1, 64);
    const bool head = lane == 0 || prev != key;
    const bool tail = lane == 63 || next != key;
    const int head_lane = wave_inclusive_max_nonneg(head ? lane : 0);
    const u32 inc = wave_inclusive_scan_u32(w, lane);
    const u32 before = __shfl(inc - w, head_lane, 64);
    const u32 sum = inc - before;
    if (tail && key != SW_NONE && sum) atomicAdd(&d[sw_phys(key)], negate ? 0u - sum : sum);
}

// compacted positions w0 + [0, len) into out[0, len); out is 16-byte aligned, span a multiple of SW_TILE
__global__ void __launch_bounds__(SW_TPB)
k_sw_tile(const u64 *__restrict__ A, const u64 *__restrict__ E, const u32 *__restrict__ SA, const u32 *__restrict__ SE,
          const u64 *__restrict__ PA, const u64 *__restrict__ PE, u32 n, u64 w0, u64 len, u64 span, u32 *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) u32 d[SW_LDS_WORDS];
    __shared__ u32 red[SW_TPB / 64];
    __shared__ u32 cur[2];
    const u32 tid = threadIdx.x;
    const int lane = tid & 63;
    const u64 c0 = (u64)blockIdx.x * span;
    if (c0 >= len) return;
    const u64 c1 = min(len, c0 + span);
    if (tid == 0) cur[0] = sw_lower_bound(A, n, w0 + c0);
    if (tid == 64) cur[1] = sw_lower_bound(E, n, w0 + c0);
    for (u32 i = tid; i < SW_LDS_WORDS; i += SW_TPB) d[i] = 0;
    __syncthreads();
    u32 ia = cur[0], ie = cur[1];
    u32 carry = (u32)PA[ia] - (u32)PE[ie];  // the count in front of the span, modulo 2^32 as every sum below
    for (u64 c = c0; c < c1; c += SW_TILE) {
        const u64 t0 = w0 + c;
        const u64 t1 = t0 + min((u64)SW_TILE, c1 - c);
        // a chunk of SW_TPB opens and SW_TPB closes per round; the columns ascend, so the events inside the tile are a
        // prefix of every chunk and a chunk that is not all inside ends the stream
        bool more_a = true, more_e = true;
        while (more_a || more_e) {
            u32 key_a = SW_NONE, key_e = SW_NONE, w_a = 0, w_e = 0;
            if (more_a) {
                const u64 i = (u64)ia + tid;
                if (i < n) {
                    const u64 v = A[i];
                    if (v >= t0 && v < t1) key_a = (u32)(v - t0), w_a = SA[i];
                }
            }
            if (more_e) {
                const u64 i = (u64)ie + tid;
                if (i < n) {
                    const u64 v = E[i];
                    if (v >= t0 && v < t1) key_e = (u32)(v - t0), w_e = SE[i];
                }
            }
            sw_add_runs(d, key_a, w_a, false, lane);
            sw_add_runs(d, key_e, w_e, true, lane);
            const u32 na = (u32)__syncthreads_count(key_a != SW_NONE);
            const u32 ne = (u32)__syncthreads_count(key_e != SW_NONE);
            ia += na;
            ie += ne;
            more_a = na == SW_TPB;
            more_e = ne == SW_TPB;
        }
        u32 v[SW_PER];
        uint4 *mine = (uint4 *)&d[tid * (SW_PER + 4)];
#pragma unroll
        for (u32 k = 0; k < SW_PER / 4; ++k) {
            const uint4 x = mine[k];
            v[4 * k] = x.x, v[4 * k + 1] = x.y, v[4 * k + 2] = x.z, v[4 * k + 3] = x.w;
        }
#pragma unroll
        for (u32 k = 1; k < SW_PER; ++k) v[k] += v[k - 1];
        u32 total;
        const u32 base = carry + block_exclusive_scan<SW_TPB>(v[SW_PER - 1], red, total);
        carry += total;
#pragma unroll
        for (u32 k = 0; k < SW_PER / 4; ++k)
            mine[k] = make_uint4(v[4 * k] + base, v[4 * k + 1] + base, v[4 * k + 2] + base, v[4 * k + 3] + base);
        __syncthreads();
        // out: consecutive lanes store consecutive 16-byte vectors; the tile is left zeroed for the next round
#pragma unroll
        for (u32 j = 0; j < SW_PER / 4; ++j) {
            const u32 q = j * SW_TPB + tid;
            uint4 *src = (uint4 *)&d[4 * (q + (q >> 2))];
            const uint4 x = *src;
            *src = make_uint4(0, 0, 0, 0);
            const u64 g = c + 4ull * q;
            if (g + 4 <= c1) {
                *(uint4 *)(out + g) = x;
            } else {
                if (g < c1) out[g] = x.x;
                if (g + 1 < c1) out[g + 1] = x.y;
                if (g + 2 < c1) out[g + 2] = x.z;
            }
        }
        __syncthreads();
    }
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

u32 sw_max_workgroups() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus <= 0)
        cus = 256;
    return (u32)cus * SW_WG_PER_CU;
}

gtars_status launch_sw(const SwPlan &p, u64 w_first, u64 w_len, u32 *d_out, hipStream_t st) {
    if (!w_len) return GTARS_OK;
    if ((uintptr_t)d_out & 15) return fail(GTARS_ERR_INVALID_ARG, "uniwig stream: the device counts must be 16-byte aligned");
    const u64 tiles = (w_len + SW_TILE - 1) / SW_TILE;
    const u64 want = std::min<u64>(tiles, sw_max_workgroups());
    const u64 span = (tiles + want - 1) / want * SW_TILE;
    const u64 grid = (w_len + span - 1) / span;
    ProfScope ps("k_sw_tile", st);
    hipLaunchKernelGGL(k_sw_tile, dim3((unsigned)grid), dim3(SW_TPB), 0, st, p.A.p, p.E.p, p.SA.p, p.SE.p, p.PA.p, p.PE.p, (u32)p.n, w_first,
                       w_len, span, d_out);
    GT_HIP(hipGetLastError());
    return GTARS_OK;
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
    u32 h_bad = SW_NONE;
    GT_TRY(fr.download(&h_bad, bad, 1));
    u64 n = n0;
    if (kind == GTARS_UNIWIG_CORE) {
        u64 *koff;
        GT_TRY(scan_total(fr, keep, n0, &koff, &n));
        if (h_bad == SW_NONE && n != n0 && n) {
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
    if (h_bad != SW_NONE)
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
    if (n > SW_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "uniwig stream: too many rows (" + std::to_string(n) + ")");
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
        u64 window = max_device_bytes ? std::max<u64>(max_device_bytes / sizeof(u32) / SW_TILE, 1) * SW_TILE : SW_DEFAULT_WINDOW;
        window = std::min(window, total);
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
