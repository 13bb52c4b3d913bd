// cov_tile.h -- the coverage tile skeleton: the one kernel body and the one launcher behind k_cov_tile (uniwig.hip, K11)
// and k_sw_tile (uniwig_stream.hip, K24), and the window rule of their host calls.
//
// A track is  count(pos) = (weights of the opens <= pos) - (weights of the closes <= pos)  over two ascending event
// columns.  A workgroup owns a SPAN of consecutive positions, finds the first open and the first close at or behind its
// first position by binary search (they give the count that enters the span), then walks the span in tiles of COV_TILE
// positions: the tile's events are streamed from the two columns in chunks of one per thread and added into an LDS
// difference tile (runs of equal positions inside a wave collapse into one LDS atomic, so a pile-up costs one atomic per
// wave, not one per event), the tile is scanned in LDS and leaves as 16-byte stores.  Global traffic: 4 bytes per
// position out, the events in; there is no difference array in global memory.
//
// What a track's events are comes from an event source `Src` (CovSrc in uniwig.hip, SwSrc in uniwig_stream.hip):
//     u32 n                                   events per column
//     static constexpr bool WEIGHTED          false: every event weighs 1
//     u32 first_open(u64 pos) / first_close   the first index whose position is >= pos
//     u32 entering(u32 ia, u32 ie)            the count in front of opens[ia] and closes[ie] (mod 2^32)
//     void open(u64 i, u64 t0, u64 t1, u32 &key, u32 &w) / close
//                                             event i < n: if its position lies in [t0, t1), key = position - t0 and
//                                             (WEIGHTED) w = its weight; otherwise both are left as they are
#pragma once
#include <algorithm>
#include <string>

#include "common.h"
#include "scan.h"

namespace gtars {

constexpr int COV_TPB = 256;
constexpr u32 COV_PER = 16;                   // consecutive positions per thread in the scan
constexpr u32 COV_TILE = COV_TPB * COV_PER;   // 4096 positions: 16 KiB of counts
// a thread's 16 words are followed by 4 words of padding: the 16 lanes of a ds_read_b128 group then read 16 different
// 16-byte slots of the 256-byte bank row (stride 80 bytes: slot 5 * lane mod 16)
constexpr u32 COV_LDS_WORDS = COV_TILE + COV_TILE / COV_PER * 4;
constexpr u32 COV_WG_PER_CU = 8;              // 20 KiB of LDS per workgroup
constexpr u32 COV_NONE = 0xFFFFFFFFu;         // the key of a lane without an event
constexpr u64 COV_MAX_N = 0xFFFFF000u;        // events per column
constexpr u64 COV_DEFAULT_WINDOW = 1ull << 28;  // positions a host call keeps on the device at a time (1 GiB)

__device__ __forceinline__ u32 cov_phys(u32 i) { return i + ((i >> 4) << 2); }

// adds the wave's events into the difference tile (negated for closes); key = the event's offset in the tile, COV_NONE
// for a lane without one.  The keys of a wave ascend, so equal keys are neighbours and the last lane of a run adds the
// whole run: its length, or (WEIGHTED) the sum of its weights -- the wave's inclusive sum at that lane minus the exclusive
// one at the run's first lane, from one DPP scan and one shuffle; a run that sums to 0 adds nothing.  Every lane of the
// wave calls this.
template <bool WEIGHTED>
__device__ __forceinline__ void cov_add_runs(u32 *__restrict__ d, u32 key, u32 w, bool negate, int lane) {
    const u32 prev = __shfl_up(key, 1, 64), next = __shfl_down(key, 1, 64);
    const bool head = lane == 0 || prev != key;
    const bool tail = lane == 63 || next != key;
    const int head_lane = wave_inclusive_max_nonneg(head ? lane : 0);
    u32 sum = (u32)(lane - head_lane + 1);
    if (WEIGHTED) {
        const u32 inc = wave_inclusive_scan_u32(w, lane);
        sum = inc - __shfl(inc - w, head_lane, 64);
    }
    if (tail && key != COV_NONE && (!WEIGHTED || sum)) atomicAdd(&d[cov_phys(key)], negate ? 0u - sum : sum);
}

// positions w0 + [0, len) of the track of `src` into out[0, len); out is 16-byte aligned, span a multiple of COV_TILE
template <class Src>
__device__ __forceinline__ void cov_tile_body(const Src &src, u64 w0, u64 len, u64 span, u32 *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) u32 d[COV_LDS_WORDS];
    __shared__ u32 red[COV_TPB / 64];
    __shared__ u32 cur[2];
    const u32 tid = threadIdx.x;
    const int lane = tid & 63;
    const u64 c0 = (u64)blockIdx.x * span;
    if (c0 >= len) return;
    const u64 c1 = min(len, c0 + span);
    if (tid == 0) cur[0] = src.first_open(w0 + c0);
    if (tid == 64) cur[1] = src.first_close(w0 + c0);
    for (u32 i = tid; i < COV_LDS_WORDS; i += COV_TPB) d[i] = 0;
    __syncthreads();
    u32 ia = cur[0], ie = cur[1];
    u32 carry = src.entering(ia, ie);  // the count in front of the span (mod 2^32, as every sum below: the counts themselves fit)
    for (u64 c = c0; c < c1; c += COV_TILE) {
        const u64 t0 = w0 + c;
        const u64 t1 = t0 + min((u64)COV_TILE, c1 - c);
        // the tile's events, a chunk of COV_TPB opens and COV_TPB closes per round; the columns ascend, so the events
        // inside the tile are a prefix of every chunk and a chunk that is not all inside ends the stream
        bool more_a = true, more_e = true;
        while (more_a || more_e) {
            u32 key_a = COV_NONE, key_e = COV_NONE, w_a = 0, w_e = 0;
            if (more_a && (u64)ia + tid < src.n) src.open((u64)ia + tid, t0, t1, key_a, w_a);
            if (more_e && (u64)ie + tid < src.n) src.close((u64)ie + tid, t0, t1, key_e, w_e);
            cov_add_runs<Src::WEIGHTED>(d, key_a, w_a, false, lane);
            cov_add_runs<Src::WEIGHTED>(d, key_e, w_e, true, lane);
            const u32 na = (u32)__syncthreads_count(key_a != COV_NONE);
            const u32 ne = (u32)__syncthreads_count(key_e != COV_NONE);
            ia += na;
            ie += ne;
            more_a = na == COV_TPB;
            more_e = ne == COV_TPB;
        }
        // scan: 16 consecutive differences per thread, the workgroup's exclusive scan of the thread sums, the running
        // counts back into LDS
        u32 v[COV_PER];
        uint4 *mine = (uint4 *)&d[tid * (COV_PER + 4)];
#pragma unroll
        for (u32 k = 0; k < COV_PER / 4; ++k) {
            const uint4 x = mine[k];
            v[4 * k] = x.x, v[4 * k + 1] = x.y, v[4 * k + 2] = x.z, v[4 * k + 3] = x.w;
        }
#pragma unroll
        for (u32 k = 1; k < COV_PER; ++k) v[k] += v[k - 1];
        u32 total;
        const u32 base = carry + block_exclusive_scan<COV_TPB>(v[COV_PER - 1], red, total);
        carry += total;
#pragma unroll
        for (u32 k = 0; k < COV_PER / 4; ++k)
            mine[k] = make_uint4(v[4 * k] + base, v[4 * k + 1] + base, v[4 * k + 2] + base, v[4 * k + 3] + base);
        __syncthreads();
        // out: consecutive lanes store consecutive 16-byte vectors; the tile is left zeroed for the next round
#pragma unroll
        for (u32 j = 0; j < COV_PER / 4; ++j) {
            const u32 q = j * COV_TPB + tid;
            uint4 *src4 = (uint4 *)&d[4 * (q + (q >> 2))];
            const uint4 x = *src4;
            *src4 = make_uint4(0, 0, 0, 0);
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

// ---- host side ---------------------------------------------------------------------------------------------------------
inline u32 cov_max_workgroups() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus <= 0)
        cus = 256;
    return (u32)cus * COV_WG_PER_CU;
}

// one launch of a tile kernel `kernel(lead..., w_first, w_len, span, d_out)` under the profiling scope `name`: as many
// workgroups as tiles, at most COV_WG_PER_CU per CU (GTARS_GRID_CAP, a test switch, lowers that: common.h), each with a
// span of whole tiles.  who: the prefix of the error message.
template <class Kernel, class... Lead>
gtars_status cov_tile_launch(const char *name, const char *who, Kernel kernel, hipStream_t st, u64 w_first, u64 w_len, u32 *d_out,
                             Lead... lead) {
    if (!w_len) return GTARS_OK;
    if ((uintptr_t)d_out & 15) return fail(GTARS_ERR_INVALID_ARG, std::string(who) + ": the device counts must be 16-byte aligned");
    const u64 tiles = (w_len + COV_TILE - 1) / COV_TILE;
    u64 want = std::min<u64>(tiles, cov_max_workgroups());
    if (const u32 low = grid_cap_switch(); low && low < want) {
        note_grid_clip();
        want = low;
    }
    const u64 span = (tiles + want - 1) / want * COV_TILE;
    const u64 grid = (w_len + span - 1) / span;
    ProfScope ps(name, st);
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(COV_TPB), 0, st, lead..., w_first, w_len, span, d_out);
    GT_HIP(hipGetLastError());
    return GTARS_OK;
}

// positions a host call keeps on the device at a time: max_device_bytes of counts in whole tiles (at least one; 0: the
// default), no more than the track's `total`
inline u64 cov_window(u64 max_device_bytes, u64 total) {
    const u64 window = max_device_bytes ? std::max<u64>(max_device_bytes / sizeof(u32) / COV_TILE, 1) * COV_TILE : COV_DEFAULT_WINDOW;
    return std::min(window, total);
}

}  // namespace gtars
