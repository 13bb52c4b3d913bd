// uniwig.hip -- K11: per-base coverage tracks on the device (gtars-uniwig: start_end_counts / core_counts,
// counting.rs:32-290; compress_counts, utils.rs:40-81; write_to_wig_file_variable, writing.rs:149-179).
//
// With unit scores, step 1 and (core track) no row whose end lies before its start + 1, the reference's sweeps reduce to
//     count(pos) = #{i : a_i <= pos} - #{i : e_i <= pos}      pos = a_0 .. max(chrom_size, a_{n-1} - 1)
// over the sorted window opens a_i and closes e_i (tests/uniwig_ref.py restates the sweeps line by line and
// tests/test_uniwig_cpu.py holds the two against each other):
//     start / end track:  a_i = max(1, p_i - m),  e_i = p_i + m + 1     p = sorted positions, m = smoothsize
//     core track:         a_i = max(1, s_i),      e_i = t_i             s = sorted start + 1, t = sorted ends
//
//   * k_cov_tile, one pass, the output written once: a workgroup owns a SPAN of consecutive positions, finds the first
//     open and the first close at or behind its first position by binary search (their difference is the count that
//     enters the span), then walks the span in tiles of COV_TILE positions: the tile's events are streamed from the two
//     sorted columns in chunks of one per thread and added into an LDS difference tile (runs of equal positions inside
//     a wave collapse into one LDS atomic, so a pile-up costs one atomic per wave, not one per event), the tile is
//     scanned in LDS and leaves as 16-byte stores.  The transform p -> (max(1, p - m), p + m + 1) is applied on load, so
//     the start and the end track read the position column as it is.  Global traffic: 4 bytes per position out, 8 bytes
//     per event in; there is no difference array in global memory.
//   * k_cov_flag_count / k_cov_compact: the run-length form (bedGraph) and the non-zero form (variableStep wig) of a
//     track that sits in device memory: flags per position, block counts, the exclusive scan of kernels.hip, scatter.
//     Only the runs / pairs cross to the host.
//   * the columns are sorted with the radix sort of sort.hip.
#include <algorithm>
#include <cstdlib>
#include <memory>

#include "common.h"
#include "pipeline.h"
#include "scan.h"
#include "uniwig.h"

namespace gtars {

namespace {

constexpr int COV_TPB = 256;
constexpr u32 COV_PER = 16;                   // consecutive positions per thread in the scan
constexpr u32 COV_TILE = COV_TPB * COV_PER;   // 4096 positions: 16 KiB of counts
// a thread's 16 words are followed by 4 words of padding: the 16 lanes of a ds_read_b128 group then read 16 different
// 16-byte slots of the 256-byte bank row (stride 80 bytes: slot 5 * lane mod 16)
constexpr u32 COV_LDS_WORDS = COV_TILE + COV_TILE / COV_PER * 4;
constexpr u32 COV_WG_PER_CU = 8;              // 20 KiB of LDS per workgroup
constexpr u64 COV_MAX_N = 0xFFFFF000u;
constexpr u64 COV_DEFAULT_WINDOW = 1ull << 28;  // positions the host call keeps on the device at a time (1 GiB)

__device__ __forceinline__ u32 cov_phys(u32 i) { return i + ((i >> 4) << 2); }

__device__ __forceinline__ i64 cov_open(const u32 *__restrict__ a, u64 i, u32 sub) {
    const i64 v = (i64)a[i] - (i64)sub;
    return v < 1 ? 1 : v;
}
__device__ __forceinline__ i64 cov_close(const u32 *__restrict__ e, u64 i, u32 add) { return (i64)e[i] + (i64)add; }

// number of events in front of position pos: the first index whose (transformed) value is >= pos
template <bool OPEN>
__device__ __forceinline__ u32 cov_lower_bound(const u32 *__restrict__ x, u32 n, u32 m, i64 pos) {
    u32 lo = 0, hi = n;
    while (lo < hi) {
        const u32 mid = lo + ((hi - lo) >> 1);
        const i64 v = OPEN ? cov_open(x, mid, m) : cov_close(x, mid, m);
        if (v >= pos) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// adds `sign` per event into the difference tile; key = the event's offset in the tile, 0xFFFFFFFF for a lane without
// one.  The keys of a wave ascend, so equal keys are neighbours: the last lane of a run adds the run's length.  Every
// lane of the wave calls this.
__device__ __forceinline__ void cov_add_runs(u32 *__restrict__ d, u32 key, u32 sign, int lane) {
    const u32 prev = __shfl_up(key, 1, 64), next = __shfl_down(key, 1, 64);
    const bool head = lane == 0 || prev != key;
    const bool tail = lane == 63 || next != key;
    const int head_lane = wave_inclusive_max_nonneg(head ? lane : 0);
    if (tail && key != 0xFFFFFFFFu) atomicAdd(&d[cov_phys(key)], sign * (u32)(lane - head_lane + 1));
}

// positions w0 + [0, len) of the track into out[0, len); out is 16-byte aligned, span a multiple of COV_TILE
__global__ void __launch_bounds__(COV_TPB)
k_cov_tile(const u32 *__restrict__ A, const u32 *__restrict__ E, u32 n, u32 sub_open, u32 add_close, u64 w0, u64 len, u64 span,
           u32 *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) u32 d[COV_LDS_WORDS];
    __shared__ u32 red[COV_TPB / 64];
    __shared__ u32 cur[2];
    const u32 tid = threadIdx.x;
    const int lane = tid & 63;
    const u64 c0 = (u64)blockIdx.x * span;
    if (c0 >= len) return;
    const u64 c1 = min(len, c0 + span);
    if (tid == 0) cur[0] = cov_lower_bound<true>(A, n, sub_open, (i64)(w0 + c0));
    if (tid == 64) cur[1] = cov_lower_bound<false>(E, n, add_close, (i64)(w0 + c0));
    for (u32 i = tid; i < COV_LDS_WORDS; i += COV_TPB) d[i] = 0;
    __syncthreads();
    u32 ia = cur[0], ie = cur[1];
    u32 carry = ia - ie;  // the count in front of the span (mod 2^32, as every sum below: the counts themselves fit)
    for (u64 c = c0; c < c1; c += COV_TILE) {
        const i64 t0 = (i64)(w0 + c);
        const i64 t1 = t0 + (i64)min((u64)COV_TILE, c1 - c);
        // the tile's events, a chunk of COV_TPB opens and COV_TPB closes per round; the columns ascend, so the events
        // inside the tile are a prefix of every chunk and a chunk that is not all inside ends the stream
        bool more_a = true, more_e = true;
        while (more_a || more_e) {
            u32 key_a = 0xFFFFFFFFu, key_e = 0xFFFFFFFFu;
            if (more_a) {
                const u64 i = (u64)ia + tid;
                if (i < n) {
                    const i64 v = cov_open(A, i, sub_open);
                    if (v >= t0 && v < t1) key_a = (u32)(v - t0);  // (v >= t0 holds for ascending columns: a caller's unsorted one must not leave the tile)
                }
            }
            if (more_e) {
                const u64 i = (u64)ie + tid;
                if (i < n) {
                    const i64 v = cov_close(E, i, add_close);
                    if (v >= t0 && v < t1) key_e = (u32)(v - t0);
                }
            }
            cov_add_runs(d, key_a, 1u, lane);
            cov_add_runs(d, key_e, 0xFFFFFFFFu, lane);
            const u32 na = (u32)__syncthreads_count(key_a != 0xFFFFFFFFu);
            const u32 ne = (u32)__syncthreads_count(key_e != 0xFFFFFFFFu);
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

// ---- run-length and non-zero forms of a track in device memory -------------------------------------------------------
constexpr int CMP_TPB = 256;
constexpr u32 CMP_PER = 16;
constexpr u32 CMP_TILE = CMP_TPB * CMP_PER;
enum { CMP_RUNS = 0, CMP_NONZERO = 1 };

// the thread's 16 entries from k0 on (0 past the end) and its flags as a bit mask.  RUNS: entry k differs from entry
// k - 1 (k >= 1); NONZERO: entry k is not 0.
template <int MODE>
__device__ __forceinline__ u32 cmp_flags(const u32 *__restrict__ c, u64 len, u64 k0, u32 (&v)[CMP_PER]) {
    if (k0 + CMP_PER <= len) {
        const uint4 *p = (const uint4 *)(c + k0);
#pragma unroll
        for (u32 k = 0; k < CMP_PER / 4; ++k) {
            const uint4 x = p[k];
            v[4 * k] = x.x, v[4 * k + 1] = x.y, v[4 * k + 2] = x.z, v[4 * k + 3] = x.w;
        }
    } else {
#pragma unroll
        for (u32 k = 0; k < CMP_PER; ++k) v[k] = k0 + k < len ? c[k0 + k] : 0u;
    }
    u32 f = 0;
    if (MODE == CMP_RUNS) {
        u32 prev = (k0 >= 1 && k0 < len) ? c[k0 - 1] : v[0];
#pragma unroll
        for (u32 k = 0; k < CMP_PER; ++k) {
            if (k0 + k < len && v[k] != prev) f |= 1u << k;
            prev = v[k];
        }
    } else {
#pragma unroll
        for (u32 k = 0; k < CMP_PER; ++k)
            if (k0 + k < len && v[k] != 0) f |= 1u << k;
    }
    return f;
}

template <int MODE>
__global__ void __launch_bounds__(CMP_TPB) k_cov_flag_count(const u32 *__restrict__ c, u64 len, u32 *__restrict__ block_count) {
    __shared__ u32 red[CMP_TPB / 64];
    u32 v[CMP_PER];
    const u64 k0 = (u64)blockIdx.x * CMP_TILE + (u64)threadIdx.x * CMP_PER;
    const u32 f = cmp_flags<MODE>(c, len, k0, v);
    u32 total;
    (void)block_exclusive_scan<CMP_TPB>((u32)__popc(f), red, total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

// RUNS (k_cov_runs): a change at entry k closes run j - 1 at S + k + 1 and opens run j there with count c[k] (compress_counts
// advances its end before it compares, so the entry that changes still belongs to the run it ends); run 0 starts at S with
// c[0], the last run ends at S + len.  o0 / o1 / o2 = run starts / ends / counts, block_off[n_blocks] + 1 runs.
// NONZERO (k_cov_nonzero): o0 / o1 = S + k / c[k] of the entries that are not 0.
template <int MODE>
__global__ void __launch_bounds__(CMP_TPB)
k_cov_compact(const u32 *__restrict__ c, u64 len, const u64 *__restrict__ block_off, u32 n_blocks, u32 S, u32 *__restrict__ o0,
              u32 *__restrict__ o1, u32 *__restrict__ o2) {
    __shared__ u32 red[CMP_TPB / 64];
    u32 v[CMP_PER];
    const u64 k0 = (u64)blockIdx.x * CMP_TILE + (u64)threadIdx.x * CMP_PER;
    const u32 f = cmp_flags<MODE>(c, len, k0, v);
    u32 total;
    u64 j = block_off[blockIdx.x] + block_exclusive_scan<CMP_TPB>((u32)__popc(f), red, total);
    if (MODE == CMP_RUNS && blockIdx.x == 0 && threadIdx.x == 0) {
        o0[0] = S;
        o2[0] = v[0];
        o1[block_off[n_blocks]] = (u32)(S + len);
    }
#pragma unroll
    for (u32 k = 0; k < CMP_PER; ++k) {
        if (!(f >> k & 1u)) continue;
        if (MODE == CMP_RUNS) {
            const u32 at = (u32)(S + k0 + k + 1);
            o1[j] = at;
            o0[j + 1] = at;
            o2[j + 1] = v[k];
        } else {
            o0[j] = (u32)(S + k0 + k);
            o1[j] = v[k];
        }
        ++j;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------
struct CovTrack {
    DevBuf<u32> a, e;
    const u32 *open = nullptr, *close = nullptr;  // ascending device columns
    u32 n = 0, sub_open = 0, add_close = 0;
    u64 first = 0, len = 0;
};

void cov_transform(int kind, u32 smoothsize, u32 *sub_open, u32 *add_close) {
    *sub_open = kind == GTARS_UNIWIG_CORE ? 0u : smoothsize;
    *add_close = kind == GTARS_UNIWIG_CORE ? 0u : smoothsize + 1u;
}

u32 cov_max_workgroups() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        cus <= 0)
        cus = 256;
    return (u32)cus * COV_WG_PER_CU;
}

gtars_status launch_cov(const u32 *open, const u32 *close, u32 n, u32 sub_open, u32 add_close, u64 w_first, u64 w_len, u32 *d_out,
                        hipStream_t st) {
    if (!w_len) return GTARS_OK;
    if ((uintptr_t)d_out & 15) return fail(GTARS_ERR_INVALID_ARG, "uniwig: the device counts must be 16-byte aligned");
    const u64 tiles = (w_len + COV_TILE - 1) / COV_TILE;
    const u64 want = std::min<u64>(tiles, cov_max_workgroups());
    const u64 span = (tiles + want - 1) / want * COV_TILE;
    const u64 grid = (w_len + span - 1) / span;
    ProfScope ps("k_cov_tile", st);
    hipLaunchKernelGGL(k_cov_tile, dim3((unsigned)grid), dim3(COV_TPB), 0, st, open, close, n, sub_open, add_close, w_first, w_len, span,
                       d_out);
    GT_HIP(hipGetLastError());
    return GTARS_OK;
}

// one column, ascending, on the device
gtars_status sorted_column(StreamFrame &fr, const u32 *h, u32 n, DevBuf<u32> &out) {
    u32 *raw, *perm;
    GT_TRY(out.alloc(n));
    GT_TRY(fr.upload(&raw, h, (size_t)n));
    GT_TRY(sort_perm(fr, raw, raw, nullptr, n, 1, &perm));
    return device_gather_u32(raw, perm, n, out.p, fr.st);
}

gtars_status cov_prepare(const u32 *opens, const u32 *closes, u64 n, u32 chrom_size, u32 smoothsize, int kind, CovTrack &t) {
    GT_TRY(uniwig_extent(opens, closes, n, chrom_size, smoothsize, kind, &t.first, &t.len));
    GT_TRY(require_device());
    t.n = (u32)n;
    cov_transform(kind, smoothsize, &t.sub_open, &t.add_close);
    if (!n) return GTARS_OK;
    StreamFrame fr(nullptr);
    GT_TRY(sorted_column(fr, opens, t.n, t.a));
    t.open = t.close = t.a.p;
    if (kind == GTARS_UNIWIG_CORE) {
        GT_TRY(sorted_column(fr, closes, t.n, t.e));
        t.close = t.e.p;
    }
    return fr.drain();
}

// the flag / scan / scatter chain over the first `len` entries of the track in d_counts; the outputs reach the host
template <int MODE>
gtars_status cov_compact(const u32 *d_counts, u64 len, u32 S, u32 **o0, u32 **o1, u32 **o2, u64 *n_out) {
    *n_out = 0;
    if (!len) {  // (the non-zero form of an empty track)
        MallocArray<u32> e0, e1;
        if (!e0.alloc(0) || !e1.alloc(0)) return fail(GTARS_ERR_INTERNAL, "out of host memory");
        *o0 = e0.release();
        *o1 = e1.release();
        return GTARS_OK;
    }
    StreamFrame fr(nullptr);
    hipStream_t st = fr.st;
    const u64 nb = (len + CMP_TILE - 1) / CMP_TILE;
    if (nb > 0x7FFFFFFFull) return fail(GTARS_ERR_INVALID_ARG, "uniwig: track too long");
    u32 *bc;
    GT_TRY(fr.alloc(&bc, (size_t)nb));
    {
        ProfScope ps("k_cov_flag_count", st);
        hipLaunchKernelGGL(k_cov_flag_count<MODE>, dim3((unsigned)nb), dim3(CMP_TPB), 0, st, d_counts, len, bc);
        GT_HIP(hipGetLastError());
    }
    u64 *off, flagged = 0;
    GT_TRY(scan_total(fr, bc, nb, &off, &flagged));
    const u64 n = MODE == CMP_RUNS ? flagged + 1 : flagged;
    const int cols = MODE == CMP_RUNS ? 3 : 2;
    u32 *d_o[3] = {nullptr, nullptr, nullptr};
    for (int k = 0; k < cols; ++k) GT_TRY(fr.alloc(&d_o[k], (size_t)n));
    {
        ProfScope ps(MODE == CMP_RUNS ? "k_cov_runs" : "k_cov_nonzero", st);
        hipLaunchKernelGGL(k_cov_compact<MODE>, dim3((unsigned)nb), dim3(CMP_TPB), 0, st, d_counts, len, off, (u32)nb, S, d_o[0], d_o[1],
                           d_o[2]);
        GT_HIP(hipGetLastError());
    }
    MallocArray<u32> h[3];
    for (int k = 0; k < cols; ++k) {
        if (!h[k].alloc(n)) return fail(GTARS_ERR_INTERNAL, "out of host memory");
        GT_TRY(fr.download(h[k].p, d_o[k], n));
    }
    GT_TRY(fr.drain());
    *o0 = h[0].release();
    *o1 = h[1].release();
    if (o2) *o2 = h[2].release();
    *n_out = n;
    return GTARS_OK;
}

// the whole track in device memory
gtars_status cov_dense(const CovTrack &t, DevBuf<u32> &d) {
    GT_TRY(d.alloc((size_t)t.len));
    hipStream_t st = nullptr;
    GT_TRY(launch_cov(t.open, t.close, t.n, t.sub_open, t.add_close, t.first, t.len, d.p, st));
    GT_HIP(hipStreamSynchronize(st));
    return GTARS_OK;
}

}  // namespace

gtars_status uniwig_extent(const uint32_t *opens, const uint32_t *closes, uint64_t n, uint32_t chrom_size, uint32_t smoothsize,
                           int kind, uint64_t *first, uint64_t *len) {
    *first = 0, *len = 0;
    if (kind != GTARS_UNIWIG_START && kind != GTARS_UNIWIG_END && kind != GTARS_UNIWIG_CORE)
        return fail(GTARS_ERR_INVALID_ARG, "uniwig: unknown track kind " + std::to_string(kind));
    if (n > COV_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "uniwig: too many rows on one chromosome (" + std::to_string(n) + ")");
    if (n && (!opens || (kind == GTARS_UNIWIG_CORE && !closes))) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    // the reference counts in i32 (counting.rs:32-37): positions, sizes and window ends must fit
    if (chrom_size > 0x7FFFFFFFu || smoothsize > 0x3FFFFFFFu)
        return fail(GTARS_ERR_INVALID_ARG, "uniwig: chromosome size or smooth size out of the i32 range");
    if (!n) return GTARS_OK;
    const u64 limit = 0x7FFFFFFFull - smoothsize - 1;
    u32 mn = 0xFFFFFFFFu, mx = 0;
    for (u64 i = 0; i < n; ++i) {
        mn = std::min(mn, opens[i]);
        mx = std::max(mx, opens[i]);
        if (opens[i] > limit || (kind == GTARS_UNIWIG_CORE && closes[i] > limit))
            return fail(GTARS_ERR_INVALID_ARG, "uniwig: position out of the i32 range at row " + std::to_string(i));
        // core_counts pairs the k-th open with the k-th close; a close in front of its open (a row with end <= start) leaves
        // the sweep's queue in a state that is no coverage track
        if (kind == GTARS_UNIWIG_CORE && closes[i] < opens[i])
            return fail(GTARS_ERR_INVALID_ARG, "uniwig: core track of a zero-length or inverted row (row " + std::to_string(i) + ")");
    }
    u32 sub, add;
    cov_transform(kind, smoothsize, &sub, &add);
    const i64 a0 = std::max<i64>(1, (i64)mn - sub), a_last = std::max<i64>(1, (i64)mx - sub);
    const i64 last = std::max<i64>((i64)chrom_size, a_last - 1);
    *first = (u64)a0;
    *len = last >= a0 ? (u64)(last - a0 + 1) : 0;
    return GTARS_OK;
}

gtars_status uniwig_counts(const uint32_t *opens, const uint32_t *closes, uint64_t n, uint32_t chrom_size, uint32_t smoothsize,
                           int kind, uint64_t max_device_bytes, uint64_t *first, uint32_t **counts, uint64_t *n_counts) {
    *counts = nullptr, *n_counts = 0, *first = 0;
    CovTrack t;
    GT_TRY(cov_prepare(opens, closes, n, chrom_size, smoothsize, kind, t));
    MallocArray<u32> h;
    if (!h.alloc(t.len)) return fail(GTARS_ERR_INTERNAL, "out of host memory");
    if (t.len) {
        // window after window: the count at a window's left edge comes from the same two searches as any span's
        u64 window = max_device_bytes ? std::max<u64>(max_device_bytes / sizeof(u32) / COV_TILE, 1) * COV_TILE : COV_DEFAULT_WINDOW;
        window = std::min(window, t.len);
        StreamFrame fr(nullptr);
        u32 *d;
        GT_TRY(fr.alloc(&d, (size_t)window));
        for (u64 w = 0; w < t.len; w += window) {
            const u64 wl = std::min(window, t.len - w);
            GT_TRY(launch_cov(t.open, t.close, t.n, t.sub_open, t.add_close, t.first + w, wl, d, fr.st));
            GT_TRY(fr.download(h.p + w, d, wl));
        }
        GT_TRY(fr.drain());
    }
    *first = t.first;
    *n_counts = t.len;
    *counts = h.release();
    return GTARS_OK;
}

gtars_status uniwig_counts_device(const uint32_t *d_opens, const uint32_t *d_closes, uint64_t n, uint32_t smoothsize, int kind,
                                  uint64_t window_first, uint64_t window_len, uint32_t *d_counts, void *stream) {
    if (kind != GTARS_UNIWIG_START && kind != GTARS_UNIWIG_END && kind != GTARS_UNIWIG_CORE)
        return fail(GTARS_ERR_INVALID_ARG, "uniwig: unknown track kind " + std::to_string(kind));
    if (n > COV_MAX_N || smoothsize > 0x3FFFFFFFu) return fail(GTARS_ERR_INVALID_ARG, "uniwig: argument out of range");
    if ((n && (!d_opens || (kind == GTARS_UNIWIG_CORE && !d_closes))) || (window_len && !d_counts))
        return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    if (window_first + window_len > (1ull << 33)) return fail(GTARS_ERR_INVALID_ARG, "uniwig: window out of range");
    GT_TRY(require_device());
    u32 sub, add;
    cov_transform(kind, smoothsize, &sub, &add);
    return launch_cov(d_opens, kind == GTARS_UNIWIG_CORE ? d_closes : d_opens, (u32)n, sub, add, window_first, window_len, d_counts,
                      (hipStream_t)stream);
}

gtars_status uniwig_runs(const uint32_t *opens, const uint32_t *closes, uint64_t n, uint32_t chrom_size, uint32_t smoothsize,
                         int kind, uint32_t start_position, uint32_t **run_start, uint32_t **run_end, uint32_t **run_count,
                         uint64_t *n_runs) {
    *run_start = *run_end = *run_count = nullptr, *n_runs = 0;
    CovTrack t;
    GT_TRY(cov_prepare(opens, closes, n, chrom_size, smoothsize, kind, t));
    // (compress_counts reads entry 0 of the track before anything else, utils.rs:49)
    if (!t.len) return fail(GTARS_ERR_EMPTY, "uniwig: the track has no entries to compress");
    DevBuf<u32> d;
    GT_TRY(cov_dense(t, d));
    return cov_compact<CMP_RUNS>(d.p, t.len, start_position, run_start, run_end, run_count, n_runs);
}

gtars_status uniwig_nonzero(const uint32_t *opens, const uint32_t *closes, uint64_t n, uint32_t chrom_size, uint32_t smoothsize,
                            int kind, uint32_t start_position, uint32_t **position, uint32_t **count, uint64_t *n_out) {
    *position = *count = nullptr, *n_out = 0;
    CovTrack t;
    GT_TRY(cov_prepare(opens, closes, n, chrom_size, smoothsize, kind, t));
    // at most chrom_size ENTRIES are looked at, wherever they lie (writing.rs:172)
    const u64 len = std::min<u64>(t.len, chrom_size);
    DevBuf<u32> d;
    if (len) {
        GT_TRY(d.alloc((size_t)len));
        GT_TRY(launch_cov(t.open, t.close, t.n, t.sub_open, t.add_close, t.first, len, d.p, nullptr));
    }
    return cov_compact<CMP_NONZERO>(d.p, len, start_position, position, count, nullptr, n_out);
}

}  // namespace gtars
