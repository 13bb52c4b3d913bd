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
//   * k_cov_tile, one pass, the output written once: the coverage tile skeleton of cov_tile.h (spans, the LDS
//     difference tile, the scan, the 16-byte stores) over the event source CovSrc -- unit weights, so the count that
//     enters a span is the difference of the two search results, and the transform p -> (max(1, p - m), p + m + 1)
//     applied on load, so the start and the end track read the position column as it is.  Global traffic: 4 bytes per
//     position out, 8 bytes per event in.
//   * k_cov_flag_count / k_cov_compact: the run-length form (bedGraph) and the non-zero form (variableStep wig) of a
//     track that sits in device memory: flags per position, block counts, the exclusive scan of kernels.hip, scatter.
//     Only the runs / pairs cross to the host.
//   * the columns are sorted with the radix sort of sort.hip.
#include <algorithm>
#include <cstdlib>
#include <memory>

#include "common.h"
#include "cov_tile.h"
#include "pipeline.h"
#include "scan.h"
#include "uniwig.h"

namespace gtars {

namespace {

// K11's event source: two u32 columns, the transform p -> (max(1, p - sub_open), p + add_close) applied on load in i64, so
// the start and the end track read the position column as it is; every event weighs 1
struct CovSrc {
    const u32 *__restrict__ A, *__restrict__ E;
    u32 n, sub_open, add_close;
    static constexpr bool WEIGHTED = false;

    __device__ __forceinline__ i64 open_at(u64 i) const {
        const i64 v = (i64)A[i] - (i64)sub_open;
        return v < 1 ? 1 : v;
    }
    __device__ __forceinline__ i64 close_at(u64 i) const { return (i64)E[i] + (i64)add_close; }

    // number of events in front of position pos: the first index whose (transformed) value is >= pos
    template <bool OPEN>
    __device__ __forceinline__ u32 lower_bound(i64 pos) const {
        u32 lo = 0, hi = n;
        while (lo < hi) {
            const u32 mid = lo + ((hi - lo) >> 1);
            if ((OPEN ? open_at(mid) : close_at(mid)) >= pos) hi = mid;
            else lo = mid + 1;
        }
        return lo;
    }
    __device__ __forceinline__ u32 first_open(u64 pos) const { return lower_bound<true>((i64)pos); }
    __device__ __forceinline__ u32 first_close(u64 pos) const { return lower_bound<false>((i64)pos); }
    __device__ __forceinline__ u32 entering(u32 ia, u32 ie) const { return ia - ie; }

    // (v >= t0 holds for ascending columns: a caller's unsorted one must not leave the tile)
    __device__ __forceinline__ void open(u64 i, u64 t0, u64 t1, u32 &key, u32 &) const {
        const i64 v = open_at(i);
        if (v >= (i64)t0 && v < (i64)t1) key = (u32)(v - (i64)t0);
    }
    __device__ __forceinline__ void close(u64 i, u64 t0, u64 t1, u32 &key, u32 &) const {
        const i64 v = close_at(i);
        if (v >= (i64)t0 && v < (i64)t1) key = (u32)(v - (i64)t0);
    }
};

// positions w0 + [0, len) of the track into out[0, len); out is 16-byte aligned, span a multiple of COV_TILE
__global__ void __launch_bounds__(COV_TPB)
k_cov_tile(const u32 *__restrict__ A, const u32 *__restrict__ E, u32 n, u32 sub_open, u32 add_close, u64 w0, u64 len, u64 span,
           u32 *__restrict__ out) {
    cov_tile_body(CovSrc{A, E, n, sub_open, add_close}, w0, len, span, out);
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

gtars_status launch_cov(const u32 *open, const u32 *close, u32 n, u32 sub_open, u32 add_close, u64 w_first, u64 w_len, u32 *d_out,
                        hipStream_t st) {
    return cov_tile_launch("k_cov_tile", "uniwig", k_cov_tile, st, w_first, w_len, d_out, open, close, n, sub_open, add_close);
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
        const u64 window = cov_window(max_device_bytes, t.len);
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
