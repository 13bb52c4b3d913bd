// signal.hip -- K13: calc_summary_signal (gtars-genomicdist/src/signal.rs:356-526) over a signal matrix that is resident
// on the device: the row-major f64 values and an AIList-kind overlap index of the rows with val = row (SignalDevice).
// The reference walks every query's hits on one thread; here one call is
//
//   * hits: the two-pass enumerate of the tokenizer (gtars_tokenize_device for the offsets and the total,
//     gtars_fill_device_n for the row ids), in the AIList's result order -- the fold below depends on it.
//   * compaction: the flag offsets[i + 1] > offsets[i] through the scan gives every query with a hit its output row (query
//     order) and the row count R; k_signal_rows writes the query index of every output row.
//   * k_signal_fold: lanes run across CONDITIONS, so a hit's row is read as contiguous 8-byte elements.  A group of
//     G = next_pow2(n_cond) <= 64 lanes owns an output row (64 / G rows side by side in a wave; more than 64 conditions:
//     the group takes them 64 at a time).  The group reads G row ids of the CSR at once -- one per lane -- and hands
//     them round by shuffle; four hit rows' loads are issued before the first is folded.  A query with more than
//     SIGNAL_SPLIT_HITS hits is folded by all four waves of the workgroup, every wave a contiguous slice of the hits,
//     and the slices' results are combined in slice order through LDS.
//   * the fold rule, per condition: the reference copies the first hit's row and then replaces a value only by a greater
//     one.  Order-free: start from -inf and let a hit replace the accumulator only when it is GREATER (NaN never is, a
//     tie keeps the earlier hit -- which decides between 0.0 and -0.0); if the FIRST hit's value is a NaN the result is
//     that NaN, bits kept.  In this form slices combine by the same comparison.  Values move as bits: results are the
//     reference's bit for bit.
//   * statistics: the R x n_cond result is sorted per condition by sort_perm (seg = condition, k1 / k2 = the halves of
//     an order-preserving key of the value; -0.0 and 0.0 share a key, as the reference's comparator calls them equal and
//     its sort is stable; NaNs sort last, the one pinned divergence -- the reference's comparator is inconsistent on a
//     column that holds one).  Conditions are sorted in groups of at most sort_elems / R, the sort's count is 32-bit.
//     k_signal_stats, a workgroup per condition, reads the sorted column THROUGH the permutation and produces the five
//     numbers of boxplot_stats / fivenum_median; its arithmetic is not contracted (the reference rounds
//     hinge - 1.5 * iqr twice).
#include <cmath>
#include <cstdlib>
#include <memory>

#include "common.h"
#include "pipeline.h"
#include "signal.h"

namespace gtars {

struct SignalDevice {
    int device = -1;
    u32 n = 0, n_cond = 0, n_chrom = 0;
    DevBuf<double> values;  // [n * n_cond]
    gtars_index_t *ix = nullptr;
};

SignalSummary::~SignalSummary() {
    free(qidx);
    free(values);
    free(stats);
}

namespace {

constexpr int SIG_TPB = 256;
constexpr int SIG_WAVES = SIG_TPB / 64;
constexpr u32 SIG_MAX_BLOCKS = 256 * 8;
constexpr u64 SIG_MAX_N = 0xFFFFF000u;

__global__ void k_signal_flags(const u64 *__restrict__ off, u32 n, u32 *__restrict__ flag) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) flag[i] = off[i + 1] > off[i];
}

__global__ void k_signal_rows(const u64 *__restrict__ off, const u64 *__restrict__ row_of, u32 n, u32 *__restrict__ qidx) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x)
        if (off[i + 1] > off[i]) qidx[row_of[i]] = (u32)i;
}

__device__ __forceinline__ bool is_nan_bits(double x) { return (__double_as_longlong(x) & 0x7FFFFFFFFFFFFFFFll) > 0x7FF0000000000000ll; }

// the fold of the hits [hb, he) of one query for condition c by a group of G lanes (this one: gl), in CSR order
template <int G>
__device__ __forceinline__ double fold_slice(const double *__restrict__ m, const u32 *__restrict__ ids, u64 hb, u64 he, u32 n_cond, u32 c,
                                             bool active, int gl) {
    double acc = -INFINITY;
    for (u64 h = hb; h < he; h += G) {
        const u32 cnt = (u32)std::min<u64>(G, he - h);
        u32 id = 0;
        if ((u32)gl < cnt) id = ids[h + gl];
        for (u32 t = 0; t < cnt; t += 4) {
            double v[4];
#pragma unroll
            for (u32 k = 0; k < 4; ++k) {
                const u32 row = __shfl(id, (int)((t + k) & (G - 1)), G);
                v[k] = active && t + k < cnt ? m[(u64)row * n_cond + c] : -INFINITY;
            }
#pragma unroll
            for (u32 k = 0; k < 4; ++k)
                if (v[k] > acc) acc = v[k];
        }
    }
    return acc;
}

template <int G>
__global__ void __launch_bounds__(SIG_TPB)
k_signal_fold(const double *__restrict__ m, u32 n_cond, const u64 *__restrict__ off, const u32 *__restrict__ ids,
              const u32 *__restrict__ qidx, u32 n_rows, double *__restrict__ out) {
    constexpr int GPB = SIG_TPB / G;
    __shared__ double part[SIG_WAVES][64];
    const int gl = threadIdx.x % G, g = threadIdx.x / G;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (u64 t0 = (u64)blockIdx.x * GPB; t0 < n_rows; t0 += (u64)gridDim.x * GPB) {
        const u64 r = t0 + g;
        if (r < n_rows) {
            const u32 q = qidx[r];
            const u64 hb = off[q], he = off[q + 1];
            if (he - hb <= SIGNAL_SPLIT_HITS) {
                const u64 first = (u64)ids[hb] * n_cond;
                for (u32 c0 = 0; c0 < n_cond; c0 += G) {
                    const u32 c = c0 + gl;
                    const bool active = c < n_cond;
                    const double acc = fold_slice<G>(m, ids, hb, he, n_cond, c, active, gl);
                    if (active) {
                        const double f = m[first + c];
                        out[r * n_cond + c] = is_nan_bits(f) ? f : acc;
                    }
                }
            }
        }
        // the tile's heavy rows, one after the other by the whole workgroup (the test is the same in every thread)
        const u32 in_tile = (u32)std::min<u64>(GPB, n_rows - t0);
        for (u32 j = 0; j < in_tile; ++j) {
            const u64 rr = t0 + j;
            const u32 q = qidx[rr];
            const u64 hb = off[q], he = off[q + 1];
            if (he - hb <= SIGNAL_SPLIT_HITS) continue;
            const u64 per = (he - hb + SIG_WAVES - 1) / SIG_WAVES;
            const u64 sb = std::min<u64>(hb + wave * per, he), se = std::min<u64>(sb + per, he);
            const u64 first = (u64)ids[hb] * n_cond;
            for (u32 c0 = 0; c0 < n_cond; c0 += 64) {
                const u32 c = c0 + lane;
                const bool active = c < n_cond;
                part[wave][lane] = fold_slice<64>(m, ids, sb, se, n_cond, c, active, lane);
                __syncthreads();
                if (wave == 0 && active) {
                    double acc = part[0][lane];
#pragma unroll
                    for (int w = 1; w < SIG_WAVES; ++w) {
                        const double v = part[w][lane];
                        if (v > acc) acc = v;
                    }
                    const double f = m[first + c];
                    out[rr * n_cond + c] = is_nan_bits(f) ? f : acc;
                }
                __syncthreads();
            }
        }
    }
}

// element e = cl * n_rows + r of a group of conditions [c0, c0 + gc): seg = cl, (k1, k2) = the halves of a key that
// ascends with the value, -0.0 as 0.0, every NaN last
__global__ void k_signal_keys(const double *__restrict__ res, u32 n_rows, u32 n_cond, u32 c0, u32 n_elems, u32 *__restrict__ seg,
                              u32 *__restrict__ k1, u32 *__restrict__ k2) {
    for (u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x; e < n_elems; e += (u64)gridDim.x * blockDim.x) {
        const u32 cl = (u32)(e / n_rows), r = (u32)(e % n_rows);
        const double x = res[(u64)r * n_cond + c0 + cl];
        u64 b = (u64)__double_as_longlong(x);
        if (b == 0x8000000000000000ull) b = 0;
        u64 key = b >> 63 ? ~b : b | 0x8000000000000000ull;
        if (is_nan_bits(x)) key = ~0ull;
        seg[e] = cl;
        k1[e] = (u32)(key >> 32);
        k2[e] = (u32)key;
    }
}

// boxplot_stats / fivenum_median (signal.rs:461-526) of condition c0 + blockIdx.x over its sorted column
__global__ void __launch_bounds__(SIG_TPB)
k_signal_stats(const double *__restrict__ res, const u32 *__restrict__ perm, u32 n_rows, u32 n_cond, u32 c0, double *__restrict__ stats) {
#pragma clang fp contract(off)
    __shared__ u32 lo_at, hi_at;  // first position >= the lower fence; 1 + last position <= the upper fence
    const u32 cl = blockIdx.x, c = c0 + cl;
    const u32 *col = perm + (u64)cl * n_rows;
    const u64 e0 = (u64)cl * n_rows;
    auto at = [&](u32 p) { return res[(u64)(col[p] - e0) * n_cond + c]; };
    auto median = [&](u32 a, u32 b) {  // of the sorted positions [a, b), b > a
        const u32 k = b - a;
        return k % 2 == 0 ? (at(a + k / 2 - 1) + at(a + k / 2)) / 2.0 : at(a + k / 2);
    };
    if (threadIdx.x == 0) lo_at = 0xFFFFFFFFu, hi_at = 0;
    const u32 mid = n_rows / 2;
    const double med = median(0, n_rows);
    const double lh = median(0, n_rows % 2 == 0 ? mid : mid + 1), uh = median(mid, n_rows);
    const double iqr = uh - lh;
    const double t = 1.5 * iqr;
    const double lf = lh - t, uf = uh + t;
    __syncthreads();
    u32 lo = 0xFFFFFFFFu, hi = 0;
    for (u32 p = threadIdx.x; p < n_rows; p += SIG_TPB) {
        const double x = at(p);
        if (x >= lf) lo = std::min(lo, p);
        if (x <= uf) hi = std::max(hi, p + 1);
    }
    atomicMin(&lo_at, lo);
    atomicMax(&hi_at, hi);
    __syncthreads();
    if (threadIdx.x == 0) {
        double *o = stats + (u64)c * 5;
        o[0] = lo_at != 0xFFFFFFFFu ? at(lo_at) : lh;
        o[1] = lh;
        o[2] = med;
        o[3] = uh;
        o[4] = hi_at ? at(hi_at - 1) : uh;
    }
}

template <int G>
void launch_fold(const SignalDevice &s, const u64 *off, const u32 *ids, const u32 *qidx, u32 n_rows, double *res, hipStream_t st) {
    hipLaunchKernelGGL(k_signal_fold<G>, dim3(grid_for(n_rows, SIG_TPB / G, SIG_MAX_BLOCKS)), dim3(SIG_TPB), 0, st, s.values.p, s.n_cond, off,
                       ids, qidx, n_rows, res);
}

template <class T>
bool host_copy(T **out, size_t n) {
    *out = (T *)malloc(std::max<size_t>(n, 1) * sizeof(T));
    return *out != nullptr;
}

// the columns are on the device, the frame's stream is the caller's
gtars_status summary_on(StreamFrame &fr, const SignalDevice &s, const u32 *qc, const u32 *qs, const u32 *qe, u64 n, bool want_rows,
                        u32 sort_elems, SignalSummary &out) {
    hipStream_t st = fr.st;
    const u32 nc = s.n_cond;
    u64 *off, total = 0;
    GT_TRY(fr.alloc(&off, (size_t)n + 1));
    GT_TRY(gtars_tokenize_device(s.ix, qc, qs, qe, n, off, nullptr, 0, &total, st));
    if (!total) return GTARS_OK;
    u32 *ids, *flag, *qidx;
    GT_TRY(fr.alloc(&ids, (size_t)total));
    GT_TRY(gtars_fill_device_n(s.ix, qc, qs, qe, n, off, ids, total, st));
    GT_TRY(fr.alloc(&flag, (size_t)n));
    hipLaunchKernelGGL(k_signal_flags, dim3(grid_for(n, SIG_TPB, SIG_MAX_BLOCKS)), dim3(SIG_TPB), 0, st, off, (u32)n, flag);
    GT_HIP(hipGetLastError());
    u64 *row_of, rows = 0;
    GT_TRY(scan_total(fr, flag, n, &row_of, &rows));
    const u32 R = (u32)rows;
    GT_TRY(fr.alloc(&qidx, (size_t)R));
    hipLaunchKernelGGL(k_signal_rows, dim3(grid_for(n, SIG_TPB, SIG_MAX_BLOCKS)), dim3(SIG_TPB), 0, st, off, row_of, (u32)n, qidx);
    GT_HIP(hipGetLastError());
    double *res, *d_stats;
    GT_TRY(fr.alloc(&res, (size_t)R * nc));
    GT_TRY(fr.alloc(&d_stats, (size_t)nc * 5));
    {
        ProfScope ps("k_signal_fold", st);
        if (nc <= 1) launch_fold<1>(s, off, ids, qidx, R, res, st);
        else if (nc <= 2) launch_fold<2>(s, off, ids, qidx, R, res, st);
        else if (nc <= 4) launch_fold<4>(s, off, ids, qidx, R, res, st);
        else if (nc <= 8) launch_fold<8>(s, off, ids, qidx, R, res, st);
        else if (nc <= 16) launch_fold<16>(s, off, ids, qidx, R, res, st);
        else if (nc <= 32) launch_fold<32>(s, off, ids, qidx, R, res, st);
        else launch_fold<64>(s, off, ids, qidx, R, res, st);
        GT_HIP(hipGetLastError());
    }
    // conditions [c0, c0 + gc) per sort: R * gc elements
    const u32 group = std::max<u32>(1, std::min<u32>(nc, sort_elems / R));
    u32 *seg, *k1, *k2;
    GT_TRY(fr.alloc(&seg, (size_t)R * group));
    GT_TRY(fr.alloc(&k1, (size_t)R * group));
    GT_TRY(fr.alloc(&k2, (size_t)R * group));
    for (u32 c0 = 0; c0 < nc; c0 += group) {
        const u32 gc = std::min(group, nc - c0), ne = R * gc;
        u32 *perm;
        {
            ProfScope ps("k_signal_keys", st);
            hipLaunchKernelGGL(k_signal_keys, dim3(grid_for(ne, SIG_TPB, SIG_MAX_BLOCKS)), dim3(SIG_TPB), 0, st, res, R, nc, c0, ne, seg, k1, k2);
            GT_HIP(hipGetLastError());
        }
        const size_t mark = fr.bufs.size();
        GT_TRY(sort_perm(fr, seg, k1, k2, ne, gc, &perm));
        {
            ProfScope ps("k_signal_stats", st);
            hipLaunchKernelGGL(k_signal_stats, dim3(gc), dim3(SIG_TPB), 0, st, res, perm, R, nc, c0, d_stats);
            GT_HIP(hipGetLastError());
        }
        if (c0 + gc < nc) {  // the next group sorts into memory of its own: this group's goes back first
            GT_TRY(fr.drain());
            fr.bufs.erase(fr.bufs.begin() + (std::ptrdiff_t)mark, fr.bufs.end());
        }
    }
    out.n_rows = R;
    if (!host_copy(&out.stats, (size_t)nc * 5)) return fail(GTARS_ERR_INTERNAL, "out of host memory");
    GT_TRY(fr.download(out.stats, d_stats, (size_t)nc * 5));
    if (want_rows) {
        if (!host_copy(&out.qidx, (size_t)R) || !host_copy(&out.values, (size_t)R * nc)) return fail(GTARS_ERR_INTERNAL, "out of host memory");
        GT_TRY(fr.download(out.qidx, qidx, (size_t)R));
        GT_TRY(fr.download(out.values, res, (size_t)R * nc));
    }
    return fr.drain();
}

gtars_status check_call(const SignalDevice &s, u64 n, u32 sort_elems) {
    if (n > SIG_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "signal summary: too many query rows (" + std::to_string(n) + ")");
    if (!sort_elems) return fail(GTARS_ERR_INVALID_ARG, "signal summary: the sort group holds no element");
    if (s.device < 0 || !s.ix) return fail(GTARS_ERR_INTERNAL, "signal summary: the matrix has no device image");
    return GTARS_OK;
}

}  // namespace

gtars_status signal_build(const uint32_t *chrom, const uint32_t *start, const uint32_t *end, uint64_t n, uint32_t n_chrom,
                          const double *values, uint32_t n_cond, SignalDevice **out) {
    *out = nullptr;
    if (!n || !n_cond) return fail(GTARS_ERR_INVALID_ARG, "signal matrix without rows or conditions");
    if (n > SIG_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "signal matrix too large (" + std::to_string(n) + " rows)");
    GT_TRY(require_device());
    std::unique_ptr<SignalDevice, void (*)(SignalDevice *)> s(new SignalDevice, signal_free);
    GT_HIP(hipGetDevice(&s->device));
    s->n = (u32)n, s->n_cond = n_cond, s->n_chrom = n_chrom;
    GT_TRY(gtars_index_build(chrom, start, end, nullptr, n, n_chrom, GTARS_KIND_AILIST, &s->ix));
    GT_TRY(s->values.alloc((size_t)n * n_cond));
    GT_HIP(hipMemcpy(s->values.p, values, (size_t)n * n_cond * sizeof(double), hipMemcpyHostToDevice));
    *out = s.release();
    return GTARS_OK;
}

void signal_free(SignalDevice *s) {
    if (!s) return;
    DeviceScope on(s->device);  // (the buffers go back to the device they came from)
    gtars_index_free(s->ix);
    delete s;
}

int signal_device(const SignalDevice *s) { return s ? s->device : -1; }

gtars_status signal_summary_device(const SignalDevice &s, const uint32_t *d_chrom, const uint32_t *d_start, const uint32_t *d_end,
                                   uint64_t n, bool want_rows, uint32_t sort_elems, SignalSummary &out, void *stream) {
    GT_TRY(check_call(s, n, sort_elems));
    if (!n) return GTARS_OK;
    if (!d_chrom || !d_start || !d_end) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    GT_TRY(require_handle_device(s.device));
    StreamFrame fr((hipStream_t)stream);
    return summary_on(fr, s, d_chrom, d_start, d_end, n, want_rows, sort_elems, out);
}

gtars_status signal_summary(const SignalDevice &s, const uint32_t *chrom, const uint32_t *start, const uint32_t *end, uint64_t n,
                            uint32_t sort_elems, SignalSummary &out) {
    GT_TRY(check_call(s, n, sort_elems));
    if (!n) return GTARS_OK;
    if (!chrom || !start || !end) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    DeviceScope on(s.device);
    GT_TRY(on.st);
    StreamFrame fr(nullptr);
    u32 *qc, *qs, *qe;
    GT_TRY(fr.upload(&qc, chrom, (size_t)n));
    GT_TRY(fr.upload(&qs, start, (size_t)n));
    GT_TRY(fr.upload(&qe, end, (size_t)n));
    return summary_on(fr, s, qc, qs, qe, n, true, sort_elems, out);
}

}  // namespace gtars
