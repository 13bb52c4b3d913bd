// annot.hip -- K10: distances from query regions to the nearest TSS / feature midpoint on the device
// (gtars-genomicdist/src/models.rs:516-690, TssIndex; gtars-python/src/models/tss_index.rs).
//
//   * index build, once per handle on the device current at the first distance call: the midpoints start + width / 2 of
//     the index set (wrapping u32), the stable radix sort of sort.hip by (chromosome, midpoint), one gather.  The host
//     knows the per-chromosome counts, so the segment offsets are its exclusive prefix sum.
//   * one kernel writes both results per query (k_tss_dist): midpoint, lower bound in its chromosome's segment, the two
//     neighbours.  An exact hit is 0; otherwise |distance| = min over the neighbours that exist, and the signed distance
//     feature - query takes the left (upstream) neighbour on a tie.  A chromosome without a segment gets u32::MAX and
//     INT64_MAX.
//   * search form: a block first stages every 2^shift-th key of the whole sorted index into LDS (at most TSS_LDS_KEYS
//     of them), so the first levels of a search stay in LDS and only the last `shift` levels load from global memory.
//     GTARS_TSS_GLOBAL_SEARCH (A/B switch) searches global memory from the top.
//   * output order: chromosomes in order of first appearance in the query set, set order within one (the ids of a set's
//     chromosome dictionary ARE first-appearance ranks).  A query whose ids never decrease (every set read from a BED
//     file) is answered in place; any other is read through the permutation of a stable sort by chromosome id.
#include <algorithm>
#include <memory>
#include <numeric>
#include <vector>

#include "annot.h"
#include "common.h"
#include "pipeline.h"

namespace gtars {

struct TssDevice {
    int device = -1;
    u32 n = 0, n_chrom = 0;
    DevBuf<u32> mids;  // sorted by (chromosome, midpoint)
    DevBuf<u32> off;   // n_chrom + 1 segment offsets
};

namespace {

constexpr int TSS_TPB = 256;
constexpr u32 TSS_LDS_KEYS = 2048;       // 8 KiB of sampled keys per block
constexpr u32 TSS_MAX_BLOCKS = 2048;     // 8 blocks per CU: the LDS table is staged once per block, not once per query
constexpr u64 TSS_MAX_N = 0xFFFFF000u;

__global__ void k_midpoints(const u32 *__restrict__ start, const u32 *__restrict__ end, u32 n, u32 *__restrict__ mid) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u32 s = start[i];
        mid[i] = s + (end[i] - s) / 2;
    }
}

template <bool LDS>
__global__ void __launch_bounds__(TSS_TPB)
k_tss_dist(const u32 *__restrict__ qc, const u32 *__restrict__ qs, const u32 *__restrict__ qe, const u32 *__restrict__ perm, u32 nq,
           const u32 *__restrict__ seg_of, const u32 *__restrict__ off, const u32 *__restrict__ mids, u32 n_keys, u32 shift,
           u32 *__restrict__ oabs, i64 *__restrict__ osig) {
    __shared__ u32 samp[LDS ? TSS_LDS_KEYS : 1];
    if (LDS) {
        for (u32 k = threadIdx.x; k < n_keys; k += TSS_TPB) samp[k] = mids[(u64)k << shift];
        __syncthreads();
    }
    for (u64 j = (u64)blockIdx.x * TSS_TPB + threadIdx.x; j < nq; j += (u64)gridDim.x * TSS_TPB) {
        const u32 i = perm ? perm[j] : (u32)j;
        const u32 seg = seg_of[qc[i]];
        u32 a = 0xFFFFFFFFu;
        i64 sg = INT64_MAX;
        if (seg != 0xFFFFFFFFu) {
            const u32 s = qs[i];
            const u32 mid = s + (qe[i] - s) / 2;
            const u32 lo = off[seg], hi = off[seg + 1];  // lo < hi: a segment exists only for a chromosome with regions
            u32 wlo = lo, whi = hi;
            if (LDS) {
                // samples k with lo <= k << shift < hi; the first one >= mid bounds the window from above, the one
                // before it (< mid) from below: at most 2^shift - 1 keys are left for global memory
                const u32 klo = (u32)(((u64)lo + (1ull << shift) - 1) >> shift);
                const u32 khi = (u32)(((u64)hi + (1ull << shift) - 1) >> shift);
                const u32 kk = first_ge(samp, klo, khi, mid);
                if (kk > klo) wlo = ((kk - 1) << shift) + 1;
                if (kk < khi) whi = kk << shift;
            }
            const u32 p = first_ge(mids, wlo, whi, mid);
            const u32 r = p < hi ? mids[p] : 0u;
            if (p < hi && r == mid) {
                a = 0;
                sg = 0;
            } else {
                const bool has_l = p > lo, has_r = p < hi;
                const u32 dl = has_l ? mid - mids[p - 1] : 0u, dr = has_r ? r - mid : 0u;
                if (has_l && (!has_r || dl <= dr)) {
                    a = dl;
                    sg = -(i64)dl;
                } else {
                    a = dr;
                    sg = (i64)dr;
                }
            }
        }
        oabs[j] = a;
        osig[j] = sg;
    }
}

// the LDS-staged search unless GTARS_TSS_GLOBAL_SEARCH (A/B switch) asks for the global one
bool lds_search() { return !cfg_flag("GTARS_TSS_GLOBAL_SEARCH"); }

}  // namespace

gtars_status tss_build(const uint32_t *chrom, const uint32_t *start, const uint32_t *end, uint64_t n, uint32_t n_chrom,
                       TssDevice **out) {
    *out = nullptr;
    if (n > TSS_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "TSS index too large (" + std::to_string(n) + " regions)");
    GT_TRY(require_device());
    std::vector<u32> off(n_chrom + 1, 0);
    for (u64 i = 0; i < n; ++i) {
        if (chrom[i] >= n_chrom) return fail(GTARS_ERR_INTERNAL, "TSS index: chromosome id out of range");
        ++off[chrom[i] + 1];
    }
    std::partial_sum(off.begin(), off.end(), off.begin());
    auto t = std::make_unique<TssDevice>();
    GT_HIP(hipGetDevice(&t->device));
    t->n = (u32)n;
    t->n_chrom = n_chrom;
    GT_TRY(t->off.upload(off));
    GT_TRY(t->mids.alloc(n));
    if (n) {
        StreamFrame fr(nullptr);
        u32 *dc, *ds, *de, *mid, *perm;
        GT_TRY(fr.upload(&dc, chrom, n));
        GT_TRY(fr.upload(&ds, start, n));
        GT_TRY(fr.upload(&de, end, n));
        GT_TRY(fr.alloc(&mid, n));
        hipLaunchKernelGGL(k_midpoints, dim3(grid_for(n, TSS_TPB)), dim3(TSS_TPB), 0, fr.st, ds, de, (u32)n, mid);
        GT_TRY(sort_perm(fr, dc, mid, nullptr, (u32)n, n_chrom, &perm));  // (chromosome, midpoint)
        GT_TRY(device_gather_u32(mid, perm, (u32)n, t->mids.p, fr.st));
        GT_HIP(hipGetLastError());
        GT_TRY(fr.drain());
    }
    *out = t.release();
    return GTARS_OK;
}

void tss_free(TssDevice *t) {
    if (!t) return;
    DeviceScope on(t->device);  // (the buffers go back to the device they came from)
    delete t;
}

int tss_device(const TssDevice *t) { return t ? t->device : -1; }

gtars_status tss_distances(const TssDevice *t, const uint32_t *q_chrom, const uint32_t *q_start, const uint32_t *q_end,
                           uint64_t nq, const std::vector<uint32_t> &seg_of, bool grouped, uint32_t *out_abs,
                           int64_t *out_signed) {
    if (!t) return fail(GTARS_ERR_INVALID_ARG, "NULL TSS index");
    if (nq > TSS_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "query set too large (" + std::to_string(nq) + " regions)");
    for (u32 s : seg_of)
        if (s != 0xFFFFFFFFu && s >= t->n_chrom) return fail(GTARS_ERR_INTERNAL, "TSS index: segment out of range");
    for (u64 i = 0; i < nq; ++i)
        if (q_chrom[i] >= seg_of.size()) return fail(GTARS_ERR_INTERNAL, "TSS query: chromosome id out of range");
    if (!nq) return GTARS_OK;
    DeviceScope on(t->device);
    GT_TRY(on.st);
    StreamFrame fr(nullptr);
    hipStream_t st = fr.st;
    const u32 n = (u32)nq;
    u32 *qc, *qs, *qe, *d_seg, *perm = nullptr, *oabs;
    i64 *osig;
    GT_TRY(fr.upload(&qc, q_chrom, nq));
    GT_TRY(fr.upload(&qs, q_start, nq));
    GT_TRY(fr.upload(&qe, q_end, nq));
    GT_TRY(fr.upload(&d_seg, seg_of.data(), seg_of.size()));
    GT_TRY(fr.alloc(&oabs, nq));
    GT_TRY(fr.alloc(&osig, nq));
    // stable by chromosome id alone (one 32-bit key, no chromosome pass)
    if (!grouped) GT_TRY(sort_perm(fr, qc, qc, nullptr, n, 1, &perm));
    // the LDS table: every 2^shift-th key of the index, at most TSS_LDS_KEYS of them
    u32 shift = 0;
    while (((u64)t->n + (1ull << shift) - 1) >> shift > TSS_LDS_KEYS) ++shift;
    const u32 n_keys = (u32)(((u64)t->n + (1ull << shift) - 1) >> shift);
    {
        ProfScope ps("tss_distance_kernel", st);
        if (lds_search() && t->n)
            hipLaunchKernelGGL(k_tss_dist<true>, dim3(grid_for(nq, TSS_TPB, TSS_MAX_BLOCKS)), dim3(TSS_TPB), 0, st, qc, qs, qe, perm, n,
                               d_seg, t->off.p, t->mids.p, n_keys, shift, oabs, osig);
        else
            hipLaunchKernelGGL(k_tss_dist<false>, dim3(grid_for(nq, TSS_TPB, TSS_MAX_BLOCKS)), dim3(TSS_TPB), 0, st, qc, qs, qe, perm, n,
                               d_seg, t->off.p, t->mids.p, 0u, 0u, oabs, osig);
        GT_HIP(hipGetLastError());
    }
    GT_TRY(fr.download(out_abs, oabs, nq));
    GT_TRY(fr.download(out_signed, osig, nq));
    return fr.drain();
}

}  // namespace gtars
