// partitions.hip -- K14: query regions classified into the partitions of a PartitionList on the device
// (gtars-genomicdist/src/partitions.rs:506-592, calc_partitions_priority / calc_partitions_bp).
//
//   * index build, once per handle on the device current at the first count: segment (p, c) holds the rows of partition
//     p on chromosome c.  Two stable radix sorts (sort.hip) give, per segment, the starts ascending with every row's own
//     end beside it, and the ends ascending on their own; scan.hip gives a u64 exclusive prefix sum of either sorted
//     column (one scan over all segments: a segment's sum is a difference of two entries).  The host knows the row
//     counts, so the [P][n_chrom + 1] offset table is its prefix sum.
//   * one kernel, one lane per query (k_partitions).  The reference tests every row with  s < qe && e > qs  (AIList).
//     For rows with s <= e and a query with qs < qe
//         #{rows hit} = #{s < qe} - #{e <= qs}                 (a row with e <= qs has s <= e <= qs < qe)
//         sum of overlap widths = F(qe) - F(qs),  F(x) = sum min(e, x) - sum min(s, x)
//     so priority mode is two binary searches per partition, first hit in list order wins, and bp mode four searches
//     and four prefix-sum reads per partition, exact however the rows of one partition overlap each other.
//   * where the identities fail.  Rows with s > e are never put into the sorted columns: they wait in a side list
//     (expected empty) that every lane walks with the literal test.  A query with qs > qe walks the rows of its segments
//     with the literal test.  A zero-length query (qs == qe) keeps the searches: the count is only off by the zero-length
//     rows that sit on the same position (each is in #{e <= qs} and not in #{s < qe}), and those are counted out by
//     looking at the rows with start == qs.  In bp mode none of these can add anything -- min(qe, e) > max(qs, s) needs
//     s < e and qs < qe -- so that mode skips them.
//   * reduction: priority mode folds the buckets by wave ballot and popcount into P + 1 LDS counters, bp mode sums every
//     partition's u64 across the wave and adds it to an LDS u64; one global atomic per bucket per block at the end.  The
//     sums leave as u64: the reference's u32 wrap is host arithmetic (partitions.cpp).
#include <memory>
#include <numeric>
#include <vector>

#include "common.h"
#include "partitions.h"
#include "pipeline.h"
#include "scan.h"

namespace gtars {

struct PartDevice {
    int device = -1;
    u32 n = 0, n_part = 0, n_chrom = 0, n_side = 0;
    DevBuf<u32> ss, es;    // starts ascending per segment, and the same rows' ends
    DevBuf<u32> se;        // ends ascending per segment
    DevBuf<u64> ps, pe;    // n + 1 exclusive prefix sums of ss and se
    DevBuf<u32> off;       // [n_part][n_chrom + 1] positions into the columns
    DevBuf<uint4> side;    // rows with start > end: {partition, chromosome, start, end}, in list order
};

namespace {

constexpr int PT_TPB = 256;
constexpr u32 PT_MAX_BLOCKS = 2048;
constexpr u64 PT_MAX_N = 0xFFFFF000u;
constexpr u32 ABSENT = 0xFFFFFFFFu;

// sum over rows [lo, hi) of min(x[i], key); x ascends, pre is its exclusive prefix sum
__device__ __forceinline__ u64 sum_min(const u32 *__restrict__ x, const u64 *__restrict__ pre, u32 lo, u32 hi, u32 key) {
    const u32 j = first_ge(x, lo, hi, key);
    return (pre[j] - pre[lo]) + (u64)(hi - j) * key;
}

template <bool BP>
__global__ void __launch_bounds__(PT_TPB)
k_partitions(const u32 *__restrict__ qc, const u32 *__restrict__ qs, const u32 *__restrict__ qe, u32 n, const u32 *__restrict__ seg_of,
             u32 n_seg_of, u32 n_part, u32 n_chrom, const u32 *__restrict__ off, const u32 *__restrict__ ss, const u32 *__restrict__ es,
             const u32 *__restrict__ se, const u64 *__restrict__ ps, const u64 *__restrict__ pe, const uint4 *__restrict__ side, u32 n_side,
             u64 *__restrict__ acc, u8 *__restrict__ assign) {
    __shared__ u64 sum[PART_MAX + 1];
    for (u32 k = threadIdx.x; k <= n_part; k += PT_TPB) sum[k] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    // every lane of a wave takes part in the ballots and shuffles: the loop bound is the wave's
    for (u64 base = (u64)blockIdx.x * PT_TPB + (threadIdx.x & ~63u); base < n; base += (u64)gridDim.x * PT_TPB) {
        const u64 j = base + lane;
        const bool live = j < n;
        u32 c = ABSENT, s = 0, e = 0;
        if (live) {
            c = qc[j], s = qs[j], e = qe[j];
            if (seg_of) c = c < n_seg_of ? seg_of[c] : ABSENT;
            if (c >= n_chrom) c = ABSENT;
        }
        if (BP) {
            for (u32 p = 0; p < n_part; ++p) {
                u64 v = 0;
                if (c != ABSENT && s < e) {
                    const u32 lo = off[p * (n_chrom + 1) + c], hi = off[p * (n_chrom + 1) + c + 1];
                    if (lo < hi)
                        v = (sum_min(se, pe, lo, hi, e) - sum_min(ss, ps, lo, hi, e)) - (sum_min(se, pe, lo, hi, s) - sum_min(ss, ps, lo, hi, s));
                }
                v = wave_reduce_sum_u64(v);
                if (lane == 0 && v) atomicAdd((unsigned long long *)&sum[p], (unsigned long long)v);
            }
            const u64 w = wave_reduce_sum_u64(live ? (u64)(u32)(e - s) : 0);
            if (lane == 0 && w) atomicAdd((unsigned long long *)&sum[n_part], (unsigned long long)w);
        } else {
            u32 bucket = n_part;
            if (c != ABSENT) {
                for (u32 p = 0; p < n_part && bucket == n_part; ++p) {
                    const u32 lo = off[p * (n_chrom + 1) + c], hi = off[p * (n_chrom + 1) + c + 1];
                    if (lo == hi) continue;
                    bool hit = false;
                    if (s <= e) {
                        // #{start < qe} > #{end <= qs}; for qs == qe the rows that sit on that very position with zero
                        // length are in the second count and not in the first: they are counted out (rows with
                        // start == qs are one short run of the start-sorted column)
                        u32 zero = 0;
                        if (s == e)
                            for (u32 i = first_ge(ss, lo, hi, s); i < hi && ss[i] == s; ++i) zero += es[i] == s;
                        hit = first_ge(ss, lo, hi, e) + zero > first_gt(se, lo, hi, s);
                    } else {
                        for (u32 i = lo; i < hi && ss[i] < e && !hit; ++i) hit = es[i] > s;
                    }
                    if (hit) bucket = p;
                }
                for (u32 k = 0; k < n_side; ++k) {
                    const uint4 r = side[k];
                    if (r.x < bucket && r.y == c && r.z < e && r.w > s) bucket = r.x;
                }
            }
            if (live && assign) assign[j] = (u8)bucket;
            unsigned long long todo = __ballot(live);
            while (todo) {  // one LDS add per bucket the wave holds
                const int l = __ffsll((long long)todo) - 1;
                const u32 b = (u32)__shfl((int)bucket, l, 64);
                const unsigned long long m = __ballot(live && bucket == b);
                if (lane == l) atomicAdd((unsigned long long *)&sum[b], (unsigned long long)__popcll(m));
                todo &= ~m;
            }
        }
    }
    __syncthreads();
    for (u32 k = threadIdx.x; k <= n_part; k += PT_TPB)
        if (sum[k]) atomicAdd((unsigned long long *)&acc[k], (unsigned long long)sum[k]);
}

// the columns are on the device, the frame's stream is the caller's
gtars_status count_on(StreamFrame &fr, const PartDevice &d, const u32 *qc, const u32 *qs, const u32 *qe, u64 n, const u32 *seg_of,
                      u32 n_seg_of, bool bp, u64 *out, u8 *d_assign) {
    u64 *acc;
    const u32 np = d.n_part;
    GT_TRY(fr.alloc(&acc, (size_t)np + 1));
    GT_HIP(hipMemsetAsync(acc, 0, ((size_t)np + 1) * 8, fr.st));
    {
        ProfScope prof(bp ? "partitions_bp_kernel" : "partitions_priority_kernel", fr.st);
        const dim3 grid(grid_for(n, PT_TPB, PT_MAX_BLOCKS)), block(PT_TPB);
        if (bp)
            hipLaunchKernelGGL(k_partitions<true>, grid, block, 0, fr.st, qc, qs, qe, (u32)n, seg_of, n_seg_of, np, d.n_chrom, d.off.p, d.ss.p,
                               d.es.p, d.se.p, d.ps.p, d.pe.p, d.side.p, d.n_side, acc, (u8 *)nullptr);
        else
            hipLaunchKernelGGL(k_partitions<false>, grid, block, 0, fr.st, qc, qs, qe, (u32)n, seg_of, n_seg_of, np, d.n_chrom, d.off.p, d.ss.p,
                               d.es.p, d.se.p, d.ps.p, d.pe.p, d.side.p, d.n_side, acc, d_assign);
        GT_HIP(hipGetLastError());
    }
    return fr.download(out, acc, (size_t)np + 1);
}

gtars_status check_call(const PartDevice *d, u64 n, bool bp, const void *assign) {
    if (!d) return fail(GTARS_ERR_INVALID_ARG, "NULL partition index");
    if (n > PT_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "query set too large (" + std::to_string(n) + " regions)");
    if (bp && assign) return fail(GTARS_ERR_INVALID_ARG, "per-query assignments exist in priority mode only");
    return GTARS_OK;
}

}  // namespace

gtars_status part_build(const std::vector<PartCols> &parts, uint32_t n_chrom, PartDevice **out) {
    *out = nullptr;
    const u32 np = (u32)parts.size();
    if (np > PART_MAX) return fail(GTARS_ERR_INVALID_ARG, "more than " + std::to_string(PART_MAX) + " partitions");
    if ((u64)np * ((u64)n_chrom + 1) > 0x7FFFFFFFull) return fail(GTARS_ERR_INVALID_ARG, "too many chromosomes");
    GT_TRY(require_device());
    // well-formed rows as (segment, start, end); the others into the side list
    std::vector<u32> seg, st, en, off((size_t)np * (n_chrom + 1), 0);
    std::vector<uint4> side;
    for (u32 p = 0; p < np; ++p) {
        const PartCols &a = parts[p];
        std::vector<u32> cnt(n_chrom, 0);
        const size_t before = seg.size();
        for (u64 i = 0; i < a.n; ++i) {
            if (a.chrom[i] >= n_chrom) return fail(GTARS_ERR_INTERNAL, "partition list: chromosome id out of range");
            if (a.start[i] > a.end[i]) {
                side.push_back(make_uint4(p, a.chrom[i], a.start[i], a.end[i]));
                continue;
            }
            seg.push_back(p * n_chrom + a.chrom[i]);
            st.push_back(a.start[i]);
            en.push_back(a.end[i]);
            ++cnt[a.chrom[i]];
        }
        u32 *row = off.data() + (size_t)p * (n_chrom + 1);
        row[0] = (u32)before;
        for (u32 c = 0; c < n_chrom; ++c) row[c + 1] = row[c] + cnt[c];
    }
    const u64 n = seg.size();
    if (n > PT_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "partition list too large (" + std::to_string(n) + " regions)");
    auto d = std::make_unique<PartDevice>();
    GT_HIP(hipGetDevice(&d->device));
    d->n = (u32)n, d->n_part = np, d->n_chrom = n_chrom, d->n_side = (u32)side.size();
    GT_TRY(d->off.upload(off));
    GT_TRY(d->side.upload(side));
    GT_TRY(d->ss.alloc(n));
    GT_TRY(d->es.alloc(n));
    GT_TRY(d->se.alloc(n));
    GT_TRY(d->ps.alloc(n + 1));
    GT_TRY(d->pe.alloc(n + 1));
    StreamFrame fr(nullptr);
    if (n) {
        u32 *dg, *ds, *de, *perm;
        GT_TRY(fr.upload(&dg, seg.data(), n));
        GT_TRY(fr.upload(&ds, st.data(), n));
        GT_TRY(fr.upload(&de, en.data(), n));
        const u32 n_seg = std::max<u32>(np * n_chrom, 1);
        GT_TRY(sort_perm(fr, dg, ds, nullptr, (u32)n, n_seg, &perm));  // (segment, start)
        GT_TRY(device_gather_u32(ds, perm, (u32)n, d->ss.p, fr.st));
        GT_TRY(device_gather_u32(de, perm, (u32)n, d->es.p, fr.st));
        GT_TRY(sort_perm(fr, dg, de, nullptr, (u32)n, n_seg, &perm));  // (segment, end)
        GT_TRY(device_gather_u32(de, perm, (u32)n, d->se.p, fr.st));
        u8 *ws;
        const size_t wsb = scan_ws_bytes(n);
        GT_TRY(fr.alloc(&ws, wsb));
        GT_TRY(launch_scan_u32_to_u64(d->ss.p, n, d->ps.p, ws, wsb, fr.st));
        GT_TRY(launch_scan_u32_to_u64(d->se.p, n, d->pe.p, ws, wsb, fr.st));
    } else {
        GT_HIP(hipMemsetAsync(d->ps.p, 0, 8, fr.st));
        GT_HIP(hipMemsetAsync(d->pe.p, 0, 8, fr.st));
    }
    GT_TRY(fr.drain());
    *out = d.release();
    return GTARS_OK;
}

void part_free(PartDevice *d) {
    if (!d) return;
    DeviceScope on(d->device);  // (the buffers go back to the device they came from)
    delete d;
}

int part_device(const PartDevice *d) { return d ? d->device : -1; }

gtars_status part_count(const PartDevice *d, const uint32_t *q_chrom, const uint32_t *q_start, const uint32_t *q_end, uint64_t n,
                        const std::vector<uint32_t> &seg_of, bool bp, uint64_t *out, uint8_t *assign) {
    GT_TRY(check_call(d, n, bp, assign));
    std::fill(out, out + d->n_part + 1, 0);
    if (!n) return GTARS_OK;
    if (!q_chrom || !q_start || !q_end) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    DeviceScope on(d->device);
    GT_TRY(on.st);
    StreamFrame fr(nullptr);
    u32 *qc, *qs, *qe, *d_seg;
    u8 *d_assign = nullptr;
    GT_TRY(fr.upload(&qc, q_chrom, (size_t)n));
    GT_TRY(fr.upload(&qs, q_start, (size_t)n));
    GT_TRY(fr.upload(&qe, q_end, (size_t)n));
    GT_TRY(fr.upload(&d_seg, seg_of.data(), seg_of.size()));
    if (assign) GT_TRY(fr.alloc(&d_assign, (size_t)n));
    GT_TRY(count_on(fr, *d, qc, qs, qe, n, d_seg, (u32)seg_of.size(), bp, out, d_assign));
    if (assign) GT_TRY(fr.download(assign, d_assign, (size_t)n));
    return fr.drain();
}

gtars_status part_count_device(const PartDevice *d, const uint32_t *d_chrom, const uint32_t *d_start, const uint32_t *d_end,
                               uint64_t n, bool bp, uint64_t *out, uint8_t *d_assign, void *stream) {
    GT_TRY(check_call(d, n, bp, d_assign));
    std::fill(out, out + d->n_part + 1, 0);
    if (!n) return GTARS_OK;
    if (!d_chrom || !d_start || !d_end) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    GT_TRY(require_handle_device(d->device));
    StreamFrame fr((hipStream_t)stream);
    GT_TRY(count_on(fr, *d, d_chrom, d_start, d_end, n, nullptr, 0, bp, out, d_assign));
    return fr.drain();
}

}  // namespace gtars
