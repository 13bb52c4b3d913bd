// hgvs.hip -- K20: the HGVS-to-VRS bridge on the device (gtars-vrs/src/hgvs/bridge.rs:625-913).  The expressions are parsed
// and their accessions looked up on the host (hgvs.cpp); what arrives here are the parsed rows as columns, the text they
// point into, the mapping tables of a bound transcript store (reftx.hip) and the packed assembly image of K12.
//
//   * k_hgvs_span, one lane per row: hgvs_span_one of hgvs_core.h, the same text the host path runs -- the one or two
//     position mappings (tx_map_one with K19's exon binary search), the span rule of the edit, the bounds check against the
//     chromosome's own length and the REF cross-check against the image.  It leaves the span, the ALT's length and how the
//     ALT is made; the lanes of a wave diverge on edit kind and strand only.
//   * the scan of kernels.hip over ref_len + alt_len, then k_hgvs_fill, eight output bytes per lane: REF is the span
//     upper-cased, ALT the parsed alternate (read backwards through the complement on the reverse strand) or the span once
//     or twice.  A lane finds its row by search, so a megabase dup is spread over as many lanes as it has eighths.
//   * the columns go into vrs_run of K18 on the same stream, unchanged.  A row that failed is passed with chromosome id
//     2^32 - 1 and two empty alleles: K18 answers VRS_NO_CHROM, a zero interval and a zero digest for it without reading
//     anything, and writes its status into a column of its own; k_hgvs_merge folds that column into the bridge's status
//     only for rows the bridge passed.
#include <cstring>

#include "common.h"
#include "hgvs.h"
#include "pipeline.h"
#include "vrs.h"
#include "vrs_core.h"

namespace gtars {

namespace {

constexpr int HG_TPB = 256;
constexpr u32 HG_MAX_BLOCKS = 256 * 8;
constexpr u64 HG_MAX_N = 0x7FFFFFF0u;
constexpr u64 HG_MAX_POOL = 0xFFFFFFF0ull;  // K18's offsets are u32

struct HgvsOut {  // per row
    u8 *status, *detail, *warnings, *mode;
    u32 *chrom, *ref_len, *alt_len, *cnt;
    u64 *start;
};

__global__ void __launch_bounds__(HG_TPB)
k_hgvs_span(TxTables t, HgvsGenome g, HgvsCols c, HgvsOut o, u32 *__restrict__ too_long) {
    for (u64 i = (u64)blockIdx.x * HG_TPB + threadIdx.x; i < c.n; i += (u64)gridDim.x * HG_TPB) {
        HgvsSpan r = hgvs_span_one(t, g, c, i);
        if (r.status == HGVS_OK && r.ref_len + r.alt_len > HG_MAX_POOL) {
            atomicOr(too_long, 1u);
            r.status = HGVS_OUT_OF_BOUNDS;  // (the call fails: nothing reads this)
        }
        const bool ok = r.status == HGVS_OK;
        o.status[i] = r.status, o.detail[i] = r.detail;
        o.warnings[i] = (c.flags[i] & HGVS_UNCERTAIN) ? (u8)HGVS_WARN_UNCERTAIN : (u8)0;
        o.mode[i] = r.mode;
        o.chrom[i] = ok ? r.chrom : TX_NONE;
        o.start[i] = ok ? r.start : 0;
        o.ref_len[i] = ok ? (u32)r.ref_len : 0u;
        o.alt_len[i] = ok ? (u32)r.alt_len : 0u;
        o.cnt[i] = ok ? (u32)(r.ref_len + r.alt_len) : 0u;
    }
}

// K18's offset columns from the scan
__global__ void __launch_bounds__(HG_TPB)
k_hgvs_offsets(const u64 *__restrict__ off, const u32 *__restrict__ ref_len, u64 n, u32 *__restrict__ ref_off, u32 *__restrict__ alt_off) {
    for (u64 i = (u64)blockIdx.x * HG_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * HG_TPB) {
        ref_off[i] = (u32)off[i];
        alt_off[i] = (u32)(off[i] + ref_len[i]);
    }
}

__global__ void __launch_bounds__(HG_TPB)
k_hgvs_fill(HgvsGenome g, HgvsCols c, HgvsOut o, const u64 *__restrict__ off, u64 total, u8 *__restrict__ out) {
    const u64 groups = (total + 7) >> 3;
    const u32 n = (u32)c.n;
    for (u64 grp = (u64)blockIdx.x * HG_TPB + threadIdx.x; grp < groups; grp += (u64)gridDim.x * HG_TPB) {
        const u64 q0 = grp << 3;
        const u64 q_end = min(q0 + 8, total);
        // the row of byte q0: the last r with off[r] <= q0, which is the one with bytes among those that share the offset
        u32 lo = 0, hi = n;
        while (hi - lo > 1) {
            const u32 m = lo + ((hi - lo) >> 1);
            if (off[m] <= q0) lo = m;
            else hi = m;
        }
        u32 r = lo;
        bool new_row = true;
        const u8 *seq = nullptr, *alt = nullptr;
        u64 start = 0, ref_len = 0, alt_len = 0, word = 0;
        u32 mode = 0;
        for (u64 q = q0; q < q_end; ++q) {
            while (off[r + 1] <= q) ++r, new_row = true;  // (q < total = off[n]: stops inside the table)
            if (new_row) {
                // (a row with bytes passed the bridge: its chromosome id and its spans are valid)
                seq = g.seq_of(o.chrom[r]);
                alt = c.text + c.text_off[r] + c.alt_off[r];
                start = o.start[r], ref_len = o.ref_len[r], alt_len = o.alt_len[r], mode = o.mode[r];
                new_row = false;
            }
            word |= (u64)hgvs_pool_byte(seq, start, ref_len, alt_len, mode, alt, q - off[r]) << (8 * (q - q0));
        }
        if (q_end - q0 == 8) *(u64 *)(out + q0) = word;  // (out comes from the allocator and q0 is a multiple of 8)
        else
            for (u64 q = q0; q < q_end; ++q) out[q] = (u8)(word >> (8 * (q - q0)));
    }
}

// K18's status reaches a row only where the bridge had none of its own
__global__ void __launch_bounds__(HG_TPB)
k_hgvs_merge(const u8 *__restrict__ vrs_status, u64 n, u8 *__restrict__ status, u8 *__restrict__ detail) {
    for (u64 i = (u64)blockIdx.x * HG_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * HG_TPB)
        if (status[i] == HGVS_OK && vrs_status[i] != VRS_OK) status[i] = HGVS_NORMALIZE_ERROR, detail[i] = vrs_status[i];
}

template <class T>
gtars_status bring(StreamFrame &fr, bool on_device, const T *src, size_t n, const T **out) {
    if (on_device) {
        *out = src;
        return GTARS_OK;
    }
    T *d;
    GT_TRY(fr.upload(&d, src, n));
    *out = d;
    return GTARS_OK;
}

// the caller's device column, or one of the frame's
template <class T>
gtars_status column(StreamFrame &fr, bool on_device, T *given, size_t n, T **out) {
    if (on_device && given) {
        *out = given;
        return GTARS_OK;
    }
    return fr.alloc(out, n);
}

}  // namespace

gtars_status hgvs_run(const Assembly &a, const TxDevice &d, const HgvsCall &call) {
    const AssemblyParts ap = assembly_parts(a);
    if (ap.device < 0) return fail(GTARS_ERR_INTERNAL, "hgvs: the assembly has no device image");
    const HgvsCols &in = call.cols;
    if (in.n > HG_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "hgvs: too many rows (" + std::to_string(in.n) + ")");
    if (!in.n) return GTARS_OK;
    if (!in.pre || !in.kind || !in.loc || !in.edit || !in.flags || !in.tx || !in.base1 || !in.off1 || !in.base2 || !in.off2 || !in.text_off ||
        !in.ref_off || !in.ref_len || !in.alt_off || !in.alt_len || (!in.text && in.text_bytes) || !call.accessions)
        return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    if (call.on_device) {
        if (call.digest && ((uintptr_t)call.digest & 7)) return fail(GTARS_ERR_INVALID_ARG, "hgvs: the device digests must be 8-byte aligned");
        int cur = -1;
        GT_HIP(hipGetDevice(&cur));
        if (cur != ap.device)
            return fail(GTARS_ERR_INVALID_ARG, "handle lives on device " + std::to_string(ap.device) + ", current device is " +
                                                   std::to_string(cur) + ": device pointers and stream must belong to the handle's device");
    }
    DeviceScope on(call.on_device ? -1 : ap.device);
    GT_TRY(on.st);
    StreamFrame fr(call.on_device ? (hipStream_t)call.stream : nullptr);
    hipStream_t st = fr.st;
    const size_t n = (size_t)in.n;
    const bool dev = call.on_device;

    HgvsCols c = in;
    GT_TRY(bring(fr, dev, in.pre, n, &c.pre));
    GT_TRY(bring(fr, dev, in.kind, n, &c.kind));
    GT_TRY(bring(fr, dev, in.loc, n, &c.loc));
    GT_TRY(bring(fr, dev, in.edit, n, &c.edit));
    GT_TRY(bring(fr, dev, in.flags, n, &c.flags));
    GT_TRY(bring(fr, dev, in.tx, n, &c.tx));
    GT_TRY(bring(fr, dev, in.base1, n, &c.base1));
    GT_TRY(bring(fr, dev, in.off1, n, &c.off1));
    GT_TRY(bring(fr, dev, in.base2, n, &c.base2));
    GT_TRY(bring(fr, dev, in.off2, n, &c.off2));
    GT_TRY(bring(fr, dev, in.text_off, n, &c.text_off));
    GT_TRY(bring(fr, dev, in.ref_off, n, &c.ref_off));
    GT_TRY(bring(fr, dev, in.ref_len, n, &c.ref_len));
    GT_TRY(bring(fr, dev, in.alt_off, n, &c.alt_off));
    GT_TRY(bring(fr, dev, in.alt_len, n, &c.alt_len));
    GT_TRY(bring(fr, dev, in.text, (size_t)in.text_bytes, &c.text));

    HgvsGenome g;
    g.seq = ap.seq, g.off = ap.off, g.len = ap.len, g.n_chrom = ap.n_chrom;
    HgvsOut o{};
    GT_TRY(column(fr, dev, call.status, n, &o.status));
    GT_TRY(column(fr, dev, call.detail, n, &o.detail));
    GT_TRY(column(fr, dev, call.warnings, n, &o.warnings));
    GT_TRY(column(fr, dev, call.chrom, n, &o.chrom));
    GT_TRY(fr.alloc(&o.mode, n));
    GT_TRY(fr.alloc(&o.ref_len, n));
    GT_TRY(fr.alloc(&o.alt_len, n));
    GT_TRY(fr.alloc(&o.cnt, n));
    GT_TRY(fr.alloc(&o.start, n));
    u32 *too_long, *h_too_long = (u32 *)fr.host(sizeof(u32));
    if (!h_too_long) return fail(GTARS_ERR_INTERNAL, "out of host memory");
    GT_TRY(fr.alloc(&too_long, 1));
    GT_HIP(hipMemsetAsync(too_long, 0, sizeof(u32), st));
    const unsigned grid = grid_for(n, HG_TPB, HG_MAX_BLOCKS);
    {
        ProfScope ps("k_hgvs_span", st);
        hipLaunchKernelGGL(k_hgvs_span, dim3(grid), dim3(HG_TPB), 0, st, tx_device_view(d), g, c, o, too_long);
        GT_HIP(hipGetLastError());
    }
    GT_TRY(fr.download(h_too_long, too_long, 1));
    u64 *off, total = 0;
    GT_TRY(scan_total(fr, o.cnt, n, &off, &total));
    if (*h_too_long || total > HG_MAX_POOL) return fail(GTARS_ERR_CAPACITY, "hgvs: the alleles of one call must fit 4 GiB; split the batch");
    u8 *pool;
    u32 *ref_off, *alt_off;
    GT_TRY(fr.alloc(&pool, (size_t)total));
    GT_TRY(fr.alloc(&ref_off, n));
    GT_TRY(fr.alloc(&alt_off, n));
    {
        ProfScope ps("k_hgvs_offsets", st);
        hipLaunchKernelGGL(k_hgvs_offsets, dim3(grid), dim3(HG_TPB), 0, st, off, o.ref_len, (u64)n, ref_off, alt_off);
        GT_HIP(hipGetLastError());
    }
    if (total) {
        ProfScope ps("k_hgvs_fill", st);
        hipLaunchKernelGGL(k_hgvs_fill, dim3(grid_for((total + 7) >> 3, HG_TPB, HG_MAX_BLOCKS)), dim3(HG_TPB), 0, st, g, c, o, off, total, pool);
        GT_HIP(hipGetLastError());
    }
    // K18, on the same stream, over the columns as they lie on the device
    u8 *vrs_status;
    u64 *ns, *ne;
    u64 *digest = nullptr;
    GT_TRY(fr.alloc(&vrs_status, n));
    GT_TRY(column(fr, dev, call.start, n, &ns));
    GT_TRY(column(fr, dev, call.end, n, &ne));
    if (call.digest) {
        if (dev) digest = (u64 *)call.digest;
        else GT_TRY(fr.alloc(&digest, 4 * n));
    }
    VrsCall v;
    v.chrom = o.chrom, v.start = o.start, v.pool = pool, v.pool_bytes = total;
    v.ref_off = ref_off, v.ref_len = o.ref_len, v.alt_off = alt_off, v.alt_len = o.alt_len, v.n = n;
    v.on_device = true, v.stream = st;
    v.accessions = call.accessions, v.h_seq = call.h_seq, v.threads = call.threads;
    v.status = vrs_status, v.new_start = ns, v.new_end = ne, v.digest = (char *)digest;
    GT_TRY(vrs_run(a, v));
    {
        ProfScope ps("k_hgvs_merge", st);
        hipLaunchKernelGGL(k_hgvs_merge, dim3(grid), dim3(HG_TPB), 0, st, vrs_status, (u64)n, o.status, o.detail);
        GT_HIP(hipGetLastError());
    }
    if (!dev) {
        if (call.status) GT_TRY(fr.download(call.status, o.status, n));
        if (call.detail) GT_TRY(fr.download(call.detail, o.detail, n));
        if (call.warnings) GT_TRY(fr.download(call.warnings, o.warnings, n));
        if (call.chrom) GT_TRY(fr.download(call.chrom, o.chrom, n));
        if (call.start) GT_TRY(fr.download(call.start, ns, n));
        if (call.end) GT_TRY(fr.download(call.end, ne, n));
        if (call.digest) GT_TRY(fr.download(call.digest, (const char *)digest, 32 * n));
    }
    return fr.drain();
}

}  // namespace gtars
