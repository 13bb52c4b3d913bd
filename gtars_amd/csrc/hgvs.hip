// hgvs.hip -- K20: the HGVS-to-VRS bridge on the device (gtars-vrs/src/hgvs/bridge.rs:625-913).  The expressions are parsed
// and their accessions looked up on the host (hgvs.cpp); what arrives here are the parsed rows as columns, the text they
// point into, the mapping tables of a bound transcript store (reftx.hip) and the packed assembly image of K12.
//
//   * k_hgvs_span, one lane per row: hgvs_span_one of hgvs_core.h, the same text the host path runs -- the one or two
//     position mappings (tx_map_one with K19's exon binary search), the span rule of the edit, the bounds check against the
//     chromosome's own length and the REF cross-check against the image.  It leaves the span, the ALT's length and how the
//     ALT is made; the lanes of a wave diverge on edit kind and strand only.
//   * the scan of kernels.hip over ref_len + alt_len, then the fill of byte_csr.h over HgvsRowSrc (profiled as
//     k_hgvs_fill), eight output bytes per lane: REF is the span
//     upper-cased, ALT the parsed alternate (read backwards through the complement on the reverse strand) or the span once
//     or twice.  A lane finds its row by search, so a megabase dup is spread over as many lanes as it has eighths.
//   * the columns go into vrs_run of K18 on the same stream, unchanged.  A row that failed is passed with chromosome id
//     2^32 - 1 and two empty alleles: K18 answers VRS_NO_CHROM, a zero interval and a zero digest for it without reading
//     anything, and writes its status into a column of its own; k_hgvs_merge folds that column into the bridge's status
//     only for rows the bridge passed.
#include <cstring>

#include "byte_csr.h"
#include "common.h"
#include "hgvs.h"
#include "image_call.h"
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

// a row of the CSR: REF | ALT of a row the bridge passed (hgvs_pool_byte)
struct HgvsRowSrc {
    HgvsGenome g;
    HgvsCols c;
    HgvsOut o;
    const u8 *seq, *alt;  // of the open row
    u64 start, ref_len, alt_len;
    u32 mode;
    __device__ __forceinline__ void open(u32 r) {
        // (a row with bytes passed the bridge: its chromosome id and its spans are valid)
        seq = g.seq_of(o.chrom[r]);
        alt = c.text + c.text_off[r] + c.alt_off[r];
        start = o.start[r], ref_len = o.ref_len[r], alt_len = o.alt_len[r], mode = o.mode[r];
    }
    __device__ __forceinline__ u32 byte(u64 k) const { return hgvs_pool_byte(seq, start, ref_len, alt_len, mode, alt, k); }
};

// K18's status reaches a row only where the bridge had none of its own
__global__ void __launch_bounds__(HG_TPB)
k_hgvs_merge(const u8 *__restrict__ vrs_status, u64 n, u8 *__restrict__ status, u8 *__restrict__ detail) {
    for (u64 i = (u64)blockIdx.x * HG_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * HG_TPB)
        if (status[i] == HGVS_OK && vrs_status[i] != VRS_OK) status[i] = HGVS_NORMALIZE_ERROR, detail[i] = vrs_status[i];
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
    GT_TRY(digests_aligned("hgvs", call.on_device, call.digest));
    if (call.on_device) GT_TRY(require_handle_device(ap.device));
    ImageCall ic(ap, call.on_device, call.stream);
    GT_TRY(ic.scope.st);
    StreamFrame &fr = ic.fr;
    hipStream_t st = fr.st;
    const size_t n = (size_t)in.n;

    HgvsCols c = in;
    GT_TRY(ic.in(in.pre, n, &c.pre));
    GT_TRY(ic.in(in.kind, n, &c.kind));
    GT_TRY(ic.in(in.loc, n, &c.loc));
    GT_TRY(ic.in(in.edit, n, &c.edit));
    GT_TRY(ic.in(in.flags, n, &c.flags));
    GT_TRY(ic.in(in.tx, n, &c.tx));
    GT_TRY(ic.in(in.base1, n, &c.base1));
    GT_TRY(ic.in(in.off1, n, &c.off1));
    GT_TRY(ic.in(in.base2, n, &c.base2));
    GT_TRY(ic.in(in.off2, n, &c.off2));
    GT_TRY(ic.in(in.text_off, n, &c.text_off));
    GT_TRY(ic.in(in.ref_off, n, &c.ref_off));
    GT_TRY(ic.in(in.ref_len, n, &c.ref_len));
    GT_TRY(ic.in(in.alt_off, n, &c.alt_off));
    GT_TRY(ic.in(in.alt_len, n, &c.alt_len));
    GT_TRY(ic.in(in.text, (size_t)in.text_bytes, &c.text));

    HgvsGenome g;
    g.seq = ap.seq, g.off = ap.off, g.len = ap.len, g.n_chrom = ap.n_chrom;
    HgvsOut o{};
    GT_TRY(ic.out(call.status, n, &o.status));
    GT_TRY(ic.out(call.detail, n, &o.detail));
    GT_TRY(ic.out(call.warnings, n, &o.warnings));
    GT_TRY(ic.out(call.chrom, n, &o.chrom));
    GT_TRY(fr.alloc(&o.mode, n));
    GT_TRY(fr.alloc(&o.ref_len, n));
    GT_TRY(fr.alloc(&o.alt_len, n));
    GT_TRY(fr.alloc(&o.cnt, n));
    GT_TRY(fr.alloc(&o.start, n));
    u32 *too_long, *h_too_long;
    GT_TRY(ic.host_word(&h_too_long));
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
    GT_TRY(csr_fill("k_hgvs_fill", HgvsRowSrc{g, c, o}, off, (u32)n, total, pool, st));
    // K18, on the same stream, over the columns as they lie on the device
    u8 *vrs_status;
    u64 *ns, *ne;
    u64 *digest = nullptr;
    GT_TRY(fr.alloc(&vrs_status, n));
    GT_TRY(ic.out(call.start, n, &ns));
    GT_TRY(ic.out(call.end, n, &ne));
    if (call.digest) GT_TRY(ic.digests_out(call.digest, n, &digest));
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
    GT_TRY(ic.back(call.status, o.status, n));
    GT_TRY(ic.back(call.detail, o.detail, n));
    GT_TRY(ic.back(call.warnings, o.warnings, n));
    GT_TRY(ic.back(call.chrom, o.chrom, n));
    GT_TRY(ic.back(call.start, ns, n));
    GT_TRY(ic.back(call.end, ne, n));
    GT_TRY(ic.digests_back(call.digest, digest, n));
    return fr.drain();
}

}  // namespace gtars
