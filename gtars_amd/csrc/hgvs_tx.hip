// hgvs_tx.hip -- K23: the transcript-anchored HGVS-to-VRS bridge on the device (gtars-vrs/src/hgvs/bridge.rs:226-534) and the
// layer under it, alleles on transcripts.  The allele lies on the transcript's own mature mRNA, whose refget accession
// ("SQ." + sha512t24u of the derived sequence) anchors the identifier; coordinates, REF, ALT and the normalization are in
// mRNA space.  The rows arrive as for K20 (hgvs.hip): parsed and resolved on the host, as columns.
//
//   * k_hgvs_tx_span, one lane per row: hgvs_tx_span_one of hgvs_tx_core.h, the same text the host path runs -- each
//     position c./n. -> genomic (tx_map_one, intronic offsets included) and back onto the mRNA (tx_map_one, kind G), the span
//     rule of the edit in transcript space, the transcript's sequence status, the bounds against the transcript's length
//     and the REF cross-check against the mRNA's bytes, read through the exons.
//   * the mRNA image of the call: k_tx_flag marks the transcripts that have a passing row, the scan of kernels.hip turns the
//     marks into slots, k_tx_slots lists them, the fill of K19 (TxRowSrc, profiled as k_hgvs_tx_image) writes their mature
//     mRNAs back to back and k_tx_digest hashes them: the image, its u64 offsets and lengths and a device-resident accession
//     table indexed by slot.  It is built per call from the rows' transcripts only, and dropped with the call.
//   * the REF | ALT pool from that image (the fill of byte_csr.h over HgvsTxRowSrc, profiled as k_hgvs_tx_fill), eight
//     output bytes per lane: REF is the span, ALT the parsed alternate as written or the span once or twice.
//   * K18 over the image (vrs_run_view): "chromosome" = slot.  Its rolls are bounded by 0 and the sequence's own length, so
//     they cross exon junctions and stop at the transcript's ends whatever the neighbouring slots hold.  Alleles above
//     GTARS_VRS_HOST_LEN finish on the host threads from mRNAs derived there for just those transcripts.
//   * k_hgvs_tx_merge folds K18's status into the bridge's with the rule of k_hgvs_merge and hands every row that passed
//     its anchor's digest.
#include <cstring>
#include <string>
#include <unordered_map>

#include "byte_csr.h"
#include "common.h"
#include "hgvs.h"
#include "hgvs_tx_core.h"
#include "host_threads.h"
#include "image_call.h"
#include "pipeline.h"
#include "reftx_image.h"
#include "vrs.h"
#include "vrs_core.h"

namespace gtars {

namespace {

constexpr int HT_TPB = 256;
constexpr u64 HT_MAX_N = 0x7FFFFFF0u;
constexpr u64 HT_MAX_POOL = 0xFFFFFFF0ull;  // K18's offsets are u32

// Every kernel of this file does a few loads and stores per row, so each is launched with exactly one lane per row
// (n <= HT_MAX_N: at most 2^23 workgroups) and has no loop over rows; the byte-heavy steps are the fills and K18.
inline unsigned rows_grid(u64 n) { return (unsigned)((n + HT_TPB - 1) / HT_TPB); }

struct HgvsTxOut {  // per row
    u8 *status, *detail, *warnings, *mode;
    u32 *tx, *ref_len, *alt_len, *cnt;
    u64 *start;
};

__global__ void __launch_bounds__(HT_TPB)
k_hgvs_tx_span(TxTables t, HgvsGenome g, HgvsCols c, HgvsTxOut o, u32 *__restrict__ too_long) {
    const u64 i = (u64)blockIdx.x * HT_TPB + threadIdx.x;
    if (i < c.n) {
        HgvsTxSpan r = hgvs_tx_span_one(t, g, c, i);
        if (r.status == HGVS_OK && r.ref_len + r.alt_len > HT_MAX_POOL) {
            atomicOr(too_long, 1u);
            r.status = HGVS_OUT_OF_BOUNDS;  // (the call fails: nothing reads this)
        }
        const bool ok = r.status == HGVS_OK;
        o.status[i] = r.status, o.detail[i] = r.detail;
        o.warnings[i] = (c.flags[i] & HGVS_UNCERTAIN) ? (u8)HGVS_WARN_UNCERTAIN : (u8)0;
        o.mode[i] = r.mode;
        o.tx[i] = ok ? r.tx : TX_NONE;
        o.start[i] = ok ? r.start : 0;
        o.ref_len[i] = ok ? (u32)r.ref_len : 0u;
        o.alt_len[i] = ok ? (u32)r.alt_len : 0u;
        o.cnt[i] = ok ? (u32)(r.ref_len + r.alt_len) : 0u;
    }
}

// the transcript of an allele row that can have a sequence, TX_NONE otherwise
__global__ void __launch_bounds__(HT_TPB) k_tx_allele_rows(TxTables t, const u32 *__restrict__ tx, u64 n, u32 *__restrict__ tx_row) {
    const u64 i = (u64)blockIdx.x * HT_TPB + threadIdx.x;
    if (i < n) {
        const u32 x = tx[i];
        tx_row[i] = x < t.n_tx && t.seq_status[x] == TXSEQ_OK ? x : TX_NONE;
    }
}

// flag[tx] = 1 for every transcript a row names (the rows of one transcript all store the same word)
__global__ void __launch_bounds__(HT_TPB) k_tx_flag(const u32 *__restrict__ tx_row, u64 n, u32 n_tx, u32 *__restrict__ flag) {
    const u64 i = (u64)blockIdx.x * HT_TPB + threadIdx.x;
    if (i < n) {
        const u32 x = tx_row[i];
        if (x < n_tx) flag[x] = 1u;
    }
}

// the slot list: slot_of is the scan of the flags
__global__ void __launch_bounds__(HT_TPB)
k_tx_slots(TxTables t, const u32 *__restrict__ flag, const u64 *__restrict__ slot_of, u32 *__restrict__ slot_tx, u32 *__restrict__ slot_cnt,
           u64 *__restrict__ slot_len) {
    const u64 x = (u64)blockIdx.x * HT_TPB + threadIdx.x;
    if (x < t.n_tx && flag[x]) {
        const u64 s = slot_of[x];
        slot_tx[s] = (u32)x, slot_cnt[s] = t.len[x], slot_len[s] = t.len[x];
    }
}

// K18's "chromosome" column: the slot of the row's transcript
__global__ void __launch_bounds__(HT_TPB)
k_tx_row_slots(const u32 *__restrict__ tx_row, const u64 *__restrict__ slot_of, u32 n_tx, u64 n, u32 *__restrict__ slot) {
    const u64 i = (u64)blockIdx.x * HT_TPB + threadIdx.x;
    if (i < n) {
        const u32 x = tx_row[i];
        slot[i] = x < n_tx ? (u32)slot_of[x] : TX_NONE;
    }
}

// K18's offset columns from the scan
__global__ void __launch_bounds__(HT_TPB)
k_hgvs_tx_offsets(const u64 *__restrict__ off, const u32 *__restrict__ ref_len, u64 n, u32 *__restrict__ ref_off, u32 *__restrict__ alt_off) {
    const u64 i = (u64)blockIdx.x * HT_TPB + threadIdx.x;
    if (i < n) {
        ref_off[i] = (u32)off[i];
        alt_off[i] = (u32)(off[i] + ref_len[i]);
    }
}

// a row of the CSR: REF | ALT of a row the bridge passed (hgvs_tx_pool_byte), from the mRNA image
struct HgvsTxRowSrc {
    const u8 *image;
    const u64 *img_off;
    const u32 *slot;
    HgvsCols c;
    HgvsTxOut o;
    const u8 *mrna, *alt;  // of the open row
    u64 start, ref_len;
    u32 mode;
    __device__ __forceinline__ void open(u32 r) {
        // (a row with bytes passed the bridge: its slot and its span are valid)
        mrna = image + img_off[slot[r]];
        alt = c.text + c.text_off[r] + c.alt_off[r];
        start = o.start[r], ref_len = o.ref_len[r], mode = o.mode[r];
    }
    __device__ __forceinline__ u32 byte(u64 k) const { return hgvs_tx_pool_byte(mrna, start, ref_len, mode, alt, k); }
};

__device__ __forceinline__ void anchor_of(bool ok, const u64 *__restrict__ acc, u32 slot, u64 *__restrict__ dst) {
    if (ok) {  // (only then is `slot` one of the image's)
        const u64 *src = acc + (u64)slot * 4;
        dst[0] = src[0], dst[1] = src[1], dst[2] = src[2], dst[3] = src[3];
    } else {
        dst[0] = dst[1] = dst[2] = dst[3] = 0;
    }
}

// K18's status reaches a row only where the bridge had none of its own (k_hgvs_merge's rule); a row that is still fine gets
// its anchor
__global__ void __launch_bounds__(HT_TPB)
k_hgvs_tx_merge(const u8 *__restrict__ vrs_status, const u32 *__restrict__ slot, const u64 *__restrict__ acc, u64 n, u8 *__restrict__ status,
                u8 *__restrict__ detail, u64 *__restrict__ anchor) {
    const u64 i = (u64)blockIdx.x * HT_TPB + threadIdx.x;
    if (i < n) {
        if (status[i] == HGVS_OK && vrs_status[i] != VRS_OK) status[i] = HGVS_NORMALIZE_ERROR, detail[i] = vrs_status[i];
        if (anchor) anchor_of(status[i] == HGVS_OK, acc, slot[i], anchor + i * 4);
    }
}

__global__ void __launch_bounds__(HT_TPB)
k_tx_anchor(const u8 *__restrict__ vrs_status, const u32 *__restrict__ slot, const u64 *__restrict__ acc, u64 n, u64 *__restrict__ anchor) {
    const u64 i = (u64)blockIdx.x * HT_TPB + threadIdx.x;
    if (i < n) anchor_of(vrs_status[i] == VRS_OK, acc, slot[i], anchor + i * 4);
}

// the mRNA image of one call; every pointer is the frame's device memory
struct TxImage {
    u32 n_slots = 0;
    u64 *slot_of = nullptr;  // [n_tx + 1]
    u32 *slot_tx = nullptr;  // [n_slots]
    u64 *off = nullptr, *len = nullptr;
    u8 *bytes = nullptr;
    u64 total = 0;
    u64 *acc = nullptr;  // [n_slots * 4]: 32 digest characters per slot
    u32 *slot = nullptr; // [n rows]
};

// tx_row[i]: the transcript row i lies on, TX_NONE for a row that takes no part
gtars_status tx_image_build(StreamFrame &fr, const AssemblyParts &ap, const TxTables &t, const u32 *tx_row, size_t n, const TxHostSide &host,
                            TxImage *im) {
    hipStream_t st = fr.st;
    const unsigned grid = rows_grid(n);
    u64 n_slots = 0;
    u32 *flag = nullptr;
    if (t.n_tx) {
        GT_TRY(fr.alloc(&flag, (size_t)t.n_tx));
        GT_HIP(hipMemsetAsync(flag, 0, (size_t)t.n_tx * sizeof(u32), st));
        {
            ProfScope ps("k_tx_flag", st);
            hipLaunchKernelGGL(k_tx_flag, dim3(grid), dim3(HT_TPB), 0, st, tx_row, (u64)n, t.n_tx, flag);
            GT_HIP(hipGetLastError());
        }
        GT_TRY(scan_total(fr, flag, t.n_tx, &im->slot_of, &n_slots));
    } else {
        GT_TRY(fr.alloc(&im->slot_of, 1));
    }
    im->n_slots = (u32)n_slots;
    u32 *slot_cnt;
    GT_TRY(fr.alloc(&im->slot_tx, (size_t)n_slots));
    GT_TRY(fr.alloc(&slot_cnt, (size_t)n_slots));
    GT_TRY(fr.alloc(&im->len, (size_t)n_slots));
    GT_TRY(fr.alloc(&im->acc, (size_t)n_slots * 4));
    GT_TRY(fr.alloc(&im->slot, n));
    if (n_slots) {
        {
            ProfScope ps("k_tx_slots", st);
            hipLaunchKernelGGL(k_tx_slots, dim3(rows_grid(t.n_tx)), dim3(HT_TPB), 0, st, t, flag, im->slot_of, im->slot_tx,
                               slot_cnt, im->len);
            GT_HIP(hipGetLastError());
        }
        GT_TRY(scan_total(fr, slot_cnt, n_slots, &im->off, &im->total));
        GT_TRY(fr.alloc(&im->bytes, (size_t)im->total));
        GT_TRY(tx_fill_rows("k_hgvs_tx_image", fr, ap, t, im->slot_tx, im->off, im->n_slots, im->total, im->bytes));
        u8 *slot_status;  // every slot's transcript has a sequence
        GT_TRY(fr.alloc(&slot_status, (size_t)n_slots));
        GT_HIP(hipMemsetAsync(slot_status, TXSEQ_OK, (size_t)n_slots, st));
        GT_TRY(tx_digest_rows(fr, ap, t, im->slot_tx, slot_cnt, slot_status, im->n_slots, im->acc, host.h_tables, host.h_seq, host.threads));
    } else {
        GT_TRY(fr.alloc(&im->off, 1));
        GT_TRY(fr.alloc(&im->bytes, 0));
    }
    {
        ProfScope ps("k_tx_row_slots", st);
        hipLaunchKernelGGL(k_tx_row_slots, dim3(grid), dim3(HT_TPB), 0, st, tx_row, im->slot_of, t.n_tx, (u64)n, im->slot);
        GT_HIP(hipGetLastError());
    }
    return GTARS_OK;
}

// K18's host tail over an image: the mRNAs of just the listed slots, derived on the host, and their accessions
struct TxImageHost {
    StreamFrame &fr;
    const TxImage &im;
    const TxHostSide &host;
    std::vector<std::string> mrna;
    std::vector<char> acc;
    gtars_status operator()(const std::vector<uint32_t> &ids, std::vector<const uint8_t *> &seq, std::vector<const char *> &out_acc) {
        if (!host.h_tables || !host.h_seq) return fail(GTARS_ERR_INTERNAL, "hgvs: the host tail needs the host tables");
        std::unordered_map<u32, size_t> at;  // slot -> its place in the lists
        std::vector<u32> slots;
        for (const u32 s : ids)
            if (at.emplace(s, slots.size()).second) slots.push_back(s);
        std::vector<u32> txs(slots.size());
        acc.assign(slots.size() * 32, '\0');
        for (size_t k = 0; k < slots.size(); ++k) {
            GT_TRY(fr.download(&txs[k], im.slot_tx + slots[k], 1));
            GT_TRY(fr.download(&acc[k * 32], (const char *)(im.acc + 4 * (size_t)slots[k]), 32));
        }
        GT_TRY(fr.drain());
        mrna.assign(slots.size(), std::string());
        const TxTables &h = *host.h_tables;
        parallel_for(slots.size(), host.threads, 1, [&](size_t k) {
            const u32 tx = txs[k];
            tx_sequence(h, tx, h.len[tx] ? host.h_seq[h.chrom[tx]] : nullptr, mrna[k]);
        });
        for (const u32 s : ids) {
            const size_t k = at[s];
            seq.push_back((const uint8_t *)mrna[k].data()), out_acc.push_back(&acc[k * 32]);
        }
        return GTARS_OK;
    }
};

VrsSeqView view_of(const AssemblyParts &ap, const TxImage &im, TxImageHost &tail) {
    VrsSeqView sv;
    sv.device = ap.device, sv.seq = im.bytes, sv.off = im.off, sv.len = im.len, sv.n_seq = im.n_slots, sv.d_acc = (const u8 *)im.acc;
    sv.host_tail = [&tail](const std::vector<uint32_t> &ids, std::vector<const uint8_t *> &seq, std::vector<const char *> &acc) {
        return tail(ids, seq, acc);
    };
    return sv;
}

}  // namespace

gtars_status hgvs_tx_run(const Assembly &a, const TxDevice &d, const HgvsTxCall &call) {
    const AssemblyParts ap = assembly_parts(a);
    if (ap.device < 0) return fail(GTARS_ERR_INTERNAL, "hgvs: the assembly has no device image");
    const HgvsCols &in = call.cols;
    if (in.n > HT_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "hgvs: too many rows (" + std::to_string(in.n) + ")");
    if (!in.n) return GTARS_OK;
    if (!in.pre || !in.kind || !in.loc || !in.edit || !in.flags || !in.tx || !in.base1 || !in.off1 || !in.base2 || !in.off2 || !in.text_off ||
        !in.ref_off || !in.ref_len || !in.alt_off || !in.alt_len || (!in.text && in.text_bytes))
        return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    GT_TRY(digests_aligned("hgvs", call.on_device, call.digest));
    GT_TRY(digests_aligned("hgvs", call.on_device, call.anchor));
    if (call.on_device) GT_TRY(require_handle_device(ap.device));
    ImageCall ic(ap, call.on_device, call.stream);
    GT_TRY(ic.scope.st);
    StreamFrame &fr = ic.fr;
    hipStream_t st = fr.st;
    const size_t n = (size_t)in.n;
    const TxTables t = tx_device_view(d);

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
    HgvsTxOut o{};
    GT_TRY(ic.out(call.status, n, &o.status));
    GT_TRY(ic.out(call.detail, n, &o.detail));
    GT_TRY(ic.out(call.warnings, n, &o.warnings));
    GT_TRY(ic.out(call.tx, n, &o.tx));
    GT_TRY(fr.alloc(&o.mode, n));
    GT_TRY(fr.alloc(&o.ref_len, n));
    GT_TRY(fr.alloc(&o.alt_len, n));
    GT_TRY(fr.alloc(&o.cnt, n));
    GT_TRY(fr.alloc(&o.start, n));
    u32 *too_long, *h_too_long;
    GT_TRY(ic.host_word(&h_too_long));
    GT_TRY(fr.alloc(&too_long, 1));
    GT_HIP(hipMemsetAsync(too_long, 0, sizeof(u32), st));
    const unsigned grid = rows_grid(n);
    {
        ProfScope ps("k_hgvs_tx_span", st);
        hipLaunchKernelGGL(k_hgvs_tx_span, dim3(grid), dim3(HT_TPB), 0, st, t, g, c, o, too_long);
        GT_HIP(hipGetLastError());
    }
    GT_TRY(fr.download(h_too_long, too_long, 1));
    u64 *off, total = 0;
    GT_TRY(scan_total(fr, o.cnt, n, &off, &total));
    if (*h_too_long || total > HT_MAX_POOL) return fail(GTARS_ERR_CAPACITY, "hgvs: the alleles of one call must fit 4 GiB; split the batch");
    // the mature mRNAs of the transcripts that have a passing row
    TxImage im;
    GT_TRY(tx_image_build(fr, ap, t, o.tx, n, call.host, &im));
    u8 *pool;
    u32 *ref_off, *alt_off;
    GT_TRY(fr.alloc(&pool, (size_t)total));
    GT_TRY(fr.alloc(&ref_off, n));
    GT_TRY(fr.alloc(&alt_off, n));
    {
        ProfScope ps("k_hgvs_tx_offsets", st);
        hipLaunchKernelGGL(k_hgvs_tx_offsets, dim3(grid), dim3(HT_TPB), 0, st, off, o.ref_len, (u64)n, ref_off, alt_off);
        GT_HIP(hipGetLastError());
    }
    GT_TRY(csr_fill("k_hgvs_tx_fill", HgvsTxRowSrc{im.bytes, im.off, im.slot, c, o}, off, (u32)n, total, pool, st));
    // K18 over the image, on the same stream: "chromosome" = slot
    u8 *vrs_status;
    u64 *ns, *ne, *digest = nullptr, *anchor = nullptr;
    GT_TRY(fr.alloc(&vrs_status, n));
    GT_TRY(ic.out(call.start, n, &ns));
    GT_TRY(ic.out(call.end, n, &ne));
    if (call.digest) GT_TRY(ic.digests_out(call.digest, n, &digest));
    if (call.anchor) GT_TRY(ic.digests_out(call.anchor, n, &anchor));
    TxImageHost tail{fr, im, call.host};
    VrsCall v;
    v.chrom = im.slot, v.start = o.start, v.pool = pool, v.pool_bytes = total;
    v.ref_off = ref_off, v.ref_len = o.ref_len, v.alt_off = alt_off, v.alt_len = o.alt_len, v.n = n;
    v.on_device = true, v.stream = st, v.threads = call.host.threads;
    v.status = vrs_status, v.new_start = ns, v.new_end = ne, v.digest = (char *)digest;
    GT_TRY(vrs_run_view(view_of(ap, im, tail), v));
    {
        ProfScope ps("k_hgvs_tx_merge", st);
        hipLaunchKernelGGL(k_hgvs_tx_merge, dim3(grid), dim3(HT_TPB), 0, st, vrs_status, im.slot, im.acc, (u64)n, o.status, o.detail, anchor);
        GT_HIP(hipGetLastError());
    }
    GT_TRY(ic.back(call.status, o.status, n));
    GT_TRY(ic.back(call.detail, o.detail, n));
    GT_TRY(ic.back(call.warnings, o.warnings, n));
    GT_TRY(ic.back(call.tx, o.tx, n));
    GT_TRY(ic.back(call.start, ns, n));
    GT_TRY(ic.back(call.end, ne, n));
    GT_TRY(ic.digests_back(call.digest, digest, n));
    GT_TRY(ic.digests_back(call.anchor, anchor, n));
    return fr.drain();
}

gtars_status vrs_tx_run(const Assembly &a, const TxDevice &d, const VrsTxCall &call) {
    const AssemblyParts ap = assembly_parts(a);
    if (ap.device < 0) return fail(GTARS_ERR_INTERNAL, "vrs: the assembly has no device image");
    if (call.n > HT_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "vrs: too many alleles (" + std::to_string(call.n) + ")");
    if (!call.n) return GTARS_OK;
    if (!call.tx || !call.start || !call.ref_off || !call.ref_len || !call.alt_off || !call.alt_len || (!call.pool && call.pool_bytes))
        return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    GT_TRY(digests_aligned("vrs", call.on_device, call.digest));
    GT_TRY(digests_aligned("vrs", call.on_device, call.anchor));
    if (call.on_device) GT_TRY(require_handle_device(ap.device));
    ImageCall ic(ap, call.on_device, call.stream);
    GT_TRY(ic.scope.st);
    StreamFrame &fr = ic.fr;
    hipStream_t st = fr.st;
    const size_t n = (size_t)call.n;
    const TxTables t = tx_device_view(d);
    const unsigned grid = rows_grid(n);
    // the columns once on the device: K18 below takes them as they lie there
    VrsCall v;
    GT_TRY(ic.in(call.start, n, &v.start));
    GT_TRY(ic.in(call.ref_off, n, &v.ref_off));
    GT_TRY(ic.in(call.ref_len, n, &v.ref_len));
    GT_TRY(ic.in(call.alt_off, n, &v.alt_off));
    GT_TRY(ic.in(call.alt_len, n, &v.alt_len));
    GT_TRY(ic.in(call.pool, (size_t)call.pool_bytes, &v.pool));
    v.pool_bytes = call.pool_bytes, v.n = n;
    const u32 *tx;
    u32 *tx_row;
    GT_TRY(ic.in(call.tx, n, &tx));
    GT_TRY(fr.alloc(&tx_row, n));
    {
        ProfScope ps("k_tx_allele_rows", st);
        hipLaunchKernelGGL(k_tx_allele_rows, dim3(grid), dim3(HT_TPB), 0, st, t, tx, (u64)n, tx_row);
        GT_HIP(hipGetLastError());
    }
    TxImage im;
    GT_TRY(tx_image_build(fr, ap, t, tx_row, n, call.host, &im));
    u8 *status;
    u64 *ns, *ne, *digest = nullptr, *anchor = nullptr;
    GT_TRY(ic.out(call.status, n, &status));
    GT_TRY(ic.out(call.new_start, n, &ns));
    GT_TRY(ic.out(call.new_end, n, &ne));
    if (call.digest) GT_TRY(ic.digests_out(call.digest, n, &digest));
    if (call.anchor) GT_TRY(ic.digests_out(call.anchor, n, &anchor));
    TxImageHost tail{fr, im, call.host};
    v.chrom = im.slot;
    v.on_device = true, v.stream = st, v.threads = call.host.threads;
    v.status = status, v.new_start = ns, v.new_end = ne, v.digest = (char *)digest;
    GT_TRY(vrs_run_view(view_of(ap, im, tail), v));
    if (anchor) {
        ProfScope ps("k_tx_anchor", st);
        hipLaunchKernelGGL(k_tx_anchor, dim3(grid), dim3(HT_TPB), 0, st, status, im.slot, im.acc, (u64)n, anchor);
        GT_HIP(hipGetLastError());
    }
    GT_TRY(ic.back(call.status, status, n));
    GT_TRY(ic.back(call.new_start, ns, n));
    GT_TRY(ic.back(call.new_end, ne, n));
    GT_TRY(ic.digests_back(call.digest, digest, n));
    GT_TRY(ic.digests_back(call.anchor, anchor, n));
    return fr.drain();
}

}  // namespace gtars
