// vrs.hip -- K18: GA4GH VRS allele identifiers over a genome assembly that is resident on the device
// (gtars-vrs/src/vcf_core.rs:126-189: per ALT allele normalize_ref, normalize.rs:362-441, then two SHA-512 digests of
// short canonical JSON texts, digest.rs:52-86).  Every allele is independent; the assembly is the packed image of K12
// (seqstats.h: the bytes as the file has them, read here through to_upper).
//
//   * k_vrs_normalize, one lane per allele: the bounds checks, REF validation, trim_left, trim_right, then roll_left and
//     roll_right with running circular indices.  A lane rolls at most GTARS_VRS_ROLL_CAP steps per direction; a roll that
//     is still matching there goes on a work list as (allele, direction).
//   * k_vrs_roll_long, one wave per list entry: 64 steps at a time, every lane one base, a ballot finds the first
//     mismatch (or the chromosome's end: the bounds are 0 and the chromosome's length, never the image's neighbours).
//     It continues at the cap, so the result does not depend on which path handled the allele.
//   * k_vrs_digest, one lane per allele: the SequenceLocation text and then the Allele text go through sha512_stream
//     (sha512.h) a byte at a time from a small state machine over the text's parts -- literals, decimal digits and the
//     location digest held in registers, the accession from a per-assembly table, left context / trimmed ALT / right
//     context from the image and the pool.  Nothing is staged in memory, the message schedule is a register ring.
//     Alleles whose normalized sequence is longer than GTARS_VRS_HOST_LEN bytes are listed for the host instead (one lane
//     must not hash a megabase serially): vrs_run finishes them with the same header on the host threads.
//   * k_vrs_lens + the scan of kernels.hip + the fill of byte_csr.h over VrsRowSrc (profiled as k_vrs_fill): the normalized
//     sequences as a byte CSR, eight output bytes per lane.
// The kernels see sequences only as (bytes, offsets, lengths, accessions): vrs_run_view runs them over any such view --
// the assembly's image (vrs_run), or the mature mRNAs a call of K23 derived (hgvs_tx.hip), where "chromosome" is a slot.
#include <cstring>

#include "byte_csr.h"
#include "common.h"
#include "host_threads.h"
#include "image_call.h"
#include "pipeline.h"
#include "sha512.h"
#include "vrs.h"
#include "vrs_core.h"

namespace gtars {

namespace {

constexpr int VRS_TPB = 256;
constexpr u32 VRS_MAX_BLOCKS = 256 * 8;
constexpr u64 VRS_MAX_N = 0x7FFFFFF0u;

struct VrsView {  // device pointers of one batch
    const u8 *seq;
    const u64 *coff, *clen;
    u32 n_chrom;
    const u8 *acc;  // [n_chrom * 32], a zero first byte: no accession; null: every chromosome counts
    const u32 *chrom;
    const u64 *start;
    const u8 *pool;
    u64 pool_bytes;
    const u32 *ref_off, *ref_len, *alt_off, *alt_len;
    u32 n;
    // per allele
    u8 *status;
    u64 *ns, *ne;            // the new interval
    u32 *lroll, *rroll;      // bases rolled
    u32 *t_off, *t_len;      // the trimmed ALT in the pool
};

struct VrsHostRec {  // an allele the digest kernel leaves to the host
    u32 idx, chrom, lroll, rroll, t_off, t_len;
    u64 ns, ne;
};

__device__ __forceinline__ u32 up(u32 b) { return b - 97u < 26u ? b - 32u : b; }

__global__ void __launch_bounds__(VRS_TPB)
k_vrs_normalize(VrsView v, u32 cap, u64 *__restrict__ work, u32 *__restrict__ n_work) {
    for (u64 i = (u64)blockIdx.x * VRS_TPB + threadIdx.x; i < v.n; i += (u64)gridDim.x * VRS_TPB) {
        const u32 c = v.chrom[i];
        const u64 st = v.start[i];
        const u32 ro = v.ref_off[i], rl0 = v.ref_len[i], ao = v.alt_off[i], al0 = v.alt_len[i];
        u32 status = VRS_OK;
        u64 len = 0;
        if (c >= v.n_chrom || (v.acc && v.acc[(u64)c * 32] == 0)) status = VRS_NO_CHROM;
        else if ((u64)ro + rl0 > v.pool_bytes || (u64)ao + al0 > v.pool_bytes) status = VRS_BAD_ALLELE;
        else if (st + rl0 < st) status = VRS_START_OUT_OF_BOUNDS;
        else {
            len = v.clen[c];
            if (st + rl0 > len) status = VRS_REF_PAST_END;
        }
        u64 s = 0, e = 0;
        u32 lroll = 0, rroll = 0, t_off = 0, t_len = 0;
        if (status == VRS_OK) {
            const u8 *__restrict__ seq = v.seq + v.coff[c];
            const u8 *__restrict__ ref = v.pool + ro, *__restrict__ alt = v.pool + ao;
            for (u32 k = 0; k < rl0; ++k)
                if (up(ref[k]) != up(seq[st + k])) {
                    status = VRS_REF_MISMATCH;
                    break;
                }
            if (status == VRS_OK) {
                u32 rl = rl0, al = al0, skip = 0;
                while (skip < rl && skip < al && ref[skip] == alt[skip]) ++skip;
                rl -= skip, al -= skip;
                ref += skip, alt += skip;
                u32 cut = 0;
                while (cut < rl && cut < al && ref[rl - 1 - cut] == alt[al - 1 - cut]) ++cut;
                rl -= cut, al -= cut;
                s = st + skip, e = st + rl0 - cut;
                t_off = ao + skip, t_len = al;
                if (rl | al) {
                    // (s <= len < 2^32: vrs_run refuses longer chromosomes)
                    const u32 max_l = (u32)s, max_r = (u32)(len - e);
                    const u32 lim_l = min(max_l, cap), lim_r = min(max_r, cap);
                    u32 ir = rl ? rl - 1 : 0, ia = al ? al - 1 : 0;
                    while (lroll < lim_l) {
                        const u32 base = up(seq[s - 1 - lroll]);
                        if ((rl && ref[ir] != base) || (al && alt[ia] != base)) break;
                        ++lroll;
                        ir = ir ? ir - 1 : (rl ? rl - 1 : 0);
                        ia = ia ? ia - 1 : (al ? al - 1 : 0);
                    }
                    if (lroll == cap && cap < max_l) work[atomicAdd(n_work, 1u)] = i * 2;
                    ir = ia = 0;
                    while (rroll < lim_r) {
                        const u32 base = up(seq[e + rroll]);
                        if ((rl && ref[ir] != base) || (al && alt[ia] != base)) break;
                        ++rroll;
                        if (rl && ++ir == rl) ir = 0;
                        if (al && ++ia == al) ia = 0;
                    }
                    if (rroll == cap && cap < max_r) work[atomicAdd(n_work, 1u)] = i * 2 + 1;
                }
            }
        }
        const bool ok = status == VRS_OK;
        v.status[i] = (u8)status;
        v.ns[i] = ok ? s - lroll : 0;
        v.ne[i] = ok ? e + rroll : 0;
        v.lroll[i] = lroll, v.rroll[i] = rroll;
        v.t_off[i] = ok ? t_off : 0, v.t_len[i] = ok ? t_len : 0;
    }
}

// one wave per work-list entry: the roll goes on from where the lane path stopped
__global__ void __launch_bounds__(VRS_TPB)
k_vrs_roll_long(VrsView v, const u64 *__restrict__ work, const u32 *__restrict__ n_work) {
    const u32 lane = threadIdx.x & 63;
    const u32 total = *n_work;
    for (u32 w = blockIdx.x * (VRS_TPB / 64) + (threadIdx.x >> 6); w < total; w += gridDim.x * (VRS_TPB / 64)) {
        const u64 entry = work[w];
        const u64 i = entry >> 1;
        const bool right = entry & 1;
        const u32 c = v.chrom[i];
        const u8 *__restrict__ seq = v.seq + v.coff[c];
        const u64 len = v.clen[c];
        // the trimmed alleles: ALT as the lane path left it, REF from the same two trims
        const u32 t_off = v.t_off[i], al = v.t_len[i];
        const u32 skip = t_off - v.alt_off[i];
        const u32 cut = v.alt_len[i] - skip - al;
        const u32 rl = v.ref_len[i] - skip - cut;
        const u8 *__restrict__ ref = v.pool + v.ref_off[i] + skip, *__restrict__ alt = v.pool + t_off;
        u64 d0 = right ? v.rroll[i] : v.lroll[i];
        const u64 edge = right ? v.ne[i] - d0 : v.ns[i] + d0;  // e or s of the trimmed allele
        const u64 max_d = right ? len - edge : edge;
        u64 d_final;
        for (;;) {
            const u64 d = d0 + lane;
            bool stop = d >= max_d;
            if (!stop) {
                const u32 base = up(seq[right ? edge + d : edge - 1 - d]);
                if (rl) {
                    const u32 m = (u32)((right ? d : d + 1) % rl);
                    stop |= ref[right ? m : (m ? rl - m : 0)] != base;
                }
                if (al) {
                    const u32 m = (u32)((right ? d : d + 1) % al);
                    stop |= alt[right ? m : (m ? al - m : 0)] != base;
                }
            }
            const unsigned long long b = __ballot(stop);
            if (b) {
                d_final = d0 + (u64)(__ffsll((long long)b) - 1);
                break;
            }
            d0 += 64;
        }
        if (lane == 0) {
            if (right) v.rroll[i] = (u32)d_final, v.ne[i] = edge + d_final;
            else v.lroll[i] = (u32)d_final, v.ns[i] = edge - d_final;
        }
    }
}

// ---- the digest ---------------------------------------------------------------------------------------------------
__device__ const char T_LOC_A[] = "{\"end\":";
__device__ const char T_LOC_B[] = ",\"sequenceReference\":{\"refgetAccession\":\"SQ.";
__device__ const char T_LOC_C[] = "\",\"type\":\"SequenceReference\"},\"start\":";
__device__ const char T_LOC_D[] = ",\"type\":\"SequenceLocation\"}";
__device__ const char T_AL_A[] = "{\"location\":\"";
__device__ const char T_AL_B[] = "\",\"state\":{\"sequence\":\"";
__device__ const char T_AL_C[] = "\",\"type\":\"LiteralSequenceExpression\"},\"type\":\"Allele\"}";
constexpr u32 N_LOC_A = sizeof(T_LOC_A) - 1, N_LOC_B = sizeof(T_LOC_B) - 1, N_LOC_C = sizeof(T_LOC_C) - 1, N_LOC_D = sizeof(T_LOC_D) - 1;
constexpr u32 N_AL_A = sizeof(T_AL_A) - 1, N_AL_B = sizeof(T_AL_B) - 1, N_AL_C = sizeof(T_AL_C) - 1;

// a number's decimal text, right-aligned in 24 characters held in three registers (first character in the top byte)
struct Digits {
    u64 w0, w1, w2;
    u32 n;
};
__device__ __forceinline__ Digits digits_of(u64 x) {
    Digits d{0, 0, 0, 0};
    do {
        u32 digit;
        if (x >> 32) {
            digit = (u32)(x % 10), x /= 10;
        } else {
            const u32 y = (u32)x;
            digit = y % 10u, x = y / 10u;
        }
        const u32 pos = 23u - d.n;
        const u64 ch = (u64)(48u + digit) << (56u - 8u * (pos & 7u));
        if (pos >= 16) d.w2 |= ch;
        else if (pos >= 8) d.w1 |= ch;
        else d.w0 |= ch;
        ++d.n;
    } while (x);
    return d;
}

// the bytes of the two texts, in order.  A part is memory (read as it is, or upper-cased) or up to 32 characters held in
// four registers; open() moves to part `seg` of the current message.
struct VrsSrc {
    // what the parts are made from
    const u8 *acc, *lctx, *alt, *rctx;
    u32 n_l, n_a, n_r;
    u64 ds0, ds1, ds2, de0, de1, de2;  // the digits of start and end
    u32 n_ds, n_de;
    u64 l0, l1, l2, l3;  // the location digest, once message 0 is done
    // the cursor
    int msg, seg;
    u32 left, mode;  // mode 0: memory, 1: memory upper-cased, 2: registers
    const u8 *p;
    u64 r0, r1, r2, r3;
    u32 at;  // next character of the registers

    __device__ __forceinline__ void mem(const void *q, u32 n, u32 m) { p = (const u8 *)q, left = n, mode = m; }
    __device__ __forceinline__ void regs(u64 a, u64 b, u64 c, u64 d, u32 first, u32 n) {
        r0 = a, r1 = b, r2 = c, r3 = d, at = first, left = n, mode = 2;
    }
    __device__ __forceinline__ void open() {
        if (msg == 0) {
            switch (seg) {
                case 0: mem(T_LOC_A, N_LOC_A, 0); break;
                case 1: regs(de0, de1, de2, 0, 24 - n_de, n_de); break;
                case 2: mem(T_LOC_B, N_LOC_B, 0); break;
                case 3: mem(acc, 32, 0); break;
                case 4: mem(T_LOC_C, N_LOC_C, 0); break;
                case 5: regs(ds0, ds1, ds2, 0, 24 - n_ds, n_ds); break;
                default: mem(T_LOC_D, N_LOC_D, 0); break;
            }
        } else {
            switch (seg) {
                case 0: mem(T_AL_A, N_AL_A, 0); break;
                case 1: regs(l0, l1, l2, l3, 0, 32); break;
                case 2: mem(T_AL_B, N_AL_B, 0); break;
                case 3: mem(lctx, n_l, 1); break;
                case 4: mem(alt, n_a, 0); break;
                case 5: mem(rctx, n_r, 1); break;
                default: mem(T_AL_C, N_AL_C, 0); break;
            }
        }
    }
    __device__ __forceinline__ void begin(int m) {
        msg = m, seg = 0;
        open();
    }
    __device__ __forceinline__ u64 length() const {
        return msg == 0 ? (u64)(N_LOC_A + N_LOC_B + 32 + N_LOC_C + N_LOC_D) + n_de + n_ds
                        : (u64)(N_AL_A + 32 + N_AL_B + N_AL_C) + n_l + n_a + n_r;
    }
    // (called length() times per message: the last part is never left)
    __device__ __forceinline__ uint8_t next() {
        while (left == 0) {
            ++seg;
            open();
        }
        --left;
        u32 b;
        if (mode == 2) {
            const u32 q = at >> 3;
            // (assignments, not a conditional expression over the members: that one selects an ADDRESS and loads from it,
            // which keeps the whole cursor in scratch)
            u64 w = r3;
            if (q == 0) w = r0;
            else if (q == 1) w = r1;
            else if (q == 2) w = r2;
            b = (u32)(w >> (56u - 8u * (at & 7u))) & 0xFFu;
            ++at;
        } else {
            b = *p++;
            if (mode == 1) b = up(b);
        }
        return (uint8_t)b;
    }
};

__global__ void __launch_bounds__(VRS_TPB)
k_vrs_digest(VrsView v, u32 host_len, u64 *__restrict__ out, VrsHostRec *__restrict__ host_list, u32 *__restrict__ n_host) {
    for (u64 i = (u64)blockIdx.x * VRS_TPB + threadIdx.x; i < v.n; i += (u64)gridDim.x * VRS_TPB) {
        u64 *dst = out + i * 4;
        if (v.status[i] != VRS_OK) {
            dst[0] = dst[1] = dst[2] = dst[3] = 0;
            continue;
        }
        const u32 c = v.chrom[i];
        const u64 ns = v.ns[i], ne = v.ne[i];
        const u32 lroll = v.lroll[i], rroll = v.rroll[i], t_off = v.t_off[i], t_len = v.t_len[i];
        if ((u64)lroll + t_len + rroll > host_len) {
            host_list[atomicAdd(n_host, 1u)] = VrsHostRec{(u32)i, c, lroll, rroll, t_off, t_len, ns, ne};
            continue;
        }
        const u8 *seq = v.seq + v.coff[c];
        VrsSrc src;
        src.acc = v.acc + (u64)c * 32;
        src.lctx = seq + ns, src.n_l = lroll;
        src.alt = v.pool + t_off, src.n_a = t_len;
        src.rctx = seq + (ne - rroll), src.n_r = rroll;
        const Digits d_start = digits_of(ns), d_end = digits_of(ne);
        src.ds0 = d_start.w0, src.ds1 = d_start.w1, src.ds2 = d_start.w2, src.n_ds = d_start.n;
        src.de0 = d_end.w0, src.de1 = d_end.w1, src.de2 = d_end.w2, src.n_de = d_end.n;
        src.l0 = src.l1 = src.l2 = src.l3 = 0;
        Sha512 sh;
#pragma unroll 1
        for (int m = 0; m < 2; ++m) {
            src.begin(m);
            sha512_stream(sh, src, src.length());
            u64 t[4];
            sha512t24u_words(sh, t);
            src.l0 = t[0], src.l1 = t[1], src.l2 = t[2], src.l3 = t[3];
        }
        // (the text's first character first in memory)
        dst[0] = __builtin_bswap64(src.l0), dst[1] = __builtin_bswap64(src.l1);
        dst[2] = __builtin_bswap64(src.l2), dst[3] = __builtin_bswap64(src.l3);
    }
}

// ---- the normalized sequences as a byte CSR -------------------------------------------------------------------------
__global__ void __launch_bounds__(VRS_TPB) k_vrs_lens(VrsView v, u32 *__restrict__ cnt, u32 *__restrict__ bad) {
    for (u64 i = (u64)blockIdx.x * VRS_TPB + threadIdx.x; i < v.n; i += (u64)gridDim.x * VRS_TPB) {
        const u64 k = v.status[i] == VRS_OK ? (u64)v.lroll[i] + v.t_len[i] + v.rroll[i] : 0;
        if (k > 0xFFFFFFFFull) atomicOr(bad, 1u);
        cnt[i] = (u32)k;
    }
}

// a row of the CSR: the left context upper-cased, the trimmed ALT, the right context upper-cased
struct VrsRowSrc {
    VrsView v;
    const u8 *lctx, *alt, *rctx;  // of the open row
    u32 lroll, t_len;
    __device__ __forceinline__ void open(u32 r) {
        const u8 *seq = v.seq + v.coff[v.chrom[r]];
        lroll = v.lroll[r], t_len = v.t_len[r];
        lctx = seq + v.ns[r], alt = v.pool + v.t_off[r], rctx = seq + (v.ne[r] - v.rroll[r]);
    }
    __device__ __forceinline__ u32 byte(u64 k) const {
        if (k < lroll) return up(lctx[k]);
        if (k < (u64)lroll + t_len) return alt[k - lroll];
        return up(rctx[k - lroll - t_len]);
    }
};

}  // namespace

gtars_status vrs_run_view(const VrsSeqView &sv, const VrsCall &call) {
    const AssemblyParts ap{sv.seq, sv.off, sv.len, sv.n_seq, sv.device};
    if (ap.device < 0) return fail(GTARS_ERR_INTERNAL, "vrs: the assembly has no device image");
    if (call.n > VRS_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "vrs: too many alleles (" + std::to_string(call.n) + ")");
    if ((call.seq_off == nullptr) != (call.seq_bytes == nullptr)) return fail(GTARS_ERR_INVALID_ARG, "vrs: sequences need both vectors");
    if (call.digest && !sv.d_acc && !sv.h_acc) return fail(GTARS_ERR_INVALID_ARG, "vrs: digests need the accession table");
    if (call.seq_off) call.seq_off->assign(1, 0), call.seq_bytes->clear();
    if (!call.n) return GTARS_OK;
    if (!call.chrom || !call.start || !call.ref_off || !call.ref_len || !call.alt_off || !call.alt_len || (!call.pool && call.pool_bytes))
        return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    GT_TRY(digests_aligned("vrs", call.on_device, call.digest));
    if (call.on_device) GT_TRY(require_handle_device(ap.device));
    ImageCall ic(ap, call.on_device, call.stream);
    GT_TRY(ic.scope.st);
    StreamFrame &fr = ic.fr;
    hipStream_t st = fr.st;
    const size_t n = (size_t)call.n;
    const long cap = std::max(1l, std::min(cfg_int("GTARS_VRS_ROLL_CAP", 64), 0x40000000l));
    const long host_len = std::max(0l, std::min(cfg_int("GTARS_VRS_HOST_LEN", 4096), 0x40000000l));

    VrsView v{};
    v.seq = ap.seq, v.coff = ap.off, v.clen = ap.len, v.n_chrom = ap.n_chrom, v.n = (u32)n, v.pool_bytes = call.pool_bytes;
    GT_TRY(ic.in(call.chrom, n, &v.chrom));
    GT_TRY(ic.in(call.start, n, &v.start));
    GT_TRY(ic.in(call.ref_off, n, &v.ref_off));
    GT_TRY(ic.in(call.ref_len, n, &v.ref_len));
    GT_TRY(ic.in(call.alt_off, n, &v.alt_off));
    GT_TRY(ic.in(call.alt_len, n, &v.alt_len));
    GT_TRY(ic.in(call.pool, (size_t)call.pool_bytes, &v.pool));
    if (sv.d_acc) {
        v.acc = sv.d_acc;
    } else if (sv.h_acc) {
        u8 *d_acc;
        GT_TRY(fr.upload(&d_acc, (const u8 *)sv.h_acc, (size_t)ap.n_chrom * 32));
        v.acc = d_acc;
    }
    // per-allele results: the caller's device columns where it gave them, the frame's otherwise
    GT_TRY(ic.out(call.status, n, &v.status));
    GT_TRY(ic.out(call.new_start, n, &v.ns));
    GT_TRY(ic.out(call.new_end, n, &v.ne));
    GT_TRY(fr.alloc(&v.lroll, n));
    GT_TRY(fr.alloc(&v.rroll, n));
    GT_TRY(fr.alloc(&v.t_off, n));
    GT_TRY(fr.alloc(&v.t_len, n));
    u64 *work;
    u32 *counters;  // [0] work-list entries, [1] host-list entries, [2] a sequence too long for the CSR
    GT_TRY(fr.alloc(&work, 2 * n));
    GT_TRY(fr.alloc(&counters, 4));
    GT_HIP(hipMemsetAsync(counters, 0, 4 * sizeof(u32), st));
    const unsigned grid = grid_for(n, VRS_TPB, VRS_MAX_BLOCKS);
    {
        ProfScope ps("k_vrs_normalize", st);
        hipLaunchKernelGGL(k_vrs_normalize, dim3(grid), dim3(VRS_TPB), 0, st, v, (u32)cap, work, counters);
        GT_HIP(hipGetLastError());
    }
    {
        ProfScope ps("k_vrs_roll_long", st);
        hipLaunchKernelGGL(k_vrs_roll_long, dim3(grid_for(2 * n, VRS_TPB / 64, 1024)), dim3(VRS_TPB), 0, st, v, work, counters);
        GT_HIP(hipGetLastError());
    }
    if (call.digest) {
        u64 *d_digest;
        GT_TRY(ic.digests_out(call.digest, n, &d_digest));
        VrsHostRec *host_list;
        GT_TRY(fr.alloc(&host_list, n));
        {
            ProfScope ps("k_vrs_digest", st);
            hipLaunchKernelGGL(k_vrs_digest, dim3(grid), dim3(VRS_TPB), 0, st, v, (u32)host_len, d_digest, host_list, counters + 1);
            GT_HIP(hipGetLastError());
        }
        u32 *h_n;
        GT_TRY(ic.host_word(&h_n));
        GT_TRY(fr.download(h_n, counters + 1, 1));
        GT_TRY(fr.drain());
        if (const u32 n_host = *h_n) {
            // the host tail: the records and their ALT bytes come back, the digests go up
            if (!sv.host_tail) return fail(GTARS_ERR_INTERNAL, "vrs: the host tail needs the host sequences");
            std::vector<VrsHostRec> recs;
            GT_TRY(fr.download(recs, host_list, n_host));
            GT_TRY(fr.drain());
            std::vector<std::vector<u8>> alts(n_host);
            std::vector<u32> ids(n_host);
            for (u32 k = 0; k < n_host; ++k) {
                ids[k] = recs[k].chrom;
                alts[k].resize(recs[k].t_len);
                GT_TRY(fr.download(alts[k].data(), v.pool + recs[k].t_off, recs[k].t_len));
            }
            GT_TRY(fr.drain());
            std::vector<const uint8_t *> h_seq;
            std::vector<const char *> h_acc;
            GT_TRY(sv.host_tail(ids, h_seq, h_acc));
            if (h_seq.size() != n_host || h_acc.size() != n_host) return fail(GTARS_ERR_INTERNAL, "vrs: the host tail got no sequences");
            std::vector<char> text((size_t)n_host * 32);
            parallel_for(n_host, call.threads, 1, [&](size_t k) {
                const VrsHostRec &r = recs[k];
                const uint8_t *seq = h_seq[k];
                char acc[35] = {'S', 'Q', '.'};
                memcpy(acc + 3, h_acc[k], 32);
                char loc[32];
                vrs_location_digest(acc, 35, r.ns, r.ne, loc);
                vrs_allele_digest(loc, seq + r.ns, r.lroll, alts[k].data(), r.t_len, seq + (r.ne - r.rroll), r.rroll, &text[k * 32]);
            });
            for (u32 k = 0; k < n_host; ++k) GT_TRY(fr.upload_to((char *)(d_digest + 4 * (size_t)recs[k].idx), &text[(size_t)k * 32], 32));
            GT_TRY(fr.drain());
        }
        GT_TRY(ic.digests_back(call.digest, d_digest, n));
    }
    if (call.seq_off) {
        u32 *cnt, *h_bad;
        GT_TRY(ic.host_word(&h_bad));
        GT_TRY(fr.alloc(&cnt, n));
        {
            ProfScope ps("k_vrs_lens", st);
            hipLaunchKernelGGL(k_vrs_lens, dim3(grid), dim3(VRS_TPB), 0, st, v, cnt, counters + 2);
            GT_HIP(hipGetLastError());
        }
        GT_TRY(fr.download(h_bad, counters + 2, 1));
        u64 *off, total = 0;
        GT_TRY(scan_total(fr, cnt, n, &off, &total));
        if (*h_bad) return fail(GTARS_ERR_CAPACITY, "vrs: a normalized sequence is longer than 2^32 - 1 bytes");
        GT_TRY(fr.download(*call.seq_off, off, n + 1));
        call.seq_bytes->resize((size_t)total);
        if (total) {
            u8 *d_bytes;
            GT_TRY(fr.alloc(&d_bytes, (size_t)total));
            GT_TRY(csr_fill("k_vrs_fill", VrsRowSrc{v}, off, v.n, total, d_bytes, st));
            GT_TRY(fr.download(call.seq_bytes->data(), d_bytes, (size_t)total));
        }
    }
    GT_TRY(ic.back(call.status, v.status, n));
    GT_TRY(ic.back(call.new_start, v.ns, n));
    GT_TRY(ic.back(call.new_end, v.ne, n));
    return fr.drain();
}

gtars_status vrs_run(const Assembly &a, const VrsCall &call) {
    const AssemblyParts ap = assembly_parts(a);
    VrsSeqView sv;
    sv.device = ap.device, sv.seq = ap.seq, sv.off = ap.off, sv.len = ap.len, sv.n_seq = ap.n_chrom, sv.h_acc = call.accessions;
    if (call.h_seq)
        sv.host_tail = [&call](const std::vector<uint32_t> &ids, std::vector<const uint8_t *> &seq, std::vector<const char *> &acc) {
            for (const uint32_t c : ids) seq.push_back(call.h_seq[c]), acc.push_back(call.accessions + (size_t)c * 32);
            return GTARS_OK;
        };
    return vrs_run_view(sv, call);
}

}  // namespace gtars
