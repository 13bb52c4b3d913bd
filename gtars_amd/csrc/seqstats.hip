// seqstats.hip -- K12: per-region GC content and dinucleotide counts over a genome assembly that is resident on the
// device (gtars-genomicdist/src/statistics.rs:331-483: calc_gc_content / calc_dinucl_freq; Dinucleotide::from_bytes,
// models.rs:467-492).  The reference walks every region's bytes on one thread; here the assembly sits in device memory
// once (Assembly: one packed byte buffer, every chromosome at a 16-byte-aligned offset with at least 16 zero bytes
// behind it) and a set of regions is a streaming read of the bytes it covers.
//
//   * work is balanced by BYTES: k_seq_pieces counts ceil(width / SEQ_PIECE) pieces per region (and zeroes the rows
//     that are not exactly one piece), the scan of kernels.hip turns the counts into offsets, and k_seq_count hands
//     piece p -- found by a search of the offsets -- to a group of LANES lanes.  A 2 Mbp region is 489 pieces spread
//     over the chip, a 200 bp peak is one.
//   * a group reads its piece as 16-byte vectors at aligned addresses, one per lane and step.  Head and tail are masked
//     by position: bytes outside the piece are replaced by 0, which is neither G / C nor a nucleotide.  The padding
//     behind every chromosome makes the last aligned vector, and the one byte behind it, legal to load.
//   * GC: four bytes at a time -- (b & 0xDB) == 0x43 holds for exactly C, G, c, g -- by a zero-byte test and a popcount.
//   * dinucleotides: a byte is classified by arithmetic (fold the case, a 32-bit register table of the four letters,
//     code = A C G T -> 0 1 2 3 from bits 1-2); a window's second byte comes from the same vector, from the neighbour
//     lane's first byte, or -- last lane of a group, last vector of a piece -- from one byte load.  A lane counts 8
//     windows into sixteen 4-bit fields of one 64-bit register, widens them into 16-bit fields (4 registers; a lane sees
//     at most 17 vectors of a piece) and the group adds the packed registers up (a piece has at most 4096 windows).
//   * a region that is one piece STORES its row, a region of several pieces ADDS with integer atomics into the row
//     k_seq_pieces zeroed: integer sums do not depend on order, the counts are exact either way.
//   * LANES = 16 or 64 (a 256-byte or a 1-KiB step): GTARS_SEQ_LANES picks, see DESIGN.md K12 for the figures.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>

#include "byte_csr.h"
#include "common.h"
#include "image_call.h"
#include "pipeline.h"
#include "seqstats.h"

namespace gtars {

struct Assembly {
    int device = -1;
    u32 n_chrom = 0;
    u64 bytes = 0;    // of the packed buffer
    DevBuf<u8> seq;   // 16-byte aligned (hipMalloc)
    DevBuf<u64> off;  // [n_chrom]
    DevBuf<u64> len;  // [n_chrom]
};

namespace {

constexpr int SEQ_TPB = 256;
constexpr u64 SEQ_MAX_N = 0xFFFFF000u;
constexpr u32 SEQ_MAX_BLOCKS = 256 * 8;
constexpr size_t SEQ_STAGE_BYTES = 32u << 20;  // one pinned staging block of the upload (GTARS_SEQ_STAGE_BYTES, a test switch)

// the staging block's size: the switch's value rounded down to a multiple of 16 (the image's alignment), at least 16
size_t stage_bytes() {
    const long v = cfg_int("GTARS_SEQ_STAGE_BYTES", (long)SEQ_STAGE_BYTES);
    return (size_t)std::max<long>(v, 16) & ~(size_t)15;
}
std::atomic<u64> g_stage_blocks{0};  // staging blocks sent by every assembly_build so far (gtars_debug_seq_stage_blocks)

// pieces per row; rows that are not one piece are zeroed here (no piece, or several that add).  A row that does not lie
// inside its chromosome gets no piece and raises *bad.
template <int COLS>
__global__ void __launch_bounds__(SEQ_TPB)
k_seq_pieces(const u32 *__restrict__ chrom, const u32 *__restrict__ start, const u32 *__restrict__ end, u32 n,
             const u64 *__restrict__ clen, u32 n_chrom, u32 *__restrict__ cnt, u32 *__restrict__ out, u32 *__restrict__ bad) {
    for (u64 i = (u64)blockIdx.x * SEQ_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * SEQ_TPB) {
        const u32 c = chrom[i], s = start[i], e = end[i];
        u32 k = 0;
        if (c >= n_chrom || s > e || (u64)e > clen[c]) {
            atomicOr(bad, 1u);
        } else {
            const u32 w = e - s;
            k = w / SEQ_PIECE + (w % SEQ_PIECE != 0);
        }
        cnt[i] = k;
        if (k != 1) {
            if (COLS == 1) {
                out[i] = 0;
            } else {
                uint4 *row = (uint4 *)(out + i * 16);
#pragma unroll
                for (int q = 0; q < 4; ++q) row[q] = make_uint4(0, 0, 0, 0);
            }
        }
    }
}

// the low k bytes of a word set (k <= 0: none, k >= 4: all)
__device__ __forceinline__ u32 low_bytes(int k) { return k <= 0 ? 0u : k >= 4 ? 0xFFFFFFFFu : (1u << (8 * k)) - 1u; }

// number of bytes of w that are C, G, c or g
__device__ __forceinline__ u32 gc_in_word(u32 w) {
    const u32 y = (w & 0xDBDBDBDBu) ^ 0x43434343u;  // a zero byte per hit
    const u32 t = ((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y;  // bit 7 of a byte set unless the byte is zero
    return (u32)__popc(~t & 0x80808080u);
}

// byte -> (is one of ACGTacgt, its code A C G T = 0 1 2 3)
__device__ __forceinline__ void classify(u32 b, u32 &ok, u32 &code) {
    const u32 c = b & 0xDFu;   // a-z -> A-Z; no other byte lands on a letter
    const u32 d = c - 0x41u;   // A 0, C 2, G 6, T 19
    ok = d < 32u ? (0x00080045u >> d) & 1u : 0u;
    const u32 x = (c >> 1) & 3u;  // A 0, C 1, G 3, T 2
    code = x ^ (x >> 1);
}

template <int LANES>
__device__ __forceinline__ u32 group_sum(u32 v) {
#pragma unroll
    for (int d = LANES / 2; d >= 1; d >>= 1) v += __shfl_xor(v, d, LANES);
    return v;
}

// first r in [0, n) with off[r + 1] > p (p < off[n])
__device__ __forceinline__ u32 row_of_piece(const u64 *__restrict__ off, u32 n, u64 p) { return last_le(off, n, p); }

template <int LANES, bool DINUCL>
__global__ void __launch_bounds__(SEQ_TPB)
k_seq_count(const u8 *__restrict__ seq, const u64 *__restrict__ coff, const u32 *__restrict__ chrom, const u32 *__restrict__ start,
            const u32 *__restrict__ end, u32 n, const u64 *__restrict__ off, u64 n_pieces, u32 *__restrict__ out) {
    constexpr int GROUPS = SEQ_TPB / LANES;
    const int gl = threadIdx.x % LANES;
    const u64 g0 = (u64)blockIdx.x * GROUPS + threadIdx.x / LANES;
    for (u64 p = g0; p < n_pieces; p += (u64)gridDim.x * GROUPS) {
        const u32 r = row_of_piece(off, n, p);
        const u64 first = off[r];
        const bool single = off[r + 1] - first == 1;
        const u64 base = coff[chrom[r]];
        const u32 s = start[r], e = end[r];
        const u64 ps = (u64)s + (p - first) * SEQ_PIECE;
        const u64 pe = std::min<u64>(e, ps + SEQ_PIECE);
        // absolute byte positions in the packed buffer: the piece's bytes [lo, hi); a window is named by its first byte
        // and needs its second one inside the REGION, so the piece's windows are [lo, hi_w)
        const i64 lo = (i64)(base + ps), hi = (i64)(base + pe);
        const i64 hi_w = DINUCL ? std::min<i64>(hi, (i64)(base + e) - 1) : hi;
        const i64 a0 = lo & ~(i64)15;
        const i64 nv = (hi - a0 + 15) >> 4;  // aligned vectors that hold the piece's bytes
        u32 gc = 0;
        u64 acc[4] = {0, 0, 0, 0};  // 16-bit fields: acc[j] field f counts dinucleotide j + 4 f
        for (i64 v0 = 0; v0 < nv; v0 += LANES) {
            const i64 v = v0 + gl;
            const bool active = v < nv;
            const i64 a = a0 + 16 * v;
            uint4 x = make_uint4(0, 0, 0, 0);
            if (active) x = *(const uint4 *)(seq + a);
            u32 w[4] = {x.x, x.y, x.z, x.w};
            if (!DINUCL) {
                const int k0 = (int)std::max<i64>(std::min<i64>(lo - a, 16), 0), k1 = (int)std::max<i64>(std::min<i64>(hi - a, 16), 0);
#pragma unroll
                for (int q = 0; q < 4; ++q) gc += gc_in_word(w[q] & low_bytes(k1 - 4 * q) & ~low_bytes(k0 - 4 * q));
            } else {
                // the byte behind the vector: the neighbour's first one, or a load of its own
                u32 nb = __shfl_down(w[0], 1, LANES) & 0xFFu;
                if (active && (gl == LANES - 1 || v + 1 >= nv)) nb = seq[a + 16];
                // bytes k0 .. k1 of the 17 stay: first bytes of the piece's windows and the second byte of its last window
                const int k0 = (int)std::max<i64>(std::min<i64>(lo - a, 17), 0), k1 = (int)std::max<i64>(std::min<i64>(hi_w - a + 1, 17), 0);
#pragma unroll
                for (int q = 0; q < 4; ++q) w[q] &= low_bytes(k1 - 4 * q) & ~low_bytes(k0 - 4 * q);
                if (k1 < 17 || k0 > 16) nb = 0;
                u32 ok_prev, code_prev;
                classify(w[0] & 0xFFu, ok_prev, code_prev);
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    u64 nib = 0;  // sixteen 4-bit fields, at most 8 windows
#pragma unroll
                    for (int k = 8 * half + 1; k <= 8 * half + 8; ++k) {
                        const u32 b = k == 16 ? nb : (w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
                        u32 ok, code;
                        classify(b, ok, code);
                        nib += (u64)(ok & ok_prev) << (4 * (code_prev * 4 + code));
                        ok_prev = ok, code_prev = code;
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] += (nib >> (4 * j)) & 0x000F000F000F000Full;
                }
            }
        }
        if (!DINUCL) {
            gc = group_sum<LANES>(gc);
            if (gl == 0) {
                if (single) out[r] = gc;
                else atomicAdd(&out[r], gc);
            }
        } else {
            u32 lo32[4], hi32[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                lo32[j] = group_sum<LANES>((u32)acc[j]);
                hi32[j] = group_sum<LANES>((u32)(acc[j] >> 32));
            }
            if (gl < 16) {  // lane k holds dinucleotide k: register k & 3, field k >> 2
                const int j = gl & 3, f = gl >> 2;
                const u32 l = j == 0 ? lo32[0] : j == 1 ? lo32[1] : j == 2 ? lo32[2] : lo32[3];
                const u32 h = j == 0 ? hi32[0] : j == 1 ? hi32[1] : j == 2 ? hi32[2] : hi32[3];
                const u32 word = f < 2 ? l : h;
                const u32 c = (word >> (16 * (f & 1))) & 0xFFFFu;
                u32 *dst = out + (u64)r * 16 + gl;
                if (single) *dst = c;
                else atomicAdd(dst, c);
            }
        }
    }
}

template <int LANES, bool DINUCL>
gtars_status launch_count(const Assembly &a, const u32 *chrom, const u32 *start, const u32 *end, u32 n, const u64 *off, u64 n_pieces,
                          u32 *out, hipStream_t st) {
    constexpr u32 groups = SEQ_TPB / LANES;
    ProfScope ps(DINUCL ? "k_seq_dinucl" : "k_seq_gc", st);
    hipLaunchKernelGGL((k_seq_count<LANES, DINUCL>), dim3(grid_for(n_pieces, groups, SEQ_MAX_BLOCKS)), dim3(SEQ_TPB), 0, st, a.seq.p,
                       a.off.p, chrom, start, end, n, off, n_pieces, out);
    GT_HIP(hipGetLastError());
    return GTARS_OK;
}

// the columns are on the device, the frame's stream is the caller's
gtars_status counts_on(ImageCall &ic, const Assembly &a, const u32 *d_chrom, const u32 *d_start, const u32 *d_end, u64 n, int mode,
                       u32 *d_out) {
    StreamFrame &fr = ic.fr;
    hipStream_t st = fr.st;
    u32 *cnt, *bad, *h_bad;
    GT_TRY(ic.host_word(&h_bad));
    GT_TRY(fr.alloc(&cnt, (size_t)n));
    GT_TRY(fr.alloc(&bad, 1));
    GT_HIP(hipMemsetAsync(bad, 0, sizeof(u32), st));
    {
        ProfScope ps("k_seq_pieces", st);
        if (mode == GTARS_SEQ_GC)
            hipLaunchKernelGGL(k_seq_pieces<1>, dim3(grid_for(n, SEQ_TPB, SEQ_MAX_BLOCKS)), dim3(SEQ_TPB), 0, st, d_chrom, d_start, d_end,
                               (u32)n, a.len.p, a.n_chrom, cnt, d_out, bad);
        else
            hipLaunchKernelGGL(k_seq_pieces<16>, dim3(grid_for(n, SEQ_TPB, SEQ_MAX_BLOCKS)), dim3(SEQ_TPB), 0, st, d_chrom, d_start, d_end,
                               (u32)n, a.len.p, a.n_chrom, cnt, d_out, bad);
        GT_HIP(hipGetLastError());
    }
    GT_TRY(fr.download(h_bad, bad, 1));
    u64 *off, n_pieces = 0;
    GT_TRY(scan_total(fr, cnt, n, &off, &n_pieces));
    if (*h_bad) return fail(GTARS_ERR_INVALID_ARG, "seqstats: a row does not lie inside its chromosome (start <= end <= length)");
    if (!n_pieces) return GTARS_OK;
    const bool wave = cfg_int("GTARS_SEQ_LANES", 16) == 64;
    if (mode == GTARS_SEQ_GC)
        return wave ? launch_count<64, false>(a, d_chrom, d_start, d_end, (u32)n, off, n_pieces, d_out, st)
                    : launch_count<16, false>(a, d_chrom, d_start, d_end, (u32)n, off, n_pieces, d_out, st);
    return wave ? launch_count<64, true>(a, d_chrom, d_start, d_end, (u32)n, off, n_pieces, d_out, st)
                : launch_count<16, true>(a, d_chrom, d_start, d_end, (u32)n, off, n_pieces, d_out, st);
}

gtars_status check_call(const Assembly &a, u64 n, int mode) {
    if (mode != GTARS_SEQ_GC && mode != GTARS_SEQ_DINUCL) return fail(GTARS_ERR_INVALID_ARG, "seqstats: unknown mode " + std::to_string(mode));
    if (n > SEQ_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "seqstats: too many rows (" + std::to_string(n) + ")");
    if (a.device < 0) return fail(GTARS_ERR_INTERNAL, "seqstats: the assembly has no device image");
    return GTARS_OK;
}

// both entries: the caller's device columns and stream, or host columns on the image's device
gtars_status counts_call(const Assembly &a, bool on_device, const u32 *chrom, const u32 *start, const u32 *end, u64 n, int mode, u32 *out,
                         void *stream) {
    GT_TRY(check_call(a, n, mode));
    if (!n) return GTARS_OK;
    if (!chrom || !start || !end || !out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    if (on_device) {
        if (mode == GTARS_SEQ_DINUCL && ((uintptr_t)out & 15))
            return fail(GTARS_ERR_INVALID_ARG, "seqstats: the device counts must be 16-byte aligned");
        GT_TRY(require_handle_device(a.device));
    }
    ImageCall ic(assembly_parts(a), on_device, stream);
    GT_TRY(ic.scope.st);
    const size_t cells = (size_t)n * (mode == GTARS_SEQ_GC ? 1 : 16);
    const u32 *d_chrom, *d_start, *d_end;
    u32 *d_out;
    GT_TRY(ic.in(chrom, (size_t)n, &d_chrom));
    GT_TRY(ic.in(start, (size_t)n, &d_start));
    GT_TRY(ic.in(end, (size_t)n, &d_end));
    GT_TRY(ic.out(out, cells, &d_out));
    GT_TRY(counts_on(ic, a, d_chrom, d_start, d_end, n, mode, d_out));
    GT_TRY(ic.back(out, d_out, cells));
    return ic.fr.drain();
}

}  // namespace

gtars_status assembly_build(const uint8_t *const *seq, const uint64_t *len, uint32_t n_chrom, Assembly **out) {
    *out = nullptr;
    GT_TRY(require_device());
    auto a = std::make_unique<Assembly>();
    GT_HIP(hipGetDevice(&a->device));
    a->n_chrom = n_chrom;
    std::vector<u64> off(n_chrom), ln(len, len + n_chrom);
    u64 at = 0;
    for (u32 c = 0; c < n_chrom; ++c) {
        off[c] = at;
        at = (at + len[c] + 16 + 15) & ~15ull;  // 16 .. 31 zero bytes, the next chromosome 16-byte aligned
    }
    a->bytes = at;
    GT_TRY(a->seq.alloc((size_t)at));
    GT_TRY(a->off.upload(off));
    GT_TRY(a->len.upload(ln));
    // the packed image leaves through two pinned blocks that take turns: one is filled while the other one's copy runs
    StreamFrame fr(nullptr);
    const size_t block = (size_t)std::min<u64>(std::max<u64>(at, 16), stage_bytes());
    u8 *stage[2] = {(u8 *)fr.host(block), (u8 *)fr.host(block)};
    if (!stage[0] || !stage[1]) return fail(GTARS_ERR_INTERNAL, "out of host memory");
    hipEvent_t done[2] = {nullptr, nullptr};
    struct Events {
        hipEvent_t *e;
        ~Events() {
            for (int k = 0; k < 2; ++k)
                if (e[k]) (void)hipEventDestroy(e[k]);
        }
    } events{done};
    for (int k = 0; k < 2; ++k) GT_HIP(hipEventCreateWithFlags(&done[k], hipEventDisableTiming));
    u32 c = 0;
    u64 in_chrom = 0;  // bytes of chromosome c (padding included) that are staged already
    int turn = 0;
    for (u64 w0 = 0; w0 < at; w0 += block, turn ^= 1) {
        const size_t wl = (size_t)std::min<u64>(block, at - w0);
        u8 *dst = stage[turn];
        GT_HIP(hipEventSynchronize(done[turn]));  // (a fresh event counts as complete)
        size_t filled = 0;
        while (filled < wl) {
            const u64 span = (c + 1 < n_chrom ? off[c + 1] : at) - off[c];  // sequence + padding
            const u64 take = std::min<u64>(span - in_chrom, wl - filled);
            const u64 data = in_chrom < len[c] ? std::min<u64>(len[c] - in_chrom, take) : 0;
            if (data) memcpy(dst + filled, seq[c] + in_chrom, (size_t)data);
            if (take > data) memset(dst + filled + data, 0, (size_t)(take - data));
            filled += (size_t)take;
            in_chrom += take;
            if (in_chrom == span) ++c, in_chrom = 0;
        }
        GT_TRY(fr.upload_to(a->seq.p + w0, dst, wl));
        GT_HIP(hipEventRecord(done[turn], fr.st));
        g_stage_blocks.fetch_add(1, std::memory_order_relaxed);
    }
    GT_TRY(fr.drain());
    *out = a.release();
    return GTARS_OK;
}

void assembly_free(Assembly *a) {
    if (!a) return;
    DeviceScope on(a->device);  // (the buffers go back to the device they came from)
    delete a;
}

uint64_t assembly_stage_blocks() { return g_stage_blocks.load(std::memory_order_relaxed); }

int assembly_device(const Assembly *a) { return a ? a->device : -1; }

AssemblyParts assembly_parts(const Assembly &a) { return AssemblyParts{a.seq.p, a.off.p, a.len.p, a.n_chrom, a.device}; }

int assembly_set_device(Assembly *a, int device) {
    const int before = a->device;
    a->device = device;
    return before;
}

gtars_status seqstats_counts_device(const Assembly &a, const uint32_t *d_chrom, const uint32_t *d_start, const uint32_t *d_end,
                                    uint64_t n, int mode, uint32_t *d_out, void *stream) {
    return counts_call(a, true, d_chrom, d_start, d_end, n, mode, d_out, stream);
}

gtars_status seqstats_counts(const Assembly &a, const uint32_t *chrom, const uint32_t *start, const uint32_t *end, uint64_t n,
                             int mode, uint32_t *out) {
    return counts_call(a, false, chrom, start, end, n, mode, out, nullptr);
}

}  // namespace gtars
