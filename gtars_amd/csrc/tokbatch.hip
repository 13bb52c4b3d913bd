// tokbatch.hip -- K15: B region sets encoded as B independent Tokenizer::tokenize calls (gtars-tokenizers/src/tokenizer.rs:140-163)
// in one device pass, and padded into the [B, W] input_ids / attention_mask a model takes (gtars-python/src/tokenizers/
// py_tokenizers/mod.rs:275-299).  The sets arrive as ONE concatenated query batch plus set_offsets[B + 1]; one call is
//
//   * hits: one gtars_tokenize_device launch over the whole batch, queued without a read-back, its ids straight into the caller's
//     buffer: the per-query CSR q_off[nq + 1] and the raw ids.
//   * k_set_lengths, a lane per set: raw length = q_off[set_offsets[b + 1]] - q_off[set_offsets[b]]; a set without an id becomes
//     [unk] (length 1), max_length clips; the longest length, the empty and the clipped sets and the batch's raw total go to
//     the host with the scan's total in the call's one synchronisation, and the set offsets are checked on the way (device
//     callers hand them over unseen).
//   * output offsets from the u32 scan.  Without a max_length: out_offsets[b] = q_off[set_offsets[b]] + (empty sets before b) --
//     the scan runs over 0 / 1 flags, no length can overflow it.  With one (< 2^32): the scan of the clipped lengths.
//   * no empty set and nothing clipped: the raw ids ARE the result and the call is over.  Otherwise they move to frame scratch
//     and k_set_pack streams them back: a workgroup takes a tile of TOKBATCH_PACK_TILE OUTPUT positions -- balanced over ids, not
//     over sets -- finds the tile's first set by one search, stages the offsets of the at most TILE sets the tile can touch
//     (every set yields at least one id) in LDS, and every lane finds its position's set there.  The lane that owns an empty
//     set's position writes its [unk].
//   * k_set_pad, a lane per cell of the [B, W] matrix, a row's cells in consecutive lanes: the id, or the pad, and the mask byte.
//     A row longer than W is reported, never cut.
#include "byte_csr.h"
#include "common.h"
#include "pipeline.h"
#include "tokbatch.h"

#include "../../include/gtars_amd_debug.h"

namespace gtars {

namespace {

constexpr int TB_TPB = 256;
constexpr u32 TB_MAX_BLOCKS = 256 * 8;
constexpr u64 TB_EMPTY = 1ull << 63;  // in a set's source word: the set has no id of its own

struct SetStats {
    unsigned long long longest;  // over the sets, after the [unk] rule and max_length
    unsigned long long raw;      // q_off[nq]: the ids of the whole batch before either
    u32 n_empty, n_clipped, bad, too_wide;
};

// cnt[b]: the clipped length (clip) or the empty flag; srcw[b]: where the set's raw ids begin | TB_EMPTY
__global__ void __launch_bounds__(TB_TPB)
k_set_lengths(const u64 *__restrict__ q_off, u64 nq, const u64 *__restrict__ set_off, u32 n_sets, u64 max_len, bool clip,
              u32 *__restrict__ cnt, u64 *__restrict__ srcw, SetStats *__restrict__ stats) {
    const int lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0) stats->raw = q_off[nq];
    for (u64 base = (u64)blockIdx.x * TB_TPB; base < n_sets; base += (u64)gridDim.x * TB_TPB) {
        const u64 b = base + threadIdx.x;
        u64 len = 0;
        bool bad = false, empty = false, clipped = false;
        if (b < n_sets) {
            const u64 lo = set_off[b], hi = set_off[b + 1];
            bad = lo > hi || hi > nq || (b == 0 && lo != 0) || (b == n_sets - 1 && hi != nq);
            u64 src = 0;
            if (!bad) {
                src = q_off[lo];
                len = q_off[hi] - src;
            }
            empty = len == 0;
            if (empty) len = 1;
            if (max_len && len > max_len) len = max_len, clipped = true;
            srcw[b] = src | (empty ? TB_EMPTY : 0);
            cnt[b] = clip ? (u32)len : (u32)empty;
        }
        u64 longest = len;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) longest = std::max<u64>(longest, __shfl_xor(longest, d, 64));
        const u32 ne = (u32)__popcll(__ballot(empty)), nc = (u32)__popcll(__ballot(clipped));
        const bool any_bad = __ballot(bad) != 0;
        if (lane == 0) {
            atomicMax(&stats->longest, (unsigned long long)longest);
            if (ne) atomicAdd(&stats->n_empty, ne);
            if (nc) atomicAdd(&stats->n_clipped, nc);
            if (any_bad) atomicOr(&stats->bad, 1u);
        }
    }
}

// out_off[b] for b in [0, n_sets]: the scan itself (clip) or the raw offset of the set's first query + the scan
__global__ void k_set_offsets(const u64 *__restrict__ q_off, const u64 *__restrict__ set_off, const u64 *__restrict__ scan, u32 n_sets,
                              bool clip, u64 *__restrict__ out_off) {
    for (u64 b = (u64)blockIdx.x * blockDim.x + threadIdx.x; b <= n_sets; b += (u64)gridDim.x * blockDim.x)
        out_off[b] = clip ? scan[b] : q_off[set_off[b]] + scan[b];
}

// out[p] for p in [0, total): total = out_off[n_sets] > 0, every set holds at least one position
__global__ void __launch_bounds__(TB_TPB)
k_set_pack(const u64 *__restrict__ out_off, const u64 *__restrict__ srcw, const u32 *__restrict__ src, u32 n_sets, u64 total, u32 unk,
           u32 *__restrict__ out) {
    constexpr u32 T = TOKBATCH_PACK_TILE;
    __shared__ u64 s_off[T + 1];
    __shared__ u64 s_src[T];
    __shared__ u32 s_b0;
    const u64 tiles = (total + T - 1) / T;
    for (u64 t = blockIdx.x; t < tiles; t += gridDim.x) {
        const u64 p0 = t * T;
        if (threadIdx.x == 0) s_b0 = last_le(out_off, n_sets, p0);
        __syncthreads();
        const u32 b0 = s_b0;
        // the tile's positions lie in the sets [b0, b0 + ns): out_off[b0 + T] >= out_off[b0 + 1] + T - 1 >= p0 + T
        const u32 ns = std::min<u32>(T, n_sets - b0);
        for (u32 i = threadIdx.x; i <= ns; i += TB_TPB) {
            s_off[i] = out_off[b0 + i];
            if (i < ns) s_src[i] = srcw[b0 + i];
        }
        __syncthreads();
        const u64 pend = std::min<u64>(p0 + T, total);
        for (u64 p = p0 + threadIdx.x; p < pend; p += TB_TPB) {
            const u32 i = last_le(s_off, ns, p);
            const u64 w = s_src[i];
            out[p] = (w & TB_EMPTY) ? unk : src[(w & ~TB_EMPTY) + (p - s_off[i])];
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(TB_TPB)
k_set_pad(const u64 *__restrict__ out_off, const u32 *__restrict__ ids, u32 n_sets, u32 width, u32 pad, bool left,
          u32 *__restrict__ input_ids, u8 *__restrict__ mask, SetStats *__restrict__ stats) {
    const u64 cells = (u64)n_sets * width;
    const bool narrow = cells <= 0xFFFFFFFFull;  // (a 32-bit division where it is enough)
    for (u64 c = (u64)blockIdx.x * TB_TPB + threadIdx.x; c < cells; c += (u64)gridDim.x * TB_TPB) {
        const u64 b = narrow ? (u64)((u32)c / width) : c / width;
        const u32 w = (u32)(c - b * width);
        const u64 o = out_off[b], len = out_off[b + 1] - o;
        if (len > width && w == 0) atomicOr(&stats->too_wide, 1u);
        const u32 l = (u32)std::min<u64>(len, width), lead = left ? width - l : 0;
        const bool is_id = w >= lead && w - lead < l;
        input_ids[c] = is_id ? ids[o + (w - lead)] : pad;
        mask[c] = is_id ? 1 : 0;
    }
}

gtars_status too_small(u64 need) { return fail(GTARS_ERR_CAPACITY, "ids buffer too small: need " + std::to_string(need)); }

// The ragged result of device columns on the frame's stream.  d_ids == null: offsets, *total and *longest only.  More ids than
// cap: the offsets are complete, *total is set, GTARS_ERR_CAPACITY.
gtars_status sets_on(StreamFrame &fr, const gtars_index_t *ix, const u32 *qc, const u32 *qs, const u32 *qe, u64 nq, const u64 *d_set_off,
                     u64 n_sets, u32 unk, u64 max_len, u64 *d_out_off, u32 *d_ids, u64 cap, u64 *total, u64 *longest) {
    hipStream_t st = fr.st;
    *total = *longest = 0;
    if (n_sets > TOKBATCH_MAX_SETS) return fail(GTARS_ERR_INVALID_ARG, "too many region sets in one batch (" + std::to_string(n_sets) + ")");
    if (!n_sets) {
        if (nq) return fail(GTARS_ERR_INVALID_ARG, "set_offsets must end at the number of regions");
        GT_HIP(hipMemsetAsync(d_out_off, 0, sizeof(u64), st));
        return fr.drain();
    }
    const u32 B = (u32)n_sets;
    if (!d_ids) cap = 0;
    u64 *q_off;
    GT_TRY(fr.alloc(&q_off, (size_t)nq + 1));
    // no total asked for: the launch is only queued, and ids that do not fit are not written (they are fetched again below if they
    // are needed).  The batch's total comes back with the sets' statistics, in the call's one synchronisation.
    if (!nq) GT_HIP(hipMemsetAsync(q_off, 0, sizeof(u64), st));
    else GT_TRY(gtars_tokenize_device(ix, qc, qs, qe, nq, q_off, d_ids, cap, nullptr, st));
    // scanning the clipped lengths needs them to fit the scan's u32 counts
    const bool clip = max_len && max_len <= 0xFFFFFFFFull;
    u32 *cnt;
    u64 *srcw, *scan, scanned = 0;
    SetStats *d_stats;
    GT_TRY(fr.alloc(&cnt, (size_t)B));
    GT_TRY(fr.alloc(&srcw, (size_t)B));
    GT_TRY(fr.alloc(&d_stats, 1));
    SetStats *h = (SetStats *)fr.host(sizeof(SetStats));
    if (!h) return fail(GTARS_ERR_INTERNAL, "out of host memory");
    GT_HIP(hipMemsetAsync(d_stats, 0, sizeof(SetStats), st));
    {
        ProfScope ps("k_set_lengths", st);
        hipLaunchKernelGGL(k_set_lengths, dim3(grid_for(B, TB_TPB, TB_MAX_BLOCKS)), dim3(TB_TPB), 0, st, q_off, nq, d_set_off, B, max_len, clip,
                           cnt, srcw, d_stats);
        GT_HIP(hipGetLastError());
    }
    GT_TRY(fr.download(h, d_stats, 1));
    GT_TRY(scan_total(fr, cnt, B, &scan, &scanned));  // (drains: the statistics and the total arrive together)
    const u64 raw = h->raw;
    if (h->bad) return fail(GTARS_ERR_INVALID_ARG, "set_offsets must start at 0, never descend and end at the number of regions");
    if (!clip && h->n_clipped)
        return fail(GTARS_ERR_INVALID_ARG, "max_length of 2^32 or more with a longer set: not supported");
    hipLaunchKernelGGL(k_set_offsets, dim3(grid_for((u64)B + 1, TB_TPB, TB_MAX_BLOCKS)), dim3(TB_TPB), 0, st, q_off, d_set_off, scan, B, clip,
                       d_out_off);
    GT_HIP(hipGetLastError());
    *total = clip ? scanned : raw + scanned;
    *longest = h->longest;
    if (!d_ids) return fr.drain();
    if (*total > cap) {
        GT_TRY(fr.drain());
        return too_small(*total);
    }
    if (!h->n_empty && !h->n_clipped) return fr.drain();  // the raw ids are the result, and they are where it belongs
    u32 *src;
    GT_TRY(fr.alloc(&src, (size_t)raw));
    if (raw > cap) GT_TRY(gtars_fill_device_n(ix, qc, qs, qe, nq, q_off, src, raw, st));
    else if (raw) GT_HIP(hipMemcpyAsync(src, d_ids, (size_t)raw * sizeof(u32), hipMemcpyDeviceToDevice, st));
    {
        ProfScope ps("k_set_pack", st);
        hipLaunchKernelGGL(k_set_pack, dim3(grid_for(*total, TOKBATCH_PACK_TILE, TB_MAX_BLOCKS)), dim3(TB_TPB), 0, st, d_out_off, srcw, src, B,
                           *total, unk, d_ids);
        GT_HIP(hipGetLastError());
    }
    return fr.drain();
}

gtars_status check_side(int side) {
    if (side != GTARS_PAD_RIGHT && side != GTARS_PAD_LEFT) return fail(GTARS_ERR_INVALID_ARG, "unknown padding side");
    return GTARS_OK;
}

// n_sets * width cells: they and their bytes must be countable
gtars_status check_cells(u64 n_sets, u64 width) {
    if (n_sets > TOKBATCH_MAX_SETS) return fail(GTARS_ERR_INVALID_ARG, "too many region sets in one batch (" + std::to_string(n_sets) + ")");
    if (width > 0xFFFFFFFFull || (n_sets && width > (SIZE_MAX / sizeof(u32) - 64) / n_sets))
        return fail(GTARS_ERR_INVALID_ARG, "n_sets * width overflows (" + std::to_string(n_sets) + " x " + std::to_string(width) + ")");
    return GTARS_OK;
}

gtars_status pad_on(StreamFrame &fr, const u64 *d_out_off, const u32 *d_ids, u64 n_sets, u64 width, u32 pad, int side, u32 *d_input_ids,
                    u8 *d_mask) {
    GT_TRY(check_side(side));
    GT_TRY(check_cells(n_sets, width));
    const u64 cells = n_sets * width;
    if (!cells) {
        // (a width of 0 holds no set: every set has an id)
        return n_sets ? fail(GTARS_ERR_INVALID_ARG, "width 0 cannot hold a set: every set has at least one id") : GTARS_OK;
    }
    SetStats *d_stats;
    GT_TRY(fr.alloc(&d_stats, 1));
    SetStats *h = (SetStats *)fr.host(sizeof(SetStats));
    if (!h) return fail(GTARS_ERR_INTERNAL, "out of host memory");
    GT_HIP(hipMemsetAsync(d_stats, 0, sizeof(SetStats), fr.st));
    {
        ProfScope ps("k_set_pad", fr.st);
        hipLaunchKernelGGL(k_set_pad, dim3(grid_for(cells, TB_TPB, TB_MAX_BLOCKS)), dim3(TB_TPB), 0, fr.st, d_out_off, d_ids, (u32)n_sets,
                           (u32)width, pad, side == GTARS_PAD_LEFT, d_input_ids, d_mask, d_stats);
        GT_HIP(hipGetLastError());
    }
    GT_TRY(fr.download(h, d_stats, 1));
    GT_TRY(fr.drain());
    if (h->too_wide) return fail(GTARS_ERR_INVALID_ARG, "a set is longer than the width " + std::to_string(width) + ": nothing is cut silently");
    return GTARS_OK;
}

template <class T>
gtars_status host_array(T **out, u64 n) {
    if (n > SIZE_MAX / sizeof(T) - 1) return fail(GTARS_ERR_INVALID_ARG, "result too large");
    *out = (T *)malloc(std::max<size_t>((size_t)n, 1) * sizeof(T));
    return *out ? GTARS_OK : fail(GTARS_ERR_INTERNAL, "out of host memory");
}

}  // namespace

gtars_status tokbatch_check_offsets(const uint64_t *set_offsets, uint64_t n_sets, uint64_t n) {
    if (!set_offsets) return fail(GTARS_ERR_INVALID_ARG, "set_offsets is NULL");
    if (n_sets > TOKBATCH_MAX_SETS) return fail(GTARS_ERR_INVALID_ARG, "too many region sets in one batch (" + std::to_string(n_sets) + ")");
    if (set_offsets[0] != 0) return fail(GTARS_ERR_INVALID_ARG, "set_offsets must start at 0");
    for (u64 b = 0; b < n_sets; ++b)
        if (set_offsets[b] > set_offsets[b + 1]) return fail(GTARS_ERR_INVALID_ARG, "set_offsets must never descend");
    if (set_offsets[n_sets] != n) return fail(GTARS_ERR_INVALID_ARG, "set_offsets must end at the number of regions");
    return GTARS_OK;
}

gtars_status tokbatch_encode(const gtars_index_t *ix, const uint32_t *chrom, const uint32_t *start, const uint32_t *end, uint64_t n,
                             const uint64_t *set_offsets, uint64_t n_sets, uint32_t unk_id, uint64_t max_length, bool ragged,
                             bool padded, uint64_t width_or_0, int side, uint32_t pad_id, TokBatchOut &out) {
    GT_TRY(require_device());
    if (!ix) return fail(GTARS_ERR_INVALID_ARG, "NULL handle");
    if (n && (!chrom || !start || !end)) return fail(GTARS_ERR_INVALID_ARG, "NULL query arrays");
    GT_TRY(tokbatch_check_offsets(set_offsets, n_sets, n));
    if (padded) {
        GT_TRY(check_side(side));
        GT_TRY(check_cells(n_sets, width_or_0));
    }
    DeviceScope on(gtars_index_device(ix));
    GT_TRY(on.st);
    StreamFrame fr(nullptr);  // (behind `out`, whose arrays the frame's copies write)
    u32 *qc, *qs, *qe, *d_ids;
    u64 *d_set_off, *d_out_off;
    GT_TRY(fr.upload(&qc, chrom, (size_t)n));
    GT_TRY(fr.upload(&qs, start, (size_t)n));
    GT_TRY(fr.upload(&qe, end, (size_t)n));
    GT_TRY(fr.upload(&d_set_off, set_offsets, (size_t)n_sets + 1));
    GT_TRY(fr.alloc(&d_out_off, (size_t)n_sets + 1));
    // a guess of two ids per region and an [unk] per set; once more with the exact size where that is short
    u64 cap = n * 2 + n_sets + 1024;
    GT_TRY(fr.alloc(&d_ids, (size_t)cap));
    gtars_status st = sets_on(fr, ix, qc, qs, qe, n, d_set_off, n_sets, unk_id, max_length, d_out_off, d_ids, cap, &out.total, &out.longest);
    if (st == GTARS_ERR_CAPACITY) {
        cap = out.total;
        GT_TRY(fr.alloc(&d_ids, (size_t)cap));
        st = sets_on(fr, ix, qc, qs, qe, n, d_set_off, n_sets, unk_id, max_length, d_out_off, d_ids, cap, &out.total, &out.longest);
    }
    GT_TRY(st);
    if (ragged) {
        GT_TRY(host_array(&out.offsets, n_sets + 1));
        GT_TRY(host_array(&out.ids, out.total));
        GT_TRY(fr.download(out.offsets, d_out_off, (size_t)n_sets + 1));
        GT_TRY(fr.download(out.ids, d_ids, (size_t)out.total));
    }
    if (padded) {
        if (width_or_0 && width_or_0 < out.longest)
            return fail(GTARS_ERR_INVALID_ARG, "width " + std::to_string(width_or_0) + " is smaller than the longest set (" +
                                                   std::to_string(out.longest) + " ids): nothing is cut silently");
        out.width = width_or_0 ? width_or_0 : out.longest;
        GT_TRY(check_cells(n_sets, out.width));
        const u64 cells = n_sets * out.width;
        u32 *d_input;
        u8 *d_mask;
        GT_TRY(fr.alloc(&d_input, (size_t)cells));
        GT_TRY(fr.alloc(&d_mask, (size_t)cells));
        GT_TRY(pad_on(fr, d_out_off, d_ids, n_sets, out.width, pad_id, side, d_input, d_mask));
        GT_TRY(host_array(&out.input_ids, cells));
        GT_TRY(host_array(&out.mask, cells));
        GT_TRY(fr.download(out.input_ids, d_input, (size_t)cells));
        GT_TRY(fr.download(out.mask, d_mask, (size_t)cells));
    }
    return fr.drain();
}

}  // namespace gtars

using namespace gtars;

extern "C" {

gtars_status gtars_tokenize_sets_device(const gtars_index_t *ix, const uint32_t *d_qchrom, const uint32_t *d_qstart,
                                        const uint32_t *d_qend, uint64_t nq, const uint64_t *d_set_offsets, uint64_t n_sets,
                                        uint32_t unk_id, uint64_t max_length, uint64_t *d_out_offsets, uint32_t *d_out_ids,
                                        uint64_t ids_capacity, uint64_t *total, uint64_t *longest, void *stream) {
    return guarded([&]() -> gtars_status {
        GT_TRY(require_device());
        if (!ix) return fail(GTARS_ERR_INVALID_ARG, "NULL handle");
        if (nq && (!d_qchrom || !d_qstart || !d_qend)) return fail(GTARS_ERR_INVALID_ARG, "NULL query arrays");
        if (!d_set_offsets || !d_out_offsets) return fail(GTARS_ERR_INVALID_ARG, "NULL set offsets");
        GT_TRY(require_handle_device(gtars_index_device(ix)));
        u64 t = 0, l = 0;
        StreamFrame fr((hipStream_t)stream);
        const gtars_status st = sets_on(fr, ix, d_qchrom, d_qstart, d_qend, nq, d_set_offsets, n_sets, unk_id, max_length, d_out_offsets,
                                        d_out_ids, ids_capacity, &t, &l);
        if (total) *total = t;
        if (longest) *longest = l;
        return st;
    });
}

gtars_status gtars_pad_sets_device(const uint64_t *d_out_offsets, const uint32_t *d_out_ids, uint64_t n_sets, uint64_t width,
                                   uint32_t pad_id, int side, uint32_t *d_input_ids, uint8_t *d_mask, void *stream) {
    return guarded([&]() -> gtars_status {
        GT_TRY(require_device());
        if (n_sets && (!d_out_offsets || !d_out_ids)) return fail(GTARS_ERR_INVALID_ARG, "NULL ragged input");
        if (n_sets && width && (!d_input_ids || !d_mask)) return fail(GTARS_ERR_INVALID_ARG, "NULL output");
        StreamFrame fr((hipStream_t)stream);
        return pad_on(fr, d_out_offsets, d_out_ids, n_sets, width, pad_id, side, d_input_ids, d_mask);
    });
}

uint32_t gtars_debug_tokbatch_tile(void) { return TOKBATCH_PACK_TILE; }

}  // extern "C"
