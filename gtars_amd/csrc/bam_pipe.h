// bam_pipe.h -- K17's window pipeline for the HIP translation units that read BAM records on the device:
// bam.hip (columns, QC) and bam_frag.hip (K26).  The handle, the loads that are valid at any byte address, the decoded columns,
// k_bam_decode, BamPipe, and the small helpers both users share.  Everything here has internal linkage but the stage times.
#pragma once

#include <chrono>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "bam.h"
#include "pipeline.h"
#include "scan.h"

struct gtars_bam {
    gtars::BamFile f;
    double t_open = 0;
};

namespace gtars {

// gtars_bam_last_stages: open (read + block table + header) | inflate | record walk | windows | records | wall of the call, seconds
// (bam.hip defines it)
extern thread_local double g_bam_stages[6];

namespace {

inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// loads that are valid at any byte address: a record starts wherever the one before it ended
__device__ __forceinline__ u32 ld16(const u8 *p) { return (u32)p[0] | ((u32)p[1] << 8); }
__device__ __forceinline__ u32 ld32(const u8 *p) { return ld16(p) | (ld16(p + 2) << 16); }

// the decoded columns of one window: 11 arrays of `cap` words in one allocation
constexpr int BAM_NCOL = 11;
constexpr u32 FLAG_NAME_MISSING = 1u << 16;  // beside the 16 flag bits: the name is stored as "*"
struct BamCols {
    i32 *ref, *pos, *end, *mapq, *lseq, *tlen;
    u32 *flag, *noff, *nlen, *hhi, *hlo;  // noff: the name's offset in the window's bytes; nlen: without the NUL
};
inline BamCols cols_of(u32 *p, size_t cap) {
    BamCols c;
    c.ref = (i32 *)p, c.pos = (i32 *)(p + cap), c.end = (i32 *)(p + 2 * cap), c.mapq = (i32 *)(p + 3 * cap);
    c.lseq = (i32 *)(p + 4 * cap), c.tlen = (i32 *)(p + 5 * cap);
    c.flag = p + 6 * cap, c.noff = p + 7 * cap, c.nlen = p + 8 * cap, c.hhi = p + 9 * cap, c.hlo = p + 10 * cap;
    return c;
}

// One lane per record.  offs[i]: the record's block_size field; the host's walk has checked that the whole record lies inside
// the window, this kernel checks that name and CIGAR lie inside the record (err otherwise, and neither is read).
__global__ void __launch_bounds__(256)
k_bam_decode(const u8 *__restrict__ bytes, const u32 *__restrict__ offs, u32 n, BamCols c, u64 hash_mask, u32 *__restrict__ err) {
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u8 *p = bytes + offs[i];
        const u32 bs = ld32(p);
        p += 4;
        const i32 pos = (i32)ld32(p + 4);
        u32 l_name = p[8], n_cigar = ld16(p + 12);
        u32 flag = ld16(p + 14);
        if (32ull + l_name + 4ull * n_cigar > bs) {
            atomicOr(err, 1u);
            l_name = 0, n_cigar = 0;
        }
        const u8 *name = p + 32;
        const u32 nlen = l_name ? l_name - 1 : 0;
        u64 h = 0xcbf29ce484222325ull;  // FNV-1a over the name, then a mix so that every kept bit depends on every byte
        for (u32 k = 0; k < nlen; ++k) h = (h ^ name[k]) * 0x100000001b3ull;
        h ^= h >> 32;
        h *= 0xd6e8feb86659fd93ull;
        h ^= h >> 32;
        h &= hash_mask;
        if (nlen == 1 && name[0] == '*') flag |= FLAG_NAME_MISSING;
        // the reference span of the in-record CIGAR: M, D, N, = and X consume reference (a CIGAR kept in a CG tag leaves kSmN
        // here, whose N carries the span)
        const u8 *cg = name + l_name;
        u32 span = 0;
        for (u32 k = 0; k < n_cigar; ++k) {
            const u32 v = ld32(cg + 4 * k), op = v & 15u;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += v >> 4;
        }
        c.ref[i] = (i32)ld32(p);
        c.pos[i] = pos;
        c.end[i] = (i32)((u32)pos + span);
        c.mapq[i] = p[9];
        c.lseq[i] = (i32)ld32(p + 16);
        c.tlen[i] = (i32)ld32(p + 28);
        c.flag[i] = flag;
        c.noff[i] = offs[i] + 36;
        c.nlen[i] = nlen;
        c.hhi[i] = (u32)(h >> 32);
        c.hlo[i] = (u32)h;
    }
}

// ---- the window pipeline ------------------------------------------------------------------------------------------------
// Window k: whole BGZF blocks of at most max_window inflated bytes (one block at least; the first window also holds every block
// the header reaches into), behind the bytes of the record the window before it cut.  Two pinned buffers, one stream: while
// window k is copied and decoded, the host threads inflate window k + 1.
struct BamPipe {
    const BamFile &f;
    u64 max_window;
    unsigned threads;
    hipStream_t st;
    HostBlock hb[2];
    size_t hn[2] = {0, 0};
    std::vector<u32> offs[2];
    BamSegs segs[2];
    u64 next_block = 0;
    BamWalk walk;
    DevBuf<u8> d_bytes;
    DevBuf<u32> d_offs, d_cols, d_err;
    size_t cols_cap = 0;
    double t_inflate = 0, t_walk = 0;
    u64 n_windows = 0;

    BamPipe(const BamFile &file, u64 mw, unsigned nt, hipStream_t s) : f(file), max_window(mw), threads(nt), st(s) {}
    ~BamPipe() { (void)hipStreamSynchronize(st); }  // (before the buffers go: copies and kernels may still be queued)

    gtars_status fill(int b, const u8 *carry, size_t carry_n) {
        const double t0 = now_s();
        const u64 nb = f.blocks.size(), b0 = next_block;
        u64 b1 = b0, bytes = 0;
        while (b1 < nb && (b1 == b0 || bytes + f.blocks[b1].isize <= max_window || f.blocks[b1].uoff < f.first_record)) bytes += f.blocks[b1++].isize;
        const u64 need = carry_n + bytes;
        if (need > 0xF0000000ull) return fail(GTARS_ERR_INVALID_ARG, "BAM window of " + std::to_string(need) + " bytes: max_window_bytes is too large");
        if (hb[b].cap < need + 16 && !hb[b].alloc(need + need / 4 + 64)) return fail(GTARS_ERR_INTERNAL, "out of host memory");
        if (carry_n) memcpy(hb[b].p, carry, carry_n);
        GT_TRY(bam_inflate(f, b0, b1, (u8 *)hb[b].p + carry_n, threads));
        hn[b] = need;
        next_block = b1;
        t_inflate += now_s() - t0;
        return GTARS_OK;
    }

    // finish(cols, n, segs, index of the window's first record, the window's bytes on the device): runs after the next window
    // has been inflated; whatever it queues is drained before the buffers are used again
    template <class Fin>
    gtars_status run(Fin &&finish) {
        GT_TRY(d_err.alloc(1));
        GT_HIP(hipMemsetAsync(d_err.p, 0, 4, st));
        const u64 hash_bits = (u64)std::min<long>(std::max<long>(cfg_int("GTARS_BAM_NAME_HASH_BITS", 64), 0), 64);
        const u64 hash_mask = hash_bits >= 64 ? ~0ull : (1ull << hash_bits) - 1ull;
        int cur = 0;
        GT_TRY(fill(0, nullptr, 0));
        for (bool first = true;; first = false, cur ^= 1) {
            const bool final = next_block == f.blocks.size();
            const u8 *data = (const u8 *)hb[cur].p;
            offs[cur].clear(), segs[cur].start.clear(), segs[cur].ref.clear();
            const u64 rec0 = walk.n_records;
            u64 consumed = 0;
            const double t0 = now_s();
            GT_TRY(bam_walk(data, hn[cur], first ? f.first_record : 0, final, (int64_t)f.refs.size(), walk, &offs[cur], nullptr, 0, &consumed,
                            &segs[cur]));
            t_walk += now_s() - t0;
            const u32 n = (u32)offs[cur].size();
            ++n_windows;
            if (n) {
                if (d_bytes.n < consumed) GT_TRY(d_bytes.alloc(consumed + consumed / 4));
                if (d_offs.n < n) GT_TRY(d_offs.alloc(n + n / 4));
                if (cols_cap < n) {
                    cols_cap = n + n / 4;
                    GT_TRY(d_cols.alloc(cols_cap * BAM_NCOL));
                }
                {
                    ProfScope p("bam_h2d", st);
                    GT_HIP(hipMemcpyAsync(d_bytes.p, data, consumed, hipMemcpyHostToDevice, st));
                    GT_HIP(hipMemcpyAsync(d_offs.p, offs[cur].data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
                }
                ProfScope p("k_bam_decode", st);
                hipLaunchKernelGGL(k_bam_decode, dim3(grid_for(n)), dim3(256), 0, st, d_bytes.p, d_offs.p, n, cols_of(d_cols.p, cols_cap), hash_mask,
                                   d_err.p);
                GT_HIP(hipGetLastError());
            }
            if (!final) GT_TRY(fill(cur ^ 1, data + consumed, hn[cur] - consumed));
            if (n) GT_TRY(finish(cols_of(d_cols.p, cols_cap), n, segs[cur], rec0, (const u8 *)d_bytes.p));
            u32 e = 0;
            GT_HIP(hipMemcpyAsync(&e, d_err.p, 4, hipMemcpyDeviceToHost, st));
            GT_HIP(hipStreamSynchronize(st));
            if (e)
                return fail(GTARS_ERR_PARSE, f.path + ": a BAM record among records " + std::to_string(rec0) + " .. " + std::to_string(rec0 + n - 1) +
                                                 " holds a name and CIGAR longer than its block_size");
            if (final) break;
        }
        g_bam_stages[1] = t_inflate, g_bam_stages[2] = t_walk, g_bam_stages[3] = (double)n_windows, g_bam_stages[4] = (double)walk.n_records;
        return GTARS_OK;
    }
};

// device array that keeps its first `used` elements when it grows
template <class T>
struct Grow {
    DevBuf<T> b;
    gtars_status ensure(size_t need, size_t used, hipStream_t st) {
        if (need <= b.n) return GTARS_OK;
        DevBuf<T> nb;
        GT_TRY(nb.alloc(std::max(need, b.n * 2)));
        if (used) GT_HIP(hipMemcpyAsync(nb.p, b.p, used * sizeof(T), hipMemcpyDeviceToDevice, st));
        GT_HIP(hipStreamSynchronize(st));
        b = std::move(nb);
        return GTARS_OK;
    }
};

// every lane of the wave calls this (after its loop, not inside it)
__device__ __forceinline__ void wave_add(u64 *dst, u64 v) {
    v = wave_reduce_sum_u64(v);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd((unsigned long long *)dst, (unsigned long long)v);
}

inline u64 window_bytes(u64 max_window_bytes) { return max_window_bytes ? max_window_bytes : 256ull << 20; }

}  // namespace
}  // namespace gtars
