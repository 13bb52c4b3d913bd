// reftx.hip -- K19: transcripts of a .reftx store over a genome assembly that is resident on the device
// (gtars-refget/src/transcripts/mapper.rs:239-475, sequence.rs:36-127).  Every query and every transcript is independent; the
// assembly is the packed image of K12 (seqstats.h: the bytes as the file has them, read here upper-cased), the store is a set
// of flat tables uploaded once per binding (reftx_core.h: TxTables).
//
//   * k_tx_map, one lane per query: tx_map_one of reftx_core.h, the same text the host path runs.  The exon of a position is
//     found by binary search of the transcript's slice; the reference scans the exons, and the answers are the same because
//     the exons of a transcript the tables accept are ascending and disjoint.
//   * k_tx_rows + the scan of kernels.hip + k_tx_fill: the mature sequences as a byte CSR, eight output bytes per lane; a
//     lane finds its row and its exon by search and walks across exon and row ends.
//   * k_tx_digest, one lane per transcript: sha512t24u of the mature sequence through sha512_stream (sha512.h) from a source
//     that walks the exons forward, or backward with the complement.  Nothing is staged in memory.  Lanes take the rows in
//     ascending order of their lengths (sort_perm), so the 64 transcripts of a wave need about the same number of blocks.
//     Transcripts longer than GTARS_TX_HOST_LEN bytes are listed for the host instead: tx_seq_run hashes them with the same
//     header on the host threads and writes the results into the device column.
#include <cstring>

#include "common.h"
#include "host_threads.h"
#include "pipeline.h"
#include "reftx.h"
#include "sha512.h"

namespace gtars {

struct TxDevice {
    DevBuf<u32> exon_off, g_start, g_end, tx_start, chrom, cds_lo, cds_hi, len;
    DevBuf<int8_t> strand;
    DevBuf<u8> bad, seq_status;
    u32 n_tx = 0;
    TxTables view() const {
        TxTables t;
        t.exon_off = exon_off.p, t.g_start = g_start.p, t.g_end = g_end.p, t.tx_start = tx_start.p, t.chrom = chrom.p;
        t.strand = strand.p, t.cds_lo = cds_lo.p, t.cds_hi = cds_hi.p, t.len = len.p, t.bad = bad.p, t.seq_status = seq_status.p;
        t.n_tx = n_tx;
        return t;
    }
};

namespace {

constexpr int TX_TPB = 256;
constexpr u32 TX_MAX_BLOCKS = 256 * 8;
constexpr u64 TX_MAX_N = 0x7FFFFFF0u;

__global__ void __launch_bounds__(TX_TPB)
k_tx_map(TxTables t, const u32 *__restrict__ tx, const u8 *__restrict__ kind, const i64 *__restrict__ pos, const i64 *__restrict__ off,
         const u8 *__restrict__ star, u64 n, u64 *__restrict__ out, u8 *__restrict__ status) {
    for (u64 i = (u64)blockIdx.x * TX_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * TX_TPB) {
        u64 r;
        const u8 st = tx_map_one(t, tx[i], kind[i], pos[i], off ? off[i] : 0, star ? star[i] : 0u, &r);
        out[i] = r;
        status[i] = st;
    }
}

// per row: its status and the bytes of its sequence (0 for a row that failed)
__global__ void __launch_bounds__(TX_TPB)
k_tx_rows(TxTables t, const u32 *__restrict__ idx, u64 n, u8 *__restrict__ status, u32 *__restrict__ cnt) {
    for (u64 i = (u64)blockIdx.x * TX_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * TX_TPB) {
        const u32 tx = idx[i];
        const u8 st = tx < t.n_tx ? t.seq_status[tx] : (u8)TXSEQ_NOT_FOUND;
        status[i] = st;
        cnt[i] = st == TXSEQ_OK ? t.len[tx] : 0;
    }
}

__global__ void __launch_bounds__(TX_TPB)
k_tx_digest(TxTables t, const u8 *__restrict__ seq, const u64 *__restrict__ coff, const u32 *__restrict__ idx, const u32 *__restrict__ perm,
            const u8 *__restrict__ status, u32 n, u32 host_len, u64 *__restrict__ out, u32 *__restrict__ host_list, u32 *__restrict__ n_host) {
    for (u64 w = (u64)blockIdx.x * TX_TPB + threadIdx.x; w < n; w += (u64)gridDim.x * TX_TPB) {
        const u32 i = perm[w];
        u64 *dst = out + (u64)i * 4;
        if (status[i] != TXSEQ_OK) {
            dst[0] = dst[1] = dst[2] = dst[3] = 0;
            continue;
        }
        const u32 tx = idx[i];
        const u32 len = t.len[tx];
        if (len > host_len) {
            host_list[atomicAdd(n_host, 1u)] = i;
            continue;
        }
        // (an empty transcript needs no chromosome and may have none)
        TxSeqSrc src{tx_exons(t, tx), len ? seq + coff[t.chrom[tx]] : seq};
        Sha512 sh;
        sha512_stream(sh, src, (u64)len);
        u64 text[4];
        sha512t24u_words(sh, text);
        // (the text's first character first in memory)
        dst[0] = __builtin_bswap64(text[0]), dst[1] = __builtin_bswap64(text[1]);
        dst[2] = __builtin_bswap64(text[2]), dst[3] = __builtin_bswap64(text[3]);
    }
}

__global__ void __launch_bounds__(TX_TPB)
k_tx_fill(TxTables t, const u8 *__restrict__ seq, const u64 *__restrict__ coff, const u32 *__restrict__ idx, u32 n,
          const u64 *__restrict__ off, u64 total, u8 *__restrict__ out) {
    const u64 groups = (total + 7) >> 3;
    for (u64 g = (u64)blockIdx.x * TX_TPB + threadIdx.x; g < groups; g += (u64)gridDim.x * TX_TPB) {
        const u64 q0 = g << 3;
        const u64 q_end = min(q0 + 8, total);
        // the row of byte q0: the last r with off[r] <= q0 whose sequence is not empty
        u32 lo = 0, hi = n;
        while (hi - lo > 1) {
            const u32 m = lo + ((hi - lo) >> 1);
            if (off[m] <= q0) lo = m;
            else hi = m;
        }
        u32 r = lo, k = 0;
        bool new_row = true;
        TxExons x{};
        const u8 *chrom_seq = nullptr;
        u64 ts = 0, te = 0, word = 0;
        for (u64 q = q0; q < q_end; ++q) {
            while (off[r + 1] <= q) ++r, new_row = true;  // (q < total = off[n]: stops inside the table)
            const u64 p = q - off[r];
            if (new_row || p >= te) {
                if (new_row) {
                    const u32 tx = idx[r];  // (a row with bytes has status 0: the index and its chromosome are valid)
                    x = tx_exons(t, tx);
                    chrom_seq = seq + coff[t.chrom[tx]];
                    new_row = false;
                }
                k = x.at(tx_exon_of(x, p));
                ts = x.ts[k], te = ts + (x.ge[k] - x.gs[k]);
            }
            word |= (u64)tx_base(x, chrom_seq, k, p - ts) << (8 * (q - q0));
        }
        if (q_end - q0 == 8) *(u64 *)(out + q0) = word;  // (out comes from the allocator and q0 is a multiple of 8)
        else
            for (u64 q = q0; q < q_end; ++q) out[q] = (u8)(word >> (8 * (q - q0)));
    }
}

template <class T>
gtars_status bring(StreamFrame &fr, bool on_device, const T *src, size_t n, const T **out) {
    if (on_device || !src) {
        *out = src;
        return GTARS_OK;
    }
    T *d;
    GT_TRY(fr.upload(&d, src, n));
    *out = d;
    return GTARS_OK;
}

gtars_status check_device(const AssemblyParts &ap, bool on_device) {
    if (ap.device < 0) return fail(GTARS_ERR_INTERNAL, "reftx: the assembly has no device image");
    if (!on_device) return GTARS_OK;
    int cur = -1;
    GT_HIP(hipGetDevice(&cur));
    if (cur != ap.device)
        return fail(GTARS_ERR_INVALID_ARG, "handle lives on device " + std::to_string(ap.device) + ", current device is " + std::to_string(cur) +
                                               ": device pointers and stream must belong to the handle's device");
    return GTARS_OK;
}

}  // namespace

gtars_status tx_device_build(const Assembly &a, const TxHostTables &h, TxDevice **out) {
    *out = nullptr;
    const AssemblyParts ap = assembly_parts(a);
    if (ap.device < 0) return fail(GTARS_ERR_INTERNAL, "reftx: the assembly has no device image");
    DeviceScope on(ap.device);
    GT_TRY(on.st);
    TxDevice *d = new TxDevice();
    d->n_tx = (u32)h.len.size();
    gtars_status st = GTARS_OK;
    auto up = [&](auto &buf, const auto &vec) {
        if (!st) st = buf.upload(vec);
    };
    up(d->exon_off, h.exon_off), up(d->g_start, h.g_start), up(d->g_end, h.g_end), up(d->tx_start, h.tx_start), up(d->chrom, h.chrom);
    up(d->cds_lo, h.cds_lo), up(d->cds_hi, h.cds_hi), up(d->len, h.len), up(d->strand, h.strand), up(d->bad, h.bad), up(d->seq_status, h.seq_status);
    if (st) {
        delete d;
        return st;
    }
    *out = d;
    return GTARS_OK;
}

void tx_device_free(TxDevice *d) { delete d; }
TxTables tx_device_view(const TxDevice &d) { return d.view(); }

gtars_status tx_map_run(const Assembly &a, const TxDevice &d, const TxMapCall &call) {
    const AssemblyParts ap = assembly_parts(a);
    GT_TRY(check_device(ap, call.on_device));
    if (call.n > TX_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "reftx: too many queries (" + std::to_string(call.n) + ")");
    if (!call.n) return GTARS_OK;
    if (!call.tx || !call.kind || !call.pos || !call.out || !call.status) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    DeviceScope on(call.on_device ? -1 : ap.device);
    GT_TRY(on.st);
    StreamFrame fr(call.on_device ? (hipStream_t)call.stream : nullptr);
    const size_t n = (size_t)call.n;
    const u32 *tx;
    const u8 *kind, *star;
    const i64 *pos, *off;
    GT_TRY(bring(fr, call.on_device, call.tx, n, &tx));
    GT_TRY(bring(fr, call.on_device, call.kind, n, &kind));
    GT_TRY(bring(fr, call.on_device, call.pos, n, &pos));
    GT_TRY(bring(fr, call.on_device, call.off, n, &off));
    GT_TRY(bring(fr, call.on_device, call.star, n, &star));
    u64 *out = call.out;
    u8 *status = call.status;
    if (!call.on_device) {
        GT_TRY(fr.alloc(&out, n));
        GT_TRY(fr.alloc(&status, n));
    }
    {
        ProfScope ps("k_tx_map", fr.st);
        hipLaunchKernelGGL(k_tx_map, dim3(grid_for(n, TX_TPB, TX_MAX_BLOCKS)), dim3(TX_TPB), 0, fr.st, d.view(), tx, kind, pos, off, star, (u64)n,
                           out, status);
        GT_HIP(hipGetLastError());
    }
    if (!call.on_device) {
        GT_TRY(fr.download(call.out, out, n));
        GT_TRY(fr.download(call.status, status, n));
    }
    return fr.drain();
}

gtars_status tx_seq_run(const Assembly &a, const TxDevice &d, const TxSeqCall &call) {
    const AssemblyParts ap = assembly_parts(a);
    GT_TRY(check_device(ap, call.on_device));
    if (call.n > TX_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "reftx: too many transcripts (" + std::to_string(call.n) + ")");
    if ((call.seq_off == nullptr) != (call.seq_bytes == nullptr)) return fail(GTARS_ERR_INVALID_ARG, "reftx: sequences need both vectors");
    if (call.seq_off) call.seq_off->assign(1, 0), call.seq_bytes->clear();
    if (!call.n) return GTARS_OK;
    if (!call.idx) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    if (call.on_device && call.digest && ((uintptr_t)call.digest & 7))
        return fail(GTARS_ERR_INVALID_ARG, "reftx: the device digests must be 8-byte aligned");
    DeviceScope on(call.on_device ? -1 : ap.device);
    GT_TRY(on.st);
    StreamFrame fr(call.on_device ? (hipStream_t)call.stream : nullptr);
    hipStream_t st = fr.st;
    const size_t n = (size_t)call.n;
    // (a negative or unreadable value is the default; 2^30 bounds the u32 the kernel compares with)
    const long host_len_cfg = cfg_int("GTARS_TX_HOST_LEN", 65536);
    const u32 host_len = (u32)std::min(host_len_cfg < 0 ? 65536l : host_len_cfg, 0x40000000l);
    const TxTables t = d.view();
    const u32 *idx;
    GT_TRY(bring(fr, call.on_device, call.idx, n, &idx));
    u8 *status;
    u32 *cnt;
    if (call.on_device && call.status) status = call.status;
    else GT_TRY(fr.alloc(&status, n));
    GT_TRY(fr.alloc(&cnt, n));
    const unsigned grid = grid_for(n, TX_TPB, TX_MAX_BLOCKS);
    {
        ProfScope ps("k_tx_rows", st);
        hipLaunchKernelGGL(k_tx_rows, dim3(grid), dim3(TX_TPB), 0, st, t, idx, (u64)n, status, cnt);
        GT_HIP(hipGetLastError());
    }
    if (call.digest) {
        u64 *d_digest;
        if (call.on_device) d_digest = (u64 *)call.digest;
        else GT_TRY(fr.alloc(&d_digest, 4 * n));
        u32 *perm, *host_list, *n_host;
        GT_TRY(sort_perm(fr, nullptr, cnt, nullptr, (u32)n, 1, &perm));
        GT_TRY(fr.alloc(&host_list, n));
        GT_TRY(fr.alloc(&n_host, 1));
        GT_HIP(hipMemsetAsync(n_host, 0, sizeof(u32), st));
        {
            ProfScope ps("k_tx_digest", st);
            hipLaunchKernelGGL(k_tx_digest, dim3(grid), dim3(TX_TPB), 0, st, t, ap.seq, ap.off, idx, perm, status, (u32)n, host_len, d_digest,
                               host_list, n_host);
            GT_HIP(hipGetLastError());
        }
        u32 *h_n = (u32 *)fr.host(sizeof(u32));
        if (!h_n) return fail(GTARS_ERR_INTERNAL, "out of host memory");
        GT_TRY(fr.download(h_n, n_host, 1));
        GT_TRY(fr.drain());
        if (const u32 n_list = *h_n) {
            // the host tail: the rows and their transcript indexes come back, the digests go up
            if (!call.h_tables || !call.h_seq) return fail(GTARS_ERR_INTERNAL, "reftx: the host tail needs the host tables");
            std::vector<u32> rows, txs(n_list);
            GT_TRY(fr.download(rows, host_list, n_list));
            GT_TRY(fr.drain());
            for (u32 k = 0; k < n_list; ++k) GT_TRY(fr.download(&txs[k], idx + rows[k], 1));
            GT_TRY(fr.drain());
            std::vector<char> text((size_t)n_list * 32);
            const TxTables &h = *call.h_tables;
            parallel_for(n_list, call.threads, 1, [&](size_t k) { tx_digest(h, txs[k], call.h_seq[h.chrom[txs[k]]], &text[k * 32]); });
            for (u32 k = 0; k < n_list; ++k) GT_TRY(fr.upload_to((char *)(d_digest + 4 * (size_t)rows[k]), &text[(size_t)k * 32], 32));
            GT_TRY(fr.drain());
        }
        if (!call.on_device) GT_TRY(fr.download(call.digest, (const char *)d_digest, 32 * n));
    }
    if (call.seq_off) {
        u64 *off, total = 0;
        GT_TRY(scan_total(fr, cnt, n, &off, &total));
        GT_TRY(fr.download(*call.seq_off, off, n + 1));
        call.seq_bytes->resize((size_t)total);
        if (total) {
            u8 *d_bytes;
            GT_TRY(fr.alloc(&d_bytes, (size_t)total));
            {
                ProfScope ps("k_tx_fill", st);
                hipLaunchKernelGGL(k_tx_fill, dim3(grid_for((total + 7) >> 3, TX_TPB, TX_MAX_BLOCKS)), dim3(TX_TPB), 0, st, t, ap.seq, ap.off,
                                   idx, (u32)n, off, total, d_bytes);
                GT_HIP(hipGetLastError());
            }
            GT_TRY(fr.download(call.seq_bytes->data(), d_bytes, (size_t)total));
        }
    }
    if (!(call.on_device && call.status) && call.status) GT_TRY(fr.download(call.status, status, n));
    return fr.drain();
}

}  // namespace gtars
