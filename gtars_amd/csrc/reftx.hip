// reftx.hip -- K19: transcripts of a .reftx store over a genome assembly that is resident on the device
// (gtars-refget/src/transcripts/mapper.rs:239-475, sequence.rs:36-127).  Every query and every transcript is independent; the
// assembly is the packed image of K12 (seqstats.h: the bytes as the file has them, read here upper-cased), the store is a set
// of flat tables uploaded once per binding (reftx_core.h: TxTables).
//
//   * k_tx_map, one lane per query: tx_map_one of reftx_core.h, the same text the host path runs.  The exon of a position is
//     found by binary search of the transcript's slice; the reference scans the exons, and the answers are the same because
//     the exons of a transcript the tables accept are ascending and disjoint.
//   * k_tx_rows + the scan of kernels.hip + the fill of byte_csr.h over TxRowSrc (profiled as k_tx_fill): the mature
//     sequences as a byte CSR, eight output bytes per lane; a lane finds its row and its exon by search and walks across
//     exon and row ends.
//   * k_tx_digest, one lane per transcript: sha512t24u of the mature sequence through sha512_stream (sha512.h) from a source
//     that walks the exons forward, or backward with the complement.  Nothing is staged in memory.  Lanes take the rows in
//     ascending order of their lengths (sort_perm), so the 64 transcripts of a wave need about the same number of blocks.
//     Transcripts longer than GTARS_TX_HOST_LEN bytes are listed for the host instead: tx_seq_run hashes them with the same
//     header on the host threads and writes the results into the device column.
#include <cstring>

#include "byte_csr.h"
#include "common.h"
#include "host_threads.h"
#include "image_call.h"
#include "pipeline.h"
#include "reftx.h"
#include "reftx_image.h"
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

// a row of the CSR: a transcript's mature sequence, read through an exon cursor that moves when k passes the exon's end
struct TxRowSrc {
    TxTables t;
    const u8 *seq;
    const u64 *coff;
    const u32 *idx;
    TxExons x;  // of the open row
    const u8 *chrom_seq;
    u32 k;       // the exon that holds transcript positions [ts, te)
    u64 ts, te;
    __device__ __forceinline__ void open(u32 r) {
        const u32 tx = idx[r];  // (a row with bytes has status 0: the index and its chromosome are valid)
        x = tx_exons(t, tx);
        chrom_seq = seq + coff[t.chrom[tx]];
        ts = te = 0;  // (no exon yet: the first byte searches)
    }
    __device__ __forceinline__ u32 byte(u64 p) {
        if (p >= te) {
            k = x.at(tx_exon_of(x, p));
            ts = x.ts[k], te = ts + (x.ge[k] - x.gs[k]);
        }
        return tx_base(x, chrom_seq, k, p - ts);
    }
};

gtars_status check_device(const AssemblyParts &ap, bool on_device) {
    if (ap.device < 0) return fail(GTARS_ERR_INTERNAL, "reftx: the assembly has no device image");
    return on_device ? require_handle_device(ap.device) : GTARS_OK;
}

}  // namespace

// sha512t24u of rows' mature sequences into d_digest (four u64 per row; zero for a row whose status is not TXSEQ_OK), cnt:
// the rows' lengths as k_tx_rows leaves them.  The stream is drained when it returns.
gtars_status tx_digest_rows(StreamFrame &fr, const AssemblyParts &ap, const TxTables &t, const u32 *idx, const u32 *cnt, const u8 *status, u32 n,
                            u64 *d_digest, const TxTables *h_tables, const uint8_t *const *h_seq, unsigned threads) {
    hipStream_t st = fr.st;
    // (a negative or unreadable value is the default; 2^30 bounds the u32 the kernel compares with)
    const long host_len_cfg = cfg_int("GTARS_TX_HOST_LEN", 65536);
    const u32 host_len = (u32)std::min(host_len_cfg < 0 ? 65536l : host_len_cfg, 0x40000000l);
    u32 *perm, *host_list, *n_host;
    GT_TRY(sort_perm(fr, nullptr, cnt, nullptr, n, 1, &perm));
    GT_TRY(fr.alloc(&host_list, n));
    GT_TRY(fr.alloc(&n_host, 1));
    GT_HIP(hipMemsetAsync(n_host, 0, sizeof(u32), st));
    {
        ProfScope ps("k_tx_digest", st);
        hipLaunchKernelGGL(k_tx_digest, dim3(grid_for(n, TX_TPB, TX_MAX_BLOCKS)), dim3(TX_TPB), 0, st, t, ap.seq, ap.off, idx, perm, status, n,
                           host_len, d_digest, host_list, n_host);
        GT_HIP(hipGetLastError());
    }
    u32 *h_n = (u32 *)fr.host(sizeof(u32));
    if (!h_n) return fail(GTARS_ERR_INTERNAL, "out of host memory");
    GT_TRY(fr.download(h_n, n_host, 1));
    GT_TRY(fr.drain());
    if (const u32 n_list = *h_n) {
        // the host tail: the rows and their transcript indexes come back, the digests go up
        if (!h_tables || !h_seq) return fail(GTARS_ERR_INTERNAL, "reftx: the host tail needs the host tables");
        std::vector<u32> rows, txs(n_list);
        GT_TRY(fr.download(rows, host_list, n_list));
        GT_TRY(fr.drain());
        for (u32 k = 0; k < n_list; ++k) GT_TRY(fr.download(&txs[k], idx + rows[k], 1));
        GT_TRY(fr.drain());
        std::vector<char> text((size_t)n_list * 32);
        const TxTables &h = *h_tables;
        parallel_for(n_list, threads, 1, [&](size_t k) { tx_digest(h, txs[k], h_seq[h.chrom[txs[k]]], &text[k * 32]); });
        for (u32 k = 0; k < n_list; ++k) GT_TRY(fr.upload_to((char *)(d_digest + 4 * (size_t)rows[k]), &text[(size_t)k * 32], 32));
        GT_TRY(fr.drain());
    }
    return GTARS_OK;
}

// the rows' mature sequences back to back: row r at d_bytes[off[r], off[r + 1]); `name` is the launch's ProfScope entry
gtars_status tx_fill_rows(const char *name, StreamFrame &fr, const AssemblyParts &ap, const TxTables &t, const u32 *idx, const u64 *off, u32 n,
                          u64 total, u8 *d_bytes) {
    return csr_fill(name, TxRowSrc{t, ap.seq, ap.off, idx}, off, n, total, d_bytes, fr.st);
}

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
    ImageCall ic(ap, call.on_device, call.stream);
    GT_TRY(ic.scope.st);
    StreamFrame &fr = ic.fr;
    const size_t n = (size_t)call.n;
    const u32 *tx;
    const u8 *kind, *star;
    const i64 *pos, *off;
    GT_TRY(ic.in(call.tx, n, &tx));
    GT_TRY(ic.in(call.kind, n, &kind));
    GT_TRY(ic.in(call.pos, n, &pos));
    GT_TRY(ic.in(call.off, n, &off));
    GT_TRY(ic.in(call.star, n, &star));
    u64 *out;
    u8 *status;
    GT_TRY(ic.out(call.out, n, &out));
    GT_TRY(ic.out(call.status, n, &status));
    {
        ProfScope ps("k_tx_map", fr.st);
        hipLaunchKernelGGL(k_tx_map, dim3(grid_for(n, TX_TPB, TX_MAX_BLOCKS)), dim3(TX_TPB), 0, fr.st, d.view(), tx, kind, pos, off, star, (u64)n,
                           out, status);
        GT_HIP(hipGetLastError());
    }
    GT_TRY(ic.back(call.out, out, n));
    GT_TRY(ic.back(call.status, status, n));
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
    GT_TRY(digests_aligned("reftx", call.on_device, call.digest));
    ImageCall ic(ap, call.on_device, call.stream);
    GT_TRY(ic.scope.st);
    StreamFrame &fr = ic.fr;
    hipStream_t st = fr.st;
    const size_t n = (size_t)call.n;
    const TxTables t = d.view();
    const u32 *idx;
    GT_TRY(ic.in(call.idx, n, &idx));
    u8 *status;
    u32 *cnt;
    GT_TRY(ic.out(call.status, n, &status));
    GT_TRY(fr.alloc(&cnt, n));
    const unsigned grid = grid_for(n, TX_TPB, TX_MAX_BLOCKS);
    {
        ProfScope ps("k_tx_rows", st);
        hipLaunchKernelGGL(k_tx_rows, dim3(grid), dim3(TX_TPB), 0, st, t, idx, (u64)n, status, cnt);
        GT_HIP(hipGetLastError());
    }
    if (call.digest) {
        u64 *d_digest;
        GT_TRY(ic.digests_out(call.digest, n, &d_digest));
        GT_TRY(tx_digest_rows(fr, ap, t, idx, cnt, status, (u32)n, d_digest, call.h_tables, call.h_seq, call.threads));
        GT_TRY(ic.digests_back(call.digest, d_digest, n));
    }
    if (call.seq_off) {
        u64 *off, total = 0;
        GT_TRY(scan_total(fr, cnt, n, &off, &total));
        GT_TRY(fr.download(*call.seq_off, off, n + 1));
        call.seq_bytes->resize((size_t)total);
        if (total) {
            u8 *d_bytes;
            GT_TRY(fr.alloc(&d_bytes, (size_t)total));
            GT_TRY(tx_fill_rows("k_tx_fill", fr, ap, t, idx, off, (u32)n, total, d_bytes));
            GT_TRY(fr.download(call.seq_bytes->data(), d_bytes, (size_t)total));
        }
    }
    GT_TRY(ic.back(call.status, status, n));
    return fr.drain();
}

}  // namespace gtars
