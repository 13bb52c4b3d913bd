// bed_text.hip -- K25: the text streams of a batch of region sets (bed_text_core.h: CHR, START, END joined by commas, LINE
// the BED text) materialised on the device, and their MD5s: the bed digest ("identifier", gtars-core/src/models/
// region_set.rs:282-306), the file digest (:308-330) and the text that to_bed writes.
//
// The batch arrives as concatenated columns (bed_text.h: BedCols) and is worked through in chunks of whole sets, so the
// text buffer stays under GTARS_BED_TEXT_BYTES.  Per chunk:
//   * k_bed_widths, one lane per (stream kind, row): the bytes of the row's piece; then the scan of kernels.hip.  The CSR's
//     row kind * n_rows + i is row i's piece of stream kind `kind`, so a stream (a set and a kind) is one run of CSR rows
//     and of text bytes, and the LINE text of one set IS the file.
//   * the fill of byte_csr.h over BedTextSrc (profiled as k_bed_fill): every requested stream's text, once.
//   * k_bed_md5, one lane per stream, workgroups of one wave: the text is read in aligned 8-byte words and shifted (a
//     stream starts at any byte) -- the blocks wholly inside a stream one block ahead of the compression, the rest and the
//     padding through md5_tail_pairs (md5.h).  Lanes take the streams in ascending order of their
//     lengths (sort_perm), so a wave's 64 streams need about the same number of blocks.  Streams longer than
//     GTARS_BED_DIGEST_HOST_LEN bytes are listed for the host threads instead, which hash the downloaded text with the
//     same header and put the results into the same column.
//   * k_bed_identifier, one lane per set: the MD5 of the 98-byte message over the set's three stream digests.
// Every kernel here takes exact geometry, ceil(n / workgroup size) workgroups and no loop over the grid: the chunk planner
// bounds the rows and streams of a chunk so that the grids fit.
#include <cstring>

#include "bed_text.h"
#include "bed_text_core.h"
#include "byte_csr.h"
#include "common.h"
#include "host_threads.h"
#include "pipeline.h"

namespace gtars {

namespace {

constexpr int BT_TPB = 256;
constexpr int BT_WAVE = 64;
constexpr u64 BT_MAX_CSR_ROWS = 0x7FFFFF00u;  // CSR rows (and streams) of a chunk: u32 row numbers, grids below 2^31
constexpr u64 BT_AUTO_HOST_FLOOR = 65536, BT_AUTO_HOST_CEIL = 16u << 20;

inline unsigned exact_grid(u64 n, int per) { return (unsigned)((n + (u64)per - 1) / (u64)per); }

// the rows of a chunk behind open(r) / byte(k) of byte_csr.h; CSR row r = (r / n_rows) kinds behind kind0, data row r % n_rows
struct BedTextSrc {
    const u32 *chrom, *start, *end;
    const u64 *name_off;
    const u8 *names;
    const u64 *rest_off;
    const u8 *rest, *has_rest;
    const u8 *last;  // 1 on the last row of a set (read for the comma streams only)
    u32 n_rows, n_names, kind0;
    u32 kind;
    BedRow row;
    // false: the row's chromosome id lies outside the names table (the row then has an empty name)
    __device__ __forceinline__ bool open_checked(u32 r) {
        const u32 slot = r / n_rows, i = r - slot * n_rows;
        kind = kind0 + slot;
        row.start = start[i], row.end = end[i];
        const u32 c = chrom[i];
        const bool known = c < n_names;
        const u64 o = known ? name_off[c] : 0;
        row.name = names + o, row.name_len = known ? (u32)(name_off[c + 1] - o) : 0u;
        row.rest = nullptr, row.rest_len = 0, row.has_rest = false, row.last = true;
        if (kind == BED_LINE) {
            if (has_rest[i]) {
                const u64 ro = rest_off[i];
                row.rest = rest + ro, row.rest_len = (u32)(rest_off[i + 1] - ro), row.has_rest = true;
            }
        } else {
            row.last = last[i] != 0;
        }
        return known;
    }
    __device__ __forceinline__ void open(u32 r) { (void)open_checked(r); }
    __device__ __forceinline__ u32 byte(u64 k) { return bed_row_byte(kind, row, (u32)k); }
};

// last[set_off[s + 1] - 1] = 1 for every set with rows (last is zeroed before)
__global__ void __launch_bounds__(BT_TPB) k_bed_mark_last(const u64 *__restrict__ set_off, u32 n_sets, u8 *__restrict__ last) {
    const u64 s = (u64)blockIdx.x * BT_TPB + threadIdx.x;
    if (s >= n_sets) return;
    if (set_off[s + 1] > set_off[s]) last[set_off[s + 1] - 1] = 1;
}

// per set, the bytes of rest its rows hold (the chunk planner's bound)
__global__ void __launch_bounds__(BT_TPB)
k_bed_rest_span(const u64 *__restrict__ set_off, u64 n_sets, const u64 *__restrict__ rest_off, u64 *__restrict__ span) {
    const u64 s = (u64)blockIdx.x * BT_TPB + threadIdx.x;
    if (s >= n_sets) return;
    span[s] = rest_off[set_off[s + 1]] - rest_off[set_off[s]];
}

__global__ void __launch_bounds__(BT_TPB) k_bed_widths(BedTextSrc src, u32 n_csr, u32 *__restrict__ cnt, u32 *__restrict__ bad) {
    const u64 r = (u64)blockIdx.x * BT_TPB + threadIdx.x;
    if (r >= n_csr) return;
    if (!src.open_checked((u32)r)) atomicOr(bad, 1u);
    cnt[r] = bed_row_bytes(src.kind, src.row);
}

// stream t = (set t / nk, kind slot t % nk): its first text byte and its length
__device__ __forceinline__ void stream_span(const u64 *off, const u64 *set_off, u32 n_rows, u32 nk, u32 t, u64 *base, u64 *len) {
    const u32 s = t / nk, slot = t - s * nk;
    const u64 r0 = (u64)slot * n_rows + set_off[s], r1 = (u64)slot * n_rows + set_off[s + 1];
    *base = off[r0], *len = off[r1] - off[r0];
}

// the sort key of a stream: its length, saturated
__global__ void __launch_bounds__(BT_TPB)
k_bed_keys(const u64 *__restrict__ off, const u64 *__restrict__ set_off, u32 n_rows, u32 nk, u32 n_streams, u32 *__restrict__ key) {
    const u64 t = (u64)blockIdx.x * BT_TPB + threadIdx.x;
    if (t >= n_streams) return;
    u64 base, len;
    stream_span(off, set_off, n_rows, nk, (u32)t, &base, &len);
    key[t] = (u32)(len < 0xFFFFFFFFull ? len : 0xFFFFFFFFull);
}

// a stream of the text, eight bytes per call from aligned loads: word c and word c + 1 of the aligned words around the
// stream's first byte, shifted together (the text buffer has 32 readable bytes behind its end: DevBuf)
struct BedTextPairs {
    const u64 *w;
    u32 sh;  // 8 * (first byte's offset in its word)
    u64 held;
    __device__ __forceinline__ u64 pair(u64 c) {
        const u64 lo = held;
        held = w[c + 1];
        return sh ? (lo >> sh) | (held << (64 - sh)) : lo;
    }
};

__global__ void __launch_bounds__(BT_WAVE)
k_bed_md5(const u8 *__restrict__ text, const u64 *__restrict__ off, const u64 *__restrict__ set_off, u32 n_rows, u32 nk, const u32 *__restrict__ perm,
          const u32 *__restrict__ key, u32 n_streams, u64 host_len, u64 *__restrict__ md5, u32 *__restrict__ host_list, u32 *__restrict__ n_host) {
    const u64 lane = (u64)blockIdx.x * BT_WAVE + threadIdx.x;
    if (lane >= n_streams) return;
    const u32 t = perm[lane];
    u64 base, len;
    stream_span(off, set_off, n_rows, nk, t, &base, &len);
    u64 limit = host_len;
    if (!limit) {  // the rule of the batch: 64 times its median stream, between 64 KiB and 16 MiB
        const u64 wide = 64 * (u64)key[perm[n_streams >> 1]];
        limit = wide < BT_AUTO_HOST_FLOOR ? BT_AUTO_HOST_FLOOR : wide > BT_AUTO_HOST_CEIL ? BT_AUTO_HOST_CEIL : wide;
    }
    if (len > limit) {
        host_list[atomicAdd(n_host, 1u)] = t;
        return;
    }
    const u64 *w = (const u64 *)(text + (base & ~7ull));
    const u32 sh = (u32)(base & 7u) * 8u;
    Md5 s;
    md5_init(s);
    // The blocks that lie wholly inside the stream: a block's nine words are loaded while the block before it is compressed
    // (one lane's loads are a chain of misses otherwise: measured at 4.4 us per block against 1 us of compression).
    const u64 full = len >> 6;
    u64 ahead[9];
    if (full) {
#pragma unroll
        for (int i = 0; i < 9; ++i) ahead[i] = w[i];
    }
#pragma unroll 1
    for (u64 blk = 0; blk < full; ++blk) {
        u64 cur[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) cur[i] = ahead[i];
        if (blk + 1 < full) {
            const u64 *p = w + 8 * (blk + 1);
#pragma unroll
            for (int i = 0; i < 9; ++i) ahead[i] = p[i];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) s.m[i] = sh ? (cur[i] >> sh) | (cur[i + 1] << (64 - sh)) : cur[i];
        md5_block(s);
    }
    // the rest of the stream and the padding, by position
    BedTextPairs src{w, sh, (full << 6) < len ? w[8 * full] : 0};
    md5_tail_pairs(s, src, len, full);
    u64 m[2];
    md5_words(s, m);
    md5[(u64)t * 2] = m[0], md5[(u64)t * 2 + 1] = m[1];
}

__global__ void __launch_bounds__(BT_TPB) k_bed_identifier(const u64 *__restrict__ md5, u32 n_sets, u64 *__restrict__ out) {
    const u64 s = (u64)blockIdx.x * BT_TPB + threadIdx.x;
    if (s >= n_sets) return;
    u64 id[2];
    bed_identifier(md5 + 6 * s, id);
    out[2 * s] = id[0], out[2 * s + 1] = id[1];
}

// One chunk: `d` holds device columns of the chunk's rows alone, d.set_off the chunk's HOST offsets (from 0).  The digests go
// to d_out[2 * n_sets] (device), the text to *text (appended).
gtars_status chunk_run(StreamFrame &fr, const BedCols &d, int what, u64 *d_out, std::string *text, unsigned threads) {
    hipStream_t st = fr.st;
    const u64 n_sets = d.n_sets, n_rows = d.set_off[n_sets];
    const u32 nk = what == GTARS_BED_IDENTIFIER ? 3u : 1u, kind0 = what == GTARS_BED_IDENTIFIER ? BED_CHR : BED_LINE;
    const u64 n_csr = nk * n_rows, n_streams = nk * n_sets;
    if (n_csr > BT_MAX_CSR_ROWS || n_streams > BT_MAX_CSR_ROWS) return fail(GTARS_ERR_INTERNAL, "bed text: a chunk beyond its planner's bounds");
    u64 *set_off;
    GT_TRY(fr.upload(&set_off, d.set_off, (size_t)n_sets + 1));
    u64 *off, total = 0;
    u8 *txt = nullptr;
    if (n_csr) {
        u8 *last = nullptr;
        if (what == GTARS_BED_IDENTIFIER) {
            GT_TRY(fr.alloc(&last, (size_t)n_rows));
            GT_HIP(hipMemsetAsync(last, 0, (size_t)n_rows, st));
            hipLaunchKernelGGL(k_bed_mark_last, dim3(exact_grid(n_sets, BT_TPB)), dim3(BT_TPB), 0, st, set_off, (u32)n_sets, last);
            GT_HIP(hipGetLastError());
        }
        const BedTextSrc src{d.chrom, d.start, d.end, d.name_off, d.names, d.rest_off, d.rest, d.has_rest, last, (u32)n_rows, d.n_names, kind0, 0, {}};
        u32 *cnt, *bad, h_bad = 0;
        GT_TRY(fr.alloc(&cnt, (size_t)n_csr));
        GT_TRY(fr.alloc(&bad, 1));
        GT_HIP(hipMemsetAsync(bad, 0, sizeof(u32), st));
        {
            ProfScope ps("k_bed_widths", st);
            hipLaunchKernelGGL(k_bed_widths, dim3(exact_grid(n_csr, BT_TPB)), dim3(BT_TPB), 0, st, src, (u32)n_csr, cnt, bad);
            GT_HIP(hipGetLastError());
        }
        GT_TRY(fr.download(&h_bad, bad, 1));
        GT_TRY(scan_total(fr, cnt, n_csr, &off, &total));  // (drains)
        if (h_bad) return fail(GTARS_ERR_INVALID_ARG, "bed text: a chromosome id outside the names table");
        GT_TRY(fr.alloc(&txt, (size_t)total));
        GT_TRY(csr_fill("k_bed_fill", src, off, (u32)n_csr, total, txt, st));
    } else {  // (no rows: every stream is empty)
        GT_TRY(fr.alloc(&off, 1));
        GT_HIP(hipMemsetAsync(off, 0, sizeof(u64), st));
        GT_TRY(fr.alloc(&txt, 0));
    }
    if (what == BED_WHAT_TEXT) {
        const size_t at = text->size();
        text->resize(at + (size_t)total);
        GT_TRY(fr.download((u8 *)&(*text)[0] + at, txt, (size_t)total));
        return fr.drain();
    }
    if (!n_streams) return fr.drain();
    u32 *key, *perm, *host_list, *n_host, h_n = 0;
    u64 *md5 = d_out;  // (a file digest is its stream's digest)
    if (what == GTARS_BED_IDENTIFIER) GT_TRY(fr.alloc(&md5, 2 * (size_t)n_streams));
    GT_TRY(fr.alloc(&key, (size_t)n_streams));
    hipLaunchKernelGGL(k_bed_keys, dim3(exact_grid(n_streams, BT_TPB)), dim3(BT_TPB), 0, st, off, set_off, (u32)n_rows, nk, (u32)n_streams, key);
    GT_HIP(hipGetLastError());
    GT_TRY(sort_perm(fr, nullptr, key, nullptr, (u32)n_streams, 1, &perm));
    GT_TRY(fr.alloc(&host_list, (size_t)n_streams));
    GT_TRY(fr.alloc(&n_host, 1));
    GT_HIP(hipMemsetAsync(n_host, 0, sizeof(u32), st));
    {
        ProfScope ps("k_bed_md5", st);
        hipLaunchKernelGGL(k_bed_md5, dim3(exact_grid(n_streams, BT_WAVE)), dim3(BT_WAVE), 0, st, txt, off, set_off, (u32)n_rows, nk, perm, key,
                           (u32)n_streams, bed_digest_host_len(), md5, host_list, n_host);
        GT_HIP(hipGetLastError());
    }
    GT_TRY(fr.download(&h_n, n_host, 1));
    GT_TRY(fr.drain());
    if (h_n) {
        // the host tail: the listed streams' text comes down, their digests go up
        std::vector<u32> list;
        GT_TRY(fr.download(list, host_list, h_n));
        GT_TRY(fr.drain());
        std::vector<u64> span(2 * (size_t)h_n);
        for (u32 k = 0; k < h_n; ++k) {
            const u32 s = list[k] / nk, slot = list[k] - s * nk;
            GT_TRY(fr.download(&span[2 * k], off + (u64)slot * n_rows + d.set_off[s], 1));
            GT_TRY(fr.download(&span[2 * k + 1], off + (u64)slot * n_rows + d.set_off[s + 1], 1));
        }
        GT_TRY(fr.drain());
        std::vector<std::vector<u8>> bytes(h_n);
        for (u32 k = 0; k < h_n; ++k) {
            bytes[k].resize((size_t)(span[2 * k + 1] - span[2 * k]));
            GT_TRY(fr.download(bytes[k].data(), txt + span[2 * k], bytes[k].size()));
        }
        GT_TRY(fr.drain());
        std::vector<u64> res(2 * (size_t)h_n);
        parallel_for(h_n, threads, 1, [&](size_t k) {
            Md5 s;
            Md5Bytes src{bytes[k].data()};
            md5_stream(s, src, bytes[k].size());
            md5_words(s, &res[2 * k]);
        });
        for (u32 k = 0; k < h_n; ++k) GT_TRY(fr.upload_to(md5 + 2 * (u64)list[k], &res[2 * k], 2));
        GT_TRY(fr.drain());
    }
    if (what == GTARS_BED_IDENTIFIER) {
        hipLaunchKernelGGL(k_bed_identifier, dim3(exact_grid(n_sets, BT_TPB)), dim3(BT_TPB), 0, st, md5, (u32)n_sets, d_out);
        GT_HIP(hipGetLastError());
    }
    return fr.drain();
}

gtars_status check_call(const BedCols &c, int what, const void *out, const std::string *text) {
    if (what != GTARS_BED_IDENTIFIER && what != GTARS_BED_FILE_DIGEST && what != BED_WHAT_TEXT)
        return fail(GTARS_ERR_INVALID_ARG, "bed text: what must be the identifier or the file digest");
    if (!c.set_off || (what == BED_WHAT_TEXT ? !text : (c.n_sets && !out))) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    if (c.set_off[0] != 0) return fail(GTARS_ERR_INVALID_ARG, "bed text: set offsets must start at 0");
    for (u64 s = 0; s < c.n_sets; ++s)
        if (c.set_off[s + 1] < c.set_off[s]) return fail(GTARS_ERR_INVALID_ARG, "bed text: set offsets must not descend");
    return GTARS_OK;
}

long switch_value(const char *name, long dflt, long most) {
    const long cfg = cfg_int(name, dflt);
    return std::min(cfg < 0 ? dflt : cfg, most);
}

}  // namespace

// (0: the rule of the batch, k_bed_md5; 2^40 bounds it)
uint64_t bed_digest_host_len() { return (u64)switch_value("GTARS_BED_DIGEST_HOST_LEN", 0, 1l << 40); }
uint64_t bed_text_bytes() { return (u64)std::max(switch_value("GTARS_BED_TEXT_BYTES", 1l << 30, 1l << 40), 1l); }
// (measured: formatting on the device, with its upload and download, does not beat the host threads up to 1e7 rows -- DESIGN.md
// section 3 K25 -- so by default no set is large enough)
uint64_t bed_text_device_rows() { return (u64)switch_value("GTARS_BED_TEXT_DEVICE_ROWS", 1l << 40, 1l << 40); }

gtars_status bed_plan_chunks(const std::vector<uint64_t> &bound, const uint64_t *set_off, uint64_t limit, uint64_t max_rows,
                             std::vector<uint64_t> &cut) {
    const u64 n_sets = bound.size();
    cut.assign(1, 0);
    u64 bytes = 0, first = 0;
    for (u64 s = 0; s < n_sets; ++s) {
        const u64 rows = set_off[s + 1] - set_off[s];
        if (rows > max_rows) return fail(GTARS_ERR_INVALID_ARG, "bed text: a set of " + std::to_string(rows) + " rows is too large");
        if (s > first && (bytes + bound[s] > limit || set_off[s + 1] - set_off[first] > max_rows || s - first >= max_rows)) {
            cut.push_back(s);
            first = s, bytes = 0;
        }
        bytes += bound[s];
    }
    if (n_sets) cut.push_back(n_sets);
    return GTARS_OK;
}

gtars_status bed_text_run_device(const BedCols &c, int what, uint64_t *d_out, std::string *text, unsigned threads, void *stream) {
    GT_TRY(check_call(c, what, d_out, text));
    if (d_out && ((uintptr_t)d_out & 7)) return fail(GTARS_ERR_INVALID_ARG, "bed text: the device digests must be 8-byte aligned");
    GT_TRY(require_device());
    const u64 n_sets = c.n_sets, n_rows = c.set_off[n_sets];
    const bool line = what != GTARS_BED_IDENTIFIER;
    if (n_rows && (!c.chrom || !c.start || !c.end || !c.name_off || (line && (!c.rest_off || !c.has_rest))))
        return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    if (!n_sets) return GTARS_OK;
    hipStream_t st = (hipStream_t)stream;
    std::vector<u64> bound(n_sets, 0), cut;
    {
        // the planner's bounds: the longest name, and for the LINE text every set's bytes of rest
        StreamFrame fr(st);
        std::vector<u64> name_off, span(n_sets, 0);
        if (n_rows) GT_TRY(fr.download(name_off, c.name_off, (size_t)c.n_names + 1));
        if (n_rows && line) {
            u64 *set_off, *d_span;
            GT_TRY(fr.upload(&set_off, c.set_off, (size_t)n_sets + 1));
            GT_TRY(fr.alloc(&d_span, (size_t)n_sets));
            hipLaunchKernelGGL(k_bed_rest_span, dim3(exact_grid(n_sets, BT_TPB)), dim3(BT_TPB), 0, st, set_off, n_sets, c.rest_off, d_span);
            GT_HIP(hipGetLastError());
            GT_TRY(fr.download(span, d_span, (size_t)n_sets));
        }
        GT_TRY(fr.drain());
        u64 max_name = 0;
        for (size_t k = 0; k + 1 < name_off.size(); ++k) max_name = std::max(max_name, name_off[k + 1] - name_off[k]);
        for (u64 s = 0; s < n_sets; ++s) bound[s] = bed_text_bound(what, c.set_off[s + 1] - c.set_off[s], span[s], max_name);
    }
    GT_TRY(bed_plan_chunks(bound, c.set_off, bed_text_bytes(), BT_MAX_CSR_ROWS / 3, cut));
    std::vector<u64> local;
    for (size_t k = 0; k + 1 < cut.size(); ++k) {
        const u64 s0 = cut[k], s1 = cut[k + 1], row0 = c.set_off[s0];
        local.assign(c.set_off + s0, c.set_off + s1 + 1);
        for (u64 &v : local) v -= row0;
        BedCols d = c;
        d.set_off = local.data(), d.n_sets = s1 - s0;
        d.chrom = c.chrom + row0, d.start = c.start + row0, d.end = c.end + row0;
        if (line) d.rest_off = c.rest_off + row0, d.has_rest = c.has_rest + row0;
        StreamFrame fr(st);  // (a chunk's buffers go back before the next chunk's are taken)
        GT_TRY(chunk_run(fr, d, what, d_out ? d_out + 2 * s0 : nullptr, text, threads));
    }
    return GTARS_OK;
}

gtars_status bed_text_run_host_cols(const uint64_t *set_off, uint64_t n_sets, const std::vector<uint64_t> &bound, const BedStage &stage, int what,
                                    uint64_t *out, std::string *text, unsigned threads) {
    BedCols all;
    all.set_off = set_off, all.n_sets = n_sets;
    GT_TRY(check_call(all, what, out, text));
    GT_TRY(require_device());
    if (!n_sets) return GTARS_OK;
    const bool line = what != GTARS_BED_IDENTIFIER;
    std::vector<u64> cut;
    GT_TRY(bed_plan_chunks(bound, set_off, bed_text_bytes(), BT_MAX_CSR_ROWS / 3, cut));
    for (size_t k = 0; k + 1 < cut.size(); ++k) {
        const u64 s0 = cut[k], s1 = cut[k + 1];
        BedCols h;
        stage(s0, s1, h);
        const size_t n = (size_t)h.set_off[h.n_sets];
        StreamFrame fr(nullptr);
        BedCols d = h;
        auto up = [&fr](auto *&col, size_t count) {  // the host column behind `col` replaced by its upload
            std::remove_const_t<std::remove_reference_t<decltype(*col)>> *dev;
            const gtars_status e = fr.upload(&dev, col, count);
            col = dev;
            return e;
        };
        GT_TRY(up(d.chrom, n));
        GT_TRY(up(d.start, n));
        GT_TRY(up(d.end, n));
        GT_TRY(up(d.name_off, (size_t)h.n_names + 1));
        GT_TRY(up(d.names, (size_t)h.name_off[h.n_names]));
        if (line) {
            GT_TRY(up(d.rest_off, n + 1));
            GT_TRY(up(d.rest, (size_t)h.rest_off[n]));
            GT_TRY(up(d.has_rest, n));
        }
        u64 *d_out = nullptr;
        if (what != BED_WHAT_TEXT) GT_TRY(fr.alloc(&d_out, 2 * (size_t)h.n_sets));
        GT_TRY(chunk_run(fr, d, what, d_out, text, threads));
        if (d_out) GT_TRY(fr.download(out + 2 * s0, d_out, 2 * (size_t)h.n_sets));
        GT_TRY(fr.drain());
    }
    return GTARS_OK;
}

}  // namespace gtars
