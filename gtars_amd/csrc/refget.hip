// refget.hip -- K21: refget digests and substrings of a sequence collection whose packed image (K12, seqstats.h: every
// record at a 16-byte-aligned offset, the bytes as the file has them, at least 16 zero bytes behind each) is resident on
// the device (gtars-refget/src/digest/fasta.rs:120-306, alphabet.rs:488-527, store/readonly.rs:1292-1352).
//
//   * k_refget_digest, one lane per record: refget_hash of refget_core.h -- the text the host path runs -- over a source
//     that loads the row in aligned 16-byte pieces; the zero bytes behind a row make its last piece readable and are
//     dropped by the loop.  One pass gives sha512t24u (four u64 of characters, K18's column form), MD5 (two u64) and the
//     alphabet class.  Lanes take the rows in ascending order of their lengths (sort_perm), so the 64 records of a wave
//     need about the same number of blocks; results land at the row.  Rows longer than GTARS_REFGET_HOST_LEN bytes are
//     listed for the host instead: refget_digest_run hashes them with the same header on the host threads and writes the
//     results into the device columns.
//   * k_refget_rows + the scan of kernels.hip + the fill of byte_csr.h over RefgetRowSrc (profiled as k_refget_fill):
//     substrings as a byte CSR, upper-cased, eight output bytes per lane.  A row that fails has no bytes and is never read
//     from the image.
#include <cstring>

#include "byte_csr.h"
#include "common.h"
#include "host_threads.h"
#include "image_call.h"
#include "pipeline.h"
#include "refget.h"

namespace gtars {

namespace {

constexpr int RG_TPB = 256;
constexpr u32 RG_MAX_BLOCKS = 256 * 8;
constexpr u64 RG_MAX_N = 0x7FFFFFF0u;

// a row of the image, sixteen bytes per load (refget_hash asks for the pairs in order)
struct RefgetImageSrc {
    const uint4 *p;
    u64 held;
    __device__ __forceinline__ u64 pair(u64 c) {
        if (c & 1) return held;
        const uint4 v = p[c >> 1];
        held = (u64)v.z | ((u64)v.w << 32);
        return (u64)v.x | ((u64)v.y << 32);
    }
};

// the sort key of a row: its length, saturated
__global__ void __launch_bounds__(RG_TPB) k_refget_keys(const u64 *__restrict__ len, u32 n, u32 *__restrict__ key) {
    for (u64 i = (u64)blockIdx.x * RG_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * RG_TPB)
        key[i] = (u32)(len[i] < 0xFFFFFFFFull ? len[i] : 0xFFFFFFFFull);
}

__global__ void __launch_bounds__(RG_TPB) __attribute__((amdgpu_waves_per_eu(3, 3)))
k_refget_digest(const u8 *__restrict__ seq, const u64 *__restrict__ off, const u64 *__restrict__ len, const u32 *__restrict__ perm, u32 n,
                u64 host_len, u64 *__restrict__ out, u64 *__restrict__ md5, u8 *__restrict__ cls, u32 *__restrict__ host_list,
                u32 *__restrict__ n_host) {
    for (u64 w = (u64)blockIdx.x * RG_TPB + threadIdx.x; w < n; w += (u64)gridDim.x * RG_TPB) {
        const u32 i = perm[w];
        const u64 l = len[i];
        if (l > host_len) {
            host_list[atomicAdd(n_host, 1u)] = i;
            continue;
        }
        RefgetImageSrc src{(const uint4 *)(seq + off[i]), 0};  // (off[i] is a multiple of 16)
        Sha512 sh;
        Md5 md;
        u32 mask;
        refget_hash(src, l, sh, md, mask);
        u64 text[4], m[2];
        sha512t24u_words(sh, text);
        md5_words(md, m);
        u64 *dst = out + (u64)i * 4;
        // (the text's first character first in memory)
        dst[0] = __builtin_bswap64(text[0]), dst[1] = __builtin_bswap64(text[1]);
        dst[2] = __builtin_bswap64(text[2]), dst[3] = __builtin_bswap64(text[3]);
        md5[(u64)i * 2] = m[0], md5[(u64)i * 2 + 1] = m[1];
        cls[i] = refget_guess(mask);
    }
}

// per row: its status and the bytes of its substring (0 for a row that failed)
__global__ void __launch_bounds__(RG_TPB)
k_refget_rows(const u64 *__restrict__ len, u32 n_seq, const u32 *__restrict__ seq, const u64 *__restrict__ start, const u64 *__restrict__ end,
              u64 n, u8 *__restrict__ status, u32 *__restrict__ cnt) {
    for (u64 i = (u64)blockIdx.x * RG_TPB + threadIdx.x; i < n; i += (u64)gridDim.x * RG_TPB) {
        const u32 s = seq[i];
        u32 bytes = 0;
        const u8 st = s < n_seq ? refget_sub_status(start[i], end[i], len[s], &bytes) : (u8)RG_SUB_NO_SEQUENCE;
        status[i] = st;
        cnt[i] = bytes;
    }
}

// a row of the CSR: bytes [start, end) of an image row, upper-cased
struct RefgetRowSrc {
    const u8 *seq;
    const u64 *off;
    const u32 *idx;
    const u64 *start;
    const u8 *base;  // of the open row
    __device__ __forceinline__ void open(u32 r) { base = seq + off[idx[r]] + start[r]; }  // (a row with bytes has status 0)
    __device__ __forceinline__ u32 byte(u64 k) { return refget_upper(base[k]); }
};

gtars_status check_device(const AssemblyParts &ap, bool on_device) {
    if (ap.device < 0) return fail(GTARS_ERR_INTERNAL, "refget: the collection has no device image");
    return on_device ? require_handle_device(ap.device) : GTARS_OK;
}

}  // namespace

uint32_t refget_host_len() {
    // (a negative or unreadable value is the default; 2^30 bounds it)
    const long cfg = cfg_int("GTARS_REFGET_HOST_LEN", 65536);
    return (u32)std::min(cfg < 0 ? 65536l : cfg, 0x40000000l);
}

gtars_status refget_digest_run(const Assembly &a, const RefgetDigestCall &call) {
    const AssemblyParts ap = assembly_parts(a);
    GT_TRY(check_device(ap, call.on_device));
    if (call.n != ap.n_chrom) return fail(GTARS_ERR_INVALID_ARG, "refget: the digest columns must have one row per record");
    if (call.n > RG_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "refget: too many records (" + std::to_string(call.n) + ")");
    if (!call.n) {
        if (call.meanwhile) call.meanwhile();
        return GTARS_OK;
    }
    GT_TRY(digests_aligned("refget", call.on_device, call.digest));
    GT_TRY(digests_aligned("refget (md5)", call.on_device, (const char *)call.md5));
    ImageCall ic(ap, call.on_device, call.stream);
    GT_TRY(ic.scope.st);
    StreamFrame &fr = ic.fr;
    hipStream_t st = fr.st;
    const size_t n = (size_t)call.n;
    const u32 host_len = refget_host_len();
    u64 *d_digest, *d_md5;
    u8 *d_cls;
    GT_TRY(ic.digests_out(call.digest, n, &d_digest));
    GT_TRY(ic.out((u64 *)call.md5, 2 * n, &d_md5));
    GT_TRY(ic.out(call.cls, n, &d_cls));
    u32 *key, *perm, *host_list, *n_host;
    GT_TRY(fr.alloc(&key, n));
    const unsigned grid = grid_for(n, RG_TPB, RG_MAX_BLOCKS);
    hipLaunchKernelGGL(k_refget_keys, dim3(grid), dim3(RG_TPB), 0, st, ap.len, (u32)n, key);
    GT_HIP(hipGetLastError());
    GT_TRY(sort_perm(fr, nullptr, key, nullptr, (u32)n, 1, &perm));
    GT_TRY(fr.alloc(&host_list, n));
    GT_TRY(fr.alloc(&n_host, 1));
    GT_HIP(hipMemsetAsync(n_host, 0, sizeof(u32), st));
    {
        ProfScope ps("k_refget_digest", st);
        hipLaunchKernelGGL(k_refget_digest, dim3(grid), dim3(RG_TPB), 0, st, ap.seq, ap.off, ap.len, perm, (u32)n, (u64)host_len, d_digest, d_md5,
                           d_cls, host_list, n_host);
        GT_HIP(hipGetLastError());
    }
    u32 *h_n;
    GT_TRY(ic.host_word(&h_n));
    GT_TRY(fr.download(h_n, n_host, 1));
    if (call.meanwhile) call.meanwhile();
    GT_TRY(fr.drain());
    if (const u32 n_list = *h_n) {
        // the host tail: the rows come back, the results go up
        if (!call.h_seq || !call.h_len) return fail(GTARS_ERR_INTERNAL, "refget: the host tail needs the host bytes");
        std::vector<u32> rows;
        GT_TRY(fr.download(rows, host_list, n_list));
        GT_TRY(fr.drain());
        std::vector<RefgetDigest> res(n_list);
        parallel_for(n_list, call.threads, 1, [&](size_t k) { refget_digest_host(call.h_seq[rows[k]], call.h_len[rows[k]], res[k]); });
        for (u32 k = 0; k < n_list; ++k) {
            GT_TRY(fr.upload_to((char *)(d_digest + 4 * (size_t)rows[k]), res[k].text, 32));
            GT_TRY(fr.upload_to((u8 *)(d_md5 + 2 * (size_t)rows[k]), res[k].md5, 16));
            GT_TRY(fr.upload_to(d_cls + rows[k], &res[k].cls, 1));
        }
        GT_TRY(fr.drain());
    }
    GT_TRY(ic.digests_back(call.digest, d_digest, n));
    GT_TRY(ic.back((u64 *)call.md5, d_md5, 2 * n));
    GT_TRY(ic.back(call.cls, d_cls, n));
    return fr.drain();
}

gtars_status refget_sub_run(const Assembly &a, const RefgetSubCall &call) {
    const AssemblyParts ap = assembly_parts(a);
    return refget_sub_run_over(ap.len, ap.n_chrom, ap.device, call,
                               [&](const u32 *seq, const u64 *start, const u64 *off, u32 n, u64 total, u8 *out, void *st) {
                                   const RefgetRowSrc rows{ap.seq, ap.off, seq, start, nullptr};
                                   return csr_fill("k_refget_fill", rows, off, n, total, out, (hipStream_t)st);
                               });
}

gtars_status refget_sub_run_over(const uint64_t *d_len, uint32_t n_seq, int device, const RefgetSubCall &call, const RefgetFill &fill) {
    const AssemblyParts ap{nullptr, nullptr, d_len, n_seq, device};  // (the frame and the row kernel need no more of an image)
    GT_TRY(check_device(ap, call.on_device));
    if (call.n > RG_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "refget: too many rows (" + std::to_string(call.n) + ")");
    if (call.off) call.off->assign(1, 0), call.bytes->clear();
    if (call.total) *call.total = 0;
    if (call.on_device && call.d_bytes && ((uintptr_t)call.d_bytes & 7))
        return fail(GTARS_ERR_INVALID_ARG, "refget: the device bytes must be 8-byte aligned");
    if (!call.n && !(call.on_device && call.d_off)) return GTARS_OK;
    if (call.n && (!call.seq || !call.start || !call.end)) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    ImageCall ic(ap, call.on_device, call.stream);
    GT_TRY(ic.scope.st);
    StreamFrame &fr = ic.fr;
    hipStream_t st = fr.st;
    const size_t n = (size_t)call.n;
    if (!n) {  // (device callers get their one offset)
        GT_HIP(hipMemsetAsync(call.d_off, 0, sizeof(u64), st));
        return fr.drain();
    }
    const u32 *seq;
    const u64 *start, *end;
    GT_TRY(ic.in(call.seq, n, &seq));
    GT_TRY(ic.in(call.start, n, &start));
    GT_TRY(ic.in(call.end, n, &end));
    u8 *status;
    u32 *cnt;
    GT_TRY(ic.out(call.status, n, &status));
    GT_TRY(fr.alloc(&cnt, n));
    {
        ProfScope ps("k_refget_rows", st);
        hipLaunchKernelGGL(k_refget_rows, dim3(grid_for(n, RG_TPB, RG_MAX_BLOCKS)), dim3(RG_TPB), 0, st, ap.len, ap.n_chrom, seq, start, end, (u64)n,
                           status, cnt);
        GT_HIP(hipGetLastError());
    }
    u64 *off, total = 0;
    GT_TRY(scan_total(fr, cnt, n, &off, &total));
    if (call.total) *call.total = total;
    if (call.on_device) {
        if (call.d_off) GT_HIP(hipMemcpyAsync(call.d_off, off, (n + 1) * sizeof(u64), hipMemcpyDeviceToDevice, st));
        if (total > call.cap || (total && !call.d_bytes)) {
            GT_TRY(fr.drain());
            return fail(GTARS_ERR_CAPACITY, "refget: the byte column is too small: need " + std::to_string(total));
        }
        GT_TRY(fill(seq, start, off, (u32)n, total, call.d_bytes, st));
    } else if (call.off) {
        GT_TRY(fr.download(*call.off, off, n + 1));
        call.bytes->resize((size_t)total);
        if (total) {
            u8 *d_bytes;
            GT_TRY(fr.alloc(&d_bytes, (size_t)total));
            GT_TRY(fill(seq, start, off, (u32)n, total, d_bytes, st));
            GT_TRY(fr.download(call.bytes->data(), d_bytes, (size_t)total));
        }
    }
    GT_TRY(ic.back(call.status, status, n));
    return fr.drain();
}

}  // namespace gtars
