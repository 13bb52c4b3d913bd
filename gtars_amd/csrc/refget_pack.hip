// refget_pack.hip -- K22: the bit-packed image of a sequence collection (the reference's Encoded storage mode:
// gtars-refget/src/digest/encoder.rs:99-130, alphabet.rs:114-123) on the device.  Record r lies at a 16-byte-aligned offset,
// ceil(len b / 8) bytes at the b = 2 / 3 / 4 / 5 / 8 bits of its own alphabet class, at least 16 zero bytes behind it (K12's
// contract, so that aligned wide loads at a record's end are legal); one image may mix the widths.
//
//   * k_refget_pack turns the resident raw image (K12 / K21) into the packed one in ONE launch: one lane per 64 symbols of a
//     record, found by last_le over the scanned table of groups per record.  The lane loads its 64 bytes as up to four
//     aligned 16-byte pieces (a piece that begins behind the record's end is not loaded), runs rg_pack_group of
//     refget_pack_core.h -- the text the host path runs -- and stores the b words that begin inside the record's bytes with
//     plain aligned 8-byte stores.  Symbols at and behind the record's end are zero BITS by rg_pack_group's mask, not by what
//     the table makes of the zero bytes found there.  The five encoding tables are built in LDS by arithmetic at the head of
//     every workgroup: a lookup indexed by data diverges over the wave.  Exactly ceil(groups / 256) workgroups, no loop.
//   * substrings and whole-record decodes are K21's call (k_refget_rows, the scan, the fill of byte_csr.h) over
//     RefgetPackedRowSrc, profiled as k_refget_fill_packed: RgPackedRow reads the record in aligned 64-bit words.  A row
//     that fails has no bytes and is never read from the image.
#include <memory>

#include "byte_csr.h"
#include "common.h"
#include "refget_pack.h"

namespace gtars {

struct PackedImage {
    int device = -1;
    u32 n = 0;
    u64 bytes = 0;
    DevBuf<u8> seq;  // 16-byte aligned (hipMalloc)
    DevBuf<u64> off, len;
    DevBuf<u8> cls;
};

namespace {

constexpr int PK_TPB = 256;

__global__ void __launch_bounds__(PK_TPB)
k_refget_pack(const u8 *__restrict__ raw, const u64 *__restrict__ raw_off, const u64 *__restrict__ len, const u8 *__restrict__ cls,
              const u64 *__restrict__ goff, u32 n, u64 groups, u8 *__restrict__ out, const u64 *__restrict__ out_off) {
    __shared__ u8 tab[5][256];
    for (u32 e = threadIdx.x; e < 5 * 256; e += PK_TPB) tab[e >> 8][e & 255] = rg_encode_byte(e >> 8, (u8)e);
    __syncthreads();
    const u64 t = (u64)blockIdx.x * PK_TPB + threadIdx.x;
    if (t >= groups) return;
    const u32 r = last_le(goff, n, t);
    const u64 g = t - goff[r], l = len[r];  // (a record with groups has l > 64 g)
    const u32 c = cls[r] < 4 ? cls[r] : 4, bits = rg_bits_of(c);
    const u32 valid = (u32)(l - 64 * g < 64 ? l - 64 * g : 64);
    const uint4 *src = (const uint4 *)(raw + raw_off[r] + 64 * g);  // (16-byte aligned: the record's base is)
    u64 in[8];
#pragma unroll
    for (u32 j = 0; j < 4; ++j) {
        // a piece that begins inside the record ends inside its 16 zero bytes at the latest
        const uint4 v = 16 * j < valid ? src[j] : make_uint4(0, 0, 0, 0);
        in[2 * j] = (u64)v.x | ((u64)v.y << 32), in[2 * j + 1] = (u64)v.z | ((u64)v.w << 32);
    }
    const u64 n_bytes = rg_packed_bytes(l, bits);
    u64 *dst = (u64 *)(out + out_off[r]) + (u64)bits * g;
    const u64 first = 8 * (u64)bits * g;  // the group's first byte in the record
    const u8 *enc = tab[c];
    rg_pack_group(bits, in, valid, [&](u8 b) { return enc[b]; },
                  [&](u32 w, u64 word) {
                      // (a word that begins inside the record ends inside its zero bytes at the latest, and carries zero bits there)
                      if (first + 8 * w < n_bytes) dst[w] = word;
                  });
}

// a row of the CSR: symbols [start, end) of a packed record, decoded
struct RefgetPackedRowSrc {
    const u8 *seq;
    const u64 *off;
    const u8 *cls;
    const u32 *idx;
    const u64 *start;
    RgPackedRow row;  // the open row
    __device__ __forceinline__ void open(u32 r) {  // (a row with bytes has status 0)
        const u32 rec = idx[r];
        row.open((const u64 *)(seq + off[rec]), cls[rec], start[r]);
    }
    __device__ __forceinline__ u32 byte(u64 k) { return row.byte(k); }
};

gtars_status columns(PackedImage &p, const u64 *off, const u64 *len, const u8 *cls, u32 n) {
    GT_TRY(p.off.upload(std::vector<u64>(off, off + n)));
    GT_TRY(p.len.upload(std::vector<u64>(len, len + n)));
    GT_TRY(p.cls.upload(std::vector<u8>(cls, cls + n)));
    return GTARS_OK;
}

}  // namespace

gtars_status packed_upload(const uint8_t *image, uint64_t bytes, const uint64_t *off, const uint64_t *len, const uint8_t *cls, uint32_t n,
                           PackedImage **out) {
    *out = nullptr;
    GT_TRY(require_device());
    auto p = std::make_unique<PackedImage>();
    GT_HIP(hipGetDevice(&p->device));
    p->n = n, p->bytes = bytes;
    GT_TRY(p->seq.alloc((size_t)bytes));
    GT_TRY(columns(*p, off, len, cls, n));
    if (bytes) GT_HIP(hipMemcpy(p->seq.p, image, (size_t)bytes, hipMemcpyHostToDevice));
    *out = p.release();
    return GTARS_OK;
}

gtars_status packed_from_raw(const Assembly &raw, const uint64_t *off, const uint64_t *len, const uint8_t *cls, uint32_t n, uint64_t bytes,
                             uint8_t *image, PackedImage **out) {
    *out = nullptr;
    const AssemblyParts ap = assembly_parts(raw);
    if (ap.device < 0 || ap.n_chrom != n) return fail(GTARS_ERR_INTERNAL, "refget: the raw image does not belong to the collection");
    DeviceScope scope(ap.device);
    GT_TRY(scope.st);
    auto p = std::make_unique<PackedImage>();
    p->device = ap.device, p->n = n, p->bytes = bytes;
    GT_TRY(p->seq.alloc((size_t)bytes));
    GT_TRY(columns(*p, off, len, cls, n));
    std::vector<u64> goff((size_t)n + 1, 0);
    for (u32 r = 0; r < n; ++r) goff[r + 1] = goff[r] + ((len[r] + 63) >> 6);
    const u64 groups = goff[n], blocks = (groups + PK_TPB - 1) / PK_TPB;
    if (blocks > 0x7FFFFFFFull) return fail(GTARS_ERR_INVALID_ARG, "refget: the collection is too long for one pack launch");
    {
        StreamFrame fr(nullptr);
        hipStream_t st = fr.st;
        if (bytes) GT_HIP(hipMemsetAsync(p->seq.p, 0, (size_t)bytes, st));
        if (groups) {
            u64 *d_goff;
            GT_TRY(fr.upload(&d_goff, goff.data(), goff.size()));
            ProfScope ps("k_refget_pack", st);
            hipLaunchKernelGGL(k_refget_pack, dim3((unsigned)blocks), dim3(PK_TPB), 0, st, ap.seq, ap.off, ap.len, p->cls.p, d_goff, n, groups,
                               p->seq.p, p->off.p);
            GT_HIP(hipGetLastError());
        }
        GT_TRY(fr.download(image, (const u8 *)p->seq.p, (size_t)bytes));
        GT_TRY(fr.drain());
    }
    *out = p.release();
    return GTARS_OK;
}

void packed_free(PackedImage *p) {
    if (!p) return;
    DeviceScope on(p->device);  // (the buffers go back to the device they came from)
    delete p;
}

int packed_device(const PackedImage *p) { return p ? p->device : -1; }

uint64_t packed_device_bytes(const PackedImage *p) { return p ? p->bytes : 0; }

gtars_status packed_sub_run(const PackedImage &p, const RefgetSubCall &call) {
    return refget_sub_run_over(p.len.p, p.n, p.device, call,
                               [&](const u32 *seq, const u64 *start, const u64 *off, u32 n, u64 total, u8 *out, void *st) {
                                   const RefgetPackedRowSrc rows{p.seq.p, p.off.p, p.cls.p, seq, start, RgPackedRow{}};
                                   return csr_fill("k_refget_fill_packed", rows, off, n, total, out, (hipStream_t)st);
                               });
}

}  // namespace gtars
