// byte_csr.h -- rows of bytes as a CSR (a scanned offset table off[0 .. n] plus one packed byte array), written eight
// output bytes at a time.  The first part is plain C++17, so that the kernel and a stand-alone checking program run one
// text: a host compiler sees no HIP include, under hipcc the functions are __host__ __device__.  The second part, hipcc
// only, is the kernel over it and its launcher: vrs.hip, reftx.hip and hgvs.hip each bring a row source and nothing else.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GT_CSR_HD __host__ __device__ __forceinline__
#else
#define GT_CSR_HD inline
#endif

namespace gtars {

// the last r in [0, n) with off[r] <= key (n >= 1, off[0] <= key; off ascends).  Among rows that share an offset this is
// the last one: in a scanned table the one that is not empty.  P: any indexable, global or LDS
template <class P>
GT_CSR_HD uint32_t last_le(P off, uint32_t n, uint64_t key) {
    uint32_t lo = 0, hi = n;  // the answer is in [lo, hi)
    while (hi - lo > 1) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        if (off[m] <= key) lo = m;
        else hi = m;
    }
    return lo;
}

// Output bytes [8 * group, min(8 * group + 8, total)) of the packed array, total = off[n] > 8 * group.  The row of the first
// byte is found by search, the rows behind it by walking over row ends, so empty rows are stepped over and never opened.
// src.open(r) is called when the bytes of row r begin (or go on) in this group, src.byte(k) returns byte k of the open row;
// k ascends between two open() calls.  A whole group leaves as one aligned 8-byte store: `out` must be 8-byte aligned and
// is written nowhere behind `total`.
template <class Src>
GT_CSR_HD void csr_fill_group(const uint64_t *__restrict__ off, uint32_t n, uint64_t total, uint64_t group, Src &src,
                              uint8_t *__restrict__ out) {
    const uint64_t q0 = group << 3;
    const uint64_t q_end = q0 + 8 < total ? q0 + 8 : total;
    uint32_t r = last_le(off, n, q0);
    uint64_t row0 = off[r], row1 = off[r + 1];  // the bytes of row r
    bool new_row = true;
    uint64_t word = 0;
    for (uint64_t q = q0; q < q_end; ++q) {
        while (row1 <= q) row0 = row1, row1 = off[++r + 1], new_row = true;  // (q < total = off[n]: stops inside the table)
        if (new_row) {
            src.open(r);
            new_row = false;
        }
        word |= (uint64_t)(uint8_t)src.byte(q - row0) << (8 * (q - q0));
    }
    uint8_t *p = out + q0;  // (8-byte aligned: the stores below are aligned to their own sizes)
    const uint32_t k = (uint32_t)(q_end - q0);
    if (k == 8) {
        *(uint64_t *)p = word;
        return;
    }
    // the last group's 1 .. 7 bytes as at most three stores (a byte loop here gets vectorised, and that loop, not the walk,
    // then sets the kernel's register count)
    if (k & 4) *(uint32_t *)p = (uint32_t)word, p += 4, word >>= 32;
    if (k & 2) *(uint16_t *)p = (uint16_t)word, p += 2, word >>= 16;
    if (k & 1) *p = (uint8_t)word;
}

}  // namespace gtars

#if defined(__HIPCC__)
#include "pipeline.h"

namespace gtars {

constexpr int CSR_TPB = 256;
constexpr u32 CSR_MAX_BLOCKS = 256 * 8;

// one lane per group, grid-stride; every group starts from the launch's copy of the source
template <class Src>
__global__ void __launch_bounds__(CSR_TPB) k_csr_fill(Src src0, const u64 *__restrict__ off, u32 n, u64 total, u8 *__restrict__ out) {
    const u64 groups = (total + 7) >> 3;
    for (u64 g = (u64)blockIdx.x * CSR_TPB + threadIdx.x; g < groups; g += (u64)gridDim.x * CSR_TPB) {
        Src src = src0;
        csr_fill_group(off, n, total, g, src, out);
    }
}

// out[0 .. total) on the stream; `name` is the launch's ProfScope entry.  out comes from the allocator (8-byte aligned).
template <class Src>
gtars_status csr_fill(const char *name, const Src &src, const u64 *off, u32 n, u64 total, u8 *out, hipStream_t st) {
    if (!total) return GTARS_OK;
    ProfScope ps(name, st);
    hipLaunchKernelGGL(k_csr_fill<Src>, dim3(grid_for((total + 7) >> 3, CSR_TPB, CSR_MAX_BLOCKS)), dim3(CSR_TPB), 0, st, src, off, n, total, out);
    GT_HIP(hipGetLastError());
    return GTARS_OK;
}

}  // namespace gtars
#endif
