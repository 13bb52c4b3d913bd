// pipeline.h -- the steps the device pipelines share: the region-set ones (setops.hip, annot.hip, uniwig.hip) and the ones
// over the packed genome image (seqstats.hip, vrs.hip, reftx.hip, hgvs.hip; their call frame is image_call.h, their
// byte-CSR fill byte_csr.h).  The host-side steps queue their work on a StreamFrame's stream and leave what they allocate
// with the frame.
#pragma once

#include "common.h"

namespace gtars {

// workgroups of `per` elements that cover n, at least one and at most `cap` (grid-stride kernels)
// (GTARS_GRID_CAP, a test switch, lowers `cap`: common.h)
inline unsigned grid_for(u64 n, u32 per = 256, u32 cap = 1u << 16) {
    const u64 want = std::max<u64>(1, (n + per - 1) / per);
    if (const u32 low = grid_cap_switch(); low && low < cap && want > low) {
        note_grid_clip();
        return low;
    }
    return (unsigned)std::min<u64>(want, cap);
}

// One launch of a grid-stride kernel of 256-lane workgroups over n elements, on the geometry above, with the launch's error
// checked: what `hipLaunchKernelGGL(k, dim3(grid_for(n)), dim3(256), 0, st, ...); GT_HIP(hipGetLastError());` spells out.
template <class K, class... A>
inline gtars_status launch_over(hipStream_t st, u64 n, K kernel, A... args) {
    hipLaunchKernelGGL(kernel, dim3(grid_for(n)), dim3(256), 0, st, args...);
    GT_HIP(hipGetLastError());
    return GTARS_OK;
}

// first position p in [lo, hi) with x[p] >= key (first_gt: > key), hi if none; x ascends.  P: any indexable, global or LDS
// (their sibling last_le -- the row of an element in a scanned offset table -- is in byte_csr.h: host programs compile it too)
template <class P>
__device__ __forceinline__ u32 first_ge(P x, u32 lo, u32 hi, u32 key) {
    while (lo < hi) {
        const u32 m = lo + ((hi - lo) >> 1);
        if (x[m] >= key) hi = m;
        else lo = m + 1;
    }
    return lo;
}
template <class P>
__device__ __forceinline__ u32 first_gt(P x, u32 lo, u32 hi, u32 key) {
    while (lo < hi) {
        const u32 m = lo + ((hi - lo) >> 1);
        if (x[m] > key) hi = m;
        else lo = m + 1;
    }
    return lo;
}

// *perm: the permutation that stably sorts n device rows by (seg, k1[, k2]), seg < n_seg (k2 may be null; a single
// 32-bit key x sorts as (x, x) with n_seg == 1).  The permutation and the sort's scratch belong to the frame.
gtars_status sort_perm(StreamFrame &fr, const u32 *seg, const u32 *k1, const u32 *k2, u32 n, u32 n_seg, u32 **perm);

// (*off)[0 .. n]: the exclusive scan of n u32 counts; *total = (*off)[n], on the host when the call returns (the
// stream is drained)
gtars_status scan_total(StreamFrame &fr, const u32 *cnt, u64 n, u64 **off, u64 *total);

}  // namespace gtars
