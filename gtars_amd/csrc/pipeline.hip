// pipeline.hip -- see pipeline.h
#include "pipeline.h"

namespace gtars {

gtars_status sort_perm(StreamFrame &fr, const u32 *seg, const u32 *k1, const u32 *k2, u32 n, u32 n_seg, u32 **perm) {
    GT_TRY(fr.alloc(perm, n));
    const size_t sb = device_sort_perm_ws_bytes(n);
    u8 *scratch;
    GT_TRY(fr.alloc(&scratch, sb));
    return device_sort_perm_ws(seg, k1, k2, n, n_seg, *perm, scratch, sb, fr.st);
}

gtars_status scan_total(StreamFrame &fr, const u32 *cnt, u64 n, u64 **off, u64 *total) {
    GT_TRY(fr.alloc(off, (size_t)n + 1));
    u8 *ws;
    const size_t wsb = scan_ws_bytes(n);
    GT_TRY(fr.alloc(&ws, wsb));
    GT_TRY(launch_scan_u32_to_u64(cnt, n, *off, ws, wsb, fr.st));
    GT_TRY(fr.download(total, *off + n, 1));
    return fr.drain();
}

}  // namespace gtars
