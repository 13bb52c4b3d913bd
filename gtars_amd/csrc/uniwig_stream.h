// uniwig_stream.h -- internal interface of uniwig_stream.hip (K24: the streaming uniwig of gtars-uniwig/src/stream.rs --
// scored, sparse, gap-filled) for the host layer.  Plain C++: host.cpp includes it without the HIP headers.
//
// Rows are (chromosome id, start, end, score) in FILE ORDER, any order.  Per row a window [ws, we] (1-based, inclusive):
//   start: c = start + 1, ws = max(1, c - m), we = c + m;   end: c = end, the same;   core: ws = start + 1, we = end - 1,
//   a core row with we < ws is dropped before anything else.
// A run is a maximal run of consecutive equal chromosome ids.  Inside a run, M_i = the inclusive prefix maximum of ws,
// B_i = the exclusive prefix maximum of we; row i adds score_i to [M_i, we_i]; it opens a segment when it is the run's
// first row or when M_i > B_i + 1 and the gap M_i - B_i - 1 is not filled (filled: max_gap < 0 or gap <= max_gap).  A
// segment spans its head's M to the largest we of its rows; with max_gap < 0 a run has one segment, which starts at 1 and
// reaches at least the chromosome's size when it has one.  The counts are the positions of all segments, one after the
// other ("compacted coordinates"), sums of scores modulo 2^32.
#pragma once

#include <cstdint>

#include "../../include/gtars_amd_host.h"

namespace gtars {

struct SwPlan;  // the segment table on the host and the event columns on the device

// rows on the host (on_device == 0) or on the current device.  sizes_by_cid[c]: the chromosome's size, 0 for none.
gtars_status uniwig_stream_plan(const uint32_t *cid, const uint32_t *start, const uint32_t *end, const uint32_t *score, uint64_t n,
                                int on_device, const uint32_t *sizes_by_cid, uint32_t n_chrom, uint32_t smoothsize, int kind,
                                int64_t max_gap, SwPlan **plan);
void uniwig_stream_plan_free(SwPlan *plan);
uint64_t uniwig_stream_plan_segments(const SwPlan *plan);
uint64_t uniwig_stream_plan_total(const SwPlan *plan);
// n_seg entries each (offset: n_seg + 1); a null pointer skips the column.  Segments of length 0 are in the table.
gtars_status uniwig_stream_plan_table(const SwPlan *plan, uint32_t *seg_cid, uint32_t *seg_first, uint32_t *seg_len, uint64_t *seg_off);

// compacted positions window_first .. window_first + window_len - 1 into d_counts (device, 16-byte aligned), queued on
// `stream`; step 1
gtars_status uniwig_stream_device(const SwPlan *plan, uint64_t window_first, uint64_t window_len, uint32_t *d_counts, void *stream);

// the whole call on host columns: the table without its empty segments (three malloc'ed columns of *n_seg) and the
// counts of the kept positions ((pos - 1) % step == 0), malloc'ed, *n_counts.  The device holds at most max_device_bytes
// of counts at a time (0: the default of K11).
gtars_status uniwig_stream(const uint32_t *cid, const uint32_t *start, const uint32_t *end, const uint32_t *score, uint64_t n,
                           const uint32_t *sizes_by_cid, uint32_t n_chrom, uint32_t smoothsize, uint32_t step, int kind,
                           int64_t max_gap, uint64_t max_device_bytes, uint32_t **seg_cid, uint32_t **seg_first,
                           uint32_t **seg_len, uint64_t *n_seg, uint32_t **counts, uint64_t *n_counts);

}  // namespace gtars
