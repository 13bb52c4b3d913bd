// uniwig.h -- internal interface of uniwig.hip (K11: per-base coverage tracks, gtars-uniwig) for the host layer.
// Plain C++: host.cpp includes it without the HIP headers.
//
// One chromosome at a time.  A track is given by two columns of n u32 each:
//   start / end track (start_end_counts, counting.rs:32-158):  opens = the positions p (start + 1 or end of every row),
//       closes = null; every p opens a window at max(1, p - smoothsize) and closes it at p + smoothsize + 1
//   core track (core_counts, counting.rs:167-290):  opens = start + 1, closes = end of the rows; smoothsize is ignored
// The columns need not be sorted (each is sorted on its own, on the device).  With a the sorted opens and e the sorted
// closes the track is  count(pos) = #{a <= pos} - #{e <= pos}  for pos = a_0 .. max(chrom_size, a_{n-1} - 1).
#pragma once

#include <cstdint>

#include "../../include/gtars_amd_host.h"

namespace gtars {

// first reported position and number of reported positions of a track (0, 0 for n == 0); checks the arguments
gtars_status uniwig_extent(const uint32_t *opens, const uint32_t *closes, uint64_t n, uint32_t chrom_size, uint32_t smoothsize,
                           int kind, uint64_t *first, uint64_t *len);

// the whole track into host memory (*counts: malloc'ed, *n_counts entries).  The device holds at most max_device_bytes
// of counts at a time (0: the library's default window), the track is produced window after window.
gtars_status uniwig_counts(const uint32_t *opens, const uint32_t *closes, uint64_t n, uint32_t chrom_size, uint32_t smoothsize,
                           int kind, uint64_t max_device_bytes, uint64_t *first, uint32_t **counts, uint64_t *n_counts);

// positions window_first .. window_first + window_len - 1 of the track into d_counts (device, 16-byte aligned), queued
// on `stream`.  d_opens / d_closes: device columns, each ASCENDING.
gtars_status uniwig_counts_device(const uint32_t *d_opens, const uint32_t *d_closes, uint64_t n, uint32_t smoothsize, int kind,
                                  uint64_t window_first, uint64_t window_len, uint32_t *d_counts, void *stream);

// compress_counts (utils.rs:40-81) of the track, runs starting at start_position: three malloc'ed columns of *n_runs
gtars_status uniwig_runs(const uint32_t *opens, const uint32_t *closes, uint64_t n, uint32_t chrom_size, uint32_t smoothsize,
                         int kind, uint32_t start_position, uint32_t **run_start, uint32_t **run_end, uint32_t **run_count,
                         uint64_t *n_runs);

// the non-zero entries among the first chrom_size entries of the track as (start_position + entry index, count)
// (write_to_wig_file_variable, writing.rs:149-179): two malloc'ed columns of *n_out
gtars_status uniwig_nonzero(const uint32_t *opens, const uint32_t *closes, uint64_t n, uint32_t chrom_size, uint32_t smoothsize,
                            int kind, uint32_t start_position, uint32_t **position, uint32_t **count, uint64_t *n_out);

}  // namespace gtars
