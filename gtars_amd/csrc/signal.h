// signal.h -- internal interface of signal.hip (K13: calc_summary_signal over a signal matrix that is resident on the
// device; gtars-genomicdist/src/signal.rs:356-526) for the host layer.  Plain C++: signal.cpp includes it without the
// HIP headers.
#pragma once

#include <cstdint>

#include "../../include/gtars_amd_host.h"

namespace gtars {

// a query with more hits than this is folded by all waves of a workgroup, every wave a contiguous slice of its hits
constexpr uint32_t SIGNAL_SPLIT_HITS = 1024;
// elements (result rows x conditions) one call of the device sort orders at most: conditions are sorted in groups
constexpr uint32_t SIGNAL_SORT_ELEMS = 1u << 26;

// The device image of a matrix: the row-major f64 values and an AIList-kind overlap index of the rows with val = row.
struct SignalDevice;

// builds the image on the current device: n rows (chromosome ids < n_chrom), values[n * n_cond]
gtars_status signal_build(const uint32_t *chrom, const uint32_t *start, const uint32_t *end, uint64_t n, uint32_t n_chrom,
                          const double *values, uint32_t n_cond, SignalDevice **out);
void signal_free(SignalDevice *s);
int signal_device(const SignalDevice *s);

// What the summary hands back, malloc'ed (nothing is allocated for n_rows == 0): the queries that have a hit, in query
// order -- qidx[n_rows] their indices, values[n_rows * n_cond] the fold of their hits' rows -- and stats[n_cond * 5] =
// lower whisker, lower hinge, median, upper hinge, upper whisker per condition.  want_rows == false: qidx and values
// stay on the device and come back null.
struct SignalSummary {
    uint64_t n_rows = 0;
    uint32_t *qidx = nullptr;
    double *values = nullptr;
    double *stats = nullptr;
    ~SignalSummary();
};

// d_chrom / d_start / d_end: n device rows, chromosome ids of the matrix (any id >= n_chrom: no hits).  Queued on
// `stream` of the current device, which must be the image's; the stream is drained on the way (hit and row counts come
// to the host) and before the call returns.  sort_elems: see SIGNAL_SORT_ELEMS.
gtars_status signal_summary_device(const SignalDevice &s, const uint32_t *d_chrom, const uint32_t *d_start, const uint32_t *d_end,
                                   uint64_t n, bool want_rows, uint32_t sort_elems, SignalSummary &out, void *stream);
// the same for host columns, on the image's device
gtars_status signal_summary(const SignalDevice &s, const uint32_t *chrom, const uint32_t *start, const uint32_t *end, uint64_t n,
                            uint32_t sort_elems, SignalSummary &out);

}  // namespace gtars
