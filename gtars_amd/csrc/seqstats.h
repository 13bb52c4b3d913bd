// seqstats.h -- internal interface of seqstats.hip (K12: per-region GC content and dinucleotide counts over a genome
// assembly that is resident on the device; gtars-genomicdist/src/statistics.rs:331-483) for the host layer.
// Plain C++: assembly.cpp includes it without the HIP headers.
#pragma once

#include <cstdint>

#include "../../include/gtars_amd_host.h"

namespace gtars {

// bytes of a region one work item of the counting kernels covers: a region of width w is ceil(w / SEQ_PIECE) pieces
constexpr uint32_t SEQ_PIECE = 4096;

// The device image of an assembly: ONE packed byte buffer -- chromosome c at the 16-byte-aligned offset off[c], len[c]
// bytes as the file has them, at least 16 zero bytes behind every chromosome (the last included) -- and the two u64
// columns off / len.
struct Assembly;

// builds the image on the current device from n_chrom host sequences (seq[c]: len[c] bytes); uploaded piece by piece
// through pinned staging
gtars_status assembly_build(const uint8_t *const *seq, const uint64_t *len, uint32_t n_chrom, Assembly **out);
void assembly_free(Assembly *a);
int assembly_device(const Assembly *a);
// the image's parts for the other kernels that read it (vrs.hip): device pointers, valid while the image lives
struct AssemblyParts {
    const uint8_t *seq;   // the packed bytes
    const uint64_t *off;  // [n_chrom] offset of every chromosome in seq
    const uint64_t *len;  // [n_chrom]
    uint32_t n_chrom;
    int device;
};
AssemblyParts assembly_parts(const Assembly &a);
int assembly_set_device(Assembly *a, int device);  // test hook (gtars_debug_set_assembly_device): -> the id recorded before
uint64_t assembly_stage_blocks();  // test hook (gtars_debug_seq_stage_blocks): staging blocks sent by every build so far

// d_chrom / d_start / d_end: n device rows, chromosome ids of the assembly, every row with start <= end <= len (a row
// that is not fails the call with GTARS_ERR_INVALID_ARG and is never read from the image).
// mode GTARS_SEQ_GC:     d_out[n]      = bytes of [start, end) that are G, C, g or c
// mode GTARS_SEQ_DINUCL: d_out[n * 16] = windows (b[i], b[i + 1]), start <= i, i + 1 < end, both bytes in ACGTacgt, by
//                                        4 * code(b[i]) + code(b[i + 1]) with A, C, G, T = 0 .. 3 (DINUCL_ORDER)
// Queued on `stream` of the current device, which must be the image's; the stream is drained once on the way (the
// number of pieces comes to the host) and again before the call returns.
gtars_status seqstats_counts_device(const Assembly &a, const uint32_t *d_chrom, const uint32_t *d_start, const uint32_t *d_end,
                                    uint64_t n, int mode, uint32_t *d_out, void *stream);

// the same for host columns, on the image's device: out[n] or out[n * 16]
gtars_status seqstats_counts(const Assembly &a, const uint32_t *chrom, const uint32_t *start, const uint32_t *end, uint64_t n,
                             int mode, uint32_t *out);

}  // namespace gtars
