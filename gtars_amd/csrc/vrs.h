// vrs.h -- internal interface of vrs.hip (K18: VRS allele identifiers over a genome assembly that is resident on the device;
// gtars-vrs/src/vcf_core.rs:126-189, normalize.rs:362-441, digest.rs:52-86) for the host layer.  Plain C++: vrs.cpp includes
// it without the HIP headers.
#pragma once

#include <cstdint>
#include <functional>
#include <vector>

#include "seqstats.h"

namespace gtars {

// One batch of alleles.  Allele i: chromosome id chrom[i] of the assembly, 0-based interbase start[i], REF =
// pool[ref_off[i], ref_off[i] + ref_len[i]), ALT likewise; rows may share pool bytes.  The columns, the pool and the outputs
// are device memory of the image's device (on_device) or host memory.
struct VrsCall {
    const uint32_t *chrom = nullptr;
    const uint64_t *start = nullptr;
    const uint8_t *pool = nullptr;
    uint64_t pool_bytes = 0;
    const uint32_t *ref_off = nullptr, *ref_len = nullptr, *alt_off = nullptr, *alt_len = nullptr;
    uint64_t n = 0;
    bool on_device = false;
    void *stream = nullptr;  // on_device only
    // HOST: 32 digest characters per chromosome ("SQ." is the kernel's), a row of zero bytes = no accession for it (its
    // alleles get VRS_NO_CHROM); null: no digests are computed, every chromosome counts as known
    const char *accessions = nullptr;
    const uint8_t *const *h_seq = nullptr;  // HOST: the chromosomes' bytes, for the digest's host tail
    unsigned threads = 1;                   // host threads of that tail
    // outputs, any may be null: status (vrs_core.h), the new interval, 32 digest characters per allele (zero bytes for an
    // allele that failed; needs `accessions`)
    uint8_t *status = nullptr;
    uint64_t *new_start = nullptr, *new_end = nullptr;
    char *digest = nullptr;
    // HOST, whatever on_device says, both or neither: the normalized sequences as a byte CSR (n + 1 offsets)
    std::vector<uint64_t> *seq_off = nullptr;
    std::vector<uint8_t> *seq_bytes = nullptr;
};

// runs the batch on the image's device: the device-affinity rule of the other handle-taking entries for on_device calls
// (the current device must be the image's), the image's device is selected for host columns
gtars_status vrs_run(const Assembly &a, const VrsCall &call);

// The sequences a batch is normalized over, without an Assembly: `n_seq` sequences packed in device memory, sequence c at
// seq[off[c], off[c] + len[c]) (each shorter than 2^32 - 16 bytes).  A roll is bounded by 0 and len[c], never by the
// neighbours in the image.  The accession table, 32 characters per sequence, is device memory (d_acc) or host memory
// (h_acc, uploaded by the call); both null: no digests, every sequence counts.  host_tail serves the digest's host tail:
// for the listed sequence ids it hands back the sequences' first bytes and their 32 accession characters on the host; the
// pointers must stay valid until vrs_run_view returns.
struct VrsSeqView {
    int device = -1;
    const uint8_t *seq = nullptr;
    const uint64_t *off = nullptr, *len = nullptr;
    uint32_t n_seq = 0;
    const uint8_t *d_acc = nullptr;
    const char *h_acc = nullptr;
    std::function<gtars_status(const std::vector<uint32_t> &ids, std::vector<const uint8_t *> &seq, std::vector<const char *> &acc)> host_tail;
};
// vrs_run over such a view (call.accessions and call.h_seq are not read: the view has them); vrs_run(const Assembly &, ...)
// is a caller of it, hgvs_tx.hip (K23) the other
gtars_status vrs_run_view(const VrsSeqView &s, const VrsCall &call);

// vrs.cpp, for the host layers on top of K18 (hgvs.cpp): the library's own host path of a batch -- host columns; the call's
// accessions, threads, status, new_start, new_end and digest are used --, the accession table of a call (the caller's 32
// characters per chromosome, or the assembly's refget digests), and the length rule every entry applies
void vrs_run_on_host(const gtars_assembly *a, const VrsCall &call);
gtars_status vrs_accession_table(gtars_assembly *a, const char *given, unsigned threads, std::vector<char> &tab);
gtars_status vrs_check_lengths(const gtars_assembly *a);

}  // namespace gtars
