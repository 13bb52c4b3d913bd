// hgvs.h -- internal interface of hgvs.hip (K20: the HGVS-to-VRS bridge over a transcript store bound to a genome assembly
// that is resident on the device; gtars-vrs/src/hgvs/bridge.rs:625-913) for the host layer.  Plain C++: hgvs.cpp includes it
// without the HIP headers.
#pragma once

#include <cstdint>

#include "hgvs_core.h"
#include "reftx.h"
#include "seqstats.h"

namespace gtars {

// One batch of parsed rows.  The columns, the text and the outputs are device memory of the image's device (on_device) or
// host memory.  Outputs, any may be null: status (HGVS_*), detail (the TX_* code of a mapping error, the VRS_* code of a
// normalize error, 0 otherwise), warnings (bit 0: uncertain expression), the chromosome id (2^32 - 1 for a row that
// failed), the normalized interval and the 32 digest characters of the Allele (zero bytes for a row that failed).
struct HgvsCall {
    HgvsCols cols;
    bool on_device = false;
    void *stream = nullptr;                 // on_device only
    const char *accessions = nullptr;       // HOST: 32 digest characters per chromosome, a row of zero bytes = none
    const uint8_t *const *h_seq = nullptr;  // HOST: the chromosomes' bytes, for K18's host tail
    unsigned threads = 1;
    uint8_t *status = nullptr, *detail = nullptr, *warnings = nullptr;
    uint32_t *chrom = nullptr;
    uint64_t *start = nullptr, *end = nullptr;
    char *digest = nullptr;  // n * 32, 8-byte aligned when on the device
};
gtars_status hgvs_run(const Assembly &a, const TxDevice &d, const HgvsCall &call);

// hgvs_tx.hip (K23: the transcript-anchored bridge, bridge.rs:226-534).  What both calls need of the host for the two host
// tails (the transcript digests of K19, the long alleles of K18): the tables and the chromosomes' bytes.
struct TxHostSide {
    const TxTables *h_tables = nullptr;
    const uint8_t *const *h_seq = nullptr;
    unsigned threads = 1;
};
// One batch of parsed rows, anchored on the transcripts' own mature mRNAs.  Outputs, any may be null: status, detail
// (TX_NOT_EXONIC with HGVS_MAPPING_ERROR: outside the mature mRNA), warnings, the transcript index (2^32 - 1 for a row the
// bridge refused), the normalized interval on the mRNA, the 32 digest characters of the Allele and the 32 characters of the
// anchor, sha512t24u of the mRNA (both zero bytes for a row that failed).
struct HgvsTxCall {
    HgvsCols cols;
    bool on_device = false;
    void *stream = nullptr;  // on_device only
    TxHostSide host;
    uint8_t *status = nullptr, *detail = nullptr, *warnings = nullptr;
    uint32_t *tx = nullptr;
    uint64_t *start = nullptr, *end = nullptr;
    char *digest = nullptr, *anchor = nullptr;  // n * 32 each, 8-byte aligned when on the device
};
gtars_status hgvs_tx_run(const Assembly &a, const TxDevice &d, const HgvsTxCall &call);

// One batch of alleles on transcripts, the layer under that bridge: allele i lies on the mature mRNA of transcript tx[i]
// at 0-based interbase start[i]; REF and ALT as in a VrsCall.  status is K18's (VRS_NO_CHROM: no such transcript, or the
// assembly cannot give its sequence).
struct VrsTxCall {
    const uint32_t *tx = nullptr;
    const uint64_t *start = nullptr;
    const uint8_t *pool = nullptr;
    uint64_t pool_bytes = 0;
    const uint32_t *ref_off = nullptr, *ref_len = nullptr, *alt_off = nullptr, *alt_len = nullptr;
    uint64_t n = 0;
    bool on_device = false;
    void *stream = nullptr;
    TxHostSide host;
    uint8_t *status = nullptr;
    uint64_t *new_start = nullptr, *new_end = nullptr;
    char *digest = nullptr, *anchor = nullptr;
};
gtars_status vrs_tx_run(const Assembly &a, const TxDevice &d, const VrsTxCall &call);

}  // namespace gtars
