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

}  // namespace gtars
