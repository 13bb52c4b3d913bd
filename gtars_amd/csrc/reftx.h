// reftx.h -- internal interface of reftx.hip (K19: coordinate mapping and spliced mRNA of a transcript store over a genome
// assembly that is resident on the device; gtars-refget/src/transcripts/mapper.rs, sequence.rs) for the host layer.
// Plain C++: reftx.cpp includes it without the HIP headers.
#pragma once

#include <cstdint>
#include <vector>

#include "reftx_core.h"
#include "seqstats.h"

namespace gtars {

// the tables of a bound store on the assembly's device, uploaded once
struct TxDevice;
gtars_status tx_device_build(const Assembly &a, const TxHostTables &h, TxDevice **out);
void tx_device_free(TxDevice *d);
TxTables tx_device_view(const TxDevice &d);  // the tables as device pointers, for the other kernels that map (hgvs.hip)

// One batch of mapping queries (tx_map_one, reftx_core.h).  The columns and the outputs are device memory of the image's
// device (on_device) or host memory; off and star may be null (all zero).
struct TxMapCall {
    const uint32_t *tx = nullptr;  // transcript index of the store, 2^32 - 1: unknown accession
    const uint8_t *kind = nullptr;
    const int64_t *pos = nullptr, *off = nullptr;
    const uint8_t *star = nullptr;
    uint64_t n = 0;
    bool on_device = false;
    void *stream = nullptr;  // on_device only
    uint64_t *out = nullptr;
    uint8_t *status = nullptr;
};
gtars_status tx_map_run(const Assembly &a, const TxDevice &d, const TxMapCall &call);

// One batch of transcripts by index: status (TXSEQ_*), the 32 characters of sha512t24u of the mature sequence (zero bytes
// for a row that failed), and -- HOST, whatever on_device says, both or neither -- the sequences as a byte CSR.
struct TxSeqCall {
    const uint32_t *idx = nullptr;
    uint64_t n = 0;
    bool on_device = false;
    void *stream = nullptr;
    uint8_t *status = nullptr;
    char *digest = nullptr;  // n * 32, 8-byte aligned when on the device
    std::vector<uint64_t> *seq_off = nullptr;
    std::vector<uint8_t> *seq_bytes = nullptr;
    // HOST, for the digest's host tail: the tables, the chromosomes' bytes, threads
    const TxTables *h_tables = nullptr;
    const uint8_t *const *h_seq = nullptr;
    unsigned threads = 1;
};
gtars_status tx_seq_run(const Assembly &a, const TxDevice &d, const TxSeqCall &call);

// reftx.cpp, for the host layers on top of a binding (hgvs.cpp): what a gtars_txbind holds, and its device tables (built
// at the first call that asks)
struct TxBindParts {
    const TxStoreData *store;
    gtars_assembly *assembly;
    const TxHostTables *tables;      // chrom / seq_status are the binding's
    const uint8_t *const *h_seq;     // [n_chrom] the chromosomes' bytes
};
TxBindParts tx_bind_parts(gtars_txbind *b);
gtars_status tx_bind_device(gtars_txbind *b, Assembly **image, TxDevice **dev);

}  // namespace gtars
