// reftx_image.h -- two steps of reftx.hip (K19) for the other device code that derives mature mRNAs (hgvs_tx.hip, K23): the
// byte-CSR fill over TxRowSrc and the digests of k_tx_digest with their host tail.  hipcc only: they take a call's frame.
#pragma once

#include "common.h"
#include "reftx.h"

namespace gtars {

// sha512t24u of the mature sequences of n rows (row r: transcript idx[r], cnt[r] its length, status[r] TXSEQ_OK or the
// row gets zero bytes) as four u64 per row at d_digest; all device memory.  Rows longer than GTARS_TX_HOST_LEN are hashed
// on `threads` host threads from the host tables and the chromosomes' host bytes.  The stream is drained on return.
gtars_status tx_digest_rows(StreamFrame &fr, const AssemblyParts &ap, const TxTables &t, const u32 *idx, const u32 *cnt, const u8 *status, u32 n,
                            u64 *d_digest, const TxTables *h_tables, const uint8_t *const *h_seq, unsigned threads);

// the rows' mature sequences back to back, row r at d_bytes[off[r], off[r + 1]) with off the scan of the lengths and
// total = off[n]; queued on the frame's stream.  `name`: the launch's ProfScope entry.
gtars_status tx_fill_rows(const char *name, StreamFrame &fr, const AssemblyParts &ap, const TxTables &t, const u32 *idx, const u64 *off, u32 n,
                          u64 total, u8 *d_bytes);

}  // namespace gtars
