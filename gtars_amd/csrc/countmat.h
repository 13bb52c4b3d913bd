// countmat.h -- internal interface of countmat.hip (K16: the sparse barcode x peak count matrix of a tokenization, in CSR,
// built on the device) for the C entry point in api.hip.
#pragma once

#include <cstdint>

#include "../../include/gtars_amd.h"

namespace gtars {

// one lane per hit in the kernels, a u32 n in the sort (whose launchers round n up to whole workgroups of 256)
constexpr uint64_t COUNTMAT_MAX_HITS = 0xFFFFF000ull;
// the sort's segment key is the row, n_rows itself the row of the dropped hits: the key's width is found with 1u << bits
constexpr uint32_t COUNTMAT_MAX_ROWS = 0x7FFFFFFEu;

// Device pointers.  d_offsets[nq + 1] / d_ids: the CSR of hits per query (gtars_tokenize_device), d_row[q] < n_rows: the matrix
// row of query q.  Out: d_indptr[n_rows + 1], and d_indices / d_data[*nnz] (room for `capacity` entries): per row the occupied
// columns in ascending order and the number of hits (q, id) with row[q] == r and id == column.  A hit with id >= n_cols and every
// hit of a query with row[q] >= n_rows is dropped.  capacity < *nnz: GTARS_ERR_CAPACITY, *nnz is what it takes, d_indices and
// d_data are untouched.  The inputs are only read; the stream is drained when the call returns.
gtars_status count_matrix_csr(const uint64_t *d_offsets, const uint32_t *d_ids, const uint32_t *d_row, uint64_t nq, uint32_t n_rows,
                              uint32_t n_cols, uint64_t *d_indptr, uint32_t *d_indices, uint32_t *d_data, uint64_t capacity,
                              uint64_t *nnz, void *stream);

}  // namespace gtars
