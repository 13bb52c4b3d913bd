// countmat.hip -- K16: the hits of a tokenization (CSR of token ids per query, a matrix row per query) as a sparse count
// matrix in CSR.  Expand the hits to (row, col) pairs, sort them with the library's stable segmented
// radix sort, and cut the sorted pairs into runs: a run is one stored entry, its length the count.
#include "countmat.h"

#include "pipeline.h"

namespace gtars {

// prow[h], pcol[h]: the matrix cell of hit h.  The query of a hit is found by a binary search of the offsets -- one lane per HIT,
// so a query with thousands of hits among queries with none costs what its hits cost, not one lane's walk over all of them.
// The lanes of a wave search for neighbouring hits and read the same words of `offsets` until the last few steps.  A dropped
// hit (id >= n_cols, or row[q] >= n_rows) goes to the sentinel row n_rows, which sorts behind every kept one.
__global__ void __launch_bounds__(256)
k_cm_expand(const u64 *__restrict__ offsets, const u32 *__restrict__ ids, const u32 *__restrict__ row, u64 nq, u32 n_hits, u32 n_rows,
            u32 n_cols, u32 *__restrict__ prow, u32 *__restrict__ pcol) {
    for (u64 h = (u64)blockIdx.x * blockDim.x + threadIdx.x; h < n_hits; h += (u64)gridDim.x * blockDim.x) {
        // first p in [1, nq] with offsets[p] > h (offsets[nq] = n_hits > h): the hit belongs to query p - 1
        u64 lo = 1, hi = nq;
        while (lo < hi) {
            const u64 m = lo + ((hi - lo) >> 1);
            if (offsets[m] > h) hi = m;
            else lo = m + 1;
        }
        const u32 r = row[lo - 1], c = ids[h];
        const bool keep = r < n_rows && c < n_cols;
        prow[h] = keep ? r : n_rows;
        pcol[h] = keep ? c : 0u;
    }
}

// the pairs in sorted order, and head[j]: sorted pair j is kept and differs from its predecessor (it opens a stored entry)
__global__ void __launch_bounds__(256)
k_cm_heads(const u32 *__restrict__ perm, const u32 *__restrict__ prow, const u32 *__restrict__ pcol, u32 n_hits, u32 n_rows,
           u32 *__restrict__ srow, u32 *__restrict__ scol, u32 *__restrict__ head) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n_hits; j += (u64)gridDim.x * blockDim.x) {
        const u32 p = perm[j];
        const u32 r = prow[p], c = pcol[p];
        bool h = r < n_rows;
        if (h && j > 0) {
            const u32 q = perm[j - 1];
            h = prow[q] != r || pcol[q] != c;
        }
        srow[j] = r;
        scol[j] = c;
        head[j] = h;
    }
}

// entry o = off[j] of head j: its column, its row and the position pos[o] where its run starts; pos[nnz] = the number of
// kept pairs (they sort first), where the last run ends
__global__ void __launch_bounds__(256)
k_cm_runs(const u32 *__restrict__ srow, const u32 *__restrict__ scol, const u32 *__restrict__ head, const u64 *__restrict__ off,
          u32 n_hits, u32 n_rows, u32 nnz, u32 *__restrict__ indices, u32 *__restrict__ rrow, u32 *__restrict__ pos) {
    for (u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x; j < n_hits; j += (u64)gridDim.x * blockDim.x) {
        const u32 r = srow[j];
        if (head[j]) {
            const u64 o = off[j];
            indices[o] = scol[j];
            rrow[o] = r;
            pos[o] = (u32)j;
        }
        if (r < n_rows && (j + 1 == n_hits || srow[j + 1] == n_rows)) pos[nnz] = (u32)(j + 1);
    }
}

// data[o] = length of run o; indptr[r] = number of entries in rows before r (a search over the entries' rows: a row without
// an entry repeats its neighbour's value, and no lane writes more than one word however many empty rows lie between two hits)
__global__ void __launch_bounds__(256)
k_cm_finish(const u32 *__restrict__ pos, const u32 *__restrict__ rrow, u32 nnz, u32 n_rows, u32 *__restrict__ data,
            u64 *__restrict__ indptr) {
    const u64 n = std::max<u64>(nnz, (u64)n_rows + 1);
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        if (i < nnz) data[i] = pos[i + 1] - pos[i];
        if (i <= n_rows) indptr[i] = first_ge(rrow, 0u, nnz, (u32)i);
    }
}

gtars_status count_matrix_csr(const uint64_t *d_offsets, const uint32_t *d_ids, const uint32_t *d_row, uint64_t nq, uint32_t n_rows,
                              uint32_t n_cols, uint64_t *d_indptr, uint32_t *d_indices, uint32_t *d_data, uint64_t capacity,
                              uint64_t *nnz, void *stream) {
    StreamFrame fr((hipStream_t)stream);
    hipStream_t st = fr.st;
    *nnz = 0;
    u64 n_hits = 0;
    if (nq) {
        GT_TRY(fr.download(&n_hits, d_offsets + nq, 1));
        GT_TRY(fr.drain());
    }
    if (n_hits > COUNTMAT_MAX_HITS)
        return fail(GTARS_ERR_INVALID_ARG, "too many hits for one count matrix (" + std::to_string(n_hits) + "): split the batch");
    if (n_hits && !d_ids) return fail(GTARS_ERR_INVALID_ARG, "d_ids is NULL");
    const size_t indptr_bytes = ((size_t)n_rows + 1) * sizeof(u64);
    if (!n_hits) {
        GT_HIP(hipMemsetAsync(d_indptr, 0, indptr_bytes, st));
        return fr.drain();
    }
    const u32 n = (u32)n_hits;
    u32 *prow, *pcol, *perm, *srow, *scol, *head;
    GT_TRY(fr.alloc(&prow, n));
    GT_TRY(fr.alloc(&pcol, n));
    {
        ProfScope p("k_cm_expand", st);
        hipLaunchKernelGGL(k_cm_expand, dim3(grid_for(n)), dim3(256), 0, st, d_offsets, d_ids, d_row, nq, n, n_rows, n_cols, prow, pcol);
    }
    {
        ProfScope p("cm_sort", st);
        GT_TRY(sort_perm(fr, prow, pcol, nullptr, n, n_rows + 1, &perm));
    }
    GT_TRY(fr.alloc(&srow, n));
    GT_TRY(fr.alloc(&scol, n));
    GT_TRY(fr.alloc(&head, n));
    {
        ProfScope p("k_cm_heads", st);
        hipLaunchKernelGGL(k_cm_heads, dim3(grid_for(n)), dim3(256), 0, st, perm, prow, pcol, n, n_rows, srow, scol, head);
    }
    GT_HIP(hipGetLastError());
    u64 *off, m = 0;
    GT_TRY(scan_total(fr, head, n, &off, &m));
    *nnz = m;
    if (!m) {
        GT_HIP(hipMemsetAsync(d_indptr, 0, indptr_bytes, st));
        return fr.drain();
    }
    if (m > capacity) return fail(GTARS_ERR_CAPACITY, "count matrix buffers too small: need " + std::to_string(m));
    if (!d_indices || !d_data) return fail(GTARS_ERR_INVALID_ARG, "NULL output");
    u32 *rrow, *pos;
    GT_TRY(fr.alloc(&rrow, m));
    GT_TRY(fr.alloc(&pos, m + 1));
    {
        ProfScope p("k_cm_runs", st);
        hipLaunchKernelGGL(k_cm_runs, dim3(grid_for(n)), dim3(256), 0, st, srow, scol, head, off, n, n_rows, (u32)m, d_indices, rrow, pos);
    }
    {
        ProfScope p("k_cm_finish", st);
        hipLaunchKernelGGL(k_cm_finish, dim3(grid_for(std::max<u64>(m, (u64)n_rows + 1))), dim3(256), 0, st, pos, rrow, (u32)m, n_rows,
                           d_data, d_indptr);
    }
    GT_HIP(hipGetLastError());
    return fr.drain();
}

}  // namespace gtars
