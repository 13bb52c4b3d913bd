"""numpy restatement of the sparse count matrix (K16, gtars_count_matrix_csr_device): the kept hits as keys row * n_cols + col,
np.unique for the occupied cells and their counts, np.searchsorted for indptr.  Nothing of the library is used.
Also what the tests of K16 share: the scoring fixtures and the oracle's barcode -> {peak -> count}."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FRAG1 = os.path.join(GOLD, "fragments", "region_scoring", "fragments1.bed.gz")
FRAG2 = os.path.join(GOLD, "fragments", "region_scoring", "fragments2.bed.gz")
CONS1 = os.path.join(GOLD, "consensus", "consensus1.bed")


def count_matrix_ref(offsets, ids, row, n_rows, n_cols):
    """offsets u64[nq + 1] / ids u32[H]: hits per query; row u32[nq]: the matrix row of each query.
    -> (indptr int64[n_rows + 1], indices int64[nnz], data int64[nnz]); a hit with id >= n_cols and every hit of a query with
    row >= n_rows is dropped."""
    offsets = np.asarray(offsets).astype(np.int64)
    nq = max(len(offsets) - 1, 0)
    n_hits = int(offsets[-1]) if nq else 0
    q_of_hit = np.repeat(np.arange(nq, dtype=np.int64), np.diff(offsets)) if nq else np.zeros(0, np.int64)
    r = np.asarray(row).astype(np.int64)[q_of_hit]
    c = np.asarray(ids).astype(np.int64)[:n_hits]
    keep = (r < n_rows) & (c < n_cols)
    keys, counts = np.unique(r[keep] * max(n_cols, 1) + c[keep], return_counts=True)
    rows_of_keys = keys // max(n_cols, 1)
    indptr = np.searchsorted(rows_of_keys, np.arange(n_rows + 1, dtype=np.int64), side="left").astype(np.int64)
    return indptr, keys % max(n_cols, 1), counts.astype(np.int64)


def csr_to_dict(labels, indptr, indices, data):
    """label -> {col -> count}, rows without an entry left out"""
    out = {}
    for i, lb in enumerate(labels):
        a, b = int(indptr[i]), int(indptr[i + 1])
        if b > a:
            out[lb] = {int(k): int(v) for k, v in zip(indices[a:b], data[a:b])}
    return out


def oracle_dict(frag, cons, n_peaks):
    """barcode -> {peak -> count} from the oracle's tokenize_fragment_file (a peak's id is its line in the sorted consensus file)"""
    import oracle

    exp = {}
    for bcode, ids in oracle.OracleTokenizer(cons).tokenize_fragment_file(frag).items():
        row = {}
        for i in ids:
            if i < n_peaks:  # (a fragment without a hit contributes the unk id: not a peak)
                row[i] = row.get(i, 0) + 1
        if row:
            exp[bcode] = row
    return exp
