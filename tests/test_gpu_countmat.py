"""The sparse count matrix on the device (K16): gtars_count_matrix_csr_device on hand-built CSR inputs, compared exactly with the
numpy restatement tests/countmat_ref.py at the sort's and the scan's tile edges, at the radix digit edges of the row key, with
one run longer than any tile, with skewed queries, at its capacity edge and on a side stream; and barcode_count_matrix against
the dict form, the oracle and the dense file x peak matrix."""
import gzip
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import countmat_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

FRAG1, FRAG2, CONS1, oracle_dict = R.FRAG1, R.FRAG2, R.CONS1, R.oracle_dict
GUARD = 64
FILL = -0x5A5A5A5B  # what untouched output words hold


def device_csr(offsets, ids, row, n_rows, n_cols, capacity=None, stream=None):
    """-> (indptr, indices, data, nnz) of the entry point as int64 numpy arrays; the words behind nnz (and the guard words behind
    the capacity) are checked to be untouched"""
    import torch

    from gtars_amd import scoring

    offsets, ids, row = (np.ascontiguousarray(a, dtype=t) for a, t in ((offsets, np.uint64), (ids, np.uint32), (row, np.uint32)))
    nq = len(row)
    dev = torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        d_off = torch.from_numpy(offsets.view(np.int64)).to(dev) if nq else None
        d_ids = torch.from_numpy(ids.view(np.int32)).to(dev) if len(ids) else None
        d_row = torch.from_numpy(row.view(np.int32)).to(dev) if nq else None
        cap = len(ids) if capacity is None else capacity
        indptr = torch.full((n_rows + 1,), -1, dtype=torch.int64, device=dev)
        indices = torch.full((cap + GUARD,), FILL, dtype=torch.int32, device=dev)
        data = torch.full((cap + GUARD,), FILL, dtype=torch.int32, device=dev)
        before = [None if t is None else t.clone() for t in (d_off, d_ids, d_row)]
        try:
            nnz = scoring.count_matrix_csr_device(*(0 if t is None else t.data_ptr() for t in (d_off, d_ids, d_row)), nq, n_rows, n_cols,
                                                  indptr.data_ptr(), indices.data_ptr(), data.data_ptr(), cap,
                                                  torch.cuda.current_stream().cuda_stream)
        except Exception:
            assert bool((indices == FILL).all()) and bool((data == FILL).all())  # an error writes no entry
            raise
        finally:
            for t, b in zip((d_off, d_ids, d_row), before):
                assert t is None or torch.equal(t, b)  # the inputs are only read
        assert bool((indices[nnz:] == FILL).all()) and bool((data[nnz:] == FILL).all())
        return (indptr.cpu().numpy(), indices[:nnz].cpu().numpy().astype(np.int64),
                data[:nnz].cpu().numpy().view(np.uint32).astype(np.int64), nnz)


def check(offsets, ids, row, n_rows, n_cols, **kw):
    got = device_csr(offsets, ids, row, n_rows, n_cols, **kw)
    exp = R.count_matrix_ref(offsets, ids, row, n_rows, n_cols)
    assert got[3] == len(exp[1])
    for g, e, what in zip(got, exp, ("indptr", "indices", "data")):
        assert np.array_equal(g, e), what
    return got


def ragged(n_hits, rng, nq=None):
    """offsets of nq queries (about n_hits / 2, some without a hit) that hold n_hits hits"""
    nq = max(1, n_hits // 2) if nq is None else nq
    cuts = np.sort(rng.integers(0, n_hits + 1, nq - 1)) if nq > 1 else np.zeros(0, np.int64)
    return np.concatenate([[0], cuts, [n_hits]]).astype(np.uint64)


# ---- the entry point ------------------------------------------------------------------------------------------------
def test_empty_inputs():
    z64, z32 = np.zeros(1, np.uint64), np.zeros(0, np.uint32)
    got = check(z64, z32, z32, 5, 7)  # nq == 0
    assert got[3] == 0 and got[0].tolist() == [0] * 6
    got = check(np.zeros(101, np.uint64), z32, np.arange(100) % 5, 5, 7)  # 100 queries without a hit
    assert got[3] == 0 and got[0].tolist() == [0] * 6
    assert check(z64, z32, z32, 0, 0)[0].tolist() == [0]


@pytest.mark.parametrize("what", ["ids", "rows"])
def test_every_hit_dropped(what):
    rng = np.random.default_rng(3)
    off = ragged(1000, rng)
    ids = rng.integers(0, 50, 1000) + (50 if what == "ids" else 0)
    row = rng.integers(0, 20, len(off) - 1) + (20 if what == "rows" else 0)
    got = check(off, ids, row, 20, 50)
    assert got[3] == 0 and not got[0].any()


EDGES = [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8191, 8192, 8193, 65535, 65536, 65537]


@pytest.mark.parametrize("n_hits", EDGES)
def test_tile_edges_with_repeated_pairs(n_hits):
    """rows and columns from ranges that hold about n_hits / 2 cells: many pairs repeat; one hit in 20 is dropped"""
    rng = np.random.default_rng(n_hits)
    n_rows = max(1, int(np.sqrt(n_hits)) // 2)
    n_cols = max(1, n_hits // (2 * n_rows))
    off = ragged(n_hits, rng)
    ids = rng.integers(0, n_cols, n_hits)
    ids[rng.random(n_hits) < 0.03] = n_cols + 1
    row = rng.integers(0, n_rows, len(off) - 1)
    row[rng.random(len(row)) < 0.03] = n_rows
    got = check(off, ids, row, n_rows, n_cols)
    assert n_hits < 64 or got[3] < n_hits


@pytest.mark.parametrize("n_hits", EDGES)
def test_tile_edges_with_distinct_pairs(n_hits):
    rng = np.random.default_rng(n_hits + 1)
    n_rows, n_cols = 300, 911
    cells = rng.choice(n_rows * n_cols, n_hits, replace=False)
    off = np.arange(n_hits + 1, dtype=np.uint64)  # one hit per query
    got = check(off, cells % n_cols, cells // n_cols, n_rows, n_cols)
    assert got[3] == n_hits and (got[2] == 1).all()


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_one_run_longer_than_every_tile(order):
    """pair (3, 5) 70,001 times -- across every tile boundary, a count beyond 65,535 -- with one pair in front and one behind"""
    n = 70_001
    row = np.concatenate([[3], np.full(n, 3), [3]])
    ids = np.concatenate([[4], np.full(n, 5), [6]])
    if order == "shuffled":
        p = np.random.default_rng(5).permutation(n + 2)
        row, ids = row[p], ids[p]
    got = check(np.arange(n + 3, dtype=np.uint64), ids, row, 9, 11)
    assert got[1].tolist() == [4, 5, 6] and got[2].tolist() == [1, n, 1] and got[0].tolist() == [0, 0, 0, 0, 3, 3, 3, 3, 3, 3]
    # the same run as the hits of ONE query (they share its row), a neighbour on either side
    got = check(np.array([0, 1, n + 1, n + 2], dtype=np.uint64), np.concatenate([[5], np.full(n, 5), [5]]), [2, 3, 4], 9, 11)
    assert got[2].tolist() == [1, n, 1]


@pytest.mark.parametrize("n_rows", [1, 255, 256, 257, 65537])
def test_row_counts_at_the_digit_edges_of_the_segment_key(n_rows):
    rng = np.random.default_rng(n_rows)
    counts = rng.integers(0, 5, 1500)
    counts[0] = counts[-1] = 2  # first and last query hold hits: both rows are occupied
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    n_hits = int(off[-1])
    row = rng.integers(0, n_rows, 1500)
    row[0], row[-1] = 0, n_rows - 1
    ids = rng.integers(0, 40, n_hits)
    got = check(off, ids, row, n_rows, 40)
    assert got[0][1] > 0 and got[0][-1] > got[0][-2]


def test_more_rows_than_hits_gives_plateaus():
    rng = np.random.default_rng(8)
    row = rng.choice([0, 57, 99_999], 600)
    row[:3] = [0, 57, 99_999]
    counts = rng.integers(0, 4, 600)
    counts[:3] = 1
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    got = check(off, rng.integers(0, 12, int(off[-1])), row, 100_000, 12)
    ip = got[0]
    assert len(np.unique(ip)) == 4 and ip[1] == ip[57] and ip[58] == ip[99_999] and ip[100_000] == got[3]


def test_column_edges():
    rng = np.random.default_rng(9)
    off = ragged(5000, rng)
    row = rng.integers(0, 30, len(off) - 1)
    check(off, np.zeros(5000), row, 30, 1)  # one column
    check(off, rng.integers(0, 2, 5000), row, 30, 1)  # ... and half of the hits beyond it
    n_cols = (1 << 20) + 3
    ids = rng.integers(0, n_cols + 2, 5000)
    ids[:4] = [n_cols - 1, n_cols, n_cols - 1, 0]
    got = check(off, ids, row, 30, n_cols)
    assert got[1].max() == n_cols - 1


@pytest.mark.parametrize("where", ["middle", "last"])
def test_one_heavy_query_among_light_ones(where):
    rng = np.random.default_rng(10)
    counts = rng.integers(0, 3, 1001)
    counts[500 if where == "middle" else 1000] = 5000
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    n_hits = int(off[-1])
    check(off, rng.integers(0, 200, n_hits), rng.integers(0, 50, 1001), 50, 200)


def test_capacity_edge():
    import torch

    from gtars_amd import CapacityError

    rng = np.random.default_rng(11)
    off = ragged(4000, rng)
    ids, row = rng.integers(0, 60, 4000), rng.integers(0, 25, len(off) - 1)
    nnz = len(R.count_matrix_ref(off, ids, row, 25, 60)[1])
    assert 1 < nnz < 4000
    check(off, ids, row, 25, 60, capacity=nnz)  # (device_csr checks the guard words)
    with pytest.raises(CapacityError) as err:
        device_csr(off, ids, row, 25, 60, capacity=nnz - 1)  # ... and that the error wrote no entry
    assert err.value.needed == nnz
    torch.cuda.synchronize()


def test_side_stream_leaves_inputs_alone():
    import torch

    rng = np.random.default_rng(12)
    off = ragged(20_000, rng)
    ids, row = rng.integers(0, 500, 20_000), rng.integers(0, 100, len(off) - 1)
    s = torch.cuda.Stream()
    check(off, ids, row, 100, 500, stream=s)  # (device_csr compares the inputs bit by bit after the call)
    s.synchronize()


def test_size_limits_are_argument_errors():
    import torch

    from gtars_amd import scoring

    dev = torch.device("cuda", torch.cuda.current_device())
    off = torch.tensor([0, 1 << 32], dtype=torch.int64, device=dev)
    one = torch.zeros(4, dtype=torch.int32, device=dev)
    ip = torch.zeros(4, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="too many hits"):
        scoring.count_matrix_csr_device(off.data_ptr(), one.data_ptr(), one.data_ptr(), 1, 2, 2, ip.data_ptr(), one.data_ptr(),
                                        one.data_ptr(), 4)
    with pytest.raises(ValueError, match="too many rows"):
        scoring.count_matrix_csr_device(off.data_ptr(), one.data_ptr(), one.data_ptr(), 1, 0xFFFFFFFF, 2, ip.data_ptr(), one.data_ptr(),
                                        one.data_ptr(), 4)


# ---- barcode_count_matrix -------------------------------------------------------------------------------------------
def test_golden_pair_equals_the_dict_form_and_the_oracle():
    from gtars_amd.scoring import barcode_count_matrix, barcode_scoring_from_fragments

    m = barcode_count_matrix(FRAG1, CONS1)
    assert m.shape == (len(m.barcodes), 4) and m.barcodes == sorted(m.barcodes, key=str.encode)
    assert m.indptr.dtype == np.int64 and m.indices.dtype == np.int32 and m.data.dtype == np.int32
    assert m.to_dict() == barcode_scoring_from_fragments(FRAG1, CONS1) == oracle_dict(FRAG1, CONS1, 4)


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    """the shape of the dict form's own test: 3,000 peaks, 20,000 fragments, 300 barcodes, the consensus written in sorted order
    (a peak's index is its line); -> (fragment file, consensus file, n_peaks, the oracle's dict, every barcode of the file)"""
    from gtars_amd import synth

    tmp = tmp_path_factory.mktemp("countmat")
    u = synth.make_universe(3_000)
    fd = synth.write_config5_inputs(str(tmp), u, 1, 20_000, 5, barcodes=300)[1]
    frag = os.path.join(fd, sorted(os.listdir(fd))[0])
    rows = sorted(zip((synth.CHROM_NAMES[c] for c in u["chrom"]), u["start"].tolist(), u["end"].tolist()))
    cons = str(tmp / "consensus_sorted.bed")
    with open(cons, "w") as fh:
        fh.write("".join(f"{c}\t{a}\t{b}\n" for c, a, b in rows))
    every = sorted({ln.split("\t")[3] for ln in gzip.open(frag, "rt").read().splitlines()}, key=str.encode)
    return frag, cons, len(rows), oracle_dict(frag, cons, len(rows)), every


def test_synthetic_shape_equals_the_oracle(synthetic):
    import torch

    from gtars_amd.scoring import barcode_count_matrix

    frag, cons, n_peaks, exp, every = synthetic
    m = barcode_count_matrix(frag, cons)
    assert m.to_dict() == exp and m.shape == (len(exp), n_peaks) and m.barcodes == sorted(exp, key=str.encode)
    full = barcode_count_matrix(frag, cons, keep_empty=True)
    assert full.barcodes == every and full.shape == (len(every), n_peaks)
    assert full.to_dict() == {bc: exp.get(bc, {}) for bc in every}
    d = barcode_count_matrix(frag, cons, device=True)
    assert all(isinstance(t, torch.Tensor) and t.is_cuda for t in (d.indptr, d.indices, d.data))
    assert d.indptr.dtype == torch.int64 and d.indices.dtype == torch.int32 and d.data.dtype == torch.int32
    assert d.barcodes == m.barcodes and d.shape == m.shape
    for a, b in zip((d.indptr, d.indices, d.data), (m.indptr, m.indices, m.data)):
        assert np.array_equal(a.cpu().numpy(), b)
    assert d.to_dict() == exp


@pytest.mark.parametrize("mode", ["chip", "atac"])
def test_column_sums_equal_the_dense_file_row(synthetic, mode):
    from gtars_amd.scoring import barcode_count_matrix, region_scoring_from_fragments

    for frag, cons in ((synthetic[0], synthetic[1]), (FRAG1, CONS1), (FRAG2, CONS1)):
        m = barcode_count_matrix(frag, cons, scoring_mode=mode)
        dense = region_scoring_from_fragments([frag], cons, mode)[0]
        sums = np.bincount(m.indices, weights=m.data.view(np.uint32), minlength=m.shape[1]).astype(np.int64)
        assert sums.tolist() == dense.astype(np.int64).tolist(), (frag, mode)


def test_two_files_as_one_matrix():
    from gtars_amd.scoring import barcode_count_matrix

    both = barcode_count_matrix([FRAG1, FRAG2], CONS1)
    singles = {}
    for stem, f in (("fragments1", FRAG1), ("fragments2", FRAG2)):
        singles.update({f"{stem}+{bc}": r for bc, r in barcode_count_matrix(f, CONS1).to_dict().items()})
    assert both.barcodes == sorted(singles, key=str.encode) and both.shape == (len(singles), 4)
    assert {lb.split("+")[0] for lb in both.barcodes} == {"fragments1", "fragments2"}
    assert both.to_dict() == singles
    # rows in label order: the two single-file matrices stacked and re-sorted
    rows = [sorted(singles[lb].items()) for lb in both.barcodes]
    assert both.indices.tolist() == [k for r in rows for k, _ in r] and both.data.tolist() == [v for r in rows for _, v in r]
    assert both.indptr.tolist() == np.cumsum([0] + [len(r) for r in rows]).tolist()


def test_empty_inputs_give_empty_matrices(tmp_path):
    from gtars_amd.scoring import barcode_count_matrix

    m = barcode_count_matrix([], CONS1)
    assert m.shape == (0, 4) and m.barcodes == [] and m.indptr.tolist() == [0] and m.nnz == 0 and m.to_dict() == {}
    none = tmp_path / "none.bed"
    none.write_text("")
    for keep in (False, True):
        m = barcode_count_matrix(str(none), CONS1, keep_empty=keep)
        assert m.shape == (0, 4) and m.nnz == 0
    far = tmp_path / "far.bed"  # fragments, none on a peak
    far.write_text("chr1\t5000\t5010\tAAA\t1\nchr9\t1\t2\tCCC\t1\n")
    assert barcode_count_matrix(str(far), CONS1).shape == (0, 4)
    m = barcode_count_matrix(str(far), CONS1, keep_empty=True, device=True)
    assert m.shape == (2, 4) and m.barcodes == ["AAA", "CCC"] and m.indptr.cpu().tolist() == [0, 0, 0] and m.to_dict() == {"AAA": {}, "CCC": {}}


def test_write_mtx_of_a_device_built_matrix(synthetic, tmp_path):
    from scipy.io import mmread

    from gtars_amd.scoring import barcode_count_matrix, write_sparse_counts_to_mtx

    frag, cons, n_peaks, exp, _ = synthetic
    m = barcode_count_matrix(frag, cons, device=True)
    m.write_mtx(str(tmp_path / "csr"))
    got = mmread(gzip.open(str(tmp_path / "csr") + "_matrix.mtx.gz")).tocsr()
    names = gzip.open(str(tmp_path / "csr") + "_barcodes.tsv.gz", "rt").read().split()
    assert names == sorted(exp, key=str.encode) and got.shape == (len(exp), n_peaks) and got.nnz == sum(len(r) for r in exp.values())
    for ri, bc in enumerate(names):
        assert {int(k): int(v) for k, v in zip(got[ri].indices, got[ri].data)} == exp[bc]
    assert (got != m.to_scipy()).nnz == 0
    write_sparse_counts_to_mtx(exp, n_peaks, str(tmp_path / "dict"))
    for part in ("_matrix.mtx.gz", "_barcodes.tsv.gz", "_features.tsv.gz"):
        assert gzip.open(str(tmp_path / "csr") + part, "rb").read() == gzip.open(str(tmp_path / "dict") + part, "rb").read(), part
