"""The sparse count matrix (K16) without a GPU: the restatement tests/countmat_ref.py against the oracle's per-barcode peak
counts on the reference's scoring fixtures, SparseCounts (to_dict, to_scipy, write_mtx) on hand-written arrays, and the argument
checks of gtars_count_matrix_csr_device that come before the device is asked for."""
import ctypes as C
import gzip
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import countmat_ref as R  # noqa: E402

FRAG1, CONS1, oracle_dict = R.FRAG1, R.CONS1, R.oracle_dict


def test_restatement_gives_the_oracles_barcode_counts():
    peaks = [ln.split() for ln in open(CONS1).read().splitlines() if ln.strip()]
    peaks = [(c, int(a), int(b)) for c, a, b in peaks]
    assert peaks == sorted(peaks)  # line number == rank in (chr, start) order
    frags = [ln.split() for ln in gzip.open(FRAG1, "rt").read().splitlines() if ln.strip() and not ln.startswith("#")]
    barcodes = sorted({f[3] for f in frags}, key=str.encode)
    # hits per fragment by the definition of an overlap, no search structure
    hits = [[k for k, (c, a, b) in enumerate(peaks) if c == f[0] and int(f[1]) < b and int(f[2]) > a] for f in frags]
    offsets = np.cumsum([0] + [len(h) for h in hits]).astype(np.uint64)
    ids = np.asarray([k for h in hits for k in h], dtype=np.uint32)
    row = np.asarray([barcodes.index(f[3]) for f in frags], dtype=np.uint32)
    indptr, indices, data = R.count_matrix_ref(offsets, ids, row, len(barcodes), len(peaks))
    exp = oracle_dict(FRAG1, CONS1, len(peaks))
    assert exp and R.csr_to_dict(barcodes, indptr, indices, data) == exp
    assert indptr[0] == 0 and indptr[-1] == len(indices) == sum(len(r) for r in exp.values())


def test_restatement_drop_rules_and_plateaus():
    #            q0: 2 hits   q1: none  q2: 3 hits        q3 (row out of range)
    offsets = np.array([0, 2, 2, 5, 6], dtype=np.uint64)
    ids = np.array([1, 1, 0, 7, 1, 0], dtype=np.uint32)  # 7 >= n_cols: dropped
    row = np.array([2, 0, 2, 9], dtype=np.uint32)
    indptr, indices, data = R.count_matrix_ref(offsets, ids, row, 4, 3)
    assert indptr.tolist() == [0, 0, 0, 2, 2] and indices.tolist() == [0, 1] and data.tolist() == [1, 3]
    indptr, indices, data = R.count_matrix_ref(np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32), 3, 5)
    assert indptr.tolist() == [0, 0, 0, 0] and len(indices) == 0 and len(data) == 0


def _hand_built():
    from gtars_amd.scoring import SparseCounts

    # labels NOT in byte order (capitals sort before lower case), one row without a count, one count beyond 2^31
    barcodes = ["b", "C", "a", "B"]
    indptr = np.array([0, 2, 2, 3, 6], dtype=np.int64)
    indices = np.array([0, 4, 2, 1, 3, 4], dtype=np.int32)
    data = np.array([1, 2, 3_000_000_000, 5, 6, 7], dtype=np.uint32).view(np.int32)
    exp = {"b": {0: 1, 4: 2}, "C": {}, "a": {2: 3_000_000_000}, "B": {1: 5, 3: 6, 4: 7}}
    return SparseCounts(barcodes, indptr, indices, data, (4, 5)), exp


def test_sparse_counts_to_dict_and_to_scipy():
    from gtars_amd.scoring import SparseCounts

    m, exp = _hand_built()
    assert m.to_dict() == exp and m.nnz == 6 and m.shape == (4, 5)
    sp = m.to_scipy()
    assert sp.shape == (4, 5) and sp.nnz == 6
    dense = np.zeros((4, 5), dtype=np.int64)
    for i, bc in enumerate(m.barcodes):
        for k, v in exp[bc].items():
            dense[i, k] = v
    assert np.array_equal(sp.toarray().astype(np.int64), dense)
    with pytest.raises(ValueError):
        SparseCounts(["a"], np.zeros(3, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), (1, 5))


def test_write_mtx_is_byte_identical_to_the_dict_writer(tmp_path):
    from scipy.io import mmread

    from gtars_amd.scoring import write_sparse_counts_to_mtx

    m, exp = _hand_built()
    m.write_mtx(str(tmp_path / "csr"))
    write_sparse_counts_to_mtx(m.to_dict(), 5, str(tmp_path / "dict"))
    for part in ("_matrix.mtx.gz", "_barcodes.tsv.gz", "_features.tsv.gz"):
        a, b = (gzip.open(str(tmp_path / k) + part, "rb").read() for k in ("csr", "dict"))
        assert a == b and a, part
    assert gzip.open(str(tmp_path / "csr") + "_barcodes.tsv.gz", "rt").read().split() == ["B", "C", "a", "b"]
    got = mmread(gzip.open(str(tmp_path / "csr") + "_matrix.mtx.gz")).tocsr()
    assert got.shape == (4, 5) and got[0].toarray().ravel().tolist() == [0, 5, 0, 6, 7] and got[1].nnz == 0
    assert int(got[2, 2]) == 3_000_000_000


def test_stem_drops_every_extension():
    from gtars_amd.scoring import _stem

    assert _stem("/x/y/fragments1.bed.gz") == "fragments1" and _stem("a.b.c.d") == "a" and _stem("plain") == "plain"
    assert _stem("/tmp/.hidden") == ".hidden" and _stem(".hidden.gz") == ".hidden"


def test_entry_point_argument_checks_need_no_device():
    import gtars_amd
    from gtars_amd._lib import lib
    from gtars_amd.scoring import barcode_count_matrix

    nnz = C.c_uint64(77)
    buf = (C.c_uint64 * 8)()
    p = C.cast(buf, C.c_void_p)
    call = lib.gtars_count_matrix_csr_device
    inv = gtars_amd._lib.ERR_INVALID_ARG
    assert call(None, None, None, 0, 3, 5, None, None, None, 0, C.byref(nnz), None) == inv  # d_indptr
    assert call(None, None, None, 0, 3, 5, p, None, None, 0, None, None) == inv  # nnz
    assert call(None, None, p, 4, 3, 5, p, None, None, 0, C.byref(nnz), None) == inv  # offsets with nq != 0
    assert call(p, None, None, 4, 3, 5, p, None, None, 0, C.byref(nnz), None) == inv  # rows with nq != 0
    assert call(None, None, None, 0, 3, 5, p, None, p, 4, C.byref(nnz), None) == inv  # indices with capacity != 0
    assert call(None, None, None, 0, 3, 5, p, p, None, 4, C.byref(nnz), None) == inv  # data with capacity != 0
    assert call(None, None, None, 0, 0xFFFFFFFF, 5, p, None, None, 0, C.byref(nnz), None) == inv
    assert "rows" in gtars_amd._lib.last_error()
    if gtars_amd.device_count() == 0:  # valid arguments: the loud error, not a fallback
        assert call(None, None, None, 0, 3, 5, p, None, None, 0, C.byref(nnz), None) == gtars_amd._lib.ERR_NO_DEVICE
        with pytest.raises(gtars_amd.NoDeviceError):
            barcode_count_matrix(FRAG1, CONS1)
    with pytest.raises(ValueError, match="Invalid scoring mode"):
        barcode_count_matrix(FRAG1, CONS1, scoring_mode="nope")
