"""The batched tokenizer (K15) without a GPU: the restatement tests/tokbatch_ref.py, fed with the oracle's per-query CSR,
against the oracle's own Tokenizer::encode set by set on the reference's tokenizer fixtures (25 regions + 7 specials,
unk = 25, pad = 26), the known-answer batch, malformed set offsets, and the no-device error of every new entry point."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tokbatch_ref as T  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOK = os.path.join(GOLD, "tokenizers")

HIT6 = ("chr1", 151399441, 151399547)
HIT78 = ("chr2", 203871346, 203871616)
MISS = ("chr1", 10, 20)
KNOWN = [[HIT6], [MISS], [HIT78]]


def _oracle_rows(tok, sets, max_length=None):
    """the restatement over the oracle's CSR of the concatenated batch"""
    flat = [r for s in sets for r in s]
    qc, qs, qe = tok._encode_regions(flat)
    q_off, ids = tok.index.tokenize(qc, qs, qe)
    so = np.cumsum([0] + [len(s) for s in sets])
    return T.encode_sets(q_off, ids, so, tok.universe.region_to_id[tok.special["unk"]], max_length)


def _fixture_sets():
    import oracle

    peaks = [tuple(r[:3]) for r in oracle.read_region_set(os.path.join(TOK, "peaks.bed"), sort=False)]
    probes = [tuple(r[:3]) for r in oracle.read_region_set(os.path.join(GOLD, "to_tokenize.bed"))]
    wide = [(c, max(s, 100) - 100, e + 100) for c, s, e in peaks]
    return [probes, [], [MISS], peaks[:7], [("chrZ", 5, 50)], wide, [MISS, ("chrZ", 1, 2)], peaks[::-1], [HIT78, HIT6, HIT78]]


@pytest.mark.parametrize("cfg", ["tokenizer.toml", "tokenizer_ailist.toml", "tokenizer_custom_specials.toml", "peaks.bed"])
def test_restatement_is_the_oracle_set_by_set(cfg):
    import oracle

    tok = oracle.OracleTokenizer(os.path.join(TOK, cfg))
    sets = _fixture_sets()
    want = [tok.encode_regions(s) for s in sets]
    assert tok.universe.region_to_id[tok.special["unk"]] == 25 and tok.universe.region_to_id[tok.special["pad"]] == 26
    assert want[1] == want[2] == want[4] == want[6] == [25]
    assert _oracle_rows(tok, sets) == want
    for ml in (1, 2, 5, 1000):
        assert _oracle_rows(tok, sets, ml) == [w[:ml] for w in want]


def test_known_answer_batch():
    import oracle

    tok = oracle.OracleTokenizer(os.path.join(TOK, "tokenizer.toml"))
    rows = _oracle_rows(tok, KNOWN)
    assert rows == [[6], [25], [7, 8]]
    off, ids = T.ragged(rows)
    assert off.tolist() == [0, 1, 2, 4] and ids.tolist() == [6, 25, 7, 8]
    right, mask = T.pad_sets(rows, 26)
    assert right.tolist() == [[6, 26], [25, 26], [7, 8]] and mask.tolist() == [[1, 0], [1, 0], [1, 1]]
    left, lmask = T.pad_sets(rows, 26, side="left")
    assert left.tolist() == [[26, 6], [26, 25], [7, 8]] and lmask.tolist() == [[0, 1], [0, 1], [1, 1]]
    wide, wmask = T.pad_sets(rows, 26, width=3, side="left")
    assert wide.tolist() == [[26, 26, 6], [26, 26, 25], [26, 7, 8]] and wmask.sum() == 4
    with pytest.raises(ValueError):
        T.pad_sets(rows, 26, width=1)
    assert T.pad_sets(_oracle_rows(tok, KNOWN, 1), 26)[0].tolist() == [[6], [25], [7]]
    assert T.pad_sets([], 26)[0].shape == (0, 0) and T.pad_sets([], 26, width=4)[0].shape == (0, 4)


def test_restatement_refuses_malformed_set_offsets():
    q_off, ids = np.array([0, 1, 1, 3], dtype=np.uint64), np.array([4, 5, 6], dtype=np.uint32)
    assert T.encode_sets(q_off, ids, [0, 0, 2, 3, 3], 9) == [[9], [4], [5, 6], [9]]
    for bad in ([1, 3], [0, 2, 1, 3], [0, 2], [0, 4], []):
        with pytest.raises(ValueError):
            T.encode_sets(q_off, ids, bad, 9)
    with pytest.raises(ValueError):
        T.encode_sets(q_off, ids, [0, 3], 9, max_length=0)


def test_every_new_entry_point_is_declared_and_bound():
    import gtars_amd._lib as L

    for name in ("gtars_tokenize_sets_device", "gtars_pad_sets_device"):
        assert name in L.EXPORTED_SYMBOLS
    for name in ("gtars_tokenizer_encode_sets", "gtars_tokenizer_encode_sets_ids", "gtars_tokenizer_encode_sets_padded"):
        assert name in L.EXPORTED_HOST_SYMBOLS
    assert L.lib.gtars_debug_tokbatch_tile() >= 64
    from gtars.tokenizers import Tokenizer

    for m in ("encode_many", "tokenize_many", "encode_many_arrays", "batch"):
        assert callable(getattr(Tokenizer, m))
    from gtars_amd import OverlapIndex

    assert callable(OverlapIndex.tokenize_sets_device) and callable(OverlapIndex.pad_sets_device)


def _entry_calls():
    """every new C entry point, called without a handle"""
    import gtars_amd._lib as L

    lib = L.lib
    so = np.zeros(1, dtype=np.uint64)
    p1, p2, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
    return [
        ("gtars_tokenize_sets_device", lambda: lib.gtars_tokenize_sets_device(None, None, None, None, 0, None, 0, 25, 0, None, None, 0,
                                                                              C.byref(n), C.byref(n), None)),
        ("gtars_pad_sets_device", lambda: lib.gtars_pad_sets_device(None, None, 1, 1, 26, 0, None, None, None)),
        ("gtars_tokenizer_encode_sets", lambda: lib.gtars_tokenizer_encode_sets(None, None, 0, 0, C.byref(p1), C.byref(p2), C.byref(n))),
        ("gtars_tokenizer_encode_sets_ids", lambda: lib.gtars_tokenizer_encode_sets_ids(None, None, None, None, 0, L.ptr(so), 0, 0,
                                                                                        C.byref(p1), C.byref(p2), C.byref(n))),
        ("gtars_tokenizer_encode_sets_padded", lambda: lib.gtars_tokenizer_encode_sets_padded(None, None, None, None, 0, L.ptr(so), 0, 0, 0,
                                                                                              0, C.byref(p1), C.byref(p2), C.byref(n))),
    ]


@pytest.mark.parametrize("name", [n for n, _ in _entry_calls()])
def test_batched_entry_points_have_no_cpu_fallback(name):
    """without a device: GTARS_ERR_NO_DEVICE, whatever the arguments; with one: the missing handle is an argument error"""
    import gtars_amd
    import gtars_amd._lib as L

    call = dict(_entry_calls())[name]
    st = call()
    if gtars_amd.device_count() == 0:
        assert st == L.ERR_NO_DEVICE
        with pytest.raises(gtars_amd.NoDeviceError):
            L.check(st)
    else:
        assert st == L.ERR_INVALID_ARG


def test_tokenizer_cannot_be_built_without_a_device():
    import gtars_amd

    if gtars_amd.device_count() > 0:
        return
    from gtars.tokenizers import Tokenizer

    with pytest.raises(RuntimeError):
        Tokenizer(os.path.join(TOK, "tokenizer.toml")).encode_many([[]])
