"""K22 on the device (csrc/refget_pack.hip) against the bit-by-bit restatement (tests/refget_pack_ref.py): k_refget_pack's exact
bytes and zero padding at the symbol-group, lane and workgroup edges; the packed substring fill (k_refget_fill_packed) at every
start phase, width and CSR offset, through both entry forms and over several trips of k_csr_fill; the store on top of them."""
import os
import random

import numpy as np
import pytest

import refget_pack_ref as P
from test_refget_store_cpu import CHRF_COL, FIXTURE, MIXED, _regions, mixed_fasta, read

pytestmark = pytest.mark.gpu

# 64 symbols per lane, 256 lanes per workgroup
EDGE_LENGTHS = [0, 1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 16383, 16384, 16385]
# both letter cases, and bytes outside each table (a zero byte included: the 3-bit table maps it to 7)
LETTERS = (b"ACGTacgt" + b"Nx\x00", b"ACGTNRYacgtnry" + b"X-\x00\xff", b"ACGTURYSWKMBDHVNacgturyswkmbdhvn" + b"EZ*\x00",
           b"ACDEFGHIKLMNPQRSTVWY*X-.acdefghiklmnpqrstvwyx" + b"BJOUZ7\x00", bytes(range(256)))
PARTIAL = 45  # 45 symbols end inside a byte at 2, 3, 4 and 5 bits


@pytest.fixture(scope="module")
def G():
    import gtars_amd.refget as G

    return G


@pytest.fixture(scope="module")
def edge_records():
    """(sequences, classes) of ONE collection: every edge length at every width, empty records between the widths; and what the
    restatement makes of them, computed once"""
    rng = random.Random(2222)
    seqs, classes = [], []
    for cls in range(5):
        for n in EDGE_LENGTHS:
            seqs.append(bytes(rng.choice(LETTERS[cls]) for _ in range(n)))
            classes.append(cls)
        seqs.append(b""), classes.append((cls + 1) % 5)
    packed = [P.encode(q, c) for q, c in zip(seqs, classes)]
    text = [P.decode(e, 0, 0, len(q), c) for q, e, c in zip(seqs, packed, classes)]
    return seqs, classes, packed, text


def test_pack_kernel_exact_bytes_and_zero_padding(G, edge_records):
    seqs, classes, packed, _ = edge_records
    handle = G._Handle.from_buffers(seqs)
    pack = G._Pack.from_handle(handle, classes)          # k_refget_pack, one launch for the whole collection
    host = G._Pack.from_handle(handle, classes, on_host=True)
    assert len(pack) == len(seqs) and pack.image_bytes == host.image_bytes and pack.image_bytes % 16 == 0
    for i, (q, cls, want) in enumerate(zip(seqs, classes, packed)):
        data, length, got_cls = pack.record(i, padding=16)
        assert (length, got_cls) == (len(q), cls)
        assert len(want) == (len(q) * P.BITS[cls] + 7) // 8
        assert data[:len(want)] == want, (cls, len(q))
        spare = 8 * len(want) - len(q) * P.BITS[cls]  # the unused low bits of the last byte
        if spare:
            assert data[len(want) - 1] & ((1 << spare) - 1) == 0, (cls, len(q))
        assert data[len(want):] == bytes(16), (cls, len(q))  # 16 zero bytes behind every record, the 3-bit ones included
        assert host.record(i, padding=16) == (data, length, got_cls)


def test_whole_record_decode(G, edge_records):
    """Encoded to Raw: every record from 0 to its length is the input upper-cased -- through the tables, so a byte outside one is
    its default and IUPAC goes through the non-inverse"""
    seqs, classes, packed, text = edge_records
    pack = G._Pack.from_buffers(packed, [len(q) for q in seqs], classes)
    off, blob = pack.decode_records()
    assert list(off) == list(np.concatenate([[0], np.cumsum([len(q) for q in seqs])]))
    for i, want in enumerate(text):
        assert blob[off[i]:off[i + 1]] == want, (classes[i], len(want))
    acgt = [i for i, (q, c) in enumerate(zip(seqs, classes)) if c == 4]
    assert all(text[i] == bytes(P.upper(b) for b in seqs[i]) for i in acgt)
    iupac = G._Pack.from_buffers([P.encode(b"ACGTDHUdhuN", 2)], [11], [2])
    assert iupac.decode_records()[1] == b"ACGTHVTHVTN"
    off_h, blob_h = pack.decode_records(on_host=True)
    assert list(off_h) == list(off) and blob_h == blob


def _substring_rows():
    """per width one record of PARTIAL symbols: every start phase modulo 8 crossed with widths 0 .. 17, then ranges that end at
    the record's end; a missing sequence (status 1) or a bad range (status 2) after every seventh row"""
    rows = []
    for rec in range(5):
        for start in range(8, 16):
            for width in range(18):
                rows.append((rec, start, start + width))
        for width in range(18):
            rows.append((rec, PARTIAL - width, PARTIAL))
    out = []
    for k, row in enumerate(rows):
        out.append(row)
        if k % 7 == 3:
            out.append((0xFFFFFFFF, 0, 1) if k % 2 else (row[0], PARTIAL - 1, PARTIAL + 1))
        if k % 7 == 5:
            out.append((row[0], 9, 4) if k % 2 else (5, 0, 1))
    return out


@pytest.fixture(scope="module")
def phase_world(G):
    rng = random.Random(2223)
    seqs = [bytes(rng.choice(LETTERS[cls]) for _ in range(PARTIAL)) for cls in range(5)]
    packed = [P.encode(q, c) for c, q in enumerate(seqs)]
    text = [P.decode(e, 0, 0, PARTIAL, c) for c, e in enumerate(packed)]
    rows = _substring_rows()
    expect = []
    for rec, start, end in rows:
        if rec >= 5:
            expect.append((1, b""))
        elif start == end:
            expect.append((0, b""))
        elif start >= PARTIAL or end > PARTIAL or start >= end:
            expect.append((2, b""))
        else:
            expect.append((0, text[rec][start:end]))
    off = np.concatenate([[0], np.cumsum([len(b) for _, b in expect])])
    live = [int(off[i]) % 8 for i, (_, b) in enumerate(expect) if b]
    assert set(live) == set(range(8))  # rows begin at every offset modulo 8 of the CSR
    assert {st for st, _ in expect} == {0, 1, 2}
    return packed, rows, expect, off


def _check_host_columns(pack, rows, expect, off, on_host=False):
    status, got_off, blob = pack.substrings([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], on_host)
    assert list(status) == [st for st, _ in expect]
    assert list(got_off) == list(off)
    assert blob == b"".join(b for _, b in expect)


def test_packed_substrings_host_columns(G, phase_world):
    packed, rows, expect, off = phase_world
    pack = G._Pack.from_buffers(packed, [PARTIAL] * 5, range(5))
    _check_host_columns(pack, rows, expect, off)
    _check_host_columns(pack, rows, expect, off, on_host=True)
    status, got_off, blob = pack.substrings([], [], [], False)
    assert len(status) == 0 and list(got_off) == [0] and blob == b""


def test_packed_substrings_device_columns(G, phase_world):
    import torch

    from gtars_amd._lib import CapacityError

    packed, rows, expect, off = phase_world
    pack = G._Pack.from_buffers(packed, [PARTIAL] * 5, range(5))
    dev = torch.device("cuda", torch.cuda.current_device())
    put = lambda values, np_dtype, as_dtype: torch.from_numpy(np.array(values, dtype=np_dtype).view(as_dtype).copy()).to(dev)  # noqa: E731
    k, total = len(rows), int(off[-1])
    seq = put([r[0] for r in rows], np.uint32, np.int32)
    start, end = put([r[1] for r in rows], np.uint64, np.int64), put([r[2] for r in rows], np.uint64, np.int64)
    status = torch.full((k,), 77, dtype=torch.uint8, device=dev)
    offsets = torch.zeros(k + 1, dtype=torch.int64, device=dev)
    out = torch.full((total + 8,), 1, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = G.substrings_device(pack, seq.data_ptr(), start.data_ptr(), end.data_ptr(), k, status.data_ptr(), offsets.data_ptr(), out.data_ptr(),
                                  total, side.cuda_stream)
    assert got == total and status.cpu().tolist() == [st for st, _ in expect]
    assert offsets.cpu().tolist() == [int(x) for x in off]
    data = out.cpu().numpy().tobytes()
    assert data[:total] == b"".join(b for _, b in expect) and data[total:] == b"\x01" * 8  # nothing behind the total
    with pytest.raises(CapacityError) as err:
        G.substrings_device(pack, seq.data_ptr(), start.data_ptr(), end.data_ptr(), k, status.data_ptr(), offsets.data_ptr(), out.data_ptr(), total - 1)
    assert err.value.needed == total
    with pytest.raises(ValueError, match="8-byte aligned"):
        G.substrings_device(pack, seq.data_ptr(), start.data_ptr(), end.data_ptr(), k, status.data_ptr(), offsets.data_ptr(), out.data_ptr() + 1, total)
    assert G.substrings_device(pack, 0, 0, 0, 0, 0, 0, 0, 0) == 0  # n == 0 touches nothing


def test_packed_fill_over_several_trips(G, phase_world, monkeypatch):
    """GTARS_GRID_CAP = 1: k_csr_fill walks its grid-stride loop several times over the packed row source"""
    import gtars_amd

    packed, rows, expect, off = phase_world
    assert int(off[-1]) > 3 * 2048  # k_csr_fill writes 2,048 bytes per workgroup and trip
    pack = G._Pack.from_buffers(packed, [PARTIAL] * 5, range(5))
    monkeypatch.setenv("GTARS_GRID_CAP", "1")
    before = gtars_amd._lib.lib.gtars_debug_grid_clips()
    _check_host_columns(pack, rows, expect, off)
    assert gtars_amd._lib.lib.gtars_debug_grid_clips() > before


# ---- the store -------------------------------------------------------------------------------------------------------------
def test_fixture_store_regions_on_the_device(G):
    store = G.RefgetStore.open_local(FIXTURE)
    seqs, status = G.substrings_many(store, CHRF_COL, ["chrF", "chrF", "chrG", "chrF", "chrF"], [0, 37, 0, 30, 7], [5, 40, 1, 41, 7], with_status=True)
    assert seqs == ["ACGTA", "CGT", None, None, ""] and list(status) == [0, 0, 1, 2, 0]
    chrf = store.list_sequences()[0].sha512t24u
    assert store.get_substrings(chrf, [(1, 9), (40, 40), (36, 40)]) == ["CGTACGTA", "", "ACGT"]


def test_store_written_on_the_device_and_reopened_as_stubs(G, tmp_path):
    fasta = mixed_fasta(tmp_path / "mixed.fa")
    memory = G.RefgetStore.in_memory()
    meta, _ = memory.add_sequence_collection_from_fasta(fasta)
    store = G.RefgetStore.on_disk(tmp_path / "dev")
    store.add_sequence_collection_from_fasta(fasta)                      # packed by k_refget_pack, written by the library
    host = G.RefgetStore.on_disk(tmp_path / "host")
    host.add_sequence_collection_from_fasta(fasta, on_host=True)
    n_seq = 0
    for dirpath, _, files in os.walk(tmp_path / "host"):
        for f in files:
            if f != "rgstore.json":
                rel = os.path.relpath(os.path.join(dirpath, f), tmp_path / "host")
                assert read(tmp_path / "dev" / rel) == read(os.path.join(dirpath, f)), rel
                n_seq += f.endswith(".seq")
    assert n_seq == len(MIXED)
    chroms, starts, ends = _regions()
    want, want_status = G.substrings_many(memory, meta.digest, chroms, starts, ends, with_status=True)
    classes = {m.name: m.alphabet.value for m in memory.list_sequences()}
    classes["two"] = 0
    through = [None if w is None else P.round_trip(w.encode("latin-1"), classes[c]).decode("latin-1") for w, c in zip(want, chroms)]
    # the image the add left behind, then the image a reopened store builds from the .seq files
    for s in (store, G.RefgetStore.open_local(tmp_path / "dev")):
        assert all(not r.is_loaded for r in s.iter_sequences())
        got, status = G.substrings_many(s, meta.digest, chroms, starts, ends, with_status=True)
        assert list(status) == list(want_status) and got == through


def test_enable_then_disable_encoding_returns_the_text(G, tmp_path):
    store = G.RefgetStore.in_memory()
    meta, _ = store.add_sequence_collection_from_fasta(mixed_fasta(tmp_path / "mixed.fa"))
    text = {r.metadata.sha512t24u: (r.sequence, r.metadata.alphabet.value) for r in store.iter_sequences()}
    chroms, starts, ends = _regions()
    raw = G.substrings_many(store, meta.digest, chroms, starts, ends)
    store.enable_encoding()
    assert store.storage_mode == G.StorageMode.Encoded
    for sha, (seq, cls) in text.items():
        rec = store.get_sequence(sha)
        assert rec.encoded and rec.sequence == P.encode(seq, cls)
    classes = {m.name: m.alphabet.value for m in store.list_sequences()}
    classes["two"] = 0
    packed = G.substrings_many(store, meta.digest, chroms, starts, ends)  # from the packed image of the records' bytes
    assert packed == [None if w is None else P.round_trip(w.encode("latin-1"), classes[c]).decode("latin-1") for w, c in zip(raw, chroms)]
    store.disable_encoding()
    assert store.storage_mode == G.StorageMode.Raw
    for sha, (seq, cls) in text.items():
        rec = store.get_sequence(sha)
        assert not rec.encoded and rec.sequence == P.round_trip(seq, cls)
