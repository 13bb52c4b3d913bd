"""K22 on the host: the bit arithmetic of csrc/refget_pack_core.h through the scalar calls and the `on_host=True` paths against
the bit-by-bit restatement (tests/refget_pack_ref.py), and the store directory against files the reference's programs wrote
(tests/golden/refget_store: its example store of one collection, chrF = ACGT x 10, Encoded; and base.rgsi, the four-header
form without ancillary digests).  No test here needs a device."""
import json
import os
import random
import re
import shutil
import subprocess

import pytest

import refget_pack_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "refget_store")
FIXTURE = os.path.join(GOLDEN, "teststore")
BASE_FA = os.path.join(HERE, "golden", "fasta", "base.fa")
CHRF = "71mfZw47FLWJKQ_wvBCMgGungdTJFoft"
CHRF_COL = "ZTJcAsOf3mUXU8XEnruxC4h4SCA_1n6X"
STORE_FILES = ("sequences.rgsi", "collections.rgci", f"collections/{CHRF_COL}.rgsi", f"sequences/71/{CHRF}.seq")

# one record per alphabet class, an empty record, a repeated name and a description; both letter cases
MIXED = [("two", "the first of its name", b"ACGTacgtTTGGCCAAACGTACGTACGTACGTACGTA"), ("three", None, b"ACGTNNRYacgtnry"),
         ("iupac", None, b"ACGTURYSWKMBDHVNacgturyswkmbdhvn"), ("prot", "a protein", b"MEFILPQX*-.ACDGHKNRSTVWYmefilpqx"),
         ("text", None, b"Hello,World!123@z"), ("empty", None, b""), ("two", None, b"GGCCggccA")]
MIXED_CLASSES = [0, 1, 2, 3, 4, 0, 0]


@pytest.fixture(scope="module")
def G():
    import gtars_amd.refget as G

    return G


def mixed_fasta(path):
    with open(path, "wb") as f:
        for name, desc, seq in MIXED:
            f.write(b">" + name.encode() + (b" " + desc.encode() if desc else b"") + b"\n")
            f.write(b"".join(seq[at:at + 10] + b"\n" for at in range(0, len(seq), 10)))
    return path


def read(path):
    with open(path, "rb") as f:
        return f.read()


# ---- the bit arithmetic ---------------------------------------------------------------------------------------------------
def test_known_answers(G):
    assert [G.bits_per_symbol(c) for c in range(6)] == [2, 3, 4, 5, 8, 8] == list(P.BITS)
    assert G.bits_per_symbol(G.AlphabetType.Protein) == 5
    assert G.encode_sequence("ACGT", G.AlphabetType.Dna2bit) == b"\x9c"
    assert G.encode_sequence(b"ACGTNRYX", 1) == bytes([0x05, 0x39, 0x77])
    assert G.encode_sequence(b"", 3) == b""
    assert G.decode_substring(b"\x9c", 0, 4, 0) == b"ACGT" and G.decode_substring(b"\x9c", 1, 3, 0) == b"CG"
    assert G.decode_substring(b"\x9c", 3, 3, 0) == b"" and G.decode_substring(b"\x9c", 3, 1, 0) == b""
    assert G.byte_range_for_bases(0, 4, 2) == (0, 1) and G.byte_range_for_bases(5, 9, 3) == (1, 4) == P.byte_range(5, 9, 3)
    assert G.byte_range_for_bases(7, 7, 5) == (4, 5)


def test_the_iupac_tables_are_no_inverse_pair(G):
    """the reference's DNA_IUPAC_DECODING_ARRAY has D at 11 (no base encodes to it), H at 13 and V at 14 and 15: D comes back as
    H, H as V, U as T"""
    enc = G.encode_sequence(b"DHUdhu", 2)
    assert enc == bytes([0xDE, 0x8D, 0xE8])
    assert G.decode_substring(enc, 0, 6, 2) == b"HVTHVT" == P.round_trip(b"DHUdhu", 2)
    assert G.decode_substring(G.encode_sequence(b"ACGTRYSWKMBVN", 2), 0, 13, 2) == b"ACGTRYSWKMBVN"


@pytest.mark.parametrize("cls", range(6))
def test_every_byte_through_every_table(G, cls):
    every = bytes(range(256))
    enc = G.encode_sequence(every, cls)
    assert enc == P.encode(every, cls)
    assert G.decode_substring(enc, 0, 256, cls) == P.decode(enc, 0, 0, 256, cls) == P.round_trip(every, cls)
    bits = P.BITS[cls]
    table = bytes(P.decode_table(cls))
    # every code of the width once, packed bit by bit, through the library's decoder
    packed = bytearray((len(table) * bits + 7) // 8)
    for i, code in enumerate(range(1 << bits)):
        for j in range(bits):
            pos = i * bits + j
            packed[pos // 8] |= ((code >> (bits - 1 - j)) & 1) << (7 - pos % 8)
    assert G.decode_substring(bytes(packed), 0, len(table), cls) == table


@pytest.mark.parametrize("cls", range(5))
def test_decoder_differential_with_windows_and_zero_fill(G, cls):
    """the reference's own differential test (encoder.rs, mod tests): random packed buffers, ranges that run up to 16 symbols past
    the end, windows that begin at a random byte_offset; bits outside the window are zero"""
    rng = random.Random(2200 + cls)
    bits = P.BITS[cls]
    for n in (0, 1, 3, 4, 5, 7, 8, 17, 64, 257, 1000):
        n_bytes = (n * bits + 7) // 8
        buf = bytes(rng.randrange(256) for _ in range(n_bytes))
        for _ in range(40):
            start = rng.randrange(0, n + 1)
            end = rng.randrange(start, min(n + 16, start + 40) + 1)
            assert G.decode_substring(buf, start, end, cls) == P.decode(buf, 0, start, end, cls), (n, start, end)
            w0 = rng.randrange(0, n_bytes + 1)
            w1 = rng.randrange(w0, n_bytes + 1)
            assert G.decode_substring(buf[w0:w1], start, end, cls, byte_offset=w0) == P.decode(buf[w0:w1], w0, start, end, cls), (n, start, end, w0, w1)
            b0, b1 = G.byte_range_for_bases(start, min(end, n), bits)
            assert (b0, b1) == P.byte_range(start, min(end, n), bits)
            if start < min(end, n):  # the bytes the range needs are enough
                assert G.decode_substring(buf[b0:b1], start, min(end, n), cls, byte_offset=b0) == P.decode(buf, 0, start, min(end, n), cls)


def test_three_bit_record_of_five_symbols_ends_on_a_zero_bit(G):
    """15 bits in two bytes: the table maps whatever lies behind the record to 7, the low bit of the last byte is zero all the same"""
    enc = G.encode_sequence(b"XXXXX", 1)
    assert enc == bytes([0xFF, 0xFE]) == P.encode(b"XXXXX", 1)
    assert G.encode_sequence(b"NRYXA", 1)[-1] & 1 == 0


# ---- the fixture store -----------------------------------------------------------------------------------------------------
def test_open_the_reference_store(G):
    store = G.RefgetStore.open_local(FIXTURE)
    assert store.storage_mode == G.StorageMode.Encoded and str(store.storage_mode) == "Encoded"
    assert store.is_persisting and store.cache_path == FIXTURE and "memory-only" not in repr(store)
    (meta,) = store.list_collections()
    assert (meta.digest, meta.n_sequences) == (CHRF_COL, 1)
    assert store.get_collection_level1(CHRF_COL) == {
        "names": "yEbCnEzUFHtAA2fDncuUKB332VPrNKXS", "lengths": "0HMaoP--cS86GDenYkwHaf0tTIjXOAR_", "sequences": "-u1i7bFwmdhMasqhyMjKtIMWsUV42-4-",
        "name_length_pairs": "dGnxaZflc62bQpE9bJ617bjIgj3i50bH", "sorted_name_length_pairs": "xJegtCcDbe0C4tx8AqzZoJ814vOIvlVA",
        "sorted_sequences": "-u1i7bFwmdhMasqhyMjKtIMWsUV42-4-"}
    assert not store.is_collection_loaded(CHRF_COL)
    (m,) = store.list_sequences()
    assert (m.name, m.length, str(m.alphabet), m.sha512t24u, m.md5, m.description) == ("chrF", 40, "dna2bit", CHRF, "9889878875bfc855a532253c415dceb6", None)
    rec = store.get_sequence(CHRF)
    assert not rec.is_loaded and rec.decode() is None
    # a stub: the range comes from a window of the file
    assert store.get_substring(CHRF, 3, 11) == "TACGTACG" and store.get_substring(m.md5, 39, 40) == "T"
    assert store.get_substring(CHRF, 40, 40) == "" and store.get_substring(CHRF, 99, 99) == ""
    for start, end in ((40, 41), (0, 41), (5, 3)):
        with pytest.raises(KeyError, match=f"Invalid substring range: start={start}, end={end}, sequence length=40"):
            store.get_substring(CHRF, start, end)
    with pytest.raises(KeyError, match="Sequence not found: nope"):
        store.get_substring("nope", 0, 1)
    assert store.get_substrings(CHRF, [(0, 4), (38, 40), (40, 40)], on_host=True) == ["ACGT", "GT", ""]
    with pytest.raises(KeyError, match="Invalid substring range: start=39, end=41, sequence length=40"):
        store.get_substrings(CHRF, [(0, 4), (39, 41)], on_host=True)
    store.load_all_sequences()
    rec = store.get_sequence(CHRF)
    assert rec.is_loaded and rec.sequence == b"\x9c" * 10 and rec.decode() == "ACGT" * 10
    assert store.get_substring(CHRF, 3, 11) == "TACGTACG"
    store.load_all_collections()
    assert store.is_collection_loaded(CHRF_COL) and store.get_sequence_by_name(CHRF_COL, "chrF") is rec
    seqs, status = G.substrings_many(store, CHRF_COL, ["chrF", "chrF", "chrG", "chrF"], [0, 37, 0, 30], [5, 40, 1, 41], on_host=True, with_status=True)
    assert seqs == ["ACGTA", "CGT", None, None] and list(status) == [0, 0, 1, 2]


def test_a_stub_substring_reads_only_its_window(G, tmp_path):
    """every byte of the .seq file outside byte_range_for_bases of the range is overwritten: the answer stays"""
    root = tmp_path / "store"
    store = G.RefgetStore.on_disk(root)
    meta, _ = store.add_sequence_collection_from_fasta(mixed_fasta(tmp_path / "mixed.fa"), on_host=True)
    for r, cls in zip(store.get_collection(meta.digest), (0, 1, 2, 3, 4, 0)):  # (one record per name: the last "two")
        m = r.metadata
        if m.length < 8:
            continue
        path = root / "sequences" / m.sha512t24u[:2] / f"{m.sha512t24u}.seq"
        data = bytearray(read(path))
        text = P.round_trip(dict((n, s) for n, _, s in MIXED)[m.name], m.alphabet.value)
        start, end = 3, m.length - 2
        b0, b1 = P.byte_range(start, end, P.BITS[m.alphabet.value])
        for k in range(len(data)):
            if not b0 <= k < b1:
                data[k] ^= 0xFF
        path.write_bytes(bytes(data))
        assert store.get_substring(m.sha512t24u, start, end) == text[start:end].decode("latin-1")


def test_rebuild_the_reference_store_byte_for_byte(G, tmp_path):
    fasta = tmp_path / "chrF.fa"
    fasta.write_bytes(b">chrF\n" + b"ACGT" * 10 + b"\n")
    root = tmp_path / "store"
    store = G.RefgetStore.on_disk(root)
    assert store.storage_mode == G.StorageMode.Encoded and store.is_persisting
    assert all((root / sub).is_dir() for sub in ("sequences", "collections", "fhr"))
    meta, new = store.add_sequence_collection_from_fasta(fasta, on_host=True)
    assert new and meta.digest == CHRF_COL
    assert not store.get_sequence(CHRF).is_loaded  # a persisting store keeps stubs
    for rel in STORE_FILES:
        assert read(root / rel) == read(os.path.join(FIXTURE, rel)), rel
    text, want_text = read(root / "rgstore.json").decode(), read(os.path.join(FIXTURE, "rgstore.json")).decode()
    got, want = json.loads(text), json.loads(want_text)
    assert list(got) == list(want)  # the reference's key order
    assert {k: v for k, v in got.items() if k not in ("created_at", "modified")} == {k: v for k, v in want.items() if k not in ("created_at", "modified")}
    stamp = r"\d{4}-\d\d-\d\dT\d\d:\d\d:\d\d(\.\d+)?\+00:00"
    assert re.fullmatch(stamp, got["created_at"]) and re.fullmatch(stamp, got["modified"])
    # the same layout: two spaces, no trailing newline
    blank = lambda t: re.sub(r'("(?:created_at|modified)": ")[^"]*', r"\1", t)  # noqa: E731
    assert blank(text) == blank(want_text)
    # on_disk on a directory that holds a store opens it
    again = G.RefgetStore.on_disk(root)
    assert [m.sha512t24u for m in again.list_sequences()] == [CHRF] and again.get_substring(CHRF, 0, 8) == "ACGTACGT"
    again.write()
    assert json.loads(read(root / "rgstore.json"))["sequences_digest"] == want["sequences_digest"]


def _regions():
    names = [n for n, _, _ in MIXED] + ["nope"]
    chroms, starts, ends = [], [], []
    rng = random.Random(2207)
    last = {n: s for n, _, s in MIXED}
    for _ in range(60):
        c = rng.choice(names)
        n = len(last.get(c, b""))
        s = rng.randrange(0, n + 2)
        chroms.append(c), starts.append(s), ends.append(rng.randrange(s, n + 3))
    return chroms, starts, ends


@pytest.mark.parametrize("mode", ["Raw", "Encoded"])
@pytest.mark.parametrize("which", ["base", "mixed"])
def test_write_then_open_round_trip(G, tmp_path, mode, which):
    fasta = BASE_FA if which == "base" else mixed_fasta(tmp_path / "mixed.fa")
    memory = G.RefgetStore.in_memory()
    assert memory.storage_mode == G.StorageMode.Raw and "memory-only" in repr(memory) and not memory.is_persisting and memory.cache_path is None
    meta, _ = memory.add_sequence_collection_from_fasta(fasta, on_host=True)
    source = G.RefgetStore.in_memory()
    if mode == "Encoded":
        source.enable_encoding(on_host=True)
    source.add_sequence_collection_from_fasta(fasta, on_host=True)
    assert str(source.storage_mode) == mode
    root = tmp_path / "out"
    source.write_store_to_dir(root)
    manifest = json.loads(read(root / "rgstore.json"))
    assert manifest["mode"] == mode and "sequences_digest" not in manifest and "collections_digest" not in manifest
    opened = G.RefgetStore.open_local(root)
    assert str(opened.storage_mode) == mode and opened.is_persisting
    key = lambda m: (m.name, m.length, str(m.alphabet), m.sha512t24u, m.md5, m.description)  # noqa: E731
    assert [key(m) for m in opened.list_sequences()] == [key(m) for m in memory.list_sequences()]
    a, b = opened.list_collections()[0], memory.list_collections()[0]
    assert vars(a) == vars(b)
    assert opened.get_collection_level2(meta.digest) == memory.get_collection_level2(meta.digest)
    assert [key(r.metadata) for r in opened.get_collection(meta.digest)] == [key(r.metadata) for r in memory.get_collection(meta.digest)]
    # region calls on the stubs (the image comes from the .seq files) against the in-memory raw store's
    if which == "mixed":
        chroms, starts, ends = _regions()
    else:
        chroms, starts, ends = ["chrX", "chr1", "chr2", "chrX", "chr9", "chr1"], [0, 1, 4, 3, 0, 2], [8, 3, 4, 9, 1, 4]  # (statuses 0, 1 and 2)
    want, want_status = G.substrings_many(memory, meta.digest, chroms, starts, ends, on_host=True, with_status=True)
    got, status = G.substrings_many(opened, meta.digest, chroms, starts, ends, on_host=True, with_status=True)
    assert list(status) == list(want_status) and {0, 1, 2} <= set(status)
    if mode == "Raw":
        assert got == want
    else:  # (through the tables: bytes outside one come back as its default, IUPAC through the non-inverse)
        for g, w, c in zip(got, want, chroms):
            cls = next((m.alphabet.value for m in memory.list_sequences() if m.name == c), 0)
            assert g == (None if w is None else P.round_trip(w.encode("latin-1"), cls).decode("latin-1"))
    # every sequence loaded and decoded
    opened.load_all_sequences()
    for m in memory.list_sequences():
        rec, text = opened.get_sequence(m.sha512t24u), memory.get_sequence(m.sha512t24u).sequence
        assert rec.is_loaded and rec.encoded == (mode == "Encoded")
        if mode == "Encoded":
            assert rec.sequence == P.encode(text, m.alphabet.value)
            assert rec.decode() == P.round_trip(text, m.alphabet.value).decode("latin-1")
        else:
            assert rec.sequence == text and rec.decode() == text.decode("latin-1")
    # written again from the loaded records: the same files
    opened.write_store_to_dir(tmp_path / "again")
    for dirpath, _, files in os.walk(root):
        for f in files:
            if f != "rgstore.json":
                rel = os.path.relpath(os.path.join(dirpath, f), root)
                assert read(tmp_path / "again" / rel) == read(os.path.join(dirpath, f)), rel


def test_mixed_collection_classes_and_packed_records(G, tmp_path):
    col = G.load_fasta(mixed_fasta(tmp_path / "mixed.fa"), on_host=True)
    assert [r.metadata.alphabet.value for r in col] == MIXED_CLASSES
    store = G.RefgetStore.in_memory()
    store.add_sequence_collection(col)
    store.enable_encoding(on_host=True)
    assert store.storage_mode == G.StorageMode.Encoded
    for (name, _, seq), cls in zip(MIXED, MIXED_CLASSES):
        rec = store.get_sequence(G.digest_sequence(seq).metadata.sha512t24u)
        assert rec.encoded and rec.sequence == P.encode(seq, cls), name
        assert rec.decode() == P.round_trip(seq, cls).decode("latin-1")
        if len(seq) > 4:
            assert store.get_substring(rec.metadata.sha512t24u, 2, len(seq) - 1) == rec.decode()[2:len(seq) - 1]
    store.disable_encoding(on_host=True)
    assert store.storage_mode == G.StorageMode.Raw
    for (name, _, seq), cls in zip(MIXED, MIXED_CLASSES):
        rec = store.get_sequence(G.digest_sequence(seq).metadata.sha512t24u)
        assert not rec.encoded and rec.sequence == P.round_trip(seq, cls), name


def test_enable_persistence_writes_what_is_resident(G, tmp_path):
    store = G.RefgetStore.in_memory()
    meta, _ = store.add_sequence_collection_from_fasta(BASE_FA, on_host=True)
    store.enable_persistence(tmp_path / "p")
    assert store.is_persisting and store.cache_path == str(tmp_path / "p")
    assert all(not r.is_loaded for r in store.iter_sequences())
    manifest = json.loads(read(tmp_path / "p" / "rgstore.json"))
    assert manifest["mode"] == "Raw" and len(manifest["sequences_digest"]) == 64
    assert read(tmp_path / "p" / "sequences" / "iY" / "iYtREV555dUFKg2_agSJW6suquUyPpMw.seq") == b"TTGGGGAA"
    assert store.get_substring("iYtREV555dUFKg2_agSJW6suquUyPpMw", 2, 6) == "GGGG"
    assert G.substrings_many(store, meta.digest, ["chrX", "chr2"], [1, 0], [8, 4], on_host=True) == ["TGGGGAA", "GCGC"]
    store.disable_persistence()
    assert not store.is_persisting


def test_base_rgsi_without_ancillary_digests_round_trips(G, tmp_path):
    path = os.path.join(GOLDEN, "base.rgsi")
    col = G.read_rgsi_file(path)
    meta = col.metadata()
    assert (meta.digest, meta.n_sequences) == ("XZlrcEGi6mlopZ2uD8ObHkQB1d0oDwKk", 3)
    assert (meta.name_length_pairs_digest, meta.sorted_name_length_pairs_digest, meta.sorted_sequences_digest) == (None, None, None)
    assert [(r.metadata.name, r.metadata.length, r.metadata.description, r.is_loaded) for r in col] == [("chrX", 8, None, False), ("chr1", 4, None, False), ("chr2", 4, None, False)]
    col.write_collection_rgsi(tmp_path / "base.rgsi")
    assert read(tmp_path / "base.rgsi") == read(path)
    # the digests the file carries are those of the FASTA it was written from
    assert G.load_fasta(BASE_FA, on_host=True).digest == meta.digest


def test_index_rows_the_reader_skips_or_accepts(G, tmp_path):
    root = tmp_path / "s"
    shutil.copytree(FIXTURE, root)
    (root / "sequences.rgsi").write_bytes(read(root / "sequences.rgsi") + b"five\t3\tklingon\tAAAA\tbbbb\n\nshort\t3\n# a comment\nbad\tx\tdna2bit\tCCCC\tdddd\t\n")
    os.remove(root / "collections.rgci")  # without the index, collections/*.rgsi are read
    store = G.RefgetStore.open_local(root)
    assert sorted(m.name for m in store.list_sequences()) == ["chrF", "five"]
    five = store.get_sequence_metadata("AAAA")
    assert five.alphabet == G.AlphabetType.Unknown and five.description is None
    assert [m.digest for m in store.list_collections()] == [CHRF_COL] and store.is_collection_loaded(CHRF_COL)
    (root / "collections.rgci").write_bytes(b"#digest\n" + CHRF_COL.encode() + b"\t1\ta\tb\tc\nshort\t1\ta\tb\n")
    store = G.RefgetStore.open_local(root)
    (meta,) = store.list_collections()
    assert (meta.names_digest, meta.name_length_pairs_digest) == ("a", None) and not store.is_collection_loaded(CHRF_COL)


@pytest.mark.parametrize("bad", ["/x", "a/../b", "a\0b"])
@pytest.mark.parametrize("key", ["seqdata_path_template", "sequence_index", "collection_index"])
def test_manifest_paths_are_refused(G, tmp_path, bad, key):
    root = tmp_path / "s"
    shutil.copytree(FIXTURE, root)
    manifest = json.loads(read(root / "rgstore.json"))
    manifest[key] = bad
    (root / "rgstore.json").write_text(json.dumps(manifest))
    with pytest.raises(ValueError, match="not allowed"):
        G.RefgetStore.open_local(root)


def test_a_seq_file_of_the_wrong_size(G, tmp_path):
    root = tmp_path / "s"
    shutil.copytree(FIXTURE, root)
    seq = root / "sequences" / "71" / f"{CHRF}.seq"
    seq.write_bytes(b"\x9c" * 9)
    store = G.RefgetStore.open_local(root)
    with pytest.raises(ValueError, match=re.escape(f"{CHRF}.seq") + ".*9 bytes.*needs 10"):
        G.substrings_many(store, CHRF_COL, ["chrF"], [0], [4], on_host=True)
    with pytest.raises(ValueError, match="9 bytes"):
        store.load_sequence(CHRF)
    os.remove(seq)
    with pytest.raises(KeyError, match="stub only"):
        store.get_substring(CHRF, 0, 4)


def test_write_on_a_memory_store(G):
    with pytest.raises(IOError, match=re.escape("write() only works with disk-backed stores - use write_store_to_dir() instead")):
        G.RefgetStore.in_memory().write()


def test_abi_header_and_binding_name_the_same_k22_entries():
    import gtars_amd._lib as L

    host = open(os.path.join(HERE, "..", "include", "gtars_amd_host.h")).read()
    want = {"gtars_refget_bits", "gtars_refget_encode", "gtars_refget_decode", "gtars_refget_byte_range", "gtars_seqpack_from_seqcol",
            "gtars_seqpack_from_files", "gtars_seqpack_from_buffers", "gtars_seqpack_write_files", "gtars_seqpack_record", "gtars_seqpack_len",
            "gtars_seqpack_device", "gtars_seqpack_free", "gtars_seqpack_substrings", "gtars_seqpack_decode_records",
            "gtars_seqcol_from_seq_files", "gtars_seqcol_from_buffers", "gtars_seqcol_write_files"}
    declared = set(re.findall(r"\b(gtars_[a-z0-9_]+)\s*\(", host))
    assert want <= declared and want <= set(L.EXPORTED_HOST_SYMBOLS)
    assert "gtars_refget_packed_substrings_device" in L.EXPORTED_SYMBOLS
    assert "gtars_refget_packed_substrings_device" in open(os.path.join(HERE, "..", "include", "gtars_amd.h")).read()


def test_the_host_pack_equals_the_restatement_at_the_group_edges(G):
    """the host path of the pack (64 symbols per group, 2^20 per task) at the lengths the device test uses"""
    rng = random.Random(2209)
    for cls, letters in enumerate((b"ACGTacgt", b"ACGTNRYacgtnryX", b"ACGTURYSWKMBDHVNacgtn", b"ACDEFGHIKLMNPQRSTVWY*X-.acd", bytes(range(1, 256)))):
        seqs = [bytes(rng.choice(letters) for _ in range(n)) for n in (0, 1, 3, 4, 5, 7, 8, 9, 63, 64, 65, 16383, 16384, 16385)]
        pack = G._Pack.from_handle(G._Handle.from_buffers(seqs), [cls] * len(seqs), on_host=True)
        for i, seq in enumerate(seqs):
            assert pack.record(i) == (P.encode(seq, cls), len(seq), cls), (cls, len(seq))
        off, blob = pack.decode_records(on_host=True)
        assert [blob[off[i]:off[i + 1]] for i in range(len(seqs))] == [P.round_trip(q, cls) for q in seqs]


def test_pack_core_under_the_sanitizers(tmp_path):
    """tests/soak/refget_pack_check.cpp, built with AddressSanitizer + UBSan: refget_pack_core.h on every length from 0 to 300 at
    every width in exactly sized heap blocks; encode against a bit loop, then every [start, end) with end - start <= 17 decoded
    from the whole encoding, from exactly its byte range, and by the image reader, against a naive loop"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "refget_pack_check"
    src = os.path.join(HERE, "soak", "refget_pack_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o",
                            str(exe), src], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("the host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    assert "warning" not in build.stderr, build.stderr[-2000:]
    run = subprocess.run([str(exe), "300"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "ok: 1806 records" in run.stdout
