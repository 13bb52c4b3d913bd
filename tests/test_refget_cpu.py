"""K21 on the host (gtars_amd.refget with on_host=True, the scalar calls, compute_fai) against the known answers of the
reference's tests, the committed fixtures (tests/golden/fasta) and the plain-Python restatement (tests/refget_ref.py)."""
import gzip
import hashlib
import importlib
import json
import os
import random
import shutil
import subprocess

import pytest

import refget_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
FASTA = os.path.join(HERE, "golden", "fasta")
CHRX = "iYtREV555dUFKg2_agSJW6suquUyPpMw"
CHRX_MD5 = "5f63cfaa3ef61f88c9635fb9d18ec945"


@pytest.fixture(scope="module")
def G():
    import gtars_amd.refget as G

    return G


def check_collection(col, want, loaded):
    """a SequenceCollection against the restatement's records, digests included"""
    assert len(col) == len(want)
    for got, w in zip(col, want):
        m = got.metadata
        assert (m.name, m.description, m.length, m.sha512t24u, m.md5, str(m.alphabet)) == (
            w["name"], w["description"], w["length"], w["sha512t24u"], w["md5"], R.ALPHABET_NAMES[w["alphabet"]]), w["name"]
        assert (None if m.fai is None else (m.fai.offset, m.fai.line_bases, m.fai.line_bytes)) == w["fai"], w["name"]
        assert got.sequence == (w["sequence"] if loaded else None) and got.is_loaded == loaded
    d = R.digests_of_records(want)
    meta = col.metadata()
    assert col.digest == meta.digest == d["top"]
    assert (col.lvl1.names_digest, col.lvl1.sequences_digest, col.lvl1.lengths_digest) == (d["names"], d["sequences"], d["lengths"])
    assert (meta.name_length_pairs_digest, meta.sorted_name_length_pairs_digest, meta.sorted_sequences_digest) == (
        d["name_length_pairs"], d["sorted_name_length_pairs"], d["sorted_sequences"])


def test_module_location(G):
    import gtars_amd

    assert importlib.import_module("gtars_amd.refget") is G
    with pytest.raises(ModuleNotFoundError):
        importlib.import_module("gtars.refget")
    for name in ("AlphabetType", "FaiMetadata", "FaiRecord", "SequenceMetadata", "SequenceRecord", "SeqColDigestLvl1", "SequenceCollectionMetadata",
                 "SequenceCollection", "RetrievedSequence", "RefgetStore", "sha512t24u_digest", "md5_digest", "digest_sequence", "digest_fasta",
                 "load_fasta", "compute_fai", "substrings_many", "digests_device", "substrings_device"):
        assert hasattr(G, name), name
    assert gtars_amd.__version__


def test_known_answers(G):
    assert G.sha512t24u_digest("ACGT") == G.sha512t24u_digest(b"ACGT") == "aKF498dAxcJAqme6QYQ7EZ07-fiw8Kw2"
    assert G.md5_digest("ACGT") == G.md5_digest(b"ACGT") == "f1f8f4bf413b16ad135722aa4591043e"
    assert G.sha512t24u_digest("") == "z4PhNX7vuL3xVChQ1m2AB9Yg5AULVxXc"
    assert G.md5_digest(b"") == "d41d8cd98f00b204e9800998ecf8427e"
    assert G.sha512t24u_digest("hello world") == G.sha512t24u_digest(b"hello world") == "MJ7MSJwS1utMxA9QyQLytNDtd-5RGnx6"
    assert G.md5_digest("hello world") == "5eb63bbbe01eeed093cb22bb8f5acdc3"
    assert G.sha512t24u_digest("acgt") != G.sha512t24u_digest("ACGT")  # (no upper-casing)
    for bad in (None, 7, ["ACGT"]):
        with pytest.raises(TypeError):
            G.sha512t24u_digest(bad)
        with pytest.raises(TypeError):
            G.md5_digest(bad)
    rng = random.Random(21)
    for n in list(range(0, 140)) + [255, 256, 257, 1000]:
        data = bytes(rng.randrange(256) for _ in range(n))
        assert G.md5_digest(data) == hashlib.md5(data).hexdigest(), n
        assert G.sha512t24u_digest(data) == R.sha512t24u(data), n


def test_digest_sequence(G):
    r = G.digest_sequence(b"acgtn", name="s", description="d e")
    assert (r.metadata.name, r.metadata.description, r.metadata.length, r.sequence, r.is_loaded, r.decode()) == ("s", "d e", 5, b"ACGTN", True, "ACGTN")
    assert (r.metadata.sha512t24u, r.metadata.md5, str(r.metadata.alphabet)) == (R.sha512t24u(b"ACGTN"), R.md5(b"ACGTN"), "dna3bit")
    assert r.metadata.alphabet == G.AlphabetType.Dna3bit
    assert G.digest_sequence("ACGT").metadata.name == ""
    assert [str(G.AlphabetType(k)) for k in range(6)] == ["dna2bit", "dna3bit", "dnaio", "protein", "ASCII", "Unknown"]


def test_base_fa(G):
    col = G.digest_fasta(os.path.join(FASTA, "base.fa"), on_host=True)
    assert len(col.sequences) == 3 and isinstance(col.sequences, list) and col.file_path.endswith("base.fa")
    m = col.sequences[0].metadata
    assert (m.name, m.length, m.sha512t24u, m.md5) == ("chrX", 8, CHRX, CHRX_MD5)
    assert col.lvl1.sequences_digest == "0uDQVLuHaOZi1u76LjV__yrVUIz9Bwhr"
    assert col.lvl1.names_digest == "Fw1r9eRxfOZD98KKrhlYQNEdSRHoVxAG"
    assert col.lvl1.lengths_digest == "cGRMZIb3AVgkcAfNv39RN7hnT5Chk7RX"
    assert str(col).startswith("SequenceCollection with 3 sequences")
    assert str(m).startswith("SequenceMetadata for sequence")
    assert str(col.lvl1).startswith("SeqColDigestLvl1:")
    for rec in col:
        assert rec.sequence is None and rec.decode() is None and not rec.is_loaded
    assert col[-1].metadata.name == "chr2" and [r.metadata.name for r in col] == ["chrX", "chr1", "chr2"]
    with pytest.raises(Exception):
        G.digest_fasta("nonexistent.fa", on_host=True)
    # gzip input: the same records, no FAI
    gz = G.digest_fasta(os.path.join(FASTA, "base.fa.gz"), on_host=True)
    assert gz.digest == col.digest
    assert [(r.metadata.name, r.metadata.sha512t24u, r.metadata.md5, r.metadata.length) for r in gz] == [
        (r.metadata.name, r.metadata.sha512t24u, r.metadata.md5, r.metadata.length) for r in col]
    assert all(r.metadata.fai is None for r in gz) and all(r.metadata.fai is not None for r in col)
    assert all(r.fai is None for r in G.compute_fai(os.path.join(FASTA, "base.fa.gz")))


def test_every_entry_of_the_digest_fixture(G):
    ref = json.load(open(os.path.join(FASTA, "test_fasta_digests.json")))
    assert len(ref) == 6
    for name, want in ref.items():
        path = os.path.join(FASTA, name)
        col = G.load_fasta(path, on_host=True)
        check_collection(col, R.walk_fasta(open(path, "rb").read()), True)
        assert col.digest == want["top_level_digest"], name
        store = G.RefgetStore.in_memory()
        meta, was_new = store.add_sequence_collection_from_fasta(path, on_host=True)
        assert was_new and meta.digest == want["top_level_digest"]
        assert meta.sorted_name_length_pairs_digest == want["sorted_name_length_pairs_digest"]
        assert store.get_collection_level1(col.digest) == want["level1"], name
        assert store.get_collection_level2(col.digest) == want["level2"], name


def test_fai_fixtures(G):
    for stem in ("base", "crlf_endings", "unwrapped", "wrapped_20", "wrapped_40"):
        got = G.compute_fai(os.path.join(FASTA, stem + ".fa"))
        lines = ["\t".join(map(str, (r.name, r.length, r.fai.offset, r.fai.line_bases, r.fai.line_bytes))) for r in got]
        assert lines == open(os.path.join(FASTA, stem + ".fa.fai")).read().splitlines(), stem
        want = R.walk_fasta(open(os.path.join(FASTA, stem + ".fa"), "rb").read())
        assert [(r.name, r.length, (r.fai.offset, r.fai.line_bases, r.fai.line_bytes)) for r in got] == [(w["name"], w["length"], w["fai"]) for w in want]


def test_alphabet(G):
    cases = {b"ACGT": "dna2bit", b"ACGTNRY": "dna3bit", b"ACGTRYMK": "dnaio", b"EFILPQ": "protein", b"Hello, World!": "ASCII",
             b"ACTGEG": "protein", b"ACTGM": "dnaio", b"ACGTSKWV": "dnaio", b"ACGTE": "protein", b"ACGT*": "protein", b"ACGT-": "protein",
             b"actgEFIL": "protein", b"ACGT123": "ASCII", b"": "dna2bit"}
    for data, want in cases.items():
        assert str(G.guess_alphabet(data)) == want == R.ALPHABET_NAMES[R.guess_alphabet(data)], data
        assert str(G.digest_sequence(data).metadata.alphabet) == want
    assert G.alphabet_class_table().tobytes() == R.CLASS_TABLE == R.CLASS_TABLE_STATED
    for b in range(256):
        assert int(G.guess_alphabet(bytes([b]))) == R.CLASS_TABLE[b], b


WALK_CASES = {
    "no trailing newline": b">a\nACGT\n>b x\nGG",
    "blank lines": b">a\n\nAC\n\n  \nGT\n\n>b\n\nT\n",
    "text before the first header": b"junk\nmore junk\n>a desc here \nACGT\n",
    "an empty record": b">a\n>b\nAC\n>c\n",
    "a repeated name": b">a\nAC\n>b\nGG\n>a\nTTT\n",
    "lower case": b">a\nacgtn\n>b\nAcGtRyKm\n",
    "inner spaces": b">a\nAC GT \n  TT\n>b\t tabbed  desc \t\nAC\tGT\n",
    "crlf": b">a d\r\nACGT\r\nAC\r\n>b\r\n\r\nGG\r\n",
    "header only": b">",
    "empty": b"",
    "not at line start": b">a\n >b\nAC\n",
    "protein and text": b">p\nMEFILPQ*\n>t\nhello world 7\n",
}


@pytest.mark.parametrize("case", sorted(WALK_CASES))
def test_record_walk(G, tmp_path, case):
    text = WALK_CASES[case]
    path = tmp_path / "x.fa"
    path.write_bytes(text)
    want = R.walk_fasta(text)
    check_collection(G.load_fasta(path, on_host=True), want, True)
    check_collection(G.digest_fasta(path, on_host=True), want, False)
    assert [(r.name, r.length, None if r.fai is None else (r.fai.offset, r.fai.line_bases, r.fai.line_bytes)) for r in G.compute_fai(path)] == [
        (w["name"], w["length"], w["fai"]) for w in want]
    gz = tmp_path / "x.fa.gz"
    gz.write_bytes(gzip.compress(text))
    check_collection(G.load_fasta(gz, on_host=True), R.walk_fasta(text, gzip_input=True), True)


def test_write_fasta(G, tmp_path):
    col = G.load_fasta(os.path.join(FASTA, "wrapped_20.fa"), on_host=True)
    out = tmp_path / "out.fa"
    col.write_fasta(out, line_width=20)
    again = G.load_fasta(out, on_host=True)
    assert again.digest == col.digest and [r.sequence for r in again] == [r.sequence for r in col]
    col.write_fasta(out)
    assert max(len(line) for line in out.read_bytes().splitlines()) <= 70
    with pytest.raises(IOError):
        G.digest_fasta(os.path.join(FASTA, "base.fa"), on_host=True).write_fasta(out)


def test_store(G, tmp_path):
    base = os.path.join(FASTA, "base.fa")
    store = G.RefgetStore.in_memory()
    assert repr(store).startswith("RefgetStore") and "n_sequences=0" in repr(store) and "memory-only" in repr(store)
    meta, was_new = store.add_sequence_collection_from_fasta(base, on_host=True)
    assert was_new and store.add_sequence_collection_from_fasta(base, on_host=True) == (meta, False)
    for key in (CHRX, CHRX_MD5):
        seq = store.get_sequence(key)
        assert seq.metadata.length == 8 and seq.sequence == b"TTGGGGAA"
    assert len(store.get_substring(CHRX, 0, 4)) == 4 and store.get_substring(CHRX_MD5, 2, 8) == "GGGGAA"
    assert len(store) == 3 and "n_sequences=3" in repr(store)
    with pytest.raises(KeyError):
        store.get_sequence("not_a_sequence")
    col = G.digest_fasta(base, on_host=True)
    by_name = store.get_sequence_by_name(col.digest, col.sequences[0].metadata.name)
    assert (by_name.metadata.length, by_name.metadata.sha512t24u) == (8, CHRX)
    assert [m.digest for m in store.list_collections()] == [col.digest] and store.get_collection_metadata(col.digest).n_sequences == 3
    assert [r.metadata.name for r in store.get_collection(col.digest)] == ["chrX", "chr1", "chr2"]
    assert [c.digest for c in store.iter_collections()] == [col.digest]
    assert sorted(m.sha512t24u for m in store.list_sequences()) == sorted(r.metadata.sha512t24u for r in col)
    assert store.get_sequence_metadata(CHRX_MD5).name == "chrX" and store.get_sequence_metadata("nope") is None
    assert len(store.iter_sequences()) == 3
    # several files: a list, a glob (sorted), a file of file names
    other = os.path.join(FASTA, "different_order.fa")
    store = G.RefgetStore.in_memory()
    results = store.add_sequence_collections_from_fastas([base, other], jobs=1, on_host=True)
    assert len(results) == 2 and all(isinstance(new, bool) and hasattr(m, "digest") for m, new in results)
    assert len(G.RefgetStore.in_memory().add_sequence_collections_from_fastas(os.path.join(FASTA, "*.fa.gz"), on_host=True)) >= 1
    globbed = G.RefgetStore.in_memory().add_sequence_collections_from_fastas(os.path.join(FASTA, "wrapped_*.fa"), on_host=True)
    assert [m.digest for m, _ in globbed] == [G.digest_fasta(os.path.join(FASTA, f), on_host=True).digest for f in ("wrapped_20.fa", "wrapped_40.fa")]
    fofn = tmp_path / "list.txt"
    fofn.write_text(f"# a comment\n\n{base}\n  {other}  \n")
    assert len(G.RefgetStore.in_memory().add_sequence_collections_from_fastas([], file_list=fofn, on_host=True)) == 2
    with pytest.raises(ValueError):
        G.RefgetStore.in_memory().add_sequence_collections_from_fastas(os.path.join(FASTA, "does_not_exist_*.fa"))
    with pytest.raises(Exception):
        store.add_sequence_collection_from_fasta("nonexistent.fa", on_host=True)
    # records that came from no file
    recs = [G.digest_sequence(b"acgt", "one"), G.digest_sequence(b"GGNN", "two", "second")]
    made = G.SequenceCollection.from_records(recs)
    want = [dict(w, fai=None) for w in R.walk_fasta(b">one\nacgt\n>two second\nGGNN\n")]
    check_collection(made, want, True)
    meta, was_new = store.add_sequence_collection(made)
    assert was_new and store.get_substring(recs[1].metadata.sha512t24u, 1, 3) == "GN"
    assert G.substrings_many(store, made.digest, ["two", "one", "zzz"], [0, 1, 0], [4, 2, 1], on_host=True, with_status=True)[0] == ["GGNN", "C", None]
    store.add_sequence(G.digest_sequence(b"TTTT", "lone"))
    assert store.get_sequence(R.sha512t24u(b"TTTT")).metadata.name == "lone"


def test_regions_and_export(G, tmp_path):
    fa = tmp_path / "test.fa"
    fa.write_text(">chr1\nATGCATGCATGC\n>chr2\nGGGGAAAA\n")
    store = G.RefgetStore.in_memory()
    store.add_sequence_collection_from_fasta(fa, on_host=True)
    digest = G.digest_fasta(fa, on_host=True).digest
    bed = tmp_path / "test.bed"
    bed.write_text("chr1\t0\t5\nchr1\t8\t12\nchr2\t0\t4")
    out = tmp_path / "sub" / "output.fa"
    store.export_fasta_from_regions(digest, bed, out, on_host=True)
    assert out.read_text() == ">chr1:0-5\nATGCA\n>chr1:8-12\nATGC\n>chr2:0-4\nGGGG\n"
    store.export_fasta_from_regions(digest, bed, tmp_path / "output.fa.gz", on_host=True)
    assert gzip.open(tmp_path / "output.fa.gz").read() == out.read_bytes()
    got = store.substrings_from_regions(digest, bed, on_host=True)
    assert got == [G.RetrievedSequence("ATGCA", "chr1", 0, 5), G.RetrievedSequence("ATGC", "chr1", 8, 12), G.RetrievedSequence("GGGG", "chr2", 0, 4)]
    assert (got[0].sequence, got[0].chrom_name, got[0].start, got[0].end) == ("ATGCA", "chr1", 0, 5)
    # a failing region raises, with the reference's text
    bed.write_text("chr1\t0\t5\nchr9\t0\t1\n")
    with pytest.raises(ValueError, match=f"^Line 3: sequence 'chr9' not found in collection '{digest}': Sequence 'chr9' not found in collection$"):
        store.substrings_from_regions(digest, bed, on_host=True)
    bed.write_text("chr2\t4\t9\n")
    sha = R.sha512t24u(b"GGGGAAAA")
    with pytest.raises(ValueError, match=f"^Line 2: failed to get substring for digest '{sha}' from 4 to 9: Invalid substring range: start=4, "
                                         "end=9, sequence length=8$"):
        store.export_fasta_from_regions(digest, bed, out, on_host=True)
    bed.write_text("chr2\tx\t9\n")
    with pytest.raises(ValueError, match="^Line 2 has invalid start or end coordinates: start=-1, end=9$"):
        store.substrings_from_regions(digest, bed, on_host=True)
    store.export_fasta(digest, tmp_path / "all.fa", line_width=5)
    assert (tmp_path / "all.fa").read_text() == ">chr1\nATGCA\nTGCAT\nGC\n>chr2\nGGGGA\nAAA\n"
    store.export_fasta(digest, tmp_path / "one.fa", ["chr2"])
    assert (tmp_path / "one.fa").read_text() == ">chr2\nGGGGAAAA\n"


def test_substring_rule(G, tmp_path):
    fa = tmp_path / "r.fa"
    fa.write_bytes(b">a\nacgtACGT\n>b\nGG\n>a\nTTTnn\n>e\n")
    recs = R.walk_fasta(fa.read_bytes())
    store = G.RefgetStore.in_memory()
    store.add_sequence_collection_from_fasta(fa, on_host=True)
    digest = G.digest_fasta(fa, on_host=True).digest
    sha = recs[0]["sha512t24u"]
    # start == end: inside, at the end, past the end; inverted and over-long ranges
    assert store.get_substring(sha, 3, 3) == store.get_substring(sha, 8, 8) == store.get_substring(sha, 100, 100) == ""
    assert store.get_substring(sha, 0, 8) == "ACGTACGT" and store.get_substring(sha, 7, 8) == "T"
    for s, e in ((10, 5), (0, 100), (8, 9), (5, 4), (9, 8)):
        with pytest.raises(KeyError, match="Invalid substring range"):
            store.get_substring(sha, s, e)
    with pytest.raises(KeyError, match="Sequence not found"):
        store.get_substring("nope", 0, 0)
    rows = [("a", 0, 5), ("a", 3, 3), ("a", 5, 5), ("a", 9, 9), ("a", 4, 2), ("a", 0, 6), ("b", 0, 2), ("b", 2, 2), ("b", 2, 3), ("zz", 0, 0),
            ("zz", 0, 1), ("e", 0, 0), ("e", 0, 1), ("a", 2, 5)]
    want = R.region_substrings(recs, *zip(*rows))
    got, status = G.substrings_many(store, digest, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], on_host=True, with_status=True)
    assert status.tolist() == [st for st, _ in want]
    assert got == [seq.decode() if st == 0 else None for st, seq in want]
    assert got[0] == "TTTNN" and got[-1] == "TNN"  # (the repeated name's LAST record, upper-cased)
    assert store.get_sequence_by_name(digest, "a").sequence == b"TTTNN"
    assert list(store._names[digest]) == ["a", "b", "e"]


def test_host_code_under_the_sanitizers(tmp_path):
    """tests/soak/refget_host_check.cpp, built with AddressSanitizer + UBSan: md5.h and the combined loop of refget_core.h on
    every message length from 0 to 300 bytes in exactly sized heap blocks against hashlib's answers, the record walk on every
    truncation of a small FASTA against the restatement's record counts and lengths."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "refget_host_check"
    src = os.path.join(HERE, "soak", "refget_host_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o",
                            str(exe), src], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("the host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    rng = random.Random(2100)
    alphabet = b"ACGTacgtNnRYkmEFIL*-.x7 \xc3\xa9"
    lines = []
    for n in range(301):
        data = bytes(rng.choice(alphabet) for _ in range(n))
        up = R.ascii_upper(data)
        lines.append(f"{data.hex() or '-'} {R.sha512t24u(up)} {R.md5(up)} {R.guess_alphabet(up)} {R.md5(data)}")
    (tmp_path / "messages.txt").write_text("\n".join(lines) + "\n")
    fasta = b"junk\n>a first one \nACgt\nAC\n\n>b\n>c\tx\r\nGGn n\r\nT\r\n>a\nEFIL*"
    walks = []
    for cut in range(len(fasta) + 1):
        recs = R.walk_fasta(fasta[:cut])
        walks.append(" ".join([str(cut), str(len(recs))] + [f"{r['length']}:{r['sha512t24u']}:{'-' if r['fai'] is None else r['fai'][0]}" for r in recs]))
    (tmp_path / "fasta.bin").write_bytes(fasta)
    (tmp_path / "walks.txt").write_text("\n".join(walks) + "\n")
    run = subprocess.run([str(exe), str(tmp_path / "messages.txt"), str(tmp_path / "fasta.bin"), str(tmp_path / "walks.txt")],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "ok" in run.stdout


@pytest.mark.skipif(__import__("gtars_amd").device_count() > 0, reason="needs a box WITHOUT a GPU")
def test_no_device_is_a_loud_error(G, tmp_path):
    import gtars_amd

    base = os.path.join(FASTA, "base.fa")
    with pytest.raises(gtars_amd.NoDeviceError):
        G.digest_fasta(base)
    with pytest.raises(gtars_amd.NoDeviceError):
        G.load_fasta(base)
    store = G.RefgetStore.in_memory()
    store.add_sequence_collection_from_fasta(base, on_host=True)
    bed = tmp_path / "r.bed"
    bed.write_text("chrX\t0\t4\n")
    with pytest.raises(gtars_amd.NoDeviceError):
        store.substrings_from_regions(G.digest_fasta(base, on_host=True).digest, bed)
