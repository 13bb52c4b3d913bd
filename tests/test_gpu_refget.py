"""K21 on the device (csrc/refget.hip) against the plain-Python restatement (tests/refget_ref.py): exact equality of digests,
MD5s, alphabet classes, collection digests, substrings and statuses.  One FASTA of 203 records is written by the test
(about 150 kB): every length at which the loads, MD5's and SHA-512's padding change their path, one record past the default
host tail, lengths in shuffled order, class-deciding bytes in the last position only."""
import os
import random

import numpy as np
import pytest

import refget_ref as R
from test_refget_cpu import check_collection

pytestmark = pytest.mark.gpu

EDGE_LENGTHS = [0, 1, 15, 16, 17, 55, 56, 63, 64, 65, 111, 112, 119, 120, 127, 128, 129, 255, 256, 257]
LONG = 70_001  # past the default GTARS_REFGET_HOST_LEN
N_RECORDS = 203


def _bases(rng, n, letters=b"ACGT"):
    return bytes(rng.choice(letters) for _ in range(n))


def _make_records():
    rng = random.Random(2121)
    recs = [(f"len{n}", _bases(rng, n, b"ACGTacgt" if n % 2 else b"ACGT")) for n in EDGE_LENGTHS]
    recs.append(("long", _bases(rng, LONG, b"ACGTacgtNn")))
    twin = _bases(rng, 77)
    recs += [("twin_a", twin), ("twin_b", twin)]                      # equal bytes under two names
    recs += [("again", _bases(rng, 40)), ("again", _bases(rng, 23, b"acgt"))]  # a repeated name
    recs += [(f"line{k}", _bases(rng, 16 * k)) for k in (1, 2, 3, 8)]  # end exactly on a 16-byte line of the image
    # the byte that decides the class in the LAST position only; the image's zero padding follows it
    recs += [("last_n", _bases(rng, 30) + b"n"), ("last_m", _bases(rng, 46) + b"m"), ("last_e", _bases(rng, 32) + b"e"),  # (33 = 16 * 2 + 1)
             ("last_7", _bases(rng, 15) + b"7"), ("last_star", _bases(rng, 64) + b"*"), ("last_at", _bases(rng, 16) + b"@")]
    recs.append(("acgt_only", b"ACGT" * 12))                          # 48 bytes, then padding: the zeros must not make it ASCII
    recs.append(("protein", b"MEFILPQX*-."))
    recs.append(("iupac", b"ACGTURYSWKMBDHVN"))
    recs.append(("text", b"Hello, World! 123"))
    while len(recs) < N_RECORDS:
        n = rng.choice([rng.randrange(0, 40), rng.randrange(40, 400), rng.randrange(400, 3000)])
        recs.append((f"r{len(recs)}", _bases(rng, n, rng.choice([b"ACGT", b"ACGTacgt", b"ACGTN", b"ACGTRYKM", b"acgtn"]))))
    head, tail = recs[:1], recs[1:]
    rng.shuffle(tail)  # lengths in shuffled order: the length permutation must put the results back
    return head + tail


RECORDS = _make_records()
assert len(RECORDS) == N_RECORDS and N_RECORDS % 64


def _fasta_text(records, width=60):
    out = []
    for k, (name, seq) in enumerate(records):
        out.append(b">" + name.encode() + (b" record %d\n" % k if k % 3 == 0 else b"\n"))
        out += [seq[at:at + width] + b"\n" for at in range(0, len(seq), width)]
    return b"".join(out)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    import gtars_amd
    import gtars_amd.refget as G

    assert gtars_amd.device_count() > 0
    path = tmp_path_factory.mktemp("refget") / "many.fa"
    text = _fasta_text(RECORDS)
    path.write_bytes(text)
    want = R.walk_fasta(text)
    assert [w["length"] for w in want] == [len(s) for _, s in RECORDS]
    return G, str(path), want


def test_digest_fasta_on_the_device(world):
    G, path, want = world
    check_collection(G.digest_fasta(path), want, False)
    check_collection(G.load_fasta(path), want, True)
    by = {w["name"]: w for w in want}
    assert [R.ALPHABET_NAMES[by[k]["alphabet"]] for k in ("last_n", "last_m", "last_e", "last_7", "acgt_only", "len0")] == [
        "dna3bit", "dnaio", "protein", "ASCII", "dna2bit", "dna2bit"]
    assert by["twin_a"]["sha512t24u"] == by["twin_b"]["sha512t24u"]


def _digests_again(G, col, want):
    text, md5, cls = G.digest_records(col)
    assert (text, md5, cls.tolist()) == ([w["sha512t24u"] for w in want], [w["md5"] for w in want], [w["alphabet"] for w in want])


def test_host_tail_gives_the_same_results(world, monkeypatch):
    """GTARS_REFGET_HOST_LEN 0 (every record that is not empty is hashed by the host threads), 8, the default and 2^20 (every
    record on the device): digest_fasta, which uploads the short records only, and the digests from the full image, whose long
    rows come back as a list"""
    G, path, want = world
    from gtars_amd._lib import lib

    assert "GTARS_REFGET_HOST_LEN" not in os.environ
    for host_len in (None, "0", "8", str(1 << 20)):
        if host_len is not None:
            monkeypatch.setenv("GTARS_REFGET_HOST_LEN", host_len)
        assert lib.gtars_refget_host_len() == (65536 if host_len is None else int(host_len))
        check_collection(G.digest_fasta(path), want, False)
        col = G.load_fasta(path)
        check_collection(col, want, True)
        _digests_again(G, col, want)


def test_device_entries_on_a_stream_and_a_forged_device(world):
    import torch

    G, path, want = world
    from gtars_amd._lib import lib

    col = G.load_fasta(path)
    n = len(col)
    dev = torch.device("cuda", torch.cuda.current_device())
    digests = torch.full((32 * n,), 1, dtype=torch.uint8, device=dev)
    md5 = torch.full((16 * n,), 1, dtype=torch.uint8, device=dev)
    cls = torch.full((n,), 77, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        G.digests_device(col, digests.data_ptr(), md5.data_ptr(), cls.data_ptr(), side.cuda_stream)
    raw, m = digests.cpu().numpy().tobytes(), md5.cpu().numpy().tobytes()
    assert [raw[32 * i:32 * i + 32].decode() for i in range(n)] == [w["sha512t24u"] for w in want]
    assert [m[16 * i:16 * i + 16].hex() for i in range(n)] == [w["md5"] for w in want]
    assert cls.cpu().tolist() == [w["alphabet"] for w in want]
    # one column alone
    cls.fill_(77)
    G.digests_device(col, 0, 0, cls.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert cls.cpu().tolist() == [w["alphabet"] for w in want]
    with pytest.raises(ValueError, match="8-byte aligned"):
        G.digests_device(col, digests.data_ptr() + 4, 0, 0)
    # substrings of device columns
    rows = [(i, 0, min(w["length"], 10)) for i, w in enumerate(want)][:64] + [(0xFFFFFFFF, 0, 1), (3, 5, 2), (n, 0, 0)]
    k = len(rows)
    put = lambda values, np_dtype, as_dtype: torch.from_numpy(np.array(values, dtype=np_dtype).view(as_dtype).copy()).to(dev)  # noqa: E731
    seq = put([r[0] for r in rows], np.uint32, np.int32)
    start, end = put([r[1] for r in rows], np.uint64, np.int64), put([r[2] for r in rows], np.uint64, np.int64)
    status = torch.full((k,), 77, dtype=torch.uint8, device=dev)
    offsets = torch.zeros(k + 1, dtype=torch.int64, device=dev)
    expect = [R.substring(want[i]["sequence"] if i < n else None, s, e) for i, s, e in rows]
    total = sum(len(b) for _, b in expect)
    out = torch.full((total + 8,), 1, dtype=torch.uint8, device=dev)
    with torch.cuda.stream(side):
        got = G.substrings_device(col, seq.data_ptr(), start.data_ptr(), end.data_ptr(), k, status.data_ptr(), offsets.data_ptr(), out.data_ptr(),
                                  total, side.cuda_stream)
    assert got == total and status.cpu().tolist() == [st for st, _ in expect]
    assert offsets.cpu().tolist() == np.concatenate([[0], np.cumsum([len(b) for _, b in expect])]).tolist()
    assert out.cpu().numpy().tobytes() == b"".join(b for _, b in expect) + b"\x01" * 8  # (nothing behind the total is written)
    from gtars_amd._lib import CapacityError

    with pytest.raises(CapacityError) as err:
        G.substrings_device(col, seq.data_ptr(), start.data_ptr(), end.data_ptr(), k, status.data_ptr(), offsets.data_ptr(), out.data_ptr(), total - 1)
    assert err.value.needed == total
    assert G.substrings_device(col, 0, 0, 0, 0, 0, 0, 0, 0) == 0  # n == 0 touches nothing
    # the calls run on the image's device or are refused
    cur = torch.cuda.current_device()
    forged = cur + 1
    asm = lib.gtars_seqcol_assembly(col._handle.h)
    assert lib.gtars_debug_set_assembly_device(asm, forged) == cur
    try:
        cls.fill_(77)
        status.fill_(77)
        with pytest.raises(ValueError, match=f"handle lives on device {forged}, current device is {cur}"):
            G.digests_device(col, 0, 0, cls.data_ptr(), torch.cuda.current_stream().cuda_stream)
        with pytest.raises(ValueError, match=f"handle lives on device {forged}, current device is {cur}"):
            G.substrings_device(col, seq.data_ptr(), start.data_ptr(), end.data_ptr(), k, status.data_ptr(), offsets.data_ptr(), out.data_ptr(), total)
        assert cls.cpu().tolist() == [77] * n and status.cpu().tolist() == [77] * k
    finally:
        assert lib.gtars_debug_set_assembly_device(asm, cur) == forged
    G.digests_device(col, 0, 0, cls.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert cls.cpu().tolist() == [w["alphabet"] for w in want]


def _check_regions(G, store, digest, want, rows):
    expect = R.region_substrings(want, *zip(*rows))
    for on_host in (False, True):
        got, status = G.substrings_many(store, digest, [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], on_host=on_host,
                                        with_status=True)
        assert status.tolist() == [st for st, _ in expect], on_host
        assert got == [b.decode() if st == 0 else None for st, b in expect], on_host
    return expect


def test_substrings(world, tmp_path):
    G, path, want = world
    store = G.RefgetStore.in_memory()
    meta, _ = store.add_sequence_collection_from_fasta(path)
    by = {w["name"]: w for w in want}  # (a repeated name: its last record)
    rows = []
    # rows of 1, 2, ... bytes make the packed output of the next row start at every offset 0 .. 7 of the fill's eight bytes,
    # with empty rows and failing rows between real ones
    for k in range(1, 20):
        rows += [("len257", k, 2 * k), ("len64", 5, 5), ("nope", 0, 3), ("len17", 9, 3)]
    # a row that ends at a sequence's last base (a neighbour lies behind it in the image), whole sequences, the first base
    for name in ("line1", "line2", "len16", "len17", "len255", "twin_b", "acgt_only", "last_e", "again"):
        n = by[name]["length"]
        rows += [(name, 0, n), (name, n - 1, n), (name, 0, 1), (name, n, n), (name, n, n + 1), (name, 0, n + 1), (name, n + 7, n + 7)]
    rows += [("long", 69_990, LONG), ("long", 0, 40_000), ("long", 123, 124), ("len0", 0, 0), ("len0", 0, 1), ("len1", 0, 1)]
    rows += [("len129", 3, 100), ("len65", 1, 65)]  # (lower-case image bytes come back upper-case)
    expect = _check_regions(G, store, meta.digest, want, rows)
    assert {st for st, _ in expect} == {0, 1, 2}
    raw = dict(RECORDS)["len129"]
    assert raw != raw.upper() and expect[-2] == (0, raw.upper()[3:100])
    again = [s for name, s in RECORDS if name == "again"]
    assert len(again) == 2 and by["again"]["sequence"] == again[-1].upper() != again[0].upper()  # the name's last record
    # the region calls, byte for byte; a failing region raises
    good = [r for r, (st, _) in zip(rows, expect) if st == 0]
    bed = tmp_path / "good.bed"
    bed.write_text("".join(f"{c}\t{s}\t{e}\n" for c, s, e in good))
    got = store.substrings_from_regions(meta.digest, bed)
    assert [(g.chrom_name, g.start, g.end, g.sequence) for g in got] == [(c, s, e, b.decode()) for (c, s, e), (st, b) in zip(rows, expect) if st == 0]
    out = tmp_path / "regions.fa"
    store.export_fasta_from_regions(meta.digest, bed, out)
    assert out.read_bytes() == R.export_fasta_from_regions(want, good)
    bed.write_text("len64\t0\t4\nlen64\t60\t65\n")
    sha = by["len64"]["sha512t24u"]
    with pytest.raises(ValueError, match=f"^Line 3: failed to get substring for digest '{sha}' from 60 to 65: Invalid substring range: start=60, "
                                         "end=65, sequence length=64$"):
        store.export_fasta_from_regions(meta.digest, bed, out)
    # a collection that came from no file gets its image at the first region call
    recs = [G.digest_sequence(b"acgtacgtacgtacgtAC", "x"), G.digest_sequence(b"", "empty"), G.digest_sequence(b"GGnnTT", "y")]
    made = G.SequenceCollection.from_records(recs)
    store.add_sequence_collection(made)
    assert G.substrings_many(store, made.digest, ["y", "x", "empty", "x"], [2, 15, 0, 0], [6, 18, 0, 19], with_status=True)[0] == ["NNTT", "TAC", "", None]


def test_random_collections(tmp_path):
    """about 40 seeded cases: random records (lengths around the block edges, mixed alphabets, blank lines, CRLF, repeated
    names) and random regions against the restatement, through the file calls and the store"""
    import gtars_amd.refget as G

    rng = random.Random(int(os.environ.get("GTARS_SOAK_SEED", "2121")))
    letters = [b"ACGT", b"ACGTacgt", b"ACGTNnRY", b"ACGTUSWKMBDHV", b"ACDEFGHIKLMNPQRSTVWY*", b"acgt-.x", b"ACGT 7z"]
    for case in range(40):
        names = [f"s{k}" for k in range(rng.randrange(1, 9))]
        eol = rng.choice([b"\n", b"\r\n"])
        parts = [b"# preamble" + eol] if rng.random() < 0.3 else []
        for k in range(rng.randrange(1, 12)):
            n = rng.choice([0, 1, rng.randrange(2, 20), rng.randrange(48, 70), rng.randrange(100, 140), rng.randrange(140, 2000)])
            seq = _bases(rng, n, rng.choice(letters)).strip(b" ")
            width = rng.choice([7, 16, 60, 4000])
            parts.append(b">" + rng.choice(names).encode() + (b" about " + str(k).encode() if rng.random() < 0.5 else b"") + eol)
            for at in range(0, len(seq), width):
                line = seq[at:at + width]
                parts.append((line if line.strip(R.WS) else b"A" + line) + eol)
                if rng.random() < 0.1:
                    parts.append(eol)
        text = b"".join(parts)
        if rng.random() < 0.3 and text.endswith(eol):
            text = text[:-len(eol)]
        path = tmp_path / f"case{case}.fa"
        path.write_bytes(text)
        want = R.walk_fasta(text)
        check_collection(G.digest_fasta(path), want, False)
        store = G.RefgetStore.in_memory()
        meta, was_new = store.add_sequence_collection_from_fasta(path)
        assert was_new and meta.digest == R.digests_of_records(want)["top"]
        rows = []
        for _ in range(30):
            name = rng.choice(names + ["missing"])
            n = R.last_by_name(want)[name]["length"] if name in R.last_by_name(want) else 10
            s = rng.randrange(0, n + 3)
            rows.append((name, s, rng.choice([s, s + 1, rng.randrange(0, n + 3), n, min(n, s + rng.randrange(0, 50))])))
        _check_regions(G, store, meta.digest, want, rows)
