"""K17 without a device: the library's BGZF reader (block table, inflate, header, record offsets) against the pure Python reader
tests/bam_ref.py on the two fixtures and on written files with chosen block cuts; every corruption the reader refuses; the
restatement of bamqc.rs on the fixtures; the TSV row; the CLI's command lines."""
import io
import os
import struct
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_ref as R  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bam")
CHR22 = os.path.join(GOLDEN, "test_chr22_small.bam")
DUMMY = os.path.join(GOLDEN, "dummy.bam")


def bam():
    from gtars_amd import bam as B

    return B


def assert_reader_equal(path):
    ref = R.read_bam(path)
    with bam().BamFile(path) as b:
        t = b.block_table()
        got = [tuple(int(t[k][i]) for k in ("coff", "csize", "isize", "crc", "uoff")) for i in range(b.n_blocks)]
        assert got == ref["blocks"]
        assert b.n_bytes == len(ref["stream"])
        for threads in (1, 4):
            assert b.inflate(threads=threads) == ref["stream"]
        if b.n_blocks > 1:  # a range in the middle lands at its own offsets
            lo, hi = ref["blocks"][1][4], ref["blocks"][-1][4]
            assert b.inflate(1, b.n_blocks - 1) == ref["stream"][lo:hi]
        assert b.header_text == ref["text"]
        assert b.references == ref["refs"]
        assert b.first_record == ref["first"]
        assert [int(x) for x in b.record_offsets()] == ref["offsets"]
    assert bam().read_bam_header(path) == [n for n, _ in ref["refs"]]
    return ref


# ---- the restatement and the fixtures -----------------------------------------------------------------------------------
def test_restatement_gives_the_fixture_literals():
    a = R.read_bam(CHR22)
    assert (len(a["blocks"]), len(a["stream"]), a["refs"], len(a["records"])) == (3, 6002, [("chr22", 50818468)], 16)
    flags = sorted(r["flag"] for r in a["records"])
    assert flags == sorted([163] * 5 + [83] * 5 + [99] * 3 + [147] * 3)
    assert sorted(r["mapq"] for r in a["records"]) == sorted([42] * 10 + [30] * 4 + [23] * 2)
    assert R.bam_qc_ref(a["refs"], a["records"]) == dict(total_reads=7, distinct=7, m1=7, m2=0, dups=0, mito_reads=0, nrf=1.0, pbc1=1.0, pbc2=7.0)
    d = R.read_bam(DUMMY)
    assert (len(d["blocks"]), len(d["stream"]), d["refs"], len(d["records"])) == (3, 344, [("chr1", 20)], 4)
    assert all(r["flag"] == 0 and r["mapq"] == 60 for r in d["records"])
    assert R.bam_qc_ref(d["refs"], d["records"]) == dict(total_reads=4, distinct=4, m1=4, m2=0, dups=0, mito_reads=0, nrf=1.0, pbc1=1.0, pbc2=4.0)


@pytest.mark.parametrize("path", [CHR22, DUMMY])
def test_reader_equals_the_python_reader_on_the_fixtures(path):
    assert_reader_equal(path)


# ---- written files ------------------------------------------------------------------------------------------------------
REFS = [("chr1", 100000), ("chr2", 50000)]


def some_records(n=6):
    return [R.rec(ref_id=i * 2 // max(n, 1), pos=100 + i, name=b"read%03d" % i, cigar=(("M", 5), ("I", 1), ("M", 4)), tlen=-i) for i in range(n)]


def test_a_cut_after_every_byte_of_one_record(tmp_path):
    """the second record's bytes, its block_size field included, are split at every position"""
    recs = some_records()
    head = len(R.encode_header(REFS, "@HD\tVN:1.6\n")) + len(R.encode_record(recs[0]))
    size = len(R.encode_record(recs[1]))
    for k in range(1, size + 1):
        p = str(tmp_path / "cut.bam")
        R.write_bam(p, REFS, recs, cuts=[head + k], text="@HD\tVN:1.6\n")
        ref = assert_reader_equal(p)
        assert len(ref["blocks"]) == 3 and ref["records"] == recs


def test_a_record_over_many_blocks_and_an_empty_block_in_the_middle(tmp_path):
    recs = some_records()
    head = len(R.encode_header(REFS))
    p = str(tmp_path / "many.bam")
    R.write_bam(p, REFS, recs, cuts=[head + 2, head + 2, head + 9, head + 30, head + 31, head + 90])
    ref = assert_reader_equal(p)
    assert 0 in [b[2] for b in ref["blocks"][:-1]] and ref["records"] == recs


def test_without_the_eof_block_zero_records_and_reference_counts(tmp_path):
    recs = some_records()
    p = str(tmp_path / "a.bam")
    R.write_bam(p, REFS, recs, eof=False)
    assert len(assert_reader_equal(p)["blocks"]) == 1
    R.write_bam(p, REFS, [])
    assert assert_reader_equal(p)["offsets"] == []
    R.write_bam(p, [], [])
    assert assert_reader_equal(p)["refs"] == []
    refs = [("contig_%d" % i, 1000 + i) for i in range(300)]
    R.write_bam(p, refs, [R.rec(ref_id=299, pos=5)], cuts=[100, 2000], text="@CO\tx\n" * 50)
    assert len(assert_reader_equal(p)["refs"]) == 300


# ---- corruptions --------------------------------------------------------------------------------------------------------
def refused(tmp_path, data, match, what=lambda b: b.record_offsets()):
    p = str(tmp_path / "bad.bam")
    with open(p, "wb") as f:
        f.write(data)
    with pytest.raises(ValueError, match=match):  # (GTARS_ERR_PARSE)
        with bam().BamFile(p) as b:
            what(b)


def good(records=None, **kw):
    return bytearray(R.bgzf_bytes(R.bam_stream(REFS, some_records() if records is None else records), **kw))


def test_container_corruptions_are_refused_with_the_block_index(tmp_path):
    head = len(R.encode_header(REFS))
    d = good(cuts=[head])
    second = len(R.bgzf_block(R.encode_header(REFS)))  # where block 1 starts
    bad = bytearray(d)
    bad[second] = 0x1e
    refused(tmp_path, bad, r"BGZF block 1 .*magic")
    bad = bytearray(d)
    bad[second + 12:second + 14] = b"XY"
    refused(tmp_path, bad, r"BGZF block 1 has no BC subfield")
    bad = bytearray(d)
    struct.pack_into("<H", bad, second + 16, 0xFFFF)
    refused(tmp_path, bad, r"BGZF block 1 runs past the end of the file")
    refused(tmp_path, d[:second + 40], r"BGZF block 1 runs past the end of the file")
    bsize = struct.unpack_from("<H", d, second + 16)[0]
    bad = bytearray(d)
    bad[second + 30] ^= 0x10  # a payload byte: the CRC (or the stream itself) gives it away
    refused(tmp_path, bad, r"BGZF block 1")
    bad = bytearray(d)
    isize_at = second + bsize + 1 - 4
    struct.pack_into("<I", bad, isize_at, struct.unpack_from("<I", d, isize_at)[0] + 1)
    refused(tmp_path, bad, r"BGZF block 1: inflate[sd]")
    bad = bytearray(d)
    struct.pack_into("<I", bad, isize_at, 65537)
    refused(tmp_path, bad, r"BGZF block 1: ISIZE 65537 > 65536")
    refused(tmp_path, R.bgzf_bytes(b"BAX\1" + bytes(20)), r"not a BAM file")
    refused(tmp_path, R.bgzf_bytes(R.encode_header(REFS)[:-3]), r"header is truncated")


def test_a_stored_block_with_a_wrong_crc_is_refused(tmp_path):
    """a flipped byte in a STORED block decodes cleanly: only the CRC-32 can refuse it"""
    stream = R.bam_stream(REFS, some_records())
    co = zlib.compressobj(0, zlib.DEFLATED, -15)
    comp = co.compress(stream) + co.flush()
    block = bytearray(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(comp) + 25) + comp +
                      struct.pack("<II", zlib.crc32(stream) & 0xFFFFFFFF, len(stream)))
    block[18 + 5 + 60] ^= 1
    refused(tmp_path, bytes(block) + R.EOF_BLOCK, r"BGZF block 0: CRC-32 mismatch", what=lambda b: b.inflate())


def test_record_corruptions_are_refused_with_the_record_index(tmp_path):
    recs = some_records()
    stream = bytearray(R.bam_stream(REFS, recs))
    at = len(R.encode_header(REFS)) + len(R.encode_record(recs[0])) + len(R.encode_record(recs[1]))
    bad = bytearray(stream)
    struct.pack_into("<I", bad, at, 31)
    refused(tmp_path, R.bgzf_bytes(bytes(bad)), r"BAM record 2: block_size 31 < 32")
    refused(tmp_path, R.bgzf_bytes(bytes(stream[:-7])), r"BAM record 5 runs past the end of the data")
    down = [R.rec(ref_id=1, pos=5), R.rec(ref_id=0, pos=9)]
    refused(tmp_path, good(down), r"BAM record 1: refID 0 follows refID 1: only coordinate-sorted")
    tail = [R.rec(ref_id=0, pos=5), R.rec(ref_id=-1, pos=-1, flag=4), R.rec(ref_id=1, pos=9)]
    refused(tmp_path, good(tail), r"BAM record 2: refID 1 follows refID -1: only coordinate-sorted")
    refused(tmp_path, good([R.rec(ref_id=2)]), r"BAM record 0: refID 2 is not in the header")


def test_a_missing_file_is_an_io_error(tmp_path):
    with pytest.raises(FileNotFoundError):
        bam().BamFile(str(tmp_path / "nothing.bam"))


def test_record_offsets_of_a_byte_range_leave_the_cut_record(tmp_path):
    recs = some_records()
    p = str(tmp_path / "a.bam")
    R.write_bam(p, REFS, recs)
    ref = R.read_bam(p)
    with bam().BamFile(p) as b:
        cut = ref["offsets"][3] + 2  # inside record 3's block_size field
        got = b.record_offsets(ref["stream"][:cut], ref["first"], final=False)
        assert [int(x) for x in got] == ref["offsets"][:3] and b.consumed == ref["offsets"][3]


# ---- TSV and CLI --------------------------------------------------------------------------------------------------------
def test_tsv_row_prints_floats_as_rust_does():
    B = bam()
    assert [B.format_f64(x) for x in (1.0, 0.1, 1e-7, 16.0, 2 / 3, 0.0, 1e21, 123456.789)] == \
        ["1", "0.1", "0.0000001", "16", "0.6666666666666666", "0", "1000000000000000000000", "123456.789"]
    r = B.BamQcResult(total_reads=10, distinct=3, m1=2, m2=1, dups=1, mito_reads=0, nrf=2 / 3, pbc1=1.0, pbc2=16.0)
    out = io.StringIO()
    B.write_bam_qc_tsv(r, out)
    lines = out.getvalue().split("\n")
    assert lines[0] == ("Total_read_pairs\tDistinct_read_pairs\tOne_read_pair\tTwo_read_pairs\tDuplicate_rate\tMitochondria_reads\t"
                        "Mitochondria_rate\tNRF\tPBC1\tPBC2")
    assert lines[1] == "10\t3\t2\t1\t0.1\t0\t0\t0.6666666666666666\t1\t16" and lines[2:] == [""]
    r = B.BamQcResult(total_reads=10_000_000, mito_reads=1, nrf=1.0, pbc1=1.0, pbc2=1.0)
    out = io.StringIO()
    B.write_bam_qc_tsv(r, out)
    assert out.getvalue().split("\n")[1] == "10000000\t0\t0\t0\t0\t1\t0.0000001\t1\t1\t1"
    assert B.BamQcResult().mito_rate() == 0.0 and B.BamQcResult().dup_rate() == 0.0


def test_cli_parses_bamqc_and_the_old_uniwig_lines(monkeypatch):
    from gtars_amd import cli

    a = cli.bamqc_parser().parse_args(["--input", "x.bam", "--output", "y.tsv"])
    assert (a.input, a.output, a.threads) == ("x.bam", "y.tsv", 1)
    a = cli.bamqc_parser().parse_args(["-i", "x.bam", "-o", "y.tsv", "-t", "4"])
    assert (a.input, a.output, a.threads) == ("x.bam", "y.tsv", 4)
    calls = []
    import gtars_amd.bam as B

    monkeypatch.setattr(B, "run_bam_qc", lambda *args: calls.append(args))
    assert cli.main(["uniwig", "bamqc", "-i", "x.bam", "-o", "y.tsv", "--threads", "3"]) == 0
    assert calls == [("x.bam", "y.tsv", 3)]
    # the old lines reach run_uniwig with the same values as before
    seen = []
    monkeypatch.setattr(cli, "run_uniwig", lambda ns: seen.append(ns) or 0)
    assert cli.main(["uniwig", "-f", "a.bed", "-c", "g.sizes", "-m", "5", "-s", "1", "-l", "out", "-y", "bedGraph", "-u", "core"]) == 0
    assert cli.main(["uniwig", "--file", "b.bam", "--filetype", "bam", "--chromref", "g", "--smoothsize", "1", "--stepsize", "1",
                     "--fileheader", "o"]) == 0
    assert calls == [("x.bam", "y.tsv", 3)]
    assert (seen[0].file, seen[0].chromref, seen[0].smoothsize, seen[0].stepsize, seen[0].fileheader, seen[0].outputtype, seen[0].counttype,
            seen[0].filetype, seen[0].wigstep, seen[0].score) == ("a.bed", "g.sizes", 5, 1, "out", "bedGraph", "core", "bed", "fixed", False)
    assert seen[1].filetype == "bam" and seen[1].file == "b.bam"
    with pytest.raises(SystemExit):  # uniwig's own options stay required
        cli.main(["uniwig", "--file", "a.bed"])


def test_uniwig_still_refuses_bam_input(capsys):
    from gtars_amd import cli, uniwig

    assert cli.main(["uniwig", "-f", "b.bam", "-t", "bam", "-c", "g", "-m", "1", "-s", "1", "-l", "o"]) == 2
    assert "bam is not provided" in capsys.readouterr().err
    assert uniwig.read_bam_header(DUMMY) == ["chr1"]


def test_alias_package_resolves_gtars_bam():
    import importlib

    import gtars_amd.bam as B

    assert importlib.import_module("gtars.bam") is B


@pytest.mark.skipif(__import__("gtars_amd").device_count() > 0, reason="needs a box WITHOUT a GPU")
def test_no_device_is_a_loud_error():
    import gtars_amd

    with pytest.raises(gtars_amd.NoDeviceError):
        bam().compute_bam_qc(DUMMY)
    with pytest.raises(gtars_amd.NoDeviceError):
        bam().BamFile(DUMMY).columns()
