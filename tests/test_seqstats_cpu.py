"""Host side of the sequence statistics (K12): the restatement (tests/seqstats_ref.py) pinned by hand on the reference's
FASTA fixtures, the FASTA and .fab readers and the .fab writer of the library against it, and the ordering / error rules
that are decided on the host before anything is launched.  No device is needed."""
import os
import struct

import pytest

import seqstats_ref as R

FASTA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fasta")
FIXTURES = ["base", "wrapped_40", "wrapped_20", "unwrapped", "crlf_endings"]


def _fa(name):
    return os.path.join(FASTA, name + ".fa")


def _fai(name):
    """columns 1-2 of the .fai: (name, length) per record"""
    return [(f[0], int(f[1])) for f in (line.split("\t") for line in open(_fa(name) + ".fai").read().splitlines())]


def _row(**kw):
    return [float(kw.get(d, 0)) for d in R.DINUCL_ORDER]


# ---- the restatement, by hand --------------------------------------------------------------------------------------------
def test_restatement_on_base_fa():
    g = R.read_fasta(_fa("base"))
    assert g == {"chrX": b"TTGGGGAA", "chr1": b"GGAA", "chr2": b"GCGC"}
    assert R.calc_gc_content([("chrX", 0, 4)], g) == [0.5]
    assert R.calc_gc_content([("chr2", 0, 4)], g) == [1.0]
    labels, raw = R.calc_dinucl_freq([("chrX", 0, 8)], g, raw_counts=True)
    assert labels == ["chrX_0_8"]
    assert raw == [_row(Aa=1, Ga=1, Gg=3, Tg=1, Tt=1)] and sum(raw[0]) == 7  # 8 bases -> 7 windows
    _, pct = R.calc_dinucl_freq([("chrX", 0, 8)], g)
    assert abs(sum(pct[0]) - 100.0) < 1e-9
    assert pct[0] == [(c / 7) * 100.0 for c in raw[0]]
    # an empty region: 0.0, a zero row, its label present
    assert R.calc_gc_content([("chr1", 2, 2)], g) == [0.0]
    assert R.calc_dinucl_freq([("chr1", 2, 2)], g) == (["chr1_2_2"], [[0.0] * 16])
    assert R.calc_dinucl_freq([("chr1", 2, 2)], g, raw_counts=True) == (["chr1_2_2"], [[0.0] * 16])


def test_restatement_on_wrapped_40():
    g = R.read_fasta(_fa("wrapped_40"))
    assert g["chr3"] == b"N" * 40
    assert R.calc_gc_content([("chr3", 0, 40)], g) == [0.0]
    assert R.calc_dinucl_counts([("chr3", 0, 40)], g) == (["chr3_0_40"], [[0] * 16])
    assert R.calc_gc_content([("chr1", 0, 40)], g) == [0.5]  # ACGT x 10
    # case and N: lower case counts, N voids both windows it touches but stays in the GC denominator
    assert R.calc_gc_content([("c", 0, 4)], {"c": b"gcNa"}) == [0.5]
    assert R.dinucl_counts(b"acNgT") == [int(d in ("Ac", "Gt")) for d in R.DINUCL_ORDER]


def test_restatement_order_skips_and_errors():
    g = {"a": b"ACGTACGT", "b": b"GGGG"}
    rows = [("b", 0, 4), ("a", 0, 2), ("zz", 0, 1), ("b", 3, 9), ("a", 5, 3), ("a", 4, 8), ("b", 1, 2)]
    labels, _ = R.calc_dinucl_counts(rows, g, ignore_unk_chroms=True)
    assert labels == ["b_0_4", "b_1_2", "a_0_2", "a_4_8"]  # grouped by first appearance, set order inside
    assert R.calc_gc_content(rows, g, ignore_unk_chroms=True) == [1.0, 1.0, 0.5, 0.5]
    with pytest.raises(RuntimeError, match="b 3 9"):
        R.calc_gc_content(rows, g)


# ---- the library's readers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_fasta_reader_matches_fai_and_restatement(name):
    from gtars_amd.seqstats import GenomeAssembly

    g = GenomeAssembly(_fa(name))
    want = _fai(name)
    assert len(g) == len(want)
    assert g.chrom_names == [n for n, _ in want]
    assert g.chrom_sizes == dict(want)
    ref = R.read_fasta(_fa(name))
    assert list(ref) == g.chrom_names
    for chr_, n in want:
        assert g.contains_chr(chr_)
        seq = g.sequence(chr_, 0, n)
        assert seq == ref[chr_] and b"\r" not in seq and b"\n" not in seq
        assert g.sequence(chr_, n, n) == b"" and g.sequence(chr_, 1, n - 1) == ref[chr_][1:n - 1]
        for bad in ((0, n + 1), (2, 1)):
            with pytest.raises(ValueError, match="Invalid range"):
                g.sequence(chr_, *bad)
    assert not g.contains_chr("chrNope")
    with pytest.raises(ValueError, match="Unknown chromosome"):
        g.sequence("chrNope", 0, 1)
    assert g.device == -1  # nothing has counted yet


def test_wrapping_does_not_change_the_bytes():
    from gtars_amd.seqstats import GenomeAssembly

    a, b, c = (GenomeAssembly(_fa(n)) for n in ("wrapped_20", "wrapped_40", "unwrapped"))
    for chr_, n in _fai("unwrapped"):
        assert a.sequence(chr_, 0, n) == b.sequence(chr_, 0, n) == c.sequence(chr_, 0, n)


def test_fasta_reader_rules(tmp_path):
    from gtars_amd.seqstats import GenomeAssembly

    p = tmp_path / "dup.fa"
    p.write_bytes(b">chrA first record\nACGT\nAC  \n\n>chrB\tdesc\nnnNN\r\n>chrA\nTT\n>\nG\n>empty\n")
    g = GenomeAssembly(str(p))
    assert g.chrom_names == ["chrA", "chrB", "", "empty"]
    assert g.chrom_sizes == {"chrA": 2, "chrB": 4, "": 1, "empty": 0}
    assert g.sequence("chrA", 0, 2) == b"TT"  # the last record of a repeated name
    assert g.sequence("chrB", 0, 4) == b"nnNN"  # bytes as they are
    assert R.read_fasta(str(p)) == {"chrA": b"TT", "chrB": b"nnNN", "": b"G", "empty": b""}
    (tmp_path / "none.fa").write_bytes(b"")
    assert len(GenomeAssembly(str(tmp_path / "none.fa"))) == 0
    (tmp_path / "bad.fa").write_bytes(b"ACGT\n>chr1\nAC\n")
    with pytest.raises(ValueError):
        GenomeAssembly(str(tmp_path / "bad.fa"))
    with pytest.raises(ValueError):
        GenomeAssembly(str(tmp_path / "missing.fa"))
    with pytest.raises(ValueError):
        R.read_fasta_records(str(tmp_path / "bad.fa"))


# ---- .fab -----------------------------------------------------------------------------------------------------------------
def _entry(name, offset, length):
    return struct.pack("<H", len(name)) + name + struct.pack("<QQ", offset, length)


def test_write_fab_is_the_layout_packed_by_hand(tmp_path):
    from gtars_amd.seqstats import write_fab

    out = tmp_path / "base.fab"
    write_fab(_fa("base"), str(out))
    head = 9 + 3 * (2 + 4 + 16)
    want = (b"GFAB" + b"\x01" + struct.pack("<I", 3) + _entry(b"chrX", head, 8) + _entry(b"chr1", head + 8, 4) +
            _entry(b"chr2", head + 12, 4) + b"TTGGGGAA" + b"GGAA" + b"GCGC")
    assert out.read_bytes() == want
    assert want == R.pack_fab(R.read_fasta_records(_fa("base")))
    with pytest.raises(ValueError):
        write_fab(str(tmp_path / "missing.fa"), str(tmp_path / "x.fab"))


@pytest.mark.parametrize("name", FIXTURES)
def test_fab_round_trip(name, tmp_path):
    from gtars_amd.seqstats import BinaryGenomeAssembly, GenomeAssembly, write_fab

    out = str(tmp_path / (name + ".fab"))
    write_fab(_fa(name), out)
    f, b = GenomeAssembly(_fa(name)), BinaryGenomeAssembly(out)
    assert b.chrom_names == f.chrom_names and b.chrom_sizes == f.chrom_sizes
    for chr_, n in f.chrom_sizes.items():
        assert b.sequence(chr_, 0, n) == f.sequence(chr_, 0, n)
    assert R.read_fab(open(out, "rb").read()) == R.read_fasta(_fa(name))


def test_fab_writes_every_record_and_reads_the_last_of_a_name(tmp_path):
    from gtars_amd.seqstats import BinaryGenomeAssembly, write_fab

    fa = tmp_path / "dup.fa"
    fa.write_bytes(b">a\nAC\n>b\nGGG\n>a\nT\n")
    write_fab(str(fa), str(tmp_path / "dup.fab"))
    data = (tmp_path / "dup.fab").read_bytes()
    assert data == R.pack_fab([("a", b"AC"), ("b", b"GGG"), ("a", b"T")])
    g = BinaryGenomeAssembly(str(tmp_path / "dup.fab"))
    assert g.chrom_sizes == {"a": 1, "b": 3} and g.sequence("a", 0, 1) == b"T"


def test_malformed_fab_files_raise(tmp_path):
    from gtars_amd.seqstats import BinaryGenomeAssembly

    good = R.pack_fab([("chr1", b"ACGT"), ("chr2", b"GG")])
    first_entry = 9 + 2 + 4
    cases = {
        "too_short": (good[:8], "too short"),
        "bad_magic": (b"GFAX" + good[4:], "bad magic"),
        "wrong_version": (good[:4] + b"\x02" + good[5:], "version"),
        "truncated_index": (good[:5] + struct.pack("<I", 3) + good[9:9 + 2 * 22], "truncated index"),
        "truncated_entry": (good[:9 + 22 + 2 + 4 + 10], "truncated index entry"),
        "beyond_the_file": (good[:first_entry + 8] + struct.pack("<Q", 5) + good[first_entry + 16:-2], "beyond file"),
    }
    assert sorted(BinaryGenomeAssembly(_write(tmp_path, "good", good)).chrom_sizes.items()) == [("chr1", 4), ("chr2", 2)]
    for name, (data, why) in cases.items():
        with pytest.raises(ValueError, match=why):
            BinaryGenomeAssembly(_write(tmp_path, name, data))
        with pytest.raises(ValueError):
            R.read_fab(data)
    with pytest.raises(ValueError):
        BinaryGenomeAssembly(str(tmp_path / "missing.fab"))


def _write(tmp_path, name, data):
    p = tmp_path / (name + ".fab")
    p.write_bytes(data)
    return str(p)


# ---- what the host decides before a launch -----------------------------------------------------------------------------------
def test_unknown_rows_fail_or_are_skipped_without_a_device():
    from gtars_amd.seqstats import DINUCLEOTIDES, calc_dinucl_freq, calc_gc_content
    from gtars_amd.models import Region, RegionSet
    from gtars_amd.seqstats import GenomeAssembly

    g = GenomeAssembly(_fa("base"))
    rs = RegionSet.from_regions([Region("chrNope", 5, 9), Region("chrX", 0, 9), Region("chr1", 3, 2), Region("chrNope", 0, 1)])
    assert DINUCLEOTIDES == R.DINUCL_ORDER
    for call in (calc_gc_content, calc_dinucl_freq):
        with pytest.raises(RuntimeError, match=r"chrNope.*5.*9"):
            call(rs, g)
        with pytest.raises(RuntimeError, match=r"chrNope.*5.*9"):
            call(rs, g, ignore_unk_chroms=False)
    # known chromosome, bad range: the first one in output order
    with pytest.raises(RuntimeError, match=r"chrX.*0.*9"):
        calc_gc_content(RegionSet.from_regions([Region("chrX", 0, 9), Region("chr1", 3, 2)]), g)
    with pytest.raises(RuntimeError, match=r"chr1.*3.*2"):
        calc_dinucl_freq(RegionSet.from_regions([Region("chr1", 3, 2)]), g)
    # every row unknown or out of range: nothing to count
    assert calc_gc_content(rs, g, ignore_unk_chroms=True) == []
    assert calc_dinucl_freq(rs, g, ignore_unk_chroms=True) == {"region_labels": [], "dinucleotides": R.DINUCL_ORDER,
                                                               "frequencies": []}
    assert calc_gc_content(RegionSet.from_regions([]), g) == []
    assert g.device == -1
    for other in (None, "hg38.fa", rs):
        with pytest.raises(RuntimeError, match="genome must be"):
            calc_gc_content(rs, other)
        with pytest.raises(RuntimeError, match="genome must be"):
            calc_dinucl_freq(rs, other)


def test_alias_package_has_the_new_names():
    import importlib

    import gtars
    import gtars_amd.seqstats as S

    assert importlib.import_module("gtars.seqstats") is S and gtars.seqstats is S and "seqstats" in gtars.__all__
    from gtars.seqstats import BinaryGenomeAssembly, GenomeAssembly, calc_dinucl_freq, calc_gc_content, write_fab

    assert (GenomeAssembly, BinaryGenomeAssembly, write_fab) == (S.GenomeAssembly, S.BinaryGenomeAssembly, S.write_fab)
    assert calc_gc_content is S.calc_gc_content and calc_dinucl_freq is S.calc_dinucl_freq


def test_restatement_on_the_lane_step_rows():
    """The rows of test_gpu_seqstats.test_lane_group_step_edges (255 rows of at most 1041 bytes around one step of either lane
    grouping): the plain-Python restatement counts them in well under a second (0.02 s when written) and agrees with a count
    of the same bytes by numpy table look-ups."""
    import time

    import numpy as np
    from test_gpu_seqstats import _make_sequences, step_edge_rows

    seqs, rows = _make_sequences(), step_edge_rows()
    assert len(rows) == 255 and max(e - s for _, s, e in rows) == 1041
    t0 = time.perf_counter()
    gc = R.calc_gc_content(rows, seqs, False)
    labels, counts = R.calc_dinucl_counts(rows, seqs, False)
    assert time.perf_counter() - t0 < 1.0
    code = np.full(256, -1, dtype=np.int64)
    for k, letter in enumerate("ACGT"):
        code[ord(letter)] = code[ord(letter.lower())] = k
    order = [4 * "ACGT".index(d[0].upper()) + "ACGT".index(d[1].upper()) for d in R.DINUCL_ORDER]
    by_label = dict(zip(labels, counts))
    for (name, s, e), got_gc in zip(rows, gc):
        b = code[np.frombuffer(seqs[name][s:e], dtype=np.uint8)]
        assert got_gc == int(((b == 1) | (b == 2)).sum()) / (e - s)
        pair = np.where((b[:-1] >= 0) & (b[1:] >= 0), 4 * b[:-1] + b[1:], -1)
        assert by_label[f"{name}_{s}_{e}"] == [int((pair == o).sum()) for o in order]
