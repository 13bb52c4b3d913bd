"""K17 on the device: BamFile.columns() against the pure Python reader and compute_bam_qc against bam_qc_ref (tests/bam_ref.py,
bamqc.rs restated), exactly -- integers equal, the three ratios bit-equal to Python's division.  Files of at most a few
thousand records, written by the test with chosen block cuts and read through chosen device windows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bam")
FIELDS = ("total_reads", "distinct", "m1", "m2", "dups", "mito_reads", "nrf", "pbc1", "pbc2")
REFS = [("chr1", 1_000_000), ("chr2", 500_000), ("chrM", 16_569)]
PAIRED, READ1, READ2, DUP, UNMAPPED = 0x1, 0x40, 0x80, 0x400, 0x4


def B():
    from gtars_amd import bam

    return bam


def as_dict(res):
    return {k: getattr(res, k) for k in FIELDS}


def check_file(path, **kw):
    """columns and QC of the file at `path`, against the Python reader's records"""
    ref = R.read_bam(path)
    want = R.bam_qc_ref(ref["refs"], ref["records"])
    got = as_dict(B().compute_bam_qc(path, **kw))
    assert got == want, (got, want)
    assert all(type(got[k]) is int for k in FIELDS[:6]) and all(type(got[k]) is float for k in FIELDS[6:])
    win = {k: v for k, v in kw.items() if k == "max_window_bytes"}
    with B().BamFile(path) as b:
        cols, exp = b.columns(**win), R.columns_ref(ref["records"])
    assert sorted(cols) == sorted(exp)
    for k in exp:
        assert cols[k].dtype == np.int32 and np.array_equal(cols[k], exp[k]), k
    return want


def check(tmp_path, refs, records, cuts=None, name="t.bam", **kw):
    p = str(tmp_path / name)
    R.write_bam(p, refs, records, cuts=cuts)
    return check_file(p, **kw)


def single(n, ref_id=0, pos0=100, **kw):
    return [R.rec(ref_id=ref_id, pos=pos0 + 3 * i, name=b"s%05d" % i, **kw) for i in range(n)]


def pair(name, pos1, pos2, ref_id=0, tlen=None, mapq=60, extra1=0, extra2=0):
    tlen = pos2 - pos1 + 10 if tlen is None else tlen
    return [R.rec(ref_id=ref_id, pos=pos1, name=name, flag=PAIRED | READ1 | 0x2 | extra1, tlen=tlen, mapq=mapq, next_ref_id=ref_id, next_pos=pos2),
            R.rec(ref_id=ref_id, pos=pos2, name=name, flag=PAIRED | READ2 | 0x2 | extra2, tlen=-tlen, mapq=mapq, next_ref_id=ref_id, next_pos=pos1)]


def coordinate_sorted(records):
    """stable: records of one position keep the order they were given in"""
    return sorted(records, key=lambda r: (r["ref_id"] if r["ref_id"] >= 0 else 1 << 30, r["pos"]))


# ---- fixtures -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,total,pbc2", [("test_chr22_small.bam", 7, 7.0), ("dummy.bam", 4, 4.0)])
def test_fixtures(name, total, pbc2):
    want = check_file(os.path.join(GOLDEN, name))
    assert want == dict(total_reads=total, distinct=total, m1=total, m2=0, dups=0, mito_reads=0, nrf=1.0, pbc1=1.0, pbc2=pbc2)
    assert as_dict(B().compute_bam_qc(os.path.join(GOLDEN, name), max_window_bytes=100)) == want


def test_run_bam_qc_writes_the_tsv(tmp_path):
    out = str(tmp_path / "qc.tsv")
    res = B().run_bam_qc(os.path.join(GOLDEN, "test_chr22_small.bam"), out)
    assert res.total_reads == 7
    assert open(out).read().split("\n")[1:] == ["7\t7\t7\t0\t0\t0\t0\t1\t1\t7", ""]


# ---- sizes, windows -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_record_counts(tmp_path, n):
    recs = single(n)
    for i in range(0, n, 5):  # some keys twice
        recs[i]["pos"] = recs[max(i - 1, 0)]["pos"]
    want = check(tmp_path, REFS, coordinate_sorted(recs))
    assert want["total_reads"] == n


def test_windows_that_cut_records_and_their_block_size_fields(tmp_path):
    recs = coordinate_sorted(single(40) + [r for i in range(20) for r in pair(b"p%d" % i, 500 + 7 * i, 560 + 7 * i, ref_id=1)])
    head = len(R.encode_header(REFS))
    sizes = [len(R.encode_record(r)) for r in recs]
    starts = np.cumsum([head] + sizes)[:-1]
    # blocks that end 1, 2 and 3 bytes into a block_size field, in the middle of a record, and exactly between two records
    cuts = sorted([int(starts[3]) + 1, int(starts[5]) + 2, int(starts[9]) + 3, int(starts[12]) + 40, int(starts[20]), int(starts[41]) + 2,
                   int(starts[60]) + 17])
    p = str(tmp_path / "w.bam")
    R.write_bam(p, REFS, recs, cuts=cuts)
    want = check_file(p)
    for mw in (1, 30, 64, 200, 333, 4096):  # one block per window ... all blocks in one; 1 and 30 are smaller than any record
        assert as_dict(B().compute_bam_qc(p, max_window_bytes=mw)) == want, mw
        with B().BamFile(p) as b:
            cols = b.columns(max_window_bytes=mw)
            assert np.array_equal(cols["start"], R.columns_ref(recs)["start"]) and np.array_equal(cols["tlen"], R.columns_ref(recs)["tlen"])
            part = b.columns(first=7, count=30, max_window_bytes=mw)
            assert np.array_equal(part["end"], R.columns_ref(recs[7:37])["end"])


def test_a_record_larger_than_many_windows(tmp_path):
    """blocks of 50 bytes and windows of 10: the window grows by a block at a time until the record is whole"""
    recs = single(3, l_seq=400) + single(2, ref_id=1)
    p = str(tmp_path / "big.bam")
    R.write_bam(p, REFS, recs, block=50)
    check_file(p, max_window_bytes=10)


# ---- single-end ---------------------------------------------------------------------------------------------------------
def test_single_end_key_counts_and_filters(tmp_path):
    recs = []
    for count, pos in ((1, 10), (2, 20), (3, 30), (64, 40)):
        recs += [R.rec(pos=pos, name=b"k%d_%d" % (pos, i), l_seq=36) for i in range(count)]
    recs += [R.rec(pos=50, l_seq=36), R.rec(pos=50, l_seq=37), R.rec(pos=50, l_seq=37)]  # equal pos, different l_seq
    recs += [R.rec(pos=60, mapq=29), R.rec(pos=60, mapq=30), R.rec(pos=61, mapq=255), R.rec(pos=62, mapq=0)]
    recs += [R.rec(pos=70, flag=UNMAPPED), R.rec(pos=71, flag=DUP), R.rec(pos=71, flag=DUP | UNMAPPED), R.rec(pos=72, flag=DUP, mapq=3)]
    recs = [R.rec(pos=-1, name=b"nopos"), R.rec(pos=-1, name=b"nopos_dup", flag=DUP)] + recs  # pos -1 sorts first
    recs += [R.rec(ref_id=-1, pos=-1, flag=UNMAPPED, name=b"tail")]
    want = check(tmp_path, REFS, recs)
    assert want["m2"] == 2 and want["dups"] == 2 and want["distinct"] == 4 + 2 + 2 + 1
    assert want["total_reads"] == 70 + 3 + 2 + 1 + 2


def test_mitochondrial_references(tmp_path):
    refs = [("chrM", 100), ("MT", 100), ("chrMt", 100), ("x_rCRSd_y", 100), ("chrM2", 100), ("chr1", 100)]
    recs = []
    for c in range(6):
        recs += [R.rec(ref_id=c, pos=5), R.rec(ref_id=c, pos=5, flag=DUP), R.rec(ref_id=c, pos=6, mapq=10), R.rec(ref_id=c, pos=7, flag=UNMAPPED)]
        recs += pair(b"m%d" % c, 8, 9, ref_id=c)
    want = check(tmp_path, refs, recs)
    assert want["mito_reads"] == 16 and want["total_reads"] == 2 and want["dups"] == 6


# ---- paired -------------------------------------------------------------------------------------------------------------
def paired_records():
    """every paired case of the issue on chr1 and chr2, 40 names per table on chr1 -- more than 16, so that 4 hash bits collide"""
    recs = []
    for i in range(40):  # complete pairs, four of them at one four-tuple, two at another
        p1 = 1000 + (0 if i < 4 else 5 if i < 6 else 11 * i)
        recs += pair(b"pair_%02d" % i, p1, p1 + 150, tlen=160 if i < 6 or i % 2 else -160)
    recs += pair(b"q", 3000, 3100) + pair(b"r", 3000, 3100)  # names of 1 byte
    recs += pair(b"n" * 254, 3200, 3300) + pair(b"n" * 253 + b"m", 3200, 3300)  # 254 bytes, equal up to the last one
    recs += pair(b"same_prefix_a", 3400, 3500) + pair(b"same_prefix_b", 3401, 3500) + pair(b"same_prefix_", 3402, 3500)
    # orphans: the mate is on chr2 (and the other way round), or nowhere
    recs += [R.rec(pos=4000, name=b"split", flag=PAIRED | READ1, tlen=0, next_ref_id=1, next_pos=77),
             R.rec(ref_id=1, pos=77, name=b"split", flag=PAIRED | READ2, tlen=0, next_ref_id=0, next_pos=4000),
             R.rec(pos=4010, name=b"lonely1", flag=PAIRED | READ1 | 0x8), R.rec(pos=4020, name=b"lonely2", flag=PAIRED | READ2 | 0x8)]
    # a name three times among the read-1 records and twice among the read-2 records: the last of each wins
    recs += [R.rec(pos=5000, name=b"again", flag=PAIRED | READ1, tlen=1), R.rec(pos=5001, name=b"again", flag=PAIRED | READ1, tlen=2),
             R.rec(pos=5002, name=b"again", flag=PAIRED | READ1, tlen=3), R.rec(pos=5003, name=b"again", flag=PAIRED | READ2, tlen=-1),
             R.rec(pos=5004, name=b"again", flag=PAIRED | READ2, tlen=-2)]
    # 0x1 alone is in no table; 0x1 | 0x40 | 0x80 is read 1
    recs += [R.rec(pos=5100, name=b"neither", flag=PAIRED), R.rec(pos=5101, name=b"both", flag=PAIRED | READ1 | READ2, tlen=9),
             R.rec(pos=5102, name=b"both", flag=PAIRED | READ2, tlen=-9)]
    # single-end records in the same chromosome, one of them twice, and filtered paired records
    recs += [R.rec(pos=5200, l_seq=50), R.rec(pos=5200, l_seq=50), R.rec(pos=5201, l_seq=50)]
    recs += pair(b"lowq", 5300, 5400, mapq=12) + pair(b"dupd", 5500, 5600, extra1=DUP, extra2=DUP)
    recs += [R.rec(pos=5700, name=b"half", flag=PAIRED | READ1, tlen=5), R.rec(pos=5800, name=b"half", flag=PAIRED | READ2 | UNMAPPED, tlen=-5)]
    recs += [R.rec(pos=-1, name=b"unplaced_mate", flag=PAIRED | READ1)]
    # chr2: read-1 records only, and pairs that repeat chr1's names and tuples (keys do not cross chromosomes)
    recs += [R.rec(ref_id=1, pos=100 + i, name=b"only1_%d" % i, flag=PAIRED | READ1, tlen=7) for i in range(5)]
    recs += pair(b"pair_00", 1000, 1150, ref_id=1, tlen=-160) + pair(b"negative", 2000, 1900, ref_id=1, tlen=-90)
    recs += pair(b"mt", 10, 50, ref_id=2)
    return coordinate_sorted(recs)


@pytest.fixture(scope="module")
def paired_file(tmp_path_factory):
    recs = paired_records()
    p = str(tmp_path_factory.mktemp("bam") / "paired.bam")
    R.write_bam(p, REFS, recs, cuts=[700, 2000, 2001, 5000])
    return p, recs


def test_paired_cases(paired_file):
    p, recs = paired_file
    want = check_file(p)
    one = R.process_chromosome(recs, 0, "chr1")
    assert sorted(one["position_counts"].values(), reverse=True)[:3] == [4, 2, 2] and want["m2"] >= 2
    assert want["total_reads"] == R.process_chromosome(recs, 0, "chr1")["num_pairs"] + 2  # joined pairs; chr2 adds two
    assert (5003, 3, 5005, -2) in one["position_counts"] and (5001, 1, 5004, -1) not in one["position_counts"]  # the last wins
    assert (5102, 9, 5103, -9) in one["position_counts"]


@pytest.mark.parametrize("bits", ["4", "0", "1", "33"])
def test_results_do_not_depend_on_the_name_hash(paired_file, monkeypatch, bits):
    """4 bits: 16 hash values for more than 40 distinct names per table on chr1, so runs of equal hash with different names are
    certain; 0 bits: every name of a table is in ONE run"""
    p, recs = paired_file
    names = {r["name"] for r in recs if r["ref_id"] == 0 and r["flag"] & READ1}
    assert len(names) >= 17
    default = as_dict(B().compute_bam_qc(p))
    monkeypatch.setenv("GTARS_BAM_NAME_HASH_BITS", bits)
    assert as_dict(B().compute_bam_qc(p)) == default
    assert as_dict(B().compute_bam_qc(p, max_window_bytes=500)) == default
    monkeypatch.delenv("GTARS_BAM_NAME_HASH_BITS")
    assert as_dict(B().compute_bam_qc(p)) == default == R.bam_qc_ref(REFS, recs)


def test_threads_and_windows_give_the_same_result(paired_file):
    p, recs = paired_file
    want = R.bam_qc_ref(REFS, recs)
    for threads in (1, 4):
        for mw in (None, 300, 5000):
            assert as_dict(B().compute_bam_qc(p, threads=threads, max_window_bytes=mw)) == want, (threads, mw)


def test_chromosomes_with_one_table_only(tmp_path):
    """read-1 records only on chr1, read-2 records only on chr2: nothing joins, and paired data divides by the pairs"""
    recs = [R.rec(pos=10 + i, name=b"a%d" % i, flag=PAIRED | READ1, tlen=30) for i in range(70)]
    recs += [R.rec(ref_id=1, pos=10 + i, name=b"a%d" % i, flag=PAIRED | READ2, tlen=-30) for i in range(70)]
    want = check(tmp_path, REFS, recs)
    assert want == dict(total_reads=0, distinct=0, m1=0, m2=0, dups=0, mito_reads=0, nrf=0.0, pbc1=0.0, pbc2=0.0)
    want = check(tmp_path, REFS, recs + [R.rec(ref_id=1, pos=500, l_seq=20), R.rec(ref_id=1, pos=500, l_seq=20)], name="mixed.bam")
    assert (want["total_reads"], want["distinct"], want["m2"], want["nrf"]) == (0, 1, 1, 0.0)


def test_three_hundred_references_three_with_reads(tmp_path):
    refs = [("ctg%03d" % i, 10_000) for i in range(300)]
    recs = []
    for c in (0, 150, 299):
        recs += coordinate_sorted(single(30, ref_id=c) + [r for i in range(10) for r in pair(b"x%d" % i, 200 + (i // 2), 300, ref_id=c)])
    want = check(tmp_path, refs, recs, max_window_bytes=2000)
    assert want["total_reads"] == 30 and want["m2"] == 15


def test_a_few_thousand_records(tmp_path):
    rng = np.random.default_rng(17)
    recs = []
    for c in (0, 1):
        pos = np.sort(rng.integers(0, 3000, 1500))
        for i, ps in enumerate(pos):
            recs += pair(b"frag_%d_%04d" % (c, rng.integers(0, 1200)), int(ps), int(ps) + int(rng.integers(50, 60)), ref_id=c,
                         mapq=int(rng.choice([60, 60, 60, 20, 255])), extra1=DUP if i % 9 == 0 else 0)
    recs += [R.rec(ref_id=2, pos=int(x)) for x in np.sort(rng.integers(0, 16000, 300))]
    want = check(tmp_path, REFS, coordinate_sorted(recs), max_window_bytes=100_000)
    assert want["m2"] > 0 and want["mito_reads"] == 300 and 0 < want["nrf"] < 1


# ---- CIGAR --------------------------------------------------------------------------------------------------------------
def test_cigar_spans(tmp_path):
    recs = [R.rec(pos=10 + i, cigar=((op, 7),)) for i, op in enumerate("MIDNSHP=X")]
    recs.append(R.rec(pos=100, cigar=(("S", 3), ("M", 20), ("I", 2), ("M", 5), ("D", 4), ("N", 1000), ("=", 6), ("X", 1), ("H", 9), ("P", 2))))
    recs.append(R.rec(pos=200, cigar=[("M", 1 + k % 3) if k % 2 else ("I", 2) for k in range(40)]))
    recs.append(R.rec(pos=300, cigar=(("S", 50), ("N", (1 << 28) - 1))))  # the placeholder of a CIGAR kept in a CG tag: kSmN
    p = str(tmp_path / "c.bam")
    R.write_bam(p, REFS, recs)
    check_file(p)
    with B().BamFile(p) as b:
        cols = b.columns()
    span = cols["end"] - cols["start"]
    assert list(span[:9]) == [7, 0, 7, 7, 0, 0, 0, 7, 7] and span[9] == 20 + 5 + 4 + 1000 + 6 + 1 and span[11] == (1 << 28) - 1


# ---- the three rules this library pins ------------------------------------------------------------------------------------
def test_rule_a_name_stored_as_star_is_missing(tmp_path):
    recs = [R.rec(pos=10, name=b"*", flag=PAIRED | READ1, tlen=5), R.rec(pos=20, name=b"*", flag=PAIRED | READ2, tlen=-5)] + pair(b"**", 30, 40)
    recs += [R.rec(pos=50, name=b"*", l_seq=9)]  # single-end: the name plays no part
    res = B().compute_bam_qc(R_write(tmp_path, REFS, recs))
    assert as_dict(res) == dict(total_reads=1, distinct=2, m1=2, m2=0, dups=0, mito_reads=0, nrf=2.0, pbc1=1.0, pbc2=2.0)


def test_rule_an_empty_cigar_counts_and_ends_at_its_position(tmp_path):
    recs = [R.rec(pos=10, cigar=()), R.rec(pos=10, cigar=()), R.rec(pos=11, cigar=(("I", 5),))]
    p = R_write(tmp_path, REFS, recs)
    res = B().compute_bam_qc(p)
    assert (res.total_reads, res.distinct, res.m1, res.m2) == (3, 2, 1, 1)
    with B().BamFile(p) as b:
        cols = b.columns()
    assert list(cols["end"]) == [10, 10, 11]


def test_rule_a_colon_in_a_reference_name_is_a_name_like_any_other(tmp_path):
    refs = [("HLA-A*01:01:01:01", 3000), ("chr1:100-200", 500)]
    recs = single(4, ref_id=0) + single(3, ref_id=1) + [R.rec(ref_id=1, pos=106)]
    res = B().compute_bam_qc(R_write(tmp_path, refs, recs))
    assert (res.total_reads, res.distinct, res.m1, res.m2) == (8, 7, 6, 1)


def R_write(tmp_path, refs, recs):
    p = str(tmp_path / "rule.bam")
    R.write_bam(p, refs, recs)
    return p


def test_a_record_whose_fields_do_not_fit_its_block_size_is_refused(tmp_path):
    """n_cigar_op says 1000 in a record of 60 bytes: the decode kernel reads nothing beyond the record and the call fails"""
    import struct

    recs = single(5)
    stream = bytearray(R.bam_stream(REFS, recs))
    at = len(R.encode_header(REFS)) + len(R.encode_record(recs[0]))
    struct.pack_into("<H", stream, at + 4 + 12, 1000)
    p = str(tmp_path / "bad.bam")
    with open(p, "wb") as f:
        f.write(R.bgzf_bytes(bytes(stream)))
    with pytest.raises(ValueError, match="longer than its block_size"):
        B().compute_bam_qc(p)
