"""K26 on the device: BamFile.fragments / bam_to_fragments against fragments_ref (tests/bam_frag_ref.py, the rule of DESIGN.md
section 3 K26 restated) -- columns, barcode list, statistics and written bytes, all exactly.  Files of at most a few
thousand records, written by the test with chosen BGZF cuts and read through chosen device windows."""
import gzip
import os
import re
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bam_frag_ref as F  # noqa: E402
from test_bam_frag_cpu import EVERY_TYPE, EXAMPLE_REFS, EXAMPLE_STATS, EXAMPLE_TEXT, example_records  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "bam")
REFS = [("chr1", 100_000), ("chr2", 50_000)]


def B():
    from gtars_amd import bam

    return bam


def pr(ref, pos, tlen, cb=b"AAC-1", flag=99, mapq=60, aux=None, next_ref=None, l_seq=10):
    """the leftmost mate of a proper pair unless the arguments say otherwise"""
    aux = (F.aux_Z("CB", cb) if cb is not None else b"") if aux is None else aux
    return F.rec(ref_id=ref, pos=pos, tlen=tlen, flag=flag, mapq=mapq, next_ref_id=ref if next_ref is None else next_ref, next_pos=pos, aux=aux,
                 l_seq=l_seq, cigar=(("M", l_seq),))


def mate(r):
    """the rightmost mate of r: the same tags, a negative tlen"""
    return dict(r, pos=r["pos"] + max(r["tlen"] - r["l_seq"], 0), tlen=-r["tlen"], flag=(r["flag"] & ~0x60) | 0x80 | 0x10)


def sort_records(records):
    return sorted(records, key=lambda r: (r["ref_id"] if r["ref_id"] >= 0 else 1 << 30, r["pos"]))


def compare(fr, refs, want):
    rows, barcodes, stats, _ = want
    cols = dict(ref=np.int32, start=np.uint32, end=np.uint32, barcode=np.uint32, count=np.uint32)
    for k, (name, dt) in enumerate(cols.items()):
        got = getattr(fr, name)
        assert got.dtype == dt and got.tolist() == [r[k] for r in rows], name
    assert fr.barcodes == [b.decode() for b in barcodes]
    assert fr.stats == stats and all(type(v) is int for v in fr.stats.values())
    assert fr.references == refs and len(fr) == len(rows)
    assert stats["records"] == sum(stats[k] for k in F.REASONS) + stats["kept_pairs"] and int(fr.count.sum()) == stats["kept_pairs"]


def check_file(path, refs, records, tmp_path, max_window_bytes=None, device_write=True, **params):
    """every output of the file at `path` against the restatement over `records`"""
    want = F.fragments_ref(refs, records, **params)
    with B().BamFile(path) as b:
        fr = b.fragments(max_window_bytes=max_window_bytes, **params)
    compare(fr, refs, want)
    out = tmp_path / "rows.tsv"
    fr.write(out)
    assert out.read_bytes() == want[3]
    if device_write:
        out2 = tmp_path / "file.tsv"
        assert B().bam_to_fragments(path, str(out2), max_window_bytes=max_window_bytes, **params) == want[2]
        assert out2.read_bytes() == want[3]
    return fr, want


def check(tmp_path, refs, records, cuts=None, block=0xFF00, name="t.bam", **kw):
    p = str(tmp_path / name)
    F.write_bam(p, refs, records, cuts=cuts, block=block)
    return check_file(p, refs, records, tmp_path, **kw)


# ---- the rule -----------------------------------------------------------------------------------------------------------
def test_the_worked_example(tmp_path):
    fr, want = check(tmp_path, EXAMPLE_REFS, example_records())
    assert want[3] == EXAMPLE_TEXT and fr.stats == EXAMPLE_STATS
    p = str(tmp_path / "t.bam")
    assert B().bam_to_fragments(p, str(tmp_path / "e.tsv.gz")) == EXAMPLE_STATS
    assert gzip.decompress((tmp_path / "e.tsv.gz").read_bytes()) == EXAMPLE_TEXT
    st = B().last_stages()
    assert st["records"] == 12 and st["windows"] >= 1 and st["call_s"] > 0


@pytest.mark.parametrize("reason,record", [
    ("unplaced", F.rec(ref_id=-1, pos=-1, flag=0x4)), ("flag", pr(0, 10, 100, flag=0x41)), ("flag", pr(0, 10, 100, flag=99 | 0x800)),
    ("mapq", pr(0, 10, 100, mapq=29)), ("mate_ref", pr(0, 10, 100, next_ref=1)), ("not_leftmost", pr(0, 10, 0)),
    ("not_leftmost", pr(0, 200, -100, flag=147)), ("too_long", pr(0, 10, 2001)), ("no_barcode", pr(0, 10, 100, cb=None)),
    ("empty", pr(0, 10, 9)), ("empty", pr(1, 49_998, 14)), ("kept_pairs", pr(0, 10, 2000)), ("kept_pairs", pr(0, 10, 10)),
    ("kept_pairs", pr(0, 10, 100, mapq=255)), ("kept_pairs", pr(0, 10, 100, mapq=30))])
def test_each_reason_alone(tmp_path, reason, record):
    fr, _ = check(tmp_path, REFS, [record], device_write=False)
    assert fr.stats[reason] == 1 and fr.stats["records"] == 1


def test_the_first_reason_that_applies_is_counted(tmp_path):
    recs = [pr(0, 10, 0, flag=0x41, mapq=3, next_ref=1, cb=None),  # flag, though every later step would drop it too
            pr(0, 10, 3000, mapq=3, next_ref=1), pr(0, 10, -5, next_ref=1), pr(0, 10, 3000, cb=None), pr(0, 10, 3, cb=None)]
    fr, _ = check(tmp_path, REFS, recs)
    assert [fr.stats[k] for k in ("flag", "mapq", "mate_ref", "too_long", "no_barcode", "empty")] == [1, 1, 1, 1, 1, 0]


def test_other_parameters(tmp_path):
    recs = sort_records([pr(0, 100 + i, 150, flag=f, mapq=q) for i, (f, q) in enumerate(
        [(99, 60), (99 | 0x400, 60), (99 | 0x400, 60), (0x41, 60), (0x1, 0), (0x0, 5), (99 | 0x100, 60), (99 | 0x200, 30), (163, 1)])])
    recs += [pr(0, 300, 2500), pr(0, 3, 40), pr(0, 3, 40), pr(1, 49_900, 120)]
    p = str(tmp_path / "p.bam")
    F.write_bam(p, REFS, recs)
    for params in (dict(exclude_flags=0xF0C), dict(require_flags=0x1, exclude_flags=0x400), dict(require_flags=0, exclude_flags=0), dict(min_mapq=0),
                   dict(min_mapq=0, require_flags=0), dict(shift=(0, 0)), dict(shift=(-50, 0)), dict(shift=(-50, 30)), dict(shift=(200, -200)),
                   dict(max_fragment_length=150), dict(max_fragment_length=149), dict(max_fragment_length=1 << 40, shift=(-(1 << 31) + 1, (1 << 31) - 1))):
        fr, _ = check_file(p, REFS, recs, tmp_path, device_write=False, **params)
    fr, _ = check_file(p, REFS, recs, tmp_path, shift=(-50, 0))
    assert fr.start[0] == 0 and fr.count[0] == 2  # a negative left shift clamps at 0
    fr, _ = check_file(p, REFS, recs, tmp_path, exclude_flags=0xF0C)
    assert fr.stats["flag"] >= 2


# ---- aux layouts --------------------------------------------------------------------------------------------------------
def test_aux_layouts(tmp_path):
    every = b"".join(EVERY_TYPE)
    layouts = [F.aux_Z("CB", "FIRST-1") + every, every + F.aux_Z("CB", "LAST-1"), F.aux_Z("CB", "ALONE-1")]
    layouts += [b"".join(e for e in EVERY_TYPE if e[2:3] == b"B") + F.aux_Z("CB", "BEHIND-B")]
    layouts += [e + F.aux_Z("CB", "B-%d" % k) for k, e in enumerate(EVERY_TYPE) if e[2:3] == b"B"]
    layouts += [F.aux_H("XH", "00FF") + F.aux_Z("XZ", "CBZfake") + F.aux_Z("CB", "BEHIND-HZ")]
    layouts += [F.aux_A("CB", "x") + F.aux_Z("CB", "SECOND"), F.aux_int("CB", "i", 7), F.aux_Z("CB", "ONE") + F.aux_Z("CB", "TWO")]
    layouts += [F.aux_Z("CB", "") + F.aux_Z("CB", "AFTER-EMPTY"), F.aux_Z("CB", ""), every, b"", F.aux_Z("CR", "RAW") + F.aux_Z("CB", "CELL")]
    layouts += [F.aux_Z("CB", "x" * 300), F.aux_Z("CB", "A"), F.aux_Z("cb", "lower")]
    recs = [pr(0, 100 + k, 120, aux=a) for k, a in enumerate(layouts)]
    fr, want = check(tmp_path, REFS, recs)
    assert fr.stats["no_barcode"] == 7 and "x" * 300 in fr.barcodes and "ONE" in fr.barcodes and "TWO" not in fr.barcodes
    fr, _ = check(tmp_path, REFS, recs, barcode_tag="CR")
    assert fr.barcodes == ["RAW"] and fr.stats["kept_pairs"] == 1
    check(tmp_path, REFS, recs, max_window_bytes=64, block=70, name="small.bam")
    # nothing behind the entry that decides is looked at
    fr, _ = check(tmp_path, REFS, [pr(0, 100, 120, aux=F.aux_Z("CB", "OK") + b"XQ?")], name="behind.bam")
    assert fr.barcodes == ["OK"]


# ---- order --------------------------------------------------------------------------------------------------------------
def test_order_of_rows_and_barcodes(tmp_path):
    recs = [pr(0, 100, 200, cb=cb) for cb in (b"ACG", b"AC", b"AB", b"ACG", b"B", b"A")]
    recs += [pr(0, 100, 150, cb=b"Z"), pr(0, 100, 250, cb=b"A"), pr(0, 101, 10, cb=b"ACG")]
    recs += [pr(1, 5, 100, cb=b"ACG"), pr(1, 5, 100, cb=b"AB")]
    fr, _ = check(tmp_path, REFS, recs)
    assert fr.barcodes == ["A", "AB", "AC", "ACG", "B", "Z"]
    assert list(zip(fr.start.tolist(), fr.end.tolist(), fr.barcode.tolist()))[:7] == [(104, 245, 5), (104, 295, 0), (104, 295, 1), (104, 295, 2),
                                                                                    (104, 295, 3), (104, 295, 4), (104, 345, 0)]
    assert fr.ref.tolist()[-2:] == [1, 1] and fr.barcode.tolist()[-2:] == [1, 3]


def test_a_repeated_tuple_in_three_windows(tmp_path):
    """records of about 120 bytes in blocks of 90 and windows of 100: every record and its aux area straddles windows"""
    recs = []
    for k in range(12):
        recs += [pr(0, 500, 300, cb=b"ACGTACGTACGTACGT-1", l_seq=40)] if k % 5 == 0 else []
        recs += [pr(0, 500, 100 + k, cb=b"ACGTACGTACGTAC%02d-1" % k, l_seq=40)]
    assert 110 <= len(F.encode_record(recs[0])) <= 130
    fr, _ = check(tmp_path, REFS, recs, block=90, max_window_bytes=100)
    assert B().last_stages()["windows"] > 12
    assert fr.count.max() == 3 and fr.stats["kept_pairs"] == 15 and fr.stats["fragments"] == 13


def test_bgzf_cuts_inside_the_tag_and_the_value(tmp_path):
    recs = [pr(0, 100 + k, 150, aux=F.aux_int("NM", "i", k) + F.aux_Z("CB", "ACGTACGT-%d" % (k % 3))) for k in range(9)]
    head = len(F.R.encode_header(REFS))
    starts = np.cumsum([head] + [len(F.encode_record(r)) for r in recs])
    aux_at = [int(starts[k + 1]) - len(recs[k]["aux"]) for k in range(9)]
    cuts = sorted([aux_at[1] + 7 + 1,   # between the two tag bytes of CB
                   aux_at[2] + 7 + 2,   # between the tag and its type
                   aux_at[4] + 7 + 3 + 4,  # inside the barcode's value
                   aux_at[5] + 7 + 3 + 10,  # in front of the value's NUL
                   aux_at[6] + 2, int(starts[7]), int(starts[7]), int(starts[8]) + 2])  # a repeated offset: an empty block
    for mw in (None, 1, 120, 400):
        check(tmp_path, REFS, recs, cuts=cuts, max_window_bytes=mw, device_write=mw is None)


# ---- sizes --------------------------------------------------------------------------------------------------------------
def sized_records(n_rows, n_barcodes, seed=3):
    """n_rows distinct (position, barcode) tuples, a third of them twice, every pair with its rightmost mate"""
    rng = np.random.default_rng(seed)
    names = sorted({b"".join(rng.choice([b"A", b"C", b"G", b"T"], 12).tolist()) + b"-1" for _ in range(n_barcodes * 2)})[:n_barcodes]
    recs = []
    for i in range(n_rows):
        r = pr(i % 2, 1000 + 3 * (i // 2), 100 + int(rng.integers(0, 5)), cb=names[i % n_barcodes] if i >= n_barcodes else names[i])
        recs += [r, mate(r)] + ([dict(r, flag=r["flag"] | 0x400), mate(r)] if i % 3 == 0 else [])
    return sort_records(recs)


@pytest.mark.parametrize("n_rows,n_barcodes", [(0, 1), (1, 1), (64, 2), (65, 1), (256, 2), (257, 300), (1025, 300)])
def test_sizes(tmp_path, n_rows, n_barcodes):
    recs = sized_records(n_rows, n_barcodes)
    fr, _ = check(tmp_path, REFS, recs, max_window_bytes=30_000, block=20_000)
    assert len(fr) == n_rows and len(fr.barcodes) == min(n_barcodes, n_rows) and fr.stats["kept_pairs"] == n_rows + (n_rows + 2) // 3
    if n_rows == 0:
        assert (tmp_path / "file.tsv").read_bytes() == b""
        p = str(tmp_path / "empty.bam")
        F.write_bam(p, REFS, [])
        check_file(p, REFS, [], tmp_path)


# Every kernel of csrc/bam_frag.hip is a grid-stride loop launched through launch_over (csrc/pipeline.h), whose grid
# GTARS_GRID_CAP clips: the test below runs each of them past the first trip of its loop.  tests/test_bam_frag_cpu.py holds
# this table to the kernels the file defines -- a new kernel there comes with a row here.  kernel -> what makes it loop twice
K26_KERNELS = {
    "k_bam_frag_rows": "2734 records in one window", "k_bam_frag_append": "2734 records in one window",
    "k_bam_frag_runs": "1367 kept rows", "k_bam_frag_fix_runs": "1367 kept rows under 4 hash bits: every run of equal hash is mixed",
    "k_bam_frag_reps": "1367 kept rows", "k_bam_frag_rep_bytes": "300 distinct barcodes", "k_bam_frag_ids": "1367 kept rows",
    "k_bam_frag_tuple_heads": "1367 kept rows", "k_bam_frag_write": "1367 kept rows", "k_bam_frag_counts": "1025 output rows",
}


@pytest.mark.parametrize("cap", [1, 3])
def test_grid_stride_loops_take_more_than_one_turn(tmp_path, monkeypatch, cap):
    from gtars_amd._lib import lib

    recs = sized_records(1025, 300)
    assert len(recs) == 2734  # (cap 3 leaves k_bam_frag_rep_bytes, over 300 barcodes, at one trip; cap 1 does not)
    monkeypatch.setenv("GTARS_GRID_CAP", str(cap))  # (tests/conftest.py: the library takes a new snapshot of its switches)
    for bits in ("64", "4"):
        monkeypatch.setenv("GTARS_BAM_CB_HASH_BITS", bits)
        before = lib.gtars_debug_grid_clips()
        fr, _ = check(tmp_path, REFS, recs, device_write=False)
        assert len(fr) == 1025 and fr.stats["kept_pairs"] == 1367
        assert lib.gtars_debug_grid_clips() - before >= len(K26_KERNELS) - 2  # (every launch over more than 256 * cap elements)


@pytest.mark.parametrize("bits", ["4", "1", "0"])
def test_the_result_does_not_depend_on_the_hash(tmp_path, monkeypatch, bits):
    """4 bits: 16 hash values for 300 barcodes, so every run of equal hash is mixed; 0 bits: all rows are ONE run"""
    recs = sized_records(600, 300)
    p = str(tmp_path / "h.bam")
    F.write_bam(p, REFS, recs)
    default, _ = check_file(p, REFS, recs, tmp_path, device_write=False)
    monkeypatch.setenv("GTARS_BAM_CB_HASH_BITS", bits)
    fr, _ = check_file(p, REFS, recs, tmp_path, device_write=False, max_window_bytes=20_000)
    assert fr.barcodes == default.barcodes and np.array_equal(fr.barcode, default.barcode) and np.array_equal(fr.count, default.count)


# ---- refusals -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["middle", "last"])
@pytest.mark.parametrize("bad", [b"XQ?abc", b"CBZno-nul", b"XBBi\xff\xff\xff\xff" + b"x" * 8, "l_seq"], ids=["type", "nul", "b-count", "aux-start"])
def test_malformed_aux_data_is_refused(tmp_path, where, bad):
    recs = [pr(0, 100 + k, 150, l_seq=40) for k in range(41)]
    at = 20 if where == "middle" else 40
    if bad != "l_seq":
        recs[at]["aux"] = bad
    stream = bytearray(F.bam_stream(REFS, recs))
    if bad == "l_seq":  # an l_seq that puts the aux start far beyond block_size
        off = len(F.R.encode_header(REFS)) + sum(len(F.encode_record(r)) for r in recs[:at])
        struct.pack_into("<I", stream, off + 4 + 16, 0x7FFFFFFF)
    else:
        with pytest.raises(F.Malformed):
            F.fragments_ref(REFS, recs)
    p = str(tmp_path / "bad.bam")
    with open(p, "wb") as f:
        f.write(F.R.bgzf_bytes(bytes(stream), block=300))
    for mw in (None, 600):
        with pytest.raises(ValueError, match="malformed aux data") as e:
            B().bam_to_fragments(p, str(tmp_path / "never.tsv"), max_window_bytes=mw)
        first, last = map(int, re.search(r"records (\d+) \.\. (\d+)", str(e.value)).groups())
        assert first <= at <= last and (mw is None or last - first < 12)
        assert not (tmp_path / "never.tsv").exists()
    with B().BamFile(p) as b:  # the record is dropped before the barcode step, or no barcode is looked for: nothing to refuse
        assert b.fragments(barcode_tag=None, sample="s").stats["kept_pairs"] == 41
        assert b.fragments(max_fragment_length=100).stats["too_long"] == 41
    check(tmp_path, EXAMPLE_REFS, example_records(), name="good.bam")


# ---- the fixtures, the fragment side, the command line ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["test_chr22_small.bam", "dummy.bam"])
def test_fixtures_without_a_barcode_tag(tmp_path, name):
    path = os.path.join(GOLDEN, name)
    refs, recs = F.read_bam(path)
    for params in (dict(barcode_tag=None, sample="s1"), dict(barcode_tag=None, sample="s1", require_flags=0, min_mapq=0, exclude_flags=0),
                   dict(barcode_tag="CB")):
        check_file(path, refs, recs, tmp_path, **params)
        check_file(path, refs, recs, tmp_path, max_window_bytes=100, device_write=False, **params)


def test_the_fragment_side_reads_the_written_file(tmp_path):
    from gtars_amd import scoring

    recs = sized_records(257, 40)
    p = str(tmp_path / "s.bam")
    F.write_bam(p, REFS, recs)
    peaks = tmp_path / "peaks.bed"
    peaks.write_text("".join("%s\t%d\t%d\n" % (c, s, s + 150) for c in ("chr1", "chr2") for s in range(900, 1500, 200)))
    for out in ("frags.tsv", "frags.tsv.gz"):
        stats = B().bam_to_fragments(p, str(tmp_path / out))
        m = scoring.barcode_count_matrix(str(tmp_path / out), str(peaks), keep_empty=True)
        assert len(m.barcodes) == stats["barcodes"] == 40 and m.shape == (40, 6)
        assert sorted(m.barcodes) == sorted(b.decode() for b in F.fragments_ref(REFS, recs)[1])


def test_the_command_line(tmp_path, capsys):
    from gtars_amd import cli

    p = str(tmp_path / "c.bam")
    F.write_bam(p, EXAMPLE_REFS, example_records())
    assert cli.main(["bam", "fragments", "--bam", p, "--output", str(tmp_path / "c.tsv")]) == 0
    assert (tmp_path / "c.tsv").read_bytes() == EXAMPLE_TEXT
    assert capsys.readouterr().out == "".join("%s\t%d\n" % (k, EXAMPLE_STATS[k]) for k in F.STATS)
    args = ["--no-barcode", "s1", "--min-mapq", "0", "--max-length", "250", "--shift", "0,0"]
    assert cli.main(["bam", "fragments", "--bam", p, "--output", str(tmp_path / "d.tsv.gz")] + args) == 0
    want = F.fragments_ref(EXAMPLE_REFS, example_records(), barcode_tag=None, sample="s1", min_mapq=0, max_fragment_length=250, shift=(0, 0))
    assert gzip.decompress((tmp_path / "d.tsv.gz").read_bytes()) == want[3]
    assert capsys.readouterr().out == "".join("%s\t%d\n" % (k, want[2][k]) for k in F.STATS)
    assert cli.main(["bam", "fragments", "--bam", p, "--output", str(tmp_path / "e.tsv"), "--barcode-tag", "CR"]) == 0
    assert (tmp_path / "e.tsv").read_bytes() == b""


# ---- random files -------------------------------------------------------------------------------------------------------
def random_file(rng):
    refs = [("ctg%d" % c, int(rng.integers(300, 5000))) for c in range(int(rng.integers(1, 5)))]
    tag = [b"CB", b"CR", b"XX"][int(rng.integers(0, 3))]
    pool = [bytes(rng.choice(list(b"ACGT"), int(rng.integers(1, 20))).tolist()) + b"-1" for _ in range(int(rng.integers(1, 30)))]
    recs = []
    for c, (_, length) in enumerate(refs):
        for pos in np.sort(rng.integers(-1, length, int(rng.integers(0, 120)))).tolist():
            aux = b"".join(EVERY_TYPE[int(k)] for k in rng.integers(0, len(EVERY_TYPE), int(rng.integers(0, 4))))
            kind = rng.random()
            if kind < 0.8:
                aux += F.aux_Z(tag, pool[int(rng.integers(0, len(pool)))])
            elif kind < 0.85:
                aux += F.aux_A(tag, "x") if kind < 0.83 else F.aux_Z(tag, "")
            aux += b"".join(EVERY_TYPE[int(k)] for k in rng.integers(0, len(EVERY_TYPE), int(rng.integers(0, 3))))
            if rng.random() < 0.05:
                aux += F.aux_Z(tag, b"LATE")
            flag = int(rng.choice([99, 99, 99, 99, 163, 147, 83, 99 | 0x400, 99 | 0x100, 99 | 0x800, 0x41, 0x1, 0x4 | 0x1, 97 | 0x8, 99 | 0x200]))
            tlen = int(rng.choice([int(rng.integers(1, 400)), int(rng.integers(1, 400)), int(rng.integers(-400, 3000)), 0, 2000, 2001]))
            rep = 1 + int(rng.random() < 0.15) * int(rng.integers(1, 4))
            recs += [pr(c, pos, tlen, flag=flag, mapq=int(rng.choice([0, 10, 29, 30, 31, 60, 60, 60, 255])), aux=aux,
                        next_ref=int(rng.integers(0, len(refs))) if rng.random() < 0.05 else None, l_seq=int(rng.integers(0, 30)))] * rep
    recs += [F.rec(ref_id=-1, pos=-1, flag=0x4 | 0x1, aux=F.aux_Z(tag, pool[0]))] * int(rng.integers(0, 3))
    size = len(F.bam_stream(refs, recs))
    cuts = sorted(int(x) for x in rng.integers(0, size, int(rng.integers(0, 6))))
    cuts += cuts[:1]
    params = dict(min_mapq=int(rng.choice([0, 30, 31])), max_fragment_length=int(rng.choice([100, 2000])),
                  shift=[(4, -5), (0, 0), (-50, 20), (10, -300)][int(rng.integers(0, 4))], require_flags=int(rng.choice([0x3, 0x1, 0])),
                  exclude_flags=int(rng.choice([0xB0C, 0xF0C, 0])))
    params.update(dict(barcode_tag=None, sample="bulk_%d" % size) if rng.random() < 0.15 else dict(barcode_tag=tag.decode()))
    return refs, recs, sorted(cuts), int(rng.choice([256, 1000, 0xFF00])), [None, 200, 1000, 5000][int(rng.integers(0, 4))], params


def test_forty_random_files(tmp_path):
    kept = rows = 0
    for seed in range(40):
        refs, recs, cuts, block, mw, params = random_file(np.random.default_rng(1000 + seed))
        try:
            fr, _ = check(tmp_path, refs, recs, cuts=cuts, block=block, max_window_bytes=mw, device_write=seed % 8 == 0, **params)
        except BaseException:
            print("seed", 1000 + seed, "block", block, "max_window_bytes", mw, "cuts", cuts, "params", params)
            raise
        kept += fr.stats["kept_pairs"]
        rows += len(fr)
    assert kept > rows > 500
