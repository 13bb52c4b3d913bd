"""The streaming uniwig (K24) without a device: the reference's known answers against the restatement
(tests/uniwig_stream_ref.py), the restatement against the closed form the device computes (written here in numpy, event
columns and all), the C++ parser against the restatement's, the single-member gzip rule, read_chrom_sizes, and the command
line up to the device call."""
import gzip
import io
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import uniwig_stream_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- the closed form, as csrc/uniwig_stream.hip computes it ---------------------------------------------------------------
def closed_form(cid, start, end, score, sizes_by_id, m, step, kind, max_gap):
    """-> (seg_cid, seg_first, seg_len, counts of the kept positions); segments of length 0 dropped"""
    cid, start, end, score = (np.asarray(x, dtype=np.int64) for x in (cid, start, end, score))
    if kind == "core":
        ws, we = start + 1, end - 1
        keep = we >= ws
        cid, ws, we, score = cid[keep], ws[keep], we[keep], score[keep]
    else:
        c = start + 1 if kind == "start" else end
        ws, we = np.maximum(1, c - m), c + m
    n = len(ws)
    empty = np.zeros(0, dtype=np.int64)
    if n == 0:
        return empty, empty, empty, empty
    head = np.r_[True, cid[1:] != cid[:-1]]
    M, binc, bx = np.empty(n, np.int64), np.empty(n, np.int64), np.zeros(n, np.int64)
    bounds = np.r_[np.flatnonzero(head), n]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        M[lo:hi] = np.maximum.accumulate(ws[lo:hi])
        binc[lo:hi] = np.maximum.accumulate(we[lo:hi])
        bx[lo + 1:hi] = binc[lo:hi - 1]
    dense = max_gap < 0
    flag = head.copy() if dense else head | ((M > bx + 1) & (M - bx - 1 > max_gap))
    seg = np.cumsum(flag) - 1
    heads = np.flatnonzero(flag)
    tails = np.r_[heads[1:] - 1, n - 1]
    seg_cid = cid[heads]
    first = np.ones(len(heads), np.int64) if dense else M[heads]
    last = binc[tails]
    if dense:
        last = np.maximum(last, np.asarray(sizes_by_id, dtype=np.int64)[seg_cid])
    length = np.maximum(last + 1 - first, 0)
    off = np.r_[0, np.cumsum(length)]
    live = (score > 0) & (we >= M)
    w = np.where(live, score, 0)
    A = off[seg] + M - first[seg]
    E = off[seg] + np.where(live, we + 1, M) - first[seg]
    assert (np.diff(A) >= 0).all() and A.min() >= 0 and E.max() <= off[-1] and (E >= A).all()
    d = np.zeros(off[-1] + 1, dtype=np.int64)
    np.add.at(d, A, w)
    np.add.at(d, E, -w)
    counts = np.cumsum(d[:-1]) & 0xFFFFFFFF
    pos = np.concatenate([np.arange(f, f + ln) for f, ln in zip(first, length)]) if len(first) else empty
    counts = counts[(pos - 1) % step == 0] if step > 1 else counts
    nz = length > 0
    return seg_cid[nz], first[nz], length[nz], counts


def closed_form_records(names, rows, sizes, m, step, kind, max_gap):
    ids = {}
    cid = [ids.setdefault(r[0], len(ids)) for r in rows]
    order = list(ids)
    sizes_by_id = [sizes.get(nme, 0) for nme in order]
    sc, sf, sl, counts = closed_form(cid, [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows], sizes_by_id, m, step, kind,
                                     max_gap)
    out, k = [], 0
    for c, f, ln in zip(sc.tolist(), sf.tolist(), sl.tolist()):
        for p in range(f, f + ln):
            if step <= 1 or (p - 1) % step == 0:
                out.append((order[c], p, int(counts[k])))
                k += 1
    assert k == len(counts)
    return out


def random_rows(rng, n_rows):
    names = ["chr1", "chr2", "chrX"]
    rows = []
    name = rng.choice(names)
    base = rng.randrange(0, 30)
    for _ in range(n_rows):
        if rng.random() < 0.15:
            name = rng.choice(names)  # (may be the same name again, or one that was there before: a returning name)
            base = rng.randrange(0, 30)
        if rng.random() < 0.7:
            base += rng.randrange(0, 9)  # mostly ascending
        else:
            base = max(0, base - rng.randrange(0, 25))  # unsorted
        start = base
        end = start + rng.choice([0, 0, 1, 2, 3, 7, 15]) - (1 if rng.random() < 0.05 else 0)
        end = max(end, 0)
        score = rng.choice([1, 1, 1, 0, 2, 5, 100])
        rows.append((name, start, end, score))
    return rows


def test_restatement_equals_the_closed_form_on_random_inputs():
    rng = random.Random(24)
    n_cases = 0
    for _ in range(2500):
        rows = random_rows(rng, rng.randrange(0, 14))
        kind = rng.choice(["start", "end", "core"])
        m = 0 if kind == "core" and rng.random() < 0.5 else rng.choice([0, 1, 2, 5])
        step = rng.choice([1, 1, 2, 3])
        max_gap = rng.choice([-1, 0, 1, 3, 10])
        sizes = {nme: rng.choice([0, 5, 40, 90]) for nme in ("chr1", "chrX") if rng.random() < 0.7}
        want = R.run_rows(rows, m, step, kind, sizes, max_gap)
        got = closed_form_records(None, rows, sizes, m, step, kind, max_gap)
        assert got == want, (rows, kind, m, step, max_gap, sizes)
        n_cases += 1
    assert n_cases == 2500


def test_closed_form_wraps_at_two_to_the_32():
    rows = [("chr1", 10, 20, (1 << 31) - 1)] * 3
    want = R.run_rows(rows, 0, 1, "start", {}, 0)
    assert want == [("chr1", 11, (3 * ((1 << 31) - 1)) & 0xFFFFFFFF)]
    assert closed_form_records(None, rows, {}, 0, 1, "start", 0) == want


# ---- the reference's known answers (stream.rs:629-1146) against the restatement ----------------------------------------------
DUMMY = b"chr1\t2\t6\nchr1\t4\t7\nchr1\t5\t9\nchr1\t7\t12\n"


def _nz(records):
    return [r for r in records if r[2] > 0]


def test_known_answers_single_reads_and_count_types():
    nz = _nz(R.run_processor(b"chr1\t100\t200\n", 0, 1, "start", {}))
    assert nz == [("chr1", 101, 1)]
    nz = _nz(R.run_processor(b"chr1\t10\t200\n", 5, 1, "start", {}))
    assert [r[1] for r in nz] == list(range(6, 17)) and all(r[2] == 1 for r in nz)
    by_pos = {r[1]: r[2] for r in R.run_processor(b"chr1\t10\t20\nchr1\t12\t25\n", 2, 1, "start", {})}
    assert (by_pos[11], by_pos[13], by_pos[9], by_pos[15]) == (2, 2, 1, 1)
    nz = _nz(R.run_processor(b"chr1\t10\t15\n", 0, 1, "core", {}))
    assert [r[1] for r in nz] == [11, 12, 13, 14]
    nz = _nz(R.run_processor(b"chr1\t10\t15\n", 2, 1, "end", {}))
    assert [r[1] for r in nz] == [13, 14, 15, 16, 17]
    assert _nz(R.run_processor(b"chr1\t10\t20\tpeak1\t3\n", 0, 1, "start", {}))[0][2] == 3
    assert R.run_processor(b"", 1, 1, "start", {}) == []
    bed = b"# comment line\ntrack name=test\nbrowser position chr1:1-100\nchr1\t10\t20\n"
    assert _nz(R.run_processor(bed, 0, 1, "start", {})) == [("chr1", 11, 1)]


def test_known_answers_transitions_steps_and_clamps():
    recs = R.run_processor(b"chr1\t10\t20\nchr2\t10\t20\n", 0, 1, "start", {})
    assert recs == [("chr1", 11, 1), ("chr2", 11, 1)]
    recs = R.run_processor(b"chr1\t0\t10\n", 3, 2, "start", {})
    assert recs and all((r[1] - 1) % 2 == 0 for r in recs) and [r[1] for r in recs] == [1, 3]
    recs = R.run_processor(b"chr1\t0\t10\n", 5, 1, "start", {})
    assert recs[0][1] == 1 and all(r[1] >= 1 for r in recs)
    bed = b"chr11 \t10\t50\nchr11\t20\t76\nchr12\t769\t2395\nchr13\t771\t3000\nchr14\t800\t2900\nchr21\t1\t30\nchr21\t2\t19\nchr21\t16\t31\n"
    assert {r[0] for r in R.run_processor(bed, 0, 1, "start", {})} == {"chr11", "chr12", "chr13", "chr14", "chr21"}


def test_known_answers_reference_fixtures():
    recs = R.run_processor(DUMMY, 1, 1, "start", {"chr1": 20})
    assert [r[1] for r in recs] == list(range(2, 10)) and [r[2] for r in recs] == [1, 1, 2, 2, 2, 2, 1, 1]
    recs = R.run_processor(DUMMY, 1, 1, "end", {"chr1": 20})
    assert [r[1] for r in recs] == list(range(5, 14)) and [r[2] for r in recs] == [1, 2, 2, 2, 1, 1, 1, 1, 1]
    recs = R.run_processor(DUMMY, 0, 1, "core", {"chr1": 20})
    assert [r[1] for r in recs] == list(range(3, 12)) and [r[2] for r in recs] == [1, 1, 2, 2, 1, 2, 1, 1, 1]


def test_known_answers_writers_and_pipeline():
    recs = [("chr1", 5, 3), ("chr1", 6, 2), ("chr1", 7, 1), ("chr2", 10, 5)]
    assert R.write_records_as_wig(recs) == b"fixedStep chrom=chr1 start=5 step=1\n3\n2\n1\nfixedStep chrom=chr2 start=10 step=1\n5\n"
    assert R.write_records_as_bedgraph(recs[:2]) == b"chr1\t4\t5\t3\nchr1\t5\t6\t2\n"
    bed = b"chr1\t10\t20\nchr1\t15\t25\n"
    recs = R.run_processor(bed, 1, 1, "start", {})
    text = R.uniwig_streaming(bed, {}, 1, 1, "start", "wig", 0)
    parsed, pos = [], 0
    for line in text.decode().splitlines():
        if line.startswith("fixedStep"):
            pos = int(line.split("start=")[1].split()[0])
        else:
            parsed.append(("chr1", pos, int(line)))
            pos += 1
    assert parsed == recs
    assert R.uniwig_streaming(gzip.compress(bed), {}, 1, 1, "start", "wig", 0) == text
    assert R.read_chrom_sizes("chr1\t248956422\nchr2\t242193529\n") == {"chr1": 248956422, "chr2": 242193529}


def test_known_answers_max_gap():
    pos = [r[1] for r in R.run_processor(b"chr1\t10\t20\nchr1\t30\t40\n", 0, 1, "start", {}, 0)]
    assert pos == [11, 31]
    bed = b"chr1\t10\t20\nchr1\t17\t25\n"
    assert [r[1] for r in R.run_processor(bed, 0, 1, "start", {}, 10)] == list(range(11, 19))
    assert [r[1] for r in R.run_processor(bed, 0, 1, "start", {}, 3)] == [11, 18]
    recs = R.run_processor(b"chr1\t5\t10\n", 0, 1, "start", {"chr1": 20}, -1)
    assert [r[1] for r in recs] == list(range(1, 21)) and [r[2] for r in recs] == [0] * 5 + [1] + [0] * 14
    recs = R.run_processor(b"chr1\t10\t20\nchr1\t30\t40\n", 0, 1, "start", {"chr1": 100}, (1 << 63) - 1)
    assert [r[1] for r in recs] == list(range(11, 32))
    assert [r[1] for r in R.run_processor(b"chr1\t10\t20\nchr1\t16\t25\n", 0, 1, "start", {}, 5)] == list(range(11, 18))
    assert [r[1] for r in R.run_processor(bed, 0, 1, "start", {}, 5)] == [11, 18]


# ---- the C++ parser ------------------------------------------------------------------------------------------------------------
CORNER_LINES = [
    b"chr1\t10\t20", b"chr1 10 20", b"  chr1\t10\t20  ", b"chr1\t+5\t7", b"chr1\t-5\t7", b"chr1\t5\t-0", b"chr1\t10\t20\tn\t7",
    b"chr1\t10\t20\tn\t-7", b"chr1\t10\t20\tn\t1.5", b"chr1\t10\t20\tn\t2147483647", b"chr1\t10\t20\tn\t2147483648", b"chr1\t10\t20\tn",
    b"chr1\t10\t20\tn\t+3\textra", b"", b"#comment", b" #not a comment", b"track name=x", b"tracker\t1\t2", b"browser x", b" browser",
    b"   ", b"\t", b"chr1\t10", b"chr1", b"chr1\tx\t20", b"chr1\t10\t2x", b"chr1\t\t", b"chr1\t2147483647\t2147483648",
    b"chr1\t-2147483648\t-2147483649", b"chr1\t+\t5", b"chr1\t-\t5", b"chr1\t1_0\t5", b"chr1\t10\t20\r", b"chr1\t10\t20\r\r",
    "chr1\u00a010\u00a020".encode(), "chr1\u200910\u300020".encode(), " chr1\t10\t20\u0085".encode(), "chr\u00e9\t1\t2".encode(),
    "chr1\t1\t2\t\u00e9\t4".encode(), b"chr1\x0b10\x0c20", b"chr1\t010\t0020", b"chr1\t00\t-00",
]


def _reference_parse(lines):
    rows = []
    for ln in lines:
        rec = R.parse_bed_line(ln.rstrip(b"\r\n"))
        if rec is not None:
            rows.append(rec)
    return rows


def _library_rows(data):
    import gtars_amd.uniwig as U

    names, cid, start, end, score = U.parse_stream_bed(data)
    return [(names[c], int(s), int(e), int(k)) for c, s, e, k in zip(cid, start, end, score)]


def test_parser_rules_line_by_line():
    import gtars_amd.uniwig as U

    for ln in CORNER_LINES:
        try:
            want = _reference_parse([ln])
        except ValueError as e:
            with pytest.raises(ValueError) as got:
                U.parse_stream_bed(ln + b"\n")
            assert str(e) in str(got.value), ln
            # a bad line anywhere fails the whole parse, without a trailing newline too
            with pytest.raises(ValueError):
                U.parse_stream_bed(b"chr1\t1\t2\n" + ln)
            continue
        assert _library_rows(ln + b"\n") == want, ln
        assert _library_rows(ln) == want, ln
        assert _library_rows(b"chrA\t1\t2\r\n" + ln + b"\r\nchrA\t3\t4") == [("chrA", 1, 2, 1)] + want + [("chrA", 3, 4, 1)], ln


def test_parser_whole_files(tmp_path):
    import gtars_amd.uniwig as U

    good = [ln for ln in CORNER_LINES if _try(ln)]
    data = b"\n".join(good) + b"\n"
    want = _reference_parse(good)
    assert _library_rows(data) == want
    assert _library_rows(io.BytesIO(data)) == want
    p = tmp_path / "x.bed"
    p.write_bytes(data)
    assert _library_rows(str(p)) == want
    names = U.parse_stream_bed(data)[0]
    assert names == list(dict.fromkeys(r[0] for r in want))  # first-seen order
    assert _library_rows(b"") == [] and _library_rows(b"\n\n#x\n") == []
    with pytest.raises(ValueError, match="UTF-8"):
        U.parse_stream_bed(b"chr1\t1\t2\n\xff\xfe\t1\t2\n")
    with pytest.raises(FileNotFoundError):
        U.parse_stream_bed(str(tmp_path / "missing.bed"))


def _try(ln):
    try:
        R.parse_bed_line(ln.rstrip(b"\r\n"))
        return True
    except ValueError:
        return False


def test_gzip_only_the_first_member_is_read(tmp_path):
    a, b = b"chr1\t10\t20\nchr1\t15\t25\tn\t4\n", b"chr2\t1\t2\n"
    two = gzip.compress(a) + gzip.compress(b)
    assert R.gunzip_first_member(two) == a
    assert _library_rows(two) == _reference_parse(a.split(b"\n"))
    assert _library_rows(gzip.compress(a) + b"trailing garbage") == _reference_parse(a.split(b"\n"))
    p = tmp_path / "two.bed.gz"
    p.write_bytes(two)
    assert _library_rows(str(p)) == _reference_parse(a.split(b"\n"))
    import gtars_amd.uniwig as U

    with pytest.raises(ValueError, match="gzip"):
        U.parse_stream_bed(gzip.compress(a * 50)[:-12])
    with pytest.raises(ValueError):
        U.parse_stream_bed(b"\x1f\x8b\x08\x00garbage that is no deflate stream")


def test_read_chrom_sizes(tmp_path):
    import gtars_amd.uniwig as U

    text = "chr1\t100\n# comment\n\n  chr2\t200\textra\r\nchr 3\t7\nchr1\t150\n"
    want = R.read_chrom_sizes(text)
    assert want == {"chr1": 150, "chr2": 200, "chr 3": 7}
    assert U.read_chrom_sizes(text.encode()) == want
    p = tmp_path / "g.chrom.sizes"
    p.write_text(text)
    assert U.read_chrom_sizes(str(p)) == want and U.read_chrom_sizes(io.BytesIO(text.encode())) == want
    for bad in ("chr1 100\n", "chr1\t-5\n", "chr1\tx\n", "chr1\t4294967296\n", "chr1\t\n"):
        with pytest.raises(ValueError) as e_ref:
            R.read_chrom_sizes(bad)
        with pytest.raises(ValueError) as e_lib:
            U.read_chrom_sizes(bad.encode())
        assert str(e_ref.value) == str(e_lib.value)
    assert U.read_chrom_sizes(b"chr1\t4294967295\n") == {"chr1": 4294967295}


def test_writers_of_records():
    import gtars_amd.uniwig as U

    recs = [("chr1", 5, 3), ("chr1", 6, 2), ("chr1", 8, 1), ("chr2", 9, 5), ("chr2", 10, 4294967295), ("chr1", 11, 0)]
    out = io.BytesIO()
    U.write_records_as_wig(out, recs)
    assert out.getvalue() == R.write_records_as_wig(recs)
    out = io.BytesIO()
    U.write_records_as_bedgraph(out, recs)
    assert out.getvalue() == R.write_records_as_bedgraph(recs)


def test_arguments_are_checked_before_the_device():
    import gtars_amd.uniwig as U

    cols = (["chr1", "chr1"], [5, 9], [8, 12])
    with pytest.raises(ValueError, match="count type"):
        U.stream_counts(cols, None, 1, 1, "shift")
    with pytest.raises(ValueError, match="row 1"):
        U.stream_counts((["chr1", "chr1"], [5, -1], [8, 12]), None, 1, 1, "start")
    with pytest.raises(ValueError, match="row 0"):
        U.stream_counts((["chr1", "chr1"], [5, 9], [(1 << 31) - 6, 12]), None, 5, 1, "end")  # end + m + 1 = 2^31
    with pytest.raises(ValueError, match="row 1"):
        U.stream_counts((["a", "b"], [5, 9], [8, 12], [1, 1 << 31]), None, 1, 1, "core")
    with pytest.raises(ValueError, match="row 1"):
        U.stream_counts(b"chr1\t1\t2\nchr1\t-4\t2\n", None, 1, 1, "start")
    with pytest.raises(ValueError, match="smooth size"):
        U.stream_counts(cols, None, -1, 1, "start")
    with pytest.raises(ValueError, match="same length"):
        U.stream_counts((["chr1"], [5, 9], [8, 12]), None, 1, 1, "start")
    with pytest.raises(ValueError, match="output format"):
        U.uniwig_streaming(b"chr1\t1\t2\n", io.BytesIO(), None, 1, 1, "start", "npy", 0)
    with pytest.raises(ValueError, match="fewer than 3 fields"):
        U.uniwig_streaming(b"chr1\t1\t2\nchr1\t1\n", io.BytesIO(), None, 1, 1, "start", "wig", 0)
    assert U.CountType("core") is U.CountType.Core and U.OutputFormat("bedgraph") is U.OutputFormat.BedGraph
    # the batch path keeps its refusals
    with pytest.raises(ValueError, match="stepsize"):
        U.start_end_counts([5], 100, 5, stepsize=2)


@pytest.mark.skipif(__import__("gtars_amd").device_count() > 0, reason="needs a box WITHOUT a GPU")
def test_no_device_is_a_loud_error_not_a_fallback(tmp_path):
    import gtars_amd
    import gtars_amd.uniwig as U

    with pytest.raises(gtars_amd.NoDeviceError):
        U.stream_counts(DUMMY, None, 1, 1, "start")
    out = tmp_path / "o.wig"
    with pytest.raises(gtars_amd.NoDeviceError):
        U.uniwig_streaming(DUMMY, str(out), None, 1, 1, "core", "wig", 0)
    assert not out.exists()
    with pytest.raises(gtars_amd.NoDeviceError):
        U.StreamPlan(4096, 4096, 4096, 4096, 1, [20], 1, "start", 0)


def test_cli_argument_handling(tmp_path, capsys):
    from gtars_amd import cli

    bed = tmp_path / "a.bed"
    bed.write_bytes(DUMMY)
    base = ["uniwig", "--streaming", "-f", str(bed), "-m", "1", "-s", "1", "-l", str(tmp_path / "o")]
    assert cli.main(base + ["--counttype", "shift"]) == 1
    assert "Error: unknown count type 'shift' for streaming mode" in capsys.readouterr().err
    assert cli.main(base + ["--outputtype", "npy"]) == 1
    assert "Error: output type 'npy' not supported in streaming mode (use wig or bedgraph)" in capsys.readouterr().err
    assert cli.main(base + ["--outputtype", "bedGraph"]) == 1  # the batch path's spelling is not the streaming one's
    capsys.readouterr()
    assert cli.main(["uniwig", "--streaming", "-f", str(bed), "-m", "1", "-s", "1"]) == 2  # no --fileheader, no --stdout
    assert "--fileheader" in capsys.readouterr().err
    assert cli.main(["uniwig", "--streaming", "-f", str(bed), "-l", str(tmp_path / "o")]) == 2
    capsys.readouterr()
    with pytest.raises(ValueError, match="fewer than 2 fields"):  # --chromref is read first, by the streaming reader
        sizes = tmp_path / "g.sizes"
        sizes.write_text("chr1 20\n")
        cli.main(base + ["-c", str(sizes)])
    with pytest.raises(SystemExit):
        cli.main(base + ["--dense", "many"])
    assert sorted(os.listdir(tmp_path)) == ["a.bed", "g.sizes"]
    # without --streaming the batch path still asks for its flags
    with pytest.raises(SystemExit):
        cli.main(["uniwig", "-f", str(bed), "-m", "1", "-s", "1", "-l", str(tmp_path / "o")])
    capsys.readouterr()


def test_cli_reaches_the_device_call_with_the_parsed_arguments(tmp_path, monkeypatch):
    from gtars_amd import cli
    import gtars_amd.uniwig as U

    calls = []

    def fake(source, output, chrom_sizes, smooth_size, step_size, count_type, output_format, max_gap):
        calls.append((source, output if isinstance(output, str) else "<stdout>", chrom_sizes, smooth_size, step_size, count_type,
                      output_format, max_gap))

    monkeypatch.setattr(U, "uniwig_streaming", fake)
    bed = tmp_path / "a.bed"
    bed.write_bytes(DUMMY)
    sizes = tmp_path / "g.sizes"
    sizes.write_text("chr1\t20\n")
    head = str(tmp_path / "o")
    assert cli.main(["uniwig", "--streaming", "-f", str(bed), "-c", str(sizes), "-m", "3", "-s", "2", "-l", head, "-y", "bg", "--dense",
                     "-1"]) == 0
    assert calls == [(str(bed), f"{head}_{k}.bedgraph", {"chr1": 20}, 3, 2, k, "bedgraph", -1) for k in ("start", "end", "core")]
    calls.clear()
    # stdin, stdout, all types, the defaults: sparse, wig, no sizes
    import argparse

    ns = argparse.Namespace(chromref=None, counttype="all", smoothsize=1, stepsize=1, outputtype="wig", stdout=True, fileheader=None,
                            file="-", dense=0)
    sink = io.BytesIO()
    assert cli.run_uniwig_streaming(ns, stdin=io.BytesIO(DUMMY), stdout=sink) == 0
    assert calls == [(DUMMY, "<stdout>", {}, 1, 1, k, "wig", 0) for k in ("start", "end", "core")]
    assert sink.getvalue() == b"# count_type=start\n# count_type=end\n# count_type=core\n"
    calls.clear()
    ns.counttype, ns.file = "end", None
    sink = io.BytesIO()
    assert cli.run_uniwig_streaming(ns, stdin=io.BytesIO(DUMMY), stdout=sink) == 0
    assert calls == [(DUMMY, "<stdout>", {}, 1, 1, "end", "wig", 0)] and sink.getvalue() == b""


def test_host_code_under_the_sanitizers(tmp_path):
    """tests/soak/uniwig_stream_host_check.cpp, built with AddressSanitizer + UBSan: the parser header on the corner lines --
    every line alone in an exactly sized heap block, with and without its newline, every prefix of the joined text, and the
    gzip forms -- against the restatement's rows and messages."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "uniwig_stream_host_check"
    src = os.path.join(HERE, "soak", "uniwig_stream_host_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o",
                            str(exe), src, "-lz"], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("the host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    cases = []
    joined = b"\n".join(ln for ln in CORNER_LINES if _try(ln)) + b"\n"
    inputs = [ln for ln in CORNER_LINES] + [ln + b"\n" for ln in CORNER_LINES] + [joined[:k] for k in range(0, len(joined), 7)]
    inputs += [gzip.compress(joined), gzip.compress(joined) + gzip.compress(b"chrZ\t1\t2\n"), gzip.compress(joined)[:-9], b"\x1f\x8b"]
    for data in inputs:
        try:
            plain = R.gunzip_first_member(data) if data[:2] == b"\x1f\x8b" else data
            plain.decode("utf-8")
            rows = _reference_parse(R.split_lines(plain))
            want = "ok " + " ".join(f"{r[0].encode().hex()}:{r[1]}:{r[2]}:{r[3]}" for r in rows)
        except UnicodeDecodeError:
            want = "err *"
        except ValueError as e:
            want = "err *" if data[:2] == b"\x1f\x8b" else "err " + str(e).encode().hex()
        cases.append(f"{data.hex() or '-'}\t{want.strip()}")
    (tmp_path / "cases.txt").write_text("\n".join(cases) + "\n")
    run = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert f"{len(cases)} cases" in run.stdout
