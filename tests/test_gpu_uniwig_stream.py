"""The streaming uniwig on the device (gtars_amd.uniwig.stream_counts, K24) against the statement-by-statement restatement
of the reference's processor (tests/uniwig_stream_ref.py).  Records, segments and bytes are compared exactly; every input
is tiny."""
import io
import os
import random

import numpy as np
import pytest

import uniwig_stream_ref as R

pytestmark = pytest.mark.gpu

TILE = 4096  # COV_TILE of cov_tile.h: compacted positions per LDS tile, and per workgroup span at these sizes
I31 = (1 << 31) - 1


def _columns(rows):
    return [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows]


def _segments_of(records):
    """(chrom, first, length) of the maximal stretches of consecutive positions of one chromosome (step 1)"""
    out = []
    for chrom, pos, _ in records:
        if out and out[-1][0] == chrom and out[-1][1] + out[-1][2] == pos:
            out[-1][2] += 1
        else:
            out.append([chrom, pos, 1])
    return [tuple(s) for s in out]


def check(rows, m=0, step=1, kind="start", max_gap=0, sizes=None, max_device_bytes=0, segments=True):
    import gtars_amd.uniwig as U

    sizes = sizes or {}
    want = R.run_rows(rows, m, step, kind, sizes, max_gap)
    track = U.stream_counts(_columns(rows), sizes, m, step, kind, max_gap, max_device_bytes)
    assert track.counts.dtype == np.uint32
    got = list(track.records())
    assert len(got) == len(want)
    assert got == want
    if segments and step == 1:
        have = [(track.chroms[c], f, ln) for c, f, ln in zip(track.seg_chrom.tolist(), track.seg_first.tolist(), track.seg_len.tolist())]
        assert have == _segments_of(want)
    return track, want


def _pile(rng, n, lo, span, max_w, scores=(1, 1, 2, 5, 0)):
    """n rows of one chromosome with ascending starts"""
    starts = sorted(rng.randrange(lo, lo + span) for _ in range(n))
    return [("chr1", s, s + rng.randrange(1, max_w), rng.choice(scores)) for s in starts]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
@pytest.mark.parametrize("kind", ["start", "end", "core"])
def test_rows_per_run(n, kind):
    rng = random.Random(n)
    rows = _pile(rng, n, 5, 3 * n + 10, 40)
    rows += [("chr2", s, e, k) for _, s, e, k in _pile(rng, n, 0, 3 * n + 10, 40)]
    rows += [("chr1", s, e, k) for _, s, e, k in _pile(rng, max(n // 2, 1), 100, 50, 9)]  # chr1 comes back
    check(rows, 3, 1, kind, 2)


@pytest.mark.parametrize("length", [4095, 4096, 4097, 8193])
def test_compacted_lengths(length):
    rng = random.Random(length)
    rows = [("chr1", 0, length + 1, 3)] + _pile(rng, 200, 1, length - 50, 45)  # core: [1, length] and what lies inside it
    track, _ = check(rows, 0, 1, "core", 0)
    assert len(track.counts) == length and track.seg_len.tolist() == [length]


@pytest.mark.parametrize("first_len", [1000, TILE, TILE + 1, 2 * TILE - 1])
def test_segment_boundary_inside_a_tile_and_on_a_tile_boundary(first_len):
    rng = random.Random(first_len)
    rows = [("chr1", 0, first_len + 1, 2)] + _pile(rng, 100, 1, first_len - 60, 50)
    rows += [("chr1", first_len + 500, first_len + 500 + 3000, 7)] + _pile(rng, 100, first_len + 600, 2000, 50)
    track, _ = check(rows, 0, 1, "core", 0)
    assert track.seg_len.tolist()[0] == first_len and len(track.seg_len) == 2


def test_close_on_a_spans_first_position_and_one_past_a_segments_end():
    # core windows [1, TILE], closing at compacted index TILE = the second workgroup's first position, inside a segment
    # of 2 * TILE + 5 positions; the longest row closes one past the segment's end, on the next segment's first slot
    rows = [("chr1", 0, 2 * TILE + 6, 1), ("chr1", 0, TILE + 1, 4), ("chr1", 0, TILE + 1, 9), ("chr1", TILE - 1, TILE + 1, 2),
            ("chr1", TILE, TILE + 2, 3), ("chr1", 3 * TILE, 3 * TILE + 10, 5), ("chr2", 7, 20, 1)]
    track, want = check(rows, 0, 1, "core", 0)
    assert track.seg_len.tolist() == [2 * TILE + 5, 9, 12]
    by_pos = {(c, p): k for c, p, k in want}
    assert by_pos[("chr1", TILE)] == 1 + 4 + 9 + 2 and by_pos[("chr1", TILE + 1)] == 1 + 3 and by_pos[("chr1", 3 * TILE + 1)] == 5


@pytest.mark.parametrize("n", [70, 300])
def test_equal_opens_with_mixed_scores(n):
    """one position opened n times: the wave collapse (70: a full wave and a part of one) and a second chunk round (300)"""
    rng = random.Random(n)
    rows = [("chr1", 50, 60 + rng.randrange(0, 30), rng.choice([1, 2, 3, 0, 1000, 65536])) for _ in range(n)]
    rows += [("chr1", 50, 60, 7)] * n  # and n equal closes
    rows += _pile(rng, 40, 51, 30, 10)
    for kind in ("start", "core"):
        check(rows, 4, 1, kind, 0)


def test_score_zero_rows():
    rows = [("chr1", 10, 20, 0), ("chr1", 12, 30, 2), ("chr1", 100, 110, 0), ("chr1", 300, 310, 0), ("chr1", 305, 320, 0), ("chr2", 5, 9, 0)]
    _, want = check(rows, 2, 1, "start", 0)
    assert any(k == 0 for _, _, k in want)  # a score 0 row adds nothing but extends the emitted range
    check(rows, 0, 1, "core", 10)
    check(rows, 1, 1, "end", -1, {"chr1": 400})


def test_counts_wrap_at_two_to_the_32():
    rows = [("chr1", 10, 20, I31)] * 3 + [("chr1", 11, 20, 5)]
    _, want = check(rows, 0, 1, "start", 0)
    assert want == [("chr1", 11, (3 * I31) & 0xFFFFFFFF), ("chr1", 12, 5)]
    check(rows, 3, 1, "start", 0)
    check(rows, 0, 1, "core", 0)


def test_unsorted_rows():
    rng = random.Random(9)
    desc = sorted(_pile(rng, 300, 0, 2000, 60), key=lambda r: -r[1])
    for kind in ("start", "end", "core"):
        check(desc, 5, 1, kind, 0)
        check(desc, 5, 1, kind, 10)
    # End on start-sorted overlapping rows: the ends do not ascend
    rows = [("chr1", s, s + w, k) for s, w, k in [(10, 500, 1), (20, 30, 2), (25, 400, 3), (30, 5, 1), (200, 20, 4), (210, 900, 1), (220, 2, 6)]]
    check(rows, 3, 1, "end", 0)
    check(rows, 0, 1, "end", 3)
    shuffled = _pile(rng, 500, 0, 5000, 80)
    rng.shuffle(shuffled)
    for kind in ("start", "end", "core"):
        check(shuffled, 2, 1, kind, 3)


def test_three_hundred_runs_with_returning_names():
    rng = random.Random(300)
    rows = []
    for r in range(300):
        name = f"chr{rng.randrange(1, 6)}"
        if rows and rows[-1][0] == name:
            name = "chrOther" if name != "chrOther" else "chr1"
        rows += [(name, s, e, k) for _, s, e, k in _pile(rng, rng.randrange(1, 6), rng.randrange(0, 400), 60, 25)]
    sizes = {"chr1": 500, "chr3": 10}
    for kind in ("start", "core"):
        track, _ = check(rows, 2, 1, kind, 0)
        check(rows, 2, 1, kind, -1, sizes)
    assert len(set(track.seg_chrom.tolist())) <= 6 and len(track.seg_first) >= 300


@pytest.mark.parametrize("max_gap", [-1, 0, 3, 10])
def test_gaps_of_exactly_max_gap_and_one_more(max_gap):
    g = max(max_gap, 0)
    # start track, m = 0: windows [11, 11] and [11 + gap + 1, ..]
    for gap in (g, g + 1):
        rows = [("chr1", 10, 20, 2), ("chr1", 10 + gap + 1, 40, 3), ("chr1", 10 + gap + 1 + 50, 90, 1)]
        track, want = check(rows, 0, 1, "start", max_gap)
        n_seg = len(track.seg_first)
        if max_gap < 0:
            assert n_seg == 1 and want[0][1] == 1
        else:
            assert n_seg == (2 if gap <= max_gap else 3)
        check(rows, 2, 1, "end", max_gap)
        check([(c, s, e + 5, k) for c, s, e, k in rows], 0, 1, "core", max_gap)


def test_dense_lead_and_tail():
    rows = [("chr1", 5, 10, 1), ("chr1", 30, 40, 2), ("chr2", 3, 9, 1), ("chr3", 0, 50, 4), ("chr1", 90, 95, 1)]
    sizes = {"chr1": 60, "chr3": 20}  # chr2 has none; chr3's windows reach past its size; the second chr1 run too
    for kind in ("start", "end", "core"):
        track, want = check(rows, 1, 1, kind, -1, sizes)
        assert track.seg_first.tolist() == [1, 1, 1, 1]
        check(rows, 1, 1, kind, -1, {})
    _, want = check(rows, 0, 1, "start", -1, sizes)
    assert [p for c, p, _ in want if c == "chr1"][:60] == list(range(1, 61))
    # End with end = 0 and m = 0: a window [1, 0] that holds nothing
    rows = [("chr1", 0, 0, 1), ("chr1", 0, 5, 1), ("chr2", 0, 0, 3), ("chr1", 0, 0, 1), ("chr1", 0, 12, 1)]
    for max_gap in (-1, 0, 3, 10):
        check(rows, 0, 1, "end", max_gap, {"chr2": 4}, segments=False)


@pytest.mark.parametrize("step", [2, 3])
def test_steps(step):
    rng = random.Random(step)
    rows = _pile(rng, 300, 0, 6000, 70) + [("chr2", s, e, k) for _, s, e, k in _pile(rng, 50, 7, 300, 20)]
    for kind in ("start", "end", "core"):
        check(rows, 3, step, kind, 0)
        check(rows, 3, step, kind, 10)
    check(rows, 3, step, "start", -1, {"chr1": 9000, "chr2": 100})
    check(rows, 3, step, "core", 0, max_device_bytes=1)
    check([("chr1", 0, 10, 1)], 3, step, "start", 0)
    assert [r[1] for r in R.run_rows([("chr1", 0, 10, 1)], 3, 2, "start", {}, 0)] == [1, 3]


@pytest.mark.parametrize("max_device_bytes", [1, 2 * TILE * 4])
def test_small_device_windows_cut_segments_and_tiles(max_device_bytes):
    rng = random.Random(77)
    rows = [("chr1", 0, 3 * TILE + 100, 2)] + _pile(rng, 400, 1, 3 * TILE, 300)  # one segment across four windows
    rows += [("chr2", s, e, k) for _, s, e, k in _pile(rng, 300, 0, 20000, 90)]   # and many short ones
    track, _ = check(rows, 0, 1, "core", 0, max_device_bytes=max_device_bytes)
    assert len(track.counts) > 4 * TILE
    check(rows, 25, 1, "start", 100, max_device_bytes=max_device_bytes)


def test_device_entry_on_resident_columns():
    import torch

    import gtars_amd.uniwig as U

    rng = random.Random(5)
    rows = [("chr1", 0, 12200, 1)] + _pile(rng, 500, 0, 12000, 120) + [("chr2", s, e, k) for _, s, e, k in _pile(rng, 100, 3, 900, 30)]
    names, start, end, score = _columns(rows)
    cid = [0 if nme == "chr1" else 1 for nme in names]
    dev = torch.device("cuda:0")
    d = [torch.tensor(x, dtype=torch.int32, device=dev) for x in (cid, start, end, score)]
    for kind, max_gap, sizes in (("core", 0, [0, 0]), ("start", 10, [0, 0]), ("end", -1, [15000, 0])):
        want = R.run_rows(rows, 4, 1, kind, {"chr1": sizes[0]} if sizes[0] else {}, max_gap)
        plan = U.StreamPlan(*(t.data_ptr() for t in d), len(rows), sizes, 4, kind, max_gap)
        assert plan.total == len(want) == int(plan.seg_off[-1])
        out = torch.full((plan.total + 8,), -1, dtype=torch.int32, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        plan.counts_device(0, plan.total, out.data_ptr(), stream)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        assert got[:plan.total].tolist() == [k for _, _, k in want] and (got[plan.total:] == 0xFFFFFFFF).all()
        # a window that starts inside a tile and ends inside another
        w0 = TILE - 37
        wl = min(TILE + 80, plan.total - w0)
        assert wl > 500
        out.fill_(-1)
        plan.counts_device(w0, wl, out.data_ptr(), stream)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        assert got[:wl].tolist() == [k for _, _, k in want[w0:w0 + wl]] and (got[wl:] == 0xFFFFFFFF).all()
        # the table: positions of the compacted indices
        pos = np.concatenate([np.arange(f, f + ln) for f, ln in zip(plan.seg_first.tolist(), plan.seg_len.tolist())])
        assert pos.tolist() == [p for _, p, _ in want]
        with pytest.raises(ValueError):
            plan.counts_device(plan.total, 1, out.data_ptr(), stream)
        plan.close()
    with pytest.raises(ValueError, match="row 3"):
        bad = torch.tensor([5, 6, 7, -1, 9], dtype=torch.int32, device=dev)
        ok = torch.tensor([5, 6, 7, 8, 9], dtype=torch.int32, device=dev)
        one = torch.ones(5, dtype=torch.int32, device=dev)
        U.StreamPlan(torch.zeros(5, dtype=torch.int32, device=dev).data_ptr(), bad.data_ptr(), ok.data_ptr(), one.data_ptr(), 5, [0], 1,
                     "start", 0)


BED = (b"# a comment\ntrack name=x\nchr1\t2\t6\nchr1 4 7 p 3\nchr1\t5\t9\tq\t-2\nchr1\t7\t12\tr\tx\n\nchr1\t300\t310\nchr2\t0\t4\t.\t7\n"
       b"chr1\t1\t3\nchr1\t20\t22\nchr9\t5\t5\n")


@pytest.mark.parametrize("fmt", ["wig", "bedgraph"])
def test_bytes_of_uniwig_streaming(tmp_path, fmt):
    import gzip

    import gtars_amd.uniwig as U

    sizes = {"chr1": 40, "chr2": 3}
    for kind in ("start", "end", "core"):
        for m, step, max_gap in ((1, 1, 0), (0, 1, 5), (2, 2, 0), (1, 3, -1), (0, 1, -1)):
            want = R.uniwig_streaming(BED, sizes, m, step, kind, fmt, max_gap)
            out = io.BytesIO()
            U.uniwig_streaming(BED, out, sizes, m, step, kind, fmt, max_gap)
            assert out.getvalue() == want, (kind, m, step, max_gap)
    # a path in, a path out, gzip with a second member that is not read
    src, dst = tmp_path / "in.bed.gz", tmp_path / "out.txt"
    src.write_bytes(gzip.compress(BED) + gzip.compress(b"chr5\t1\t2\n"))
    dst.write_bytes(b"old contents that must go")
    U.uniwig_streaming(str(src), str(dst), None, 1, 1, U.CountType.Core, U.OutputFormat.Wig if fmt == "wig" else U.OutputFormat.BedGraph, 0)
    assert dst.read_bytes() == R.uniwig_streaming(BED, {}, 1, 1, "core", fmt, 0)
    # an empty run between two runs of one name whose positions happen to continue: no header in between
    rows = b"chr1\t3\t9\nchr2\t0\t0\nchr1\t6\t10\n"
    out = io.BytesIO()
    U.uniwig_streaming(rows, out, None, 0, 1, "end", fmt, 0)
    assert out.getvalue() == R.uniwig_streaming(rows, {}, 0, 1, "end", fmt, 0)


def test_cli_end_to_end(tmp_path, capsysbinary):
    from gtars_amd import cli

    bed, sizes = tmp_path / "a.bed", tmp_path / "g.chrom.sizes"
    bed.write_bytes(BED)
    sizes.write_text("chr1\t40\nchr2\t3\n")
    head = str(tmp_path / "o")
    assert cli.main(["uniwig", "--streaming", "--file", str(bed), "--chromref", str(sizes), "--smoothsize", "1", "--stepsize", "1",
                     "--fileheader", head, "--dense", "-1"]) == 0
    assert sorted(os.listdir(tmp_path)) == ["a.bed", "g.chrom.sizes", "o_core.wig", "o_end.wig", "o_start.wig"]
    for kind in ("start", "end", "core"):
        assert (tmp_path / f"o_{kind}.wig").read_bytes() == R.uniwig_streaming(BED, {"chr1": 40, "chr2": 3}, 1, 1, kind, "wig", -1)
    capsysbinary.readouterr()
    assert cli.main(["uniwig", "--streaming", "-f", str(bed), "-m", "2", "-s", "2", "-u", "all", "-y", "bg", "--stdout"]) == 0
    want = b"".join(f"# count_type={k}\n".encode() + R.uniwig_streaming(BED, {}, 2, 2, k, "bedgraph", 0) for k in ("start", "end", "core"))
    assert capsysbinary.readouterr().out == want
