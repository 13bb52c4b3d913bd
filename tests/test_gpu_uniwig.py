"""Coverage tracks on the device (gtars_amd.uniwig, K11) against the plain-Python restatement of the reference's sweeps
(tests/uniwig_ref.py) and, where that is too slow, against the closed form both were checked to agree with
(tests/test_uniwig_cpu.py).  Exact equality everywhere."""
import json
import os
import shutil

import numpy as np
import pytest

import uniwig_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TILE = 4096  # COV_TILE of cov_tile.h: positions per LDS tile


def _pairs(v):
    return [(int(x), 1) for x in v]


def _rows(seed, n, span, max_w, pile=0):
    rng = np.random.default_rng(seed)
    start = rng.integers(0, span, n)
    width = rng.integers(1, max_w + 1, n)
    width[rng.random(n) < 0.1] = 1
    if pile:
        start[:pile] = span // 2 + rng.integers(0, 200, pile)
    start[-1] = 0
    return start.astype(np.uint32), (start + width).astype(np.uint32)


def _check_tracks_vs_restatement(start, end, chrom_size, m):
    import gtars_amd.uniwig as U

    s1, e = np.sort(start + np.uint32(1)), np.sort(end)
    for p in (s1, e):
        got, first = U.start_end_counts(p[::-1].copy(), chrom_size, m)  # any order: the device sorts
        want, pos = R.start_end_counts(_pairs(p), chrom_size, m, 1)
        assert got.dtype == np.uint32 and got.tolist() == want
        assert (first if want else None) == (pos[0] if want else None)
    got, first = U.core_counts(start + np.uint32(1), end, chrom_size)
    want, pos = R.core_counts(_pairs(s1), _pairs(e), chrom_size, 1)
    assert got.tolist() == want and (not want or first == pos[0])


@pytest.mark.parametrize("n,chrom_size,pile", [(1000, 60_000, 0), (10_000, 400_000, 3000), (100_000, 2_000_000, 20_000)])
def test_three_tracks_match_the_restatement(n, chrom_size, pile):
    start, end = _rows(n, n, chrom_size - 50, 400, pile)
    _check_tracks_vs_restatement(start, end, chrom_size, 25)


def _closed_form_by_windows(opens, closes, first, length, window=1 << 24):
    """count(pos) = #{a <= pos} - #{e <= pos} for pos = first .. first + length - 1, window by window: the count entering a
    window from two searches, a difference array of the window's events, its running sum"""
    a, e = np.sort(opens.astype(np.int64)), np.sort(closes.astype(np.int64))
    for w0 in range(first, first + length, window):
        w1 = min(w0 + window, first + length)
        ia0, ia1 = np.searchsorted(a, [w0, w1], side="left")
        ie0, ie1 = np.searchsorted(e, [w0, w1], side="left")
        d = np.bincount(a[ia0:ia1] - w0, minlength=w1 - w0) - np.bincount(e[ie0:ie1] - w0, minlength=w1 - w0)
        yield w0 - first, (int(ia0) - int(ie0) + np.cumsum(d)).astype(np.uint32)


def test_closed_form_at_ten_million_rows():
    import gtars_amd.uniwig as U

    n, chrom_size, m = 10_000_000, 250_000_000, 25
    rng = np.random.default_rng(2024)
    start = rng.integers(0, chrom_size - 2000, n).astype(np.uint32)
    end = start + rng.integers(1, 1500, n).astype(np.uint32)
    # the windowed closed form is the closed form of tests/uniwig_ref.py
    chk, f0 = R.closed_form_start_end(end[:2000], 300_000_000, m)
    assert f0 == int(end[:2000].min()) - m
    for off, part in _closed_form_by_windows(np.maximum(1, end[:2000].astype(np.int64) - m), end[:2000].astype(np.int64) + m + 1, f0,
                                             len(chk), window=1 << 26):
        assert np.array_equal(part, chk[off:off + len(part)])
    s1 = start + np.uint32(1)
    for kind, o, c in (("start", s1, None), ("end", end, None), ("core", s1, end)):
        if kind == "core":
            got, first = U.core_counts(o, c, chrom_size)
            a, e = o.astype(np.int64), c.astype(np.int64)
        else:
            got, first = U.start_end_counts(o, chrom_size, m)
            a, e = np.maximum(1, o.astype(np.int64) - m), o.astype(np.int64) + m + 1
        assert first == int(a.min()) and len(got) == max(chrom_size, int(a.max()) - 1) - first + 1
        for off, part in _closed_form_by_windows(a, e, first, len(got)):
            assert np.array_equal(got[off:off + len(part)], part), (kind, off)


def test_edge_cases():
    import gtars_amd.uniwig as U

    u = lambda *v: np.array(v, dtype=np.uint32)  # noqa: E731
    # n = 1
    _check_tracks_vs_restatement(u(10), u(30), 200, 5)
    # all rows identical: a pile-up of several chunks of events on one position
    _check_tracks_vs_restatement(np.full(3000, 77, dtype=np.uint32), np.full(3000, 300, dtype=np.uint32), 1000, 3)
    # a row at position 0, rows reaching and passing chrom_size, 1 bp rows
    _check_tracks_vs_restatement(u(0, 0, 5, 90, 99, 120, 150), u(1, 40, 6, 100, 130, 121, 400), 100, 7)
    # m = 0 through the calls (uniwig() itself writes nothing for it, as the reference)
    _check_tracks_vs_restatement(u(3, 3, 8, 50), u(9, 4, 20, 51), 80, 0)
    # a window that exceeds the chromosome on both sides
    _check_tracks_vs_restatement(u(10, 20, 30), u(15, 25, 45), 60, 500)
    # the first open lies past the chromosome: an empty track
    got, first = U.start_end_counts(u(500), 100, 5)
    assert len(got) == 0 and R.start_end_counts(_pairs([500]), 100, 5, 1) == ([], [])
    # no rows at all
    got, first = U.start_end_counts(u(), 100, 5)
    assert len(got) == 0 and first == 0


@pytest.mark.parametrize("m", [0, 3])
def test_events_on_tile_boundaries(m):
    """opens and closes exactly on the first and the last position of a tile (the track starts at its first open, so tile k
    covers positions first + k * TILE .. first + (k + 1) * TILE - 1)"""
    first = 5
    edges = []
    for k in (0, 1, 2, 5):
        edges += [first + k * TILE, first + (k + 1) * TILE - 1, first + (k + 1) * TILE]
    # start track: opens at p - m, closes at p + m + 1 -- put both on the edges
    p = sorted({e + m for e in edges} | {e - m - 1 for e in edges if e - m - 1 > first + m} | {first + m})
    p = np.array(p + p[:4], dtype=np.uint32)
    chrom_size = first + 7 * TILE + 11
    _check_tracks_vs_restatement(p - np.uint32(1), p + np.uint32(TILE), chrom_size, m)
    # core track: opens (start + 1) and closes (end) on the edges
    start = np.array([e - 1 for e in edges], dtype=np.uint32)
    for width in (1, TILE - 1, TILE, TILE + 1):
        _check_tracks_vs_restatement(start, start + np.uint32(width), chrom_size, m)
    # a chromosome that ends exactly on a tile boundary, one entry before and one behind it
    for size in (first + 2 * TILE - 2, first + 2 * TILE - 1, first + 2 * TILE):
        _check_tracks_vs_restatement(start[:3], start[:3] + np.uint32(9), size, m)


def test_windowed_production_equals_one_shot():
    import gtars_amd.uniwig as U

    start, end = _rows(9, 20_000, 300_000, 900, 4000)
    s1 = start + np.uint32(1)
    for budget in (1, 4 * TILE, 12 * TILE, 4 * 100_000):
        for p in (s1, end):
            a, fa = U.start_end_counts(p, 310_000, 25)
            b, fb = U.start_end_counts(p, 310_000, 25, max_device_bytes=budget)
            assert fa == fb and np.array_equal(a, b)
        a, fa = U.core_counts(s1, end, 310_000)
        b, fb = U.core_counts(s1, end, 310_000, max_device_bytes=budget)
        assert fa == fb and np.array_equal(a, b)


@pytest.mark.parametrize("n,chrom_size,pile", [(50, 3000, 0), (5000, 150_000, 1500), (40_000, 1_000_000, 0)])
def test_runs_and_nonzero_pairs_match_the_restatement(n, chrom_size, pile):
    import gtars_amd.uniwig as U

    start, end = _rows(31 + n, n, chrom_size + 500, 300, pile)  # some rows pass the chromosome
    s1, e = np.sort(start + np.uint32(1)), np.sort(end)
    m = 25
    for kind, opens, closes, res, s_pos in (
            ("start", s1, None, R.start_end_counts(_pairs(s1), chrom_size, m, 1), R.clamped_start_position_zero_pos(int(s1[0]), m)),
            ("end", e, None, R.start_end_counts(_pairs(e), chrom_size, m, 1), R.clamped_start_position(int(e[0]), m, 0)),
            ("core", s1, e, R.core_counts(_pairs(s1), _pairs(e), chrom_size, 1), R.clamped_start_position_zero_pos(int(s1[0]), 0))):
        got = U.compress_counts(kind, opens, closes, chrom_size, m, s_pos)
        want = R.compress_counts(res, s_pos)
        assert [x.tolist() for x in got] == [list(x) for x in want], kind
        assert all(x.dtype == np.uint32 for x in got)
        pos, cnt = U.nonzero_counts(kind, opens, closes, chrom_size, m, 7)
        want_pairs = [(7 + i, c) for i, c in enumerate(res[0][:chrom_size]) if c > 0]
        assert list(zip(pos.tolist(), cnt.tolist())) == want_pairs, kind
    # a track that is one run
    got = U.compress_counts("start", np.array([4], dtype=np.uint32), None, 4, 9, 0)
    assert [x.tolist() for x in got] == [list(x) for x in R.compress_counts(R.start_end_counts([(4, 1)], 4, 9, 1), 0)]
    with pytest.raises(ValueError):  # nothing to compress: the reference reads entry 0
        U.compress_counts("start", np.array([50], dtype=np.uint32), None, 10, 2, 0)


def test_device_form_on_a_side_stream():
    import torch

    import gtars_amd.uniwig as U

    start, end = _rows(5, 30_000, 500_000, 700, 5000)
    s1, e = np.sort(start + np.uint32(1)), np.sort(end)
    dev = torch.device("cuda:0")
    side = torch.cuda.Stream(device=dev)
    d_s = torch.from_numpy(s1.view(np.int32)).to(dev)
    d_e = torch.from_numpy(e.view(np.int32)).to(dev)
    torch.cuda.synchronize()
    for kind, o, c, m in (("start", d_s, None, 25), ("end", d_e, None, 25), ("core", d_s, d_e, 0)):
        host_o = s1 if o is d_s else e
        first, length = U.track_extent(kind, host_o, e if c is not None else None, 510_000, m)
        want = U._track(kind, host_o, e if c is not None else None, 510_000, m)[0]
        # the whole track, and a window that starts and ends inside tiles
        for w0, wl in ((first, length), (first + 3 * TILE + 17, 5 * TILE + 100)):
            with torch.cuda.stream(side):
                out = torch.full((wl + 8,), -1, dtype=torch.int32, device=dev)
                U.counts_device(kind, o.data_ptr(), c.data_ptr() if c is not None else 0, len(s1), m, w0, wl, out.data_ptr(),
                                side.cuda_stream)
            side.synchronize()
            got = out.cpu().numpy().view(np.uint32)
            assert np.array_equal(got[:wl], want[w0 - first:w0 - first + wl]), (kind, w0)
            assert (got[wl:] == 0xFFFFFFFF).all()  # nothing behind the window is written
    with pytest.raises(ValueError, match="aligned"):
        U.counts_device("start", d_s.data_ptr(), 0, len(s1), 25, 1, 64, d_e.data_ptr() + 4, side.cuda_stream)


def _truncated_sizes(bed, sizes_path, m, tmp_path):
    """The plain-Python sweeps cannot walk hg38's chromosomes (5.4e8 positions per track).  Behind the last window close a
    sweep has an empty queue and its count stays 0 (tests/test_uniwig_cpu.py checks the restatement for it), so the reference's
    files for the full sizes are its files for sizes cut behind the last event, followed by zero entries."""
    sizes = R.read_chromosome_sizes(sizes_path)
    cut = {}
    for name, starts, ends in R.create_chrom_vec_default_score(bed):
        if name in sizes:
            cut[name] = min(sizes[name], max(cut.get(name, 0), max(x[0] for x in ends) + m + 64))
    path = tmp_path / "cut.chrom.sizes"
    path.write_text("".join(f"{k}\t{v}\n" for k, v in cut.items()))
    return sizes, cut, str(path)


@pytest.mark.parametrize("output_type", ["bedGraph", "npy", "wig"])
def test_uniwig_end_to_end_on_the_golden_bed(output_type, tmp_path):
    import gtars_amd.uniwig as U

    bed = os.path.join(GOLDEN, "test_sorted_small.bed")
    sizes_path = os.path.join(GOLDEN, "hg38.chrom.sizes")
    m = 5
    sizes, cut, cut_path = _truncated_sizes(bed, sizes_path, m, tmp_path)
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    chroms = U.uniwig(bed, sizes_path, m, output_prefix=str(a / "t"), output_type=output_type)
    R.uniwig_main(["start", "end", "core"], m, bed, cut_path, str(b / "t"), output_type)
    assert chroms == [c[0] for c in R.get_final_chromosomes(bed, sizes)]
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and os.listdir(a)
    for f in sorted(os.listdir(a)):
        if output_type == "bedGraph":
            # the closing run of every chromosome reaches to the end of the track: its end moves with the size
            want = [ln.split("\t") for ln in (b / f).read_text().splitlines()]
            for i, ln in enumerate(want):
                if i + 1 == len(want) or want[i + 1][0] != ln[0]:
                    assert ln[3] == "0"
                    ln[2] = str(int(ln[2]) + sizes[ln[0]] - cut[ln[0]])
            assert (a / f).read_text() == "".join("\t".join(ln) + "\n" for ln in want)
        elif f.endswith(".json"):
            want = json.loads((b / f).read_text())
            for k in want:
                want[k]["reported_chrom_size"] = sizes[k]
            assert json.loads((a / f).read_text()) == want
        elif output_type == "npy":
            chrom = f[1:].split("_")[0]
            with open(a / f, "rb") as fh:
                assert fh.read(8) == b"\x93NUMPY\x01\x00"
            got = np.load(str(a / f), mmap_mode="r")
            small = np.load(str(b / f))
            assert got.dtype == np.uint32 and len(got) == len(small) + sizes[chrom] - cut[chrom]
            assert np.array_equal(got[:len(small)], small) and not got[len(small):].any()
        else:
            got = (a / f).read_bytes()
            blocks = (b / f).read_bytes().split(b"fixedStep")[1:]
            at = 0
            for blk in blocks:
                chrom = blk.split(b"chrom=")[1].split(b" ")[0].decode()
                want = b"fixedStep" + blk
                assert got[at:at + len(want)] == want
                at += len(want)
                extra = sizes[chrom] - cut[chrom]
                assert got[at:at + 2 * extra] == b"0\n" * extra
                at += 2 * extra
            assert at == len(got)
    shutil.rmtree(a)


def test_uniwig_variable_step_wig(tmp_path):
    import gtars_amd.uniwig as U

    bed = os.path.join(GOLDEN, "test_sorted_small.bed")
    sizes_path = os.path.join(GOLDEN, "hg38.chrom.sizes")
    sizes, cut, cut_path = _truncated_sizes(bed, sizes_path, 5, tmp_path)
    U.uniwig(bed, sizes_path, 5, output_prefix=str(tmp_path / "a"), output_type="wig", wig_variable=True)
    R.uniwig_main(["start", "end", "core"], 5, bed, cut_path, str(tmp_path / "b"), "wig", wigstep="variable")
    for kind in ("start", "end", "core"):  # the zero tail adds no line
        assert (tmp_path / f"a_{kind}.wig").read_bytes() == (tmp_path / f"b_{kind}.wig").read_bytes()
