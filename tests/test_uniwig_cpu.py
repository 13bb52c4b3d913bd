"""CPU-side checks of the coverage tracks (gtars_amd.uniwig, K11): the restatement of the reference's sweeps
(tests/uniwig_ref.py) against the closed form the device computes and against hand-computed literals; the BED reader, the
writers' bytes, the argument checks, the CLI, and the refusal to compute without a device."""
import gzip
import importlib
import json
import os
import shutil

import numpy as np
import pytest

import uniwig_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BEDS = ("test_sorted_small.bed", "test_unsorted_small.bed")


def _pairs(v):
    return [(int(x), 1) for x in v]


def _rows(rng, n, span, max_w, pile=0):
    """n rows with end > start: duplicates, 1 bp rows, rows at position 0 and (span may exceed the chromosome) rows that
    reach or pass chrom_size; `pile` of them inside one 50 bp window"""
    start = rng.integers(0, span, n)
    width = rng.integers(1, max_w + 1, n)
    width[rng.random(n) < 0.2] = 1
    if pile:
        start[:pile] = span // 3 + rng.integers(0, 50, pile)
    if n > 2:
        start[-1] = 0
        start[-2] = start[-3]  # a duplicate row
        width[-2] = width[-3]
    return start.astype(np.int64), (start + width).astype(np.int64)


# chrom_size, span of the starts, widest row, rows, rows in the pile-up
SHAPES = [(400, 380, 30, 60, 0), (300, 420, 40, 80, 0), (500, 480, 25, 200, 120), (50, 45, 8, 1, 0), (120, 100, 200, 40, 0),
          (200, 100, 5, 3, 0)]


@pytest.mark.parametrize("m", [0, 1, 5, 25])
@pytest.mark.parametrize("shape", SHAPES)
def test_start_end_sweep_is_the_closed_form(shape, m):
    chrom_size, span, max_w, n, pile = shape
    for seed in range(6):
        rng = np.random.default_rng(1000 * seed + m)
        start, end = _rows(rng, n, span, max_w, pile)
        for p in (np.sort(start + 1), np.sort(end)):
            counts, positions = R.start_end_counts(_pairs(p), chrom_size, m, 1)
            want, first = R.closed_form_start_end(p, chrom_size, m)
            assert counts == want.tolist(), (shape, m, seed)
            assert positions == list(range(first, first + len(want)))


@pytest.mark.parametrize("shape", SHAPES)
def test_core_sweep_is_the_closed_form(shape):
    chrom_size, span, max_w, n, pile = shape
    for seed in range(8):
        rng = np.random.default_rng(77 + seed)
        start, end = _rows(rng, n, span, max_w, pile)
        s, e = np.sort(start + 1), np.sort(end)  # sorted independently of each other
        counts, positions = R.core_counts(_pairs(s), _pairs(e), chrom_size, 1)
        want, first = R.closed_form_core(s, e, chrom_size)
        assert counts == want.tolist(), (shape, seed)
        assert positions == list(range(first, first + len(want)))


def test_sweeps_against_hand_computed_literals():
    # rows (2, 5), (4, 6), (9, 10) on a chromosome of 14 bp, smoothsize 1
    starts, ends = [3, 5, 10], [5, 6, 10]  # start + 1 and end
    # start track: windows [2, 5), [4, 7), [9, 12) -> positions 2 .. 14
    assert R.start_end_counts(_pairs(starts), 14, 1, 1) == ([1, 1, 2, 1, 1, 0, 0, 1, 1, 1, 0, 0, 0], list(range(2, 15)))
    # end track: windows [4, 7), [5, 8), [9, 12) -> positions 4 .. 14
    assert R.start_end_counts(_pairs(ends), 14, 1, 1) == ([1, 2, 2, 1, 0, 1, 1, 1, 0, 0, 0], list(range(4, 15)))
    # core track: opens 3, 5, 10, closes 5, 6, 10 (the 1 bp row opens and closes at 10) -> positions 3 .. 14
    assert R.core_counts(_pairs(starts), _pairs(ends), 14, 1) == ([1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0], list(range(3, 15)))
    # the runs of the start track from max(0, 3 - 1) = 2: a change at entry k ends its run at 2 + k + 1
    res = R.start_end_counts(_pairs(starts), 14, 1, 1)
    assert R.compress_counts(res, 2) == ([2, 5, 6, 8, 10, 13], [5, 6, 8, 10, 13, 15], [1, 2, 1, 0, 1, 0])
    for fn, args in ((R.closed_form_start_end, (starts, 14, 1)), (R.closed_form_start_end, (ends, 14, 1)),
                     (R.closed_form_core, (starts, ends, 14))):
        assert fn(*args)[0].dtype == np.uint32


def test_rows_past_the_chromosome_walk_to_the_last_open():
    # the sweep reports up to the last open - 1 even past chrom_size, and nothing when the first open lies past it
    assert R.start_end_counts(_pairs([5, 40]), 20, 2, 1)[1][-1] == 37
    assert R.start_end_counts(_pairs([30]), 20, 2, 1) == ([], [])
    assert R.closed_form_start_end([5, 40], 20, 2)[0].tolist() == R.start_end_counts(_pairs([5, 40]), 20, 2, 1)[0]
    assert len(R.closed_form_start_end([30], 20, 2)[0]) == 0


def test_module_imports_under_gtars_amd_only():
    import gtars_amd.uniwig as U

    for name in ("read_chromosomes", "start_end_counts", "core_counts", "compress_counts", "nonzero_counts", "uniwig",
                 "counts_device", "write_to_wig_file", "write_to_wig_file_variable", "write_to_bed_graph_file",
                 "write_to_npy_file", "write_combined_files"):
        assert callable(getattr(U, name)), name
    with pytest.raises(ModuleNotFoundError):
        importlib.import_module("gtars.uniwig")


@pytest.mark.parametrize("bed", BEDS)
def test_read_chromosomes_matches_the_restatement(bed, tmp_path):
    from gtars_amd.uniwig import read_chromosomes

    path = os.path.join(GOLDEN, bed)
    gz = str(tmp_path / (bed + ".gz"))
    with open(path, "rb") as src, gzip.open(gz, "wb") as dst:
        shutil.copyfileobj(src, dst)
    want = R.create_chrom_vec_default_score(path)
    assert len(want) >= 1
    for p in (path, gz):
        got = read_chromosomes(p)
        assert [c.chrom for c in got] == [w[0] for w in want]
        for c, w in zip(got, want):
            assert c.starts.dtype == np.uint32 and c.ends.dtype == np.uint32
            assert c.starts.tolist() == [x[0] for x in w[1]]
            assert c.ends.tolist() == [x[0] for x in w[2]]
    assert R.create_chrom_vec_default_score(gz) == want


def test_read_chromosomes_keeps_runs_in_file_order(tmp_path):
    from gtars_amd.uniwig import read_chromosomes

    bed = tmp_path / "runs.bed"
    bed.write_text("chr2\t10\t20\nchr2\t5\t30\nchr1\t7\t9\nchr2\t1\t2\n")
    got = read_chromosomes(str(bed))
    want = R.create_chrom_vec_default_score(str(bed))
    assert [c.chrom for c in got] == ["chr2", "chr1", "chr2"] == [w[0] for w in want]
    assert got[0].starts.tolist() == [6, 11] and got[0].ends.tolist() == [20, 30]
    assert got[2].starts.tolist() == [2] and got[2].ends.tolist() == [2]


def test_writers_bytes_match_the_restatement(tmp_path):
    import gtars_amd.uniwig as U

    rng = np.random.default_rng(5)
    counts = rng.integers(0, 4, 500).astype(np.uint32)
    counts[100:140] = 0
    counts[200] = 4_000_000_000
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    for limit in (1000, 300, 0):
        for d, mod in ((a, U), (b, R)):
            mod.write_to_wig_file(counts if mod is U else counts.tolist(), str(d / f"f{limit}.wig"), "chrT", 7, 1, limit)
        assert (a / f"f{limit}.wig").read_bytes() == (b / f"f{limit}.wig").read_bytes()
        R.write_to_wig_file_variable(counts.tolist(), str(b / f"v{limit}.wig"), "chrT", 7, 1, limit)
        nz = np.flatnonzero(counts[:limit])
        U.write_to_wig_file_variable(7 + nz, counts[:limit][nz], str(a / f"v{limit}.wig"), "chrT")
        assert (a / f"v{limit}.wig").read_bytes() == (b / f"v{limit}.wig").read_bytes()
    runs = R.compress_counts((counts.tolist(), list(range(500))), 3)
    U.write_to_bed_graph_file(tuple(np.asarray(x, dtype=np.uint32) for x in runs), str(a / "g.bedGraph"), "chrT")
    R.write_to_bed_graph_file(runs, str(b / "g.bedGraph"), "chrT", 1)
    assert (a / "g.bedGraph").read_bytes() == (b / "g.bedGraph").read_bytes()
    # appending, as the reference opens every file
    U.write_to_bed_graph_file(tuple(np.asarray(x, dtype=np.uint32) for x in runs), str(a / "g.bedGraph"), "chrU")
    R.write_to_bed_graph_file(runs, str(b / "g.bedGraph"), "chrU", 1)
    assert (a / "g.bedGraph").read_bytes() == (b / "g.bedGraph").read_bytes()
    for n in (500, 0, 1):
        for d, mod in ((a, U), (b, R)):
            mod.write_to_npy_file(counts[:n] if mod is U else counts[:n].tolist(), str(d / f"c{n}.npy"), "chrT", 7, 1,
                                  str(d / "start.meta"))
        assert (a / f"c{n}.npy").read_bytes() == (b / f"c{n}.npy").read_bytes()
        back = np.load(str(a / f"c{n}.npy"))
        assert back.dtype == np.uint32 and np.array_equal(back, counts[:n])
    assert (a / "start.meta").read_bytes() == (b / "start.meta").read_bytes()
    # write_combined_files: chromosome order, the parts removed
    for d, mod in ((a, U), (b, R)):
        for chrom in ("chrB", "chrA"):
            mod.write_to_wig_file(counts[:5] if mod is U else counts[:5].tolist(), str(d / f"p_{chrom}_start.wig"), chrom, 1, 1, 9)
    U.write_combined_files("start", "wig", str(a / "p_"), [U.Chromosome("chrB", None, None), U.Chromosome("chrX", None, None),
                                                           U.Chromosome("chrA", None, None)])
    R.write_combined_files("start", "wig", str(b / "p_"), [("chrB",), ("chrX",), ("chrA",)])
    assert (a / "p__start.wig").read_bytes() == (b / "p__start.wig").read_bytes()
    assert not (a / "p_chrB_start.wig").exists() and not (a / "p_chrA_start.wig").exists()


def test_calls_outside_the_domain_raise_value_error(tmp_path):
    import gtars_amd.uniwig as U

    with pytest.raises(ValueError, match="stepsize"):
        U.start_end_counts([5, 9], 100, 5, stepsize=2)
    with pytest.raises(ValueError, match="stepsize"):
        U.core_counts([5, 9], [8, 12], 100, stepsize=3)
    with pytest.raises(ValueError, match="zero-length"):
        U.core_counts([5, 9], [8, 8], 100)  # the row (8, 8): start + 1 = 9 > end
    with pytest.raises(ValueError, match="zero-length"):
        U.compress_counts("core", [5, 9], [8, 8], 100, 0, 5)
    with pytest.raises(ValueError, match="zero-length"):
        U.nonzero_counts("core", [5, 9], [8, 8], 100, 0, 5)
    bed = os.path.join(GOLDEN, BEDS[0])
    sizes = os.path.join(GOLDEN, "hg38.chrom.sizes")
    with pytest.raises(ValueError, match="stepsize"):
        U.uniwig(bed, sizes, 5, stepsize=10, output_prefix=str(tmp_path / "x"), output_type="npy")
    with pytest.raises(ValueError, match="scored"):
        U.uniwig(bed, sizes, 5, output_prefix=str(tmp_path / "x"), output_type="npy", score=True)
    with pytest.raises(ValueError, match="bigWig"):
        U.uniwig(bed, sizes, 5, output_prefix=str(tmp_path / "x"), output_type="bw")
    with pytest.raises(ValueError):
        U.track_extent("middle", [5], None, 100, 5)
    assert not os.listdir(tmp_path)
    # the extent is host arithmetic: first = max(1, p0 - m), last = max(chrom_size, last open - 1)
    assert U.track_extent("start", [40, 5], None, 20, 2) == (3, 35)
    assert U.track_extent("start", [30], None, 20, 2) == (28, 0)
    assert U.track_extent("core", [3, 5, 10], [5, 6, 10], 14, 0) == (3, 12)
    assert U.track_extent("start", [], None, 20, 2) == (0, 0)


@pytest.mark.skipif(__import__("gtars_amd").device_count() > 0, reason="needs a box WITHOUT a GPU")
def test_no_device_is_a_loud_error_not_a_fallback(tmp_path):
    import gtars_amd
    import gtars_amd.uniwig as U

    with pytest.raises(gtars_amd.NoDeviceError):
        U.start_end_counts([5, 9], 100, 5)
    with pytest.raises(gtars_amd.NoDeviceError):
        U.core_counts([5, 9], [8, 12], 100)
    with pytest.raises(gtars_amd.NoDeviceError):
        U.compress_counts("end", [5, 9], None, 100, 5, 1)
    with pytest.raises(gtars_amd.NoDeviceError):
        U.nonzero_counts("start", [5, 9], None, 100, 5, 1)
    with pytest.raises(gtars_amd.NoDeviceError):
        U.counts_device("start", 4096, 0, 1, 5, 1, 16, 4096)
    with pytest.raises(gtars_amd.NoDeviceError):
        U.uniwig(os.path.join(GOLDEN, BEDS[0]), os.path.join(GOLDEN, "hg38.chrom.sizes"), 5, output_prefix=str(tmp_path / "x"),
                 output_type="bedGraph")


def test_smoothsize_zero_writes_what_the_reference_writes(tmp_path):
    """lib.rs:135: with smoothsize 0 nothing is counted -- no device is needed, the combined files come out empty"""
    import gtars_amd.uniwig as U

    bed = os.path.join(GOLDEN, BEDS[0])
    sizes = os.path.join(GOLDEN, "hg38.chrom.sizes")
    for out_type in ("wig", "bedGraph", "npy"):
        a, b = tmp_path / ("a" + out_type), tmp_path / ("b" + out_type)
        a.mkdir(), b.mkdir()
        U.uniwig(bed, sizes, 0, output_prefix=str(a / "t"), output_type=out_type)
        R.uniwig_main(["start", "end", "core"], 0, bed, sizes, str(b / "t"), out_type)
        assert sorted(os.listdir(a)) == sorted(os.listdir(b)) and os.listdir(a)
        for f in os.listdir(a):
            if f.endswith(".json"):
                assert json.loads((a / f).read_text()) == json.loads((b / f).read_text())
            else:
                assert (a / f).read_bytes() == (b / f).read_bytes()


def test_cli_arguments(tmp_path, capsys):
    from gtars_amd import cli

    bed = os.path.join(GOLDEN, BEDS[0])
    sizes = os.path.join(GOLDEN, "hg38.chrom.sizes")
    base = ["uniwig", "-f", bed, "-c", sizes, "-m", "5", "-s", "1", "-l", str(tmp_path / "o")]
    assert cli.main(base + ["--filetype", "bam"]) == 2
    assert "bam is not provided" in capsys.readouterr().err
    assert cli.main(base + ["--outputtype", "bw"]) == 2
    assert "bw is not provided" in capsys.readouterr().err
    assert cli.main(base + ["-u", "shift"]) == 2
    assert not os.listdir(tmp_path)
    with pytest.raises(SystemExit):  # the reference's required flags
        cli.main(["uniwig", "-f", bed])
    capsys.readouterr()
    with pytest.raises(ValueError, match="stepsize"):
        cli.main(["uniwig", "--file", bed, "--chromref", sizes, "--smoothsize", "5", "--stepsize", "3", "--fileheader",
                  str(tmp_path / "o"), "--outputtype", "npy", "--counttype", "core", "--wigstep", "variable"])
    # smoothsize 0 runs without a device (nothing is counted): the long flags end to end
    assert cli.main(["uniwig", "--file", bed, "--filetype", "bed", "--chromref", sizes, "--smoothsize", "0", "--stepsize", "1",
                     "--fileheader", str(tmp_path / "z"), "--outputtype", "bedGraph", "--counttype", "start"]) == 0
    assert os.listdir(tmp_path) == ["z_start.bedGraph"]
    # the two other commands are still there
    with pytest.raises(SystemExit):
        cli.main(["overlaprs"])
    with pytest.raises(SystemExit):
        cli.main(["igd", "search"])


@pytest.mark.parametrize("m", [1, 25])
def test_sweeps_stay_at_zero_behind_the_last_close(m):
    """Behind the last window close the sweeps' queues are empty and every further entry is 0: the results for a larger
    chromosome are the results for a smaller one (that still holds every event) followed by zeros.  The end-to-end GPU test
    leans on this to compare whole-genome files without walking 1e8 positions in Python."""
    rng = np.random.default_rng(3 + m)
    start, end = _rows(rng, 40, 300, 30)
    s, e = np.sort(start + 1), np.sort(end)
    small = int(e[-1]) + m + 64
    for extra in (1, 7, 500):
        for fn, args in ((R.start_end_counts, (_pairs(s),)), (R.start_end_counts, (_pairs(e),))):
            a = fn(*args, small, m, 1)
            b = fn(*args, small + extra, m, 1)
            assert b[0] == a[0] + [0] * extra and b[1] == a[1] + list(range(small + 1, small + extra + 1))
        a = R.core_counts(_pairs(s), _pairs(e), small, 1)
        b = R.core_counts(_pairs(s), _pairs(e), small + extra, 1)
        assert b[0] == a[0] + [0] * extra
        ra, rb = R.compress_counts(a, 4), R.compress_counts(b, 4)
        assert ra[2][-1] == 0 and rb == (ra[0], ra[1][:-1] + [ra[1][-1] + extra], ra[2])
