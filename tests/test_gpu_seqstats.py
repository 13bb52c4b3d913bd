"""GC content and dinucleotide counts on the device (csrc/seqstats.hip, K12) against the plain-Python restatement
(tests/seqstats_ref.py).  Exact equality everywhere: the device counts integers and the divisions are the library's host f64
arithmetic in the reference's order.  The assembly is loaded both as FASTA and as .fab; every check runs on both, and every
device check runs under both lane groupings of k_seq_count (GTARS_SEQ_LANES = 16 and 64: a 256-byte and a 1-KiB step)."""
import random

import numpy as np
import pytest

import seqstats_ref as R

pytestmark = pytest.mark.gpu

# name -> length: around one 16-byte vector, around one piece, several pieces, and one long chromosome
LENGTHS = [("c1", 1), ("c2", 2), ("c15", 15), ("c16", 16), ("c17", 17), ("c4095", 4095), ("c4096", 4096), ("c4097", 4097),
           ("c100k", 100_003), ("c2m", 2_000_000)]
MID, LONG = "c100k", "c2m"


def _make_sequences():
    rng = np.random.default_rng(12)
    alphabet = np.frombuffer(b"ACGTacgtNn", dtype=np.uint8)
    seqs = {}
    for name, n in LENGTHS:
        s = alphabet[rng.integers(0, len(alphabet), n)].copy()
        if n > 4000:
            s[n // 3:n // 3 + 700] = ord("N")                                      # a run of N across vector boundaries
            s[n // 2:n // 2 + 1500] = np.frombuffer(b"acgt", np.uint8)[rng.integers(0, 4, 1500)]  # a soft-masked stretch
        # first and last byte are nucleotides: a window that leaked across the packed boundary between two chromosomes
        # (or into the next one's first byte) would be a VALID pair and show as a wrong count
        s[-1] = ord("c")
        s[0] = ord("G")
        seqs[name] = s.tobytes()
    return seqs


@pytest.fixture(scope="module")
def genomes(tmp_path_factory):
    from gtars_amd.seqstats import BinaryGenomeAssembly, GenomeAssembly, write_fab

    seqs = _make_sequences()
    d = tmp_path_factory.mktemp("seqstats")
    fa = d / "asm.fa"
    with open(fa, "wb") as f:
        for name, s in seqs.items():
            f.write(b">" + name.encode() + b" made for the test\n")
            for k in range(0, len(s), 60):
                f.write(s[k:k + 60] + b"\n")
    write_fab(str(fa), str(d / "asm.fab"))
    fasta, fab = GenomeAssembly(str(fa)), BinaryGenomeAssembly(str(d / "asm.fab"))
    assert fasta.chrom_sizes == fab.chrom_sizes == dict(LENGTHS)
    assert fasta.sequence(LONG, 0, 2_000_000) == seqs[LONG]
    return seqs, (fasta, fab)


LANES = ("16", "64")  # GTARS_SEQ_LANES: k_seq_count<16, *> and k_seq_count<64, *>


@pytest.fixture
def lane_settings(monkeypatch):
    """-> a generator function: sets GTARS_SEQ_LANES to each grouping in turn (the library takes a new snapshot of its switches)"""
    def settings():
        for lanes in LANES:
            monkeypatch.setenv("GTARS_SEQ_LANES", lanes)
            yield lanes

    return settings


def _rs(rows):
    from gtars_amd.models import RegionSet

    return RegionSet.from_vectors([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])


def _check(genomes, rows, settings, ignore=False):
    """both library calls on both assemblies under every lane grouping against the restatement; -> the labels and integer rows"""
    from gtars_amd.seqstats import calc_dinucl_freq, calc_gc_content

    seqs, loaded = genomes
    rs = _rs(rows)
    want_gc = R.calc_gc_content(rows, seqs, ignore)
    labels, counts = R.calc_dinucl_counts(rows, seqs, ignore)
    want_raw = [[float(c) for c in row] for row in counts]
    for lanes in settings():
        for g in loaded:
            assert calc_gc_content(rs, g, ignore_unk_chroms=ignore) == want_gc, lanes
            got = calc_dinucl_freq(rs, g, raw_counts=True, ignore_unk_chroms=ignore)
            assert got["region_labels"] == labels, lanes
            assert got["frequencies"] == want_raw, lanes
            assert g.device >= 0
    return labels, counts


def test_short_regions_at_every_alignment(genomes, lane_settings):
    rows = [(MID, s, s + w) for s in range(4080, 4112) for w in (0, 1, 2, 3, 15, 16, 17, 31, 32, 33)]
    _check(genomes, rows, lane_settings)


def test_piece_edges(genomes, lane_settings):
    from gtars_amd.seqstats import SEQ_PIECE as PIECE

    assert PIECE >= 16 and 3 * PIECE + 5 + 16 < 100_003
    rows = [(MID, s, s + w) for s in (0, 1, 15, 16) for w in (PIECE - 1, PIECE, PIECE + 1, 2 * PIECE, 3 * PIECE + 5)]
    rows += [(LONG, 1_000_000 - 7, 1_000_000 - 7 + 3 * PIECE + 5)]
    _check(genomes, rows, lane_settings)


def test_chromosome_ends(genomes, lane_settings):
    rows = []
    for name, n in LENGTHS:
        rows += [(name, n - k, n) for k in range(0, 34) if k <= n]
        rows += [(name, 0, n), (name, 0, 0)]
    labels, counts = _check(genomes, rows, lane_settings)
    whole = dict(zip(labels, counts))
    assert sum(whole["c1_0_1"]) == 0 and sum(whole["c2_0_2"]) <= 1


@pytest.fixture(scope="module")
def mixed_rows():
    rng = random.Random(5)
    rows = [(LONG, 50_000, 1_950_000)]
    for _ in range(20_000):
        name, n = (MID, 100_003) if rng.random() < 0.3 else (LONG, 2_000_000)
        w = rng.randint(1, 2000)
        s = rng.randint(0, n - w)
        rows.append((name, s, s + w))
    rng.shuffle(rows)
    return rows


def test_long_and_mixed(genomes, mixed_rows, lane_settings):
    from gtars_amd.seqstats import calc_dinucl_freq, calc_gc_content

    labels, counts = _check(genomes, mixed_rows, lane_settings)
    shuffled = dict(zip(labels, ([float(c) for c in row] for row in counts)))
    assert sum(shuffled[f"{LONG}_50000_1950000"]) > 1_000_000  # the long region went through the adding path
    # the same set in sorted order: the same row for every region
    ordered = _rs(sorted(mixed_rows))
    want_gc = sorted(R.calc_gc_content(mixed_rows, genomes[0]))
    for lanes in lane_settings():
        for g in genomes[1]:
            got = calc_dinucl_freq(ordered, g, raw_counts=True)
            assert len(got["region_labels"]) == len(mixed_rows)
            assert all(shuffled[label] == row for label, row in zip(got["region_labels"], got["frequencies"])), lanes
            assert sorted(calc_gc_content(ordered, g)) == want_gc, lanes


def test_order_and_skipping(genomes):
    from gtars_amd.seqstats import calc_dinucl_freq, calc_gc_content
    from gtars_amd.models import Region, RegionSet

    seqs, loaded = genomes
    rows = [(LONG, 10, 5000), ("chrNope", 0, 10), (MID, 0, 100), (LONG, 1_999_990, 2_000_001), ("c16", 0, 16), (MID, 50, 40),
            ("other", 5, 6), (LONG, 0, 1), (MID, 99_000, 100_003), ("c16", 3, 3), ("chrNope", 1, 2), (LONG, 7, 4100)]
    rs = RegionSet.from_regions([Region(*r) for r in rows])
    labels, counts = R.calc_dinucl_counts(rows, seqs, True)
    assert labels[:3] == [f"{LONG}_10_5000", f"{LONG}_0_1", f"{LONG}_7_4100"] and len(labels) == 7
    for g in loaded:
        got = calc_dinucl_freq(rs, g, raw_counts=True, ignore_unk_chroms=True)
        assert got["region_labels"] == labels and got["frequencies"] == [[float(c) for c in row] for row in counts]
        assert calc_gc_content(rs, g, ignore_unk_chroms=True) == R.calc_gc_content(rows, seqs, True)
        # output order decides which row fails the call: the long chromosome comes first
        with pytest.raises(RuntimeError, match=rf"{LONG}.*1999990.*2000001"):
            calc_gc_content(rs, g)
        with pytest.raises(RuntimeError, match=rf"{LONG}.*1999990.*2000001"):
            calc_dinucl_freq(rs, g)
        # the handle is as usable as before
        assert calc_gc_content(rs, g, ignore_unk_chroms=True) == R.calc_gc_content(rows, seqs, True)


def _device_counts(g, mode, rows):
    import torch

    from gtars_amd.seqstats import counts_device

    ids = {name: k for k, name in enumerate(g.chrom_names)}
    dev = torch.device("cuda", torch.cuda.current_device())
    cols = [torch.from_numpy(np.array(c, dtype=np.uint32).view(np.int32)).to(dev)
            for c in ([ids[r[0]] for r in rows], [r[1] for r in rows], [r[2] for r in rows])]
    width = 1 if mode == "gc" else 16
    out = torch.full((max(len(rows), 1) * width,), -1, dtype=torch.int32, device=dev)
    counts_device(g, mode, cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), len(rows), out.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
    return out.cpu().numpy().view(np.uint32).reshape(-1, width)


def test_device_entry(genomes, mixed_rows, lane_settings):
    from gtars_amd.seqstats import calc_dinucl_freq

    seqs, loaded = genomes
    want_gc = [R.gc_count(seqs[c][s:e]) for c, s, e in mixed_rows]
    for lanes in lane_settings():
        for g in loaded:
            # n == 0: success, nothing touched
            assert (_device_counts(g, "gc", []).view(np.int32) == -1).all()
            assert (_device_counts(g, "dinucl", []).view(np.int32) == -1).all()
            one = [(MID, 4090, 4131)]
            seq = seqs[MID][4090:4131]
            assert _device_counts(g, "gc", one).tolist() == [[R.gc_count(seq)]], lanes
            assert _device_counts(g, "dinucl", one).tolist() == [R.dinucl_counts(seq)], lanes
        # input order out; equal to the library call's counts row by row
        g = loaded[0]
        gc = _device_counts(g, "gc", mixed_rows)[:, 0].tolist()
        di = _device_counts(g, "dinucl", mixed_rows).tolist()
        assert gc == want_gc, lanes
        lib_rows = calc_dinucl_freq(_rs(mixed_rows), g, raw_counts=True)
        by_label = dict(zip(lib_rows["region_labels"], lib_rows["frequencies"]))
        assert [[float(c) for c in row] for row in di] == [by_label[f"{c}_{s}_{e}"] for c, s, e in mixed_rows], lanes
        with pytest.raises(ValueError):  # a row outside its chromosome is refused, never read
            _device_counts(g, "gc", [(MID, 0, 100_004)])


# one step of a lane group is LANES x 16 bytes: 256 bytes for 16 lanes, 1024 for 64
STEP_WIDTHS = {"16": (255, 256, 257, 271, 272, 273), "64": (1007, 1008, 1009, 1023, 1024, 1025, 1039, 1040, 1041)}


def step_edge_rows():
    """rows on c100k with start in 4080 .. 4096 and widths around one step of each grouping and around the step plus one vector"""
    return [(MID, s, s + w) for s in range(4080, 4097) for w in STEP_WIDTHS["16"] + STEP_WIDTHS["64"]]


@pytest.mark.parametrize("lanes", LANES)
def test_lane_group_step_edges(genomes, monkeypatch, lanes):
    """Widths at which the number of aligned 16-byte vectors of a piece, nv, passes LANES and LANES + 1 for both groupings, at
    every alignment of the start: the last lane of the group (gl == LANES - 1) reads the second byte of its last window with a
    load of its own; lane 0 of the next step names a window whose first byte the previous step saw; the last vector of a piece
    is the first vector of a step.  Both modes, through the library calls (both assemblies) and through the device entry."""
    seqs, loaded = genomes
    rows = step_edge_rows()
    first = rows[0][1] & ~15
    nvs = {((e - first) + 15) // 16 for _, s, e in rows if s == rows[0][1]}
    assert {16, 17, 18, 64, 65, 66} <= nvs  # LANES, LANES + 1 and one more, for both groupings
    monkeypatch.setenv("GTARS_SEQ_LANES", lanes)
    _, counts = _check(genomes, rows, lambda: [lanes])
    for g in loaded:
        assert _device_counts(g, "gc", rows)[:, 0].tolist() == [R.gc_count(seqs[c][s:e]) for c, s, e in rows]
        assert _device_counts(g, "dinucl", rows).tolist() == counts


def test_python_surface(genomes):
    import gtars.seqstats as S
    from gtars_amd.seqstats import DINUCLEOTIDES, calc_dinucl_freq, calc_gc_content

    seqs, (fasta, fab) = genomes
    rows = [(MID, 100, 700), (LONG, 0, 9000), ("c2", 0, 2), (MID, 33_330, 34_050), ("c17", 0, 0)]
    rs = _rs(rows)
    gc = calc_gc_content(rs, fasta)
    assert all(type(v) is float for v in gc) and len(gc) == len(rows)
    labels, counts = R.calc_dinucl_counts(rows, seqs)
    raw = calc_dinucl_freq(rs, fab, raw_counts=True)
    assert raw["dinucleotides"] == DINUCLEOTIDES == R.DINUCL_ORDER and raw["region_labels"] == labels
    assert all(type(v) is float and v == int(v) for row in raw["frequencies"] for v in row)
    assert [sum(row) for row in raw["frequencies"]] == [float(sum(c)) for c in counts]
    pct = calc_dinucl_freq(rs, fab)
    for got, c in zip(pct["frequencies"], counts):
        total = sum(c)
        assert got == ([(x / total) * 100.0 for x in c] if total else [0.0] * 16)
    assert pct["frequencies"][-1] == [0.0] * 16 and sum(counts[0]) > 0
    assert S.calc_gc_content is calc_gc_content and S.calc_dinucl_freq is calc_dinucl_freq
    assert S.GenomeAssembly is type(fasta) and S.BinaryGenomeAssembly is type(fab)
