"""K18 on the device (csrc/vrs.hip) against the plain-Python restatement (tests/vrs_ref.py): exact equality of statuses, intervals,
normalized sequences and identifiers.  The assembly is written by the test (about 0.6 MB): one chromosome of random bases with
repeats planted at known places, two neighbours that end and start with AAAA, and a chromosome of length 1.

Positions have 1 to 6 decimal digits: a 9-digit position needs a chromosome of 100 Mb, which a test's assembly cannot be; the
digit texts of longer numbers are the host's (tests/test_vrs_cpu.py), the device's are the same register code for any count."""
import random

import numpy as np
import pytest

import vrs_ref as R
from test_vrs_cpu import SEQS as SMALL_SEQS, VCF_TEXT, vcf_variants, write_fasta

pytestmark = pytest.mark.gpu

CAP = 8  # GTARS_VRS_ROLL_CAP of the tests that send alleles to the wave-per-allele path
BIG_N = 600_011


def _plant(s, at, text):
    s[at:at + len(text)] = text
    return at


def _make_sequences():
    rng = random.Random(18)
    big = bytearray(rng.choice(b"ACGT") for _ in range(BIG_N))
    where = {}
    # every planted repeat stands between two bases it cannot roll through
    for name, at, unit, n in [("homo", 1_000, b"A", 40), ("di", 2_000, b"AC", 23), ("tri", 3_000, b"CAG", 17), ("soft", 4_000, b"t", 30),
                              ("softdi", 4_200, b"ga", 12), ("long", 100_000, b"T", 1_300), ("longtri", 200_000, b"GAT", 500)]:
        text = unit * n
        if name == "di":
            text += b"A"       # ends in the middle of a unit
        if name == "tri":
            text += b"CA"
        if name == "longtri":
            text += b"G"
        first = bytes([next(b for b in b"TGCA" if b not in unit.upper())])  # a base the repeat's unit does not have
        _plant(big, at - 1, first)
        _plant(big, at, text)
        _plant(big, at + len(text), b"N" if name == "homo" else first)
        where[name] = (at, len(text), unit)
    _plant(big, 5_000, b"ACGTNNNNNNNNACGT")
    _plant(big, 5_100, b"CNNNNNNNNC")
    big[0:4] = b"GATC"
    return {"big": bytes(big), "e1": b"CGTACGTGCAAAA", "e2": b"AAAAGTCGATCG", "one": b"G"}, where


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from gtars_amd.seqstats import BinaryGenomeAssembly, GenomeAssembly, write_fab

    seqs, where = _make_sequences()
    d = tmp_path_factory.mktemp("vrs_gpu")
    write_fasta(d / "asm.fa", seqs, width=61)
    write_fab(str(d / "asm.fa"), str(d / "asm.fab"))
    fasta, fab = GenomeAssembly(str(d / "asm.fa")), BinaryGenomeAssembly(str(d / "asm.fab"))
    acc = R.refget_digests(seqs)
    assert fasta.refget_digests() == acc == fab.refget_digests()
    return seqs, where, (fasta, fab), acc


def _check(world, rows, genomes=None, accessions=None):
    """both batch calls on the device against the restatement -> the restatement's columns"""
    from gtars_amd import vrs as V

    seqs, _, loaded, acc = world
    st, ns, ne, sq, ids = R.alleles(seqs, acc if accessions is None else {k: v[-32:] for k, v in accessions.items()}, rows)
    plain = (st, ns, ne, sq) if accessions is None else R.alleles(seqs, acc, rows)[:4]  # (normalization knows no accessions)
    cols = [[r[k] for r in rows] for k in range(4)]
    for g in genomes or loaded[:1]:
        got = V.normalize_alleles(g, *cols)
        assert got["statuses"].tolist() == plain[0]
        assert got["starts"].tolist() == plain[1] and got["ends"].tolist() == plain[2]
        assert got["sequences"] == plain[3]
        got = V.vrs_ids(g, *cols, accessions=accessions)
        assert got["statuses"].tolist() == st
        assert got["ids"] == ids
        assert g.device >= 0
    return st, ns, ne, sq, ids


def _mnv(seq, at, n, rng):
    """REF = seq[at, at + n), ALT of n bases that differs from it at both ends: nothing trims, nothing rolls"""
    ref = seq[at:at + n]
    other = {65: 67, 67: 71, 71: 84, 84: 65, 78: 65}
    alt = bytearray(rng.choice(b"ACGT") for _ in range(n))
    alt[0], alt[-1] = other[ref[0] & 0xDF], other[ref[-1] & 0xDF]
    return bytes(ref), bytes(alt)


POSITIONS = [3, 57, 412, 6_003, 60_011, 500_009]  # 1 .. 6 digits


def test_padding_lengths(world):
    """normalized lengths that put the Allele message at 111, 112, 127, 0 and 1 bytes past a block edge (the padding takes the
    rest of the block, or one more), and the empty sequence; starts and ends of every digit count the assembly allows"""
    seqs, _, loaded, acc = world
    big = seqs["big"]
    rng = random.Random(1)
    empty = len(R.allele_text("x" * 32, b""))
    rows, want_mod = [], []
    for k, target in enumerate([111, 112, 127, 0, 1]):
        for extra in (0, 128):
            n = (target - empty) % 128 + extra
            at = POSITIONS[(k + extra // 128) % len(POSITIONS)]
            rows.append(("big", at) + _mnv(big, at, n, rng))
            want_mod.append(target)
    for at in POSITIONS + [0, 9, 10, 99, 100, 999, 1000, 9_999, 10_000, 99_999, 100_000 - 2]:
        rows.append(("big", at, big[at:at + 2], big[at:at + 2]))  # ref == alt: the empty sequence
        rows.append(("big", at) + _mnv(big, at, 1, rng))
    st, ns, ne, sq, ids = _check(world, rows, genomes=loaded)
    assert set(st) == {R.OK}
    assert [len(R.allele_text("x" * 32, s)) % 128 for s in sq[:10]] == want_mod
    assert {len(str(v)) for v in ns} == {1, 2, 3, 4, 5, 6} and b"" in sq
    lens = {len(R.location_text("SQ." + acc["big"], a, b)) for a, b in zip(ns, ne)}
    assert len(lens) >= 6  # the location text at several alignments of its digits


def test_bounds_between_neighbours(world):
    """e1 ends in AAAA and e2, its neighbour in the packed image, starts with AAAA: a roll stops at the chromosome's length and
    at 0; a chromosome of length 1"""
    seqs, _, loaded, _ = world
    n1 = len(seqs["e1"])
    rows = [("e1", n1, b"", b"A"), ("e1", n1 - 1, b"A", b"AA"), ("e1", n1 - 2, b"AA", b"A"), ("e2", 0, b"", b"A"), ("e2", 0, b"A", b"AA"),
            ("e2", 1, b"AA", b"A"), ("e2", 0, b"AAAA", b""), ("e1", n1 - 4, b"AAAA", b"A"),
            ("one", 0, b"G", b"T"), ("one", 0, b"", b"G"), ("one", 1, b"", b"G"), ("one", 0, b"G", b""), ("one", 0, b"G", b"G"),
            ("one", 1, b"", b"GG"), ("one", 0, b"", b"C")]
    st, ns, ne, sq, _ = _check(world, rows, genomes=loaded)
    assert set(st) == {R.OK}
    assert (ns[0], ne[0], sq[0]) == (n1 - 4, n1, b"AAAAA") and (ns[3], ne[3], sq[3]) == (0, 4, b"AAAAA")
    assert (ns[9], ne[9], sq[9]) == (0, 1, b"GG") and (ns[10], ne[10]) == (0, 1)


def _repeat_rows(where, seqs):
    big = seqs["big"]
    rows = []
    for name in ("homo", "di", "tri", "soft", "softdi"):
        at, n, unit = where[name]
        up = unit.upper()
        for k in (0, 1, len(unit), n // 2, n - 1, n):
            rows.append(("big", at + k, b"", up))                                   # insert one unit (upper-case alleles)
            if k + len(unit) <= n:
                rows.append(("big", at + k, big[at + k:at + k + len(unit)].upper(), b""))  # delete one unit
                rows.append(("big", at + k, big[at + k:at + k + len(unit)], b""))           # ... REF as the assembly has it
        rows.append(("big", at + 2, b"", unit.lower()))                              # a lower-case ALT does not roll
        rows.append(("big", at + 2, b"", up * 2 + up[:1]))                           # an allele that is no whole number of units
    rows += [("big", 5_004, b"", b"N"), ("big", 5_006, b"NN", b"N"), ("big", 5_003, b"TN", b"T"), ("big", 5_105, b"", b"N"),
             ("big", 5_000 + 12, b"A", b"AN")]
    return rows


def test_repeats_roll_through_the_circular_index(world):
    seqs, where, loaded, _ = world
    rows = _repeat_rows(where, seqs)
    st, ns, ne, sq, _ = _check(world, rows, genomes=loaded)
    assert set(st) == {R.OK}
    got = {(r[1], r[2], r[3]): (a, b, s) for r, a, b, s in zip(rows, ns, ne, sq)}
    at, n, _ = where["di"]
    assert got[(at + 2, b"", b"AC")][:2] == (at, at + n) and got[(at + 1, b"", b"AC")][:2] == (at + 1, at + 1)          # the whole repeat, its half unit at the end included
    at, n, _ = where["tri"]
    assert got[(at + 3, b"", b"CAG")][:2] == (at, at + n)
    at, n, _ = where["soft"]
    assert got[(at + n // 2, b"", b"T")] == (at, at + n, b"T" * (n + 1))  # a soft-masked repeat rolls, its context comes back upper-case
    assert got[(at + 2, b"", b"t")] == (at + 2, at + 2, b"t")           # a lower-case ALT does not
    assert got[(5_004, b"", b"N")][:2] == (5_004, 5_012)


def _cap_rows(where):
    """insertions into the long runs whose rolls are CAP - 1, CAP, CAP + 1 and CAP + 63, 64, 65, about 1000 in each direction"""
    at, n, _ = where["long"]
    rows = []
    for d in (1, CAP - 1, CAP, CAP + 1, CAP + 62, CAP + 63, CAP + 64, CAP + 65, CAP + 127, CAP + 128, CAP + 129, CAP + 1000):
        rows.append(("big", at + d, b"", b"T"))       # left roll d, right roll n - d
        rows.append(("big", at + n - d, b"", b"T"))   # right roll d
        rows.append(("big", at + d, b"T", b""))       # a deletion: left roll d, right roll n - d - 1
    at, n, _ = where["longtri"]
    for d in (CAP - 1, CAP, CAP + 1, CAP + 63, CAP + 64, CAP + 65, 997):
        for alt in (b"GAT", b"ATG", b"TGA"):
            rows.append(("big", at + d, b"", alt))
    return rows


def test_roll_cap_and_the_wave_path(world, monkeypatch):
    """the same alleles with the cap at 8 (most rolls finish in k_vrs_roll_long), at its default, and so large that no allele
    leaves the lane path: one result, the restatement's"""
    from gtars_amd import vrs as V

    seqs, where, loaded, _ = world
    rows = _cap_rows(where) + _repeat_rows(where, seqs)
    cols = [[r[k] for r in rows] for k in range(4)]
    results = {}
    for cap in (str(CAP), None, str(1 << 20), "1"):
        if cap is None:
            monkeypatch.delenv("GTARS_VRS_ROLL_CAP", raising=False)
        else:
            monkeypatch.setenv("GTARS_VRS_ROLL_CAP", cap)
        st, ns, ne, sq, ids = _check(world, rows)
        got = V.normalize_alleles(loaded[0], *cols)
        results[cap] = (got["starts"].tolist(), got["ends"].tolist(), got["sequences"])
    assert results[str(CAP)] == results[None] == results[str(1 << 20)] == results["1"]
    at, n, _ = where["long"]
    rolled = {(r[1], r[2], r[3]): (a, b) for r, a, b in zip(rows, ns, ne)}
    assert rolled[(at + CAP + 64, b"", b"T")] == (at, at + n) and rolled[(at + n - CAP, b"", b"T")] == (at, at + n)
    left = sorted({r[1] - a for r, a in zip(rows, ns) if r[2] == b"" and r[3] == b"T" and at <= r[1] <= at + n})
    assert {CAP - 1, CAP, CAP + 1, CAP + 63, CAP + 64, CAP + 65, CAP + 1000} <= set(left)


def _kinds(seqs):
    big = seqs["big"]
    rng = random.Random(4)
    p = 7_000
    ref = big[p:p + 6]
    flip = {65: b"C", 67: b"G", 71: b"T", 84: b"A"}
    rows = [
        ("big", p, ref[:1], flip[ref[0]]),                                    # SNV
        ("big", p) + _mnv(big, p, 4, rng),                                    # MNV
        ("big", p, ref, ref[:2] + flip[ref[2]] + flip[ref[3]] + b"T" + ref[4:]),  # delins, both trimmed alleles non-empty
        ("big", p, b"", b"GATTACA"),                                          # pure insertion, empty REF
        ("big", p, ref[:4], ref[:1]),                                         # deletion
        ("big", p, ref, ref),                                                 # ref == alt
        ("big", p, ref.lower(), ref.lower()[:3]),                             # lower-case alleles
    ]
    failing = [
        ("big", BIG_N + 5, b"A", b"C"),                # start beyond the chromosome: REF past its end, as the reference says it
        ("big", BIG_N - 1, big[-1:] + b"A", b"C"),     # REF past the end
        ("big", BIG_N, b"A", b""),
        ("big", p, flip[ref[0]], b"A"),                # REF mismatch
        ("big", p, ref[:3] + flip[ref[3]], b"A"),      # ... in its last base
        ("big", (1 << 64) - 1, b"AC", b"A"),           # start + len(REF) overflows
        ("nope", 5, b"A", b"C"),                       # a name the assembly lacks
    ]
    return rows, failing


def test_kinds_and_failing_rows_leave_their_neighbours_alone(world):
    seqs, _, loaded, _ = world
    good, failing = _kinds(seqs)
    alone = _check(world, good, genomes=loaded)
    assert set(alone[0]) == {R.OK}
    mixed = []
    for k in range(max(len(good), len(failing))):
        mixed += failing[k:k + 1] + good[k:k + 1]
    st, ns, ne, sq, ids = _check(world, mixed, genomes=loaded)
    assert [s for s in st if s != R.OK] == [R.REF_PAST_END, R.REF_PAST_END, R.REF_PAST_END, R.REF_MISMATCH, R.REF_MISMATCH,
                                            R.START_OUT_OF_BOUNDS, R.UNKNOWN_CHROMOSOME]
    assert [i for i, s in zip(ids, st) if s == R.OK] == alone[4]
    # a caller's table that lacks a chromosome: its rows are status 4, the others use the table's digests
    seqs_acc = {"big": "SQ." + "Q" * 32, "one": "z" * 32}
    st2 = _check(world, mixed + [("e1", 2, b"T", b"G"), ("one", 0, b"G", b"T")], accessions=seqs_acc)[0]
    assert st2[-2:] == [R.UNKNOWN_CHROMOSOME, R.OK]


@pytest.fixture(scope="module")
def mixed_batch(world):
    seqs, where, _, _ = world
    good, failing = _kinds(seqs)
    rng = random.Random(9)
    rows = _cap_rows(where)[:40] + _repeat_rows(where, seqs) + good + failing
    big = seqs["big"]
    while len(rows) < 300:
        at = rng.randrange(0, BIG_N - 40)
        kind = rng.random()
        if kind < 0.6:
            rows.append(("big", at) + _mnv(big, at, 1, rng))
        elif kind < 0.8:
            rows.append(("big", at, big[at:at + 1], big[at:at + 1] + bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 5)))))
        else:
            rows.append(("big", at, big[at:at + rng.randint(2, 30)], big[at:at + 1]))
    rng.shuffle(rows)
    return rows


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_batch_sizes(world, mixed_batch, n):
    st = _check(world, mixed_batch[:n])[0]
    assert len(st) == n


def test_host_tail_gives_the_same_identifiers(world, mixed_batch, monkeypatch):
    """GTARS_VRS_HOST_LEN 0 (every non-empty sequence is hashed by the host threads), 8, and larger than every allele"""
    from gtars_amd import vrs as V

    cols = [[r[k] for r in mixed_batch] for k in range(4)]
    seen = []
    for host_len in ("0", "8", str(1 << 20)):
        monkeypatch.setenv("GTARS_VRS_HOST_LEN", host_len)
        monkeypatch.setenv("GTARS_VRS_ROLL_CAP", str(CAP))
        st, ns, ne, sq, ids = _check(world, mixed_batch)
        seen.append(V.vrs_ids(world[2][0], *cols)["ids"])
    assert seen[0] == seen[1] == seen[2] == ids
    assert any(len(s) > 8 for s in sq) and any(0 < len(s) <= 8 for s in sq) and max(len(s) for s in sq) > 1000


def test_device_path_equals_the_host_path(world, mixed_batch):
    from gtars_amd import vrs as V

    g = world[2][1]
    cols = [[r[k] for r in mixed_batch] for k in range(4)]
    dev, host = V.normalize_alleles(g, *cols), V.normalize_alleles(g, *cols, on_host=True)
    assert dev["statuses"].tolist() == host["statuses"].tolist() and dev["sequences"] == host["sequences"]
    assert dev["starts"].tolist() == host["starts"].tolist() and dev["ends"].tolist() == host["ends"].tolist()
    assert V.vrs_ids(g, *cols)["ids"] == V.vrs_ids(g, *cols, on_host=True)["ids"]


def test_sequences_at_every_group_offset_and_tail(world):
    """the byte CSR of the normalized sequences (byte_csr.h over the source of vrs.hip: eight output bytes per lane, whole
    groups stored as one word): sequences that start at every offset 0 .. 7 of a group, made of left context, ALT and right
    context or of the ALT alone, one to 1300 bytes long; failing rows -- empty sequences -- first, twice in a row in the middle
    and last; eight batches that drop 0 .. 7 trailing one-byte rows, so the packed total has every residue mod 8"""
    from gtars_amd import vrs as V

    seqs, where, loaded, acc = world
    big = seqs["big"]
    rng = random.Random(21)
    failing = _kinds(seqs)[1]

    def mnvs(count, first):
        return [("big", first + 50 * k) + _mnv(big, first + 50 * k, 1 + k % 11, rng) for k in range(count)]

    head = failing[3:4] + _repeat_rows(where, seqs) + mnvs(90, 10_000) + failing[0:1] + failing[4:5] + _cap_rows(where)[:6] + mnvs(90, 20_000)
    ones = [("big", 30_000 + 50 * k) + _mnv(big, 30_000 + 50 * k, 1, rng) for k in range(7)]
    last = failing[1:2]
    rows = head + ones + last
    st, _, _, sq, _ = R.alleles(seqs, acc, rows)
    assert 200 <= len(rows) <= 400
    n_head = len(head)
    assert [len(s) for s in sq[n_head:]] == [1] * 7 + [0] and st[-1] != R.OK
    assert st[0] != R.OK and sq[0] == b"" and any(st[k] != R.OK and st[k + 1] != R.OK and sq[k] == sq[k + 1] == b"" for k in range(1, n_head - 1))
    starts = np.cumsum([0] + [len(s) for s in sq])[:-1]
    assert {int(o) % 8 for o, s in zip(starts, sq) if s} == set(range(8))
    assert {int(o) % 8 for o, s in zip(starts, sq) if len(s) > 8} == set(range(8))  # ... of sequences that cross a group's end, too
    totals = set()
    for drop in range(8):
        keep = list(range(n_head + 7 - drop)) + [len(rows) - 1]
        batch, want = [rows[k] for k in keep], [sq[k] for k in keep]
        totals.add(sum(len(s) for s in want) % 8)
        cols = [[r[k] for r in batch] for k in range(4)]
        for g in loaded:
            dev, host = V.normalize_alleles(g, *cols), V.normalize_alleles(g, *cols, on_host=True)
            assert dev["statuses"].tolist() == [st[k] for k in keep] == host["statuses"].tolist()
            assert dev["sequences"] == want
            assert host["sequences"] == want
    assert totals == set(range(8))


def test_file_call(tmp_path):
    """the CPU test's small VCF through compute_vrs_ids, plain and BGZF, row for row; with one REF mismatch the call raises for
    the first failing row in file order"""
    from gtars_amd import vrs as V
    from gtars_amd.seqstats import GenomeAssembly

    write_fasta(tmp_path / "small.fa", SMALL_SEQS)
    g = GenomeAssembly(str(tmp_path / "small.fa"))
    acc = R.refget_digests(SMALL_SEQS)
    want = R.compute_vrs_ids(VCF_TEXT, SMALL_SEQS, acc)
    assert len(want) == 10
    for name, data in vcf_variants().items():
        (tmp_path / name).write_bytes(data)
        res = V.compute_vrs_ids(str(tmp_path / name), g)
        assert list(zip(res.chrom, res.pos, res.ref_allele, res.alt_allele, res.vrs_id)) == want, name
    assert g.device >= 0
    bad = VCF_TEXT.replace(b"chr2\t13\t.\tATC\tA", b"chr2\t13\t.\tATG\tA") + b"\nchr1\t999\t.\tA\tC\n"
    (tmp_path / "bad.vcf").write_bytes(bad)
    with pytest.raises(ValueError) as err:
        V.compute_vrs_ids(str(tmp_path / "bad.vcf"), g)
    assert str(err.value) == "Failed to normalize variant at chr2:13: ref allele mismatch at interbase 12: VCF says ATG, reference has ATC"
    # a caller's table: chr2 is not in it, so its rows -- the failing one too -- are skipped
    mine = {k: v for k, v in acc.items() if k != "chr2"}
    with pytest.raises(ValueError, match=r"Failed to normalize variant at chr1:999: ref allele \(start=998, len=1\) extends past"):
        V.compute_vrs_ids(str(tmp_path / "bad.vcf"), g, accessions=mine)
    res = V.compute_vrs_ids(str(tmp_path / "plain.vcf"), g, accessions=mine)
    assert list(zip(res.chrom, res.pos, res.ref_allele, res.alt_allele, res.vrs_id)) == [r for r in want if r[0] != "chr2"]


def test_device_entry_on_a_stream_and_a_forged_device(world, mixed_batch):
    import torch

    from gtars_amd import vrs as V
    from gtars_amd._lib import lib

    seqs, _, loaded, acc = world
    g = loaded[0]
    rows = mixed_batch
    st, ns, ne, sq, ids = R.alleles(seqs, acc, rows)
    c = V._Columns(g, *[[r[k] for r in rows] for k in range(4)])
    dev = torch.device("cuda", torch.cuda.current_device())
    n = c.n

    def put(a, dtype):
        return torch.from_numpy(a.view(dtype).copy()).to(dev)

    chrom, start = put(c.chrom, np.int32), put(c.start, np.int64)
    pool = put(c.pool, np.uint8)
    ro, rl, ao, al = (put(x, np.int32) for x in (c.ref_off, c.ref_len, c.alt_off, c.alt_len))
    status = torch.full((n,), 77, dtype=torch.uint8, device=dev)
    d_ns, d_ne = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    digests = torch.zeros(32 * n, dtype=torch.uint8, device=dev)

    def call(stream):
        V.ids_device(g, chrom.data_ptr(), start.data_ptr(), pool.data_ptr(), c.pool.size, ro.data_ptr(), rl.data_ptr(), ao.data_ptr(),
                     al.data_ptr(), n, status.data_ptr(), d_ns.data_ptr(), d_ne.data_ptr(), digests.data_ptr(), stream)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(side.cuda_stream)
    assert status.cpu().tolist() == st
    assert d_ns.cpu().numpy().view(np.uint64).tolist() == ns and d_ne.cpu().numpy().view(np.uint64).tolist() == ne
    raw = digests.cpu().numpy().tobytes()
    got = ["ga4gh:VA." + raw[32 * i:32 * i + 32].decode() if st[i] == R.OK else None for i in range(n)]
    assert got == ids
    assert all(raw[32 * i:32 * i + 32] == bytes(32) for i in range(n) if st[i] != R.OK)
    # n == 0 touches nothing
    V.ids_device(g, 0, 0, 0, 0, 0, 0, 0, 0, 0)
    # the call runs on the assembly's device or is refused
    cur = torch.cuda.current_device()
    forged = cur + 1
    assert lib.gtars_debug_set_assembly_device(g._h, forged) == cur
    try:
        assert g.device == forged
        status.fill_(77)
        with pytest.raises(ValueError, match=f"handle lives on device {forged}, current device is {cur}"):
            call(torch.cuda.current_stream().cuda_stream)
        assert status.cpu().tolist() == [77] * n
    finally:
        assert lib.gtars_debug_set_assembly_device(g._h, cur) == forged
    call(torch.cuda.current_stream().cuda_stream)
    assert status.cpu().tolist() == st
