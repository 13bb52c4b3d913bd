"""K19 on the device (csrc/reftx.hip) against the plain-Python restatement (tests/reftx_ref.py): exact equality of mapped
positions, statuses, mature sequences and digests.  The assembly is written by the test (about 10 kB): one chromosome of random
bases with soft-masked, N and IUPAC stretches, two neighbours of the packed image, a chromosome of length 1."""
import random

import numpy as np
import pytest

import reftx_ref as R
from test_reftx_cpu import build_store, random_queries, random_transcript, run_rows
from test_vrs_cpu import write_fasta

pytestmark = pytest.mark.gpu

C1_N = 9_001


def _make_sequences():
    rng = random.Random(19)
    c1 = bytearray(rng.choice(b"ACGT") for _ in range(C1_N))
    c1[300:340] = bytes(c1[300:340]).lower()                 # soft-masked
    c1[420:430] = b"N" * 10
    c1[500:516] = b"RYKMSWBDHVNrykmn"                        # IUPAC codes, some lower-case
    c1[0:4], c1[-4:] = b"GATC", b"CTAG"
    # e1 ends where e2 starts in the packed image (whole 16-byte lines, then the padding): an exon that ends at e1's last
    # base must not run on, one that starts at e2's first base must not reach back
    e1 = bytes(rng.choice(b"ACGT") for _ in range(40)) + b"ACGTACGT"
    e2 = b"ACGTACGT" + bytes(rng.choice(b"acgt") for _ in range(25))
    return {"c1": bytes(c1), "e1": e1, "e2": e2, "one": b"G"}


SEQS = _make_sequences()


def _split(total, parts, lo, hi, gap=3):
    """`parts` ascending disjoint exons inside [lo, hi) whose lengths add up to `total`"""
    sizes = [total // parts + (1 if k < total % parts else 0) for k in range(parts)]
    assert sum(sizes) + gap * parts <= hi - lo
    out, at = [], lo
    for n in sizes:
        out.append((at, at + n))
        at += n + gap
    return out


def _map_transcripts(d):
    three = [(100, 200), (300, 350), (400, 500)]
    many = [(20 * k + 5, 20 * k + 12) for k in range(200)]
    txs = []
    for sign, tag in ((1, "F"), (-1, "R")):
        txs += [R.make_tx(f"NM_3{tag}.1", d, sign, three, (150, 450), gene=f"G3{tag}", mane=1),
                R.make_tx(f"NM_EDGE{tag}.1", d, sign, three, (300, 350)),           # the CDS is exactly the middle exon
                R.make_tx(f"NM_WHOLE{tag}.1", d, sign, three, (100, 500)),          # ... starts and ends at the transcript's edges
                R.make_tx(f"NM_ONE{tag}.1", d, sign, [(50, 250)], (100, 200)),
                R.make_tx(f"NM_BASES{tag}.1", d, sign, [(10, 11), (20, 21), (30, 31)], (10, 31)),  # single-base exons
                R.make_tx(f"NM_SINGLEBASE{tag}.1", d, sign, [(77, 78)], (77, 78)),
                R.make_tx(f"NM_200{tag}.1", d, sign, many, (20 * 3 + 7, 20 * 190 + 9)),
                R.make_tx(f"NM_ZERO{tag}.1", d, sign, [(0, 0), (100, 150), (160, 160), (170, 220), (230, 230)], (120, 200)),
                R.make_tx(f"NM_LOW{tag}.1", d, sign, [(0, 3), (5, 9)], (0, 9)),     # offsets that fall below 0
                R.make_tx(f"NR_{tag}.1", d, sign, three),                           # non-coding
                R.make_tx(f"NM_INTRON{tag}.1", d, sign, three, (150, 250))]         # a CDS end in an intron: non-coding
    txs.append(R.make_tx("NM_BAD.1", d, 1, [(10, 20), (15, 30)], (12, 18)))
    txs.append(R.make_tx("NM_NONE.1", d, 1, []))
    return txs


def _map_rows(txs):
    rows = []
    for tx in txs:
        acc = tx["accession"]
        length = sum(e - s for s, e in tx["exons"]) if R.exons_ok(tx) else 10
        wide = length > 600
        step = 7 if wide else 1
        for pos in list(range(-length - 2, length + 3, step)) + [0, 1, -1, length, length + 1]:
            for star in (False, True):
                rows.append((acc, "c", pos, 0, star))
            rows.append((acc, "n", pos, 0, False))
            if not wide or pos % 5 == 0:
                for off in (1, -1):
                    rows.append((acc, "c", pos, off, False))
                    rows.append((acc, "n", pos, off, False))
                rows.append((acc, "c", pos, 2, True))
        if tx["exons"]:
            lo, hi = tx["exons"][0][0], tx["exons"][-1][1]
            for g in range(max(lo - 2, 0), hi + 2, step):
                rows.append((acc, "g", g, 0, False))
        # every exon boundary in transcript coordinates, as n. and as c. positions, with offsets that stay and that leave u64
        offs = R.exon_offsets(tx) if R.exons_ok(tx) else []
        bounds = R.cds_tx_bounds(tx, offs) if offs else None
        for ts, te, _, _ in offs:
            for anchor in (ts, te - 1):
                for off in (1, -1, 5, -5, 1 << 40, -(1 << 40), (1 << 63) - 1, -(1 << 63)):
                    rows.append((acc, "n", anchor + 1, off, False))
                    if bounds:
                        rows.append((acc, "c", anchor - bounds[0] + (1 if anchor >= bounds[0] else 0), off, False))
                        if anchor >= bounds[1]:
                            rows.append((acc, "c", anchor - bounds[1] + 1, off, True))
    rows += [("NM_NOPE.1", "c", 1, 0, False), ("NM_NOPE.1", "n", 1, 0, False), ("NM_NOPE.1", "g", 1, 0, False),
             ("NM_3F.1", "c", (1 << 63) - 1, 0, False), ("NM_3F.1", "c", -(1 << 63), 0, False), ("NM_3F.1", "c", (1 << 63) - 1, 0, True),
             ("NM_3F.1", "n", (1 << 63) - 1, 0, False), ("NM_3F.1", "g", (1 << 64) - 1, 0, False), ("NM_3F.1", "g", 1 << 32, 0, False)]
    return rows


def _seq_transcripts(acc):
    c1, e1, e2, one = (R.digest_bytes(acc[k]) for k in ("c1", "e1", "e2", "one"))
    txs = []
    k = 0
    for total in (1, 111, 112, 127, 128, 129, 8191, 8192, 8193, 239, 240, 255, 256, 257):  # SHA-512 padding and block edges
        for sign in (1, -1):
            parts = 1 if total == 1 else 3 if total < 1000 else 7
            txs.append(R.make_tx(f"NM_LEN{total}_{'F' if sign > 0 else 'R'}.1", c1, sign, _split(total, parts, 600 + 5 * k, C1_N - 1 + (total > 8000))))
            k += 1
    for n in range(1, 17):  # rows that start at every offset of the fill kernel's eight bytes
        txs.append(R.make_tx(f"NM_ROW{n}.1", c1, 1 if n % 3 else -1, [(1000 + 20 * n, 1000 + 20 * n + n)]))
    n1, n2 = len(SEQS["e1"]), len(SEQS["e2"])
    txs += [R.make_tx("NM_SEAM1F.1", e1, 1, [(0, 5), (n1 - 8, n1)]), R.make_tx("NM_SEAM1R.1", e1, -1, [(3, 9), (n1 - 1, n1)]),
            R.make_tx("NM_SEAM2F.1", e2, 1, [(0, 8), (n2 - 4, n2)]), R.make_tx("NM_SEAM2R.1", e2, -1, [(0, 1), (10, n2)]),
            R.make_tx("NM_WHOLE1.1", e1, -1, [(0, n1)]), R.make_tx("NM_ONE.1", one, 1, [(0, 1)]), R.make_tx("NM_ONER.1", one, -1, [(0, 1)]),
            R.make_tx("NM_SOFTF.1", c1, 1, [(290, 350), (410, 440)]), R.make_tx("NM_SOFTR.1", c1, -1, [(290, 350), (410, 440)]),
            R.make_tx("NM_IUPACF.1", c1, 1, [(495, 520)]), R.make_tx("NM_IUPACR.1", c1, -1, [(495, 508), (508, 520)]),
            R.make_tx("NM_ZEROF.1", c1, 1, [(700, 700), (710, 720), (725, 725), (730, 745), (750, 750)]),
            R.make_tx("NM_ZEROR.1", c1, -1, [(710, 720), (725, 725), (730, 745)]),
            R.make_tx("NM_EMPTY.1", bytes(24), 1, []), R.make_tx("NM_ALLEMPTY.1", bytes(24), -1, [(5, 5), (9, 9)]),
            R.make_tx("NM_LOST.1", bytes([9]) * 24, 1, [(0, 10)]),                       # a chromosome the assembly lacks
            R.make_tx("NM_PAST.1", one, 1, [(0, 1), (1, 2)]),                            # an exon past the chromosome's end
            R.make_tx("NM_PASTR.1", c1, -1, [(10, 20), (C1_N - 1, C1_N + 1)]),
            R.make_tx("NM_LASTBASE.1", c1, -1, [(10, 20), (C1_N - 1, C1_N)]),
            R.make_tx("NM_BAD.1", c1, 1, [(10, 20), (15, 30)])]
    return txs


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from gtars_amd.seqstats import BinaryGenomeAssembly, GenomeAssembly, write_fab

    d = tmp_path_factory.mktemp("reftx_gpu")
    write_fasta(d / "asm.fa", SEQS, width=61)
    write_fab(str(d / "asm.fa"), str(d / "asm.fab"))
    fasta, fab = GenomeAssembly(str(d / "asm.fa")), BinaryGenomeAssembly(str(d / "asm.fab"))
    acc = R.refget_digests(SEQS)
    assert fasta.refget_digests() == acc
    return (fasta, fab), acc


@pytest.fixture(scope="module")
def map_world(world):
    """(transcripts, rows in a fixed shuffled order, the restatement's values and statuses, the library's store)"""
    txs = _map_transcripts(R.digest_bytes(world[1]["c1"]))
    rng = random.Random(5)
    txs += [random_transcript(rng, f"NM_RND{k}.1", bytes(24), rng.choice([60, 400, 5000])) for k in range(30)]
    rows = _map_rows(txs[:24]) + random_queries(rng, txs, 3000)
    rng.shuffle(rows)
    return txs, rows, R.map_rows(txs, rows), build_store(txs)


def test_mapping_every_case_and_error_kind(world, map_world):
    from gtars_amd import reftx as T

    txs, rows, want, store = map_world
    assert set(want[1]) == set(range(11)) - {R.BAD_KIND}  # every error kind, failing rows between good ones
    for genome in world[0]:
        mapper = T.CoordinateMapper(store, genome)
        assert run_rows(mapper, rows) == want
        assert genome.device >= 0
    assert run_rows(T.CoordinateMapper(store), rows, on_host=True) == want
    # a few of the cases by hand: c.-N at the 5' UTR's length and one past it, c.*N at the last base and one past it, c.0
    by = {(r[0], r[1], r[2], r[3], r[4]): (v, s) for r, v, s in zip(rows, *want)}
    assert by[("NM_3F.1", "c", -50, 0, False)] == (100, R.OK) and by[("NM_3F.1", "c", -51, 0, False)] == (0, R.UTR5_OVERFLOW)
    assert by[("NM_3F.1", "c", 50, 0, True)] == (499, R.OK) and by[("NM_3F.1", "c", 51, 0, True)] == (0, R.UTR3_OVERFLOW)
    assert by[("NM_3R.1", "c", 1, 0, False)] == (449, R.OK) and by[("NM_3R.1", "c", -50, 0, False)] == (499, R.OK)
    assert by[("NM_3F.1", "c", 0, 0, False)] == (0, R.OUTSIDE_CDS)
    assert by[("NM_3F.1", "c", 50, 1, False)] == (200, R.OK) and by[("NM_3F.1", "c", 51, -1, False)] == (299, R.OK)   # c.50+1, c.51-1
    assert by[("NM_3R.1", "c", 50, 1, False)] == (399, R.OK) and by[("NM_3R.1", "c", 51, -1, False)] == (350, R.OK)
    assert by[("NM_3F.1", "c", 50, -1, False)] == (0, R.INVALID_OFFSET) and by[("NM_3F.1", "n", 250, 1, False)] == (0, R.INVALID_OFFSET)  # the last exon's last base
    assert by[("NM_LOWF.1", "n", 4, -5, False)] == (0, R.OK) and by[("NM_LOWF.1", "n", 4, -(1 << 40), False)] == (0, R.INVALID_OFFSET)
    assert by[("NM_200F.1", "n", 7 * 199 + 1, -1, False)] == (20 * 199 + 4, R.OK) and by[("NM_200R.1", "n", 1, 0, False)] == (20 * 199 + 11, R.OK)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_mapping_batch_sizes(world, map_world, n):
    from gtars_amd import reftx as T

    txs, rows, want, store = map_world
    sub = [r for r in rows if r[1] == "c"][:n]
    mapper = T.CoordinateMapper(store, world[0][0])
    values, status = mapper.c_to_g_many([r[0] for r in sub], [r[2] for r in sub], [r[3] for r in sub], [1 if r[4] else 0 for r in sub])
    assert (values.tolist(), status.tolist()) == R.map_rows(txs, sub) and len(values) == n


@pytest.fixture(scope="module")
def seq_world(world):
    """(transcripts, the library's store, per transcript of the store's order: the restatement's status and sequence)"""
    txs = _seq_transcripts(world[1])
    store = build_store(txs)
    order = [R.lookup(txs, store.transcript(i).accession) for i in range(len(store))]
    return txs, store, order, [R.mature(SEQS, tx) for tx in order]


def _check_sequences(genome, store, order, want, **kw):
    from gtars_amd import reftx as T

    seqs, status = T.mature_mrnas(genome, store, with_status=True, **kw)
    assert status.tolist() == [st for st, _ in want]
    assert seqs == [s.decode() if st == R.SEQ_OK else None for st, s in want]
    ids = T.transcript_accessions(genome, store, **kw)
    assert ids == {tx["accession"]: "SQ." + R.sha512t24u(s) for tx, (st, s) in zip(order, want) if st == R.SEQ_OK}
    return seqs, ids


def test_sequences_and_digests(world, seq_world):
    from gtars_amd import reftx as T

    txs, store, order, want = seq_world
    by = {tx["accession"]: w for tx, w in zip(order, want)}
    assert {len(s) for st, s in want if st == R.SEQ_OK} >= {0, 1, 111, 112, 127, 128, 129, 8191, 8192, 8193} | set(range(1, 17))
    assert {st for st, _ in want} == {R.SEQ_OK, R.SEQ_NO_SEQUENCE, R.SEQ_PAST_END, R.SEQ_BAD_EXONS}
    # what the byte rule says: forward keeps IUPAC codes upper-cased, reverse turns everything outside ACGTN into N
    assert by["NM_IUPACF.1"][1] == SEQS["c1"][495:520].upper() and b"R" in by["NM_IUPACF.1"][1] and b"r" not in by["NM_IUPACF.1"][1]
    assert set(by["NM_IUPACR.1"][1][4:20]) == {ord("N")} and by["NM_SOFTF.1"][1] == (SEQS["c1"][290:350] + SEQS["c1"][410:440]).upper()
    assert by["NM_SEAM1F.1"][1] == SEQS["e1"][:5] + b"ACGTACGT" and by["NM_EMPTY.1"] == (R.SEQ_OK, b"") and by["NM_ALLEMPTY.1"] == (R.SEQ_OK, b"")
    for genome in world[0]:
        _check_sequences(genome, store, order, want)
        assert genome.device >= 0
    _check_sequences(world[0][0], store, order, want, on_host=True)
    # a batch by accession: unknown ones and failing rows between good ones, repeated rows
    names = ["NM_LEN129_R.1", "NM_NOPE.1", "NM_LOST.1", "NM_ROW5.1", "NM_PAST.1", "NM_LEN129_R.1", "NM_BAD.1", "NM_LASTBASE.1", "NM_PASTR.1"]
    seqs, status = T.mature_mrnas(world[0][0], store, names, with_status=True)
    assert status.tolist() == [0, 1, 2, 0, 3, 0, 4, 0, 3]
    assert seqs == [by[a][1].decode() if st == 0 else None for a, st in zip(names, status.tolist())]
    assert T.mature_mrna(world[0][0], store, "NM_SEAM2R.1") == by["NM_SEAM2R.1"][1].decode()
    with pytest.raises(ValueError, match="^Transcript not found: NM_NOPE.1$"):
        T.mature_mrna(world[0][0], store, "NM_NOPE.1")
    with pytest.raises(ValueError, match="^Sequence not found: " + "CQkJ" * 8 + "$"):
        T.mature_mrna(world[0][0], store, "NM_LOST.1")
    assert T.mature_mrnas(world[0][0], store, []) == []


def test_host_tail_gives_the_same_digests(world, seq_world, monkeypatch):
    """GTARS_TX_HOST_LEN 0 (every non-empty transcript is hashed by the host threads), 8, and larger than every transcript"""
    txs, store, order, want = seq_world
    seen = []
    for host_len in ("0", "8", str(1 << 20)):
        monkeypatch.setenv("GTARS_TX_HOST_LEN", host_len)
        seen.append(_check_sequences(world[0][0], store, order, want)[1])
    assert seen[0] == seen[1] == seen[2]


def test_device_entries_on_a_stream_and_a_forged_device(world, map_world, seq_world):
    import torch

    from gtars_amd import reftx as T
    from gtars_amd._lib import lib

    g = world[0][0]
    txs, rows, want, store = map_world
    rows = rows[:1000]
    bound = T.BoundTxStore(g, store)
    dev = torch.device("cuda", torch.cuda.current_device())
    n = len(rows)
    signed = lambda v: v - (1 << 64) if v >= 1 << 63 else v  # noqa: E731

    def put(values, np_dtype, as_dtype):
        return torch.from_numpy(np.array(values, dtype=np_dtype).view(as_dtype).copy()).to(dev)

    tx = put(store.indices_of([r[0] for r in rows]), np.uint32, np.int32)
    kind = put(["cng".index(r[1]) for r in rows], np.uint8, np.uint8)
    pos = put([signed(r[2]) for r in rows], np.int64, np.int64)
    off = put([r[3] for r in rows], np.int64, np.int64)
    star = put([1 if r[4] else 0 for r in rows], np.uint8, np.uint8)
    out = torch.zeros(n, dtype=torch.int64, device=dev)
    status = torch.full((n,), 77, dtype=torch.uint8, device=dev)

    def call(stream):
        bound.map_device(tx.data_ptr(), kind.data_ptr(), pos.data_ptr(), off.data_ptr(), star.data_ptr(), n, out.data_ptr(), status.data_ptr(), stream)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(side.cuda_stream)
    assert (out.cpu().numpy().view(np.uint64).tolist(), status.cpu().tolist()) == (want[0][:n], want[1][:n])
    # the digests of a device column of transcript numbers
    stxs, sstore, order, swant = seq_world
    sbound = T.BoundTxStore(g, sstore)
    m = len(order)
    numbers = list(range(m)) + [0xFFFFFFFF, m]
    idx = put(numbers, np.uint32, np.int32)
    d_status = torch.full((m + 2,), 77, dtype=torch.uint8, device=dev)
    digests = torch.full((32 * (m + 2),), 1, dtype=torch.uint8, device=dev)
    with torch.cuda.stream(side):
        sbound.digests_device(idx.data_ptr(), m + 2, d_status.data_ptr(), digests.data_ptr(), side.cuda_stream)
    raw = digests.cpu().numpy().tobytes()
    assert d_status.cpu().tolist() == [st for st, _ in swant] + [R.SEQ_NOT_FOUND] * 2
    for i, (st, s) in enumerate(swant + [(1, b"")] * 2):
        assert raw[32 * i:32 * i + 32] == (R.sha512t24u(s).encode() if st == R.SEQ_OK else bytes(32))
    # n == 0 touches nothing
    bound.map_device(0, 0, 0, 0, 0, 0, 0, 0)
    sbound.digests_device(0, 0, 0, 0)
    # the calls run on the assembly's device or are refused
    cur = torch.cuda.current_device()
    forged = cur + 1
    assert lib.gtars_debug_set_assembly_device(g._h, forged) == cur
    try:
        status.fill_(77)
        d_status.fill_(77)
        with pytest.raises(ValueError, match=f"handle lives on device {forged}, current device is {cur}"):
            call(torch.cuda.current_stream().cuda_stream)
        with pytest.raises(ValueError, match=f"handle lives on device {forged}, current device is {cur}"):
            sbound.digests_device(idx.data_ptr(), m + 2, d_status.data_ptr(), digests.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert status.cpu().tolist() == [77] * n and d_status.cpu().tolist() == [77] * (m + 2)
    finally:
        assert lib.gtars_debug_set_assembly_device(g._h, cur) == forged
    call(torch.cuda.current_stream().cuda_stream)
    assert status.cpu().tolist() == want[1][:n]
