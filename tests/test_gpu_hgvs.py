"""K20 on the device (csrc/hgvs.hip, then csrc/vrs.hip) against the library's host path and the plain-Python restatement
(tests/hgvs_ref.py): exact equality of statuses, details, warnings, chromosomes, intervals and identifiers.  The 75 cases of the
reference's synthetic corpus in one launch; random expressions over random transcripts at the wave and block edges of a
lane-per-row kernel; failed and passing rows interleaved; spans at every offset of the fill kernel's eight-byte lanes and
across its 2048-byte workgroups and its grid stride; the host tail of K18; the last base of a chromosome that has a neighbour
behind it.  Nothing here provokes a fault: rows that point outside a chromosome are data the kernel answers with a status."""
import random

import numpy as np
import pytest

import hgvs_ref as HR
import reftx_ref as R
from test_hgvs_cpu import check_batch, golden_cases, golden_world, make_world, random_strings
from test_reftx_cpu import build_store
from test_vrs_cpu import write_fasta

pytestmark = pytest.mark.gpu

LANE, BLOCK = 8, 256 * 8             # output bytes per lane and per workgroup of k_hgvs_fill
GRID = 2048 * BLOCK                  # ... and per pass of its grid stride


def both(genome, store, strings, **kw):
    """the batch on the device and on the host path, equal in every column -> the device's"""
    from gtars_amd import hgvs as H

    dev, host = H.hgvs_to_vrs_ids(genome, store, strings, **kw), H.hgvs_to_vrs_ids(genome, store, strings, on_host=True, **kw)
    assert dev["ids"] == host["ids"]
    for key in ("statuses", "details", "warnings", "chroms", "starts", "ends"):
        assert dev[key].tolist() == host[key].tolist(), key
    assert genome.device >= 0 or not len(strings)  # (an empty batch touches nothing, the device image included)
    return dev


@pytest.fixture(scope="module")
def golden():
    from gtars_amd.seqstats import GenomeAssembly

    fa, seqs, txs = golden_world()
    return GenomeAssembly(fa), build_store(txs), golden_cases()


def test_golden_cases_in_one_launch(golden):
    from test_hgvs_cpu import NEGATIVE

    genome, store, cases = golden
    r = both(genome, store, [c["hgvs_string"] for c in cases])
    assert r["ids"] == [c["expected_vrs_id"] or None for c in cases]
    for k, c in enumerate(cases):
        if not c["expected_vrs_id"]:
            assert (r["statuses"][k], r["details"][k]) == NEGATIVE[c["hgvs_string"]], c["case_id"]
    assert sum(1 for x in r["ids"] if x) == 69


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from gtars_amd.reftx import BoundTxStore

    genome, store, seqs, txs, accessions, aliases, rng = make_world(tmp_path_factory.mktemp("hgvs_gpu"), 23)
    strings = random_strings(rng, seqs, txs, 3001, aliases)
    want = HR.bridge(seqs, accessions, txs, strings, aliases)  # computed once, shared, left unchanged
    assert {w["status"] for w in want} == set(range(12))
    return genome, BoundTxStore(genome, store), seqs, txs, accessions, aliases, strings, want


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 3001])
def test_batch_sizes(world, n):
    """the wave and block edges: the tail behind the last full block is where a lane-per-row kernel goes wrong"""
    genome, bound, seqs, _, accessions, aliases, strings, want = world
    # (the batches end at different rows of the shared list, so their tails differ)
    got = both(genome, bound, strings[-n:] if n else [], accessions=accessions, aliases=aliases)
    check_batch(got, want[-n:] if n else [], seqs, n)


def test_failed_and_passing_rows_interleaved(world):
    """a wrong pool offset behind a failed row would show as a wrong REF or ALT of the next passing one"""
    genome, bound, seqs, _, accessions, aliases, strings, want = world
    ok = [k for k, w in enumerate(want) if w["status"] == HR.OK and w["end"] > w["start"]][:200]
    bad = [k for k, w in enumerate(want) if w["status"] != HR.OK]
    by_status = {}
    for k in bad:
        by_status.setdefault(want[k]["status"], []).append(k)
    order, rng = [], random.Random(5)
    for j, k in enumerate(ok):
        order += [rng.choice(by_status[s]) for s in rng.sample(sorted(by_status), j % 4)]  # 0 .. 3 failed rows of different kinds
        order.append(k)
    order.append(bad[0])
    got = both(genome, bound, [strings[k] for k in order], accessions=accessions, aliases=aliases)
    check_batch(got, [want[k] for k in order], seqs)
    assert {want[k]["status"] for k in order} == set(range(12))


def test_every_row_fails_and_the_empty_batch(world):
    genome, bound, seqs, _, accessions, aliases, strings, want = world
    bad = [k for k, w in enumerate(want) if w["status"] not in (HR.OK, HR.NORMALIZE_ERROR)][:300]
    got = both(genome, bound, [strings[k] for k in bad], accessions=accessions, aliases=aliases)
    check_batch(got, [want[k] for k in bad], seqs)
    assert got["ids"] == [None] * len(bad) and not got["starts"].any() and (got["chroms"] == 0xFFFFFFFF).all()
    assert both(genome, bound, [])["ids"] == []


def test_k18_host_tail_switch_changes_nothing(world, monkeypatch):
    """GTARS_VRS_HOST_LEN 0 and 8: K18 hands the normalized sequences to the host threads; the bridge's columns are the same"""
    from gtars_amd import hgvs as H

    genome, bound, seqs, _, accessions, aliases, strings, want = world
    for host_len in ("0", "8"):
        monkeypatch.setenv("GTARS_VRS_HOST_LEN", host_len)
        check_batch(H.hgvs_to_vrs_ids(genome, bound, strings[:700], accessions=accessions, aliases=aliases), want[:700], seqs, host_len)


# ---- spans against the fill kernel's geometry ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fill_world(tmp_path_factory):
    """chrA: 24 kb of random bases in both cases; chrE: 37 bases, with chrN right behind it in the image; chrB: a reverse-strand
    and a forward-strand transcript"""
    from gtars_amd.reftx import BoundTxStore
    from gtars_amd.seqstats import GenomeAssembly

    rng = random.Random(24)
    seqs = {"chrA": bytes(rng.choice(b"ACGTACGTacgtN") for _ in range(24_000)), "chrE": bytes(rng.choice(b"ACGT") for _ in range(36)) + b"C",
            "chrN": b"GGGGGGGGGGGGGGGGTTTT", "chrB": bytes(rng.choice(b"ACGT") for _ in range(3_000))}
    own = R.refget_digests(seqs)
    dig = {k: R.digest_bytes(v) for k, v in own.items()}
    txs = [R.make_tx("NM_REV.1", dig["chrB"], -1, [(100, 400), (700, 1000), (1500, 1800)], (150, 1700), gene="REVG", mane=1),
           R.make_tx("NM_FWD.1", dig["chrB"], 1, [(2000, 2300), (2500, 2900)], (2050, 2800)),
           R.make_tx("NM_END.1", dig["chrE"], 1, [(10, 20), (30, 45)])]  # its last exon reaches past chrE's end
    d = tmp_path_factory.mktemp("hgvs_fill")
    write_fasta(d / "f.fa", seqs, width=70)
    genome = GenomeAssembly(str(d / "f.fa"))
    assert genome.chrom_names == list(seqs)
    return genome, BoundTxStore(genome, build_store(txs)), seqs, txs, own


def _check_fill(fill_world, strings):
    genome, bound, seqs, txs, own = fill_world
    want = HR.bridge(seqs, own, txs, strings)
    check_batch(both(genome, bound, strings), want, seqs)
    return want


def test_spans_at_every_lane_offset_and_across_workgroups(fill_world):
    """dups and identities of 1 .. 2049 bases whose first pool byte lies at offset 0 .. 7 of a lane's eight, some across the 2048
    bytes of a workgroup; an insertion in front of each pads the pool to the offset"""
    _, _, seqs, _, _ = fill_world
    strings, pool, offsets, crossings = [], 0, set(), 0
    lengths = [1, 7, 8, 9, 255, 256, 257, 681, 682, 683, 1023, 1024, 1025, 2047, 2048, 2049]
    for j, n in enumerate(lengths):
        for k in range(LANE):
            at = 1 + 37 * (j * LANE + k)
            pad = (k - pool - 1) % LANE + 1  # 1 .. 8 ALT bytes of an insertion
            strings.append(f"chrA:g.{at}_{at + 1}ins" + "ACGTTGCA"[:pad])
            pool += pad
            assert pool % LANE == k
            offsets.add(pool % LANE)
            edit, size = ("dup", 3 * n) if (j + k) % 2 else ("=", 2 * n)
            strings.append(f"chrA:g.{at + 5}{'' if n == 1 else '_%d' % (at + 4 + n)}{edit}")
            crossings += pool // BLOCK != (pool + size - 1) // BLOCK
            pool += size
    assert offsets == set(range(LANE)) and crossings > 40
    want = _check_fill(fill_world, strings)
    assert all(w["status"] == HR.OK for w in want)


def test_pool_longer_than_one_pass_of_the_grid(fill_world):
    """4,000 dups of 400 bases: 4.8 MB of REF and ALT, more than the 4 MiB the fill kernel's grid covers in one pass"""
    genome, bound, seqs, _, _ = fill_world
    strings = [f"chrA:g.{1 + 5 * k}_{400 + 5 * k}dup" for k in range(4_000)]
    assert 4_000 * 1_200 > GRID
    r = both(genome, bound, strings)
    assert (r["statuses"] == 0).all() and None not in r["ids"] and len(set(r["ids"])) > 3_900  # (two dups of a tandem repeat may be one allele)
    sample = list(range(0, 4_000, 333)) + [3_494, 3_495, 3_496, 3_999]  # (row 3,495 holds the grid's edge)
    _, _, _, txs, own = fill_world
    want = HR.bridge(seqs, own, txs, [strings[k] for k in sample])
    assert [r["ids"][k] for k in sample] == [w["id"] for w in want]


def test_dup_longer_than_the_host_length_of_k18(fill_world):
    """a dup of 6,000 bases: its normalized sequence is longer than GTARS_VRS_HOST_LEN (4096), so K18's host tail hashes it"""
    want = _check_fill(fill_world, ["chrA:g.101_6100dup", "chrA:g.5C>T", "chrA:g.9000_15000=", "chrA:g.7001_12999del"])
    assert want[0]["status"] == HR.OK and want[0]["end"] - want[0]["start"] >= 6_000


def test_reverse_strand_alternates_across_lanes(fill_world):
    """delins and ins on the reverse strand with ALTs of 1 .. 33 bytes: read backwards across the eight-byte lanes, at every offset"""
    strings = []
    for n in (1, 7, 8, 9, 15, 16, 17, 33):
        alt = "".join("ACGT"[(3 * i + n) % 4] for i in range(n))
        strings += [f"NM_REV.1:c.{5 + n}_{7 + n}delins{alt}", f"NM_REV.1:c.{40 + n}_{41 + n}ins{alt}N", f"REVG:c.-{n}delins{alt}",
                    f"NM_REV.1:c.200+{n}_201-{n}delins{alt}", f"NM_FWD.1:c.{5 + n}_{7 + n}delins{alt}", f"NM_REV.1:c.{5 + n}delins{alt}r"]
    want = _check_fill(fill_world, strings)
    assert [w["status"] for w in want[:5]] == [HR.OK] * 5 and want[5]["status"] == HR.INCONSISTENT_EDIT
    assert sum(w["status"] == HR.OK for w in want) == 40


def test_the_last_base_of_a_chromosome_with_a_neighbour(fill_world):
    """chrE ends with C and chrN, which starts with G, lies behind it in the image: a span that ends at chrE's last base passes, one
    a base longer is out of bounds, and the neighbour's bytes are never read as reference"""
    _, _, seqs, _, _ = fill_world
    assert seqs["chrE"][36:37] == b"C" and len(seqs["chrE"]) == 37
    last8 = seqs["chrE"][29:37].decode()
    strings = ["chrE:g.37=", "chrE:g.37C>T", "chrE:g.30_37dup", f"chrE:g.30_37del{last8}", "chrE:g.37_38insA", "chrE:g.37dup",  # inside
               "chrE:g.38=", "chrE:g.38G>T", "chrE:g.37_38del", "chrE:g.37_38delCG", "chrE:g.30_38dup", "chrE:g.38_39insA", "chrE:g.38dup",
               "chrE:g.37_53=", "NM_END.1:n.17=", "NM_END.1:n.18=", "NM_END.1:n.16_18del", "NM_END.1:n.10+17=", "NM_END.1:n.10+18="]
    want = _check_fill(fill_world, strings)
    assert [w["status"] for w in want] == [HR.OK] * 6 + [HR.OUT_OF_BOUNDS] * 8 + [HR.OK, HR.OUT_OF_BOUNDS, HR.OUT_OF_BOUNDS, HR.OK, HR.OUT_OF_BOUNDS]


def test_device_entry_on_resident_rows(world):
    """resolve() on the host, the columns uploaded by the test, the device entry on a side stream: the column call's results"""
    import torch

    from gtars_amd import hgvs as H

    genome, bound, seqs, _, accessions, aliases, strings, want = world
    strings, want = strings[:1500], want[:1500]
    n = len(strings)
    cols = H.resolve(genome, bound, strings, aliases=aliases)
    assert [name for name, _ in H.COLUMN_DTYPES] + ["text"] == list(cols)
    dev = torch.device("cuda", torch.cuda.current_device())
    signed = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64, np.dtype(np.int64): np.int64}
    resident = {name: torch.from_numpy(a.view(signed[a.dtype]).copy()).to(dev) for name, a in cols.items()}
    status, detail, warnings = (torch.full((n,), 77, dtype=torch.uint8, device=dev) for _ in range(3))
    chrom = torch.zeros(n, dtype=torch.int32, device=dev)
    ns, ne = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
    digests = torch.zeros(32 * n, dtype=torch.uint8, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        H.ids_device(genome, bound, {k: v.data_ptr() for k, v in resident.items()}, cols["text"].size, n, status.data_ptr(), detail.data_ptr(),
                     warnings.data_ptr(), chrom.data_ptr(), ns.data_ptr(), ne.data_ptr(), digests.data_ptr(), side.cuda_stream, accessions=accessions)
    raw = digests.cpu().numpy().tobytes()
    st = status.cpu().numpy()
    got = {"ids": ["ga4gh:VA." + raw[32 * i:32 * i + 32].decode() if st[i] == 0 else None for i in range(n)], "statuses": st,
           "details": detail.cpu().numpy(), "warnings": warnings.cpu().numpy(), "chroms": chrom.cpu().numpy().view(np.uint32),
           "starts": ns.cpu().numpy().view(np.uint64), "ends": ne.cpu().numpy().view(np.uint64)}
    check_batch(got, want, seqs)
    column_call = H.hgvs_to_vrs_ids(genome, bound, strings, accessions=accessions, aliases=aliases)
    assert got["ids"] == column_call["ids"] and got["chroms"].tolist() == column_call["chroms"].tolist()
    assert all(raw[32 * i:32 * i + 32] == bytes(32) for i in range(n) if st[i] != 0)
    H.ids_device(genome, bound, {k: 0 for k in cols}, 0, 0)  # n == 0 touches nothing
