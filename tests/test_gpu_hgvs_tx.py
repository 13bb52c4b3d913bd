"""K23 on the device: the kernels of csrc/hgvs_tx.hip (span, the per-call mRNA image, the REF | ALT pool, K18 over the image)
against the plain-Python restatement (tests/hgvs_tx_ref.py) and against the library's host path, row by row and exactly.  The
roll across an exon junction on both strands -- on the lane path, on the wave path (GTARS_VRS_ROLL_CAP=2) and through K18's
host tail (GTARS_VRS_HOST_LEN=4) --, the transcript's ends with a homopolymer continuing in the neighbouring slots of the
image, every status, the batch shapes, the device entry on resident columns and 70,000 rows."""
import numpy as np
import pytest

import hgvs_ref as HR
import hgvs_tx_cases as K
import hgvs_tx_ref as TR
import vrs_ref as V
from test_hgvs_tx_cpu import ALLELE_ROWS, check_alleles, check_rows
from test_reftx_cpu import build_store
from test_vrs_cpu import write_fasta

pytestmark = pytest.mark.gpu
COLUMNS = ("statuses", "details", "warnings", "transcripts", "starts", "ends")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """(assembly, bound store, restatement transcripts, every expression, the restatement's rows for them)"""
    from gtars_amd import hgvs as H
    from gtars_amd.seqstats import GenomeAssembly

    d = tmp_path_factory.mktemp("hgvs_tx_gpu")
    write_fasta(d / "asm.fa", K.SEQS)
    txs = K.transcripts()
    genome = GenomeAssembly(str(d / "asm.fa"))
    strings = K.everything()
    return genome, H.BoundTxStore(genome, build_store(txs)), txs, strings, TR.bridge(K.SEQS, txs, strings)


def same(a, b):
    assert a["ids"] == b["ids"] and a["accessions"] == b["accessions"]
    for k in COLUMNS:
        assert np.array_equal(a[k], b[k]), k


def test_device_equals_restatement_and_host_path(world):
    from gtars_amd import hgvs as H

    genome, bound, _, strings, want = world
    got = H.hgvs_to_transcript_vrs_ids(genome, bound, strings)
    check_rows(got, want, bound.store, strings)
    same(got, H.hgvs_to_transcript_vrs_ids(genome, bound, strings, on_host=True))
    assert H.hgvs_to_transcript_vrs_id("NM_FWD.1:c.6C>A", genome, bound) == want[0]["id"] != H.hgvs_to_vrs_id("NM_FWD.1:c.6C>A", genome, bound)
    with pytest.raises(ValueError, match="is intronic or outside the mature mRNA"):
        H.hgvs_to_transcript_vrs_id("NM_FWD.1:c.8+1A>G", genome, bound)
    # orientation: an IUPAC alternate passes on the transcript, the genome path answers inconsistent edit
    assert H.hgvs_to_transcript_vrs_ids(genome, bound, ["NM_REV.1:c.3A>R"])["statuses"][0] == H.OK
    assert H.hgvs_to_vrs_ids(genome, bound, ["NM_REV.1:c.3A>R"])["statuses"][0] == H.INCONSISTENT_EDIT


def junction_and_ends(genome, bound):
    """the junction cases on both strands and the two ends between their neighbours: the stated values"""
    from gtars_amd import hgvs as H

    strings = ["NR_JUN.1:" + e for e, _, _, _ in K.JUNCTION] + ["NR_MIR.1:" + e for e, _, _, _ in K.JUNCTION]
    strings += K.NEIGHBOUR_ROWS[:12] + [s for s, _, _, _ in K.ENDS] + K.NEIGHBOUR_ROWS[12:]
    r = H.hgvs_to_transcript_vrs_ids(genome, bound, strings)
    jun, end = TR.accession_of(K.MRNA_JUNCTION), TR.accession_of(K.MRNA_ENDS)
    for k, (e, ns, ne, allele) in enumerate(K.JUNCTION + K.JUNCTION):
        assert (r["statuses"][k], r["starts"][k], r["ends"][k], r["ids"][k], r["accessions"][k]) == (0, ns, ne, V.vrs_id(jun, ns, ne, allele), jun), strings[k]
    for s, ns, ne, allele in K.ENDS:
        k = strings.index(s)
        assert (r["statuses"][k], r["starts"][k], r["ends"][k], r["ids"][k]) == (0, ns, ne, V.vrs_id(end, ns, ne, allele)), s
    nbr = TR.accession_of(b"AAAAAAAA")
    for k, s in enumerate(strings):
        if s.startswith("NR_NBR"):
            seq = b"A" * (9 if s.endswith("dup") else 7)
            assert (r["statuses"][k], r["starts"][k], r["ends"][k], r["ids"][k]) == (0, 0, 8, V.vrs_id(nbr, 0, 8, seq)), s


def test_roll_across_the_junction_and_at_the_ends(world):
    genome, bound, _, _, _ = world
    order = [bound.store.index_of(a) for a in K.NEIGHBOURS]
    assert min(order) < bound.store.index_of("NR_END.1") < max(order)  # slots on both sides continue the homopolymer
    junction_and_ends(genome, bound)


@pytest.mark.parametrize("switch,value", [("GTARS_VRS_ROLL_CAP", "2"), ("GTARS_VRS_HOST_LEN", "4"), ("GTARS_TX_HOST_LEN", "9")])
def test_roll_on_the_wave_path_and_through_the_host_tails(world, monkeypatch, switch, value):
    """ROLL_CAP 2 hands every roll to k_vrs_roll_long across the junction; VRS_HOST_LEN 4 hashes the alleles on the host threads
    from mRNAs derived there; TX_HOST_LEN 9 hashes the longer mRNAs of the image on the host threads"""
    from gtars_amd import hgvs as H

    genome, bound, _, strings, want = world
    monkeypatch.setenv(switch, value)
    junction_and_ends(genome, bound)
    check_rows(H.hgvs_to_transcript_vrs_ids(genome, bound, strings), want, bound.store, strings)


def test_batch_shapes(world):
    from gtars_amd import hgvs as H

    genome, bound, txs, _, _ = world
    r = H.hgvs_to_transcript_vrs_ids(genome, bound, [])
    assert r["ids"] == [] and all(len(r[k]) == 0 for k in r)
    failing = [s for s, st, _ in K.FAILURES + K.OTHERS if st != HR.OK]
    r = H.hgvs_to_transcript_vrs_ids(genome, bound, failing)  # no row passes: the image is empty
    check_rows(r, TR.bridge(K.SEQS, txs, failing), bound.store, failing)
    assert not any(r["ids"]) and (r["transcripts"] == 0xFFFFFFFF).all()
    mixed = ["NM_FWD.1:c.6C>A", "NM_FWD.1:c.6T>A", "NR_JUN.1:n.8_10del", "NM_NONE.1:c.6C>A", "NM_REV.1:c.3A>G", "NM_REV.1:c.8+1A>G"]
    check_rows(H.hgvs_to_transcript_vrs_ids(genome, bound, mixed), TR.bridge(K.SEQS, txs, mixed), bound.store, mixed)
    # a store bound for one expression only
    one = H.hgvs_to_transcript_vrs_ids(genome, bound.store, ["NR_END.1:n.7del"])
    assert (one["starts"][0], one["ends"][0]) == (5, 8)


def test_transcript_vrs_ids(world):
    from gtars_amd import vrs as VR

    genome, bound, txs, _, _ = world
    cols = list(zip(*ALLELE_ROWS))
    got = VR.transcript_vrs_ids(genome, bound, list(cols[0]), cols[1], cols[2], cols[3])
    check_alleles(got, txs)
    host = VR.transcript_vrs_ids(genome, bound, list(cols[0]), cols[1], cols[2], cols[3], on_host=True)
    assert got["ids"] == host["ids"] and got["accessions"] == host["accessions"]
    assert all(np.array_equal(got[k], host[k]) for k in ("statuses", "starts", "ends"))
    assert VR.transcript_vrs_ids(genome, bound, [], [], [], [])["ids"] == []


def _device_entry(genome, bound, strings, stream):
    import torch

    from gtars_amd import hgvs as H

    n = len(strings)
    cols = H.resolve(genome, bound, strings)
    dev = torch.device("cuda", torch.cuda.current_device())
    signed = {np.dtype(np.uint8): np.uint8, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64, np.dtype(np.int64): np.int64}
    resident = {name: torch.from_numpy(a.view(signed[a.dtype]).copy()).to(dev) for name, a in cols.items()}
    status, detail, warnings = (torch.full((n,), 77, dtype=torch.uint8, device=dev) for _ in range(3))
    tx = torch.zeros(n, dtype=torch.int32, device=dev)
    ns, ne = torch.full((n,), 7, dtype=torch.int64, device=dev), torch.full((n,), 7, dtype=torch.int64, device=dev)
    digests, anchors = torch.full((32 * n,), 9, dtype=torch.uint8, device=dev), torch.full((32 * n,), 9, dtype=torch.uint8, device=dev)
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        H.transcript_ids_device(genome, bound, {k: v.data_ptr() for k, v in resident.items()}, cols["text"].size, n, status.data_ptr(),
                                detail.data_ptr(), warnings.data_ptr(), tx.data_ptr(), ns.data_ptr(), ne.data_ptr(), digests.data_ptr(),
                                anchors.data_ptr(), stream.cuda_stream)
    raw, raw_a, st = digests.cpu().numpy().tobytes(), anchors.cpu().numpy().tobytes(), status.cpu().numpy()
    assert all(raw[32 * i:32 * i + 32] == bytes(32) == raw_a[32 * i:32 * i + 32] for i in range(n) if st[i] != 0)
    return {"ids": ["ga4gh:VA." + raw[32 * i:32 * i + 32].decode() if st[i] == 0 else None for i in range(n)],
            "accessions": ["SQ." + raw_a[32 * i:32 * i + 32].decode() if st[i] == 0 else None for i in range(n)],
            "statuses": st, "details": detail.cpu().numpy(), "warnings": warnings.cpu().numpy(), "transcripts": tx.cpu().numpy().view(np.uint32),
            "starts": ns.cpu().numpy().view(np.uint64), "ends": ne.cpu().numpy().view(np.uint64)}


def test_device_entry_on_resident_columns(world):
    """resolve() on the host, the columns uploaded by the test, the device entry on a side stream: the host-pointer call's results"""
    import torch

    from gtars_amd import hgvs as H

    genome, bound, _, strings, want = world
    got = _device_entry(genome, bound, strings, torch.cuda.Stream())
    check_rows(got, want, bound.store, strings)
    same(got, H.hgvs_to_transcript_vrs_ids(genome, bound, strings))
    H.transcript_ids_device(genome, bound, {k: 0 for k in list(dict(H.COLUMN_DTYPES)) + ["text"]}, 0, 0)  # n == 0 touches nothing


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257, 513])
def test_rows_at_the_wave_and_workgroup_edges(world, n):
    """the per-row kernels run one lane per row in workgroups of 256: batches that end just before, at and just behind a wave
    and a workgroup, the last row a passing one"""
    from gtars_amd import hgvs as H

    genome, bound, _, strings, want = world
    rows = [strings[(7 * k) % len(strings)] for k in range(n - 1)] + ["NR_JUN.1:n.8_10del"]
    got = H.hgvs_to_transcript_vrs_ids(genome, bound, rows)
    same(got, H.hgvs_to_transcript_vrs_ids(genome, bound, rows, on_host=True))
    assert (got["statuses"][-1], got["starts"][-1], got["ends"][-1]) == (0, 1, 13)


def test_70000_rows_equal_the_host_path(world):
    """more rows than a wave and a block hold, drawn from every fixture: the device against the host path row by row"""
    from gtars_amd import hgvs as H

    genome, bound, _, strings, _ = world
    rng = np.random.default_rng(23)
    rows = [strings[k] for k in rng.integers(0, len(strings), 70_000)]
    same(H.hgvs_to_transcript_vrs_ids(genome, bound, rows), H.hgvs_to_transcript_vrs_ids(genome, bound, rows, on_host=True))
