"""K23 on the host: the plain-Python restatement (tests/hgvs_tx_ref.py) is checked against the reference's own answers
(bridge.rs:1046-1304) and against values that follow from vrs_ref.normalize over the mRNA alone; the library's host path
(gtars_amd.hgvs.hgvs_to_transcript_*, gtars_amd.vrs.transcript_vrs_ids, on_host) is checked against both, row by row and
exactly.  A stand-alone ASan/UBSan program over csrc/hgvs_tx_core.h."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import hgvs_ref as HR
import hgvs_tx_cases as K
import hgvs_tx_ref as TR
import reftx_ref as R
import vrs_ref as V
from test_reftx_cpu import build_store
from test_vrs_cpu import write_fasta

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from gtars_amd.seqstats import GenomeAssembly

    d = tmp_path_factory.mktemp("hgvs_tx_cpu")
    write_fasta(d / "asm.fa", K.SEQS)
    txs = K.transcripts()
    return GenomeAssembly(str(d / "asm.fa")), build_store(txs), txs


def check_rows(got, want, store, strings):
    """the library's batch result against the restatement's rows, exactly"""
    for k, (s, w) in enumerate(zip(strings, want)):
        assert (got["statuses"][k], got["details"][k], got["warnings"][k]) == (w["status"], w["detail"], w["warning"]), s
        assert (got["ids"][k], got["accessions"][k], got["starts"][k], got["ends"][k]) == (w["id"], w["accession"], w["start"], w["end"]), s
        assert got["transcripts"][k] == (store.index_of(w["tx"]) if w["tx"] else 0xFFFFFFFF), s


# ---- the restatement against known answers -------------------------------------------------------------------------------
def test_restatement_gives_the_reference_fixtures():
    txs = K.transcripts()
    for s, span in K.SPANS:
        got = TR.bridge_one(K.SEQS, txs, s)
        assert got["status"] == HR.OK and got["span"] == span, s
    for s, status, detail in K.FAILURES + K.OTHERS:
        got = TR.bridge_one(K.SEQS, txs, s)
        assert (got["status"], got["detail"]) == (status, detail), s
    assert TR.bridge_one(K.SEQS, txs, "NM_FWD.1:c.8+1A>G")["text"] == \
        "position 12 on NM_FWD.1 is intronic or outside the mature mRNA (no transcript-mRNA coordinate)"
    # the accession is "SQ." + digest(mature mRNA); the identifier is not the genome path's
    fwd = TR.bridge_one(K.SEQS, txs, "NM_FWD.1:c.6C>A")
    assert fwd["accession"] == "SQ." + V.sha512t24u(b"ACGTACGTTTAACCGG") and (fwd["start"], fwd["end"]) == (5, 6)
    assert fwd["id"] == V.vrs_id(fwd["accession"], 5, 6, b"A")
    assert fwd["id"] != HR.bridge_one(K.SEQS, R.refget_digests(K.SEQS), txs, "NM_FWD.1:c.6C>A")["id"]
    assert TR.bridge_one(K.SEQS, txs, "NM_FWD.1:c.(6C>A)")["warning"] == 1


def test_restatement_rolls_on_the_mrna_alone():
    txs = K.transcripts()
    assert R.mature(K.SEQS, R.lookup(txs, "NR_JUN.1")) == (R.SEQ_OK, K.MRNA_JUNCTION) == R.mature(K.SEQS, R.lookup(txs, "NR_MIR.1"))
    assert R.mature(K.SEQS, R.lookup(txs, "NR_END.1")) == (R.SEQ_OK, K.MRNA_ENDS)
    acc = TR.accession_of(K.MRNA_JUNCTION)
    for e, ns, ne, allele in K.JUNCTION:
        fwd, rev = TR.bridge_one(K.SEQS, txs, "NR_JUN.1:" + e), TR.bridge_one(K.SEQS, txs, "NR_MIR.1:" + e)
        assert (fwd["status"], fwd["start"], fwd["end"], fwd["id"]) == (HR.OK, ns, ne, V.vrs_id(acc, ns, ne, allele)), e
        assert {k: v for k, v in rev.items() if k != "tx"} == {k: v for k, v in fwd.items() if k != "tx"}, e
    # the chromosome would give another interval: the genome path rolls through the intron's bases
    g = HR.bridge_one(K.SEQS, R.refget_digests(K.SEQS), txs, "NR_JUN.1:n.5_7del")
    assert (g["status"], g["start"], g["end"]) == (HR.OK, 5, 17)
    for s, ns, ne, allele in K.ENDS:
        got = TR.bridge_one(K.SEQS, txs, s)
        assert (got["status"], got["start"], got["end"], got["id"]) == (HR.OK, ns, ne, V.vrs_id(TR.accession_of(K.MRNA_ENDS), ns, ne, allele)), s
    g = HR.bridge_one(K.SEQS, R.refget_digests(K.SEQS), txs, "NR_END.1:n.2del")
    assert (g["status"], g["start"], g["end"]) == (HR.OK, 0, 11)


# ---- the library's host path -----------------------------------------------------------------------------------------------
def test_host_path_equals_the_restatement(world):
    from gtars_amd import hgvs as H

    genome, store, txs = world
    strings = K.everything()
    got = H.hgvs_to_transcript_vrs_ids(genome, store, strings, on_host=True)
    assert set(got) == {"ids", "statuses", "details", "warnings", "transcripts", "accessions", "starts", "ends"}
    check_rows(got, TR.bridge(K.SEQS, txs, strings), store, strings)
    # a batch on fewer threads and a bound store that is kept give the same
    bound = H.BoundTxStore(genome, store)
    again = H.hgvs_to_transcript_vrs_ids(genome, bound, strings, on_host=True, threads=1)
    assert again["ids"] == got["ids"] and all(np.array_equal(again[k], got[k]) for k in ("statuses", "details", "starts", "ends", "transcripts"))


def test_host_path_known_answers(world):
    from gtars_amd import hgvs as H

    genome, store, _ = world
    acc = TR.accession_of(K.MRNA_JUNCTION)
    for tx in ("NR_JUN.1", "NR_MIR.1"):
        r = H.hgvs_to_transcript_vrs_ids(genome, store, [tx + ":" + e for e, _, _, _ in K.JUNCTION], on_host=True)
        for k, (e, ns, ne, allele) in enumerate(K.JUNCTION):
            assert (r["statuses"][k], r["starts"][k], r["ends"][k], r["ids"][k], r["accessions"][k]) == (0, ns, ne, V.vrs_id(acc, ns, ne, allele), acc), e
    # the ends: the neighbours of NR_END.1 in the store's order continue its homopolymer on both sides
    order = [store.index_of(a) for a in K.NEIGHBOURS]
    assert min(order) < store.index_of("NR_END.1") < max(order)
    strings = K.NEIGHBOUR_ROWS[:12] + [s for s, _, _, _ in K.ENDS] + K.NEIGHBOUR_ROWS[12:]
    r = H.hgvs_to_transcript_vrs_ids(genome, store, strings, on_host=True)
    for s, ns, ne, allele in K.ENDS:
        k = strings.index(s)
        assert (r["statuses"][k], r["starts"][k], r["ends"][k], r["ids"][k]) == (0, ns, ne, V.vrs_id(TR.accession_of(K.MRNA_ENDS), ns, ne, allele))
    # the transcript id is not the genome id
    assert H.hgvs_to_transcript_vrs_id("NM_FWD.1:c.6C>A", genome, store, on_host=True) != H.hgvs_to_vrs_id("NM_FWD.1:c.6C>A", genome, store, on_host=True)
    # orientation: an IUPAC alternate passes here, the genome path has to complement it and cannot
    assert H.hgvs_to_transcript_vrs_ids(genome, store, ["NM_REV.1:c.3A>R"], on_host=True)["statuses"][0] == H.OK
    assert H.hgvs_to_vrs_ids(genome, store, ["NM_REV.1:c.3A>R"], on_host=True)["statuses"][0] == H.INCONSISTENT_EDIT


def test_scalar_calls_and_their_errors(world):
    from gtars_amd import hgvs as H

    genome, store, txs = world
    for s, (start, end, alt) in K.SPANS:
        a = H.hgvs_to_transcript_allele(s, genome, store)
        mrna = R.mature(K.SEQS, R.lookup(txs, s.split(":")[0]))[1]
        assert a["location"]["sequenceReference"]["refgetAccession"] == TR.accession_of(mrna), s
        assert (a["location"]["start"], a["location"]["end"], a["state"]["sequence"]) == (start, end, alt.decode()), s
    assert H.hgvs_to_transcript_allele("NM_FWD.1:c.5_6dup", genome, store)["state"]["sequence"] == "ACAC"
    want = TR.bridge_one(K.SEQS, txs, "NR_JUN.1:n.8_10del")
    assert H.hgvs_to_transcript_vrs_id("NR_JUN.1:n.8_10del", genome, store, on_host=True) == want["id"]
    texts = {
        "NM_FWD.1:c.8+1A>G": "position 12 on NM_FWD.1 is intronic or outside the mature mRNA (no transcript-mRNA coordinate)",
        "NM_FWD.1:c.5+1A>G": "provider error: Mapping error: Intronic offset 1 at transcript position 5 is invalid (not at exon boundary)",
        "NM_FWD.1:c.1_5insAT": "inconsistent edit: ins range positions are not adjacent on the transcript: offsets 0 and 4",
        "NM_FWD.1:c.6T>A": "REF mismatch at NM_FWD.1:5: HGVS says T, sequence has C",
        "chrF:g.6C>A": "unsupported reference type: G (v1 supports g., c., n.)",
        "NM_FWD.1:c.5_6inv": "unsupported edit: inv",
        "NM_FWD.1:c.(4_5)_6insA": "unsupported edit: ins position range",
        "NM_NONE.1:c.6C>A": "provider error: Transcript not found: NM_NONE.1",
        "GENEB:c.6C>A": "provider error: No MANE Select transcript for gene: GENEB",
        "NM_NOCHR.1:c.3A>T": "refget error: Sequence not found: " + V.sha512t24u(b"no such chromosome"),
        "NM_UTR.1:c.*5G>T": "provider error: Mapping error: 3' UTR position c.*5 extends beyond transcript end",
    }
    for s, text in texts.items():
        for call in (lambda: H.hgvs_to_transcript_vrs_id(s, genome, store, on_host=True), lambda: H.hgvs_to_transcript_allele(s, genome, store)):
            with pytest.raises(ValueError) as e:
                call()
            assert str(e.value) == text and not isinstance(e.value, H.HgvsError), s
    with pytest.raises(ValueError, match="refget error: Transcript NR_PAST.1 has an exon past the end"):
        H.hgvs_to_transcript_vrs_id("NR_PAST.1:n.3A>T", genome, store, on_host=True)
    for call in (H.hgvs_to_transcript_vrs_id, H.hgvs_to_transcript_allele):
        with pytest.raises(H.HgvsError):
            call("NM_FWD.1:c.6C>", genome, store)
    import gtars.hgvs
    import gtars.vrs.hgvs

    assert gtars.vrs.hgvs.hgvs_to_transcript_vrs_id is H.hgvs_to_transcript_vrs_id is gtars.hgvs.hgvs_to_transcript_vrs_id


def test_batch_shapes_on_the_host(world):
    from gtars_amd import hgvs as H

    genome, store, txs = world
    r = H.hgvs_to_transcript_vrs_ids(genome, store, [], on_host=True)
    assert r["ids"] == [] and all(len(r[k]) == 0 for k in r)
    failing = [s for s, st, _ in K.FAILURES + K.OTHERS if st != HR.OK]
    r = H.hgvs_to_transcript_vrs_ids(genome, store, failing, on_host=True)  # no row passes: there is no mRNA to derive
    assert not any(r["ids"]) and (r["statuses"] != 0).all() and (r["transcripts"] == 0xFFFFFFFF).all() and not r["starts"].any()
    check_rows(r, TR.bridge(K.SEQS, txs, failing), store, failing)
    # 600 rows, more than a thread's block, that switch transcripts and fail in between
    strings = (K.everything() * 5)[:600]
    check_rows(H.hgvs_to_transcript_vrs_ids(genome, store, strings, on_host=True, threads=3), TR.bridge(K.SEQS, txs, strings), store, strings)


ALLELE_ROWS = [("NR_JUN.1", 4, b"CAG", b""), ("NR_JUN.1", 7, b"CAG", b""), ("NR_JUN.1", 10, b"CAG", b""), ("NR_JUN.1", 7, b"", b"CAG"),
               ("NR_MIR.1", 4, b"CAG", b""), ("NR_END.1", 1, b"A", b""), ("NR_END.1", 6, b"A", b""), ("NR_END.1", 3, b"c", b"T"),
               ("NR_JUN.1", 4, b"CAT", b""),          # REF mismatch
               ("NR_END.1", 9, b"", b"A"),            # a start past the transcript's end
               ("NR_END.1", 8, b"", b"A"),            # at the end: fine
               ("NR_END.1", 7, b"AA", b""),           # REF past the end
               ("NM_NONE.1", 0, b"A", b"T"), ("NM_NOCHR.1", 0, b"A", b"T"), ("NR_PAST.1", 0, b"A", b"T")]


def check_alleles(got, txs):
    want = TR.alleles(K.SEQS, txs, ALLELE_ROWS)
    for k, (st, ns, ne, vid, acc) in enumerate(want):
        assert (got["statuses"][k], got["starts"][k], got["ends"][k], got["ids"][k], got["accessions"][k]) == (st, ns, ne, vid, acc), ALLELE_ROWS[k]
    assert [w[0] for w in want[8:10]] == [V.REF_MISMATCH, V.REF_PAST_END] and want[10][0] == V.OK and want[11][0] == V.REF_PAST_END
    jun = TR.accession_of(K.MRNA_JUNCTION)
    assert [(w[1], w[2], w[3]) for w in want[:5]] == [(1, 13, V.vrs_id(jun, 1, 13, b"CAGCAGCAG"))] * 3 + \
        [(1, 13, V.vrs_id(jun, 1, 13, b"CAGCAGCAGCAGCAG")), (1, 13, V.vrs_id(jun, 1, 13, b"CAGCAGCAG"))]
    assert [(w[1], w[2]) for w in want[5:7]] == [(0, 3), (5, 8)]


def test_transcript_vrs_ids_on_the_host(world):
    from gtars_amd import vrs as VR

    genome, store, txs = world
    cols = list(zip(*ALLELE_ROWS))
    check_alleles(VR.transcript_vrs_ids(genome, store, list(cols[0]), cols[1], cols[2], cols[3], on_host=True), txs)
    # by number in the store
    idx = [store.index_of(a) if store.index_of(a) >= 0 else 0xFFFFFFFF for a in cols[0]]
    check_alleles(VR.transcript_vrs_ids(genome, store, idx, cols[1], cols[2], cols[3], on_host=True), txs)
    assert VR.transcript_vrs_ids(genome, store, [], [], [], [], on_host=True)["ids"] == []


def test_new_calls_need_a_device_unless_on_host(world):
    import gtars_amd
    from gtars_amd import hgvs as H
    from gtars_amd import vrs as VR

    if gtars_amd.device_count() > 0:
        pytest.skip("needs a box WITHOUT a GPU")
    genome, store, _ = world
    with pytest.raises(gtars_amd.NoDeviceError):
        H.hgvs_to_transcript_vrs_ids(genome, store, ["NM_FWD.1:c.6C>A"])
    with pytest.raises(gtars_amd.NoDeviceError):
        VR.transcript_vrs_ids(genome, store, ["NR_JUN.1"], [4], [b"CAG"], [b""])


def test_span_rules_under_the_sanitizers(tmp_path):
    """tests/soak/hgvs_tx_host_check.cpp, built with AddressSanitizer + UBSan: the span rules and the ins adjacency of
    csrc/hgvs_tx_core.h on the reference's fixtures, then random columns in and out of range over random transcripts with the
    chromosome, the text and the mRNA in exactly sized heap blocks."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "hgvs_tx_host_check"
    src = os.path.join(HERE, "soak", "hgvs_tx_host_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o",
                            str(exe), src], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("the host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe), "23"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "ok" in run.stdout
