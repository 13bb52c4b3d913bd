"""K19 on the host: the plain-Python restatement (tests/reftx_ref.py) and the library's host calls (gtars_amd.reftx, on_host)
are both checked against the reference's known answers -- the cases of gtars-python/tests/test_reftx.py, the
g_to_transcript_offset tables of mapper.rs:501-553, the n.0 error of store.rs:779, the sequence tests of sequence.rs:179 ff.
and the golden .reftx image of store.rs:838-930 (tests/golden/reftx/golden_v2.reftx: the bytes of that test) -- then against
each other on random stores.  Corrupt stores, hand-written cdot and MANE files, and a stand-alone ASan/UBSan program."""
import gzip
import json
import os
import random
import shutil
import subprocess

import pytest

import reftx_ref as R
from test_vrs_cpu import write_fasta

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "reftx", "golden_v2.reftx")


def _chrom_accession(seq: bytes = b"A" * 100) -> str:
    return "SQ." + R.sha512t24u(seq)


def _tx_dict(tx):
    """a restatement transcript as the dict add_transcript takes"""
    return {"accession": tx["accession"], "gene": tx["gene"] or None, "chrom": R.accession_of(tx["digest"]), "strand": "+" if tx["strand"] > 0 else "-",
            "cds_start": tx["cds_start"], "cds_end": tx["cds_end"], "exons": list(tx["exons"]),
            "mane": {"select": bool(tx["mane"] & 1), "plus_clinical": bool(tx["mane"] & 2)} if tx["mane"] else None}


def build_store(transcripts):
    """the library's store of restatement transcripts, through the builder and the image"""
    from gtars_amd import reftx as T

    b = T.TxStoreBuilder()
    for tx in transcripts:
        b.add_transcript(_tx_dict(tx))
    return T.ReadonlyTxStore.from_bytes(b.to_bytes())


def _simple(tmp_path, mane=False, plus=True):
    from gtars_amd import reftx as T

    chrom_acc = _chrom_accession()
    b = T.TxStoreBuilder()
    b.add_transcript({"accession": "NM_TEST.1", "gene": "TEST", "chrom": chrom_acc, "strand": "+" if plus else "-", "cds_start": 100,
                      "cds_end": 200, "exons": [(50, 250)], "mane": {"select": True, "plus_clinical": False} if mane else None})
    out = str(tmp_path / "test.reftx")
    b.build(out)
    return T.ReadonlyTxStore.open(out), chrom_acc


# ---- the cases of gtars-python/tests/test_reftx.py ---------------------------------------------------------------------
def test_builder_roundtrip(tmp_path):
    from gtars_amd import reftx as T

    chrom_acc = _chrom_accession()
    b = T.TxStoreBuilder()
    b.add_transcript({"accession": "NM_A.1", "gene": "A", "chrom": chrom_acc, "strand": "+", "cds_start": 100, "cds_end": 200, "exons": [(50, 250)]})
    b.add_transcript({"accession": "NM_B.1", "gene": "B", "chrom": chrom_acc, "strand": "-", "cds_start": 1000, "cds_end": 1100,
                      "exons": [(900, 1200)]})
    assert len(b) == 2
    out = tmp_path / "two.reftx"
    b.build(str(out))
    assert sorted(os.listdir(tmp_path)) == ["two.reftx"]  # the temporary file took the name
    store = T.ReadonlyTxStore.open(str(out))
    assert len(store) == 2
    a = store.lookup("NM_A.1")
    assert (a.accession, a.gene, a.strand) == ("NM_A.1", "A", T.Strand.Plus)
    assert (a.transcript_length, a.cds_length, a.is_coding) == (200, 100, True)
    assert store.lookup("NM_B.1").strand == T.Strand.Minus and store.get_strand("NM_B.1") == T.Strand.Minus
    assert store.lookup("NM_NOPE.1") is None and store.get_chrom_accession("NM_NOPE.1") is None
    assert store.get_chrom_accession("NM_A.1") == chrom_acc
    # the restatement reads the same file
    txs, has_mane = R.decode(out.read_bytes())
    assert sorted(t["accession"] for t in txs) == ["NM_A.1", "NM_B.1"] and not has_mane
    assert R.encode(txs) == out.read_bytes()
    with pytest.raises(T.TxStoreError, match="No transcripts to write"):
        T.TxStoreBuilder().build(str(tmp_path / "none.reftx"))


def test_mane_index_and_by_gene(tmp_path):
    from gtars_amd import reftx as T

    store, _ = _simple(tmp_path, mane=True)
    assert store.has_mane_index()
    tx = store.lookup_mane("TEST")
    assert tx.accession == "NM_TEST.1" and tx.mane is not None and tx.mane.select and not tx.mane.plus_clinical
    assert store.lookup_mane("test").accession == "NM_TEST.1" and store.lookup_mane("OTHER") is None
    full = T.CoordinateMapper(store).c_to_g_by_gene("TEST", 1)
    assert full["accession"] == "NM_TEST.1" and full["genomic_pos"] == 100
    with pytest.raises(T.MappingError, match="No MANE Select transcript for gene: NOPE"):
        T.CoordinateMapper(store).c_to_g_by_gene("NOPE", 1)
    plain, _ = _simple(tmp_path, mane=False)
    assert not plain.has_mane_index() and plain.lookup_mane("TEST") is None


def test_coordinate_mapper_known_answers(tmp_path):
    from gtars_amd import reftx as T

    store, chrom_acc = _simple(tmp_path)
    m = T.CoordinateMapper(store)
    assert m.c_to_g("NM_TEST.1", 1) == 100 and m.c_to_g("NM_TEST.1", 50) == 149
    full = m.c_to_g_full("NM_TEST.1", 1)
    assert set(full) >= {"chrom", "chrom_accession", "genomic_pos", "strand"}
    assert (full["chrom_accession"], full["genomic_pos"], full["strand"]) == (chrom_acc, 100, T.Strand.Plus)
    assert m.n_to_g_full("NM_TEST.1", 1)["genomic_pos"] == 50
    # datum=1 -> c.*N: the base behind the CDS end; 5' UTR; the error kinds' texts
    assert m.c_to_g("NM_TEST.1", 1, datum=1) == 200 and m.c_to_g("NM_TEST.1", 50, datum=1) == 249 and m.c_to_g("NM_TEST.1", -50) == 50
    for call, text in [(lambda: m.c_to_g("NM_NOPE.1", 1), "Transcript not found: NM_NOPE.1"),
                       (lambda: m.c_to_g("NM_TEST.1", 101), "Position 101 is outside CDS"),
                       (lambda: m.c_to_g("NM_TEST.1", 0), "Position 0 is outside CDS"),
                       (lambda: m.c_to_g("NM_TEST.1", -51), "5' UTR position c.-51 extends beyond transcript start"),
                       (lambda: m.c_to_g("NM_TEST.1", 51, datum=1), r"3' UTR position c.\*51 extends beyond transcript end"),
                       (lambda: m.n_to_g("NM_TEST.1", 0), "Position 0 is outside transcript"),  # store.rs:779
                       (lambda: m.n_to_g("NM_TEST.1", 201), "Position 201 is outside transcript"),
                       (lambda: m.c_to_g("NM_TEST.1", 5, offset=2), r"Intronic offset 2 at transcript position 5 is invalid \(not at exon boundary\)")]:
        with pytest.raises(T.MappingError, match=text):
            call()
    # the restatement gives the same answers
    tx = R.make_tx("NM_TEST.1", R.digest_bytes(chrom_acc), 1, [(50, 250)], (100, 200))
    assert R.c_to_g(tx, 1) == (R.OK, 100) and R.c_to_g(tx, 50) == (R.OK, 149) and R.c_to_g(tx, 1, star=True) == (R.OK, 200)
    assert R.n_to_g(tx, 0) == (R.OUTSIDE_TRANSCRIPT, 0) and R.c_to_g(None, 1) == (R.NOT_FOUND, 0)
    # c.1 of a reverse-strand gene is the last CDS base, not the stop codon's end of the interval
    rev, _ = _simple(tmp_path, plus=False)
    assert T.CoordinateMapper(rev).c_to_g("NM_TEST.1", 1) == 199 and T.CoordinateMapper(rev).c_to_g("NM_TEST.1", 100) == 100
    assert R.c_to_g(dict(tx, strand=-1), 1) == (R.OK, 199)


def test_small_classes_and_dicts(tmp_path):
    from gtars_amd import reftx as T

    assert T.Strand.from_str("+") == T.Strand.Plus and T.Strand.from_str("-") == T.Strand.Minus and T.Strand.from_str("-1") == T.Strand.Minus
    with pytest.raises(ValueError):
        T.Strand.from_str("?")
    assert str(T.Strand.Minus) == "-" and repr(T.Strand.Plus) == "Strand.Plus"
    assert T.Exon(start=10, end=20).to_dict() == {"start": 10, "end": 20}
    assert T.ManeStatus(select=True, plus_clinical=False).to_dict() == {"select": True, "plus_clinical": False}
    store, chrom_acc = _simple(tmp_path, mane=True)
    d = store.lookup("NM_TEST.1").to_dict()
    assert set(d) == {"accession", "gene", "chrom", "strand", "cds_start", "cds_end", "exons", "mane"}
    assert (d["accession"], d["chrom"], d["strand"], d["cds_start"], d["exons"]) == ("NM_TEST.1", chrom_acc, "+", 100, [{"start": 50, "end": 250}])
    assert d["mane"] == {"select": True, "plus_clinical": False}
    b = T.TxStoreBuilder()
    b.add_transcript(store.lookup("NM_TEST.1"))  # a Transcript goes back in
    assert T.ReadonlyTxStore.from_bytes(b.to_bytes()).lookup("NM_TEST.1").to_dict() == d
    with pytest.raises(T.TxStoreError, match="Invalid base64url chrom accession"):
        b.add_transcript({"accession": "NM_X.1", "chrom": "SQ.notbase64!!!", "strand": "+", "exons": [(0, 10)]})
    with pytest.raises(T.TxStoreError, match="Chrom accession must decode to 24 bytes, got 3"):
        b.add_transcript({"accession": "NM_X.1", "chrom": "SQ.QUJD", "strand": "+", "exons": [(0, 10)]})
    with pytest.raises(KeyError):
        b.add_transcript({"accession": "NM_X.1", "chrom": chrom_acc, "exons": [(0, 10)]})
    with pytest.raises(ValueError):
        b.add_transcript({"accession": "NM_X.1", "chrom": chrom_acc, "strand": "0", "exons": [(0, 10)]})
    with pytest.raises(TypeError):
        b.add_transcript(["NM_X.1"])
    assert len(b) == 1


def test_g_to_transcript_offset_tables():
    """mapper.rs:501-553"""
    from gtars_amd import reftx as T

    digest = bytes(24)
    fwd = R.make_tx("NM_F.1", digest, 1, [(10, 14), (20, 24)], gene="G")
    rev = R.make_tx("NM_R.1", digest, -1, [(10, 14), (20, 24)], gene="G")
    m = T.CoordinateMapper(build_store([fwd, rev]))
    for acc, tx, table in [("NM_F.1", fwd, {10: 0, 13: 3, 20: 4, 23: 7, 16: None, 0: None}),
                           ("NM_R.1", rev, {23: 0, 20: 3, 13: 4, 10: 7, 16: None})]:
        for g, want in table.items():
            assert m.g_to_transcript_offset(acc, g) == want
            assert R.g_to_tx(tx, g) == ((R.OK, want) if want is not None else (R.NOT_EXONIC, 0))
    with pytest.raises(T.MappingError):
        m.g_to_transcript_offset("NM_MISSING.1", 0)
    values, status = m.g_to_transcript_offset_many(["NM_F.1", "NM_MISSING.1", "NM_R.1", "NM_F.1"], [13, 0, 13, 16], on_host=True)
    assert values.tolist() == [3, 0, 4, 0] and status.tolist() == [R.OK, R.NOT_FOUND, R.OK, R.NOT_EXONIC]
    with pytest.raises(ValueError, match="on_host=True"):
        m.g_to_transcript_offset_many(["NM_F.1"], [13])


# ---- sequences: sequence.rs:179 ff. ---------------------------------------------------------------------------------------
SEQ_CHROMS = {"chrFwd": b"ATCGATCGATCGATCGATCGATCGATCGATCG", "chrRev": b"ACGTTTAAGGCCAACCGGTT", "chrSingle": b"AAACCCGGGTTT",
              "chrSoft": b"acgtNNRYacgtAC"}


@pytest.fixture(scope="module")
def seq_world(tmp_path_factory):
    from gtars_amd.seqstats import GenomeAssembly

    d = tmp_path_factory.mktemp("reftx_cpu")
    write_fasta(d / "asm.fa", SEQ_CHROMS)
    acc = {name: R.digest_bytes(v) for name, v in R.refget_digests(SEQ_CHROMS).items()}
    txs = [R.make_tx("NM_FWD.1", acc["chrFwd"], 1, [(2, 6), (10, 14)]), R.make_tx("NM_REV.1", acc["chrRev"], -1, [(0, 4), (4, 8)]),
           R.make_tx("NM_SINGLE.1", acc["chrSingle"], 1, [(3, 9)]), R.make_tx("NM_EMPTY.1", bytes(24), 1, []),
           R.make_tx("NM_UNKNOWN.1", bytes(24), 1, [(0, 2)]), R.make_tx("NM_PAST.1", acc["chrSingle"], 1, [(3, 9), (10, 13)]),
           R.make_tx("NM_SOFT_F.1", acc["chrSoft"], 1, [(0, 6), (6, 6), (6, 14)]), R.make_tx("NM_SOFT_R.1", acc["chrSoft"], -1, [(0, 8), (10, 14)])]
    return GenomeAssembly(str(d / "asm.fa")), build_store(txs), txs


def test_mature_mrna_known_answers(seq_world):
    from gtars_amd import reftx as T

    g, store, txs = seq_world
    want = {"NM_FWD.1": "CGATCGAT", "NM_REV.1": "TTAAACGT", "NM_SINGLE.1": "CCCGGG", "NM_EMPTY.1": "",
            "NM_SOFT_F.1": "ACGTNNRYACGTAC",   # forward: upper-cased as it is, IUPAC codes kept
            "NM_SOFT_R.1": "GTACNNNNACGT"}     # reverse: R and Y are outside ACGTN and become N
    assert R.reverse_complement(b"ACGTTTAA") == b"TTAAACGT" and R.reverse_complement(b"acgt") == b"acgt" and R.reverse_complement(b"") == b""
    for acc, seq in want.items():
        assert T.mature_mrna(g, store, acc, on_host=True) == seq
        assert R.mature(SEQ_CHROMS, R.lookup(txs, acc)) == (R.SEQ_OK, seq.encode())
    with pytest.raises(ValueError, match="^Transcript not found: NM_MISSING.1$"):
        T.mature_mrna(g, store, "NM_MISSING.1", on_host=True)
    with pytest.raises(ValueError, match="^Sequence not found: " + "A" * 32 + "$"):
        T.mature_mrna(g, store, "NM_UNKNOWN.1", on_host=True)
    with pytest.raises(ValueError, match="past the end"):
        T.mature_mrna(g, store, "NM_PAST.1", on_host=True)
    assert R.mature(SEQ_CHROMS, R.lookup(txs, "NM_UNKNOWN.1"))[0] == R.SEQ_NO_SEQUENCE and R.mature(SEQ_CHROMS, R.lookup(txs, "NM_PAST.1"))[0] == R.SEQ_PAST_END
    order = [store.transcript(i).accession for i in range(len(store))]
    seqs, status = T.mature_mrnas(g, store, on_host=True, with_status=True)
    assert seqs == [want.get(a) for a in order]
    assert status.tolist() == [R.mature(SEQ_CHROMS, R.lookup(txs, a))[0] for a in order]
    assert T.mature_mrnas(g, store, ["NM_REV.1", "nope", "NM_FWD.1"], on_host=True) == ["TTAAACGT", None, "CGATCGAT"]
    ids = T.transcript_accessions(g, store, on_host=True)
    assert ids == {a: "SQ." + R.sha512t24u(s.encode()) for a, s in want.items()}
    assert g.device == -1  # nothing of this touched a device


# ---- the container ---------------------------------------------------------------------------------------------------
def test_golden_image():
    """the byte image of store.rs:838-930, which the reference's own encoder did not write"""
    from gtars_amd import reftx as T

    image = open(GOLDEN, "rb").read()
    assert len(image) == 133
    want = R.make_tx("NM_1.1", bytes([7]) * 24, 1, [(10, 20)], (100, 200), gene="G", mane=1)
    txs, has_mane = R.decode(image)
    assert txs == [want] and has_mane and R.encode([want]) == image
    store = T.ReadonlyTxStore.open(GOLDEN)
    tx = store.lookup("NM_1.1")
    assert len(store) == 1 and (tx.gene, tx.chrom, tx.strand, tx.cds_start, tx.cds_end) == ("G", R.accession_of(bytes([7]) * 24), T.Strand.Plus, 100, 200)
    assert tx.mane.select and [(e.start, e.end) for e in tx.exons] == [(10, 20)]
    assert store.lookup_mane("g").accession == "NM_1.1"
    b = T.TxStoreBuilder()
    b.add_transcript(_tx_dict(want))
    assert b.to_bytes() == image


def _two():
    d = R.digest_bytes(_chrom_accession())
    return [R.make_tx("NM_004333.6", d, 1, [(50, 500), (600, 700)], (100, 400), gene="BRAF", mane=1),
            R.make_tx("NR_1.2", d, -1, [(10, 20), (30, 30), (40, 45)], gene="other")]


def test_corrupt_stores_are_errors():
    from gtars_amd import reftx as T

    image = R.encode(_two())
    assert len(T.ReadonlyTxStore.from_bytes(image)) == 2
    for bad, text in [(b"X" + image[1:], "Invalid magic number: expected RFTX"), (image[:4] + b"\x03" + image[5:], "Unsupported format version: 3"),
                      (image[:4] + b"\x01" + image[5:], "Unsupported format version: 1")]:
        with pytest.raises(T.TxStoreError, match=text):
            T.ReadonlyTxStore.from_bytes(bad)
        with pytest.raises(ValueError, match=text):
            R.decode(bad)
    for n in range(len(image)):  # a truncated file at every length
        with pytest.raises(T.TxStoreError):
            T.ReadonlyTxStore.from_bytes(image[:n])
        with pytest.raises(ValueError):
            R.decode(image[:n])
    # a record whose exon count, accession or gene length reaches past the records
    first = 40
    for at, value in [(first, 255), (first + 1 + image[first], 255)]:
        bad = bytearray(image)
        bad[at] = value
        with pytest.raises(T.TxStoreError):
            T.ReadonlyTxStore.from_bytes(bytes(bad))
    # accession or gene over the 255 bytes a record allows (store.rs:796-830); exactly 255 is fine
    d = _two()[0]
    for field, text in (("accession", "accession"), ("gene", "gene")):
        for n, ok in ((255, True), (256, False), (300, False)):
            b = T.TxStoreBuilder()
            b.add_transcript(_tx_dict(dict(d, **{field: "A" * n})))
            if ok:
                assert len(T.ReadonlyTxStore.from_bytes(b.to_bytes())) == 1
            else:
                with pytest.raises(T.TxStoreError, match=f"{text} .* is {n} bytes; exceeds 255-byte .reftx limit"):
                    b.to_bytes()
                with pytest.raises(ValueError):
                    R.encode([dict(d, **{field: "A" * n})])
    with pytest.raises(T.TxStoreError):
        T.ReadonlyTxStore.open("/nonexistent/dir/x.reftx")


# ---- cdot and MANE files -------------------------------------------------------------------------------------------------
CDOT = {"transcripts": {
    "NM_1.3": {"id": "NM_1.3", "gene_name": "ONE", "contig": "NC_1.11", "strand": 1, "cds_start": 120, "cds_end": 180, "exons": [[100, 150], [160, 200]]},
    "NM_2.1": {"id": "NM_2.1", "gene_name": "TWO", "contig": "NC_1.11", "strand": -1, "exons": [[300, 400]]},
    "NM_3.9": {"id": "NM_3.9", "gene_name": "THREE", "contig": "NC_UNKNOWN.1", "strand": 1, "exons": [[1, 2]]},      # unknown contig
    "NM_4.1": {"id": "NM_4.1", "gene_name": "FOUR", "contig": "NC_1.11", "strand": 0, "exons": [[1, 2]]},            # strand 0
    "NM_5.1": {"id": "NM_5.1", "gene_name": "FIVE", "contig": "NC_1.11", "strand": 1, "exons": []},                  # no exons
    "NM_6.2": {"id": "NM_6.2", "contig": "NC_2.5", "strand": 1, "cds_start": None, "cds_end": None, "exons": [[5, 9]]},
    "ENST7.4": {"id": "ENST7.4", "gene_name": "SEVEN", "contig": "NC_2.5", "strand": -1, "exons": [[50, 60]]}}}
MANE = ("#NCBI_GeneID\tEnsembl_Gene\tsymbol\tRefSeq_nuc\tEnsembl_nuc\tMANE_status\n"
        "1\tENSG1\tONE\tNM_1.3\tENST1.1\tMANE Select\n"
        "2\tENSG2\tTWO\tNM_2.7\tENST2.1\tMANE Plus Clinical\n"          # another version: found by the base accession
        "\n# a comment\n"
        "6\tENSG6\tSIX\tNM_6.2\t\tsomething else\n"                      # no MANE status we know
        "7\tENSG7\tSEVEN\t\tENST7.4\tMANE Select\n"
        "8\tshort line\n")


@pytest.mark.parametrize("gz", [False, True])
def test_cdot_and_mane_files(tmp_path, gz):
    from gtars_amd import reftx as T

    opener = gzip.open if gz else open
    cdot, mane = tmp_path / ("cdot.json" + (".gz" if gz else "")), tmp_path / ("mane.txt" + (".gz" if gz else ""))
    with opener(cdot, "wt") as f:
        json.dump(CDOT, f)
    with opener(mane, "wt") as f:
        f.write(MANE)
    acc1, acc2 = _chrom_accession(b"ACGT"), _chrom_accession(b"TTTT")
    b = T.TxStoreBuilder()
    b.add_chrom_mapping("NC_1.11", acc1)
    b.add_chrom_mapping("NC_2.5", acc2[3:])  # "SQ." is optional
    assert b.load_mane_summary(str(mane)) == 5
    assert (b.load_cdot_gz if gz else b.load_cdot)(str(cdot)) == 4 and len(b) == 4
    out = tmp_path / "cdot.reftx"
    b.build(str(out))
    store = T.ReadonlyTxStore.open(str(out))
    got = {store.transcript(i).accession: store.transcript(i).to_dict() for i in range(len(store))}
    assert sorted(got) == ["ENST7.4", "NM_1.3", "NM_2.1", "NM_6.2"]
    assert got["NM_1.3"] == {"accession": "NM_1.3", "gene": "ONE", "chrom": acc1, "strand": "+", "cds_start": 120, "cds_end": 180,
                             "exons": [{"start": 100, "end": 150}, {"start": 160, "end": 200}], "mane": {"select": True, "plus_clinical": False}}
    assert got["NM_2.1"]["mane"] == {"select": True, "plus_clinical": True} and got["NM_2.1"]["cds_start"] is None
    assert got["NM_6.2"]["mane"] is None and got["NM_6.2"]["gene"] is None and got["NM_6.2"]["chrom"] == acc2
    assert got["ENST7.4"]["mane"] == {"select": True, "plus_clinical": False}
    assert store.lookup_mane("two").accession == "NM_2.1" and store.lookup_mane("SIX") is None
    with pytest.raises(T.TxStoreError, match="RefSeq_nuc column not found"):
        (tmp_path / "bad.txt").write_text("a\tb\n")
        b.load_mane_summary(str(tmp_path / "bad.txt"))
    with pytest.raises(T.TxStoreError):
        b.load_cdot(str(tmp_path / "missing.json"))
    with pytest.raises(T.TxStoreError, match="Invalid base64url"):
        b.add_chrom_mapping("x", "SQ.***")


# ---- random stores: the restatement against the library's host path ------------------------------------------------------
def random_transcript(rng, name, digest, span):
    """ascending disjoint exons inside [0, span), some empty, some touching; a CDS that mostly lies in exons, at exon edges often"""
    n = rng.choice([1, 1, 2, 3, 5, 8, 13])
    cuts = sorted(rng.randrange(0, span) for _ in range(2 * n))
    exons = []
    for k in range(n):
        s, e = cuts[2 * k], cuts[2 * k + 1]
        if rng.random() < 0.15:
            e = s  # an empty exon
        if exons and rng.random() < 0.2:
            s = exons[-1][1]  # touches the one before
            e = max(e, s)
        exons.append((s, e))
    real = [x for x in exons if x[0] < x[1]]
    cds = (None, None)
    kind = rng.random()
    if real and kind < 0.75:
        a, b = sorted((rng.choice(real), rng.choice(real)))
        s = rng.choice([a[0], a[0], rng.randrange(a[0], a[1])])
        e = rng.choice([b[1], b[1], rng.randrange(b[0], b[1]) + 1])
        cds = (s, e) if s < e else (a[0], b[1])
    elif kind < 0.85:
        cds = (rng.randrange(0, span), rng.randrange(0, span))  # wherever: mostly not in exons
    elif kind < 0.9:
        cds = (rng.randrange(0, span), None)
    return R.make_tx(name, digest, rng.choice([1, -1]), exons, cds, gene="G" + name)


def random_queries(rng, txs, n):
    rows = []
    for _ in range(n):
        tx = rng.choice(txs)
        acc = tx["accession"] if rng.random() < 0.95 else "NM_NOPE.1"
        length = sum(e - s for s, e in tx["exons"])
        kind = rng.choice("ccnng")
        if kind == "g":
            span = (tx["exons"][0][0], tx["exons"][-1][1]) if tx["exons"] else (0, 10)
            rows.append((acc, "g", rng.randrange(max(span[0] - 2, 0), span[1] + 3), 0, False))
            continue
        pos = rng.choice([rng.randrange(-length - 2, length + 3), rng.randrange(-3, 4), rng.randrange(1, length + 2)])
        offset = rng.choice([0, 0, 1, -1, 7, -7, 1 << 40, -(1 << 40)])
        if offset and rng.random() < 0.7 and tx["exons"]:  # aim at an exon boundary in transcript coordinates
            offs = R.exon_offsets(tx)
            ts, te, _, _ = rng.choice(offs)
            bounds = R.cds_tx_bounds(tx, offs)
            anchor = (te - 1 if offset > 0 else ts)
            pos = anchor + 1 if kind == "n" else anchor - bounds[0] + (1 if anchor >= bounds[0] else 0) if bounds else pos
        rows.append((acc, kind, pos, offset, kind == "c" and rng.random() < 0.2))
    return rows


def run_rows(mapper, rows, **kw):
    """rows through the three batch calls -> (values, statuses) in row order"""
    values, statuses = [0] * len(rows), [0] * len(rows)
    for kind in "cng":
        at = [i for i, r in enumerate(rows) if r[1] == kind]
        sub = [rows[i] for i in at]
        acc, pos, off = [r[0] for r in sub], [r[2] for r in sub], [r[3] for r in sub]
        if kind == "c":
            v, s = mapper.c_to_g_many(acc, pos, off, [1 if r[4] else 0 for r in sub], **kw)
        elif kind == "n":
            v, s = mapper.n_to_g_many(acc, pos, off, **kw)
        else:
            v, s = mapper.g_to_transcript_offset_many(acc, pos, **kw)
        assert len(v) == len(s) == len(sub)
        for i, a, b in zip(at, v.tolist(), s.tolist()):
            values[i], statuses[i] = a, b
    return values, statuses


def test_random_stores_host_path_equals_the_restatement():
    from gtars_amd import reftx as T

    rng = random.Random(19)
    seen = set()
    for round_ in range(6):
        txs = [random_transcript(rng, f"NM_{round_}_{k}.1", bytes(24), rng.choice([60, 400, 5000])) for k in range(40)]
        txs.append(R.make_tx(f"NM_{round_}_bad.1", bytes(24), 1, [(10, 20), (15, 30)], (12, 18)))  # overlapping exons
        txs.append(R.make_tx(f"NM_{round_}_none.1", bytes(24), -1, []))
        image = R.encode(txs)
        b = T.TxStoreBuilder()
        for tx in txs:
            b.add_transcript(_tx_dict(tx))
        assert b.to_bytes() == image
        assert R.decode(image)[0] == sorted(txs, key=lambda t: R.fnv1a(t["accession"].encode()))
        store = T.ReadonlyTxStore.from_bytes(image)
        for tx in txs[::7]:
            got = store.lookup(tx["accession"])
            assert dict(got.to_dict(), exons=[(e.start, e.end) for e in got.exons]) == _tx_dict(tx)
            if R.exons_ok(tx):
                assert got.transcript_length == sum(e - s for s, e in tx["exons"])
        rows = random_queries(rng, txs, 1500) + [(f"NM_{round_}_bad.1", "c", 1, 0, False), (f"NM_{round_}_none.1", "n", 1, 0, False)]
        want = R.map_rows(txs, rows)
        assert run_rows(T.CoordinateMapper(store), rows, on_host=True) == want
        seen |= set(want[1])
    assert seen == {R.OK, R.NOT_FOUND, R.NON_CODING, R.OUTSIDE_CDS, R.OUTSIDE_TRANSCRIPT, R.UTR5_OVERFLOW, R.UTR3_OVERFLOW, R.INVALID_OFFSET,
                    R.NOT_EXONIC, R.BAD_EXONS}


def test_decoder_and_mapper_under_the_sanitizers(tmp_path):
    """tests/soak/reftx_host_check.cpp, built with AddressSanitizer + UBSan: the .reftx decoder on every truncation and on
    random byte flips of a small store in exactly sized heap blocks, the scalar mapper on random transcripts against a
    linear-scan copy, the streamed digest against the sequence hashed from memory."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "reftx_host_check"
    src = os.path.join(HERE, "soak", "reftx_host_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o",
                            str(exe), src], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("the host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    store = tmp_path / "two.reftx"
    store.write_bytes(R.encode(_two()))
    run = subprocess.run([str(exe), str(store), "7"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "ok" in run.stdout
