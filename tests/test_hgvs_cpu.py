"""K20 on the host: the plain-Python restatement (tests/hgvs_ref.py) and the library's host path (gtars_amd.hgvs, on_host) are
both checked against the reference's known answers -- the 75 cases of its synthetic corpus (tests/golden/hgvs: cases.tsv over
synthetic.fa and synthetic_transcripts.json), the inline answers of parser.rs and tests/hgvs_parser.rs, the literals of
bridge.rs:930-958 and the golden identifier of bridge.rs:964 -- then against each other on random expressions over random
transcripts.  The import surface, and a stand-alone ASan/UBSan program over csrc/hgvs_core.h."""
import importlib
import json
import os
import random
import shutil
import subprocess

import pytest

import hgvs_ref as HR
import reftx_ref as R
from test_reftx_cpu import build_store, random_transcript
from test_vrs_cpu import write_fasta

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "hgvs")

# what the ported rules give for the six negative rows (the corpus's expected_error column is a label, the reference's own
# test only requires an error): the mapper's codes for c.*999 (past the 3' UTR), c.500 (past the 199-bp CDS) and c.0
# (mapper.rs:359-362: "c.0 is not a valid HGVS coordinate", OutsideCds; parser.rs reads the 0 as an integer), out of bounds
# for g.30100, and -- the mapper does not bound intronic offsets -- a REF mismatch for the two offsets of 50 into a 4-bp intron
NEGATIVE = {"NM_synth_fwd:c.*999A>T": (HR.MAPPING_ERROR, R.UTR3_OVERFLOW), "NM_synth_fwd:c.0A>T": (HR.MAPPING_ERROR, R.OUTSIDE_CDS),
            "NM_synth_simple:c.500A>T": (HR.MAPPING_ERROR, R.OUTSIDE_CDS), "NM_synth_tiny:c.8+50A>T": (HR.REF_MISMATCH, 0),
            "NM_synth_tiny:c.9-50A>T": (HR.REF_MISMATCH, 0), "chr_synth:g.30100A>T": (HR.OUT_OF_BOUNDS, 0)}
NEGATIVE_TEXT = {"NM_synth_fwd:c.*999A>T": "provider error: Mapping error: 3' UTR position c.*999 extends beyond transcript end",
                 "NM_synth_fwd:c.0A>T": "provider error: Mapping error: Position 0 is outside CDS",
                 "NM_synth_simple:c.500A>T": "provider error: Mapping error: Position 500 is outside CDS",
                 "NM_synth_tiny:c.8+50A>T": "REF mismatch at chr_synth:9059: HGVS says A, sequence has ",
                 "NM_synth_tiny:c.9-50A>T": "REF mismatch at chr_synth:8964: HGVS says A, sequence has ",
                 "chr_synth:g.30100A>T": "coordinate 30100 out of bounds for chr_synth (len=30000)"}


def read_fasta(path):
    seqs, name = {}, None
    for line in open(path, "rb").read().splitlines():
        if line.startswith(b">"):
            name = line[1:].split()[0].decode()
            seqs[name] = b""
        elif name is not None:
            seqs[name] += line.strip()
    return seqs


def golden_cases():
    rows = [line.split("\t") for line in open(os.path.join(GOLDEN, "cases.tsv")).read().splitlines() if line and not line.startswith("#")]
    head = rows[0]
    return [dict(zip(head, r + [""] * (len(head) - len(r)))) for r in rows[1:]]


def golden_world():
    """(path of the FASTA, {name: bytes}, restatement transcripts) of the synthetic corpus"""
    fa = os.path.join(GOLDEN, "synthetic.fa")
    seqs = read_fasta(fa)
    digests = R.refget_digests(seqs)
    txs = []
    for t in json.load(open(os.path.join(GOLDEN, "synthetic_transcripts.json")))["transcripts"].values():
        txs.append(R.make_tx(t["id"], R.digest_bytes(digests[t["contig"]]), t["strand"], t["exons"], (t.get("cds_start"), t.get("cds_end")),
                             gene=t.get("gene_name") or ""))
    return fa, seqs, txs


@pytest.fixture(scope="module")
def golden():
    from gtars_amd.seqstats import GenomeAssembly

    fa, seqs, txs = golden_world()
    return GenomeAssembly(fa), build_store(txs), seqs, txs, golden_cases()


def test_fixture_is_the_corpus(golden):
    _, _, seqs, txs, cases = golden
    manifest = json.load(open(os.path.join(GOLDEN, "refget_collection.json")))
    assert R.refget_digests(seqs) == {"chr_synth": manifest["sequences"]["chr_synth"]["sha512t24u"]} == {"chr_synth": "xR1CjxR1t5kbrBkPm59BbDSSId73exim"}
    assert len(seqs["chr_synth"]) == 30000 and len(txs) == 5
    assert len(cases) == 75 and sum(1 for c in cases if c["expected_vrs_id"]) == 69
    assert {c["hgvs_string"] for c in cases if not c["expected_vrs_id"]} == set(NEGATIVE)


def test_restatement_gives_the_corpus(golden):
    _, _, seqs, txs, cases = golden
    acc = R.refget_digests(seqs)
    for c in cases:
        got = HR.bridge_one(seqs, acc, txs, c["hgvs_string"])
        if c["expected_vrs_id"]:
            assert (got["status"], got["id"]) == (HR.OK, c["expected_vrs_id"]), c["case_id"]
        else:
            assert (got["status"], got["detail"]) == NEGATIVE[c["hgvs_string"]] and got["id"] is None, c["case_id"]


def test_host_path_gives_the_corpus(golden):
    from gtars_amd import hgvs as H

    genome, store, _, _, cases = golden
    strings = [c["hgvs_string"] for c in cases]
    r = H.hgvs_to_vrs_ids(genome, store, strings, on_host=True)
    for k, c in enumerate(cases):
        if c["expected_vrs_id"]:
            assert (r["statuses"][k], r["ids"][k]) == (H.OK, c["expected_vrs_id"]), c["case_id"]
            assert r["chroms"][k] == 0 and H.hgvs_to_vrs_id(c["hgvs_string"], genome, store, on_host=True) == c["expected_vrs_id"]
        else:
            assert (r["statuses"][k], r["details"][k]) == NEGATIVE[c["hgvs_string"]] and r["ids"][k] is None, c["case_id"]
            assert r["chroms"][k] == H.NONE_U32 and r["starts"][k] == 0 and r["ends"][k] == 0
            with pytest.raises(ValueError) as e:
                H.hgvs_to_vrs_id(c["hgvs_string"], genome, store, on_host=True)
            assert str(e.value).startswith(NEGATIVE_TEXT[c["hgvs_string"]]) and not isinstance(e.value, H.HgvsError), str(e.value)
    assert not r["warnings"].any()


# ---- the parser's known answers ---------------------------------------------------------------------------------------------
def _single(base, offset=0, datum="cds"):
    return {"kind": "certain", "position": {"base": base, "offset": offset, "datum": datum}, "low": None, "high": None}


def _variant(acc, rt, kind, start, end, edit, gene=None, uncertain=False):
    return {"accession": acc, "gene": gene, "reference_type": rt,
            "pos_edit": {"location_kind": kind, "start": start, "end": end, "edit": dict(zip(("kind", "ref", "alt"), edit)), "uncertain": uncertain}}


NM = "NM_004333.6"
KNOWN = [  # parser.rs:585-792, tests/hgvs_parser.rs:33-77
    ("NC_000007.14:g.140753336A>T", _variant("NC_000007.14", "g", "single", _single(140753336, 0, "seq_start"), None, ("substitution", "A", "T"))),
    (NM + ":c.1799T>A", _variant(NM, "c", "single", _single(1799), None, ("substitution", "T", "A"))),
    (NM + ":c.-14C>T", _variant(NM, "c", "single", _single(-14), None, ("substitution", "C", "T"))),
    (NM + ":c.*37A>G", _variant(NM, "c", "single", _single(37, 0, "cds_stop"), None, ("substitution", "A", "G"))),
    (NM + ":c.1798+5G>A", _variant(NM, "c", "single", _single(1798, 5), None, ("substitution", "G", "A"))),
    (NM + ":c.1799-3T>A", _variant(NM, "c", "single", _single(1799, -3), None, ("substitution", "T", "A"))),
    (NM + ":c.100delAGT", _variant(NM, "c", "single", _single(100), None, ("deletion", "AGT", None))),
    (NM + ":c.100del", _variant(NM, "c", "single", _single(100), None, ("deletion", None, None))),
    (NM + ":c.100_102dupATG", _variant(NM, "c", "range", _single(100), _single(102), ("duplication", "ATG", None))),
    (NM + ":c.100_101insATG", _variant(NM, "c", "range", _single(100), _single(101), ("insertion", None, "ATG"))),
    (NM + ":c.100_102delinsCT", _variant(NM, "c", "range", _single(100), _single(102), ("delins", None, "CT"))),
    (NM + ":c.100_102delAGTinsCT", _variant(NM, "c", "range", _single(100), _single(102), ("delins", "AGT", "CT"))),
    (NM + ":c.100=", _variant(NM, "c", "single", _single(100), None, ("identity", None, None))),
    (NM + "(BRAF):c.1799T>A", _variant(NM, "c", "single", _single(1799), None, ("substitution", "T", "A"), gene="BRAF")),
    ("BRAF:c.1799T>A", _variant("BRAF", "c", "single", _single(1799), None, ("substitution", "T", "A"))),
    (NM + ":c.(1799T>A)", _variant(NM, "c", "single", _single(1799), None, ("substitution", "T", "A"), uncertain=True)),
    ("NC_000007.14:g.100_200inv", _variant("NC_000007.14", "g", "range", _single(100, 0, "seq_start"), _single(200, 0, "seq_start"),
                                           ("inversion", None, None))),
    (NM + ":c.1798_1800delAGT", _variant(NM, "c", "range", _single(1798), _single(1800), ("deletion", "AGT", None))),
]
FORMS = ["NM_1.1:c.(4_6)_246del", "NM_1.1:c.4_(245_246)del", "NM_1.1:c.(?_6)_(245_?)dup", "NM_1.1:c.(?_?)_5del", "NM_1.1:c.(4_6)del", "NC_1.1:g.=",
         "NC_1.1:g.?", "NC_1.1:g.5_9copy3", "NC_1.1:g.5CA[4]", "NM_1.1:c.5del3", "NM_1.1:c.5G=", "NM_1.1:c.+5A>T", "NM_1.1:r.76a>c",
         "NC_1.1:m.3243A>G", "NM_1.1:c.5delA3", "NM_1.1:c.5delins", "NM_1.1:c.5>T", "NM_1.1:c.5A>", "NM_1.1:c.5CA[4", "NM_1.1:c.(5A>T",
         "NM_1.1:c.99999999999999999999A>T", "NM_1.1:c.18446744073709551615A>T", "NM_1.1:c.-9223372036854775808A>T", "NM_1.1:n.*5A>T",
         ":c.5A>T", "NM_1.1():c.5A>T", "NM_1.1(G:c.5A>T", "NM_1.1", "NM_1.1:", "NM_1.1:x.5A>T", "NM_1.1:c5A>T", "NM_1.1:c.5A>T ", "NM_1.1:c.5_A>T",
         "NM_1.1:c.5-A>T", "NM_1.1:c.(5_?)A>T", "café:c.5A>T", "NM_1.1:c.5A>Té", "NP_1.1:p.Val600Glu", "NP_1.1(BRAF):p.V600E"]


def test_parser_known_answers_and_forms():
    from gtars_amd import hgvs as H

    for text, want in KNOWN:
        assert HR.parse(text) == want, text
        v = H.parse_hgvs(text)
        assert v.to_dict() == want, text
        assert v.accession == want["accession"] and v.pos_edit.edit.kind == want["pos_edit"]["edit"]["kind"]
    v = H.parse_hgvs(NM + ":c.1798+5G>A")
    p = v.pos_edit.start.position
    assert (v.reference_type, p.base, p.offset, p.datum) == (H.ReferenceType.Coding, 1798, 5, H.Datum.Cds)
    assert repr(v.reference_type) == "ReferenceType.Coding" and v.pos_edit.end is None and v.pos_edit.location_kind == "single"
    for text in ("NM_004333.6", "NM_004333.6:x.100A>T"):  # parser.rs:783-792
        with pytest.raises(H.HgvsError, match="HGVS parse error at position"):
            H.parse_hgvs(text)
    # every other form: the library's parser and the restatement agree on the tree, or on the error's position and message
    for text in FORMS + [k[0] for k in KNOWN]:
        for cut in sorted({len(text), *range(0, len(text), 3)}):
            s = text[:cut]
            try:
                want = HR.parse(s)
            except HR.ParseError as e:
                with pytest.raises(H.HgvsError) as got:
                    H.parse_hgvs(s)
                assert str(got.value).startswith(f"HGVS parse error at position {e.pos}: {e.msg} (in: "), s
                continue
            except HR.Protein:
                with pytest.raises(H.HgvsError, match="protein expressions are not parsed"):
                    H.parse_hgvs(s)
                continue
            assert H.parse_hgvs(s).to_dict() == want, s
    assert str(pytest.raises(H.HgvsError, H.parse_hgvs, 'a"b').value) == 'HGVS parse error at position 3: expected `:` after accession (in: "a\\"b")'


def test_looks_like_gene_symbol():
    from gtars_amd import hgvs as H

    yes = ["BRAF", "TP53", "KIT", "MTOR", "MTHFR", "GLI1", "KIF5B", "MT-CO1", "MT-ND1"]  # bridge.rs:930-958
    no = ["NM_004333.6", "NC_000007.14", "ENST00000288602", "ENSG00000157764", "chr7", "chrM", "chrMT", "MT", "GL000220.1", "KI270728.1",
          "GL000220", "KI270728"]
    for f in (H.looks_like_gene_symbol, HR.looks_like_gene_symbol):
        assert all(f(s) for s in yes) and not any(f(s) for s in no)


def test_chrf_golden_identifier(tmp_path):
    from gtars_amd import hgvs as H
    from gtars_amd.seqstats import GenomeAssembly

    seqs = {"chrF": b"ACGT" * 10}
    write_fasta(tmp_path / "f.fa", seqs)
    g = GenomeAssembly(str(tmp_path / "f.fa"))
    want = "ga4gh:VA._q-idtHGQxQ4XiEPJ1ExYl_htUeNEkir"  # bridge.rs:964
    assert H.hgvs_to_vrs_id("chrF:g.6C>T", g, None, on_host=True) == want == H.hgvs_to_vrs_id("NC_six.1:g.6C>T", g, aliases={"NC_six.1": "chrF"}, on_host=True)
    assert HR.bridge_one(seqs, R.refget_digests(seqs), [], "chrF:g.6C>T")["id"] == want
    with pytest.raises(H.HgvsError):
        H.hgvs_to_vrs_id("chrF:g.6C>", g, on_host=True)
    for text, message in (("chrF:g.6A>T", "REF mismatch at chrF:5: HGVS says A, sequence has C"), ("chrG:g.6C>T", "chromosome accession chrG not found in collection"),
                          ("chrF:g.0C>T", "inconsistent edit: g. position must be >= 1, got 0"), ("chrF:g.6_9insA", "inconsistent edit: ins range positions are not adjacent: 5 and 8"),
                          ("chrF:g.6_9inv", "unsupported edit: inv"), ("chrF:g.=", "unsupported edit: whole-sequence edit"),
                          ("chrF:g.(1_2)_9del", "unsupported edit: uncertain position range"), ("chrF:m.6C>T", "unsupported reference type: M (v1 supports g., c., n.)"),
                          ("BRAF:c.6C>T", "provider error: No MANE Select transcript for gene: BRAF"), ("NM_1.1:c.6C>T", "provider error: Transcript not found: NM_1.1"),
                          ("chrF:g.41C>T", "coordinate 41 out of bounds for chrF (len=40)")):
        with pytest.raises(ValueError) as e:
            H.hgvs_to_vrs_id(text, g, on_host=True)
        assert str(e.value) == message
    r = H.hgvs_to_vrs_ids(g, None, ["chrF:g.(6C>T)", "chrF:g.6C>T"], on_host=True)
    assert r["ids"] == [want, want] and r["warnings"].tolist() == [H.WARN_UNCERTAIN, 0]
    assert H.hgvs_to_vrs_ids(g, None, [], on_host=True)["ids"] == []


# ---- random expressions: the restatement against the library's host path -----------------------------------------------------
SPECIAL = ["chrA:g.=", "chrA:g.?", "chrA:g.5_9inv", "chrA:g.5_9copy3", "chrA:g.5CA[4]", "chrA:g.(5_9)_20del", "chrA:g.5_(9_?)del", "chrA:m.5A>T",
           "{acc}:r.5a>c", "NP_1.1:p.Val600Glu", "{acc}:c.5", "{acc}", "chrA:g.(5del)", "{acc}:c.(5_6insACGT)", "chrNOPE:g.5del", "NC_five.1:g.5del",
           "chrA:g.0del", "chrA:g.3_9insAC", "{gene}:c.5del", "NOGENE:c.5del", "NM_NOPE.1:n.5del", "{acc}:n.(4_6)del"]


def random_world(rng, tag):
    """an assembly {name: bytes} of four chromosomes (mixed case, some N) and transcripts on three of them and on none"""
    seqs = {name: bytes(rng.choice(b"ACGTACGTACGTacgtN") for _ in range(n)) for name, n in (("chrA", 900), ("chrB", 400), ("ctg.C", 250), ("chrD", 120))}
    # planted repeats, so that dups and deletions roll
    a = bytearray(seqs["chrA"])
    a[100:160] = b"CAG" * 20
    a[300:340] = b"A" * 40
    seqs["chrA"] = bytes(a)
    own = R.refget_digests(seqs)
    txs = []
    for k in range(30):
        name = rng.choice(["chrA", "chrA", "chrB", "ctg.C", None])
        digest = R.digest_bytes(own[name]) if name else bytes(24)
        span = len(seqs[name]) + (30 if rng.random() < 0.2 else 0) if name else 300  # (some exons reach past the chromosome)
        tx = random_transcript(rng, f"NM_{tag}_{k}.1", digest, span)
        tx["gene"], tx["mane"] = f"GENE{tag}X{k}", rng.choice([0, 1, 1, 3])
        txs.append(tx)
    return seqs, txs


def _position_text(rng, tx, kind):
    length = sum(e - s for s, e in tx["exons"])
    pos = rng.choice([rng.randrange(-length - 2, length + 3), rng.randrange(-3, 4), rng.randrange(1, length + 2)])
    offset = rng.choice([0, 0, 0, 1, -1, 7, -7])
    star = kind == "c" and rng.random() < 0.15
    if offset and rng.random() < 0.8 and tx["exons"] and R.exons_ok(tx):  # aim at an exon boundary
        offs = R.exon_offsets(tx)
        ts, te, _, _ = rng.choice(offs)
        bounds = R.cds_tx_bounds(tx, offs)
        anchor = te - 1 if offset > 0 else ts
        if kind == "n":
            pos, star = anchor + 1, False
        elif bounds:
            pos, star = anchor - bounds[0] + (1 if anchor >= bounds[0] else 0), False
    if kind == "n" or star:
        pos = abs(pos)
    return ("*" if star else "") + str(pos) + ("%+d" % offset if offset else ""), pos


def random_strings(rng, seqs, txs, n, aliases):
    """expressions of every kind over the world, with REF alleles that mostly agree with the assembly"""
    own = R.refget_digests(seqs)
    out = []
    while len(out) < n:
        tx = rng.choice(txs)
        if rng.random() < 0.08:
            out.append(rng.choice(SPECIAL).format(acc=tx["accession"], gene=tx["gene"]))
            continue
        kind = rng.choice("ccnng")
        if kind == "g":
            acc = rng.choice(["chrA", "chrA", "chrB", "ctg.C", "chrD", "NC_five.1", "chrNOPE"])
            length = len(seqs.get(aliases.get(acc, acc), b"x" * 50))
            p = rng.choice([rng.randrange(1, length + 1), rng.randrange(95, 165), length, length + 1, 1])
            first, second = str(p), str(p + rng.choice([1, 1, 2, 5, 40]))
        else:
            acc = tx["accession"] if rng.random() < 0.9 else tx["gene"]
            first, p = _position_text(rng, tx, kind)
            second = _position_text(rng, tx, kind)[0] if rng.random() < 0.2 else ("*" if first.startswith("*") else "") + str(p + rng.choice([1, 1, 2, 3]))
        loc = first if rng.random() < 0.55 else first + "_" + second
        edit = rng.choice(["sub", "del", "dup", "ins", "delins", "="])
        alt = "".join(rng.choice("ACGT") for _ in range(rng.choice([1, 1, 2, 3, 9, 17])))
        if rng.random() < 0.05:
            alt = rng.choice([alt.lower(), alt + "R", "N" + alt])
        head = f"{acc}:{kind}.{loc}"
        # the span's own bytes as the REF allele, from the restatement's mapping of the expression without one
        probe = HR.bridge_one(seqs, own, txs, head + "del", aliases)
        ref = ""
        if probe["span"] and probe["span"][2] <= len(seqs[probe["span"][0]]):
            chrom, s, e, strand = probe["span"]
            ref = seqs[chrom][s:e].upper()
            ref = (ref if strand > 0 else HR.revcomp(ref) or b"").decode()
        r = rng.random()
        if r < 0.06:
            ref = "".join({"A": "C", "C": "G", "G": "T", "T": "A"}.get(c, "A") for c in ref[:1]) + ref[1:] or "A"
        elif r < 0.1:
            ref = ref.lower()
        elif r < 0.13:
            ref += "A"
        with_ref = rng.random() < 0.5 and len(ref) < 40
        text = {"sub": f"{ref or 'A'}>{alt}", "del": "del" + (ref if with_ref else ""), "dup": "dup" + (ref if with_ref else ""), "ins": "ins" + alt,
                "delins": ("del" + ref + "ins" if with_ref else "delins") + alt, "=": "="}[edit]
        out.append(f"({head}{text})".replace("(" + acc + ":" + kind + ".", acc + ":" + kind + ".(") if rng.random() < 0.03 else head + text)
    return out


def check_batch(got, want, seqs, context=""):
    """a result of hgvs_to_vrs_ids against the restatement's rows, field by field"""
    names = list(seqs)
    assert len(got["ids"]) == len(want)
    for k, w in enumerate(want):
        row = (int(got["statuses"][k]), int(got["details"][k]), int(got["warnings"][k]), got["ids"][k], int(got["starts"][k]), int(got["ends"][k]))
        assert row == (w["status"], w["detail"], w["warning"], w["id"], w["start"], w["end"]), (context, k)
        if w["status"] == HR.OK:
            assert names[got["chroms"][k]] == w["chrom"], (context, k)
        elif w["status"] != HR.NORMALIZE_ERROR:
            assert got["chroms"][k] == 0xFFFFFFFF, (context, k)


def make_world(tmp_path, seed):
    """a random world as the library's objects and the restatement's: (genome, store, seqs, txs, accessions, aliases)"""
    from gtars_amd.seqstats import GenomeAssembly

    rng = random.Random(seed)
    seqs, txs = random_world(rng, seed)
    write_fasta(tmp_path / f"w{seed}.fa", seqs)
    accessions = {k: v for k, v in R.refget_digests(seqs).items() if k != "chrD"}  # chrD has no accession: K18's status 4
    return GenomeAssembly(str(tmp_path / f"w{seed}.fa")), build_store(txs), seqs, txs, accessions, {"NC_five.1": "chrB"}, rng


def test_random_expressions_host_path_equals_the_restatement(tmp_path):
    from gtars_amd import hgvs as H

    assert H.STATUS_NAMES == HR.STATUS_NAMES
    seen, kinds = set(), set()
    for seed in (20, 21, 22):
        genome, store, seqs, txs, accessions, aliases, rng = make_world(tmp_path, seed)
        strings = random_strings(rng, seqs, txs, 1500, aliases)
        want = HR.bridge(seqs, accessions, txs, strings, aliases)
        got = H.hgvs_to_vrs_ids(genome, store, strings, accessions=accessions, aliases=aliases, on_host=True, threads=3)
        check_batch(got, want, seqs, seed)
        seen |= {w["status"] for w in want}
        for s, w in zip(strings, want):
            if w["status"] == HR.OK:
                v = HR.parse(s)
                kinds.add((v["reference_type"], v["pos_edit"]["edit"]["kind"], w["span"][3], v["pos_edit"]["location_kind"]))
        # an ins across an exon junction: adjacent on the transcript, not on the genome
        own = R.refget_digests(seqs)
        for tx in txs:
            offs = [o for o in R.exon_offsets(tx) if o[0] < o[1]] if R.exons_ok(tx) else []
            bound = any(R.digest_bytes(d) == tx["digest"] for d in own.values())
            if bound and len(offs) > 1 and (offs[1][2] - offs[0][3] if tx["strand"] > 0 else offs[0][2] - offs[1][3]) > 0:
                text = f"{tx['accession']}:n.{offs[0][1]}_{offs[0][1] + 1}insA"
                one = H.hgvs_to_vrs_ids(genome, store, [text], on_host=True)
                assert one["statuses"][0] == HR.bridge_one(seqs, own, txs, text)["status"] == HR.INCONSISTENT_EDIT, text
                with pytest.raises(ValueError, match="ins range positions are not adjacent"):
                    H.hgvs_to_vrs_id(text, genome, store, on_host=True)
                break
        else:
            raise AssertionError("no exon junction in this world")
    assert seen == set(range(12))  # every status code
    for rt in "gcn":
        for edit in ("substitution", "deletion", "duplication", "insertion", "delins", "identity"):
            for strand in ((1,) if rt == "g" else (1, -1)):
                assert any(k[:3] == (rt, edit, strand) for k in kinds), (rt, edit, strand)


def test_import_surface():
    import gtars
    import gtars_amd
    import gtars_amd.hgvs as H
    from gtars.vrs.hgvs import HgvsError, hgvs_to_vrs_id, parse_hgvs  # noqa: F401

    for path in ("gtars_amd.hgvs", "gtars_amd.vrs.hgvs", "gtars.hgvs", "gtars.vrs.hgvs"):
        assert importlib.import_module(path) is H, path
    assert gtars.vrs.hgvs is H and gtars_amd.vrs.hgvs is H and parse_hgvs is H.parse_hgvs
    assert issubclass(HgvsError, Exception) and not issubclass(HgvsError, ValueError)
    for name in ("ReferenceType", "Datum", "Position", "Edit", "PositionBound", "PosEdit", "HgvsVariant", "parse_hgvs", "hgvs_to_vrs_id",
                 "hgvs_to_vrs_ids", "HgvsError"):
        assert hasattr(H, name), name
    with pytest.raises(ModuleNotFoundError):
        importlib.import_module("gtars.refget")


@pytest.mark.skipif(__import__("gtars_amd").device_count() > 0, reason="needs a box WITHOUT a GPU")
def test_no_device_is_a_loud_error(golden):
    import gtars_amd
    from gtars_amd import hgvs as H

    genome, store, _, _, _ = golden
    with pytest.raises(gtars_amd.NoDeviceError):
        H.hgvs_to_vrs_ids(genome, store, ["chr_synth:g.4000A>T"])
    with pytest.raises(gtars_amd.NoDeviceError):
        H.hgvs_to_vrs_id("chr_synth:g.4000A>T", genome, store)


def test_parser_and_bridge_under_the_sanitizers(tmp_path):
    """tests/soak/hgvs_host_check.cpp, built with AddressSanitizer + UBSan: hgvs_parse on every prefix and on random byte flips
    of valid expressions in exactly sized heap blocks, the span and alt functions on random transcripts."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "hgvs_host_check"
    src = os.path.join(HERE, "soak", "hgvs_host_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o",
                            str(exe), src], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("the host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe), "20"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "ok" in run.stdout
