"""Genomic partitions without a GPU: the restatement tests/partitions_ref.py against the reference's own literals
(gtars-genomicdist/src/partitions.rs tests, the R-derived C. elegans UTR sets), and the host parts of K14 -- the UTR
reader gtars_gtf_read_utrs and gtars_partition_expected -- against the restatement."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import annot_ref as A  # noqa: E402
import partitions_ref as P  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regionset")
CE = os.path.join(GOLD, "C_elegans_cropped_example.gtf.gz")


def _gold(name):
    return os.path.join(GOLD, name)


def _native_utrs(path, pc, conv):
    """gtars_gtf_read_utrs -> (three, five) as stranded rows"""
    from gtars_amd import models as M

    rows, strand, kind = M._read_gtf_utrs(path, pc, conv)
    names, ids, s, e = rows.chrom_names, rows.chrom_ids, rows.starts, rows.ends
    out = ([], [])
    for i in range(len(rows)):
        out[kind[i]].append((names[ids[i]], int(s[i]), int(e[i]), int(strand[i])))
    return out


def _both(path, pc, conv):
    """the two UTR sets from the native reader, checked against the restatement as multisets (only their reduce is used)"""
    three, five = _native_utrs(path, pc, conv)
    want3, want5 = P.gtf_utr_rows(P.read_bytes(path), pc, conv)
    assert sorted(three) == sorted(want3) and sorted(five) == sorted(want5)
    return three, five


def _bed3(name):
    rows = [(c, s, e) for c, s, e, _ in P.bed_stranded(_gold(name))]
    return sorted(rows, key=lambda r: (r[0], r[1]))


def _bed_model(utrs=True):
    return P.model_of(P.bed_stranded(_gold("test_genes.bed")), P.bed_stranded(_gold("test_exons.bed")),
                      P.bed_stranded(_gold("test_three_utr.bed")) if utrs else None,
                      P.bed_stranded(_gold("test_five_utr.bed")) if utrs else None)


def test_names_import():
    import gtars
    import gtars_amd
    from gtars.models import GeneModel
    from gtars.partitions import PartitionList, calc_expected_partitions, calc_partitions, partition_assignments  # noqa: F401

    assert gtars.partitions is gtars_amd.partitions and "partitions" in gtars.__all__
    assert hasattr(GeneModel, "from_bed_files") and hasattr(PartitionList, "from_annotation")
    with pytest.raises(TypeError):
        PartitionList()


def test_ref_from_bed_files_counts():
    m = _bed_model()
    assert (len(m["genes"]), len(m["exons"]), len(m["three_utr"]), len(m["five_utr"])) == (6, 19, 6, 6)
    m = _bed_model(utrs=False)
    assert len(m["genes"]) == 6 and m["three_utr"] is None and m["five_utr"] is None


def test_gtf_fixture_counts_and_coordinates():
    path = _gold("test_gene_model.gtf")
    rows = A.read_gtf(path, False, False)
    three, five = _both(path, False, False)
    m = P.model_of([r[:4] for r in rows if r[4] == A.GENE], [r[:4] for r in rows if r[4] == A.EXON], three, five)
    assert (len(m["genes"]), len(m["exons"]), len(m["three_utr"]), len(m["five_utr"])) == (3, 7, 2, 2)
    assert [g[1:3] for g in m["genes"] if g[0] == "chr1"] == [(1000, 5000)]
    assert [g[1:3] for g in m["genes"] if g[0] == "chr2"] == [(3000, 8000)]
    rows = A.read_gtf(path, True, False)
    genes, exons = A.gene_model(rows)
    assert len(genes) == 2 and len(exons) == 5 and all(g[0] != "chr3" for g in genes)
    three, five = _both(path, True, False)
    assert all(r[0] != "chr3" for r in three + five)


@pytest.mark.parametrize("pc,tag", [(False, "all"), (True, "pc")])
def test_utr_sets_against_r(pc, tag):
    three, five = _both(CE, pc, False)
    assert A.reduce_unstranded(three) == _bed3(f"ce_ref_three_utr_{tag}.bed")
    assert A.reduce_unstranded(five) == _bed3(f"ce_ref_five_utr_{tag}.bed")


def test_ensembl_fixture_has_both_utr_sets():
    for conv in (False, True):
        three, five = _both(_gold("test_gene_model_ensembl.gtf"), False, conv)
        assert three and five
        assert all(r[0].startswith("chr") == conv for r in three + five)


def _gtf(tmp_path, rows):
    p = tmp_path / "m.gtf"
    p.write_text("".join("\t".join(str(x) for x in r) + "\n" for r in rows))
    return str(p)


def _attr(tx=None, extra=""):
    return 'gene_id "g"; ' + (f'transcript_id "{tx}"; ' if tx else "") + extra


def test_branch_typed_rows(tmp_path):
    # typed rows are taken as they are, UTR rows next to them are classified, exon-minus-CDS never runs
    path = _gtf(tmp_path, [
        ("chr1", "t", "three_prime_utr", 101, 200, ".", "+", ".", _attr("t1")),
        ("chr1", "t", "five_prime_utr", 301, 400, ".", "-", ".", _attr()),
        ("chr1", "t", "five_prime_utr", 501, 600, ".", "", ".", _attr()),      # empty strand field: '.', unstranded
        ("chr1", "t", "exon", 1, 1000, ".", "+", ".", _attr("t1")),
        ("chr1", "t", "CDS", 401, 500, ".", "+", ".", _attr("t1")),
        ("chr1", "t", "UTR", 901, 950, ".", "+", ".", _attr("t1")),
    ])
    three, five = _both(path, False, False)
    assert sorted(three) == [("chr1", 100, 200, A.PLUS), ("chr1", 900, 950, A.PLUS)]
    assert sorted(five) == [("chr1", 300, 400, A.MINUS), ("chr1", 500, 600, A.UNSTRANDED)]


def test_branch_utr_rows_classified_by_cds(tmp_path):
    path = _gtf(tmp_path, [
        ("chr1", "t", "UTR", 101, 200, ".", "+", ".", _attr("p")),        # before the CDS on +: five
        ("chr1", "t", "CDS", 301, 400, ".", "+", ".", _attr("p")),
        ("chr1", "t", "CDS", 501, 600, ".", "+", ".", _attr("p")),
        ("chr1", "t", "UTR", 701, 800, ".", "+", ".", _attr("p")),        # behind it: three
        ("chr1", "t", "UTR", 401, 500, ".", "+", ".", _attr("p")),        # midpoint 450 == CDS midpoint 450: not <, three
        ("chr2", "t", "UTR", 101, 200, ".", "-", ".", _attr("m")),        # before the CDS on -: three
        ("chr2", "t", "UTR", 701, 800, ".", "-", ".", _attr("m")),        # behind it: five
        ("chr2", "t", "CDS", 301, 600, ".", "-", ".", _attr("m")),
        ("chr2", "t", "UTR", 701, 900, ".", ".", ".", _attr("m")),        # any other strand character: the > rule
        ("chr2", "t", "UTR", 1, 50, ".", "", ".", _attr("m")),            # empty: '+', the < rule, strand Plus
        ("chr3", "t", "UTR", 101, 200, ".", "+", ".", _attr("nocds")),    # transcript without CDS: dropped
        ("chr3", "t", "UTR", 101, 200, ".", "+", ".", _attr()),           # no transcript: dropped
        ("chr3", "t", "UTR", 301, 400, ".", "+", ".", 'x "1"; transcript_id "p"; transcript_id "nocds";'),  # first marker
        ("chr3", "t", "exon", 1, 5000, ".", "+", ".", _attr("p")),        # exons are not used once a UTR row exists
    ])
    three, five = _both(path, False, False)
    assert sorted(five) == [("chr1", 100, 200, A.PLUS), ("chr2", 0, 50, A.PLUS), ("chr2", 700, 800, A.MINUS),
                            ("chr2", 700, 900, A.UNSTRANDED), ("chr3", 300, 400, A.PLUS)]
    assert sorted(three) == [("chr1", 400, 500, A.PLUS), ("chr1", 700, 800, A.PLUS), ("chr2", 100, 200, A.MINUS)]


def test_branch_exon_minus_cds(tmp_path):
    path = _gtf(tmp_path, [
        ("chr1", "t", "exon", 101, 1000, ".", "+", ".", _attr("p")),      # spans the whole CDS: both pieces
        ("chr1", "t", "CDS", 301, 600, ".", "+", ".", _attr("p")),
        ("chr1", "t", "exon", 1, 50, ".", "+", ".", _attr("p")),          # wholly before: five, end = min(end, cds start)
        ("chr1", "t", "exon", 401, 500, ".", "+", ".", _attr("p")),       # inside the CDS: nothing
        ("chr2", "t", "exon", 101, 1000, ".", "-", ".", _attr("m")),
        ("chr2", "t", "CDS", 301, 400, ".", "-", ".", _attr("m")),
        ("chr2", "t", "CDS", 501, 600, ".", "-", ".", _attr("m")),
        ("chr3", "t", "exon", 101, 200, ".", "+", ".", _attr("nocds")),   # non-coding transcript: nothing
        ("chr3", "t", "exon", 101, 200, ".", "+", ".", _attr()),
    ])
    three, five = _both(path, False, False)
    assert sorted(five) == [("chr1", 0, 50, A.PLUS), ("chr1", 100, 300, A.PLUS), ("chr2", 600, 1000, A.MINUS)]
    assert sorted(three) == [("chr1", 600, 1000, A.PLUS), ("chr2", 100, 300, A.MINUS)]


def test_native_utr_reader_errors(tmp_path):
    from gtars_amd import models as M

    with pytest.raises(ValueError):
        M._read_gtf_utrs(str(tmp_path / "missing.gtf"), True, True)
    path = _gtf(tmp_path, [("chr1", "t", "UTR", "x", 200, ".", "+", ".", _attr("p"))])
    with pytest.raises(ValueError, match="Parsing GTF start: invalid digit found in string"):
        M._read_gtf_utrs(path, False, False)


# ---- the restatement against the reference's partition tests ---------------------------------------------------------
def test_ref_partition_list_literals():
    parts = P.partition_list(_bed_model(), 100, 2000)
    assert [n for n, _ in parts] == ["promoterCore", "promoterProx", "threeUTR", "fiveUTR", "exon", "intron"]
    assert [n for n, _ in P.partition_list(_bed_model(False), 100, 2000)] == ["promoterCore", "promoterProx", "exon", "intron"]
    for i in range(len(parts)):
        for j in range(i + 1, len(parts)):
            assert not [r for r in parts[j][1] if P.hits(r[0], r[1], r[2], parts[i][1])], (parts[i][0], parts[j][0])
    m = P.model_of([("chr1", 5000, 10000, A.UNSTRANDED)], [("chr1", 5000, 5500, A.UNSTRANDED), ("chr1", 9000, 10000, A.UNSTRANDED)])
    parts = P.partition_list(m, 100, 2000)
    assert parts[0][1] == [("chr1", 4900, 5000)] and parts[1][1] == [("chr1", 3000, 4900)]
    m = P.model_of([("chr1", 1000, 5000, A.PLUS), ("chr1", 6000, 9000, A.MINUS)], [("chr1", 1000, 1500, A.PLUS), ("chr1", 6000, 6500, A.MINUS)])
    assert sorted(r[1] for r in P.partition_list(m, 100, 2000)[0][1]) == [900, 9000]


def test_ref_calc_partitions_literals():
    m = P.model_of([("chr1", 100, 1000, A.UNSTRANDED)], [("chr1", 50, 150, A.UNSTRANDED)])
    counts, total = P.calc_partitions([("chr1", 0, 120)], P.partition_list(m, 100, 200))
    assert counts[0] == 1 and total == 1
    parts = P.partition_list(_bed_model(), 100, 2000)
    assert P.calc_partitions([("chr1", 50000, 50200)], parts)[0][-1] == 1
    query = _bed3("test_query_promoter_enriched.bed")
    counts, total = P.calc_partitions(query, parts)
    assert sum(counts) == total == len(query)
    counts, total = P.calc_partitions(query, parts, True)
    assert sum(counts) == total == sum(e - s for _, s, e in query)
    m = P.model_of([("chr1", 1000, 5000, A.UNSTRANDED)], [("chr1", 1000, 2000, A.UNSTRANDED)])
    parts = P.partition_list(m, 100, 200)
    counts, total = P.calc_partitions([("chr1", 750, 950)], parts, True)
    prom = counts[0] + counts[1]
    assert total == 200 and prom > 0 and counts[-1] > 0 and prom + counts[-1] == 200
    sizes = {"chr1": 100000, "chr2": 80000, "chr3": 60000}
    parts = P.partition_list(_bed_model(), 100, 2000)
    counts, exp, oe, pv = P.calc_expected_partitions(query, parts, sizes)
    assert all(0.0 <= p <= 1.0 for p in pv) and (oe[0] > 0 or oe[1] > 0)


# ---- chi-square --------------------------------------------------------------------------------------------------------
def _native_expected(observed, partition_bp, total, genome):
    import ctypes as C

    from gtars_amd._lib import check, lib, ptr

    obs = np.asarray(observed, dtype=np.uint32)
    bp = np.asarray(partition_bp, dtype=np.uint64)
    out = [np.zeros(len(obs), dtype=np.float64) for _ in range(3)]
    check(lib.gtars_partition_expected(ptr(obs), ptr(bp), len(bp), int(total), int(genome), *(ptr(o) for o in out)))
    return [o.tolist() for o in out]


def test_chi_square_literals_and_early_returns():
    assert abs(P.chi_square_2x2(50.0, 50.0, 100.0) - 1.0) < 0.01
    assert P.chi_square_2x2(90.0, 10.0, 100.0) < 1e-3
    assert P.chi_square_2x2(5.0, 0.0, 0.0) == 1.0 and P.chi_square_2x2(5.0, 0.0, 10.0) == 1.0 and P.chi_square_2x2(5.0, 10.0, 10.0) == 1.0
    # the same through the compiled entry: expected = (bp / genome) * total
    _, _, pv = _native_expected([50, 50], [500], 100, 1000)
    assert abs(pv[0] - 1.0) < 0.01
    _, _, pv = _native_expected([90, 10], [100], 100, 1000)
    assert pv[0] < 1e-3
    assert _native_expected([5, 0], [500], 0, 1000)[2] == [1.0, 1.0]            # total == 0
    assert _native_expected([5, 5], [0], 10, 1000)[2][0] == 1.0                 # expected == 0
    assert _native_expected([5, 5], [1000], 10, 1000)[2] == [1.0, 1.0]          # total - expected == 0; intergenic expects 0


def test_native_expected_against_restatement_on_a_grid():
    # chi / 2 crosses a + 1 = 1.5 between the series and the continued fraction: obs == exp up to obs = 20 * exp
    genome, checked, branches = 1 << 20, 0, set()
    for total in (1, 7, 100, 12345, 4_000_000_000):
        for bp in (1, 1000, genome // 3, genome // 2, genome - 1):
            exp = bp / genome * total
            for obs in sorted({0, 1, total // 2, total, int(exp), int(exp) + 1, int(exp * 1.5) + 1, int(exp * 3) + 2, int(exp * 20) + 3}):
                if obs > 0xFFFFFFFF:
                    continue
                want = P.expected_rows([obs, obs], total, [bp], genome)
                got = _native_expected([obs, obs], [bp], total, genome)
                for w, g in zip(want, got):
                    for a, b in zip(w, g):
                        if math.isinf(a):
                            assert a == b
                        else:
                            assert b == pytest.approx(a, rel=1e-9, abs=1e-300)
                if total - exp != 0.0:
                    x = ((obs - exp) ** 2 / exp + ((total - obs) - (total - exp)) ** 2 / (total - exp)) / 2.0
                    branches.add(x < 1.5)
                checked += 1
    assert checked > 100 and branches == {True, False}


def test_native_expected_infinities_and_saturation():
    exp, oe, pv = _native_expected([0, 4, 6], [0, 3000], 10, 1000)  # the sizes exceed the genome: intergenic saturates at 0
    assert oe == [-math.inf, math.log10(4 / 30.0), math.inf] and exp == [0.0, 30.0, 0.0]
    assert P.expected_rows([0, 4, 6], 10, [0, 3000], 1000)[1] == oe
