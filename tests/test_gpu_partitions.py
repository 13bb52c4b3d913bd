"""Genomic partitions on the MI355X (csrc/partitions.hip, K14; the stranded setdiff on K8's sweep) against the plain-Python
restatement tests/partitions_ref.py: partition lists row for row, priority assignments per region, bp counts, the
expected / chi-square rows.  Nothing here compares the device with itself."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import annot_ref as A  # noqa: E402
import partitions_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regionset")
SIZES = {"chr1": 100000, "chr2": 80000, "chr3": 60000}
STRAND = "+-."
ALL6 = ["promoterCore", "promoterProx", "threeUTR", "fiveUTR", "exon", "intron"]


def _gold(name):
    return os.path.join(GOLD, name)


def _rs(regs):
    from gtars.models import RegionSet

    return RegionSet.from_vectors([r[0] for r in regs], [r[1] for r in regs], [r[2] for r in regs])


def _rows(rs):
    return [(r.chr, r.start, r.end) for r in rs.regions]


def _bed6(path, regs):
    path.write_text("".join(f"{c}\t{s}\t{e}\tn\t0\t{STRAND[st]}\n" for c, s, e, st in regs))
    return str(path)


def _model(tmp_path, genes, exons, three=None, five=None):
    """the same gene model on the device side (through BED6 files) and as the restatement's"""
    from gtars.models import GeneModel

    paths = [_bed6(tmp_path / f"{k}.bed", regs) if regs is not None else None
             for k, regs in (("genes", genes), ("exons", exons), ("three", three), ("five", five))]
    return GeneModel.from_bed_files(*paths), P.model_of(genes, exons, three, five)


def _same_list(pl, parts):
    assert pl.partition_names() == [n for n, _ in parts] and len(pl) == len(parts)
    for name, rows in parts:
        assert _rows(pl.partition(name)) == rows, name


def _bed_models():
    from gtars.models import GeneModel

    files = [_gold(f"test_{k}.bed") for k in ("genes", "exons", "three_utr", "five_utr")]
    return GeneModel.from_bed_files(*files), P.model_of(*(P.bed_stranded(f) for f in files))


def _fixture_query():
    from gtars.models import RegionSet

    q = RegionSet(_gold("test_query_promoter_enriched.bed"))
    return q, _rows(q)


# ---- surface ---------------------------------------------------------------------------------------------------------
def test_surface_and_errors():
    from gtars.partitions import calc_partitions  # noqa: F401
    from gtars.models import GeneModel, GenomicDistAnnotation
    from gtars.partitions import PartitionList

    with pytest.raises(ValueError):
        PartitionList.from_gtf(_gold("missing.gtf"), 100, 2000)
    m = GeneModel.from_bed_files(_gold("test_genes.bed"), _gold("test_exons.bed"), _gold("test_three_utr.bed"), _gold("test_five_utr.bed"))
    assert (m.n_genes, m.n_exons, len(m.three_utr), len(m.five_utr)) == (6, 19, 6, 6)
    assert repr(m) == "GeneModel(n_genes=6, n_exons=19)"
    m = GeneModel.from_bed_files(_gold("test_genes.bed"), _gold("test_exons.bed"))
    assert m.n_genes == 6 and m.three_utr is None and m.five_utr is None
    pl = PartitionList.from_gene_model(m, 100, 2000)
    assert pl.partition_names() == ["promoterCore", "promoterProx", "exon", "intron"] and len(pl) == 4
    assert repr(pl) == 'PartitionList(partitions=["promoterCore", "promoterProx", "exon", "intron"])'
    gda = GenomicDistAnnotation.from_gtf(_gold("test_gene_model.gtf"), True, False)
    assert PartitionList.from_annotation(gda, 100, 2000).partition_names() == ALL6
    assert PartitionList.from_gtf(_gold("test_gene_model_ensembl.gtf"), 100, 2000, False, True).partition_names() == ALL6


@pytest.mark.parametrize("name,pc", [("test_gene_model.gtf", False), ("test_gene_model.gtf", True), ("test_gene_model_ensembl.gtf", False),
                                     ("C_elegans_cropped_example.gtf.gz", False), ("C_elegans_cropped_example.gtf.gz", True)])
def test_gtf_models_row_for_row(name, pc):
    from gtars.models import GeneModel
    from gtars.partitions import PartitionList

    path = _gold(name)
    rows = A.read_gtf(path, pc, False)
    three, five = P.gtf_utr_rows(P.read_bytes(path), pc, False)
    ref = P.model_of([r[:4] for r in rows if r[4] == A.GENE], [r[:4] for r in rows if r[4] == A.EXON], three, five)
    m = GeneModel.from_gtf(path, pc, False)
    for key, got in (("three_utr", m.three_utr), ("five_utr", m.five_utr)):
        assert (got is None) == (ref[key] is None)
        if got is not None:
            assert _rows(got) == P.unstrand(ref[key])
    _same_list(PartitionList.from_gene_model(m, 100, 2000), P.partition_list(ref, 100, 2000))


# ---- partition list rules ----------------------------------------------------------------------------------------------
def test_list_rules_literals(tmp_path):
    from gtars.partitions import PartitionList

    m, ref = _bed_models()
    pl = PartitionList.from_gene_model(m, 100, 2000)
    assert pl.partition_names() == ALL6
    _same_list(pl, P.partition_list(ref, 100, 2000))
    _same_list(PartitionList.from_gene_model(m, 100, 2000, SIZES), P.partition_list(ref, 100, 2000, SIZES))
    # one unstranded gene
    m, ref = _model(tmp_path, [("chr1", 5000, 10000, 2)], [("chr1", 5000, 5500, 2), ("chr1", 9000, 10000, 2)])
    pl = PartitionList.from_gene_model(m, 100, 2000)
    assert _rows(pl.partition("promoterCore")) == [("chr1", 4900, 5000)] and _rows(pl.partition("promoterProx")) == [("chr1", 3000, 4900)]
    _same_list(pl, P.partition_list(ref, 100, 2000))
    # strand-aware placement from the GTF fixture
    core = _rows(PartitionList.from_gtf(_gold("test_gene_model.gtf"), 100, 2000, True, False).partition("promoterCore"))
    assert [r for r in core if r[0] == "chr2"] == [("chr2", 8000, 8100)] and [r for r in core if r[0] == "chr1"] == [("chr1", 900, 1000)]
    m, ref = _model(tmp_path, [("chr1", 1000, 5000, 0), ("chr1", 6000, 9000, 1)], [("chr1", 1000, 1500, 0), ("chr1", 6000, 6500, 1)])
    pl = PartitionList.from_gene_model(m, 100, 2000)
    assert sorted(r[1] for r in _rows(pl.partition("promoterCore"))) == [900, 9000]
    _same_list(pl, P.partition_list(ref, 100, 2000))


def test_list_rules_saturation_trim_and_strands(tmp_path):
    from gtars.partitions import PartitionList

    genes = [("chr1", 50, 500, 0),               # saturates at 0
             ("chr1", 3000, 4294967200, 1),      # minus strand: [end, end + up) saturates at u32::MAX
             ("chr2", 900, 990, 1),              # with sizes: clipped to [990, 1000)
             ("chr2", 995, 1000, 1),             # with sizes: zero width after the clip, dropped
             ("chr2", 1200, 1500, 1),            # with sizes: start beyond the size, dropped
             ("chrU", 100, 990, 1)]              # no size for the chromosome: kept as it is
    # a + prox that overlaps a - core: + gene at 1300 gives prox [300, 1200) (core [1200, 1300)); the - gene ending at 1000
    # has core [1000, 1100), which a strand-blind setdiff would cut out of it
    genes += [("chr4", 1300, 2000, 0), ("chr4", 500, 1000, 1)]
    exons = [(c, s, min(s + 50, e), st) for c, s, e, st in genes]
    m, ref = _model(tmp_path, genes, exons)
    sizes = {"chr1": 4294967295, "chr2": 1000, "chr4": 5000}
    for cs in (None, sizes):
        pl = PartitionList.from_gene_model(m, 100, 1000, cs)
        _same_list(pl, P.partition_list(ref, 100, 1000, cs))
    core, prox = _rows(pl.partition("promoterCore")), _rows(pl.partition("promoterProx"))
    assert ("chr1", 0, 50) in core and ("chr1", 4294967200, 4294967295) in core
    assert [r for r in core if r[0] == "chr2"] == [("chr2", 990, 1000)] and ("chrU", 990, 1090) in core
    assert ("chr4", 300, 1200) in prox and ("chr4", 1000, 1100) in core
    nosize = _rows(PartitionList.from_gene_model(m, 100, 1000).partition("promoterCore"))
    assert [r for r in nosize if r[0] == "chr2"] == [("chr2", 990, 1100), ("chr2", 1500, 1600)]  # the first two merge: one strand


def test_stranded_setdiff_free_form():
    # the stranded sweep itself, outside well-formed gene models: inverted and zero-length rows on either side, duplicates,
    # rows that touch, three strand codes, a chromosome only one side has -- against the reference's loop
    from gtars_amd import models as M

    rng = np.random.default_rng(21)

    def side(n, names):
        s = rng.integers(0, 1500, n)
        w = rng.choice([-30, 0, 0, 1, 40, 300], n)
        return [(str(c), int(a), int(max(a + b, 0)), int(st)) for c, a, b, st in zip(rng.choice(names, n), s, w, rng.integers(0, 3, n))]

    for na, nb in ((1, 0), (0, 5), (65, 40), (300, 257)):
        a, b = side(na, ["chr1", "chr2", "chrA"]), side(nb, ["chr1", "chr2", "chrB"])
        sets = [M._Stranded(_rs(x), np.array([r[3] for r in x], dtype=np.uint8)) for x in (a, b)]
        got = M._stranded_setdiff(*sets)
        rows = [(c, s, e, int(st)) for (c, s, e), st in zip(_rows(got.regions), got.strands)]
        assert rows == P.stranded_setdiff(a, b), (na, nb)


def test_partition_mutual_exclusivity():
    from gtars.partitions import PartitionList

    m, _ = _bed_models()
    pl = PartitionList.from_gene_model(m, 100, 2000)
    sets = [pl.partition(n) for n in pl.partition_names()]
    for i in range(len(sets)):
        for j in range(i + 1, len(sets)):
            if len(sets[i]) and len(sets[j]):
                assert not any(sets[j].find_overlaps(sets[i])), (i, j)


# ---- literal cases of both modes ---------------------------------------------------------------------------------------
def test_priority_literals(tmp_path):
    from gtars.partitions import calc_partitions, partition_assignments
    from gtars.partitions import PartitionList

    m, _ = _model(tmp_path, [("chr1", 100, 1000, 2)], [("chr1", 50, 150, 2)])
    pl = PartitionList.from_gene_model(m, 100, 200)
    r = calc_partitions(_rs([("chr1", 0, 120)]), pl)
    assert r["partition"] == ["promoterCore", "promoterProx", "exon", "intron", "intergenic"]
    assert r["count"] == [1, 0, 0, 0, 0] and r["total"] == 1
    assert pl.device == 0
    m, ref = _bed_models()
    pl = PartitionList.from_gene_model(m, 100, 2000)
    r = calc_partitions(_rs([("chr1", 50000, 50200)]), pl)
    assert r["count"][-1] == 1 and sum(r["count"]) == 1
    q, qrows = _fixture_query()
    r = calc_partitions(q, pl)
    assert sum(r["count"]) == r["total"] == len(q)
    parts = P.partition_list(ref, 100, 2000)
    assert (r["count"], r["total"]) == P.calc_partitions(qrows, parts)
    assert partition_assignments(q, pl).tolist() == P.assignments(qrows, parts)
    # an empty query set
    r = calc_partitions(_rs([]), pl)
    assert r["count"] == [0] * 7 and r["total"] == 0 and len(partition_assignments(_rs([]), pl)) == 0
    assert calc_partitions(_rs([]), pl, True)["count"] == [0] * 7


def test_bp_literals(tmp_path):
    from gtars.partitions import calc_partitions
    from gtars.partitions import PartitionList

    m, ref = _model(tmp_path, [("chr1", 1000, 5000, 2)], [("chr1", 1000, 2000, 2)])
    pl = PartitionList.from_gene_model(m, 100, 200)
    r = calc_partitions(_rs([("chr1", 750, 950)]), pl, True)
    prom = r["count"][0] + r["count"][1]
    assert r["total"] == 200 and prom > 0 and r["count"][-1] > 0 and prom + r["count"][-1] == 200
    assert (r["count"], r["total"]) == P.calc_partitions([("chr1", 750, 950)], P.partition_list(ref, 100, 200), True)
    m, ref = _bed_models()
    pl = PartitionList.from_gene_model(m, 100, 2000)
    q, qrows = _fixture_query()
    r = calc_partitions(q, pl, bp_proportion=True)
    assert sum(r["count"]) == r["total"] == sum(e - s for _, s, e in qrows)
    assert (r["count"], r["total"]) == P.calc_partitions(qrows, P.partition_list(ref, 100, 2000), True)


# ---- random sets against the restatement -------------------------------------------------------------------------------
N_SIZES = [1, 63, 64, 65, 255, 257, 5000]


def _random_model(rng):
    genes, exons, three, five = [], [], [], []
    for c in ("chr1", "chr2", "chr3"):
        for _ in range(100):
            s = int(rng.integers(3000, 400_000))
            e = s + int(rng.integers(300, 6000))
            st = int(rng.integers(0, 3))
            genes.append((c, s, e, st))
            for _ in range(int(rng.integers(1, 4))):
                a = int(rng.integers(s, e - 50))
                exons.append((c, a, min(a + int(rng.integers(20, 800)), e), st))
            three.append((c, e - int(rng.integers(20, 200)), e, st))
            # some 5'UTRs lie inside a 3'UTR of their strand
            five.append((c, e - 15, e - 5, st) if rng.random() < 0.3 else (c, s, s + int(rng.integers(20, 200)), st))
    genes.append(("chrL", 1000, 5000, 0))  # a chromosome no query has
    exons.append(("chrL", 1000, 1200, 0))
    return genes, exons, three, five


@pytest.fixture(scope="module")
def random_case(tmp_path_factory):
    """one model, 5000 unsorted queries, and the restatement's assignments for them, computed once"""
    from gtars.partitions import PartitionList

    rng = np.random.default_rng(14)
    m, ref = _model(tmp_path_factory.mktemp("k14"), *_random_model(rng))
    parts = P.partition_list(ref, 100, 2000)
    pl = PartitionList.from_gene_model(m, 100, 2000)
    _same_list(pl, parts)
    n = max(N_SIZES)
    chrom = rng.choice(["chr1", "chr2", "chr3", "chrQ"], n, p=[0.4, 0.3, 0.25, 0.05])  # chrQ: absent from the list
    start = rng.integers(0, 420_000, n)
    width = np.where(rng.random(n) < 0.1, 0, rng.integers(1, 3000, n))  # zero-length queries among them
    query = [(str(c), int(s), int(s + w)) for c, s, w in zip(chrom, start, width)]
    return pl, parts, query, P.assignments(query, parts)


@pytest.mark.parametrize("n", N_SIZES)
def test_random_priority(random_case, n):
    from gtars.partitions import calc_partitions, partition_assignments

    pl, parts, query, want = random_case
    q = _rs(query[:n])
    assert partition_assignments(q, pl).tolist() == want[:n]
    r = calc_partitions(q, pl)
    assert r["count"] == [want[:n].count(k) for k in range(len(parts) + 1)] and r["total"] == n
    if n == max(N_SIZES):
        assert all(c > 0 for c in r["count"][:3]) and r["count"][-1] > 0


@pytest.mark.parametrize("n", N_SIZES)
def test_random_bp(random_case, n):
    from gtars.partitions import calc_partitions

    pl, parts, query, _ = random_case
    r = calc_partitions(_rs(query[:n]), pl, True)
    assert (r["count"], r["total"]) == P.calc_partitions(query[:n], parts, True)


def _free_list(sets):
    """a partition list straight from region sets (rows of any shape), and the same for the restatement"""
    from gtars.partitions import PartitionList

    names = [f"p{k}" for k in range(len(sets))]
    return PartitionList._from_sets(names, [_rs(s) for s in sets]), list(zip(names, sets))


def _check_free(sets, query):
    from gtars.partitions import calc_partitions, partition_assignments

    pl, parts = _free_list(sets)
    q = _rs(query)
    want = P.assignments(query, parts)
    assert partition_assignments(q, pl).tolist() == want
    assert calc_partitions(q, pl)["count"] == [want.count(k) for k in range(len(parts) + 1)]
    r = calc_partitions(q, pl, True)
    assert (r["count"], r["total"]) == P.calc_partitions(query, parts, True)
    return want, r


def test_edges_touching_zero_length_and_inverted():
    sets = [[("chr1", 100, 200), ("chr1", 150, 150)],       # a zero-length row inside another row
            [],                                               # an empty partition
            [("chr1", 300, 300), ("chr1", 500, 400)],       # a zero-length row on its own; an inverted row (side list)
            [("chr1", 50, 600), ("chr2", 10, 20)]]
    query = [("chr1", 50, 100), ("chr1", 200, 250),          # qe == start, qs == end of p0's row: no hit there -> p3
             ("chr1", 120, 120),                             # zero-length query strictly inside a row: hit
             ("chr1", 150, 150),                             # ... on a zero-length row's position: the other row still hits
             ("chr1", 290, 310),                             # a zero-length partition row strictly inside the query: p2
             ("chr1", 300, 310), ("chr1", 290, 300),         # ... touching it: p3
             ("chr1", 600, 700), ("chr1", 0, 50),            # touching p3 from either side: intergenic
             ("chr1", 450, 420), ("chr1", 650, 350), ("chr1", 510, 390),  # inverted queries: the literal test per row
             ("chr1", 390, 510),                             # a well-formed query over the inverted row: 500 < 510 and 400 > 390 -> p2
             ("chr1", 700, 650), ("chr2", 15, 12), ("chr3", 1, 2)]
    want, _ = _check_free(sets, query)
    assert want[:9] == [3, 3, 0, 0, 2, 3, 3, 4, 4] and want[12] == 2 and want[-3:] == [4, 3, 4]


def test_edges_random_free_form():
    # rows that overlap inside a partition, inverted and zero-length rows and queries, duplicates, all at random
    rng = np.random.default_rng(7)

    def regs(n, names):
        s = rng.integers(0, 3000, n)
        w = rng.choice([-40, 0, 0, 5, 60, 400], n)
        return [(str(c), int(a), int(max(a + b, 0))) for c, a, b in zip(rng.choice(names, n), s, w)]

    sets = [regs(60, ["chr1", "chr2"]), regs(5, ["chr2"]), [], regs(200, ["chr1", "chr2", "chr3"])]
    _check_free(sets, regs(700, ["chr1", "chr2", "chr3", "chr4"]))


def test_bp_overlapping_rows_saturation_and_wrap():
    # two opposite-strand promoters that overlap stay two rows of one partition: a query's bp count once per row
    from gtars.partitions import calc_partitions

    sets = [[("chr1", 1000, 2000), ("chr1", 1500, 2500)], [("chr1", 0, 5000)]]
    want, r = _check_free(sets, [("chr1", 1400, 1600)])
    assert r["count"] == [300, 200, 0] and r["total"] == 200  # assigned 500 > total 200: the remainder saturates at 0
    # u64 sums beyond 2^32 wrap as the reference's u32 does: 3 rows x 2 queries x 4e9
    big = 4_000_000_000
    sets = [[("chrB", 0, big)] * 3, [("chrB", 5, big)]]
    pl, parts = _free_list(sets)
    query = [("chrB", 0, big), ("chrB", 0, big), ("chrB", 10, 20)]
    r = calc_partitions(_rs(query), pl, True)
    assert (r["count"], r["total"]) == P.calc_partitions(query, parts, True)
    assert r["count"][0] == (6 * big + 30) % (1 << 32) and r["total"] == (2 * big + 10) % (1 << 32)


# ---- calc_expected_partitions ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bp", [False, True])
def test_expected_partitions(bp):
    from gtars.partitions import calc_expected_partitions
    from gtars.partitions import PartitionList

    m, ref = _bed_models()
    pl = PartitionList.from_gene_model(m, 100, 2000)
    q, qrows = _fixture_query()
    r = calc_expected_partitions(q, pl, SIZES, bp)
    assert {"promoterCore", "promoterProx", "exon", "intron", "intergenic"} <= set(r["partition"])
    assert all(0.0 <= p <= 1.0 for p in r["pvalue"])
    if not bp:
        oe = dict(zip(r["partition"], r["log10OE"]))
        assert oe["promoterCore"] > 0 or oe["promoterProx"] > 0
    counts, exp, oe, pv = P.calc_expected_partitions(qrows, P.partition_list(ref, 100, 2000), SIZES, bp)
    assert r["observed"] == [float(c) for c in counts]
    for key, want in (("expected", exp), ("log10OE", oe), ("pvalue", pv)):
        for g, w in zip(r[key], want):
            assert g == w if math.isinf(w) else g == pytest.approx(w, rel=1e-9), key
    one = calc_expected_partitions(_rs([("chr1", 500, 600)]), pl, SIZES)
    assert len(one["partition"]) == 7 and one["log10OE"].count(-math.inf) == 6


# ---- the device-pointer entry and the index's device ------------------------------------------------------------------
def test_device_pointer_entry_and_device_scope(random_case):
    import torch

    from gtars.partitions import calc_partitions, partition_assignments, partitions_count_device

    pl, parts, query, want = random_case
    n = 3000
    names = pl.chrom_names
    qc = np.array([names.index(c) if c in names else 0xFFFFFFFF for c, _, _ in query[:n]], dtype=np.uint32)
    qs = np.array([s for _, s, _ in query[:n]], dtype=np.uint32)
    qe = np.array([e for _, _, e in query[:n]], dtype=np.uint32)
    host = calc_partitions(_rs(query[:n]), pl)
    host_bp = calc_partitions(_rs(query[:n]), pl, True)
    dev = torch.device("cuda", pl.device)
    with torch.cuda.device(dev):
        d = [torch.from_numpy(x.view(np.int32)).to(dev) for x in (qc, qs, qe)]
        assign = torch.full((n,), 255, dtype=torch.uint8, device=dev)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            counts, total = partitions_count_device(pl, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n, stream.cuda_stream,
                                                    d_assign=assign.data_ptr())
            counts_bp, total_bp = partitions_count_device(pl, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n, stream.cuda_stream, True)
    assert counts.tolist() == host["count"] and total == host["total"] == n
    assert assign.cpu().tolist() == want[:n]
    assert counts_bp.tolist() == host_bp["count"] and total_bp == host_bp["total"]
    if torch.cuda.device_count() > 1:  # a host call made on another device follows the index's
        with torch.cuda.device((pl.device + 1) % torch.cuda.device_count()):
            assert partition_assignments(_rs(query[:n]), pl).tolist() == want[:n]
        assert pl.device == dev.index
