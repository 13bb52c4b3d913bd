"""TSS / feature distances and gene models on the MI355X (csrc/annot.hip, K10; the stranded reduce on K8's device reduce)
against the plain-Python restatement tests/annot_ref.py: seeded differentials with exact equality.  The literal cases, the
interleaved batch and the index sizes around the staged sample are answered by both forms of the distance kernel on ONE index:
k_tss_dist<true> (the sampled keys staged in LDS, the default) and k_tss_dist<false> (GTARS_TSS_GLOBAL_SEARCH=1)."""
import gzip
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import annot_ref as A  # noqa: E402
import edge_layouts as E  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regionset")
U32 = 0xFFFFFFFF
GTFS = ["test_gene_model.gtf", "test_gene_model_ensembl.gtf", "C_elegans_cropped_example.gtf.gz"]


def _rs(regs):
    from gtars.models import RegionSet

    return RegionSet.from_vectors([r[0] for r in regs], [r[1] for r in regs], [r[2] for r in regs])


@pytest.fixture
def search_forms(monkeypatch):
    """-> a generator function: GTARS_TSS_GLOBAL_SEARCH unset, then "1" (the library takes a new snapshot of its switches at
    every change, so a handle built before the change is answered by the other kernel)"""
    def forms():
        monkeypatch.delenv("GTARS_TSS_GLOBAL_SEARCH", raising=False)
        yield "lds"
        monkeypatch.setenv("GTARS_TSS_GLOBAL_SEARCH", "1")
        yield "global"
        monkeypatch.delenv("GTARS_TSS_GLOBAL_SEARCH")

    return forms


def _check(index_regs, query_regs, tss=None, forms=None):
    """one index (its device image is built once), the queries under every search form of `forms` (default: as the process is)"""
    from gtars.models import TssIndex

    tss = tss or TssIndex.from_regionset(_rs(index_regs))
    q = _rs(query_regs)
    want_abs, want_signed = A.distances(A.build_index(index_regs), query_regs)
    for form in (forms() if forms else ["default"]):
        assert tss.calc_tss_distances(q) == want_abs, form
        assert tss.feature_distances(q) == want_signed, form
    return tss


def _random_regs(rng, n, names, span, width=(0, 2000)):
    c = rng.choice(names, n)
    s = rng.integers(0, span, n)
    e = s + rng.integers(width[0], width[1], n)
    return c, s.astype(np.int64), np.minimum(e, U32).astype(np.int64)


def _tuples(c, s, e, order=None):
    idx = range(len(c)) if order is None else order
    return [(str(c[i]), int(s[i]), int(e[i])) for i in idx]


def test_literal_cases(search_forms):
    from gtars.models import Region, RegionSet, TssIndex

    feats = RegionSet.from_regions([Region("chr1", 100, 101)])
    tss = TssIndex.from_regionset(feats)
    # models.rs: dummy.narrowPeak against dummy_tss.bed
    t = TssIndex(os.path.join(GOLD, "dummy_tss.bed"))
    peaks = RegionSet(os.path.join(GOLD, "dummy.narrowPeak"))
    for form in search_forms():
        q = RegionSet.from_regions([Region("chr1", 200, 210)])
        assert tss.calc_tss_distances(q) == [105], form
        assert tss.feature_distances(q) == [-105.0], form
        assert tss.feature_distances(RegionSet.from_regions([Region("chr2", 200, 210)])) == [None], form
        assert tss.calc_tss_distances(RegionSet.from_regions([Region("chr2", 200, 210)])) == [U32], form
        d = t.calc_tss_distances(peaks)
        sg = t.feature_distances(peaks)
        assert len(d) == 9 and min(d) == 2 and [abs(int(v)) for v in sg] == d, form
    _check([(r.chr, r.start, r.end) for r in RegionSet(os.path.join(GOLD, "dummy_tss.bed"))],
           [(r.chr, r.start, r.end) for r in peaks], t, search_forms)
    import gtars_amd

    assert gtars_amd._lib.lib.gtars_tss_index_device(t._h) == 0


@pytest.mark.parametrize("n_index", [60_000, 1_000_000])
def test_million_queries_sorted_and_shuffled(n_index):
    rng = np.random.default_rng(n_index)
    names = np.array([f"chr{k}" for k in range(1, 23)] + ["chrX", "chrY"])
    ic, is_, ie = _random_regs(rng, n_index, names[:-1], 250_000_000, (0, 3))
    index = _tuples(ic, is_, ie)
    qc, qs, qe = _random_regs(rng, 1_000_000, names, 250_000_000)
    # BED-like order: sorted by (chr, start) -- grouped, answered in place
    order = sorted(range(len(qc)), key=lambda i: (qc[i], qs[i]))
    tss = _check(index, _tuples(qc, qs, qe, order))
    # shuffled: chromosomes interleave, the results come back grouped by first appearance
    _check(index, _tuples(qc, qs, qe), tss)


def test_interleaved_missing_chromosomes_and_edges(search_forms):
    rng = np.random.default_rng(11)
    index = [("a", 10, 11), ("a", 20, 21), ("a", 20, 21), ("a", 30, 31), ("b", U32 - 3, U32), ("b", 7, 3),
             ("c", 0, 0), ("c", U32, U32), ("d", 5, 9)]
    q = [("b", 0, 1), ("zz", 1, 2), ("a", 15, 16), ("a", 20, 20), ("c", 5, 1), ("a", 24, 26), ("b", U32 - 1, U32),
         ("zz", 9, 9), ("a", 0, 1), ("a", 40, 41), ("c", U32, U32), ("c", 0, 0), ("d", 7, 7), ("d", 6, 8), ("yy", 3, 4)]
    _check(index, q, forms=search_forms)
    # random interleaving over few positions: many exact hits, duplicate midpoints, equal-distance ties
    names = ["a", "b", "c", "d", "e", "zz"]
    idx = [(str(rng.choice(names[:4])), int(s), int(s) + int(w)) for s, w in
           zip(rng.integers(0, 400, 3000), rng.choice([0, 1, 2, 4], 3000))]
    qq = []
    for _ in range(50_000):
        s = int(rng.integers(0, 420))
        e = s + int(rng.integers(0, 9)) if rng.random() > 0.1 else max(s - int(rng.integers(1, 9)), 0)
        if rng.random() < 0.02:
            s, e = U32 - int(rng.integers(0, 5)), int(rng.choice([U32, 3]))
        qq.append((str(rng.choice(names)), s, e))
    _check(idx, qq, forms=search_forms)


def test_empty_query_and_empty_index():
    from gtars.models import TssIndex

    tss = TssIndex.from_regionset(_rs([("chr1", 5, 9)]))
    assert tss.calc_tss_distances(_rs([])) == [] and tss.feature_distances(_rs([])) == []
    empty = TssIndex.from_regionset(_rs([]))
    assert len(empty) == 0
    assert empty.calc_tss_distances(_rs([("chr1", 5, 9), ("chr2", 1, 2)])) == [U32, U32]
    assert empty.feature_distances(_rs([("chr1", 5, 9)])) == [None]


def _model_rows(gm):
    out = []
    for part in (gm._genes, gm._exons):
        rs = part.regions
        names, ids, s, e = rs.chrom_names, rs.chrom_ids, rs.starts, rs.ends
        out.append([(names[int(ids[i])], int(s[i]), int(e[i]), int(part.strands[i])) for i in range(len(rs))])
    return out


def _check_model(path, pc, cv, rng):
    from gtars.models import GeneModel, GenomicDistAnnotation

    genes, exons = A.gene_model(A.read_gtf(path, pc, cv))
    gm = GeneModel.from_gtf(path, pc, cv)
    assert (gm.n_genes, gm.n_exons) == (len(genes), len(exons))
    assert _model_rows(gm) == [genes, exons]
    assert repr(gm) == f"GeneModel(n_genes={len(genes)}, n_exons={len(exons)})"
    gda = GenomicDistAnnotation.from_gtf(path, pc, cv)
    assert repr(gda) == f"GenomicDistAnnotation(n_genes={len(genes)}, n_exons={len(exons)})"
    assert gda.gene_model().n_genes == len(genes)
    tss_regs = A.tss_regions(genes)
    tss = gda.tss_index()
    assert len(tss) == len(tss_regs)
    names = sorted({g[0] for g in genes} | {"chrUn"})
    hi = max([g[2] for g in genes] + [10_000]) + 1000
    q = [(str(rng.choice(names)), int(s), int(s) + int(w)) for s, w in zip(rng.integers(0, hi, 3000), rng.integers(0, 500, 3000))]
    q += [(c, p, p + 1) for c, p, _ in tss_regs]
    _check(tss_regs, q, tss)


@pytest.mark.parametrize("name", GTFS)
def test_gene_models_of_fixtures(name):
    rng = np.random.default_rng(5)
    for pc in (True, False):
        for cv in (True, False):
            _check_model(os.path.join(GOLD, name), pc, cv, rng)
    from gtars.models import GeneModel, GenomicDistAnnotation, RegionSet

    if name == "test_gene_model.gtf":
        gm = GeneModel.from_gtf(os.path.join(GOLD, name))
        assert gm.n_genes == 2 and gm.n_exons > 0
        assert GeneModel.from_gtf(os.path.join(GOLD, name), filter_protein_coding=False).n_genes == 3
        tss = GenomicDistAnnotation.from_gtf(os.path.join(GOLD, name)).tss_index()
        assert tss.calc_tss_distances(RegionSet.from_vectors(["chr1"], [1000], [1001])) == [0]


def test_gene_model_synthetic_200k_rows(tmp_path):
    rng = np.random.default_rng(200)
    n = 200_000
    chrs = rng.choice(["1", "2", "X", "chr3", "MT", "chr10"], n)
    feats = rng.choice(["gene", "exon", "exon", "exon", "CDS", "UTR", "transcript"], n)
    s = rng.integers(1, 3_000_000, n)
    e = s + rng.integers(-50, 30_000, n)  # some inverted rows
    strand = rng.choice(["+", "-", "."], n, p=[0.45, 0.45, 0.1])
    bio = rng.choice(['gene_biotype "protein_coding";', 'gene_type "protein_coding";', 'gene_biotype "lncRNA";'], n)
    lines = [f"{chrs[i]}\tsyn\t{feats[i]}\t{s[i]}\t{max(int(e[i]), 0)}\t.\t{strand[i]}\t.\t{bio[i]}" for i in range(n)]
    data = ("##synthetic\n" + "\n".join(lines) + "\n").encode()
    p = tmp_path / "syn.gtf.gz"
    half = len(data) // 2
    p.write_bytes(gzip.compress(data[:half]) + gzip.compress(data[half:]))
    for pc in (True, False):
        _check_model(str(p), pc, True, rng)


@pytest.mark.parametrize("n_index,boundary", E.edge_cases())
def test_index_sizes_around_the_staged_sample(n_index, boundary, search_forms):
    """index sizes on the edges of a lane, a wave, a workgroup and the 2048 sampled keys a workgroup stages, on one
    chromosome and on two whose second begins at index 2048 resp. 2047 of the (chromosome, midpoint) order; 50 000
    queries with exact hits on the first and the last midpoint of every chromosome; both search forms on the one index"""
    rng = np.random.default_rng(6000 + n_index)
    ic, is_, ie = _random_regs(rng, n_index, ["chr10"], 3_000_000, (0, 3))
    index = _tuples(ic, is_, ie)
    if boundary is not None:
        index = E.split_at(index, boundary, key=lambda r: A.midpoint(r[1], r[2]))
        assert sum(1 for r in index if r[0] == "chr10") == boundary
        first = next(i for i, r in enumerate(index) if r[0] == "chr10")
        index[0], index[first] = index[first], index[0]  # "chr10" also appears first: it is the first chromosome either way
    qc, qs, qe = _random_regs(rng, 50_000, ["chr10", "chr2", "chr3"], 3_000_100, (0, 50))
    q = _tuples(qc, qs, qe)
    for name in sorted({c for c, _, _ in index}):
        mids = sorted(A.midpoint(s, e) for c, s, e in index if c == name)
        q += [(name, mids[0], mids[0] + 1), (name, mids[-1], mids[-1] + 1), (name, mids[0], mids[0]), (name, mids[-1], mids[-1])]
    _check(index, q, forms=search_forms)
