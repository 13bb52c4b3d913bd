"""TSS / feature distances and GTF gene models without a GPU: the plain-Python restatement (tests/annot_ref.py) against
the reference's literal cases, its own brute-force form and the R-derived ce_ref_* beds; the C++ GTF reader against the
restatement on seeded synthetic GTFs; construction, len and repr on the host; the device calls refusing to compute (no
CPU fallback); the new import surface."""
import gzip
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import annot_ref as A  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regionset")
U32 = 0xFFFFFFFF


def _gold(name):
    return os.path.join(GOLD, name)


def _bed(name):
    out = []
    for line in open(_gold(name)):
        f = line.rstrip("\n").split("\t")
        if len(f) >= 3:
            out.append((f[0], int(f[1]), int(f[2])))
    return sorted(out, key=lambda r: (r[0].encode(), r[1]))


def _rs(regs):
    from gtars.models import RegionSet

    return RegionSet.from_vectors([r[0] for r in regs], [r[1] for r in regs], [r[2] for r in regs])


def _no_gpu():
    import gtars_amd

    return gtars_amd.device_count() == 0


# ------------------------------------------------------------------------------------------------------ import surface
def test_annotation_classes_import_from_gtars_models():
    from gtars.models import GeneModel, GenomicDistAnnotation, TssIndex
    import gtars.models as M

    assert TssIndex.__module__ == GeneModel.__module__ == GenomicDistAnnotation.__module__ == "gtars_amd.models"
    for absent in ("PartitionList", "GenomeAssembly", "BinaryGenomeAssembly", "SignalMatrix"):
        assert not hasattr(M, absent), absent
    from gtars.models import GenomicDistAnnotation as G

    assert not hasattr(G, "partition_list") and not hasattr(G, "load_bin")
    import gtars.genomic_distributions as gd

    for absent in ("calc_gc_content", "calc_partitions", "calc_summary_signal"):
        assert not hasattr(gd, absent), absent


# ---------------------------------------------------------------------------------------- the restatement, literally
def test_ref_python_binding_cases():
    # gtars-python/tests/test_genomicdist.py TestTssIndex
    idx = A.build_index([("chr1", 100, 101)])
    assert A.distances(idx, [("chr1", 200, 210)]) == ([105], [-105.0])
    assert A.distances(idx, [("chr2", 200, 210)]) == ([U32], [None])
    assert len(A.build_index([("chr1", 100, 101), ("chr1", 500, 501)])["chr1"]) == 2


def test_ref_sentinels_for_missing_chromosome():
    # models.rs test_tss_distances_sentinel_for_missing_chrom / test_feature_distances_sentinel_for_missing_chrom
    idx = A.build_index([("chr1", 50, 51)])
    q = [("chr1", 40, 45), ("chr2", 10, 20)]
    assert A.distances(idx, q) == ([8, U32], [8.0, None])


def test_ref_dummy_peaks_against_dummy_tss():
    # models.rs test_calc_tss_distances / test_calc_feature_distances: 9 values, min 2, |signed| == abs, both signs
    from gtars.models import RegionSet

    peaks = RegionSet(_gold("dummy.narrowPeak"))
    q = [(r.chr, r.start, r.end) for r in peaks]
    idx = A.build_index(_bed("dummy_tss.bed"))
    ab, sg = A.distances(idx, q)
    assert len(ab) == 9 and min(ab) == 2
    assert [abs(int(v)) for v in sg] == ab
    assert any(v > 0 for v in sg) and any(v < 0 for v in sg)


def test_ref_ties_exact_hits_and_wrapping():
    idx = A.build_index([("c", 10, 11), ("c", 20, 21), ("c", 20, 21), ("c", 30, 31)])
    # midpoint 15: 5 to 10 and 5 to 20 -> the upstream one; 20 exact; 25 tie again; 40 beyond the last
    assert A.distances(idx, [("c", 15, 16), ("c", 20, 20), ("c", 24, 26), ("c", 40, 41), ("c", 0, 1)]) == (
        [5, 0, 5, 10, 10], [-5.0, 0.0, -5.0, -10.0, 10.0])
    # an inverted region's width wraps: start + (end - start mod 2^32) / 2 mod 2^32
    assert A.midpoint(10, 4) == (10 + (2 ** 32 - 6) // 2) & U32
    assert A.midpoint(U32 - 1, U32) == U32 - 1


def test_ref_output_order_is_first_appearance():
    idx = A.build_index([("a", 0, 2), ("b", 100, 102)])
    q = [("b", 90, 92), ("a", 5, 7), ("b", 110, 112), ("a", 1, 3)]
    assert A.distances(idx, q)[0] == [10, 10, 5, 1]


@pytest.mark.parametrize("seed", range(6))
def test_ref_bisect_equals_brute_force(seed):
    rng = np.random.default_rng(seed)
    names = ["chr1", "chr2", "chrX", "chrY"]
    n_idx, n_q = int(rng.integers(0, 80)), int(rng.integers(0, 300))
    span = int(rng.choice([50, 5000]))
    regs = []
    for _ in range(n_idx):
        s = int(rng.integers(0, span))
        regs.append((str(rng.choice(names[:3])), s, s + int(rng.integers(0, 20))))
    q = []
    for _ in range(n_q):
        s = int(rng.integers(0, span))
        e = s + int(rng.integers(0, 30)) if rng.random() > 0.1 else max(s - int(rng.integers(1, 9)), 0)
        if rng.random() < 0.05:
            s, e = U32 - int(rng.integers(0, 10)), U32
        q.append((str(rng.choice(names)), s, e))
    assert A.distances(A.build_index(regs), q) == A.distances_brute(regs, q)


def test_ref_gene_model_fixture_counts():
    # gtars-python TestGeneModel: 2 protein-coding genes, 3 in all
    rows = A.read_gtf(_gold("test_gene_model.gtf"))
    genes, exons = A.gene_model(rows)
    assert len(genes) == 2 and len(exons) > 0
    assert len(A.gene_model(A.read_gtf(_gold("test_gene_model.gtf"), filter_protein_coding=False))[0]) == 3
    # TestGenomicDistAnnotation.test_tss_index_strand_aware: TSS at 1000 (+) and 7999 (-)
    assert sorted(A.tss_regions(genes)) == [("chr1", 1000, 1001), ("chr2", 7999, 8000)]
    ens, _ = A.gene_model(A.read_gtf(_gold("test_gene_model_ensembl.gtf")))
    assert [g[0] for g in ens] == ["chr1", "chrX"]


@pytest.mark.parametrize("pc, tag", [(True, "pc"), (False, "all")])
def test_ref_against_r_gene_models(pc, tag):
    # partitions.rs test_gtf_vs_r_protein_coding / _all_features: from_gtf(path, pc, convert=False), then an
    # unstranded reduce, against getGeneModelsFromGTF's beds
    genes, exons = A.gene_model(A.read_gtf(_gold("C_elegans_cropped_example.gtf.gz"), pc, False))
    assert A.reduce_unstranded(genes) == _bed(f"ce_ref_genes_{tag}.bed")
    assert A.reduce_unstranded(exons) == _bed(f"ce_ref_exons_{tag}.bed")


def test_ref_stranded_reduce_rules():
    rows = [("c", 10, 20, A.PLUS), ("c", 20, 25, A.PLUS), ("c", 5, 30, A.MINUS), ("c", 26, 27, A.PLUS),
            ("b", 0, 1, A.UNSTRANDED), ("c", 12, 3, A.PLUS)]
    # touching merges; strands never merge; the inverted row (12, 3) sorts by its start inside the first run
    assert A.stranded_reduce(rows) == [("b", 0, 1, 2), ("c", 10, 25, 0), ("c", 26, 27, 0), ("c", 5, 30, 1)]
    # an inverted row that opens a run ends it below its start: the next row starts a new run
    assert A.stranded_reduce([("c", 52, 60, 0), ("c", 50, 40, 0)]) == [("c", 50, 40, 0), ("c", 52, 60, 0)]
    # ... and inside a run it changes nothing
    assert A.stranded_reduce([("c", 50, 40, 0), ("c", 45, 60, 0), ("c", 55, 56, 0)]) == [("c", 45, 60, 0)]


# --------------------------------------------------------------------------------------------- the C++ GTF reader
def _native_rows(path, pc=True, cv=True):
    from gtars_amd import models as M

    rows, strand, feature = M._read_gtf(path, pc, cv)
    names, ids, s, e = rows.chrom_names, rows.chrom_ids, rows.starts, rows.ends
    return [(names[int(ids[i])], int(s[i]), int(e[i]), int(strand[i]), int(feature[i])) for i in range(len(rows))]


def _gtf_lines(rng, n, bad_dropped=True):
    """rows of every kind the reader meets; bad numbers only on rows the filters drop"""
    feats = ["gene", "exon", "three_prime_utr", "five_prime_utr", "UTR", "CDS", "transcript", "start_codon", "Gene"]
    chrs = ["1", "chr1", "X", "chrX", "MT", "ch2", "chr10", "scaffold_7", "é9"]
    lines = []
    for _ in range(n):
        r = rng.random()
        if r < 0.04:
            lines.append("#" + "\t".join(["chr1", "x", "gene", "1", "2", ".", "+", ".", "junk"]))
            continue
        if r < 0.07:
            lines.append("\t".join(["chr1", "x", "gene", "1", "2", "."][: int(rng.integers(0, 6))]))
            continue
        ft = str(rng.choice(feats))
        key = str(rng.choice(["gene_biotype", "gene_type", "transcript_biotype"]))
        bio = str(rng.choice(["protein_coding", "lncRNA"]))
        attrs = f'gene_id "g{int(rng.integers(0, 99))}"; {key} "{bio}";'
        s = int(rng.integers(0, 2_000_000))
        e = s + int(rng.integers(-5, 5000))
        s_txt = str(s)
        if rng.random() < 0.05:
            s_txt = "+" + s_txt
        if rng.random() < 0.02:
            s_txt, e = "0", int(rng.integers(0, 9))
        if rng.random() < 0.01:
            s_txt = str(U32)
        e_txt = str(max(e, 0))
        dropped = ft not in A.FEATURES  # (dropped whatever the flags)
        if bad_dropped and dropped and rng.random() < 0.2:
            s_txt = str(rng.choice(["", "-5", " 7", "1e3", "99999999999", "+"]))
        strand = str(rng.choice(["+", "-", ".", "", "?x"]))
        extra = ["more\tcols"] if rng.random() < 0.1 else []
        lines.append("\t".join([str(rng.choice(chrs)), "src", ft, s_txt, e_txt, ".", strand, ".", attrs] + extra))
    return lines


def _write(tmp_path, name, lines, eol="\n", members=1, final_eol=True):
    text = eol.join(lines) + (eol if final_eol else "")
    data = text.encode("utf-8")
    p = tmp_path / name
    if name.endswith(".gz"):
        k = max(1, len(data) // members)
        p.write_bytes(b"".join(gzip.compress(data[i:i + k]) for i in range(0, len(data), k)))
    else:
        p.write_bytes(data)
    return str(p)


@pytest.mark.parametrize("seed", range(4))
def test_native_reader_matches_restatement(tmp_path, seed):
    rng = np.random.default_rng(100 + seed)
    lines = _gtf_lines(rng, 3000)
    for pc in (True, False):
        for cv in (True, False):
            for name, kw in (("a.gtf", {}), ("b.gtf", {"eol": "\r\n", "final_eol": False}), ("c.gtf.gz", {"members": 5})):
                p = _write(tmp_path, name, lines, **kw)
                want = A.read_gtf(p, pc, cv)
                assert _native_rows(p, pc, cv) == want, (name, pc, cv)


def test_native_reader_chunked_file(tmp_path):
    # > 1 MiB: cut into chunks at line starts and read by several host threads; chromosome ids in first-seen order
    rng = np.random.default_rng(7)
    lines = _gtf_lines(rng, 40000)
    p = _write(tmp_path, "big.gtf", lines)
    assert os.path.getsize(p) > 2 << 20
    got = _native_rows(p, False, True)
    assert got == A.read_gtf(p, False, True)
    from gtars_amd import models as M

    rows = M._read_gtf(p, False, True)[0]
    seen = []
    for c in (r[0] for r in got):
        if c not in seen:
            seen.append(c)
    assert rows.chrom_names == seen


def test_native_reader_fixtures():
    for name in ("test_gene_model.gtf", "test_gene_model_ensembl.gtf", "C_elegans_cropped_example.gtf.gz"):
        for pc in (True, False):
            for cv in (True, False):
                assert _native_rows(_gold(name), pc, cv) == A.read_gtf(_gold(name), pc, cv), (name, pc, cv)


def test_native_reader_details(tmp_path):
    row = 'X\ts\tgene\t{s}\t{e}\t.\t{st}\t.\tgene_type "protein_coding";'
    p = _write(tmp_path, "d.gtf", [row.format(s="+5", e="9", st="-"), row.format(s="0", e="0", st="+"),
                                   row.format(s="1", e="2", st=""), "chrY\ts\texon\t3\t4\t.\t+\t.\tgene_biotype \"protein_coding\"",
                                   "MT\ts\tCDS\t7\t8\t.\t+x\t.\tx; gene_biotype \"protein_coding\";\tmore"])
    assert _native_rows(p) == [("chrX", 4, 9, 1, 0), ("chrX", 0, 0, 0, 0), ("chrX", 0, 2, 2, 0), ("chrY", 2, 4, 0, 1),
                               ("chrMT", 6, 8, 0, 5)]
    # the biotype must sit in the 9th field itself, not in a later one
    q = _write(tmp_path, "e.gtf", ['1\ts\tgene\t1\t2\t.\t+\t.\tx;\tgene_biotype "protein_coding";'])
    assert _native_rows(q) == []
    assert _native_rows(q, pc=False) == [("chr1", 0, 2, 0, 0)]


@pytest.mark.parametrize("field, text, msg", [
    (3, "-5", "Parsing GTF start: invalid digit found in string"),
    (3, "", "Parsing GTF start: cannot parse integer from empty string"),
    (3, "4294967296", "Parsing GTF start: number too large to fit in target type"),
    (3, " 5", "Parsing GTF start: invalid digit found in string"),
    (4, "1e3", "Parsing GTF end: invalid digit found in string"),
    (4, "+", "Parsing GTF end: invalid digit found in string"),
])
def test_native_reader_bad_number_on_a_kept_row(tmp_path, field, text, msg):
    from gtars.models import GeneModel

    f = ["chr1", "s", "exon", "10", "20", ".", "+", ".", 'gene_biotype "protein_coding";']
    f[field] = text
    ok = "\t".join(["chr1", "s", "exon", "1", "2", ".", "+", ".", 'gene_biotype "protein_coding";'])
    dropped = "\t".join(["chr1", "s", "transcript", "x", "y", ".", "+", ".", 'gene_biotype "protein_coding";'])
    p = _write(tmp_path, "bad.gtf", [ok, dropped, "\t".join(f)])
    with pytest.raises(ValueError) as ei:
        _native_rows(p)
    assert str(ei.value) == msg
    with pytest.raises(ValueError, match="Parsing GTF"):
        A.read_gtf(p)
    with pytest.raises(ValueError, match="Parsing GTF"):
        GeneModel.from_gtf(p)  # before any device work: a ValueError on a box without a GPU too


def test_native_reader_bad_numbers_on_dropped_rows_are_never_seen(tmp_path):
    lines = ["chr1\ts\ttranscript\tx\ty\t.\t+\t.\tgene_biotype \"protein_coding\";",
             "chr1\ts\tgene\tx\ty\t.\t+\t.\tgene_biotype \"lncRNA\";",
             "chr1\ts\tgene\t5\t9\t.\t+\t.\tgene_biotype \"protein_coding\";"]
    p = _write(tmp_path, "drop.gtf", lines)
    assert _native_rows(p) == [("chr1", 4, 9, 0, 0)]
    with pytest.raises(ValueError):
        _native_rows(p, pc=False)  # the lncRNA gene is kept now, and its start is read


def test_native_reader_non_utf8(tmp_path):
    good = b"chr1\ts\tgene\t5\t9\t.\t+\t.\tgene_biotype \"protein_coding\";\n"
    for bad in (b"# comment \xff\n", b"chr1\ts\tgene\t5\t9\t.\t+\t.\tx \xc0\xaf\n", b"\xed\xa0\x80\n"):
        p = tmp_path / "u.gtf"
        p.write_bytes(good + bad + good)
        with pytest.raises(ValueError, match="UTF-8"):
            _native_rows(str(p))
        with pytest.raises(ValueError, match="UTF-8"):
            A.read_gtf(str(p))
    p.write_bytes(good + "é\n".encode() + good)
    assert len(_native_rows(str(p))) == 2


def test_native_reader_first_error_in_file_order(tmp_path):
    rng = np.random.default_rng(3)
    lines = _gtf_lines(rng, 30000, bad_dropped=False)
    k = len(lines) * 3 // 4
    lines[k] = "chr1\ts\tgene\t+\t9\t.\t+\t.\tgene_biotype \"protein_coding\";"
    data = ("\n".join(lines) + "\n").encode()
    cut = data.rfind(b"\n", 0, len(data) - 1000)
    p = tmp_path / "late.gtf"
    p.write_bytes(data[:cut + 1] + b"\xff\n" + data[cut + 1:])  # a UTF-8 error AFTER the parse error
    with pytest.raises(ValueError, match="Parsing GTF start"):
        _native_rows(str(p), pc=False)


def test_native_reader_missing_file_and_bad_gzip(tmp_path):
    from gtars.models import GeneModel, GenomicDistAnnotation

    with pytest.raises(ValueError):
        GeneModel.from_gtf(str(tmp_path / "nope.gtf"))
    with pytest.raises(ValueError):
        GenomicDistAnnotation.from_gtf(str(tmp_path / "nope.gtf.gz"))
    p = tmp_path / "plain.gtf.gz"
    p.write_bytes(b"chr1\ts\tgene\t5\t9\t.\t+\t.\tgene_biotype \"protein_coding\";\n")
    with pytest.raises(ValueError):
        _native_rows(str(p))


# ------------------------------------------------------------------------------------------------ host-side handles
def test_tss_index_from_path_errors():
    from gtars.models import TssIndex

    for bad in ("/nonexistent/file.bed", os.path.join(GOLD, "no_such.bed.gz")):
        with pytest.raises(ValueError) as ei:
            TssIndex(bad)
        assert str(ei.value) == "No TSS's found for region. Double-check your index!"


def test_tss_index_len_and_repr_without_device():
    from gtars.models import TssIndex

    t = TssIndex(_gold("dummy_tss.bed"))
    assert len(t) == 8
    assert repr(t) == str(t) == "RegionSet with 8 regions."
    u = TssIndex.from_regionset(_rs([("chr1", 100, 101), ("chr1", 500, 501), ("chr2", 5, 1)]))
    assert len(u) == 3 and repr(u) == "RegionSet with 3 regions."
    assert len(TssIndex.from_regionset(_rs([]))) == 0


def test_constructors_are_not_public():
    from gtars.models import GeneModel, GenomicDistAnnotation

    with pytest.raises(TypeError):
        GeneModel()
    with pytest.raises(TypeError):
        GenomicDistAnnotation()


@pytest.mark.skipif(not _no_gpu(), reason="needs a box WITHOUT a GPU")
def test_device_calls_refuse_without_a_gpu():
    import gtars_amd
    from gtars.models import GeneModel, GenomicDistAnnotation, TssIndex

    t = TssIndex(_gold("dummy_tss.bed"))
    q = _rs([("chr1", 10, 20)])
    with pytest.raises(gtars_amd.NoDeviceError):
        t.calc_tss_distances(q)
    with pytest.raises(gtars_amd.NoDeviceError):
        t.feature_distances(q)
    assert len(t) == 8
    with pytest.raises(gtars_amd.NoDeviceError):
        GeneModel.from_gtf(_gold("test_gene_model.gtf"))
    with pytest.raises(gtars_amd.NoDeviceError):
        GenomicDistAnnotation.from_gtf(_gold("test_gene_model.gtf"))
