"""K18 on the host: the plain-Python restatement (tests/vrs_ref.py) and the library's host calls (gtars_amd/vrs.py over
csrc/vrs.cpp, csrc/vrs_core.h, csrc/sha512.h) must each equal values pinned from outside -- the GA4GH VRS 2.0 vectors and
the normalization known answers the reference's own tests carry -- and each other on the VCF rules, the refget digests and
the library's host path of the batch calls.  No device is needed."""
import base64
import gzip
import hashlib
import os
import random
import shutil
import subprocess

import pytest

import bam_ref
import vrs_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))

SHA_VECTORS = [(b"", "z4PhNX7vuL3xVChQ1m2AB9Yg5AULVxXc"), (b"ACGT", "aKF498dAxcJAqme6QYQ7EZ07-fiw8Kw2")]
# (accession, start, end, SequenceLocation digest)
LOCATIONS = [
    ("SQ.IIB53T8CNeJJdUqzn9V_JnRtQadwWCbl", 44908821, 44908822, "wIlaGykfwHIpPY2Fcxtbx4TINbbODFVz"),
    ("SQ.F-LrLMe1SRpfUZHkQmvkVKFEGaoDeHul", 44908821, 44908822, "4t6JnYWqHwYw9WzBT_lmWBb3tLQNalkT"),
    ("SQ.F-LrLMe1SRpfUZHkQmvkVKFEGaoDeHul", 55181319, 55181320, "_G2K0qSioM74l_u3OaKR0mgLYdeTL7Xd"),
]
# (accession, start, end, literal sequence, Allele identifier)
ALLELES = [
    ("SQ.IIB53T8CNeJJdUqzn9V_JnRtQadwWCbl", 44908821, 44908822, "T", "ga4gh:VA.0AePZIWZUNsUlQTamyLrjm2HWUw2opLt"),
    ("SQ.F-LrLMe1SRpfUZHkQmvkVKFEGaoDeHul", 55181319, 55181320, "T", "ga4gh:VA.Hy2XU_-rp4IMh6I_1NXNecBo8Qx8n0oE"),
    ("SQ.KEO-4XBcm1cxeo_DIQ8_ofqGUkp4iZhI", 128325834, 128325835, "T", "ga4gh:VA.SZIS2ua7AL-0YgUTAqyBsFPYK3vE8h_d"),
]
# (sequence, start, ref, alt) -> (start, end, allele): the known answers of the reference's normalization tests
NORMALIZED = [
    (("ACGTACGT", 2, "G", "T"), (2, 3, "T")),
    (("TAAAAG", 1, "A", "AA"), (1, 5, "AAAAA")),
    (("TAAAAG", 1, "AA", "A"), (1, 5, "AAA")),
    (("ACGTACGT", 2, "GT", "GT"), (4, 4, "")),
    (("ACGTACGT", 2, "g", "t"), (2, 3, "t")),
]
# ... and the failures, with the status and NormalizeError's text
REFUSED = [
    (("ACGT", 10, "G", "T"), R.REF_PAST_END, "ref allele (start=10, len=1) extends past sequence length 4"),
    (("ACGTACGT", 2, "A", "T"), R.REF_MISMATCH, "ref allele mismatch at interbase 2: VCF says A, reference has G"),
    (("ACGTACGT", 2, "GG", "G"), R.REF_MISMATCH, "ref allele mismatch at interbase 2: VCF says GG, reference has GT"),
    (("ACGT", (1 << 64) - 1, "G", "T"), R.START_OUT_OF_BOUNDS, "start position 18446744073709551615 exceeds sequence length 4"),
]


def test_restatement_equals_the_pinned_values():
    for data, want in SHA_VECTORS:
        assert R.sha512t24u(data) == want
    for acc, s, e, want in LOCATIONS:
        assert R.location_digest(acc, s, e) == want
    for acc, s, e, seq, want in ALLELES:
        assert R.vrs_id(acc, s, e, seq) == want
    for (seq, s, ref, alt), (ns, ne, allele) in NORMALIZED:
        assert R.normalize(seq.encode(), s, ref.encode(), alt.encode()) == (ns, ne, allele.encode())
    ns, ne, _ = R.normalize(b"ACGTACGT", 2, b"", b"AA")  # an empty REF has nothing to validate
    assert ns == ne
    for (seq, s, ref, alt), status, text in REFUSED:
        with pytest.raises(R.NormalizeError) as err:
            R.normalize(seq.encode(), s, ref.encode(), alt.encode())
        assert err.value.status == status and str(err.value) == text


def test_library_scalar_calls_equal_the_pinned_values():
    import gtars.vrs
    from gtars_amd import vrs as V

    assert gtars.vrs is V
    for data, want in SHA_VECTORS:
        assert V.sha512t24u(data) == want and V.sha512t24u(data.decode()) == want
    for acc, s, e, want in LOCATIONS:
        assert V.location_digest(acc, s, e) == want
    for acc, s, e, seq, want in ALLELES:
        assert V.vrs_id(acc, s, e, seq) == want and V.vrs_digest(acc, s, e, seq) == want[len("ga4gh:VA."):]
    for args, (ns, ne, allele) in NORMALIZED:
        assert V.normalize_allele(*args) == {"start": ns, "end": ne, "allele": allele}
    got = V.normalize_allele("ACGTACGT", 2, "", "AA")
    assert got["start"] == got["end"]
    for args, _, text in REFUSED:
        with pytest.raises(ValueError) as err:
            V.normalize_allele(*args)
        assert str(err.value) == text


def test_sha512_at_every_padding_length():
    from gtars_amd import vrs as V

    rng = random.Random(3)
    for n in list(range(0, 300)) + [1000, 4096, 4097]:
        data = bytes(rng.randrange(256) for _ in range(n))
        assert V.sha512t24u(data) == R.sha512t24u(data), n


def test_scalar_calls_against_the_restatement_on_random_alleles():
    from gtars_amd import vrs as V

    rng = random.Random(11)
    done = 0
    for _ in range(3000):
        letters = "ACGTacgtN"[:rng.choice((1, 2, 4, 9))]
        seq = "".join(rng.choice(letters) for _ in range(rng.randint(1, 30)))
        start = rng.randint(0, len(seq) + 1)
        ref = seq[start:start + rng.randint(0, 3)]
        if rng.random() < 0.3:
            ref = ref.upper() if rng.random() < 0.5 else ref + "T"
        alt = "".join(rng.choice("ACGTa") for _ in range(rng.randint(0, 4)))
        try:
            ns, ne, allele = R.normalize(seq.encode(), start, ref.encode(), alt.encode())
        except R.NormalizeError as err:
            with pytest.raises(ValueError) as got:
                V.normalize_allele(seq, start, ref, alt)
            assert str(got.value) == str(err)
            continue
        assert V.normalize_allele(seq, start, ref, alt) == {"start": ns, "end": ne, "allele": allele.decode()}
        assert V.vrs_id("SQ.abc", ns, ne, allele.decode()) == R.vrs_id("SQ.abc", ns, ne, allele)
        done += 1
    assert done > 1000


# ---- a small assembly and a hand-written VCF -------------------------------------------------------------------------
SEQS = {
    "chr1": b"ACGTACGTTAAAAGCCGGTTacgtnnNNACACACACGT" + b"GATTACA" * 5,
    "chr2": b"TTTTTTTTGGGCATCATCATCAGN",
    "chrM": b"a",
}
VCF_LINES = [
    b"##fileformat=VCFv4.2",
    b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO",
    b"chr1\t3\trs1\tG\tT\t50\tPASS\tAC=1",
    b"",
    b"chr1\t10\t.\tA\tAA,<DEL>,*,.,,T\t.\t.\tX=a\tb,c",
    b"chr1\t11\t.\tAA\tA\r",
    b"chr1\t5\t.\tA",
    b"chr1\t0\t.\tA\tC",
    b"chr1\tx\t.\tA\tC",
    b"chr1\t+4\t.\tt\tc",
    b"chrUn\t1\t.\tA\tC",
    b"chr2\t9\t.\tG\tGG,GT",
    b"chr2\t13\t.\tATC\tA\t.",
    b"chrM\t1\t.\tA\tG",
    b"chr1\t30\t.\tCA\tC\t.\t.\t.",
]
VCF_TEXT = b"\n".join(VCF_LINES[:5]) + b"\r\n" + b"\n".join(VCF_LINES[5:])  # (one \r\n ending, one bare \r at a line's end, no final newline)
EXPECTED_ROWS = [("chr1", 2, "G", "T"), ("chr1", 9, "A", "AA"), ("chr1", 9, "A", "T"), ("chr1", 10, "AA", "A"), ("chr1", 3, "t", "c"),
                 ("chr2", 8, "G", "GG"), ("chr2", 8, "G", "GT"), ("chr2", 12, "ATC", "A"), ("chrM", 0, "A", "G"), ("chr1", 29, "CA", "C")]


def vcf_variants():
    """the text as plain, gzip and BGZF bytes, each under a name whose extension says nothing"""
    return {"plain.vcf": VCF_TEXT, "gzip.vcf.txt": gzip.compress(VCF_TEXT), "bgzf.vcf": bam_ref.bgzf_bytes(VCF_TEXT, block=97)}


def write_fasta(path, seqs, width=11):
    with open(path, "wb") as f:
        for name, s in seqs.items():
            f.write(b">" + name.encode() + b" test\n")
            for k in range(0, len(s), width):
                f.write(s[k:k + width] + b"\n")


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    from gtars_amd.seqstats import GenomeAssembly

    d = tmp_path_factory.mktemp("vrs_cpu")
    write_fasta(d / "asm.fa", SEQS)
    return GenomeAssembly(str(d / "asm.fa"))


def test_restatement_parses_the_vcf_rules():
    rows = R.parse_vcf(R.open_vcf_bytes(VCF_TEXT), set(SEQS))
    assert [(c, p, r.decode(), a.decode()) for c, p, r, a in rows] == EXPECTED_ROWS
    for data in vcf_variants().values():
        assert R.open_vcf_bytes(data) == VCF_TEXT


def test_library_parses_the_vcf_rules(genome, tmp_path):
    from gtars_amd import vrs as V

    for name, data in vcf_variants().items():
        p = tmp_path / name
        p.write_bytes(data)
        for threads in (1, 3):
            got = V.read_vcf_alleles(str(p), genome, threads=threads)
            assert list(zip(got.chrom, got.pos, got.ref_allele, got.alt_allele)) == EXPECTED_ROWS, (name, threads)
            assert got.vrs_id is None and len(got) == len(EXPECTED_ROWS)
    # a table of accessions that lacks a chromosome: its rows are skipped like those of an unknown name
    acc = {k: v for k, v in R.refget_digests(SEQS).items() if k != "chr2"}
    got = V.read_vcf_alleles(str(tmp_path / "plain.vcf"), genome, accessions=acc)
    assert list(zip(got.chrom, got.pos, got.ref_allele, got.alt_allele)) == [r for r in EXPECTED_ROWS if r[0] != "chr2"]
    with pytest.raises(FileNotFoundError):
        V.read_vcf_alleles(str(tmp_path / "missing.vcf"), genome)


def test_many_lines_parse_the_same_on_every_thread_count(genome, tmp_path):
    from gtars_amd import vrs as V

    rng = random.Random(8)
    lines = [b"#header"]
    for _ in range(20_000):
        c = rng.choice(["chr1", "chr2", "chrM", "chrNope"])
        alts = ",".join(rng.choice(["A", "C", "GT", "<INS>", "*", ".", "", "TTT"]) for _ in range(rng.randint(1, 4)))
        lines.append(f"{c}\t{rng.randint(0, 40)}\t.\t{rng.choice(['A', 'AC', 'g'])}\t{alts}\t.\tPASS\t{'x' * rng.randint(0, 200)}".encode())
    text = b"\n".join(lines) + b"\n"
    p = tmp_path / "many.vcf"
    p.write_bytes(gzip.compress(text))
    want = [(c, pos, r.decode(), a.decode()) for c, pos, r, a in R.parse_vcf(text, set(SEQS))]
    assert len(want) > 10_000
    for threads in (1, 2, 5):
        got = V.read_vcf_alleles(str(p), genome, threads=threads)
        assert list(zip(got.chrom, got.pos, got.ref_allele, got.alt_allele)) == want, threads


def test_refget_digests(genome):
    from gtars_amd.seqstats import BinaryGenomeAssembly, write_fab

    want = {name: base64.urlsafe_b64encode(hashlib.sha512(s.upper()).digest()[:24]).decode() for name, s in SEQS.items()}
    assert genome.refget_digests() == want == R.refget_digests(SEQS)
    assert genome.refget_digests(threads=1) == want  # (kept on the handle)
    assert BinaryGenomeAssembly.refget_digests is type(genome).refget_digests


def test_host_path_of_the_batch_calls(genome, tmp_path):
    """the library's own host path (on_host=True): the same columns as the device calls, no device"""
    from gtars_amd import vrs as V

    acc = R.refget_digests(SEQS)
    rows = [(c, p, r.encode(), a.encode()) for c, p, r, a in EXPECTED_ROWS]
    rows += [("chr1", 38, b"", b"GATTACA"), ("chr1", 28, b"AC", b""), ("chr2", 0, b"", b"T"), ("chr2", 24, b"", b"A"), ("chr1", 0, b"ACGT", b"ACGT"),
             ("chr1", 20, b"ACGT", b"ACGT"), ("chr1", 20, b"acgt", b"t"), ("chr1", 500, b"A", b"C"), ("chr2", 22, b"GNA", b"G"), ("chr2", 3, b"A", b"C"),
             ("chrNope", 3, b"A", b"C"), ("chr1", (1 << 64) - 1, b"AC", b"C"), ("chr1", 24, b"nn", b"n")]
    st, ns, ne, seqs, ids = R.alleles(SEQS, acc, rows)
    assert {R.OK, R.START_OUT_OF_BOUNDS, R.REF_PAST_END, R.REF_MISMATCH, R.UNKNOWN_CHROMOSOME} <= set(st)
    cols = [[r[k] for r in rows] for k in range(4)]
    for threads in (1, 4):
        got = V.normalize_alleles(genome, *cols, on_host=True, threads=threads)
        assert got["statuses"].tolist() == st and got["starts"].tolist() == ns and got["ends"].tolist() == ne
        assert got["sequences"] == seqs
        got = V.vrs_ids(genome, *cols, on_host=True, threads=threads)
        assert got["ids"] == ids and got["statuses"].tolist() == st
    # a caller's own table; a chromosome it lacks is status 4
    mine = {"chr1": "SQ." + "A" * 32, "chrM": "B" * 32}
    st2, _, _, _, ids2 = R.alleles(SEQS, {k: v[-32:] for k, v in mine.items()}, rows)
    got = V.vrs_ids(genome, *cols, accessions=mine, on_host=True)
    assert got["ids"] == ids2 and got["statuses"].tolist() == st2 and R.UNKNOWN_CHROMOSOME in st2
    with pytest.raises(ValueError, match="32 digest characters"):
        V.vrs_ids(genome, *cols, accessions={"chr1": "short"}, on_host=True)
    assert V.vrs_ids(genome, [], [], [], [], on_host=True)["ids"] == []
    # the file call on the host path: row for row, then the first failing row raises with the reference's text
    (tmp_path / "a.vcf").write_bytes(VCF_TEXT)
    res = V.compute_vrs_ids(str(tmp_path / "a.vcf"), genome, on_host=True)
    assert list(zip(res.chrom, res.pos, res.ref_allele, res.alt_allele, res.vrs_id)) == R.compute_vrs_ids(VCF_TEXT, SEQS, acc)
    assert res[0]["vrs_id"].startswith("ga4gh:VA.") and len(res) == len(EXPECTED_ROWS)
    bad = VCF_TEXT.replace(b"chr2\t13\t.\tATC\tA", b"chr2\t13\t.\tATG\tA")
    assert bad != VCF_TEXT
    (tmp_path / "bad.vcf").write_bytes(bad + b"\nchr1\t999\t.\tA\tC\n")
    with pytest.raises(ValueError) as err:
        V.compute_vrs_ids(str(tmp_path / "bad.vcf"), genome, on_host=True)
    assert str(err.value) == "Failed to normalize variant at chr2:13: ref allele mismatch at interbase 12: VCF says ATG, reference has ATC"
    with pytest.raises(ValueError) as want:
        R.compute_vrs_ids(bad, SEQS, acc)
    assert str(want.value) == str(err.value)


def test_sha512_and_line_parser_under_the_sanitizers(tmp_path):
    """tests/soak/vrs_host_check.cpp, built with AddressSanitizer + UBSan: csrc/sha512.h on messages of every length 0 .. 300
    against digests written here with hashlib, the VCF line parser on random lines, well-formed lines and all their
    truncations in exactly sized heap blocks, the normalizer on random short sequences."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    digests = tmp_path / "digests.txt"
    with open(digests, "w") as f:
        for n in range(301):
            f.write(f"{n} {R.sha512t24u(bytes((31 * n + 7 * k) & 0xFF for k in range(n)))}\n")
    exe = tmp_path / "vrs_host_check"
    src = os.path.join(HERE, "soak", "vrs_host_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o",
                            str(exe), src], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("the host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe), str(digests), "5"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "all checks passed: 301 digests" in run.stdout
