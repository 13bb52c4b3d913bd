"""K25 on the host: RegionSet.identifier / file_digest / to_bed / to_bed_gz / sort and RegionSetList.identifier (csrc/bed_text.cpp,
on_host=True and the single-set properties) against the reference's literals (gtars-core/src/models/region_set.rs:1552-1557,
1657-1663, region_set_list.rs:358-364) and the hashlib restatement (tests/bed_text_ref.py)."""
import glob
import gzip
import os
import random
import shutil
import subprocess

import pytest

import bed_text_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
PEAKS = os.path.join(HERE, "golden", "regionset", "dummy.narrowPeak")
BEDSET = sorted(glob.glob(os.path.join(HERE, "golden", "bedset", "*")))
IDENTIFIER = "f0b2cf73383b53bd97ff525a0380f200"
FILE_DIGEST = "6224c4d40832b3e0889250f061e01120"
BEDSET_IDENTIFIER = "17a10ce63638431b34e7d044c3eac186"


@pytest.fixture(scope="module")
def M():
    import gtars_amd.models as M

    return M


def make_set(M, rows):
    return M.RegionSet.from_regions([M.Region(*r) for r in rows])


def rows_of(rs):
    return [(r.chr, r.start, r.end, r.rest) for r in rs.regions]


def random_rows(rng, n):
    names = ["chr1", "chr10", "chr2", "chrX", "c", "chrUn_KI270742v1", "scaffold_" + "x" * 31]
    edges = [0, 9, 10, 99, 100, 999999999, 1000000000, 4294967295]
    rows = []
    for _ in range(n):
        s = rng.choice(edges) if rng.random() < 0.2 else rng.randrange(0, 250_000_000)
        e = rng.choice(edges) if rng.random() < 0.2 else s + rng.randrange(0, 5000)
        rest = None if rng.random() < 0.5 else "\t".join("f%d" % rng.randrange(1000) for _ in range(rng.randrange(1, 4)))
        rows.append((rng.choice(names), s, min(e, 4294967295), rest))
    return rows


def test_the_reference_literals(M):
    assert len(BEDSET) == 4
    for path in (PEAKS, PEAKS + ".bed.gz"):
        rows = R.load(path)
        assert (R.identifier(rows), R.file_digest(rows)) == (IDENTIFIER, FILE_DIGEST)
        rs = M.RegionSet(path)
        assert (rs.identifier, rs.file_digest) == (IDENTIFIER, FILE_DIGEST)
    sets = [R.load(p) for p in BEDSET]
    assert len({R.identifier(s) for s in sets}) == 1  # (the four files share one identifier)
    assert R.list_identifier(sets) == BEDSET_IDENTIFIER
    lst = M.RegionSetList([M.RegionSet(p) for p in BEDSET])
    assert lst.identifier(on_host=True) == BEDSET_IDENTIFIER
    assert lst.identifiers(on_host=True) == [R.identifier(s) for s in sets] == [s.identifier for s in lst]
    assert lst.file_digests(on_host=True) == [R.file_digest(s) for s in sets]
    assert lst.identifiers(on_host=True, threads=1) == lst.identifiers(on_host=True, threads=3)


def test_to_bed_round_trip(M, tmp_path):
    """the reference's test_save_bed: the written file reloads to the same identifier; to_bed_gz inflates to to_bed's bytes"""
    rs = M.RegionSet(PEAKS)
    out = tmp_path / "new" / "dir" / "out.bed"  # (parent directories are created)
    rs.to_bed(out)
    assert out.read_bytes() == R.bed_text(R.load(PEAKS)) == rs._bed_text(True)
    assert M.RegionSet(str(out)).identifier == IDENTIFIER
    out.write_bytes(b"stale contents that are longer than nothing\n" * 100)
    rs.to_bed(str(out))  # (an existing file is replaced)
    assert out.read_bytes() == R.bed_text(R.load(PEAKS))
    gz = tmp_path / "out.bed.gz"
    rs.to_bed_gz(gz)
    packed = gz.read_bytes()
    assert packed[:2] == b"\x1f\x8b" and gzip.decompress(packed) == out.read_bytes()
    assert M.RegionSet(str(gz)).identifier == IDENTIFIER


def test_sort(M, tmp_path):
    rng = random.Random(2501)
    rows = random_rows(rng, 400)
    rows += [("chr2", 77, 90, "first"), ("chr2", 77, 80, "second"), ("chr2", 77, 85, None), ("chr2", 77, 70, "fourth")]  # equal keys
    rng.shuffle(rows)
    rs = make_set(M, rows)
    assert rows_of(rs) == rows and rs.identifier == R.identifier(rows)  # (not sorted until asked)
    before = rs.identifier
    rs.sort()
    want = R.sort_rows(rows)
    assert rows_of(rs) == want
    assert [r[3] for r in want if r[0] == "chr2" and r[1] == 77] == [r[3] for r in rows if r[0] == "chr2" and r[1] == 77]  # stable
    assert rs.identifier == R.identifier(want) != before  # (the cached identifier went with the old order)
    # the order of the file loader
    path = tmp_path / "shuffled.bed"
    path.write_bytes(R.bed_text(rows))
    assert rows_of(M.RegionSet(str(path))) == want
    # strands move with their rows
    strands = [rng.choice("+-") for _ in rows]
    st = M.RegionSet.from_regions([M.Region(*r) for r in rows], strands)
    st.sort()
    order = sorted(range(len(rows)), key=lambda i: (rows[i][0].encode(), rows[i][1]))
    assert st.strands == [strands[i] for i in order] and rows_of(st) == want


def test_empty_set_and_rest_with_tabs(M):
    empty = M.RegionSet.from_regions([])
    assert empty.identifier == R.identifier([]) and empty.file_digest == R.file_digest([]) == "d41d8cd98f00b204e9800998ecf8427e"
    assert empty._bed_text(True) == b""
    empty.sort()
    rows = [("chr1", 5, 9, "a\tb\t\tc"), ("chr1", 1, 2, None), ("chrM", 0, 4294967295, "x"), ("chr1", 3, 4, "\t")]
    rs = make_set(M, rows)
    assert rs._bed_text(True) == R.bed_text(rows) == b"chr1\t5\t9\ta\tb\t\tc\nchr1\t1\t2\nchrM\t0\t4294967295\tx\nchr1\t3\t4\t\t\n"
    assert (rs.identifier, rs.file_digest) == (R.identifier(rows), R.file_digest(rows))
    one = make_set(M, rows[:1])
    assert (one.identifier, one.file_digest) == (R.identifier(rows[:1]), R.file_digest(rows[:1]))


def test_host_path_on_random_sets(M):
    rng = random.Random(2502)
    sets = [random_rows(rng, rng.randrange(0, 301)) for _ in range(200)]
    lst = M.RegionSetList([make_set(M, rows) for rows in sets])
    assert lst.identifiers(on_host=True) == [R.identifier(rows) for rows in sets]
    assert lst.file_digests(on_host=True) == [R.file_digest(rows) for rows in sets]
    assert lst.identifier(on_host=True) == R.list_identifier(sets)
    for k in (0, 17, 199):
        assert (lst[k].identifier, lst[k].file_digest) == (R.identifier(sets[k]), R.file_digest(sets[k]))
        assert lst[k]._bed_text(True) == R.bed_text(sets[k])


def test_host_code_under_the_sanitizers(tmp_path):
    """tests/soak/bed_text_host_check.cpp, built with AddressSanitizer + UBSan: the width, digit and byte functions of
    bed_text_core.h at every digit-count edge, md5_stream_pairs on every message length from 0 to 300 in exactly sized heap
    blocks, and the four streams of the golden file against the reference's literals."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "bed_text_host_check"
    src = os.path.join(HERE, "soak", "bed_text_host_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o",
                            str(exe), src], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("the host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    rows = R.load(PEAKS)
    edges = [0, 9, 10, 99, 100, 999999999, 1000000000, 4294967295]
    extra = [("c", a, b, "r" if (a + b) % 2 else None) for a in edges for b in edges]
    for name, want_rows in (("golden", rows), ("edges", extra), ("empty", [])):
        path = tmp_path / (name + ".tsv")
        path.write_bytes(R.bed_text(want_rows))
        run = subprocess.run([str(exe), str(path), R.identifier(want_rows), R.file_digest(want_rows)], capture_output=True, text=True)
        assert run.returncode == 0, (name, run.stdout[-1000:], run.stderr[-3000:])
        assert f"{len(want_rows)} rows, 0 failure(s)" in run.stdout
    assert (R.identifier(rows), R.file_digest(rows)) == (IDENTIFIER, FILE_DIGEST)
