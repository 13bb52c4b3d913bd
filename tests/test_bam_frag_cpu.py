"""K26 without a device: the restatement (tests/bam_frag_ref.py) on the worked example of DESIGN.md section 3 K26, the aux
walker on every type and every malformed form, the library's host text writer, parameter validation, the ABI, and the rule
of csrc/bam_frag_core.h under the sanitizers (tests/soak/bam_frag_host_check.cpp)."""
import gzip
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bam_frag_ref as F  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "bam")
EXAMPLE_REFS = [("chr1", 1000), ("chr2", 500)]
EXAMPLE_TEXT = (b"chr1\t104\t245\tAAC-1\t1\n" b"chr1\t104\t295\tAAA-1\t1\n" b"chr1\t104\t295\tAAC-1\t2\n" b"chr1\t994\t1000\tAAC-1\t1\n"
                b"chr2\t34\t125\tAAC-1\t1\n")
EXAMPLE_STATS = dict(records=12, kept_pairs=6, fragments=5, barcodes=2, mapq=1, not_leftmost=1, empty=1, too_long=1, no_barcode=1, unplaced=1,
                     flag=0, mate_ref=0)


def example_records():
    """the twelve records of the worked example, from its literals"""
    def r(ref, pos, tlen, flag=99, cb=b"AAC-1", mapq=60):
        return F.rec(ref_id=ref, pos=pos, tlen=tlen, flag=flag, mapq=mapq, next_ref_id=ref, next_pos=pos, aux=F.aux_Z("CB", cb) if cb else b"")

    return [r(0, 100, 200), r(0, 100, 200), r(0, 100, 200, cb=b"AAA-1"), r(0, 100, 150), r(0, 120, 200, cb=None, mapq=10),
            r(0, 291, -200, flag=147), r(0, 990, 50), r(1, 0, 8), r(1, 10, 3000), r(1, 20, 100, cb=None), r(1, 30, 100, flag=99 | 0x400),
            F.rec(ref_id=-1, pos=-1, tlen=0, flag=0x4, next_ref_id=-1)]


def test_the_worked_example():
    rows, barcodes, stats, text = F.fragments_ref(EXAMPLE_REFS, example_records())
    assert text == EXAMPLE_TEXT
    assert stats == EXAMPLE_STATS
    assert barcodes == [b"AAA-1", b"AAC-1"]
    assert rows == [(0, 104, 245, 1, 1), (0, 104, 295, 0, 1), (0, 104, 295, 1, 2), (0, 994, 1000, 1, 1), (1, 34, 125, 1, 1)]
    assert stats["records"] == sum(stats[k] for k in F.REASONS) + stats["kept_pairs"] and sum(r[4] for r in rows) == stats["kept_pairs"]


def test_the_example_survives_the_writer_and_the_reader():
    stream = F.bam_stream(EXAMPLE_REFS, example_records())
    refs, recs = F.parse_stream(stream)
    assert refs == EXAMPLE_REFS and [r["aux"] for r in recs] == [r["aux"] for r in example_records()]
    assert F.fragments_ref(refs, recs)[3] == EXAMPLE_TEXT


def test_no_barcode_tag_gives_the_sample():
    rows, barcodes, stats, text = F.fragments_ref(EXAMPLE_REFS, example_records(), barcode_tag=None, sample="s1")
    assert barcodes == [b"s1"] and stats["no_barcode"] == 0 and stats["kept_pairs"] == 7
    assert text.split(b"\n")[1] == b"chr1\t104\t295\ts1\t3"


EVERY_TYPE = [F.aux_A("XA", "q"), F.aux_int("Xc", "c", -3), F.aux_int("XC", "C", 200), F.aux_int("Xs", "s", -300), F.aux_int("XS", "S", 60000),
              F.aux_int("Xi", "i", -70000), F.aux_int("XI", "I", 4000000000), F.aux_f("Xf", 1.5), F.aux_Z("XZ", "CB in a text"),
              F.aux_H("XH", "1AE301"), F.aux_B("Bc", "c", [-1, 2]), F.aux_B("BC", "C", []), F.aux_B("Bs", "s", [-5]), F.aux_B("BS", "S", [1, 2, 3]),
              F.aux_B("Bi", "i", [7]), F.aux_B("BI", "I", [1, 2]), F.aux_B("Bf", "f", [0.5, 2.0])]


def test_the_aux_walker_on_every_type():
    aux = b"".join(EVERY_TYPE)
    entries = F.aux_entries(aux)
    assert [t for t, _, _ in entries] == [e[:2] for e in EVERY_TYPE]
    assert [(ty, len(v)) for _, ty, v in entries] == [("A", 1), ("c", 1), ("C", 1), ("s", 2), ("S", 2), ("i", 4), ("I", 4), ("f", 4), ("Z", 13),
                                                       ("H", 7), ("B", 7), ("B", 5), ("B", 7), ("B", 11), ("B", 9), ("B", 13), ("B", 13)]
    assert F.find_barcode(aux + F.aux_Z("CB", "T-1"), b"CB") == b"T-1"
    assert F.find_barcode(F.aux_Z("CB", "T-1") + aux, b"CB") == b"T-1"
    assert F.find_barcode(aux, b"CB") is None and F.find_barcode(b"", b"CB") is None
    assert F.find_barcode(F.aux_Z("CB", "one") + F.aux_Z("CB", "two"), b"CB") == b"one"
    assert F.find_barcode(F.aux_Z("CB", "") + F.aux_Z("CB", "two"), b"CB") is None
    assert F.find_barcode(F.aux_A("CB", "x") + F.aux_Z("CB", "two"), b"CB") is None
    assert F.find_barcode(F.aux_Z("CR", "raw") + F.aux_Z("CB", "cell"), b"CR") == b"raw"
    assert F.find_barcode(F.aux_Z("CB", "A") + b"XQ?", b"CB") == b"A"  # nothing behind the entry that decides is looked at


@pytest.mark.parametrize("aux", [b"XQ?abc", b"CBZno-nul", b"XHH12", b"XiiAB", b"CB", b"X", b"XBBi\xff\xff\xff\xff" + b"x" * 8,
                                 b"XBBI\x03\0\0\0" + b"x" * 11, b"XBBZ\0\0\0\0", b"XBBA\0\0\0\0", b"XBBc\0\0", None],
                         ids=["type", "z-nul", "h-nul", "value-cut", "header-cut", "one-byte", "b-count", "b-cut", "b-subtype", "b-subtype-A",
                              "b-header-cut", "aux-start"])
def test_the_aux_walker_refuses_every_malformed_form(aux):
    with pytest.raises(F.Malformed):
        F.find_barcode(aux, b"CB")
    if aux is not None:
        with pytest.raises(F.Malformed):
            F.aux_entries(aux)
        rec = F.rec(tlen=100, flag=99, next_ref_id=0, aux=aux)
        with pytest.raises(F.Malformed):
            F.fragments_ref(EXAMPLE_REFS, [rec])
        assert F.fragments_ref(EXAMPLE_REFS, [dict(rec, mapq=3)])[2]["mapq"] == 1  # an earlier step decides: the aux area is not walked
        assert F.fragments_ref(EXAMPLE_REFS, [rec], barcode_tag=None)[2]["kept_pairs"] == 1


def test_a_reader_sees_an_aux_start_beyond_block_size_as_none():
    stream = bytearray(F.bam_stream(EXAMPLE_REFS, [F.rec(tlen=100, flag=99, next_ref_id=0, aux=F.aux_Z("CB", "A"))]))
    at = len(F.R.encode_header(EXAMPLE_REFS))
    struct.pack_into("<I", stream, at + 4 + 16, 0x7FFFFFFF)
    _, recs = F.parse_stream(bytes(stream))
    assert recs[0]["aux"] is None
    with pytest.raises(F.Malformed):
        F.fragments_ref(EXAMPLE_REFS, recs)


# ---- the library's host side ------------------------------------------------------------------------------------------
def _frags(rows, barcodes, refs):
    from gtars_amd.bam import BamFragments

    cols = [np.asarray([r[k] for r in rows], dtype=np.int32 if k == 0 else np.uint32) for k in range(5)]
    return BamFragments(*cols, [b.decode() for b in barcodes], refs, {})


def test_the_host_text_writer_equals_pythons_formatting(tmp_path):
    rows, barcodes, _, text = F.fragments_ref(EXAMPLE_REFS, example_records())
    fr = _frags(rows, barcodes, EXAMPLE_REFS)
    assert len(fr) == 5
    fr.write(tmp_path / "sub" / "f.tsv")
    assert (tmp_path / "sub" / "f.tsv").read_bytes() == text == EXAMPLE_TEXT
    fr.write(str(tmp_path / "f.tsv.gz"))
    packed = (tmp_path / "f.tsv.gz").read_bytes()
    assert packed[:2] == b"\x1f\x8b" and gzip.decompress(packed) == text
    # every digit count of the three numbers, long and one-byte names, more rows than one piece of the writer
    rng = np.random.default_rng(5)
    refs = [("c", 1), ("chrUn_KI270442v1_with_a_long_name", 2)]
    bcs = [b"A", b"ACGTACGTACGTACGT-1", b"x" * 200]
    n = 70_001
    digits = rng.integers(1, 11, size=(n, 3))
    vals = np.minimum((10.0 ** digits * rng.random((n, 3))).astype(np.uint64), 0xFFFFFFFF)
    vals[:4] = [[0, 0, 0], [0xFFFFFFFF] * 3, [9, 10, 99], [1000000000, 999999999, 100]]
    big = [(int(rng.integers(0, 2)), int(s), int(e), int(rng.integers(0, 3)), int(c)) for s, e, c in vals]
    _frags(big, bcs, refs).write(tmp_path / "big.tsv")
    want = b"".join(b"%s\t%d\t%d\t%s\t%d\n" % (refs[r][0].encode(), s, e, bcs[b], c) for r, s, e, b, c in big)
    assert (tmp_path / "big.tsv").read_bytes() == want
    _frags([], [], EXAMPLE_REFS).write(tmp_path / "none.tsv")
    assert (tmp_path / "none.tsv").read_bytes() == b""
    _frags([], [], EXAMPLE_REFS).write(tmp_path / "none.tsv.gz")
    assert gzip.decompress((tmp_path / "none.tsv.gz").read_bytes()) == b""
    for bad in ([(2, 1, 2, 0, 1)], [(-1, 1, 2, 0, 1)], [(0, 1, 2, 2, 1)]):
        with pytest.raises(ValueError, match="names no reference or no barcode"):
            _frags(bad, barcodes, EXAMPLE_REFS).write(tmp_path / "bad.tsv")


@pytest.mark.parametrize("kw,match", [(dict(barcode_tag="C"), "two bytes"), (dict(barcode_tag="CBX"), "two bytes"), (dict(barcode_tag=""), "two bytes"),
                                      (dict(barcode_tag=None, sample=""), "sample"), (dict(barcode_tag=None, sample="a b"), "sample"),
                                      (dict(barcode_tag=None, sample="a\tb"), "sample"), (dict(min_mapq=-1), "min_mapq"),
                                      (dict(max_fragment_length=0), "max_fragment_length"), (dict(shift=(1, 2, 3)), "shift")])
def test_bad_parameters_raise_before_any_device_work(tmp_path, kw, match):
    from gtars_amd import bam

    path = os.path.join(GOLDEN, "dummy.bam")
    with bam.BamFile(path) as b:
        with pytest.raises(ValueError, match=match):
            b.fragments(**kw)
    with pytest.raises(ValueError, match=match):
        bam.bam_to_fragments(path, str(tmp_path / "o.tsv"), **kw)
    assert not (tmp_path / "o.tsv").exists()
    with pytest.raises(TypeError):
        bam.bam_to_fragments(path, str(tmp_path / "o.tsv"), barcode="CB")


def test_the_c_entry_point_validates_as_well():
    import ctypes as C

    from gtars_amd import bam
    from gtars_amd._lib import last_error, lib

    with bam.BamFile(os.path.join(GOLDEN, "dummy.bam")) as b:
        for change, match in ((dict(min_mapq=-1), "min_mapq"), (dict(max_fragment_length=0), "max_fragment_length"),
                              (dict(use_barcode_tag=0, sample=b"a b"), "sample"), (dict(use_barcode_tag=0, sample=None), "sample"),
                              (dict(barcode_tag=b"C"), "two bytes")):
            p = bam._FragParams()
            lib.gtars_bam_frag_params_default(C.byref(p))
            assert (p.barcode_tag, p.use_barcode_tag, p.sample, p.min_mapq, p.max_fragment_length, p.shift_left, p.shift_right, p.require_flags,
                    p.exclude_flags) == (b"CB", 1, b"bulk", 30, 2000, 4, -5, 0x3, 0xB0C)
            for k, v in change.items():
                setattr(p, k, v)
            h = C.c_void_p()
            assert lib.gtars_bam_fragments(b._h, C.byref(p), 0, 0, C.byref(h)) != 0 and not h.value
            assert match in last_error()


def test_abi():
    import gtars_amd._lib as L

    new = ("gtars_bam_frag_params_default", "gtars_bam_fragments", "gtars_bam_frags_len", "gtars_bam_frags_ref", "gtars_bam_frags_start",
           "gtars_bam_frags_end", "gtars_bam_frags_barcode", "gtars_bam_frags_count", "gtars_bam_frags_n_barcodes", "gtars_bam_frags_barcode_name",
           "gtars_bam_frags_stats", "gtars_bam_frags_write", "gtars_bam_frags_free", "gtars_fragments_write_text")
    out = subprocess.check_output(["nm", "-D", "--defined-only", L.LIB_PATH], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in new:
        assert name in L.EXPORTED_HOST_SYMBOLS and name in exported, name
    for header in ("gtars_amd.h", "gtars_amd_host.h"):
        assert "gtars_debug_" not in open(os.path.join(HERE, "..", "include", header)).read()
    from gtars_amd import bam

    assert callable(bam.BamFile.fragments) and callable(bam.bam_to_fragments) and callable(bam.BamFragments.write)
    assert len(bam.FRAG_STATS) == 12 and bam.FRAG_STATS == F.STATS


def test_every_kernel_of_k26_has_a_multi_trip_test():
    """csrc/bam_frag.hip launches through launch_over (csrc/pipeline.h) alone, so GTARS_GRID_CAP clips every one of its grids;
    tests/test_gpu_bam_frag.py's K26_KERNELS names each kernel of the file and what makes
    test_grid_stride_loops_take_more_than_one_turn run it past the first trip of its loop (the table is read from the module's
    text, as tests/test_grid_cap_inventory_cpu.py reads its own)."""
    import ast
    import re

    csrc = os.path.join(HERE, "..", "gtars_amd", "csrc")
    text = open(os.path.join(csrc, "bam_frag.hip")).read()
    kernels = set(re.findall(r"__global__\b[^;{}]*?\b(k_\w+)\s*\(", text))
    assert len(kernels) == text.count("__global__") >= 10
    assert "hipLaunchKernelGGL" not in text and "<<<" not in text  # no launch of its own: every grid is launch_over's
    launched = set(re.findall(r"launch_over\(st, \w+, (k_\w+),", text))
    assert launched == kernels
    assert "GTARS_GRID_CAP" in open(os.path.join(csrc, "common.h")).read() and "grid_for(n)" in open(os.path.join(csrc, "pipeline.h")).read()
    tree = ast.parse(open(os.path.join(HERE, "test_gpu_bam_frag.py")).read())
    table = [ast.literal_eval(n.value) for n in tree.body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "K26_KERNELS"]
    assert table and set(table[0]) == kernels and all(v.strip() for v in table[0].values())
    assert "test_grid_stride_loops_take_more_than_one_turn" in {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}


def test_the_rule_under_the_sanitizers(tmp_path):
    """tests/soak/bam_frag_host_check.cpp, built with AddressSanitizer + UBSan: csrc/bam_frag_core.h -- the function the kernel
    calls -- on the worked example, on every aux layout and on malformed aux data in heap blocks of exactly the record's size"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "bam_frag_host_check"
    src = os.path.join(HERE, "soak", "bam_frag_host_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o",
                            str(exe), src], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("the host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "ok" in run.stdout
