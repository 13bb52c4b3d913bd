"""csrc/byte_csr.h on the host: the group function the three byte-CSR fill kernels (vrs.hip, reftx.hip, hgvs.hip) run, under a
stand-alone ASan/UBSan program."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_fill_group_under_the_sanitizers(tmp_path):
    """tests/soak/byte_csr_check.cpp, built with AddressSanitizer + UBSan: csr_fill_group on offset tables of 0 .. 40 rows of
    0 .. 19 bytes (empty rows first, last, in runs, alone; totals of every residue mod 8) against a per-row loop, with the rows
    it opens and the guard bytes behind the total checked."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "byte_csr_check"
    src = os.path.join(HERE, "soak", "byte_csr_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o",
                            str(exe), src], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("the host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    assert "warning" not in build.stderr, build.stderr[-2000:]
    run = subprocess.run([str(exe), "20"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "ok" in run.stdout
