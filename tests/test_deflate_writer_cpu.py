"""The DEFLATE streams of tests/deflate_writer.py (the named corpus, the 200 random streams and the libdeflate fixtures) held to
zlib's inflate on the CPU -- the proof that the expected bytes the GPU test (tests/test_gpu_inflate_streams.py) takes as given are
what the reference decodes, and that the streams declared invalid are invalid -- and the host decoder csrc/inflate_fast.h on the
same streams, as a stand-alone program under ASan + UBSan (tests/soak/inflate_corpus_check.cpp)."""
import os
import shutil
import subprocess
import zlib

import pytest

import deflate_writer as dw

HERE = os.path.dirname(os.path.abspath(__file__))


def _zlib_inflate(stream):
    z = zlib.decompressobj(-15)
    out = z.decompress(stream)
    return out, z.eof, z.unused_data


def test_zlib_decodes_every_valid_corpus_stream_to_the_replay_and_refuses_the_invalid_ones():
    cases = dw.corpus()
    assert 500 <= len(cases) <= 600
    n_valid = n_invalid = 0
    for name, stream, want in cases:
        if want is None:
            with pytest.raises(zlib.error):
                _zlib_inflate(stream)
            n_invalid += 1
        else:
            assert len(want) <= 100 * 1024, name
            got, eof, unused = _zlib_inflate(stream)
            assert got == want and eof and unused == b"", (name, len(got), len(want), eof, len(unused))
            n_valid += 1
    assert n_invalid >= 25 and n_valid >= 500
    # the one class the project's decoders refuse by design is valid for zlib
    assert sum(1 for name, _, want in cases if name.startswith(dw.EOB_ONLY) and want is not None) == 2


def test_corpus_places_what_it_names():
    """the cases whose point is a position hold it: stream lengths, and the 48-bit symbol (15 + 5 + 15 + 13) in the named byte"""
    by_name = {name: (stream, want) for name, stream, want in dw.corpus()}
    for n in (1023, 1024, 1025, 2047, 2048, 2049, 4096):
        assert len(by_name["stream_of_%d_bytes" % n][0]) == n
    assert {len(by_name["stream_of_%d_bytes" % (3000 + r)][0]) % 16 for r in range(16)} == set(range(16))
    assert sorted(l for l in dw.S48_LL if l) == dw.STAIR and dw.S48_LL[284] == 15 and dw.LEN_EXTRA[284 - 257] == 5
    assert sorted(l for l in dw.S48_D if l) == dw.STAIR and dw.S48_D[28] == dw.S48_D[29] == 15 and dw.DIST_EXTRA[28] == dw.DIST_EXTRA[29] == 13
    for n in (4095, 4096, 4097, 32767, 32768, 32769, 65536):
        for how in ("literal", "match", "stored"):
            assert len(by_name["out_%d_ends_with_%s" % (n, how)][1]) == n


def test_zlib_decodes_every_random_stream_to_the_replay():
    streams = dw.random_streams()
    assert len(streams) == 200
    kinds = set()
    for k, (stream, want) in enumerate(streams):
        got, eof, unused = _zlib_inflate(stream)
        assert got == want and eof and unused == b"", (k, len(got), len(want))
        assert len(want) <= 40000 + 258
        kinds.add(stream[0] >> 1 & 3)
    assert kinds == {0, 1, 2}  # (first blocks of every type)
    assert dw.random_stream(7) == streams[7]  # seeded: the same stream every time


def test_libdeflate_fixtures_inflate_with_zlib_to_one_fragment_text():
    golden = dw.golden_streams()
    assert len(golden) == 4
    text = golden[0][2]
    rows = text.split(b"\n")
    assert len(rows) == 151 and rows[-1] == b"" and all(len(r.split(b"\t")) == 5 for r in rows[:-1])
    for name, stream, want in golden:
        assert len(stream) <= 4096 and want == text, name
        got, eof, unused = _zlib_inflate(stream)
        assert got == text and eof and unused == b"", name


def test_host_inflate_on_the_corpus_under_the_sanitizers(tmp_path):
    """tests/soak/inflate_corpus_check.cpp, built with AddressSanitizer + UBSan, over every stream: valid ones decode exactly with
    the right in_used (only the end-of-block-only code may be refused), invalid ones return false"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "inflate_corpus_check"
    src = os.path.join(HERE, "soak", "inflate_corpus_check.cpp")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o",
                            str(exe), src], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("the host compiler has no sanitizer runtime")
    assert build.returncode == 0, build.stderr[-2000:]
    assert "warning" not in build.stderr, build.stderr[-2000:]
    entries = dw.all_streams()
    corpus_file = tmp_path / "corpus.bin"
    dw.write_corpus_file(str(corpus_file), entries)
    run = subprocess.run([str(exe), str(corpus_file)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "ok" in run.stdout and "%d streams" % len(entries) in run.stdout
