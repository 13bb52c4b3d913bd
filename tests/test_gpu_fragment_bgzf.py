"""The fused fragment pipeline on BGZF input with the inflate on the device (GTARS_FRAG_INFLATE=device; csrc/host.cpp: the member
table, csrc/fragparse.hip: the compressed form of a wave's file, csrc/inflate_dev.hip: the member kernel).  Every folder runs four
ways -- device inflate under both ring sizes, GTARS_FRAG_INFLATE=host, and the oracle's restatement of the two-step pipeline --
which must agree barcode by barcode and id by id.  For these zlib-written inputs the library's timing report must say that the
device inflated every BGZF member and handed no file back.  A damaged file raises the message of the host route."""
import ctypes as C
import gzip
import os
import re
import struct
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bam_ref  # noqa: E402
import deflate_writer as dw  # noqa: E402
import fragment_edge_cases as fe  # noqa: E402
from test_sharding_gloo import oracle_fragment_pipeline, same_cluster_results  # noqa: E402

pytestmark = pytest.mark.gpu

RINGS = ("8", "32")


def bgzf(text, cuts=(), level=6, eof=True):
    """the BGZF file of `text`: a member ends at every offset of `cuts` and after 0xFF00 bytes at the latest"""
    out, at = [], 0
    for c in sorted(cuts) + [len(text)]:
        while c - at > 0xFF00:
            out.append(bam_ref.bgzf_block(text[at:at + 0xFF00], level))
            at += 0xFF00
        if c > at:
            out.append(bam_ref.bgzf_block(text[at:c], level))
            at = c
    return b"".join(out) + (bam_ref.EOF_BLOCK if eof else b"")


def host_decoder_accepts_every_member(blob):
    """the generator against the one class of valid streams the device decoder refuses by design (a literal/length code that is
    nothing but a 1-bit end of block): the host's fast decoder refuses the same class, and here it takes every member -> members"""
    from gtars_amd import _lib

    blocks, _ = bam_ref.read_blocks(blob)
    for coff, csize, isize, _, _ in blocks:
        one = np.frombuffer(blob[coff:coff + csize], dtype=np.uint8)
        n, last = C.c_uint64(0), C.c_int32(0)
        rc = _lib.lib.gtars_bgzf_members(one.ctypes.data, len(one), 0, C.addressof(n), None, None, None, None, None, C.addressof(last))
        assert rc == 0 and n.value == 1 and last.value != -2 and (last.value == -1) == (isize == 0), (coff, rc, last.value)
    return len(blocks)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    import gtars_amd
    import oracle
    from gtars_amd.tokenizers import Tokenizer

    assert gtars_amd.device_count() > 0
    return tmp_path_factory.mktemp("fragment_bgzf"), Tokenizer.from_bed(fe.GOLDEN_PEAKS), oracle.OracleTokenizer(fe.GOLDEN_PEAKS)


def make_case(root, name, files, lead=False):
    """files: [(file name, inflated bytes, bytes on disk or None for plain text)] -> the case, and its BGZF members"""
    case = fe.write_case(fe.Case(name, root), files, fe._simple_map(sorted({n.split(".")[0] for n, _, _ in files})), lead=lead)
    n_members = 0
    for n, _, blob in files:
        if blob is not None and blob[:4] == b"\x1f\x8b\x08\x04" and blob[12:14] == b"BC":
            n_members += host_decoder_accepts_every_member(blob)
    return case, n_members


def text_of(seed, n_lines, final_newline=True):
    g = fe.Gen(seed, fe.BARCODES)
    t = "".join(g.natural() for _ in range(n_lines)).encode()
    return t if final_newline else t[:-1]


def run(case, tok):
    from gtars_amd.fragsplit import BarcodeToClusterMap, fragsplit_tokenize

    return fragsplit_tokenize(case.frags, BarcodeToClusterMap.from_file(case.map), tok, as_arrays=True)


REPORT = re.compile(r"device inflate: (\d+) BGZF members inflated on the device, (\d+) files handed back to the host, (\d+) compressed bytes")


def four_ways(case, n_members, world, monkeypatch, capfd, rings=RINGS, min_waves=1):
    import oracle
    from gtars_amd.fragsplit import list_fragment_files

    _, tok, otok = world
    want = oracle_fragment_pipeline(list_fragment_files(case.frags), oracle.OracleBarcodeMap(case.map), otok)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("GTARS_FRAG_INFLATE", "host")
    assert same_cluster_results(run(case, tok), want), (case.name, "host inflate")
    monkeypatch.setenv("GTARS_FRAG_INFLATE", "device")
    monkeypatch.setenv("GTARS_HOST_TIMING", "1")
    for ring in rings:
        monkeypatch.setenv("GTARS_FRAG_INFLATE_RING", ring)
        capfd.readouterr()
        got = run(case, tok)
        err = capfd.readouterr().err
        assert same_cluster_results(got, want), (case.name, "device inflate, ring", ring)
        m, w = REPORT.search(err), re.search(r"(\d+) files in (\d+) wave\(s\)", err)
        assert m and w, err
        # a condition: every BGZF member on the device, no file handed back
        assert (int(m.group(1)), int(m.group(2))) == (n_members, 0), (case.name, ring, m.groups(), n_members)
        assert int(w.group(2)) >= min_waves, err
    monkeypatch.delenv("GTARS_HOST_TIMING")
    # the host parser ignores the switch
    monkeypatch.setenv("GTARS_FRAG_HOST_PARSE", "1")
    assert same_cluster_results(run(case, tok), want), (case.name, "host parser")
    monkeypatch.delenv("GTARS_FRAG_HOST_PARSE")
    return want


def test_member_cuts_inside_lines_fields_and_one_byte_members(world, monkeypatch, capfd):
    t0, t1, t2 = text_of(1, 300), text_of(2, 200), text_of(3, 250)
    nl = [i + 1 for i in range(len(t0)) if t0[i:i + 1] == b"\n"]
    tab = [i for i in range(len(t1)) if t1[i:i + 1] == b"\t"]
    files = [
        ("f0.bed.gz", t0, bgzf(t0, nl[::7])),                                            # directly behind a newline
        ("f1.bed.gz", t1, bgzf(t1, [x + 2 for x in tab[::5]] + [x for x in tab[3::11]])),   # inside a field, and in front of a tab
        ("f2.bed.gz", t2, bgzf(t2, list(range(1000, 1060)) + [5000, 5003, len(t2) - 1])),  # one byte per member for a stretch
        ("f3.bed.gz", t0, bgzf(t0, [len(t0) // 2 + 13], level=1)),                       # inside a line
    ]
    case, n = make_case(world[0], "cuts", files)
    assert n > 150
    want = four_ways(case, n, world, monkeypatch, capfd)
    assert sum(int(v[1][-1]) for v in want.values()) > 0


def test_file_shapes_and_a_wave_of_all_three_forms(world, monkeypatch, capfd):
    t = [text_of(10 + k, 120 + 10 * k) for k in range(7)]
    no_nl = text_of(20, 150, final_newline=False)
    empties = bgzf(no_nl, [100])[:-len(bam_ref.EOF_BLOCK)] + bam_ref.bgzf_block(b"") * 3 + bam_ref.EOF_BLOCK
    files = [
        ("g0.bed.gz", t[0], bgzf(t[0], [777])),
        ("g1.bed.gz", no_nl, bgzf(no_nl, [4000])),                    # no final newline: the loader appends one
        ("g2.bed.gz", b"", bam_ref.EOF_BLOCK),                        # the EOF block alone
        ("g3.bed.gz", t[1], bgzf(t[1], [1], eof=False)),              # no EOF block
        ("g4.bed.gz", t[2], gzip.compress(t[2])),                     # plain gzip: inflated by the host threads
        ("g5.bed", t[3], None),                                       # plain text
        ("g6.bed.gz", t[4], bgzf(t[4], [50], level=0)),               # stored blocks
        ("g7.bed.gz", no_nl, empties),                                # no final newline, empty members behind the last byte
        ("g8.bed.gz", t[5], bgzf(t[5], [], level=9)),
        ("g9.bed.gz", t[6], gzip.compress(t[6][:3000]) + bgzf(t[6][3000:])),  # a plain member in front of BGZF ones: host
    ]
    case, n = make_case(world[0], "shapes", files)
    want = four_ways(case, n, world, monkeypatch, capfd)
    assert sum(int(v[1][-1]) for v in want.values()) > 0


def test_two_waves(world, monkeypatch, capfd):
    t = [text_of(30 + k, 200) for k in range(3)]
    files = [("h%d.bed.gz" % k, t[k], bgzf(t[k], [999 * (k + 1)])) for k in range(3)]
    case, n = make_case(world[0], "two_waves", files, lead=True)
    lead = bgzf(fe._lead_text(), level=1)  # (1 MiB under GTARS_FRAG_BATCH_MB=1: a batch of its own)
    with open(case.path(fe.LEAD_NAME), "wb") as f:
        f.write(lead)
    case.env["GTARS_FRAG_DEVICE_WAVE_MB"] = "2"
    four_ways(case, n + host_decoder_accepts_every_member(lead), world, monkeypatch, capfd, min_waves=2)


def test_a_valid_member_the_device_refuses_is_handed_back_and_decoded_by_the_host(world, monkeypatch, capfd):
    """a member whose last block is the end-of-block-only code: valid for zlib, refused by design on the device (status 2) -- the
    file goes back to the host's decoders and the call ends with the same result as under GTARS_FRAG_INFLATE=host"""
    import oracle
    from gtars_amd.fragsplit import list_fragment_files

    t = [text_of(60 + k, 80) for k in range(3)]
    ll = [0] * 257
    ll[256] = 1
    stream, data = dw.Deflate().fixed(list(t[1][:900])).dynamic(ll, [0], [], final=True).finish()
    assert data == t[1][:900] and zlib.decompress(stream, -15) == data
    member = (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(stream) + 25) + stream +
              struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))
    files = [("v0.bed.gz", t[0], bgzf(t[0], [500])), ("v1.bed.gz", t[1], member + bgzf(t[1][900:], [300])), ("v2.bed.gz", t[2], bgzf(t[2]))]
    assert bam_ref.read_blocks(files[1][2])[1] == t[1]
    case = fe.write_case(fe.Case("handed_back", world[0]), files, fe._simple_map(["v0", "v1", "v2"]))
    _, tok, otok = world
    want = oracle_fragment_pipeline(list_fragment_files(case.frags), oracle.OracleBarcodeMap(case.map), otok)
    monkeypatch.setenv("GTARS_FRAG_INFLATE", "host")
    assert same_cluster_results(run(case, tok), want)
    monkeypatch.setenv("GTARS_FRAG_INFLATE", "device")
    monkeypatch.setenv("GTARS_HOST_TIMING", "1")
    for ring in RINGS:
        monkeypatch.setenv("GTARS_FRAG_INFLATE_RING", ring)
        capfd.readouterr()
        got = run(case, tok)
        m = REPORT.search(capfd.readouterr().err)
        assert same_cluster_results(got, want), ring
        # (the wave ran again without v1: the members of the other two files)
        assert m and int(m.group(2)) == 1 and int(m.group(1)) == len(bam_ref.read_blocks(files[0][2])[0]) + len(bam_ref.read_blocks(files[2][2])[0]), m


def _damaged(kind, good):
    """`good`: a BGZF file of several members; the damage is in the second"""
    blocks, _ = bam_ref.read_blocks(good)
    coff, csize, isize, crc, _ = blocks[1]
    b = bytearray(good)
    if kind == "flipped_bit":
        b[coff + 18 + (csize - 26) // 2] ^= 0x10
    elif kind == "wrong_crc":
        b[coff + csize - 8:coff + csize - 4] = struct.pack("<I", crc ^ 1)
    elif kind == "isize_too_small":
        b[coff + csize - 4:coff + csize] = struct.pack("<I", isize - 1)
    elif kind == "isize_too_large":
        b[coff + csize - 4:coff + csize] = struct.pack("<I", isize + 1)
    elif kind == "truncated":
        return good[:-len(bam_ref.EOF_BLOCK) - 9]
    return bytes(b)


@pytest.mark.parametrize("kind", ["flipped_bit", "wrong_crc", "isize_too_small", "isize_too_large", "truncated"])
def test_damaged_files_raise_the_host_routes_message(world, monkeypatch, kind):
    t = [text_of(40 + k, 150) for k in range(3)]
    files = [("e%d.bed.gz" % k, t[k], bgzf(t[k], [2000, 4000])) for k in range(3)]
    files[1] = (files[1][0], t[1], _damaged(kind, files[1][2]))  # (the good file behind it must not mask it)
    case = fe.write_case(fe.Case("damaged_" + kind, world[0]), files, fe._simple_map(["e0", "e1", "e2"]))
    _, tok, _ = world
    monkeypatch.setenv("GTARS_FRAG_INFLATE", "host")
    with pytest.raises(RuntimeError) as e:
        run(case, tok)
    want = str(e.value)
    print(kind, "->", want)
    monkeypatch.setenv("GTARS_FRAG_INFLATE", "device")
    for ring in RINGS:
        monkeypatch.setenv("GTARS_FRAG_INFLATE_RING", ring)
        with pytest.raises(RuntimeError) as e:
            run(case, tok)
        assert str(e.value) == want, (kind, ring)


def test_forty_random_folders(world, monkeypatch, capfd):
    rng = np.random.default_rng(2024)
    for k in range(40):
        files = []
        for f in range(int(rng.integers(1, 4))):
            t = text_of(1000 + 10 * k + f, int(rng.integers(1, 120)), final_newline=bool(rng.integers(0, 4)))
            form = int(rng.integers(0, 6))
            name = "r%d.bed%s" % (f, "" if form == 0 else ".gz")
            if form == 0:
                blob = None
            elif form == 1:
                blob = gzip.compress(t, int(rng.integers(1, 10)))
            else:
                cuts = [int(x) for x in rng.integers(0, len(t) + 1, int(rng.integers(0, 12)))]
                blob = bgzf(t, cuts, level=int(rng.choice([0, 1, 6, 9])), eof=bool(rng.integers(0, 5)))
            files.append((name, t, blob))
        case, n = make_case(world[0], "random_%d" % k, files)
        case.env = {"GTARS_FRAG_DEVICE_THREADS": str(int(rng.integers(1, 3)))}
        if rng.integers(0, 3) == 0:
            case.env["GTARS_FRAG_HOST_CRC"] = "1"  # (plain gzip files: checked by the host; BGZF ones stay on the device)
        four_ways(case, n, world, monkeypatch, capfd, rings=(RINGS[k % 2],))
        for name in case.env:
            monkeypatch.delenv(name)
