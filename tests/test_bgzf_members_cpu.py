"""The BGZF member table of the fragment pipeline's loader (csrc/host.cpp: bgzf_member_table, bgzf_last_byte; entry
gtars_bgzf_members): what GTARS_FRAG_INFLATE=device hands to the device without inflating the file.  The checker is the BGZF
reader of tests/bam_ref.py.  Whatever is not BGZF from the first byte to the last is answered with "not BGZF" and takes the
ordinary gzip reader."""
import ctypes as C
import gzip
import struct
import zlib

import numpy as np
import pytest

import bam_ref

PARSE_ERROR = 6


def members(data):
    """-> None (not BGZF) | (stream_off, stream_len, isize, crc, uoff, last_byte)"""
    from gtars_amd import _lib

    buf = np.frombuffer(bytes(data), dtype=np.uint8) if data else np.zeros(1, dtype=np.uint8)
    n = C.c_uint64(0)
    last = C.c_int32(0)
    rc = _lib.lib.gtars_bgzf_members(buf.ctypes.data, len(data), 0, C.addressof(n), None, None, None, None, None, C.addressof(last))
    if rc == PARSE_ERROR:
        assert n.value == 0
        return None
    assert rc == 0
    k = n.value
    soff, uoff = np.zeros(k, dtype=np.uint64), np.zeros(k, dtype=np.uint64)
    slen, isize, crc = (np.zeros(k, dtype=np.uint32) for _ in range(3))
    rc = _lib.lib.gtars_bgzf_members(buf.ctypes.data, len(data), k, C.addressof(n), soff.ctypes.data, slen.ctypes.data, isize.ctypes.data,
                                     crc.ctypes.data, uoff.ctypes.data, None)
    assert rc == 0 and n.value == k
    return soff, slen, isize, crc, uoff, last.value


def check_against_reference(data):
    got = members(data)
    assert got is not None
    blocks, stream = bam_ref.read_blocks(data)
    soff, slen, isize, crc, uoff, last = got
    assert len(blocks) == len(soff)
    for k, (coff, csize, want_isize, want_crc, want_uoff) in enumerate(blocks):
        # (the writer's header is 18 bytes: the raw deflate stream lies between it and the 8-byte trailer)
        assert (soff[k], slen[k], isize[k], crc[k], uoff[k]) == (coff + 18, csize - 26, want_isize, want_crc, want_uoff), k
        assert zlib.decompress(data[int(soff[k]):int(soff[k] + slen[k])], -15) == stream[want_uoff:want_uoff + want_isize]
    assert last == (stream[-1] if stream else -1)
    return got


@pytest.fixture(scope="module")
def text():
    rng = np.random.default_rng(5)
    return b"".join(b"chr%d\t%d\t%d\tBC%04d\t1\n" % (rng.integers(1, 23), s, s + 100, rng.integers(0, 500)) for s in range(0, 400000, 40))


def test_table_equals_the_reference_readers(text):
    assert len(text) > 3 * 0xFF00
    check_against_reference(bam_ref.bgzf_bytes(text))                                   # the writer's own 0xFF00-byte blocks
    check_against_reference(bam_ref.bgzf_bytes(text, eof=False))                        # no EOF block
    got = check_against_reference(bam_ref.bgzf_bytes(text, cuts=[1, 2, 3, 17, 17, 1000, 70000, 70001, len(text) - 1]))
    assert 0 in got[2][:-1]                                                             # (a repeated cut: an empty member in the middle)
    soff, slen, isize, crc, uoff, last = check_against_reference(bam_ref.EOF_BLOCK)     # an empty file: the EOF block alone
    assert list(isize) == [0] and last == -1
    soff, slen, isize, crc, uoff, last = check_against_reference(bam_ref.bgzf_bytes(text[:65536], block=65536))
    assert list(isize) == [65536, 0]                                                    # a member of the largest ISIZE


def test_last_byte_is_found_in_front_of_empty_members(text):
    body = text[:5000] + b"x"  # (no final newline)
    data = bam_ref.bgzf_bytes(body, cuts=[100, 5001, 5001, 5001], eof=True)
    soff, slen, isize, crc, uoff, last = check_against_reference(data)
    assert list(isize[-4:]) == [0, 0, 0, 0] and isize[-5] > 0 and last == ord("x")
    whole = text[:text.rindex(b"\n", 0, 5000) + 1]
    assert check_against_reference(bam_ref.bgzf_bytes(whole, cuts=[len(whole), len(whole)]))[5] == ord("\n")


def test_what_is_not_bgzf_from_end_to_end_is_not_bgzf(text):
    good = bam_ref.bgzf_bytes(text[:3000], cuts=[1000])
    assert members(good) is not None
    assert members(gzip.compress(text[:3000])) is None                                  # plain gzip
    assert members(good + gzip.compress(b"more\n")) is None                             # BGZF, then a plain member
    assert members(gzip.compress(b"more\n") + good) is None
    assert members(good + b"\0") is None and members(good + b"trailing bytes, more than a header's worth") is None
    assert members(good[:-1]) is None and members(good[:-30]) is None                   # a truncated last member
    assert members(b"") is None and members(text[:3000]) is None
    block = bytearray(bam_ref.bgzf_block(text[:1000]))
    assert members(bytes(block)) is not None
    wrong_len = bytearray(block)
    wrong_len[14:16] = struct.pack("<H", 3)                                             # the BC subfield's length: 3
    assert members(bytes(wrong_len)) is None
    other = bytearray(block)
    other[12:14] = b"XY"                                                                # no BC subfield at all
    assert members(bytes(other)) is None
    past = bytearray(block)
    past[16:18] = struct.pack("<H", len(block) + 5)                                     # BSIZE points past the file
    assert members(bytes(past)) is None
    short = bytearray(block)
    short[16:18] = struct.pack("<H", len(block) - 10)                                   # BSIZE stops inside the member
    assert members(bytes(short) + bam_ref.EOF_BLOCK) is None
    flags = bytearray(block)
    flags[3] = 4 | 8                                                                    # FEXTRA + FNAME: not what bgzip writes
    assert members(bytes(flags)) is None
