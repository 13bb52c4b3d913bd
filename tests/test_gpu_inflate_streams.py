"""The device DEFLATE decoder (csrc/inflate_dev.hip, entry gtars_debug_inflate_streams) on streams zlib's compressor never writes:
the corpus and the random streams of tests/deflate_writer.py and the libdeflate fixtures of tests/golden/deflate.  The expected
bytes are the writer's replay, which tests/test_deflate_writer_cpu.py holds to zlib's inflate stream by stream; here they are
taken as given.  A valid stream must come out exact (status 0, length, bytes consumed, bytes); the one class refused by design is
the literal/length code that is only a 1-bit end of block (status 2).  A stream zlib refuses must be refused.  Behind every
stream's output sits a guard stream of 64 bytes' capacity and no output: not a byte of it may change."""
import pytest

import deflate_writer as dw
from test_gpu_inflate import _run

pytestmark = pytest.mark.gpu

GUARD = dw.Deflate().stored(b"", final=True).finish()[0]
GUARD_CAP = 64


def _run_guarded(streams, caps):
    """_run with a guard stream behind every stream -> (status, out_len, consumed, outputs) of the streams themselves, after the
    check that every guard decoded to nothing and its 64 bytes still hold the 0xEE they were filled with"""
    all_streams, all_caps = [], []
    for s, c in zip(streams, caps):
        all_streams += [s, GUARD]
        all_caps += [c, GUARD_CAP]
    st, ln, used, outs = _run(all_streams, all_caps)
    for k in range(len(streams)):
        g = 2 * k + 1
        assert st[g] == 0 and ln[g] == 0 and used[g] == len(GUARD), ("guard", k, st[g], ln[g], used[g])
        assert outs[g] == b"\xEE" * GUARD_CAP, ("bytes behind the capacity of stream", k)
    return st[0::2], ln[0::2], used[0::2], outs[0::2]


def _check_exact(names, streams, wants, result):
    st, ln, used, outs = result
    refused = [(n, int(s)) for n, s in zip(names, st) if s != 0]
    # the cap on refusals is a condition: only the end-of-block-only code, and that with status 2
    assert refused == [(n, 2) for n in names if n.startswith(dw.EOB_ONLY)], refused
    for k, (name, stream, want) in enumerate(zip(names, streams, wants)):
        if st[k] != 0:
            continue
        assert ln[k] == len(want) and used[k] == len(stream), (name, ln[k], len(want), used[k], len(stream))
        assert outs[k][:len(want)] == want, name
        assert set(outs[k][len(want):]) <= {0xEE}, name  # (the bytes up to the next 16-byte boundary)


@pytest.fixture(scope="module")
def valid_launch():
    """the valid corpus and the libdeflate fixtures in one launch, each into a capacity equal to its output"""
    cases = [c for c in dw.corpus() if c[2] is not None] + dw.golden_streams()
    names, streams, wants = (list(x) for x in zip(*cases))
    return names, streams, wants, _run_guarded(streams, [len(w) for w in wants])


def test_device_inflate_decodes_the_corpus_exactly(valid_launch):
    names, streams, wants, result = valid_launch
    assert sum(n.startswith("libdeflate_level") for n in names) == 4 and len(names) > 500
    _check_exact(names, streams, wants, result)


def test_device_inflate_decodes_200_random_streams_exactly():
    pairs = dw.random_streams()
    assert len(pairs) == 200
    streams, wants = [s for s, _ in pairs], [w for _, w in pairs]
    _check_exact(["random_%d" % k for k in dw.RANDOM_SEEDS], streams, wants, _run_guarded(streams, [len(w) for w in wants]))


def test_device_inflate_refuses_short_capacities_and_what_zlib_refuses(valid_launch):
    names, streams, wants, result = valid_launch
    _check_exact(names, streams, wants, result)  # (the refusals are looked at only once the valid launch has passed)
    # capacity one byte short: status 5 wherever the last byte comes from -- a literal, a match, a stored block, across the flush
    # pieces and the window -- and a 200-byte output into 100 bytes, which no 4-KiB check sees on the way
    short = [(n, s, w, len(w) - 1) for n, s, w in zip(names, streams, wants)
             if n.startswith(("out_", "literal_lands_on_", "stored_crosses_", "sym48_p0", "sym48_p63", "win_len258_dist32768_", "periodic_dist1_",
                              "libdeflate_", "final_", "stored_1_and"))]
    assert len(short) >= 50
    by_name = dict(zip(names, zip(streams, wants)))
    s200, w200 = by_name["out_200"]
    assert len(w200) == 200
    short += [("out_200_into_100", s200, w200, 100), ("out_200_into_0", s200, w200, 0)]
    st, ln, used, outs = _run_guarded([s for _, s, _, _ in short], [c for _, _, _, c in short])
    for k, (name, _, _, cap) in enumerate(short):
        assert st[k] == 5, (name, st[k])
        assert set(outs[k][cap:]) <= {0xEE}, name
    # the streams zlib refuses, in a launch of their own; the capacity is no reason to refuse any of them
    bad = [(n, s) for n, s, w in dw.corpus() if w is None]
    assert len(bad) >= 25
    cap = 32768
    st, ln, used, outs = _run_guarded([s for _, s in bad], [cap] * len(bad))
    accepted = [n for (n, _), s in zip(bad, st) if s == 0]
    assert accepted == [], accepted
    assert all(s != 5 for s in st), [(n, int(s)) for (n, _), s in zip(bad, st)]
