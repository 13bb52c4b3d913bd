"""The member kernel of the device DEFLATE decoder (csrc/inflate_dev.hip, entry gtars_debug_inflate_members) as the fused fragment
pipeline launches it on the members of BGZF files: streams at ANY byte offset of the compressed buffer, outputs packed back to
back at ANY byte offset, under both ring sizes (32 KiB: every match source in LDS; 8 KiB: far sources read back from the result).
The checker is zlib for what zlib's compressor writes and the replay of tests/deflate_writer.py for what it never writes.  The
output buffer is filled with 0xEE and the members' ranges touch: after every launch the WHOLE buffer is compared, so a store
outside a member's range shows either as a changed 0xEE or as a wrong byte of the neighbour."""
import zlib

import numpy as np
import pytest

import deflate_writer as dw
from test_gpu_inflate import _deflate, _fragment_text

pytestmark = pytest.mark.gpu

RINGS = (8, 32)
HEAD = 37  # bytes in front of the first member's output (odd: the first member starts unaligned as well)


def _launch(streams, caps, ring, in_gaps=None, out_start=HEAD):
    """streams packed at in_gaps[k] junk bytes behind the previous one, outputs packed back to back from out_start ->
    (status, out_len, consumed, the whole output buffer, output offsets)"""
    import torch
    from gtars_amd import _lib

    dev = torch.device("cuda:0")
    n = len(streams)
    in_gaps = in_gaps if in_gaps is not None else [(7 * k + 3) % 16 for k in range(n)]
    in_off, at = [], 0
    for s, g in zip(streams, in_gaps):
        at += g
        in_off.append(at)
        at += len(s)
    blob = np.full(at + 64, 0xA5, dtype=np.uint8)  # (junk between and behind the streams: the decoder may read it, never use it)
    for o, s in zip(in_off, streams):
        blob[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    out_off = list(out_start + np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.int64)) if n else []
    total = out_start + int(sum(caps)) + 64
    mk = lambda a, dt: torch.from_numpy(np.asarray(a, dtype=dt)).to(dev)
    d_blob = torch.from_numpy(blob).to(dev)
    d_out = torch.full((total,), 0xEE, dtype=torch.uint8, device=dev)
    d_in_off, d_in_len = mk(in_off, np.uint64), mk([len(s) for s in streams], np.uint32)
    d_out_off, d_cap = mk(out_off, np.uint64), mk(caps, np.uint32)
    d_len, d_used, d_st = (torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev) for _ in range(3))
    rc = _lib.lib.gtars_debug_inflate_members(d_blob.data_ptr(), d_in_off.data_ptr(), d_in_len.data_ptr(), d_out.data_ptr(), d_out_off.data_ptr(),
                                              d_cap.data_ptr(), n, d_len.data_ptr(), d_used.data_ptr(), d_st.data_ptr(), ring,
                                              torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    return d_st.cpu().numpy()[:n], d_len.cpu().numpy()[:n], d_used.cpu().numpy()[:n], d_out.cpu().numpy().tobytes(), out_off


def _expect_all_exact(streams, wants, ring, names=None, **kw):
    """every stream valid, capacity = its output: status, lengths and the whole buffer, 0xEE around the members"""
    st, ln, used, out, out_off = _launch(streams, [len(w) for w in wants], ring, **kw)
    names = names or list(range(len(streams)))
    bad = [(nm, int(s)) for nm, s in zip(names, st) if s != 0]
    assert not bad, bad
    for k, nm in enumerate(names):
        assert ln[k] == len(wants[k]) and used[k] == len(streams[k]), (nm, ln[k], len(wants[k]), used[k], len(streams[k]))
    start = kw.get("out_start", HEAD)
    want = b"\xEE" * start + b"".join(wants) + b"\xEE" * 64
    if out != want:
        at = next(i for i in range(len(want)) if out[i] != want[i])
        k = int(np.searchsorted(np.asarray(out_off, dtype=np.int64), at, side="right")) - 1
        raise AssertionError(("first wrong byte", at, "member", names[max(k, 0)], "at its byte", at - (out_off[k] if k >= 0 else 0)))


@pytest.fixture(scope="module")
def text():
    return _fragment_text(np.random.default_rng(41), 6000)  # ~270 KB


@pytest.mark.parametrize("ring", RINGS)
def test_every_pair_of_input_and_output_misalignment_in_one_launch(text, ring):
    """256 members of 100-300 bytes: member k's stream starts at k % 16 and its output at k // 16, modulo 16"""
    datas, gaps, in_at, out_at, src, pairs = [], [], 0, 48, 0, set()
    for k in range(256):
        # (the outputs touch: a member's length decides where the next one starts)
        n = 100 + (((k + 1) // 16) % 16 - (out_at + 100)) % 16 + 16 * (k % 12)
        assert 100 <= n <= 300
        d = text[src:src + n]
        src += n
        s = _deflate(d)
        g = (k % 16 - in_at) % 16
        gaps.append(g)
        pairs.add(((in_at + g) % 16, out_at % 16))
        in_at += g + len(s)
        datas.append((s, d))
        out_at += n
    assert len(pairs) == 256
    _expect_all_exact([s for s, _ in datas], [d for _, d in datas], ring, in_gaps=gaps, out_start=48)


LENGTHS = (0, 1, 15, 16, 17, 4095, 4096, 4097, 8191, 8192, 8193, 65280, 65535, 65536)


@pytest.mark.parametrize("ring", RINGS)
def test_output_lengths_around_the_vector_the_flush_piece_the_ring_and_the_largest_member(text, ring):
    names, streams, wants = [], [], []
    for n in LENGTHS:
        d = text[1000:1000 + n]
        for kind, s, w in (("literals", _deflate(d, 6, zlib.Z_HUFFMAN_ONLY), d), ("stored", _deflate(d, 0), d),
                           ("run", _deflate(b"\n" * n, 6), b"\n" * n), ("level6", _deflate(d, 6), d)):
            names.append("%s_%d" % (kind, n))
            streams.append(s)
            wants.append(w)
    _expect_all_exact(streams, wants, ring, names)


def _far_match_streams():
    """matches whose sources lie at the ring's edge, built by hand: a stored filler of random bytes, then a fixed-code block of
    matches at distance R - 258 .. R + 257 and 32768 for R = 8192 and 32768 -- lengths 3 and 258; with length 258 and a distance
    just below R the first source bytes have left an R-byte ring and the last have not -- and literals in between, so that the
    matches start at different offsets from the last flush"""
    rng = np.random.default_rng(42)
    out = []
    for filler in (32768 + 5, 36864 - 100, 40000):
        for r in (8192, 32768):
            dists = sorted({d for d in (r - 258, r - 100, r - 1, r, r + 1, r + 257, 32768) if d <= 32768})
            d = dw.Deflate()
            data = bytes(rng.integers(0, 256, filler, dtype=np.uint8))
            d.stored(data[:30000]).stored(data[30000:])
            tokens = []
            for dist in dists:
                tokens += [(258, dist), 65, (3, dist), (258, dist), 66, 67]
            tokens += [(258, x) for x in dists] * 8  # (across a flush piece: 14 KB of far matches in a row)
            d.fixed(tokens, final=True)
            s, w = d.finish()
            assert len(w) <= 65536
            out.append(("far_r%d_filler%d" % (r, filler), s, w))
    return out


@pytest.mark.parametrize("ring", RINGS)
def test_matches_at_the_edge_of_the_ring_and_at_the_largest_distance(ring):
    names, streams, wants = (list(x) for x in zip(*_far_match_streams()))
    for s, w in zip(streams, wants):
        assert zlib.decompress(s, -15) == w
    _expect_all_exact(streams, wants, ring, names)


GUARD_STREAM, GUARD_BYTES = dw.Deflate().fixed(list(b"<guard>"), final=True).finish()


def _launch_between_guards(streams, caps, ring):
    """a 7-byte guard member in front of, between and behind the streams: a byte written outside a stream's capacity is a wrong
    byte of a guard, or a changed 0xEE -> (status, out_len, consumed, outputs up to the capacity) of the streams themselves"""
    all_s, all_c = [GUARD_STREAM], [len(GUARD_BYTES)]
    for s, c in zip(streams, caps):
        all_s += [s, GUARD_STREAM]
        all_c += [c, len(GUARD_BYTES)]
    st, ln, used, out, off = _launch(all_s, all_c, ring)
    assert set(out[:HEAD]) == {0xEE} and set(out[-64:]) == {0xEE}
    for g in range(0, len(all_s), 2):
        assert st[g] == 0 and out[off[g]:off[g] + len(GUARD_BYTES)] == GUARD_BYTES, ("guard", g // 2)
    return st[1::2], ln[1::2], used[1::2], [out[off[k]:off[k] + all_c[k]] for k in range(1, len(all_s), 2)]


@pytest.fixture(scope="module")
def valid_cases():
    cases = [c for c in dw.corpus() if c[2] is not None and len(c[2]) <= 65536]
    cases += [("random_%d" % k, s, w) for k, (s, w) in zip(dw.RANDOM_SEEDS, dw.random_streams())]
    assert len(cases) > 600 and sum(n.startswith("random_") for n, _, _ in cases) == 200
    return cases


@pytest.mark.parametrize("ring", RINGS)
def test_the_writers_corpus_and_random_streams_at_odd_offsets(valid_cases, ring):
    names, streams, wants = (list(x) for x in zip(*valid_cases))
    st, ln, used, out, off = _launch(streams, [len(w) for w in wants], ring)
    refused = [(n, int(s)) for n, s in zip(names, st) if s != 0]
    # a condition: the end-of-block-only code is the one class refused, and with status 2
    assert refused == [(n, 2) for n in names if n.startswith(dw.EOB_ONLY)], refused
    assert set(out[:HEAD]) == {0xEE} and set(out[-64:]) == {0xEE}
    for k, (name, s, w) in enumerate(valid_cases):
        if st[k] != 0:
            continue
        assert ln[k] == len(w) and used[k] == len(s), (name, ln[k], len(w), used[k], len(s))
        assert out[off[k]:off[k] + len(w)] == w, name


@pytest.mark.parametrize("ring", RINGS)
def test_refusals_leave_the_neighbours_alone(valid_cases, ring):
    # what zlib refuses is refused, whatever it wrote stays inside its capacity
    bad = [(n, s) for n, s, w in dw.corpus() if w is None]
    assert len(bad) >= 25
    st, ln, used, outs = _launch_between_guards([s for _, s in bad], [32768] * len(bad), ring)
    assert [n for (n, _), s in zip(bad, st) if s == 0] == []
    assert all(s != 5 for s in st), [(n, int(s)) for (n, _), s in zip(bad, st)]
    # a capacity one byte short: status 5 wherever the last byte comes from, and the guard behind it untouched
    short = [(n, s, w) for n, s, w in valid_cases
             if len(w) >= 1 and n.startswith(("out_", "literal_lands_on_", "stored_crosses_", "sym48_p0", "sym48_p63", "win_len258_dist32768_",
                                              "periodic_dist1_", "final_", "stored_1_and", "random_1"))]
    assert len(short) >= 50
    st, ln, used, outs = _launch_between_guards([s for _, s, _ in short], [len(w) - 1 for _, _, w in short], ring)
    assert [(n, int(x)) for (n, _, _), x in zip(short, st) if x != 5] == []
