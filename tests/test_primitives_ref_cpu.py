"""The numpy references and closed-form layouts that the GPU edge tests trust, checked on a machine without a GPU:
tests/primitives_ref.py against element-by-element Python, tests/edge_layouts.py (scaled down to a few thousand
regions: the closed forms do not depend on the tile size) against the plain-Python restatements."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_layouts as E  # noqa: E402
import genomicdist_ref as G  # noqa: E402
import primitives_ref as P  # noqa: E402
import setops_ref as R  # noqa: E402

SMALL = [0, 1, 2, 3, 64, 257, 1500]


def _running_max_loop(seg, val):
    """out[i] = max of val over [segment head, i]"""
    out, cur = [], 0
    for i in range(len(seg)):
        head = i == 0 or seg[i] != seg[i - 1]
        cur = int(val[i]) if head else max(cur, int(val[i]))
        out.append(cur)
    return out


def _open_flags_loop(seg, val, start, gap):
    """out[i] = 1 where i opens a run: a head, or start[i] > sat(max of val over [head, i) + gap)"""
    out, before = [], 0
    for i in range(len(seg)):
        head = i == 0 or seg[i] != seg[i - 1]
        out.append(1 if head or int(start[i]) > min(before + gap, P.M32) else 0)
        before = int(val[i]) if head else max(before, int(val[i]))
    return out


@pytest.mark.parametrize("n", SMALL)
def test_segmented_max_references_match_a_plain_loop(n):
    rng = np.random.default_rng(n)
    pats = P.seg_patterns(n, rng)
    # the tile- and chunk-sized patterns degenerate at these sizes: add segments of a few elements
    pats["short_segments"] = (np.cumsum(rng.random(n) < 0.2).astype(np.uint32), pats["random_segments"][1], pats["random_segments"][2])
    pats["max_values"] = (pats["short_segments"][0], np.where(rng.random(n) < 0.3, P.M32, 5).astype(np.uint32),
                          np.where(rng.random(n) < 0.5, P.M32, 4).astype(np.uint32))
    for name, (seg, val, start) in pats.items():
        assert P.seg_running_max_ref(seg, val).tolist() == _running_max_loop(seg, val), name
        for gap in (0, 100, P.M32):
            assert P.seg_open_flags_ref(seg, val, start, gap).tolist() == _open_flags_loop(seg, val, start, gap), (name, gap)


@pytest.mark.parametrize("n", SMALL)
def test_sort_and_scan_references_match_plain_python(n):
    rng = np.random.default_rng(50 + n)
    chrom = P.chrom_column(n, 300, rng)
    k1 = rng.integers(0, 4, n, dtype=np.uint64).astype(np.uint32)
    k2 = rng.integers(0, 3, n, dtype=np.uint64).astype(np.uint32)
    assert P.sort_perm_ref(chrom, k1, k2).tolist() == sorted(range(n), key=lambda i: (chrom[i], k1[i], k2[i], i))
    assert P.sort_perm_ref(chrom, k1).tolist() == sorted(range(n), key=lambda i: (chrom[i], k1[i], i))
    for name, c in P.scan_count_patterns(n, rng).items():
        want, run = [0], 0
        for x in c.tolist():
            run += x
            want.append(run)
        assert P.scan_ref(c).tolist() == want, name


def test_patterns_hit_the_edges_they_are_named_for():
    rng = np.random.default_rng(1)
    n = P.CHUNK + 2049
    c = P.scan_count_patterns(n, rng)["one_tile_of_3e6"]
    assert int(c[P.TILE:2 * P.TILE].sum(dtype=np.uint64)) >= 1 << 32 and int(c[P.CHUNK:P.CHUNK + P.TILE].sum(dtype=np.uint64)) >= 1 << 32
    pats = P.seg_patterns(n, rng)
    assert np.flatnonzero(P.seg_heads(pats["heads_on_tile_firsts"][0])).tolist() == list(range(0, n, P.TILE))
    assert np.flatnonzero(P.seg_heads(pats["heads_on_tile_lasts"][0])).tolist() == [0] + list(range(P.TILE - 1, n, P.TILE))
    assert np.flatnonzero(P.seg_heads(pats["head_on_chunk_first"][0])).tolist() == [0, P.CHUNK]
    assert np.flatnonzero(P.seg_heads(pats["head_on_chunk_last"][0])).tolist() == [0, P.CHUNK - 1]
    assert P.seg_heads(pats["one_segment_max_first"][0]).sum() == 1 and pats["one_segment_max_first"][1].argmax() == 0
    for n_chrom in P.N_CHROMS:
        ch = P.chrom_column(1000, n_chrom, rng)
        assert ch.min() == 0 and ch.max() == n_chrom - 1
    k = P.sort_key_patterns(n, rng)
    for b in range(4):
        assert len(np.unique(k[f"byte{b}_only"] & ~np.uint32(0xFF << (8 * b)))) == 1 and len(np.unique(k[f"byte{b}_only"])) == 256
    assert len(np.unique(k["one_digit_fills_a_tile"][P.TILE:2 * P.TILE])) == 1


# ------------------------------------------------------------------------------------------- closed-form layouts
def _regs(lay):
    return [(lay.names[c], int(s), int(e)) for c, s, e in zip(lay.chrom.tolist(), lay.start.tolist(), lay.end.tolist())]


def _tuples(names, cols):
    c, s, e = cols
    return [(names[ci], si, ei) for ci, si, ei in zip(c.tolist(), s.tolist(), e.tolist())]


@pytest.mark.parametrize("n", [1, 2, 5000])
def test_covering_layout_closed_forms(n):
    lay = E.covering(n, seed=3)
    regs = _regs(lay)
    assert _tuples(lay.names, lay.reduce) == R.reduce(regs)
    assert lay.cluster0.tolist() == R.cluster(regs, 0)
    assert _tuples(lay.names, lay.disjoin) == G.disjoin(regs)


@pytest.mark.parametrize("per_chrom,shift", [(None, 0), (64, 0), (64, 1), (7, 1)])
@pytest.mark.parametrize("n", [1, 2, 4099])
def test_disjoint_layout_closed_forms(n, per_chrom, shift):
    lay = E.disjoint(n, seed=4, per_chrom=per_chrom, shift=shift)
    regs = _regs(lay)
    assert _tuples(lay.names, lay.reduce) == R.reduce(regs)
    assert lay.cluster0.tolist() == R.cluster(regs, 0)
    assert lay.neighbor_distances.tolist() == G.neighbor_distances(regs)
    assert R.setdiff(regs, regs) == [] and R.intersect(regs, regs) == _tuples(lay.names, lay.reduce) and R.jaccard(regs, regs) == 1.0
    assert lay.chromosome_statistics == G.chromosome_statistics(regs)
    for n_bins in (250, 7):
        assert lay.distribution(n_bins) == G.distribution(regs, n_bins, lay.sizes)
