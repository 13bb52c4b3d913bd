"""numpy references of the three device primitives (stable sort permutation, u32 -> u64 exclusive scan, segmented
max-scan) for tests/test_gpu_primitives.py, and the input patterns those tests run.  The references are vectorised so
that 2^24 elements cost seconds; tests/test_primitives_ref_cpu.py checks them against element-by-element Python at
small sizes on a machine without a GPU.
"""
from __future__ import annotations

import numpy as np

M32 = 0xFFFFFFFF
TILE = 2048            # elements per workgroup tile of all three primitives
CHUNK = 1024 * TILE    # tiles are combined 1024 at a time by one workgroup: 2^21 elements per chunk

SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4097, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 2049]
SORT_DIGIT_TABLE_SIZE = 2048 * 8192 + 1  # 256 digits x 8193 tiles: the digit table's scan takes a second chunk
# a small, a tile-edge and a chunk-edge size for the value patterns
PATTERN_SIZES = [300, 2 * TILE + 1, CHUNK + 2049]


# ------------------------------------------------------------------------------------------------------------- sort
def sort_perm_ref(chrom, k1, k2=None):
    """perm such that (chrom, k1, [k2], input row) ascends"""
    n = len(chrom)
    if k2 is None:
        return np.lexsort((np.arange(n), k1, chrom)).astype(np.uint32)
    return np.lexsort((np.arange(n), k2, k1, chrom)).astype(np.uint32)


def sort_key_patterns(n, rng):
    """name -> one u32 key column of n elements"""
    i = np.arange(n, dtype=np.uint64)
    out = {
        "all_equal": np.full(n, 0x12345678, dtype=np.uint32),
        "sorted": (i * 3).astype(np.uint32),
        "reversed": ((n - i) * 3).astype(np.uint32),
        "top_byte_only": (rng.integers(0, 256, n, dtype=np.uint64) << 24).astype(np.uint32),
        "zero_and_ones": np.where(rng.random(n) < 0.5, 0, M32).astype(np.uint32),
    }
    for b in range(4):
        out[f"byte{b}_only"] = ((rng.integers(0, 256, n, dtype=np.uint64) << (8 * b)) | 0x01010101 & ~(0xFF << (8 * b))).astype(np.uint32)
    # one digit holds a whole tile: the second tile (and the tile at the chunk seam) is constant, the rest random
    k = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    k[TILE:2 * TILE] = 0xABABABAB
    k[CHUNK:CHUNK + TILE] = 0xCDCDCDCD
    if n <= TILE:
        k[:] = 0xABABABAB
        k[n // 2:] = 0xABABABAC
    out["one_digit_fills_a_tile"] = k
    return out


N_CHROMS = [1, 2, 255, 256, 257, 65_536, 65_537, (1 << 24) + 1]


def chrom_column(n, n_chrom, rng):
    """ids in [0, n_chrom) with 0 and n_chrom - 1 present (n >= 2), heavy on the extremes of every key byte"""
    c = rng.integers(0, n_chrom, n, dtype=np.uint64)
    edge = rng.random(n) < 0.2
    c[edge] = rng.choice(np.array([0, n_chrom - 1, n_chrom // 2, min(255, n_chrom - 1), min(256, n_chrom - 1),
                                   min(65_535, n_chrom - 1), min(65_536, n_chrom - 1)], dtype=np.uint64), int(edge.sum()))
    if n >= 2:
        a, b = rng.choice(n, 2, replace=False)
        c[a], c[b] = 0, n_chrom - 1
    return c.astype(np.uint32)


# ------------------------------------------------------------------------------------------------------------- scan
def scan_ref(counts):
    out = np.zeros(len(counts) + 1, dtype=np.uint64)
    np.cumsum(np.asarray(counts, dtype=np.uint64), out=out[1:])
    return out


def scan_count_patterns(n, rng):
    out = {
        "all_zero": np.zeros(n, dtype=np.uint32),
        "all_one": np.ones(n, dtype=np.uint32),
        "all_max": np.full(n, M32, dtype=np.uint32),
        "random": rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32),
    }
    for pos in sorted({0, TILE - 1, TILE, n - 1}):
        if 0 <= pos < n:
            c = np.zeros(n, dtype=np.uint32)
            c[pos] = 0x9000_0001
            out[f"single_at_{pos}"] = c
    # one tile whose 2048 counts sum to 6.1e9 >= 2^32, between ordinary tiles; a second one at the chunk seam
    c = rng.integers(0, 50, n, dtype=np.uint64).astype(np.uint32)
    c[TILE:2 * TILE] = 3_000_000
    c[CHUNK:CHUNK + TILE] = 3_000_000
    if n <= TILE:
        c[:] = 3_000_000
    out["one_tile_of_3e6"] = c
    return out


# ---------------------------------------------------------------------------------------------------- segmented max
def seg_heads(seg):
    seg = np.asarray(seg)
    h = np.ones(len(seg), dtype=bool)
    h[1:] = seg[1:] != seg[:-1]
    return h


def seg_running_max_ref(seg, val):
    """out[i] = max of val over [head of i's segment, i]; a head is element 0 and every i with seg[i] != seg[i - 1]"""
    n = len(seg)
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    sid = np.cumsum(seg_heads(seg), dtype=np.int64) - 1  # ascending, so the running maximum of (sid, val) never leaves a segment
    key = (sid << 33) | np.asarray(val, dtype=np.int64)
    return (np.maximum.accumulate(key) - (sid << 33)).astype(np.uint32)


def seg_open_flags_ref(seg, val, start, gap):
    """out[i] = 1 where i opens a run: a head, or start[i] > min(max of val over [head, i) + gap, 2^32 - 1)"""
    n = len(seg)
    if n == 0:
        return np.zeros(0, dtype=np.uint32)
    h = seg_heads(seg)
    incl = seg_running_max_ref(seg, val).astype(np.int64)
    before = np.zeros(n, dtype=np.int64)
    before[1:] = incl[:-1]  # (only read where i is not a head: there i - 1 is in i's segment)
    lim = np.minimum(before + int(gap), M32)
    return (h | (np.asarray(start, dtype=np.int64) > lim)).astype(np.uint32)


def seg_patterns(n, rng):
    """name -> (seg, val, start): segment ids (only their changes matter), values, starts for the flag form"""
    i = np.arange(n, dtype=np.int64)
    rnd_val = rng.integers(0, 1 << 20, n, dtype=np.uint64).astype(np.uint32)
    # starts around the running maximum so that both answers occur
    rnd_start = rng.integers(0, (1 << 20) + 300, n, dtype=np.uint64).astype(np.uint32)
    out = {}
    v = rnd_val.copy()
    if n:
        v[0] = M32 - 7
    s = rnd_start.copy()
    s[rng.random(n) < 0.3] = M32  # above everything unless the limit saturates
    s[rng.random(n) < 0.1] = M32 - 7
    out["one_segment_max_first"] = (np.zeros(n, dtype=np.uint32), v, s)
    out["every_element_a_head"] = (i.astype(np.uint32), rnd_val, rnd_start)
    out["heads_on_tile_firsts"] = ((i // TILE).astype(np.uint32), rnd_val, rnd_start)
    out["heads_on_tile_lasts"] = (((i + 1) // TILE).astype(np.uint32), rnd_val, rnd_start)
    out["head_on_chunk_first"] = ((i >= CHUNK).astype(np.uint32) if n > CHUNK else (i >= n // 2).astype(np.uint32), rnd_val, rnd_start)
    out["head_on_chunk_last"] = ((i >= CHUNK - 1).astype(np.uint32) if n > CHUNK else (i >= n - 1).astype(np.uint32), rnd_val, rnd_start)
    zo = np.where(rng.random(n) < 0.002, M32, 0).astype(np.uint32)
    out["values_zero_and_max"] = ((i // 5000).astype(np.uint32), zo, np.where(rng.random(n) < 0.5, M32, 0).astype(np.uint32))
    # long random segments: some span many tiles, most heads fall inside tiles
    seg = np.cumsum(rng.random(n) < 1.0 / 3000).astype(np.uint32)
    out["random_segments"] = (seg, rnd_val, rnd_start)
    return out
