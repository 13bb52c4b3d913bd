"""Inputs and the reference for hit totals that need more than 32 bits (tests/test_gpu_wide_totals.py), in plain numpy.

A universe of ``n_u`` STACKED intervals -- interval i is ``[base + i, base + length + i)`` on chromosome 0 -- gives a query up to
``n_u`` hits, so a batch of 1.4e5 queries reaches 7e9 hits while the inputs stay a few megabytes.  A few dozen ordinary
intervals on chromosomes 1 and 2 keep the chromosome offsets from being all zero.

The batch is an INDEX VECTOR into a pool of at most 256 distinct queries.  The reference counts the pool by the definition
(interval.rs:48-50: ``s < qe and e > qs`` on the same chromosome; kept iff ``min_overlap <= 1 or min(e, qe) - max(s, qs) >=
min_overlap``), every pool entry against every interval, in int64 -- no closed form stands in for it -- and a batch's counts
are a lookup, its offsets an int64 cumulative sum.  This module imports neither the library nor the oracle.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

UNK = 0xFFFFFFFF
LENGTH = 1_000_000
POOL_MAX = 256
TWO32 = 1 << 32


def stacked(n_u: int, base: int = 0, length: int = LENGTH, nest: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (chrom, start, end) as int64: interval i = [base + i, base + length + i) on chromosome 0; every one of them contains
    [base + n_u, base + length), which needs n_u < length.  ``nest``: every nest-th interval ends 2 * length later -- it
    contains its followers, which is what moves it to a second AIList sub-list (ailist.rs:198-236); the common part stays."""
    assert 0 < n_u < length and base + 3 * length + n_u <= UNK
    i = np.arange(n_u, dtype=np.int64)
    s, e = base + i, base + length + i
    if nest:
        e[::nest] += 2 * length
    return np.zeros(n_u, dtype=np.int64), s, e


def extras(seed: int = 3, per_chrom: int = 24) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """ordinary intervals on chromosomes 1 and 2 (some overlap their neighbours)"""
    rng = np.random.default_rng(seed)
    c = np.repeat(np.array([1, 2], dtype=np.int64), per_chrom)
    s = np.sort(rng.integers(0, 50_000, (2, per_chrom)), axis=1).reshape(-1).astype(np.int64)
    e = s + rng.integers(1, 4_000, 2 * per_chrom)
    return c, s, e


def universe(n_u: int, base: int = 0, length: int = LENGTH, nest: int = 0):
    """the stack followed by the extras -> (chrom, start, end) int64, 3 chromosomes"""
    return tuple(np.concatenate(p) for p in zip(stacked(n_u, base, length, nest), extras()))


N_FULL = 8


def query_pool(n_u: int, base: int = 0, n_prefix: int = 200, seed: int = 11, length: int = LENGTH):
    """-> (chrom, start, end, kind) of at most POOL_MAX distinct queries; kind: 0 full ([base + n_u + j, + 10): hits all n_u of the
    stack), 1 prefix ([base + k, base + k + 1): hits the k + 1 intervals that start at or before base + k), 2 the others
    (chromosomes 1 and 2, misses, one unknown chromosome)."""
    rng = np.random.default_rng(seed)
    rows = [(0, base + n_u + j, base + n_u + j + 10, 0) for j in range(N_FULL)]
    ks = np.unique(np.concatenate([[0, 1, n_u - 2, n_u - 1], rng.integers(0, n_u, n_prefix)]))[:n_prefix]
    rows += [(0, base + int(k), base + int(k) + 1, 1) for k in ks]
    ec, es, ee = extras()
    for j in range(0, len(ec), 3):  # on chromosomes 1 and 2: around an interval's start, 1 to a few hits
        rows.append((int(ec[j]), max(int(es[j]) - 5, 0), int(es[j]) + 900, 2))
    rows.append((0, base + 3 * length + n_u + 7, base + 3 * length + n_u + 9, 2))  # behind every end: a miss
    rows.append((1, 60_000_000, 60_000_010, 2))                                    # a miss on chromosome 1
    if base:
        rows.append((0, 5, 25, 2))                                                 # in front of every start
    rows.append((UNK, base + n_u, base + n_u + 10, 2))                             # an unknown chromosome
    a = np.array(rows, dtype=np.int64)
    assert len(a) <= POOL_MAX and len(np.unique(a[:, :3], axis=0)) == len(a)
    return a[:, 0], a[:, 1], a[:, 2], a[:, 3]


def pool_counts(uni, pool, min_overlap: Optional[int] = None, group=None, n_groups: int = 1) -> np.ndarray:
    """The definition, pool entry by pool entry over ALL intervals -> int64[len(pool), n_groups]: hits of each pool query among
    the intervals of each group (``group``: an id per interval -- the IGD file; None: one group)."""
    c, s, e = (np.asarray(x, dtype=np.int64) for x in uni)
    qc, qs, qe = (np.asarray(x, dtype=np.int64) for x in pool[:3])
    mo = 0 if min_overlap is None else int(min_overlap)
    out = np.zeros((len(qc), n_groups), dtype=np.int64)
    grp = None if group is None else np.asarray(group)
    for chrom in np.unique(qc):
        rows = np.flatnonzero(c == chrom)  # (chrom equal): the intervals every query of this chromosome is tested against
        sc, ec = s[rows], e[rows]
        for k in np.flatnonzero(qc == chrom):
            hit = (sc < qe[k]) & (ec > qs[k])
            if mo > 1:
                hit &= np.minimum(ec, qe[k]) - np.maximum(sc, qs[k]) >= mo
            if grp is None:
                out[k, 0] = np.count_nonzero(hit)
            else:
                out[k] = np.bincount(grp[rows[hit]], minlength=n_groups)
    return out


def batch_offsets(counts: np.ndarray, idx: np.ndarray) -> np.ndarray:
    """CSR offsets int64[len(idx) + 1] of the batch pool[idx], counts = pool_counts(...)[:, 0]"""
    off = np.zeros(len(idx) + 1, dtype=np.int64)
    np.cumsum(counts[idx], out=off[1:])
    return off


def batch_group_totals(counts: np.ndarray, idx: np.ndarray, binary: bool = False) -> list:
    """per group the batch's total as Python ints; binary: the number of the batch's queries with any hit in the group"""
    per = np.bincount(idx, minlength=len(counts))  # how often each pool entry is in the batch
    c = (counts > 0) if binary else counts
    return [sum(int(n) * int(v) for n, v in zip(per, c[:, g]) if n) for g in range(counts.shape[1])]


def mixed_batch(kind: np.ndarray, nq: int, seed: int = 5, others: float = 0.03) -> np.ndarray:
    """index vector int64[nq]: full queries at the even positions, at the odd ones prefix queries and (a share of `others`)
    the other kinds"""
    rng = np.random.default_rng(seed)
    full, prefix, rest = (np.flatnonzero(kind == k) for k in (0, 1, 2))
    idx = np.empty(nq, dtype=np.int64)
    idx[0::2] = full[np.arange((nq + 1) // 2) % len(full)]
    odd = nq // 2
    pick = np.where(rng.random(odd) < others, rest[rng.integers(0, len(rest), odd)], prefix[rng.integers(0, len(prefix), odd)])
    idx[1::2] = pick
    return idx


def heavy_first_batch(kind: np.ndarray, n_heavy: int, n_mixed: int, seed: int = 9) -> np.ndarray:
    """n_heavy full queries in a row, then n_mixed mixed ones"""
    full = np.flatnonzero(kind == 0)
    return np.concatenate([full[np.arange(n_heavy) % len(full)], mixed_batch(kind, n_mixed, seed)])


def in_order(pool, idx: np.ndarray) -> np.ndarray:
    """the batch's index vector in (chromosome, start) order, stable (an unknown chromosome, 0xFFFFFFFF, comes last)"""
    return idx[np.lexsort((pool[1][idx], pool[0][idx]))]


def queries_of(pool, idx: np.ndarray):
    """-> (chrom, start, end) u32 of the batch"""
    return tuple(np.ascontiguousarray(pool[j][idx]).astype(np.uint32) for j in range(3))


def first_at_or_past(off: np.ndarray, value: int) -> int:
    """the first query whose offset is >= value (len(off) when there is none)"""
    return int(np.searchsorted(off, value, side="left"))


def max_tile_total(off: np.ndarray, tile: int) -> int:
    """the largest hit total of `tile` consecutive queries that start at a multiple of `tile`"""
    b = np.arange(0, len(off) - 1, tile)
    return int((off[np.minimum(b + tile, len(off) - 1)] - off[b]).max())


# ---- K15: the [unk] rule and max_length over sets of queries (tokenizer.rs: an empty result is [unk]; truncation to max_length)

def set_lengths(off: np.ndarray, set_off, max_length: int) -> Tuple[list, int, int]:
    """-> (out_offsets, total, longest) as Python ints for sets [set_off[b], set_off[b + 1]) of queries"""
    out, longest = [0], 0
    for lo, hi in zip(set_off[:-1], set_off[1:]):
        n = int(off[hi]) - int(off[lo])
        n = 1 if n == 0 else n
        if max_length and n > max_length:
            n = max_length
        longest = max(longest, n)
        out.append(out[-1] + n)
    return out, out[-1], longest


def deal_files(n_u: int, weights=(1, 2, 4)) -> np.ndarray:
    """the stack's records dealt to len(weights) files in the proportion of `weights`, cyclically"""
    pattern = np.repeat(np.arange(len(weights)), weights)
    return pattern[np.arange(n_u) % len(pattern)].astype(np.int64)


# ---- the shapes of tests/test_gpu_wide_totals.py (their properties are asserted on the CPU by tests/test_wide_totals_ref_cpu.py)

N_U = 70_000       # (a), (c), (d): the stack
NQ_A = 140_000     # (a), (c): the batch
HIGH_BASE = 3_000_000_000
NEST = 16          # (a), nested AIList: every 16th interval contains its followers
DENSE = (524_288, 1_048_576, 1_048_577, 2_097_152)  # (b)
DENSE_LENGTH = 4_194_304   # (b): the stack's intervals are longer than the stack is deep, so that they keep a common part
DENSE_REFUSED = 4_194_304  # (b): a stack no tile of any kernel can count in 32 bits (1024 queries x 2^22)
DENSE_REFUSED_LENGTH = 8_388_608
NQ_D = 320_000     # (d): the batch of (a) at a length at which two sets of it have a file total past 2^32 each (count_sets)
NQ_D_ONE = 220_000  # (d): its first queries, as many as put the largest file's total past 2^32 (count_device)
SETS_D = (0, 150_000, 151_000, 301_000, NQ_D)  # (d): count_sets


def heavy_tile(dense: int) -> int:
    """the fewest full queries whose hits reach 2^32: 8192, 4096, 4096, 2048 for DENSE"""
    return -(-TWO32 // dense)


_cache: dict = {}


def case_a(base: int = 0, nest: int = 0):
    """-> (pool, counts int64[len(pool)], idx): the stack of N_U, its pool and the batch of NQ_A"""
    key = ("a", base, nest)
    if key not in _cache:
        pool = query_pool(N_U, base)
        counts = pool_counts(universe(N_U, base, nest=nest), pool)[:, 0]
        _cache[key] = (pool, counts, mixed_batch(pool[3], NQ_A))
    return _cache[key]


def case_b(dense: int):
    """-> (pool, counts, idx): a stack of `dense`, a batch of heavy_tile(dense) full queries and three times as many mixed ones"""
    key = ("b", dense)
    if key not in _cache:
        pool = query_pool(dense, n_prefix=24, length=DENSE_LENGTH)
        counts = pool_counts(universe(dense, length=DENSE_LENGTH), pool)[:, 0]
        t = heavy_tile(dense)
        _cache[key] = (pool, counts, heavy_first_batch(pool[3], t, 3 * t))
    return _cache[key]


def light_tail(kind: np.ndarray, counts: np.ndarray, n: int, seed: int = 21) -> np.ndarray:
    """n queries that are cheap to count -- the other kinds, one prefix query of at most 64 hits in 16 -- for a long batch behind
    a heavy tile"""
    rng = np.random.default_rng(seed)
    rest = np.flatnonzero(kind == 2)
    small = np.flatnonzero((kind == 1) & (counts <= 64))
    assert len(small)
    return np.where(rng.random(n) < 1 / 16, small[rng.integers(0, len(small), n)], rest[rng.integers(0, len(rest), n)])


def sets_c(counts: np.ndarray, idx: np.ndarray):
    """(c): the batch of (a) cut into sets -> (set_off with a set longer than 2^32, set_off without one)"""
    empty = np.flatnonzero(counts[idx] == 0)
    p0 = int(empty[empty < 100][0])                 # a query without hits in front of the long set
    p1 = int(empty[empty > 100_000][0])             # and one behind it
    long_sets = [0, p0, p0 + 1, 100, 100, 100_000, p1, p1 + 1, p1 + 1, len(idx) - 1, len(idx)]
    short_sets = list(range(0, len(idx) + 1, 10_000))
    return long_sets, short_sets


def case_d():
    """-> (universe, file per record, pool, counts int64[len(pool), 4] per min_overlap in {1, 10}, idx): the stack of N_U dealt
    1 : 2 : 4 to three files, the extras (chromosomes 1 and 2) as a fourth; the batch of (a) at NQ_D queries"""
    if "d" not in _cache:
        uni = universe(N_U)
        files = np.concatenate([deal_files(N_U), np.full(len(uni[0]) - N_U, 3, dtype=np.int64)])
        pool = query_pool(N_U)
        counts = {mo: pool_counts(uni, pool, mo, files, 4) for mo in (1, 10)}
        _cache["d"] = (uni, files, pool, counts, mixed_batch(pool[3], NQ_D))
    return _cache["d"]


def lola_cells(user_hits, universe_hits, user_size: int, universe_size: int):
    """enrichment.rs:214-220 in Python ints: a = user hits, b = universe hits - a, c = user size - a, d = universe size - a - b - c"""
    a = [int(x) for x in user_hits]
    b = [int(v) - x for v, x in zip(universe_hits, a)]
    c = [user_size - x for x in a]
    d = [universe_size - x - y - z for x, y, z in zip(a, b, c)]
    return a, b, c, d
