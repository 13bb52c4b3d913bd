"""The overlap family by its definitions, in numpy -- what Bits / AIList answer, not how they search.

Written from the semantics of the reference (gtars-core/src/models/interval.rs, gtars-overlaprs/src/bits.rs, ailist.rs,
multi_chrom_overlapper.rs, indexed_region_set.rs), independently of ``oracle/gtars_oracle.c`` and of the HIP kernels: this module
imports neither.  All inputs are u32 arrays; every comparison is made on values widened to int64, so nothing wraps.

* Hit set (interval.rs:48-50): interval i hits query q iff ``s_i < qe_q and e_i > qs_q`` on the same chromosome.  The model
  builds that boolean matrix, in blocks of queries -- no search, no ``max_len``, no early exit.  The lower bound and the break
  of Bits (bits.rs:141-156, 433-446) and the ``max_ends`` exit of AIList (ailist.rs:238-263) only skip intervals that the
  predicate rejects anyway, so they do not change the set: the model is the statement of that fact.
* Bits (bits.rs:105, interval.rs:24-30): stored order = stable sort by (start, end), ties in input order; ``max_len`` = the
  largest ``end - start`` over intervals with ``end >= start``, 0 for the others (bits.rs:110-119); find order = stored order.
* AIList (ailist.rs:105-151, 198-236), per chromosome, in rounds: stable sort by start only; in one round an interval moves to
  the next round iff at least 10 of the next up-to-19 intervals of that round's list have an end strictly smaller than its own;
  the intervals that stay form a sub-list in that order; ``headers`` are the sub-lists' start offsets.  Find order: the
  sub-lists in order, each one from its last hit to its first (ailist.rs:153-178, 247-262).
* Derived calls (multi_chrom_overlapper.rs:483-563, indexed_region_set.rs:201-263): masks and reductions over the same matrix;
  a hit is kept iff ``min_bp <= 1 or min(qe, e) - max(qs, s) >= min_bp`` (i64; ``None`` is 0).
* A chromosome id >= n_chrom (0xFFFFFFFF: unknown) has no hits, as a query and as an index row.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

KIND_BITS = 0
KIND_AILIST = 1

AILIST_WINDOW = 19     # followers looked at: 1 .. 2 * minimum_coverage_length - 1 (ailist.rs:207)
AILIST_THRESHOLD = 10  # minimum_coverage_length (ailist.rs:129, 217)
QUERY_BLOCK = 2048     # rows of the hit matrix built at a time


def _i64(a) -> np.ndarray:
    a = np.asarray(a)
    if a.size and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
        raise ValueError("coordinates and ids are u32 values")
    return np.ascontiguousarray(a, dtype=np.int64)


def ailist_round(ends: np.ndarray) -> np.ndarray:
    """One decomposition round over a list's ends (int64): True where the interval moves on to the next round.  Shifted-array
    form: follower k of position i is position i + k; positions past the list's end count for nothing."""
    m = len(ends)
    padded = np.concatenate([ends, np.full(AILIST_WINDOW, np.iinfo(np.int64).max, dtype=np.int64)])
    smaller = np.zeros(m, dtype=np.int64)
    for k in range(1, AILIST_WINDOW + 1):
        smaller += ends > padded[k:k + m]
    return smaller >= AILIST_THRESHOLD


def ailist_layout(starts: np.ndarray, ends: np.ndarray) -> Tuple[np.ndarray, List[int]]:
    """-> (stored order as positions into the given arrays, header_list) for one chromosome's intervals in input order"""
    cur = np.argsort(starts, kind="stable")
    stored, headers, filled = [], [0], 0
    while True:
        moves = ailist_round(ends[cur])
        stored.append(cur[~moves])
        filled += int((~moves).sum())
        cur = cur[moves]
        if len(cur) == 0:
            break
        headers.append(filled)
    return np.concatenate(stored), headers


class Hits:
    """The hit matrix of one query batch in sparse form: ``q[k]`` hits the interval at find position ``pos[k]``, rows ascending
    by query, each query's hits in find order.  Every derived call is a mask or a reduction over these pairs."""

    def __init__(self, model: "Model", qc, qs, qe, q, pos):
        self.m, self.nq = model, len(qc)
        self.qc, self.qs, self.qe = qc, qs, qe
        self.q, self.pos = q, pos
        self._bp = None

    def _keep(self, min_overlap: Optional[int]):
        """min_bp <= 1 || overlap_bp >= min_bp, min_overlap.unwrap_or(0)"""
        min_bp = 0 if min_overlap is None else int(min_overlap)
        if min_bp <= 1:
            return slice(None)
        if self._bp is None:
            m = self.m
            self._bp = np.minimum(self.qe[self.q], m.f_end[self.pos]) - np.maximum(self.qs[self.q], m.f_start[self.pos])
        return self._bp >= min_bp

    def _offsets(self, q) -> np.ndarray:
        off = np.zeros(self.nq + 1, dtype=np.uint64)
        np.cumsum(np.bincount(q, minlength=self.nq), out=off[1:])
        return off

    def tokenize(self) -> Tuple[np.ndarray, np.ndarray]:
        """-> (CSR offsets u64[nq + 1], vals u32 in find order)"""
        return self._offsets(self.q), self.m.f_val[self.pos].astype(np.uint32)

    def count_overlaps(self, min_overlap: Optional[int] = None) -> np.ndarray:
        return np.bincount(self.q[self._keep(min_overlap)], minlength=self.nq).astype(np.uint64)

    def any_overlaps(self, min_overlap: Optional[int] = None) -> np.ndarray:
        return self.count_overlaps(min_overlap) > 0

    def find_overlaps(self, min_overlap: Optional[int] = None):
        """-> (offsets u64[nq + 1], starts, ends, vals) of the kept hits, in find order"""
        k = self._keep(min_overlap)
        p, m = self.pos[k], self.m
        return (self._offsets(self.q[k]), m.f_start[p].astype(np.uint32), m.f_end[p].astype(np.uint32),
                m.f_val[p].astype(np.uint32))

    def find_overlap_indices(self, min_overlap: Optional[int] = None, val=None):
        """IndexedRegionSet::find_overlaps: per query the kept hits' vals, ascending and unique.  (The reference collects every
        source row that shares a hit's coordinates: such a row is a hit itself, so with val = source row this is the same
        set.)  ``val``: a value per INPUT row to use instead of the index's own."""
        k = self._keep(min_overlap)
        pairs = np.unique((self.q[k].astype(np.int64) << 32) | self._vals(val)[self.pos[k]])  # sorted by (query, val), unique
        return self._offsets(pairs >> 32), (pairs & 0xFFFFFFFF).astype(np.uint32)

    def subset_by_overlaps(self, min_overlap: Optional[int] = None):
        """MultiChromOverlapper::subset_by_overlaps: unique (chrom, start, end) of the kept hits, sorted"""
        p, m = np.unique(self.pos[self._keep(min_overlap)]), self.m
        rows = np.unique(np.stack([m.f_chrom[p], m.f_start[p], m.f_end[p]], axis=1), axis=0).reshape(-1, 3)
        return rows[:, 0].astype(np.uint32), rows[:, 1].astype(np.uint32), rows[:, 2].astype(np.uint32)

    def subset_source_indices(self, min_overlap: Optional[int] = None, val=None) -> np.ndarray:
        """IndexedRegionSet::subset_by_overlaps / intersect_all: the kept hits' vals, ascending and unique"""
        return np.unique(self._vals(val)[self.pos[self._keep(min_overlap)]]).astype(np.uint32)

    def _vals(self, val):
        return self.m.f_val if val is None else _i64(val)[self.m.f_row]


class Model:
    """Per-chromosome Bits / AIList collection over integer chromosome ids, as definitions."""

    def __init__(self, chrom, start, end, val=None, n_chrom: Optional[int] = None, kind: int = KIND_BITS):
        chrom, start, end = _i64(chrom), _i64(start), _i64(end)
        n = len(chrom)
        val = np.arange(n, dtype=np.int64) if val is None else _i64(val)
        if n_chrom is None:
            n_chrom = int(chrom.max()) + 1 if n else 0
        self.n_chrom, self.kind = int(n_chrom), kind
        rows = np.flatnonzero(chrom < self.n_chrom)  # (input order)
        self._headers: List[List[int]] = [[] for _ in range(self.n_chrom)]
        stored, find = [], []
        self.chrom_off = np.zeros(self.n_chrom + 1, dtype=np.int64)
        for c in range(self.n_chrom):
            r = rows[chrom[rows] == c]
            if kind == KIND_BITS:
                st = r[np.lexsort((end[r], start[r]))]  # stable: ties keep the input order
                fi = st
            else:
                if len(r):
                    order, self._headers[c] = ailist_layout(start[r], end[r])
                    st = r[order]
                    bounds = self._headers[c] + [len(r)]
                    fi = np.concatenate([st[a:b][::-1] for a, b in zip(bounds[:-1], bounds[1:])])
                else:
                    st = fi = r
            stored.append(st)
            find.append(fi)
            self.chrom_off[c + 1] = self.chrom_off[c] + len(r)
        cat = lambda xs: np.concatenate(xs) if xs else np.zeros(0, dtype=np.int64)
        self._stored_row = cat(stored)
        self._chrom, self._start, self._end, self._val = chrom, start, end, val
        self.f_row = cat(find)  # input row at every find position
        self.f_chrom, self.f_start, self.f_end, self.f_val = chrom[self.f_row], start[self.f_row], end[self.f_row], val[self.f_row]

    def chrom_len(self, c: int) -> int:
        return int(self.chrom_off[c + 1] - self.chrom_off[c]) if c < self.n_chrom else 0

    def stored(self, c: int):
        """-> (starts, ends, vals) u32 of chromosome c in stored order"""
        r = self._stored_row[self.chrom_off[c]:self.chrom_off[c + 1]]
        return tuple(a[r].astype(np.uint32) for a in (self._start, self._end, self._val))

    def max_len(self, c: int) -> int:
        """Bits only (0 for AIList, as the introspection calls of both implementations give)"""
        if self.kind != KIND_BITS or self.chrom_len(c) == 0:
            return 0
        r = self._stored_row[self.chrom_off[c]:self.chrom_off[c + 1]]
        return int(np.where(self._end[r] >= self._start[r], self._end[r] - self._start[r], 0).max())

    def headers(self, c: int) -> List[int]:
        """AIList header_list of chromosome c.  For a chromosome without intervals, and for Bits, this is [] -- the convention
        of the two implementations' introspection calls (a chromosome without intervals has no AIList at all in the
        reference's map; AIList::build of an empty list would give [0], ailist.rs:126), not a definition."""
        return list(self._headers[c]) if self.kind == KIND_AILIST else []

    def query(self, qc, qs, qe) -> Hits:
        qc, qs, qe = _i64(qc), _i64(qs), _i64(qe)
        nq = len(qc)
        Q, P = [], []
        for b0 in range(0, nq, QUERY_BLOCK):
            bc = qc[b0:b0 + QUERY_BLOCK]
            bq, bp = [], []
            for c in np.unique(bc):
                if c >= self.n_chrom or self.chrom_len(int(c)) == 0:
                    continue
                lo, hi = self.chrom_off[c], self.chrom_off[c + 1]
                rows = b0 + np.flatnonzero(bc == c)
                hit = (self.f_start[None, lo:hi] < qe[rows, None]) & (self.f_end[None, lo:hi] > qs[rows, None])
                r, j = np.nonzero(hit)  # row-major: per query, ascending find position
                bq.append((rows[r]).astype(np.int32))
                bp.append((lo + j).astype(np.int32))
            if bq:
                bq, bp = np.concatenate(bq), np.concatenate(bp)
                o = np.argsort(bq, kind="stable")
                Q.append(bq[o])
                P.append(bp[o])
        z = np.zeros(0, dtype=np.int32)
        return Hits(self, qc, qs, qe, np.concatenate(Q) if Q else z, np.concatenate(P) if P else z)
