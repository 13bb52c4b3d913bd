"""Plain-Python restatement of the folds and indexed pair calls over a list of region sets
(gtars.models.RegionSetList: union_all / intersect_all / union_except / bulk_union_except, pintersect_at / pintersect_count /
jaccard_at / union_at / setdiff_at / region_count), for the tests of csrc/setops.hip.

Every function is a fold over tests/setops_ref.py (``reduce``, ``union``, ``intersect``, ``setdiff``, ``jaccard``) in the
order the contract states it: the accumulator starts as a copy of one set *as it is* (rows in their order, unmerged) and
is only ever replaced by a ``union`` / ``intersect`` with the next set, so a list of one set -- and ``union_except`` on a
list of two -- returns that copy.  ``bulk_union_except`` builds the prefix unions, the suffix unions and one union per
inner index, as the contract describes it.  A set is a list of ``(chr, start, end)`` tuples; "no answer" is ``None``.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import setops_ref as R

Reg = R.Reg
Set = Sequence[Reg]


def _get(sets: Sequence[Set], i: int) -> Optional[List[Reg]]:
    """an index below 0 or past the end has no set (the contract's indices are unsigned)"""
    return list(sets[i]) if 0 <= i < len(sets) else None


def pintersect(a: Set, b: Set) -> List[Reg]:
    """pairwise by position over the shorter length: [max start, min end), empty at max start when the two do not
    overlap, empty at a's start when the chromosomes differ"""
    out: List[Reg] = []
    for (ac, a_s, a_e), (bc, b_s, b_e) in zip(a, b):
        if ac != bc:
            out.append((ac, a_s, a_s))
            continue
        s, e = max(a_s, b_s), min(a_e, b_e)
        out.append((ac, s, s if s >= e else e))
    return out


def pintersect_at(sets: Sequence[Set], i: int, j: int) -> Optional[List[Reg]]:
    a, b = _get(sets, i), _get(sets, j)
    return None if a is None or b is None else pintersect(a, b)


def pintersect_count(sets: Sequence[Set], i: int, j: int) -> Optional[int]:
    r = pintersect_at(sets, i, j)
    return None if r is None else len(r)


def jaccard_at(sets: Sequence[Set], i: int, j: int) -> Optional[float]:
    a, b = _get(sets, i), _get(sets, j)
    return None if a is None or b is None else R.jaccard(a, b)


def union_at(sets: Sequence[Set], i: int, j: int) -> Optional[List[Reg]]:
    a, b = _get(sets, i), _get(sets, j)
    return None if a is None or b is None else R.union(a, b)


def setdiff_at(sets: Sequence[Set], i: int, j: int) -> Optional[List[Reg]]:
    a, b = _get(sets, i), _get(sets, j)
    return None if a is None or b is None else R.setdiff(a, b)


def region_count(sets: Sequence[Set], i: int) -> Optional[int]:
    a = _get(sets, i)
    return None if a is None else len(a)


def union_except(sets: Sequence[Set], skip: int) -> Optional[List[Reg]]:
    n = len(sets)
    if n < 2 or not 0 <= skip < n:
        return None
    first = 1 if skip == 0 else 0
    acc = list(sets[first])
    for k in range(first + 1, n):
        if k == skip:
            continue
        acc = R.union(acc, sets[k])
    return acc


def bulk_union_except(sets: Sequence[Set]) -> Optional[Tuple[List[Reg], List[List[Reg]]]]:
    n = len(sets)
    if n < 2:
        return None
    # prefix[i] = union of sets 0..i
    prefix = [list(sets[0])]
    for i in range(1, n):
        prefix.append(R.union(prefix[i - 1], sets[i]))
    # suffix[i] = union of sets i..n-1, from the right
    suffix: List[Optional[List[Reg]]] = [None] * n
    suffix[n - 1] = list(sets[n - 1])
    for i in range(n - 2, -1, -1):
        suffix[i] = R.union(sets[i], suffix[i + 1])
    full = list(prefix[n - 1])
    results = []
    for i in range(n):
        if i == 0:
            results.append(list(suffix[1]))
        elif i == n - 1:
            results.append(list(prefix[i - 1]))
        else:
            results.append(R.union(prefix[i - 1], suffix[i + 1]))
    return full, results


def union_all(sets: Sequence[Set]) -> Optional[List[Reg]]:
    if not sets:
        return None
    acc = list(sets[0])
    for s in sets[1:]:
        acc = R.union(acc, s)
    return acc


def intersect_all(sets: Sequence[Set]) -> Optional[List[Reg]]:
    if not sets:
        return None
    acc = list(sets[0])
    for s in sets[1:]:
        acc = R.intersect(acc, s)
    return acc


# ------------------------------------------------------------------------------------- the device's closed forms
def union_except_closed(sets: Sequence[Set], skip: int) -> List[Reg]:
    """what the device computes for n >= 3: one reduce of the concatenation of every set but ``skip``"""
    return R.reduce([r for k, s in enumerate(sets) if k != skip for r in s])


def intersect_all_closed(sets: Sequence[Set]) -> List[Reg]:
    """what the device computes for n >= 2: each set reduced, the regions with start >= end dropped (they never yield a
    piece of a sweep), then the stretches between consecutive boundaries of a chromosome that all n sets cover"""
    n = len(sets)
    ev = {}
    for s in sets:
        for c, st, en in R.reduce(s):
            if st < en:
                ev.setdefault(c, []).append((st, 1))
                ev[c].append((en, -1))
    out: List[Reg] = []
    for c in sorted(ev, key=lambda x: x.encode("utf-8")):
        e = sorted(ev[c])
        depth = 0
        for j, (pos, d) in enumerate(e):
            depth += d
            if j + 1 < len(e) and e[j + 1][0] != pos and depth == n:
                out.append((c, pos, e[j + 1][0]))
    return out


# --------------------------------------------------------------------- the device's top-2-by-owner scan, row by row
def t2_merge(a, b):
    """the scan's operator on summaries (m1, s1, m2) of a span of (end, set) rows, None: no row yet.  m1: the largest
    end, s1: a set that attains it, m2: the largest end among the rows of every other set (None: no such row)."""
    if b is None:
        return a
    if a is None:
        return b
    if a[1] == b[1]:
        m2 = [x for x in (a[2], b[2]) if x is not None]
        return (max(a[0], b[0]), a[1], max(m2) if m2 else None)
    w, l = (b, a) if b[0] > a[0] else (a, b)
    return (w[0], w[1], l[0] if w[2] is None else max(w[2], l[0]))


def bulk_union_except_top2(sets: Sequence[Set]) -> Tuple[List[Reg], List[List[Reg]]]:
    """(reduce of all, [reduce without set i]) the way the device computes them: one stable sort of the concatenation by
    (name, start); per row the summary of the chromosome's earlier rows; row k opens a run of output i (i != its own set;
    i == n: the union of all) when the running maximum without set i -- m2 if s1 == i, else m1 -- is None or below its
    start; a run ends at its head's end when the head is inverted, else at that running maximum where the next run of
    the chromosome opens or the chromosome ends."""
    n = len(sets)
    rows = sorted(((c, s, e, k) for k, regs in enumerate(sets) for c, s, e in regs), key=lambda r: (r[0].encode("utf-8"), r[1]))
    out: List[List[list]] = [[] for _ in range(n + 1)]

    def without(state, i):
        if state is None:
            return None
        return state[2] if state[1] == i else state[0]

    def close(state, i):
        m = without(state, i)
        if m is not None and out[i] and out[i][-1][3]:
            c, s, e, _ = out[i][-1]
            out[i][-1] = [c, s, e if s > e else m, False]

    state = None
    for k, (c, s, e, own) in enumerate(rows):
        if k and rows[k - 1][0] != c:
            for i in range(n + 1):
                close(state, i)
            state = None
        for i in range(n + 1):
            m = without(state, i)
            if i != own and (m is None or s > m):
                close(state, i)
                out[i].append([c, s, e, True])
        state = t2_merge(state, (e, own, None))
    for i in range(n + 1):
        close(state, i)
    res = [[(c, s, e) for c, s, e, _ in o] for o in out]
    return res[n], res[:n]
