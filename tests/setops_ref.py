"""Plain-Python restatement of the region-set algebra contracts (gtars.models.RegionSet set operations and
RegionSetList.pairwise_jaccard), written from the behaviour as specified, for the tests of csrc/setops.hip.

Regions are ``(chr, start, end)`` tuples of ``str, int, int`` with 0 <= start, end < 2^32.  Chromosome names order
bytewise (``"chr10" < "chr2"``).  Widths and bp totals are u32 values as a release build computes them:
``(end - start) mod 2^32``, summed modulo 2^32.
"""
from __future__ import annotations

from bisect import bisect_left
from typing import Dict, List, Sequence, Tuple

M32 = 0xFFFFFFFF
Reg = Tuple[str, int, int]


def _name(c: str) -> bytes:
    return c.encode("utf-8")


def width(r: Reg) -> int:
    return (r[2] - r[1]) & M32


def nucleotides_length(regs: Sequence[Reg]) -> int:
    return sum(width(r) for r in regs) & M32


def reduce(regs: Sequence[Reg]) -> List[Reg]:
    """stable sort by (name, start) -- not by end -- then merge while next.start <= current.end"""
    if not regs:
        return []
    srt = sorted(regs, key=lambda r: (_name(r[0]), r[1]))
    out: List[Reg] = []
    c, s, e = srt[0]
    for rc, rs, re_ in srt[1:]:
        if rc == c and rs <= e:
            e = max(e, re_)
        else:
            out.append((c, s, e))
            c, s, e = rc, rs, re_
    out.append((c, s, e))
    return out


def union(a: Sequence[Reg], b: Sequence[Reg]) -> List[Reg]:
    return reduce(list(a) + list(b))


def _group(regs: Sequence[Reg]) -> Dict[str, List[Reg]]:
    g: Dict[str, List[Reg]] = {}
    for r in regs:
        g.setdefault(r[0], []).append(r)
    return g


def _runs(regs: Sequence[Reg]):
    """consecutive runs of one chromosome, in order"""
    i = 0
    while i < len(regs):
        j = i
        while j < len(regs) and regs[j][0] == regs[i][0]:
            j += 1
        yield regs[i][0], regs[i:j]
        i = j


def _setdiff_chr(c: str, a: Sequence[Reg], b: Sequence[Reg]) -> List[Reg]:
    out: List[Reg] = []
    bi = 0
    for _, s, e in a:
        while bi < len(b) and b[bi][2] <= s:
            bi += 1
        pos, j = s, bi
        while j < len(b) and b[j][1] < e and pos < e:
            if b[j][1] > pos:
                out.append((c, pos, b[j][1]))
            pos = max(pos, b[j][2])
            j += 1
        if pos < e:
            out.append((c, pos, e))
    return out


def _intersect_chr(c: str, a: Sequence[Reg], b: Sequence[Reg]) -> List[Reg]:
    out: List[Reg] = []
    bi = 0
    for _, s, e in a:
        while bi < len(b) and b[bi][2] <= s:
            bi += 1
        j = bi
        while j < len(b) and b[j][1] < e:
            ps, pe = max(s, b[j][1]), min(e, b[j][2])
            if ps < pe:
                out.append((c, ps, pe))
            j += 1
    return out


def setdiff(a: Sequence[Reg], b: Sequence[Reg]) -> List[Reg]:
    ra, bb = reduce(a), _group(reduce(b))
    out: List[Reg] = []
    for c, run in _runs(ra):
        out += _setdiff_chr(c, run, bb.get(c, []))
    return out


def intersect(a: Sequence[Reg], b: Sequence[Reg]) -> List[Reg]:
    ra, bb = reduce(a), _group(reduce(b))
    out: List[Reg] = []
    for c, run in _runs(ra):
        if c in bb:
            out += _intersect_chr(c, run, bb[c])
    return out


def jaccard(a: Sequence[Reg], b: Sequence[Reg]) -> float:
    a_bp, b_bp = nucleotides_length(reduce(a)), nucleotides_length(reduce(b))
    u = nucleotides_length(union(a, b))
    if u == 0:
        return 0.0
    return ((a_bp + b_bp - u) & M32) / u


def coverage(a: Sequence[Reg], b: Sequence[Reg]) -> float:
    ra = reduce(a)
    self_bp = nucleotides_length(ra)
    if self_bp == 0:
        return 0.0
    return 1.0 - (nucleotides_length(setdiff(ra, b)) / self_bp)


def overlap_coefficient(a: Sequence[Reg], b: Sequence[Reg]) -> float:
    a_bp, b_bp = nucleotides_length(reduce(a)), nucleotides_length(reduce(b))
    m = min(a_bp, b_bp)
    if m == 0:
        return 0.0
    u = nucleotides_length(union(a, b))
    return ((a_bp + b_bp - u) & M32) / m


def _gap(a: Reg, b: Reg) -> int:
    if a[1] < b[2] and b[1] < a[2]:
        return 0
    if b[2] <= a[1]:
        return a[1] - b[2]
    return b[1] - a[2]


def closest(a: Sequence[Reg], other: Sequence[Reg]) -> List[Tuple[int, int, int]]:
    """the interleaved walk (right, then left, per step) from the insertion point; the insertion point is the
    FIRST candidate whose start equals the query's start (lower bound) -- the one rule this library fixes where
    the reference leaves the index unspecified"""
    if not other:
        return []
    by: Dict[str, List[Tuple[int, Reg]]] = {}
    for i, r in enumerate(other):
        by.setdefault(r[0], []).append((i, r))
    starts, maxw = {}, {}
    for c, v in by.items():
        v.sort(key=lambda t: t[1][1])
        starts[c] = [r[1] for _, r in v]
        maxw[c] = max(width(r) for _, r in v)
    out = []
    for qi, q in enumerate(a):
        cand = by.get(q[0])
        if cand is None:
            continue
        n = len(cand)
        ins = bisect_left(starts[q[0]], q[1])
        mw = maxw[q[0]]
        best_i, best = 0, None
        left_done, right_done = ins == 0, ins >= n
        li, ri = (ins - 1 if ins > 0 else 0), ins
        while not left_done or not right_done:
            if not right_done:
                oi, b = cand[ri]
                d = _gap(q, b)
                if best is None or abs(d) < abs(best):
                    best, best_i = d, oi
                if best == 0:
                    break
                ri += 1
                if ri >= n or b[1] - q[2] > abs(best):
                    right_done = True
            if not left_done:
                oi, b = cand[li]
                d = _gap(q, b)
                if best is None or abs(d) < abs(best):
                    best, best_i = d, oi
                if best == 0:
                    break
                if li == 0 or q[1] - b[1] > abs(best) + mw:
                    left_done = True
                else:
                    li -= 1
        out.append((qi, best_i, best))
    return out


def cluster(regs: Sequence[Reg], max_gap: int = 0) -> List[int]:
    n = len(regs)
    if n == 0:
        return []
    order = sorted(range(n), key=lambda i: (_name(regs[i][0]), regs[i][1], regs[i][2]))
    res = [0] * n
    cid = 0
    c, cend = regs[order[0]][0], regs[order[0]][2]
    for i in order[1:]:
        r = regs[i]
        if r[0] != c or r[1] > min(cend + max_gap, M32):
            cid += 1
            c, cend = r[0], r[2]
        else:
            cend = max(cend, r[2])
        res[i] = cid
    return res


def pairwise_jaccard(sets: Sequence[Sequence[Reg]]) -> List[List[float]]:
    red = [reduce(s) for s in sets]
    n = len(sets)
    return [[1.0 if i == j else jaccard(red[i], red[j]) for j in range(n)] for i in range(n)]
