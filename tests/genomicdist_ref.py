"""Plain-Python restatement of the structural operations and region-set statistics (RegionSet.disjoin / gaps / trim /
promoters / pintersect / concat / widths / mean_region_width / get_max_end_per_chr / neighbor_distances /
nearest_neighbors / distribution / chromosome_statistics, and gtars.genomic_distributions.consensus /
median_abs_distance), written from the behaviour as specified, for the tests of the K9 kernels in csrc/setops.hip.

Regions are ``(chr, start, end)`` tuples as in tests/setops_ref.py.  Chromosome names order bytewise.  Widths are
``(end - start) mod 2^32`` and u32 sums and additions wrap, as the reference's release build computes them.

Where the reference's own loop costs more than O(n log n) (disjoin tests every piece against every interval, consensus
queries every union region against every set, the neighbour statistics filter the whole set once per chromosome) there
are two forms: ``*_brute`` follows the reference's loops and is for small n, the plain name is the fast form used at GPU
sizes.  The tests check one against the other.  The remaining operations are single passes and have one form.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import setops_ref as S

M32 = 0xFFFFFFFF
I64_MAX = (1 << 63) - 1
Reg = Tuple[str, int, int]
_name = S._name
width = S.width


def _by_chr(regs: Sequence[Reg]) -> Dict[str, List[Tuple[int, int]]]:
    """chromosome -> its (start, end) in set order; dict order = first appearance (iter_chroms, region_set.rs:399-407)"""
    by: Dict[str, List[Tuple[int, int]]] = {}
    for c, s, e in regs:
        by.setdefault(c, []).append((s, e))
    return by


# ---------------------------------------------------------------------------------------------------------- disjoin
def disjoin_brute(regs: Sequence[Reg]) -> List[Reg]:
    """region_set.rs:1051-1090: boundaries = every start and end, deduplicated; piece [b_k, b_k+1) kept when some
    interval has start <= b_k and b_k+1 <= end; result sorted by (chr, start)"""
    out: List[Reg] = []
    for c, iv in _by_chr(regs).items():
        b = sorted({x for s, e in iv for x in (s, e)})
        for k in range(len(b) - 1):
            if any(s <= b[k] and b[k + 1] <= e for s, e in iv):
                out.append((c, b[k], b[k + 1]))
    out.sort(key=lambda r: (_name(r[0]), r[1]))
    return out


def disjoin(regs: Sequence[Reg]) -> List[Reg]:
    """the same pieces from a sweep: +1 / -1 depth from the well-formed intervals (start < end) only; inverted and
    zero-width intervals add a boundary and no depth; a piece is kept where the depth after its left boundary is > 0"""
    out: List[Reg] = []
    by = _by_chr(regs)
    for c in sorted(by, key=_name):
        ev: Dict[int, int] = {}
        for s, e in by[c]:
            d = 1 if s < e else 0
            ev[s] = ev.get(s, 0) + d
            ev[e] = ev.get(e, 0) - d
        pos = sorted(ev)
        depth = 0
        for k in range(len(pos) - 1):
            depth += ev[pos[k]]
            if depth > 0:
                out.append((c, pos[k], pos[k + 1]))
    return out


# ------------------------------------------------------------------------------------------------------------- gaps
def karyotype_key(chr_: str) -> Tuple[int, int, bytes]:
    """chrom_karyotype_key (gtars-core/src/utils.rs:359-370): "chr" stripped; u32 numbers (Rust's u32::from_str: an
    optional '+', then ASCII digits, no overflow) first, then X, Y, M / MT, then the rest by the bare name"""
    bare = chr_[3:] if chr_.startswith("chr") else chr_
    if bare == "X":
        return (1, 0, b"")
    if bare == "Y":
        return (2, 0, b"")
    if bare in ("M", "MT"):
        return (3, 0, b"")
    digits = bare[1:] if bare.startswith("+") else bare
    if digits and all("0" <= ch <= "9" for ch in digits) and int(digits) <= M32:
        return (0, int(digits), b"")
    return (4, 0, _name(bare))


def gaps(regs: Sequence[Reg], chrom_sizes: Dict[str, int]) -> List[Reg]:
    """region_set.rs:786-878 on reduce(regs).  The reference sorts by (karyotype key, start) and leaves names that share a
    key in hash-map order; this restatement pins (key, start, name bytewise)."""
    by: Dict[str, List[Reg]] = {}
    for r in S.reduce(regs):
        if r[0] in chrom_sizes:
            by.setdefault(r[0], []).append(r)
    out: List[Reg] = []
    for c, cs in chrom_sizes.items():
        if cs == 0:
            continue
        rr = by.get(c)
        if rr is None:
            out.append((c, 0, cs))
            continue
        if rr[0][1] > 0:
            out.append((c, 0, min(rr[0][1], cs)))
        for p, q in zip(rr, rr[1:]):
            gs, ge = p[2], q[1]
            if gs < ge and min(gs, cs) < min(ge, cs):
                out.append((c, min(gs, cs), min(ge, cs)))
        if rr[-1][2] < cs:
            out.append((c, rr[-1][2], cs))
    out.sort(key=lambda r: (karyotype_key(r[0]), r[1], _name(r[0])))
    return out


# -------------------------------------------------------------------------------------------------------- consensus
def consensus_brute(sets: Sequence[Sequence[Reg]]) -> List[Tuple[str, int, int, int]]:
    """gtars-genomicdist/src/consensus.rs:29-68: union = reduce(concat); count = the sets with any region that the
    AIList reports for the union region: same chromosome, start < u.end and u.start < end"""
    if not sets:
        return []
    union = S.reduce([r for s in sets for r in s])
    return [(c, us, ue, sum(1 for s in sets if any(r[0] == c and r[1] < ue and us < r[2] for r in s)))
            for c, us, ue in union]


def consensus(sets: Sequence[Sequence[Reg]]) -> List[Tuple[str, int, int, int]]:
    """one reduce over the concatenation carrying each region's set; a region is tested against its own run only.  No
    region can hit another run: a run opens at a start greater than every end of the runs before it, so an earlier
    region ends before a later run starts, and a later region starts after an earlier run ends."""
    if not sets:
        return []
    rows = sorted(((r[0], r[1], r[2], k) for k, s in enumerate(sets) for r in s), key=lambda t: (_name(t[0]), t[1]))
    runs: List[list] = []
    for c, s, e, k in rows:
        if runs and runs[-1][0] == c and s <= runs[-1][2]:
            runs[-1][2] = max(runs[-1][2], e)
            runs[-1][3].append((s, e, k))
        else:
            runs.append([c, s, e, [(s, e, k)]])
    return [(c, s, e, len({k for rs, re_, k in m if rs < e and s < re_})) for c, s, e, m in runs]


# ------------------------------------------------------------------------------------------------------ neighbours
def _sorted_chroms_brute(regs: Sequence[Reg]):
    seen: List[str] = []
    for r in regs:
        if r[0] not in seen:
            seen.append(r[0])
    for c in seen:
        yield sorted((r for r in regs if r[0] == c), key=lambda r: (r[1], r[2]))


def _sorted_chroms(regs: Sequence[Reg]):
    for c, iv in _by_chr(regs).items():
        yield [(c, s, e) for s, e in sorted(iv)]


def _neighbor_distances(chroms) -> List[int]:
    out: List[int] = []
    for rr in chroms:
        for p, q in zip(rr, rr[1:]):
            d = q[1] - p[2]
            if d > 0:
                out.append(d)
    return out


def _nearest_neighbors(chroms) -> List[int]:
    out: List[int] = []
    for rr in chroms:
        if len(rr) < 2:
            continue
        d = [max(q[1] - p[2], 0) for p, q in zip(rr, rr[1:])]
        out.append(d[0])
        out += [min(x, y) for x, y in zip(d, d[1:])]
        out.append(d[-1])
    return out


def neighbor_distances_brute(regs: Sequence[Reg]) -> List[int]:
    """statistics.rs:258-285: per chromosome in first-appearance order, regions sorted by (start, end), every
    next.start - prev.end > 0"""
    return _neighbor_distances(_sorted_chroms_brute(regs))


def neighbor_distances(regs: Sequence[Reg]) -> List[int]:
    return _neighbor_distances(_sorted_chroms(regs))


def nearest_neighbors_brute(regs: Sequence[Reg]) -> List[int]:
    """statistics.rs:287-316: gaps clamped at 0; the first and last region take their one neighbour's, the others the
    smaller of two; chromosomes with one region skipped"""
    return _nearest_neighbors(_sorted_chroms_brute(regs))


def nearest_neighbors(regs: Sequence[Reg]) -> List[int]:
    return _nearest_neighbors(_sorted_chroms(regs))


# ---------------------------------------------------------------------------------------------------- distribution
def get_max_end_per_chr(regs: Sequence[Reg]) -> Dict[str, int]:
    """region_set.rs:584-606: per chromosome, the largest end of its LAST contiguous run in set order.  The reference
    indexes regions[0] and panics on an empty set; this restatement raises ValueError."""
    if not regs:
        raise ValueError("empty region set")
    out: Dict[str, int] = {}
    cur, m = regs[0][0], regs[0][2]
    for c, _, e in regs[1:]:
        if c == cur:
            m = max(m, e)
        else:
            out[cur] = m
            cur, m = c, e
    out[cur] = m
    return out


def mid_point(r: Reg) -> int:
    return (r[1] + width(r) // 2) & M32


def distribution(regs: Sequence[Reg], n_bins: int = 250, chrom_sizes: Optional[Dict[str, int]] = None) -> List[dict]:
    """statistics.rs:143-256 and the Python wrapper region_set.rs:322-349: regions counted per (chr, bin) of their
    midpoint, the bins as dicts {chr, start, end, n, rid} sorted by (chr, start).  bin_start + bin_size wraps in u32."""
    bins: Dict[Tuple[str, int], list] = {}
    if chrom_sizes is None:
        if not regs:
            return []
        ends = get_max_end_per_chr(regs)
        longest = max(ends.values())
        bin_size = max(longest, 1) if n_bins == 0 else max(longest // n_bins, 1)
        for r in regs:
            rid = mid_point(r) // bin_size
            start = rid * bin_size
            stop = min((start + bin_size) & M32, ends[r[0]])
            bins.setdefault((r[0], rid), [start, stop, 0])[2] += 1
    else:
        if not regs or n_bins == 0:
            return []
        longest = max(chrom_sizes.values()) if chrom_sizes else 1
        bin_size = max(longest // n_bins, 1)
        for r in regs:
            cs = chrom_sizes.get(r[0])
            if cs is None:
                continue
            mid = mid_point(r)
            if mid >= cs:
                continue
            rid = min(mid // bin_size, n_bins - 1)
            start = rid * bin_size
            stop = cs if rid == n_bins - 1 else min((start + bin_size) & M32, cs)
            bins.setdefault((r[0], rid), [start, stop, 0])[2] += 1
    keys = sorted(bins, key=lambda k: (_name(k[0]), bins[k][0]))
    return [{"chr": k[0], "start": bins[k][0], "end": bins[k][1], "n": bins[k][2], "rid": k[1]} for k in keys]


# ---------------------------------------------------------------------------------------------------- statistics
def chromosome_statistics(regs: Sequence[Reg]) -> Dict[str, tuple]:
    """statistics.rs:88-141: per chromosome (number_of_regions, start_nucleotide_position (min start),
    end_nucleotide_position (max end), minimum_region_length, maximum_region_length, mean_region_length (u64 sum /
    count), median_region_length).  An even count adds the two middle widths in wrapping u32 before the division."""
    w: Dict[str, List[int]] = {}
    bounds: Dict[str, List[int]] = {}
    for r in regs:
        w.setdefault(r[0], []).append(width(r))
        b = bounds.setdefault(r[0], [r[1], r[2]])
        b[0], b[1] = min(b[0], r[1]), max(b[1], r[2])
    out = {}
    for c, ws in w.items():
        ws.sort()
        n = len(ws)
        median = ((ws[n // 2 - 1] + ws[n // 2]) & M32) / 2.0 if n % 2 == 0 else float(ws[n // 2])
        out[c] = (n, bounds[c][0], bounds[c][1], ws[0], ws[-1], sum(ws) / n, median)
    return out


# -------------------------------------------------------------------------------------------- host-side operations
def widths(regs: Sequence[Reg]) -> List[int]:
    return [width(r) for r in regs]


def mean_region_width(regs: Sequence[Reg]) -> float:
    """region_set.rs:527-537: wrapping u32 sum / count, x 100, f64::round (half away from zero), / 100; nan when empty"""
    if not regs:
        return float("nan")
    v = (S.nucleotides_length(regs) / len(regs)) * 100.0
    r = math.floor(v)
    return (r + 1.0 if v - r >= 0.5 else float(r)) / 100.0


def trim(regs: Sequence[Reg], chrom_sizes: Dict[str, int]) -> List[Reg]:
    """region_set.rs:744-766: unsized chromosomes dropped, start and end clamped to the size, clamped start > end dropped"""
    out = []
    for c, s, e in regs:
        if c not in chrom_sizes:
            continue
        cs = chrom_sizes[c]
        s, e = min(s, cs), min(e, cs)
        if s <= e:
            out.append((c, s, e))
    return out


def promoters(regs: Sequence[Reg], upstream: int, downstream: int) -> List[Reg]:
    """region_set.rs:993-1005: [start - upstream, start + downstream), saturating in u32"""
    return [(c, max(s - upstream, 0), min(s + downstream, M32)) for c, s, _ in regs]


def pintersect(a: Sequence[Reg], b: Sequence[Reg]) -> List[Reg]:
    """region_set.rs:1008-1041: pairs up to the shorter length; [a.start, a.start) when the chromosomes differ,
    [max_start, max_start) when the pair does not overlap"""
    out = []
    for x, y in zip(a, b):
        if x[0] != y[0]:
            out.append((x[0], x[1], x[1]))
            continue
        s, e = max(x[1], y[1]), min(x[2], y[2])
        out.append((x[0], s, s) if s >= e else (x[0], s, e))
    return out


def median_abs_distance(distances: Sequence[float]) -> Optional[float]:
    """gtars-python/src/genomic_distributions/tools.rs:157-168 and gtars-genomicdist/src/utils.rs:40-56: NaN and +-inf
    become i64::MAX, other values truncate to i64 (saturating); i64::MAX is dropped; the median of |value| as f64"""
    vals = []
    for d in distances:
        d = float(d)
        t = I64_MAX if (math.isnan(d) or math.isinf(d)) else max(min(math.trunc(d), I64_MAX), -(1 << 63))
        if t != I64_MAX:
            vals.append(abs(float(t)))
    if not vals:
        return None
    vals.sort()
    n = len(vals)
    return (vals[n // 2 - 1] + vals[n // 2]) / 2.0 if n % 2 == 0 else vals[n // 2]
