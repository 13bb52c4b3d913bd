"""``gtars.genomic_distributions`` mirror: the functions of gtars-python/src/genomic_distributions/tools.rs that need
nothing beyond region sets.

``consensus`` runs on the GPU (csrc/setops.hip, K9): one reduce over the concatenation of the sets, carrying each
region's set through the sort, and a count of the distinct sets whose regions hit each union region under the AIList
rule (start < u.end && u.start < end).  ``median_abs_distance`` is host arithmetic.  ``calc_gc_content`` /
``calc_dinucl_freq`` live in ``gtars.seqstats`` and ``calc_summary_signal`` in ``gtars.signal``; ``calc_partitions`` and
``calc_expected_partitions`` in ``gtars.partitions``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional, Sequence

from ._lib import check, lib
from .models import RegionSet, _take

_I64_MAX = (1 << 63) - 1


def consensus(region_sets: Sequence[RegionSet]) -> List[dict]:
    """union of the sets (reduce of their concatenation) with, per union region, the number of sets overlapping it:
    dicts {chr, start, end, count} in union order (gtars-genomicdist/src/consensus.rs:29-68)"""
    sets = list(region_sets)
    if not sets:
        return []
    handles = (C.c_void_p * len(sets))(*[s._h for s in sets])
    h, p = C.c_void_p(), C.c_void_p()
    check(lib.gtars_regionset_consensus(C.cast(handles, C.c_void_p), len(sets), C.byref(h), C.byref(p)))
    union = RegionSet._from_handle(h)
    count = _take(p, C.c_uint32, len(union))
    names, ids, s, e = union.chrom_names, union.chrom_ids.tolist(), union.starts.tolist(), union.ends.tolist()
    return [{"chr": names[ids[i]], "start": s[i], "end": e[i], "count": count[i]} for i in range(len(union))]


def median_abs_distance(distances: Sequence[float]) -> Optional[float]:
    """median of |trunc(d)| over the finite distances; None when none is left (tools.rs:157-168, utils.rs:40-56).
    Truncation saturates to i64 as a Rust cast does; a value that lands on i64::MAX is dropped as the reference drops it."""
    vals = []
    for d in distances:
        d = float(d)
        if math.isnan(d) or math.isinf(d):
            continue
        t = max(min(math.trunc(d), _I64_MAX), -(1 << 63))
        if t == _I64_MAX:
            continue
        vals.append(abs(float(t)))
    if not vals:
        return None
    vals.sort()
    n = len(vals)
    return (vals[n // 2 - 1] + vals[n // 2]) / 2.0 if n % 2 == 0 else vals[n // 2]
