#!/usr/bin/env python3
"""Randomised differential soak of K18 (csrc/vrs.hip): normalize_alleles and vrs_ids on random alleles over a random assembly
against vrs_ref.alleles -- statuses, starts, ends, normalized sequences and identifiers equal.

A case is an assembly of 2 to 5 chromosomes (at most about 20 kB, a random FASTA line width, loaded from the FASTA or from its
.fab image) and a batch of 0 to about 600 alleles.  The chromosomes are random bases with planted repeats of unit length 1 to 6
and runs of 2 to about 1500 bases -- some end in the middle of a unit, some are soft-masked, some stand flush against position 0
or the chromosome's length, some stop at an N -- N runs, a few IUPAC codes, a chromosome of length 1, and two neighbours in the
packed image that end and start with the same unit.  The alleles: SNVs, MNVs, delins, ref == alt, insertions of a run's unit, of
a rotation of it and of several units plus a partial one, deletions of k units, lower-case alleles, insertions at 0 and at the
chromosome's length, an N into a run of N, placed so that they roll cap - 1, cap, cap + 1, cap + 63, 64, 65, 128 and about 1000 bases for the case's
GTARS_VRS_ROLL_CAP; about one row in ten fails (REF mismatch, REF or start past the end, start + len overflow, unknown name).
GTARS_VRS_ROLL_CAP and GTARS_VRS_HOST_LEN are drawn per case; half of the cases also run on_host=True, some pass an accession
table that lacks a chromosome.

make_case(seed) and expected(case) need no device (tests/test_soak_generators_cpu.py runs them, and check(..., on_host=True));
run_device(case, tmp) does.

Run on the GPU box:  python tests/soak/fuzz_vrs.py [rounds] [first_seed]"""
import os, random, shutil, sys, tempfile, time
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
import vrs_ref as R

COUNTS = [0, 1, 63, 64, 65, 257, 600]
CAPS = [None, 1, 8, 63, 64, 65, 1 << 20]
HOST_LENS = [None, 0, 8, 1 << 20]
DEFAULT_CAP = 64
NEAR = (-1, 0, 1, 63, 64, 65, 128)   # roll distances next to the cap: cap - 1 .. cap + 128
FAILING = ("mismatch", "ref_past_end", "start_past_end", "overflow", "unknown")


def write_fasta(path, seqs, width):
    with open(path, "wb") as f:
        for name, s in seqs.items():
            f.write(b">" + name.encode() + b" fuzz\n")
            for k in range(0, len(s), width):
                f.write(s[k:k + width] + b"\n")


def _other(rng, base, *more):
    """an upper-case base that is none of the given ones (compared upper-cased)"""
    avoid = {b & 0xDF for b in (base,) + more}
    return rng.choice([b for b in b"ACGT" if b not in avoid])


def _unit(rng):
    u = rng.randint(1, 6)
    return bytes(rng.choice(b"ACGT") for _ in range(u))


def _plant(rng, seq, at, unit, length, soft, stop_left=None, stop_right=None):
    """`length` bases of the repeat of `unit` at `at`, between two bases it cannot roll through -> the run's record"""
    text = (unit * (length // len(unit) + 1))[:length]
    seq[at:at + length] = text.lower() if soft else text
    if at > 0:
        seq[at - 1] = stop_left or _other(rng, unit[-1])
    if at + length < len(seq):
        seq[at + length] = stop_right or _other(rng, unit[length % len(unit)])
    return dict(at=at, length=length, unit=unit, soft=soft)


def make_assembly(rng, cap):
    """{name: bytes} in file order, and the planted runs per chromosome"""
    n_main = rng.choice([3000, 6000, 9000])
    main = bytearray(rng.choice(b"ACGT") for _ in range(n_main))
    runs = {"main": []}
    lengths = [rng.choice([2, 3, 5, 17]), cap + 70 + rng.randrange(7), cap + 140 + rng.randrange(7), rng.choice([7, 40, cap + 131]),
               rng.choice([1100, 1300, 1500]) + rng.randrange(6)]
    rng.shuffle(lengths)
    at = 0 if rng.random() < 0.5 else rng.randint(1, 30)  # the first run may stand flush against position 0
    free = [0, n_main]  # the random stretch that no run uses
    for k, length in enumerate(lengths):
        if at + length + 2 > n_main:
            break
        free[0] = at
        if k == len(lengths) - 1 and rng.random() < 0.5:
            at = n_main - length  # ... and the last one against the chromosome's length
            free[1] = at - 1
        else:
            free[0] = at + length + 1
        runs["main"].append(_plant(rng, main, at, _unit(rng), length, rng.random() < 0.3,
                                   stop_left=ord("N") if rng.random() < 0.2 else None, stop_right=ord("N") if rng.random() < 0.2 else None))
        at += length + rng.randint(2, 60)
    for _ in range(3):  # N runs and IUPAC codes in the random stretch
        if free[1] - free[0] > 60:
            k = rng.choice([1, 8, 20])
            p = rng.randrange(free[0], free[1] - 30)
            main[p:p + k] = b"N" * k
            q = rng.randrange(free[0], free[1] - 30)
            main[q:q + 6] = rng.choice([b"RYKMSW", b"rykmBD", b"NnRAYC"])
    seqs = {"main": bytes(main)}
    if rng.random() < 0.75:  # two neighbours of the packed image that end and start with the same unit
        unit = _unit(rng)
        k1, k2 = rng.choice([4, 9, cap + 3]), rng.choice([4, 9, cap + 3])
        e1 = bytearray(rng.choice(b"ACGT") for _ in range(rng.randint(5, 60))) + bytearray(k1)
        e2 = bytearray(k2) + bytearray(rng.choice(b"ACGT") for _ in range(rng.randint(5, 60)))
        runs["e1"] = [_plant(rng, e1, len(e1) - k1, unit, k1, False)]
        # e2 starts in the phase in which e1 ends: a roll that crossed the seam would go on matching
        phase = k1 % len(unit)
        runs["e2"] = [_plant(rng, e2, 0, unit[phase:] + unit[:phase], k2, rng.random() < 0.3)]
        seqs["e1"], seqs["e2"] = bytes(e1), bytes(e2)
    if rng.random() < 0.75 or len(seqs) == 1:
        seqs["one"] = bytes([rng.choice(b"ACGTNa")])
    if rng.random() < 0.4:
        extra = bytearray(rng.choice(b"ACGTacgt") for _ in range(rng.choice([50, 700])))
        runs["extra"] = [_plant(rng, extra, len(extra) - 30, _unit(rng), 30, False)]
        seqs["extra"] = bytes(extra)
    names = [k for k in seqs if k != "e2"]
    rng.shuffle(names)
    order = [x for k in names for x in ((k, "e2") if k == "e1" else (k,))]
    return {k: seqs[k] for k in order}, runs


def _phase_text(run, phase, n):
    """n bases of the run's pattern from `phase` on, upper-case: what an in-phase insertion at that place adds"""
    u = run["unit"]
    return bytes(u[(phase + i) % len(u)] for i in range(n))


def make_rows(rng, seqs, runs, n, cap):
    """rows of (chrom, start, ref, alt) and their kinds"""
    place = cap if cap <= 65 else DEFAULT_CAP
    with_runs = [(c, r) for c in seqs for r in runs.get(c, [])]
    rows, kinds = [], []
    while len(rows) < n:
        x = rng.random()
        chrom = rng.choice(list(seqs))
        seq = seqs[chrom]
        if x < 0.10:
            kind = rng.choice(FAILING)
            p = rng.randrange(len(seq))
            row = {"mismatch": (chrom, p, bytes([_other(rng, seq[p])]) if rng.random() < 0.5 or p + 3 > len(seq)
                                else seq[p:p + 2] + bytes([_other(rng, seq[p + 2])]), b"A"),
                   "ref_past_end": (chrom, len(seq) - 1, seq[-1:] + b"A", b"C"),
                   "start_past_end": (chrom, len(seq) + rng.choice([1, 5, 1 << 40]), b"A", b"C"),
                   "overflow": (chrom, (1 << 64) - rng.choice([1, 2]), b"AC", b"A"),
                   "unknown": ("nope", 5, b"A", b"C")}[kind]
        elif x < 0.45 and with_runs:
            chrom, run = rng.choice(with_runs)
            seq = seqs[chrom]
            at, length, u = run["at"], run["length"], len(run["unit"])
            # d bases from one of the run's ends: long runs are mostly entered near an end, so that the other side's roll stays cheap
            d = rng.choice([place + k for k in NEAR] + [rng.randrange(0, 8)] * 4 + ([1000] if rng.random() < 0.3 else []))
            if d > length or (length > 600 and d < 1000 and rng.random() < 0.8):
                d = rng.randrange(0, min(length, 12) + 1)
            kind = rng.choice(["ins", "ins", "ins_multi_partial", "del_units", "ins_lower"])
            if kind == "del_units":
                k = rng.choice([1, 1, 2, 5]) * u
                if k > length:
                    k = length
                p = at + d if rng.random() < 0.5 else at + length - d - k
                p = min(max(p, at), at + length - k)
                ref = seq[p:p + k] if rng.random() < 0.5 else seq[p:p + k].upper()
                row = (chrom, p, ref, b"")
            else:
                p = at + d if rng.random() < 0.5 else at + length - d
                size = u if kind != "ins_multi_partial" else rng.choice([2, 3]) * u + rng.randrange(1, u + 1)
                alt = _phase_text(run, (p - at) % u, size)
                if kind == "ins":
                    kind = "ins_unit" if (p - at) % u == 0 else "ins_rot"
                row = (chrom, p, b"", alt.lower() if kind == "ins_lower" else alt)
        else:
            kind = rng.choice(["snv", "snv", "mnv", "delins", "same", "ins", "del", "lower", "ins@0", "ins@len", "ins_n"])
            p = rng.randrange(len(seq))
            if kind == "ins_n":  # an N into a run of N: it rolls like any other base
                p = seq.find(b"NN")
                kind, p = ("ins_n", p + 1) if p >= 0 else ("snv", 0)
            k = min(rng.choice([1, 2, 4, 11, 30]), len(seq) - p)
            ref = seq[p:p + k]
            if kind == "snv":
                row = (chrom, p, ref[:1], bytes([_other(rng, ref[0])]))
            elif kind == "mnv":  # differs at both ends: nothing trims
                alt = bytearray(rng.choice(b"ACGT") for _ in range(k))
                alt[0], alt[-1] = _other(rng, ref[0]), _other(rng, ref[-1])
                row = (chrom, p, ref.upper(), bytes(alt))
            elif kind == "delins":
                row = (chrom, p, ref, ref[:k // 2].upper() + bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 5))) + ref[k // 2 + 1:].upper())
            elif kind == "same":
                row = (chrom, p, ref, ref)
            elif kind == "ins":
                row = (chrom, p, ref[:1], ref[:1] + bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 5))))
            elif kind == "del":
                row = (chrom, p, ref, ref[:1])
            elif kind == "ins_n":
                row = (chrom, p, b"", b"N")
            elif kind == "lower":
                row = (chrom, p, ref.lower(), ref.lower()[:k // 2] + rng.choice([b"", b"a", b"ct"]))
            else:
                run = next(iter(runs.get(chrom, [])), None) if kind == "ins@0" else next(iter(runs.get(chrom, [])[::-1]), None)
                alt = run["unit"] if run and rng.random() < 0.6 else bytes(rng.choice(b"ACGT") for _ in range(rng.randint(1, 4)))
                row = (chrom, 0 if kind == "ins@0" else len(seq), b"", alt)
        rows.append(row)
        kinds.append(kind)
    return rows, kinds


def make_case(seed):
    """pure: the same assembly, rows, switches and call choices for the same seed"""
    rng = random.Random(seed)
    cap_sw, host_sw = rng.choice(CAPS), rng.choice(HOST_LENS)
    cap = DEFAULT_CAP if cap_sw is None else cap_sw
    seqs, runs = make_assembly(rng, cap if cap <= 65 else DEFAULT_CAP)
    n = rng.choice(COUNTS)
    rows, kinds = make_rows(rng, seqs, runs, n, cap)
    switches = {}
    if cap_sw is not None:
        switches["GTARS_VRS_ROLL_CAP"] = str(cap_sw)
    if host_sw is not None:
        switches["GTARS_VRS_HOST_LEN"] = str(host_sw)
    accessions = None
    if rng.random() < 0.25:  # a caller's table: one chromosome missing (its rows are status 4), one digest of the caller's own
        own = R.refget_digests(seqs)
        names = list(seqs)
        gone, swapped = rng.choice(names), rng.choice(names)
        accessions = {k: ("SQ." if rng.random() < 0.5 else "") + ("Q" * 32 if k == swapped else v) for k, v in own.items() if k != gone}
    return dict(seed=seed, seqs=seqs, runs=runs, rows=rows, kinds=kinds, cap=cap, switches=switches, width=rng.choice([7, 60, 61, 80, 1000]),
                binary=seed % 2 == 1, also_host=rng.random() < 0.5, accessions=accessions)


def _trimmed(row):
    """(start, end) of the allele after the prefix and suffix trim of vrs_ref.normalize, and the trimmed alleles"""
    _, s, ref, alt = row
    e = s + len(ref)
    while ref and alt and ref[0] == alt[0]:
        ref, alt, s = ref[1:], alt[1:], s + 1
    while ref and alt and ref[-1] == alt[-1]:
        ref, alt, e = ref[:-1], alt[:-1], e - 1
    return s, e, ref, alt


def expected(case):
    """vrs_ref.alleles over the case: "plain" = (statuses, starts, ends, sequences) of normalize_alleles, "ids" = (statuses, ids)
    of vrs_ids under the case's accession table, and the tags the answer puts the case on"""
    seqs, rows = case["seqs"], case["rows"]
    own = R.refget_digests(seqs)
    st, ns, ne, sq, ids = R.alleles(seqs, own, rows)
    want = dict(plain=(st, ns, ne, sq), ids=(st, ids))
    if case["accessions"] is not None:
        table = {k: v[-32:] for k, v in case["accessions"].items()}
        again = R.alleles(seqs, table, rows)
        want["ids"] = (again[0], again[4])
    want["tags"] = answer_tags(case, want)
    return want


def answer_tags(case, want):
    seqs, rows, kinds, cap = case["seqs"], case["rows"], case["kinds"], case["cap"]
    names = list(seqs)
    sw = case["switches"]
    tags = {"n=%d" % len(rows), "cap=%s" % sw.get("GTARS_VRS_ROLL_CAP", "unset"), "host_len=%s" % sw.get("GTARS_VRS_HOST_LEN", "unset"),
            "binary" if case["binary"] else "fasta"}
    if case["also_host"]:
        tags.add("also_host")
    if case["accessions"] is not None and R.UNKNOWN_CHROMOSOME in want["ids"][0]:
        tags.add("table_lacks_chrom")
    host_len = int(sw.get("GTARS_VRS_HOST_LEN", 4096))
    st, ns, ne, sq = want["plain"]
    for k, (row, kind) in enumerate(zip(rows, kinds)):
        if st[k] != R.OK:
            good = [j for j in (k - 1, k + 1) if 0 <= j < len(rows) and st[j] == R.OK]
            if kind in FAILING and good:
                tags.add("fail=%s:%d" % (kind, st[k]))
            continue
        if len(sq[k]) > host_len:
            tags.add("host_tail")
        seq = seqs[row[0]]
        s, e, ref, alt = _trimmed(row)
        left, right = s - ns[k], ne[k] - e
        for side, roll in (("left", left), ("right", right)):
            if not roll:
                continue
            if cap <= 65 and roll - cap in NEAR:
                tags.add("%s_roll=cap%+d" % (side, roll - cap))
            if roll > cap:
                tags.add(side + "_roll>cap")
            if 900 <= roll <= 1600:
                tags.add(side + "_roll~1000")
        if left and ns[k] == 0:
            tags.add("left_stop=0")
            if names.index(row[0]) > 0:
                tags.add("left_stop=0_chrom_in_front")
        if right and ne[k] == len(seq):
            tags.add("right_stop=len")
            if row[0] == "e1" and "e2" in seqs and seqs["e2"][:1].upper() == _phase_text(case["runs"]["e1"][0], case["runs"]["e1"][0]["length"], 1):
                tags.add("right_stop=len_like_neighbour")
        if (left and ns[k] > 0 and seq[ns[k] - 1] in b"Nn") or (right and ne[k] < len(seq) and seq[ne[k]] in b"Nn"):
            tags.add("roll_stop=N")
        if (left or right) and seq[ns[k]:ne[k]] != seq[ns[k]:ne[k]].upper():
            tags.add("roll_through_soft_mask")
        if kind == "ins_rot" and (left or right):
            tags.add("ins_rot_rolls")
        if kind == "ins_multi_partial" and (left or right):
            tags.add("ins_multi_partial_rolls")
        if kind == "del_units" and (left or right):
            tags.add("del_units_rolls")
        if kind == "ins_n" and left and right:
            tags.add("n_into_n_rolls")
        if not left and not right and alt != alt.upper() and not ref:
            a, b, _ = R.normalize(seq, row[1], row[2], row[3].upper())
            if (a, b) != (ns[k], ne[k]):
                tags.add("lower_alt_does_not_roll")
        if kind in ("ins@0", "ins@len", "same", "mnv", "delins", "lower", "snv"):
            tags.add("kind=" + kind)
    return tags


def check(case, tmp, want, on_host):
    """the two batch calls over the case, on the device or on the library's host path, against `want`"""
    import gtars_amd
    from gtars_amd import vrs as V
    from gtars_amd.seqstats import BinaryGenomeAssembly, GenomeAssembly, write_fab

    seed = case["seed"]
    fa = os.path.join(tmp, "vrs_%d.fa" % seed)
    write_fasta(fa, case["seqs"], case["width"])
    for k in ("GTARS_VRS_ROLL_CAP", "GTARS_VRS_HOST_LEN"):
        os.environ.pop(k, None)
    os.environ.update(case["switches"])
    gtars_amd.reload_env()
    try:
        if case["binary"]:
            write_fab(fa, fa + "b")
            g = BinaryGenomeAssembly(fa + "b")
        else:
            g = GenomeAssembly(fa)
        assert g.chrom_names == list(case["seqs"]), ("vrs names", seed)
        cols = [[r[k] for r in case["rows"]] for k in range(4)]
        st, ns, ne, sq = want["plain"]
        got = V.normalize_alleles(g, *cols, on_host=on_host)
        assert got["statuses"].tolist() == st, ("vrs statuses", seed, on_host)
        assert got["starts"].tolist() == ns and got["ends"].tolist() == ne, ("vrs intervals", seed, on_host)
        assert got["sequences"] == sq, ("vrs sequences", seed, on_host)
        got = V.vrs_ids(g, *cols, accessions=case["accessions"], on_host=on_host)
        assert got["statuses"].tolist() == want["ids"][0], ("vrs id statuses", seed, on_host)
        assert got["ids"] == want["ids"][1], ("vrs ids", seed, on_host)
        if not on_host and case["rows"]:
            assert g.device >= 0, ("vrs ran on no device", seed)
        del g
    finally:
        for p in (fa, fa + "b", fa + ".fai"):
            if os.path.exists(p):
                os.remove(p)


def run_device(case, tmp, want=None):
    want = expected(case) if want is None else want
    check(case, tmp, want, False)
    if case["also_host"]:
        check(case, tmp, want, True)


def one(seed, tmp=None):
    own = tmp is None
    tmp = tempfile.mkdtemp(prefix="gtars_fuzzvrs_") if own else str(tmp)
    try:
        case = make_case(seed)
        want = expected(case)
        run_device(case, tmp, want)
        return want["tags"]
    finally:
        if own:
            shutil.rmtree(tmp, ignore_errors=True)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    base = int(sys.argv[2]) if len(sys.argv) > 2 else 18_000
    t = time.time()
    tags = set()
    tmp = tempfile.mkdtemp(prefix="gtars_fuzzvrs_")
    try:
        for seed in range(rounds):
            tags |= one(base + seed, tmp)
            if seed % 25 == 24:
                print(f"  {seed + 1} rounds, {time.time() - t:.0f} s", flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(f"fuzz_vrs: {rounds} random batches (seeds {base} .. {base + rounds - 1}) equal to vrs_ref, {len(tags)} tags ({time.time() - t:.0f} s)")


if __name__ == "__main__":
    main()
