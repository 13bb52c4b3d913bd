#!/usr/bin/env python3
"""Randomised differential soak of K19 (csrc/reftx.hip) and K20 (csrc/hgvs.hip, which feeds K18): CoordinateMapper rows against
reftx_ref.map_rows, mature_mrnas and transcript_accessions against reftx_ref.mature and sha512t24u, hgvs_to_vrs_ids against
hgvs_ref.bridge -- every column equal.

A case is one random world of the CPU tests' own generators (test_hgvs_cpu.random_world, random_strings; test_reftx_cpu.
random_queries), seeded per case, its assembly written per case: four chromosomes with planted repeats, a few IUPAC codes planted
here, 30 random transcripts and two hand-made ones (overlapping exons, no exons), batches of 0 to about 1500 mapping rows and
HGVS expressions.  Part of the expressions are dups, deletions and in-phase insertions inside the planted repeats, so that their
alleles roll in K18 behind the bridge -- past GTARS_VRS_ROLL_CAP when the case draws a small one.  GTARS_TX_HOST_LEN,
GTARS_VRS_ROLL_CAP and GTARS_VRS_HOST_LEN are drawn per case.

make_case(seed) and expected(case) need no device (tests/test_soak_generators_cpu.py runs them, and check(..., on_host=True));
run_device(case, tmp) does.

Run on the GPU box:  python tests/soak/fuzz_transcripts.py [rounds] [first_seed]"""
import os, random, shutil, sys, tempfile, time
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
import hgvs_ref as HR
import reftx_ref as R
from test_hgvs_cpu import check_batch, random_strings, random_world
from test_reftx_cpu import build_store, random_queries, run_rows
from test_vrs_cpu import write_fasta

COUNTS = [0, 1, 63, 64, 65, 255, 256, 257, 1500]
TX_HOST_LENS = [None, 0, 8]
CAPS = [None, 1, 8, 63, 64, 65, 1 << 20]
HOST_LENS = [None, 0, 8, 1 << 20]
REPEATS = {"CAG": (100, 160), "A": (300, 340)}  # random_world's planted repeats on chrA: unit -> [start, end)
ALIASES = {"NC_five.1": "chrB"}
SWITCHES = ("GTARS_TX_HOST_LEN", "GTARS_VRS_ROLL_CAP", "GTARS_VRS_HOST_LEN")


def plant_iupac(rng, seqs, txs):
    """a few IUPAC codes outside the planted repeats; the transcripts follow their chromosomes' new digests"""
    old = {R.digest_bytes(d): name for name, d in R.refget_digests(seqs).items()}
    for name in ("chrA", "chrB"):
        s = bytearray(seqs[name])
        for _ in range(4):
            p = rng.randrange(350, len(s) - 8)
            s[p:p + 3] = rng.choice([b"RYK", b"ryM", b"SWN", b"BdH"])
        seqs[name] = bytes(s)
    new = R.refget_digests(seqs)
    for tx in txs:
        if tx["digest"] in old:
            tx["digest"] = R.digest_bytes(new[old[tx["digest"]]])


def repeat_strings(rng, n):
    """g. expressions inside chrA's planted repeats: their alleles roll through the repeat"""
    out = []
    for _ in range(n):
        unit, (lo, hi) = rng.choice(sorted(REPEATS.items()))
        u = len(unit)
        p = rng.randrange(lo, hi - 2 * u)          # 0-based
        p -= (p - lo) % u if rng.random() < 0.7 else 0  # mostly at a unit's first base
        k = rng.choice([1, 1, 2, 3]) * u
        last = min(p + k, hi) - 1
        span = str(p + 1) if last == p else "%d_%d" % (p + 1, last + 1)
        kind = rng.random()
        if kind < 0.4:
            out.append("chrA:g.%sdup" % span)
        elif kind < 0.8:
            out.append("chrA:g.%sdel" % span)
        else:
            phase = (p + 1 - lo) % u
            out.append("chrA:g.%d_%dins%s" % (p + 1, p + 2, (unit[phase:] + unit[:phase]) * rng.choice([1, 2])))
    return out


def make_case(seed):
    """pure: the same world, rows, names, expressions and switches for the same seed"""
    rng = random.Random(seed)
    seqs, txs = random_world(rng, seed % 100_000)
    plant_iupac(rng, seqs, txs)
    own = R.refget_digests(seqs)
    tag = seed % 100_000
    txs.append(R.make_tx(f"NM_{tag}_bad.1", R.digest_bytes(own["chrA"]), 1, [(10, 20), (15, 30)], (12, 18), gene=f"BAD{tag}"))  # overlapping exons
    txs.append(R.make_tx(f"NM_{tag}_none.1", bytes(24), -1, []))
    n = rng.choice(COUNTS)
    rows = random_queries(rng, txs, n)
    names = [rng.choice(txs)["accession"] if rng.random() < 0.9 else "NM_NOPE.1" for _ in range(min(n, 300))]
    strings = random_strings(rng, seqs, txs, n, ALIASES)
    for k in rng.sample(range(n), n // 6 if n > 1 else n):
        strings[k] = repeat_strings(rng, 1)[0]
    accessions = {k: v for k, v in own.items() if k != "chrD" or rng.random() < 0.3}  # mostly, chrD has no accession: K18's status 4
    switches = {}
    for name, values in zip(SWITCHES, (TX_HOST_LENS, CAPS, HOST_LENS)):
        v = rng.choice(values)
        if v is not None:
            switches[name] = str(v)
    return dict(seed=seed, seqs=seqs, txs=txs, rows=rows, names=names, strings=strings, accessions=accessions, switches=switches,
                width=rng.choice([11, 60, 61, 1000]))


def expected(case):
    """the restatements' answers: "map" (values, statuses), "mature" [(status, bytes)] per name, "digests" {accession: SQ. digest}
    of the whole store, "bridge" rows, and the tags the answers put the case on"""
    seqs, txs = case["seqs"], case["txs"]
    want = dict(map=R.map_rows(txs, case["rows"]), mature=[R.mature(seqs, R.lookup(txs, a)) for a in case["names"]])
    whole = {tx["accession"]: R.mature(seqs, tx) for tx in txs}
    want["whole"] = whole
    want["digests"] = {a: "SQ." + R.sha512t24u(s) for a, (st, s) in whole.items() if st == R.SEQ_OK}
    want["bridge"] = HR.bridge(seqs, case["accessions"], txs, case["strings"], ALIASES)
    want["tags"] = answer_tags(case, want)
    return want


def answer_tags(case, want):
    sw = case["switches"]
    tags = {"n=%d" % len(case["rows"])} | {"%s=%s" % (k[6:].lower(), sw.get(k, "unset")) for k in SWITCHES}
    tags |= {"map_status=%d" % s for s in want["map"][1]}
    tags |= {"seq_status=%d" % st for st, _ in want["mature"]} | {"seq_status=%d" % st for st, _ in want["whole"].values()}
    tx_host_len = int(sw.get("GTARS_TX_HOST_LEN", 65536))
    if any(st == R.SEQ_OK and len(s) > tx_host_len for st, s in want["whole"].values()):
        tags.add("tx_host_tail")
    if any(st == R.SEQ_OK and tx["strand"] < 0 and set(s.upper()) - set(b"ACGTN") for tx in case["txs"]
           for st, s in [R.mature(case["seqs"], dict(tx, strand=1))]):
        tags.add("reverse_strand_iupac")
    cap, host_len = int(sw.get("GTARS_VRS_ROLL_CAP", 64)), int(sw.get("GTARS_VRS_HOST_LEN", 4096))
    tags |= {"hgvs_status=%d" % w["status"] for w in want["bridge"]}
    for w in want["bridge"]:
        if w["status"] != HR.OK:
            continue
        _, s, e, _ = w["span"]
        if s - w["start"] > 0 or w["end"] - e > 0:
            tags.add("hgvs_rolls")
        if s - w["start"] > cap or w["end"] - e > cap:
            tags.add("hgvs_rolls_past_cap")
        if w["end"] - w["start"] > host_len:
            tags.add("hgvs_k18_host_tail")
    return tags


def check(case, tmp, want, on_host):
    """the library's batch calls over the case, on the device or on its host path, against `want`"""
    import gtars_amd
    from gtars_amd import hgvs as H
    from gtars_amd import reftx as T
    from gtars_amd.seqstats import GenomeAssembly

    seed = case["seed"]
    fa = os.path.join(tmp, "tx_%d.fa" % seed)
    write_fasta(fa, case["seqs"], case["width"])
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(case["switches"])
    gtars_amd.reload_env()
    try:
        g = GenomeAssembly(fa)
        store = build_store(case["txs"])
        mapper = T.CoordinateMapper(store) if on_host else T.CoordinateMapper(store, g)
        got = run_rows(mapper, case["rows"], on_host=on_host)
        assert got == want["map"], ("tx map", seed, on_host, next(i for i in range(len(case["rows"])) if (got[0][i], got[1][i]) != (want["map"][0][i], want["map"][1][i])))
        seqs, status = T.mature_mrnas(g, store, case["names"], with_status=True, on_host=on_host)
        assert status.tolist() == [st for st, _ in want["mature"]], ("tx sequence statuses", seed, on_host)
        assert seqs == [s.decode() if st == R.SEQ_OK else None for st, s in want["mature"]], ("tx sequences", seed, on_host)
        assert T.transcript_accessions(g, store, on_host=on_host) == want["digests"], ("tx digests", seed, on_host)
        got = H.hgvs_to_vrs_ids(g, store, case["strings"], accessions=case["accessions"], aliases=ALIASES, on_host=on_host)
        check_batch(got, want["bridge"], case["seqs"], ("hgvs", seed, on_host))
        if not on_host and case["rows"]:
            assert g.device >= 0, ("transcripts ran on no device", seed)
        del mapper, store, g
    finally:
        for p in (fa, fa + ".fai"):
            if os.path.exists(p):
                os.remove(p)


def run_device(case, tmp, want=None):
    check(case, tmp, expected(case) if want is None else want, False)


def one(seed, tmp=None):
    own = tmp is None
    tmp = tempfile.mkdtemp(prefix="gtars_fuzztx_") if own else str(tmp)
    try:
        case = make_case(seed)
        want = expected(case)
        run_device(case, tmp, want)
        return want["tags"]
    finally:
        if own:
            shutil.rmtree(tmp, ignore_errors=True)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    base = int(sys.argv[2]) if len(sys.argv) > 2 else 19_000
    t = time.time()
    tags = set()
    tmp = tempfile.mkdtemp(prefix="gtars_fuzztx_")
    try:
        for seed in range(rounds):
            tags |= one(base + seed, tmp)
            if seed % 25 == 24:
                print(f"  {seed + 1} rounds, {time.time() - t:.0f} s", flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(f"fuzz_transcripts: {rounds} random worlds (seeds {base} .. {base + rounds - 1}) equal to reftx_ref and hgvs_ref, {len(tags)} tags ({time.time() - t:.0f} s)")


if __name__ == "__main__":
    main()
