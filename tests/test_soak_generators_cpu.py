"""The generators and references of the K17 - K20 fuzzers (tests/soak/fuzz_bam.py, fuzz_vrs.py, fuzz_transcripts.py), without a
device, over exactly the seeds tests/test_gpu_soak_short.py runs on one:

  1. the union of the cases' tags -- each computed from the case and the restatement's answer, never from the library -- holds a
     required set of edges written out here, so the short run is known to reach them;
  2. the library's host paths (on_host=True of VRS, reftx and hgvs) equal `expected` on every case, which holds the generators and
     the restatements to the library on the CPU; BAM has no host QC: there the Python reader's round trip (inside expected) and
     BamFile.record_offsets are checked on every file;
  3. small mutations of the restatements, monkeypatched here (the committed restatements stay as they are), must change
     `expected` for at least one seed each: a reference this suite could not tell from a subtly wrong one checks nothing;
  4. make_case(seed) gives the same inputs on two calls.

Run with -s to see the tags reached and the count of seeds that notice each mutation."""
import importlib.util
import os

import numpy as np
import pytest

import bam_ref
import hgvs_ref
import reftx_ref
import vrs_ref
from test_gpu_soak_short import BAM_SEEDS, SOAK, TRANSCRIPT_SEEDS, VRS_SEEDS


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(SOAK, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SEEDS = {"fuzz_bam": BAM_SEEDS, "fuzz_vrs": VRS_SEEDS, "fuzz_transcripts": TRANSCRIPT_SEEDS}


@pytest.fixture(scope="module")
def runs():
    """per fuzzer: the module and [(case, expected)] over the short run's seeds, computed once and left unchanged"""
    out = {}
    for name, seeds in SEEDS.items():
        fz = _load(name)
        pairs = []
        for seed in seeds:
            case = fz.make_case(seed)
            pairs.append((case, fz.expected(case)))
        out[name] = (fz, pairs)
    return out


def _tags(pairs):
    tags = {}
    for case, want in pairs:
        for t in set(case.get("tags", ())) | set((want or {}).get("tags", ())):
            tags[t] = tags.get(t, 0) + 1
    return tags


# ---- 1. the edges the short run reaches -----------------------------------------------------------------------------------
BAM_REQUIRED = {
    "cut+1", "cut+2", "cut+3",      # a block ends 1, 2 and 3 bytes into a block_size field
    "cut=record", "cut_in_name",
    "window<record",                # a device window smaller than a record
    "chrom>=3windows",              # a chromosome's records over three or more windows: Grow::ensure keeps earlier names
    "chrom_change_in_window",
    "name_x3",                      # a name three times in one table: the last wins
    "last_byte_siblings",           # two names of one table that differ in the last byte only
    "names>16",                     # more names in a table than 4 hash bits tell apart
    "star_paired",                  # a `*` name on a paired record
    "single_and_paired_chrom",
    "read1_only_chrom",             # nothing joins
    "unplaced_tail", "empty_file", "refusal", "mito", "refs=300",
    "hash_bits=unset", "hash_bits=0", "hash_bits=1", "hash_bits=4", "hash_bits=33",
    "window=None", "window=1", "window=64", "window=500", "window=5000",
    "block=50", "block=333", "block=65280", "threads=1", "threads=4",
} | {"n=%d" % n for n in (0, 1, 2, 63, 64, 65, 256, 257, 1500)}

VRS_REQUIRED = {"%s_roll=cap%+d" % (side, d) for side in ("left", "right") for d in (-1, 0, 1, 63, 64, 65)} | {
    "left_roll~1000", "right_roll~1000",
    "left_stop=0",                        # a roll stopped by position 0
    "right_stop=len_like_neighbour",      # ... by the chromosome's length, the next chromosome of the image going on with the unit
    "roll_stop=N", "roll_through_soft_mask", "lower_alt_does_not_roll", "ins_rot_rolls", "ins_multi_partial_rolls", "del_units_rolls",
    "n_into_n_rolls",
    "fail=mismatch:3", "fail=ref_past_end:2", "fail=start_past_end:2", "fail=overflow:1", "fail=unknown:4",
    "table_lacks_chrom", "host_tail", "also_host", "binary", "fasta", "kind=ins@0", "kind=ins@len", "kind=same", "kind=lower",
} | {"n=%d" % n for n in (0, 1, 63, 64, 65, 257, 600)} | {"cap=%s" % c for c in ("unset", 1, 8, 63, 64, 65, 1 << 20)} | {
    "host_len=%s" % h for h in ("unset", 0, 8, 1 << 20)}

TRANSCRIPT_REQUIRED = {"map_status=%d" % s for s in range(11) if s != reftx_ref.BAD_KIND} | {"seq_status=%d" % s for s in range(5)} | {
    "tx_host_tail",                       # a digest finished by the host threads
    "hgvs_rolls_past_cap",                # an HGVS row whose allele goes to K18's wave path
    "hgvs_k18_host_tail", "reverse_strand_iupac",
} | {"hgvs_status=%d" % s for s in range(12)} | {"tx_host_len=%s" % h for h in ("unset", 0, 8)} | {
    "vrs_roll_cap=%s" % c for c in ("unset", 1, 8, 63, 64, 65, 1 << 20)} | {"vrs_host_len=%s" % h for h in ("unset", 0, 8, 1 << 20)} | {
    "n=%d" % n for n in (0, 1, 63, 64, 65, 255, 256, 257, 1500)}


@pytest.mark.parametrize("name,required", [("fuzz_bam", BAM_REQUIRED), ("fuzz_vrs", VRS_REQUIRED), ("fuzz_transcripts", TRANSCRIPT_REQUIRED)])
def test_the_short_run_reaches_the_edges(runs, name, required):
    tags = _tags(runs[name][1])
    print(f"\n{name}: {len(SEEDS[name])} seeds from {SEEDS[name][0]}, tags reached (cases): " + ", ".join(f"{t} ({n})" for t, n in sorted(tags.items())))
    assert not required - set(tags), sorted(required - set(tags))


# ---- 2. the host paths over the same seeds ----------------------------------------------------------------------------------
def test_bam_files_read_back_and_their_record_offsets(runs, tmp_path):
    """expected() has read every file back through the Python reader and compared it with the generator's records; here the
    library's BGZF reader and host record walk over the same bytes (the refusal files too: the walk follows block_size alone)"""
    from gtars_amd import bam as B

    fz, pairs = runs["fuzz_bam"]
    for case, want in pairs:
        p = str(tmp_path / "f.bam")
        with open(p, "wb") as f:
            f.write(case["data"])
        blocks, stream = bam_ref.read_blocks(case["data"])
        with B.BamFile(p) as b:
            assert b.references == case["refs"] and b.first_record == case["first"], case["seed"]
            assert b.n_blocks == len(blocks) and b.n_bytes == len(stream), case["seed"]
            assert b.inflate() == stream, case["seed"]
            assert b.record_offsets().tolist() == case["starts"], case["seed"]
        assert (want is None) == case["refused"]
    print(f"\nfuzz_bam: {len(pairs)} files read back, record offsets equal")


@pytest.mark.parametrize("name", ["fuzz_vrs", "fuzz_transcripts"])
def test_host_paths_equal_the_restatements(runs, tmp_path, name, monkeypatch):
    import gtars_amd

    fz, pairs = runs[name]
    before = {k: v for k, v in os.environ.items() if k.startswith("GTARS_")}
    try:
        for case, want in pairs:
            fz.check(case, str(tmp_path), want, True)
    finally:
        for k in [k for k in os.environ if k.startswith("GTARS_") and k not in before]:
            del os.environ[k]
        os.environ.update(before)
        gtars_amd.reload_env()
    print(f"\n{name}: the library's host path equals expected() on {len(pairs)} cases")


# ---- 3. sensitivity -------------------------------------------------------------------------------------------------------------
def _same(a, b):
    """two results of expected(), tags aside"""
    if a is None or b is None:
        return a is b
    for k in a:
        if k == "tags":
            continue
        if k == "columns":
            if any(not np.array_equal(a[k][c], b[k][c]) for c in a[k]):
                return False
        elif a[k] != b[k]:
            return False
    return True


def _noticing(fz, pairs):
    return [case["seed"] for case, want in pairs if not _same(fz.expected(case), want)]


def process_chromosome_mutated(first_wins=False, keep_star=False, no_l_seq=False):
    """bam_ref.process_chromosome with one rule bent"""
    def process_chromosome(records, c, chrom):
        res = dict(position_counts={}, total_reads=0, num_pairs=0, dup_count=0, mito_reads=0, is_paired=False)
        if bam_ref.is_mitochondrial(chrom):
            return ORIGINAL_PROCESS_CHROMOSOME(records, c, chrom)
        read1, read2 = {}, {}
        pc = res["position_counts"]
        for r in (x for x in records if x["ref_id"] == c):
            if (r["mapq"] != 255 and r["mapq"] < bam_ref.MIN_MAPQ) or r["flag"] & 0x4:
                continue
            res["total_reads"] += 1
            if r["flag"] & 0x400:
                res["dup_count"] += 1
            if r["pos"] == -1:
                continue
            pos = r["pos"] + 1
            if r["flag"] & 0x1:
                res["is_paired"] = True
                if r["name"] == b"*" and not keep_star:
                    continue
                table = read1 if r["flag"] & 0x40 else read2 if r["flag"] & 0x80 else None
                if table is not None and not (first_wins and r["name"] in table):
                    table[r["name"]] = (pos, r["tlen"])
            else:
                key = (pos, 0 if no_l_seq else r["l_seq"], 0, 0)
                pc[key] = pc.get(key, 0) + 1
        if res["is_paired"]:
            for qname, (pos1, tlen1) in read1.items():
                if qname in read2:
                    key = (pos1, tlen1) + read2[qname]
                    pc[key] = pc.get(key, 0) + 1
                    res["num_pairs"] += 1
        return res
    return process_chromosome


ORIGINAL_PROCESS_CHROMOSOME = bam_ref.process_chromosome


def test_the_unbent_copy_is_the_restatement(runs):
    """the copy above with no rule bent gives what bam_ref gives: the mutations differ from it by their one rule only"""
    copy = process_chromosome_mutated()
    for case, want in runs["fuzz_bam"][1]:
        for c, (chrom, _) in enumerate(case["refs"]):
            if any(r["ref_id"] == c for r in case["records"]):
                assert copy(case["records"], c, chrom) == ORIGINAL_PROCESS_CHROMOSOME(case["records"], c, chrom), case["seed"]


def normalize_mutated(stop_short=False, lower_rolls=False, drop_partial=False):
    """vrs_ref.normalize with one rule bent"""
    def period(a):
        return next(p for p in range(1, len(a) + 1) if all(a[i] == a[i % p] for i in range(len(a))))

    def normalize(sequence, start, ref, alt):
        n = len(sequence)
        ORIGINAL_NORMALIZE(sequence, start, ref, alt)  # (the checks, and their errors)
        s, e = start, start + len(ref)
        while ref and alt and ref[0] == alt[0]:
            ref, alt, s = ref[1:], alt[1:], s + 1
        while ref and alt and ref[-1] == alt[-1]:
            ref, alt, e = ref[:-1], alt[:-1], e - 1
        alleles = [a for a in (ref, alt) if a]
        if lower_rolls:
            alleles = [a.upper() for a in alleles]
        if drop_partial:  # an allele of whole units and a partial one is taken for its whole units
            alleles = [a[:len(a) - len(a) % period(a)] for a in alleles]
        left = right = 0
        if alleles:
            while left < s:
                base = sequence[s - 1 - left:s - left].upper()[0]
                if any(a[-((left + 1) % len(a))] != base if (left + 1) % len(a) else a[0] != base for a in alleles):
                    break
                left += 1
            while e + right < n - (1 if stop_short else 0):
                base = sequence[e + right:e + right + 1].upper()[0]
                if any(a[right % len(a)] != base for a in alleles):
                    break
                right += 1
        return s - left, e + right, sequence[s - left:s].upper() + alt + sequence[e:e + right].upper()
    return normalize


ORIGINAL_NORMALIZE = vrs_ref.normalize


def test_the_unbent_copy_is_normalize(runs):
    copy = normalize_mutated()
    for case, want in runs["fuzz_vrs"][1][:20]:
        for row, st in zip(case["rows"], want["plain"][0]):
            if st == vrs_ref.OK:
                assert copy(case["seqs"][row[0]], *row[1:]) == ORIGINAL_NORMALIZE(case["seqs"][row[0]], *row[1:]), (case["seed"], row)


def _c_to_g_star_one_off(tx, c_pos, offset=0, star=False):
    return ORIGINAL_C_TO_G(tx, c_pos + 1 if star else c_pos, offset, star)


ORIGINAL_C_TO_G = reftx_ref.c_to_g

MUTATIONS = [
    ("fuzz_bam", "the first entry of a name wins", bam_ref, "process_chromosome", process_chromosome_mutated(first_wins=True)),
    ("fuzz_bam", "mapq <= 30 is dropped", bam_ref, "MIN_MAPQ", 31),
    ("fuzz_bam", "the single-end key without l_seq", bam_ref, "process_chromosome", process_chromosome_mutated(no_l_seq=True)),
    ("fuzz_bam", "* is kept as a name", bam_ref, "process_chromosome", process_chromosome_mutated(keep_star=True)),
    ("fuzz_vrs", "a roll stops one base short of the chromosome's end", vrs_ref, "normalize", normalize_mutated(stop_short=True)),
    ("fuzz_vrs", "a lower-case ALT rolls", vrs_ref, "normalize", normalize_mutated(lower_rolls=True)),
    ("fuzz_vrs", "a partial unit is ignored", vrs_ref, "normalize", normalize_mutated(drop_partial=True)),
    ("fuzz_transcripts", "the reverse strand keeps IUPAC codes", reftx_ref, "reverse_complement",
     lambda seq: bytes(reftx_ref.COMPLEMENT.get(b, b) for b in reversed(seq))),
    ("fuzz_transcripts", "c.*N is anchored one base off", reftx_ref, "c_to_g", _c_to_g_star_one_off),
    ("fuzz_transcripts", "any position takes an intronic offset", reftx_ref, "is_exon_boundary", lambda tx_pos, offsets, positive: True),
    ("fuzz_transcripts", "a reverse-strand ALT is complemented but not reversed", hgvs_ref, "revcomp",
     lambda b: None if b.strip(b"ACGTN") else b.translate(hgvs_ref.REVCOMP)),
]


@pytest.mark.parametrize("name", sorted(SEEDS))
def test_expected_repeats_itself(runs, name):
    """unbent, a second expected() equals the first: what the mutations change, they change"""
    assert _noticing(*runs[name]) == []


@pytest.mark.parametrize("name,what,module,attr,value", MUTATIONS, ids=[m[1] for m in MUTATIONS])
def test_a_bent_restatement_is_noticed(runs, monkeypatch, name, what, module, attr, value):
    fz, pairs = runs[name]
    monkeypatch.setattr(module, attr, value)
    seeds = _noticing(fz, pairs)
    print(f"\n{name}: '{what}' changes expected() for {len(seeds)} of {len(pairs)} seeds")
    assert seeds, what


# ---- 4. the generators are pure ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SEEDS))
def test_make_case_repeats_itself(runs, name):
    fz, pairs = runs[name]
    case = pairs[3][0]
    again = fz.make_case(case["seed"])
    assert sorted(again) == sorted(case)
    for k in case:
        assert again[k] == case[k], k
    assert fz.make_case(case["seed"] + 1) != case
