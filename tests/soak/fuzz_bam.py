#!/usr/bin/env python3
"""Randomised differential soak of K17 (csrc/bam.hip): compute_bam_qc and BamFile.columns on random BAM files against the
pure Python writer, reader and bamqc restatement of tests/bam_ref.py -- integers equal, the three ratios bit-equal, every
column equal as int32.

A case is a whole file: 1 to 6 references (300 now and then; mitochondrial names and the near-miss chrM2 among them), 0 to about
1500 single-end and paired records with names from a small pool (repeats, shared prefixes, siblings that differ in the last
byte, `*`), pile-ups, pos -1, an unplaced tail, random CIGARs; BGZF blocks of 50, 333 or 0xFF00 bytes with cuts 1, 2 and 3 bytes
into a block_size field, between two records and inside a name; read through device windows of 1 byte to 256 MiB, on 1 or 4
host threads, with the name hash cut to 0 .. 33 bits.  About one case in twenty is the kernel's designed refusal: one record
whose n_cigar_op or l_read_name says more than its block_size holds; the call must raise, nothing else is damaged.

make_case(seed) and expected(case) need no device (tests/test_soak_generators_cpu.py runs them); run_device(case, tmp) does.

Run on the GPU box:  python tests/soak/fuzz_bam.py [rounds] [first_seed]"""
import os, random, shutil, struct, sys, tempfile, time
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np
import bam_ref as R

FIELDS = ("total_reads", "distinct", "m1", "m2", "dups", "mito_reads", "nrf", "pbc1", "pbc2")
PAIRED, PROPER, MATE_UNMAPPED, READ1, READ2, UNMAPPED, DUP = 0x1, 0x2, 0x8, 0x40, 0x80, 0x4, 0x400
REF_NAMES = ["chr1", "chr2", "chr3", "chrX", "ctgA", "chrM", "MT", "chrMt", "x_rCRSd_y", "chrM2"]
COUNTS = [0, 1, 2, 63, 64, 65, 256, 257, 1500]
BLOCKS = [50, 333, 0xFF00]
WINDOWS = [None, 1, 64, 500, 5000]
HASH_BITS = [None, "0", "1", "4", "33"]
DEFAULT_WINDOW = 256 << 20
REFUSAL = "longer than its block_size"


def coordinate_sorted(records):
    """stable: records of one position keep the order they were given in; the unplaced tail goes last"""
    return sorted(records, key=lambda r: (r["ref_id"] if r["ref_id"] >= 0 else 1 << 30, r["pos"]))


def name_pool(rng, k):
    """names of 1 to 254 bytes: three stems shared by many names, siblings that differ in their last byte only"""
    stems = [b"", b"frag_", bytes(rng.choice(b"ACGTxyz_:") for _ in range(rng.choice([1, 30, 200, 253])))]
    pool = [b"q", b"n" * 254][:rng.choice([0, 1, 2])]
    while len(pool) < k:
        name = (rng.choice(stems) + b"%d" % rng.randrange(10 ** rng.choice([1, 3, 6])))[:254]
        pool.append(name)
        if rng.random() < 0.3:
            pool.append(name[:-1] + bytes([name[-1] ^ 1]))
    return pool


def random_cigar(rng, l_seq):
    kind = rng.random()
    if kind < 0.1:
        return []
    if kind < 0.2:  # the placeholder of a CIGAR kept in a CG tag
        return [("S", max(l_seq, 1)), ("N", rng.choice([1000, (1 << 28) - 1]))]
    if kind < 0.6:
        return [("M", max(l_seq, 1))]
    return [(rng.choice(R.CIGAR_OPS), rng.randint(1, 200)) for _ in range(rng.randint(1, 40))]


def make_records(rng, n_ref, n):
    active = sorted(rng.sample(range(n_ref), min(n_ref, rng.choice([1, 1, 2, 3, 4]))))
    mode = {c: rng.choice(["single", "paired", "paired", "mixed", "read1"]) for c in active}
    span = {c: rng.choice([3, 3, 40, 40, 2000, 100_000]) for c in active}  # mostly pile-ups: keys collide
    pool = name_pool(rng, rng.choice([1, 2, 5, 30, 200, max(n, 1)]))
    tail = min(n, rng.choice([0, 0, 1, 5]))
    recs = []
    while len(recs) < n - tail:
        c = rng.choice(active)
        pos = rng.randrange(span[c]) if rng.random() > 0.03 else -1
        mapq = rng.choice([60, 60, 60, 60, 255, 30, 29, 0])
        extra = (DUP if rng.random() < 0.1 else 0) | (UNMAPPED if rng.random() < 0.04 else 0)
        name = b"*" if rng.random() < 0.04 else rng.choice(pool)
        l_seq = rng.choice([36, 36, 37, 10, 1, 0])
        kind = mode[c] if mode[c] != "mixed" else rng.choice(["single", "paired"])
        common = dict(ref_id=c, pos=pos, mapq=mapq, name=name, l_seq=l_seq, cigar=random_cigar(rng, l_seq))
        if kind == "single":
            recs.append(R.rec(flag=extra | rng.choice([0, 0, 0, READ1, READ2, PROPER, MATE_UNMAPPED]), tlen=rng.choice([0, 0, 50, -50]), **common))
        elif kind == "read1":
            recs.append(R.rec(flag=PAIRED | READ1 | extra | rng.choice([0, PROPER, MATE_UNMAPPED]), tlen=rng.choice([50, 51, -50]), **common))
        elif rng.random() < 0.6 and len(recs) + 2 <= n - tail:  # both mates
            pos2 = pos + rng.choice([0, 1, 50]) if pos >= 0 else rng.randrange(span[c])
            tlen = rng.choice([50, 51, -50, 0, 300])
            recs.append(R.rec(flag=PAIRED | PROPER | READ1 | extra, tlen=tlen, next_ref_id=c, next_pos=pos2, **common))
            recs.append(R.rec(flag=PAIRED | PROPER | READ2 | (DUP if rng.random() < 0.05 else 0), tlen=-tlen, next_ref_id=c, next_pos=pos,
                              **dict(common, pos=pos2, cigar=random_cigar(rng, l_seq))))
        else:  # one mate, or a paired record that says neither or both
            which = rng.choice([READ1, READ2, READ1, READ2, READ1 | READ2, 0, READ1 | MATE_UNMAPPED, READ2 | MATE_UNMAPPED])
            recs.append(R.rec(flag=PAIRED | which | extra, tlen=rng.choice([50, 51, -50, -51, 0]), **common))
    for _ in range(tail):
        recs.append(R.rec(ref_id=-1, pos=-1, mapq=0, flag=UNMAPPED | rng.choice([0, PAIRED | READ1, PAIRED | READ2, DUP]), name=rng.choice(pool),
                          cigar=[], l_seq=rng.choice([36, 0])))
    return coordinate_sorted(recs)


def windows_of(blocks, first_record, max_window):
    """csrc/bam.hip, BamPipe::fill: whole blocks of at most max_window inflated bytes, one at least; the first window also holds
    every block the header reaches into -> the inflated offset at which each window ends"""
    ends, b0 = [], 0
    while b0 < len(blocks):
        b1, size = b0, 0
        while b1 < len(blocks) and (b1 == b0 or size + blocks[b1][2] <= max_window or blocks[b1][4] < first_record):
            size += blocks[b1][2]
            b1 += 1
        ends.append(blocks[b1 - 1][4] + blocks[b1 - 1][2])
        b0 = b1
    return ends


def case_tags(case, blocks):
    """the edges this case sits on, from its records, its block table and its switches"""
    recs, refs, starts, sizes = case["records"], case["refs"], case["starts"], case["sizes"]
    tags = {"n=%d" % len(recs), "block=%d" % case["block"], "window=%s" % case["max_window_bytes"], "threads=%d" % case["threads"],
            "hash_bits=%s" % case["switches"].get("GTARS_BAM_NAME_HASH_BITS", "unset")}
    if len(refs) >= 300:
        tags.add("refs=300")
    if not recs:
        tags.add("empty_file")
    if case["refused"]:  # (the call stops at the refusal: the file's other edges are not counted)
        return tags | {"refusal"}
    bounds = {b[4] for b in blocks if b[4] > 0}
    for s, size, r in zip(starts, sizes, recs):
        for d in (1, 2, 3):
            if s + d in bounds:
                tags.add("cut+%d" % d)
        if s in bounds and s != starts[0]:
            tags.add("cut=record")
        if any(b in bounds for b in range(s + 37, s + 36 + len(r["name"]))):
            tags.add("cut_in_name")
    mw = case["max_window_bytes"] or DEFAULT_WINDOW
    if sizes and max(sizes) > mw:
        tags.add("window<record")
    ends = windows_of(blocks, case["first"], mw)
    window_of = {}
    k = 0
    for i, (s, size) in enumerate(zip(starts, sizes)):
        while ends[k] < s + size:
            k += 1
        window_of[i] = k  # the window in which the record is whole
    per_chrom = {}
    for i, r in enumerate(recs):
        per_chrom.setdefault(r["ref_id"], set()).add(window_of[i])
    if any(len(w) >= 3 for c, w in per_chrom.items() if c >= 0):
        tags.add("chrom>=3windows")
    for i in range(1, len(recs)):
        if recs[i]["ref_id"] != recs[i - 1]["ref_id"] and window_of[i] == window_of[i - 1] and recs[i]["ref_id"] >= 0:
            tags.add("chrom_change_in_window")
    if any(r["ref_id"] < 0 for r in recs):
        tags.add("unplaced_tail")
    # what reaches the name tables of bamqc.rs: per chromosome, the read-1 and the read-2 names in file order
    for c, (chrom, _) in enumerate(refs):
        mine = [r for r in recs if r["ref_id"] == c]
        if not mine:
            continue
        if R.is_mitochondrial(chrom):
            tags.add("mito")
            continue
        kept = [r for r in mine if (r["mapq"] == 255 or r["mapq"] >= R.MIN_MAPQ) and not r["flag"] & UNMAPPED and r["pos"] != -1]
        if any(r["flag"] & PAIRED and r["name"] == b"*" for r in kept):
            tags.add("star_paired")
        if any(not r["flag"] & PAIRED for r in kept) and any(r["flag"] & PAIRED for r in kept):
            tags.add("single_and_paired_chrom")
        tables = ([r["name"] for r in kept if r["flag"] & PAIRED and r["name"] != b"*" and r["flag"] & READ1],
                  [r["name"] for r in kept if r["flag"] & PAIRED and r["name"] != b"*" and not r["flag"] & READ1 and r["flag"] & READ2])
        if tables[0] and not tables[1]:
            tags.add("read1_only_chrom")
        for t in tables:
            if any(t.count(x) >= 3 for x in set(t)):
                tags.add("name_x3")
            stems = {}
            for x in set(t):
                stems.setdefault(x[:-1], set()).add(x)
            if any(len(v) >= 2 for v in stems.values()):
                tags.add("last_byte_siblings")
            if len(set(t)) > 16:
                tags.add("names>16")
    return tags


def make_case(seed):
    """pure: the same file bytes, call arguments, switches and tags for the same seed"""
    rng = random.Random(seed)
    if rng.random() < 0.06:
        refs = [("ctg%03d" % i, 10_000_000) for i in range(300)]
        for k in rng.sample(range(300), 3):
            refs[k] = (rng.choice(REF_NAMES[5:]) + "_%d" % k if rng.random() < 0.5 else "rCRSd%d" % k, 16_569)
    else:
        refs = [(name, 10_000_000) for name in rng.sample(REF_NAMES, rng.randint(1, 6))]
    n = rng.choice(COUNTS)
    recs = make_records(rng, len(refs), n)
    head = len(R.encode_header(refs))
    sizes = [len(R.encode_record(r)) for r in recs]
    starts = []
    at = head
    for s in sizes:
        starts.append(at)
        at += s
    cuts = [rng.randrange(0, at + 1) for _ in range(rng.choice([0, 1, 3, 10]))]
    for _ in range(rng.choice([0, 2, 6]) if recs else 0):  # forced: inside a block_size field, between two records, inside a name
        i = rng.randrange(len(recs))
        inside = 36 + rng.randrange(1, len(recs[i]["name"])) if len(recs[i]["name"]) > 1 else 36
        cuts.append(starts[i] + rng.choice([1, 2, 3, 0, inside]))
    block = rng.choice(BLOCKS)
    stream = bytearray(R.bam_stream(refs, recs))
    refused = bool(recs) and rng.random() < 0.05
    if refused:  # one record's n_cigar_op or l_read_name says more than its block_size holds; nothing else is damaged
        i = rng.randrange(len(recs))
        body = sizes[i] - 4
        if rng.random() < 0.5 and 32 + 255 + 4 * len(recs[i]["cigar"]) > body:
            stream[starts[i] + 4 + 8] = 255
        else:
            struct.pack_into("<H", stream, starts[i] + 4 + 12, rng.choice([65535, (body - 32 - len(recs[i]["name"]) - 1) // 4 + 1]))
    data = R.bgzf_bytes(bytes(stream), sorted(cuts), True, block)
    first = rng.randint(0, len(recs))
    count = rng.choice([None, 0, rng.randint(0, len(recs) - first)])
    bits = rng.choice(HASH_BITS)
    case = dict(seed=seed, refs=refs, records=recs, data=data, block=block, starts=starts, sizes=sizes, first=head, refused=refused,
                max_window_bytes=rng.choice(WINDOWS), threads=rng.choice([1, 4]), col_first=first, col_count=count,
                switches={} if bits is None else {"GTARS_BAM_NAME_HASH_BITS": bits})
    case["tags"] = case_tags(case, R.read_blocks(data)[0])
    return case


def expected(case):
    """the restatement's answer from the file's own bytes (read back through the pure Python reader): the nine QC fields and
    the columns of the case's record range; None for the refusal case"""
    if case["refused"]:
        return None
    blocks, stream = R.read_blocks(case["data"])
    text, refs, first, offs, recs = R.parse_stream(stream)
    assert (refs, first, offs, recs) == (case["refs"], case["first"], case["starts"], case["records"]), ("reader round trip", case["seed"])
    a = case["col_first"]
    b = len(recs) if case["col_count"] is None else a + case["col_count"]
    return dict(qc=R.bam_qc_ref(refs, recs), columns=R.columns_ref(recs[a:b]))


def bits_of(x):
    return struct.pack("<d", x)


def run_device(case, tmp, want=None):
    import gtars_amd
    from gtars_amd import bam as B

    seed = case["seed"]
    want = expected(case) if want is None else want
    path = os.path.join(tmp, "fuzz_%d.bam" % seed)
    with open(path, "wb") as f:
        f.write(case["data"])
    os.environ.pop("GTARS_BAM_NAME_HASH_BITS", None)
    os.environ.update(case["switches"])
    gtars_amd.reload_env()
    kw = dict(threads=case["threads"], max_window_bytes=case["max_window_bytes"])
    try:
        if case["refused"]:
            try:
                B.compute_bam_qc(path, **kw)
            except ValueError as e:
                assert REFUSAL in str(e), ("bam refusal text", seed, str(e))
            else:
                raise AssertionError(("bam refusal: the call returned", seed))
            return
        res = B.compute_bam_qc(path, **kw)
        got = {k: getattr(res, k) for k in FIELDS}
        for k in FIELDS[:6]:
            assert type(got[k]) is int and got[k] == want["qc"][k], ("bam qc", seed, k, got[k], want["qc"][k])
        for k in FIELDS[6:]:
            assert bits_of(got[k]) == bits_of(want["qc"][k]), ("bam qc", seed, k, got[k], want["qc"][k])
        with B.BamFile(path) as b:
            cols = b.columns(first=case["col_first"], count=case["col_count"], threads=case["threads"], max_window_bytes=case["max_window_bytes"])
        assert sorted(cols) == sorted(want["columns"]), ("bam columns", seed)
        for k, w in want["columns"].items():
            assert cols[k].dtype == np.int32 and np.array_equal(cols[k], w), ("bam column", seed, k)
    finally:
        os.remove(path)


def one(seed, tmp=None):
    own = tmp is None
    tmp = tempfile.mkdtemp(prefix="gtars_fuzzbam_") if own else str(tmp)
    try:
        case = make_case(seed)
        run_device(case, tmp, expected(case))
        return case["tags"]
    finally:
        if own:
            shutil.rmtree(tmp, ignore_errors=True)


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    base = int(sys.argv[2]) if len(sys.argv) > 2 else 17_000
    t = time.time()
    tags = set()
    tmp = tempfile.mkdtemp(prefix="gtars_fuzzbam_")
    try:
        for seed in range(rounds):
            tags |= one(base + seed, tmp)
            if seed % 25 == 24:
                print(f"  {seed + 1} rounds, {time.time() - t:.0f} s", flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    print(f"fuzz_bam: {rounds} random files (seeds {base} .. {base + rounds - 1}) bit-exact vs bam_ref, {len(tags)} tags ({time.time() - t:.0f} s)")


if __name__ == "__main__":
    main()
