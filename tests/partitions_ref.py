"""Genomic partitions as the reference states them, in plain Python -- the checker for csrc/partitions.hip, the UTR reader
and the stranded setdiff.  Written as the loops of gtars-genomicdist/src/partitions.rs and stranded_region_set.rs: no
search, no prefix sums, a literal overlap test per row.  Stranded rows are (chr, start, end, strand) with annot_ref's
strand codes; a partition list is [(name, [(chr, start, end), ...]), ...].  u32 arithmetic is masked by hand where
the reference's release build wraps."""
import gzip
import math

from annot_ref import MINUS, PLUS, U32, UNSTRANDED, read_lines, rust_parse_u32, stranded_reduce

THREE, FIVE = 0, 1


def strand_of(ch):
    """Strand::from_char"""
    return PLUS if ch == "+" else MINUS if ch == "-" else UNSTRANDED


# ---- GeneModel (partitions.rs:63-349) --------------------------------------------------------------------------------
def transcript_id(attrs):
    marker = 'transcript_id "'
    at = attrs.find(marker)
    if at < 0:
        return None
    b = at + len(marker)
    e = attrs.find('"', b)
    return None if e < 0 else attrs[b:e]


def gtf_utr_rows(data: bytes, filter_protein_coding=True, convert_ensembl_ucsc=True):
    """(three_utr, five_utr) of GeneModel::from_gtf before their reduce, each a list of stranded rows"""
    three, five, pending, cds, tx_exons = [], [], [], {}, {}
    for line in read_lines(data):
        if line.startswith("#"):
            continue
        f = line.split("\t")
        if len(f) < 9 or f[2] not in ("gene", "exon", "three_prime_utr", "five_prime_utr", "UTR", "CDS"):
            continue
        if filter_protein_coding and 'gene_biotype "protein_coding"' not in f[8] and 'gene_type "protein_coding"' not in f[8]:
            continue
        chr_ = f[0]
        if convert_ensembl_ucsc and not chr_.startswith("chr"):
            chr_ = "chr" + chr_
        start, err = rust_parse_u32(f[3])
        if err:
            raise ValueError("Parsing GTF start: " + err)
        start = max(start - 1, 0)
        end, err = rust_parse_u32(f[4])
        if err:
            raise ValueError("Parsing GTF end: " + err)
        strand = strand_of(f[6][:1] or ".")
        strand_char = f[6][:1] or "+"
        tid = transcript_id(f[8])
        if f[2] == "exon" and tid is not None:
            tx_exons.setdefault(tid, []).append((chr_, start, end, strand_char))
        elif f[2] == "three_prime_utr":
            three.append((chr_, start, end, strand))
        elif f[2] == "five_prime_utr":
            five.append((chr_, start, end, strand))
        elif f[2] == "CDS" and tid is not None:
            lo, hi = cds.get(tid, (U32, 0))
            cds[tid] = (min(lo, start), max(hi, end))
        elif f[2] == "UTR" and tid is not None:
            pending.append((chr_, start, end, strand_char, tid))
    for chr_, start, end, ch, tid in pending:
        if tid not in cds:
            continue
        utr_mid, cds_mid = (start + end) // 2, (cds[tid][0] + cds[tid][1]) // 2
        is_five = utr_mid < cds_mid if ch == "+" else utr_mid > cds_mid
        (five if is_five else three).append((chr_, start, end, strand_of(ch)))
    if not five and not three:
        for tid, exons in tx_exons.items():
            if tid not in cds:
                continue
            cds_start, cds_end = cds[tid]
            for chr_, e_start, e_end, ch in exons:
                if e_start < cds_start:
                    (three if ch == "-" else five).append((chr_, e_start, min(e_end, cds_start), strand_of(ch)))
                if e_end > cds_end:
                    (five if ch == "-" else three).append((chr_, max(e_start, cds_end), e_end, strand_of(ch)))
    return three, five


def read_bytes(path):
    with open(path, "rb") as fh:
        data = fh.read()
    return gzip.decompress(data) if str(path).endswith(".gz") else data


def bed_stranded(path):
    """stranded_from_regionset of a BED file: strand from column 6 when rest has at least 3 fields"""
    rows = []
    with open(path) as fh:
        for line in fh:
            f = line.rstrip("\n").split("\t")
            if len(f) < 3:
                continue
            rest = f[3:]
            rows.append((f[0], int(f[1]), int(f[2]), strand_of(rest[2][:1] or ".") if len(rest) >= 3 else UNSTRANDED))
    return rows


def model_of(genes, exons, three=None, five=None):
    """a GeneModel as a dict of stranded-reduced sets; an empty UTR set is None"""
    return {"genes": stranded_reduce(genes), "exons": stranded_reduce(exons),
            "three_utr": stranded_reduce(three) if three else None, "five_utr": stranded_reduce(five) if five else None}


# ---- StrandedRegionSet (stranded_region_set.rs:16-217) ---------------------------------------------------------------
def promoters_stranded(regs, upstream, downstream):
    out = []
    for c, s, e, st in regs:
        if st == MINUS:
            out.append((c, max(e - downstream, 0), min(e + upstream, U32), st))
        else:
            out.append((c, max(s - upstream, 0), min(s + downstream, U32), st))
    return out


def trim_stranded(regs, chrom_sizes):
    out = []
    for c, s, e, st in regs:
        if c in chrom_sizes:
            s2, e2 = min(s, chrom_sizes[c]), min(e, chrom_sizes[c])
            if s2 < e2:
                out.append((c, s2, e2, st))
        else:
            out.append((c, s, e, st))
    return out


def stranded_setdiff(a_in, b_in):
    a, b = stranded_reduce(a_in), stranded_reduce(b_in)
    b_map = {}
    for r in b:
        b_map.setdefault((r[0], r[3]), []).append(r)
    out = []
    i = 0
    while i < len(a):
        chr_, strand = a[i][0], a[i][3]
        j = i
        while j < len(a) and a[j][0] == chr_ and a[j][3] == strand:
            j += 1
        bs = b_map.get((chr_, strand), [])
        b_idx = 0
        for _, a_start, a_end, _ in a[i:j]:
            while b_idx < len(bs) and bs[b_idx][2] <= a_start:
                b_idx += 1
            pos, k = a_start, b_idx
            while k < len(bs) and bs[k][1] < a_end and pos < a_end:
                if bs[k][1] > pos:
                    out.append((chr_, pos, bs[k][1], strand))
                pos = max(pos, bs[k][2])
                k += 1
            if pos < a_end:
                out.append((chr_, pos, a_end, strand))
        i = j
    return out


# ---- genome_partition_list (partitions.rs:410-483) -------------------------------------------------------------------
def unstrand(regs):
    return [(c, s, e) for c, s, e, _ in regs]


def partition_list(model, core_prom, prox_prom, chrom_sizes=None):
    def prom(size):
        raw = promoters_stranded(model["genes"], size, 0)
        return stranded_reduce(trim_stranded(raw, chrom_sizes) if chrom_sizes is not None else raw)

    core = prom(core_prom)
    parts = [("promoterCore", unstrand(core)), ("promoterProx", unstrand(stranded_setdiff(prom(prox_prom), core)))]
    three = stranded_reduce(model["three_utr"]) if model["three_utr"] is not None else None
    five = stranded_reduce(model["five_utr"]) if model["five_utr"] is not None else None
    if three is not None:
        parts.append(("threeUTR", unstrand(three)))
    if five is not None:
        parts.append(("fiveUTR", unstrand(stranded_setdiff(five, three) if three is not None else five)))
    exon = stranded_reduce(model["exons"])
    intron = stranded_reduce(model["genes"])
    for utr in (three, five):
        if utr is not None:
            exon = stranded_setdiff(exon, utr)
    parts.append(("exon", unstrand(exon)))
    for utr in (three, five):
        if utr is not None:
            intron = stranded_setdiff(intron, utr)
    intron = stranded_setdiff(intron, stranded_reduce(model["exons"]))
    parts.append(("intron", unstrand(intron)))
    return parts


# ---- calc_partitions (partitions.rs:493-592) -------------------------------------------------------------------------
def hits(c, qs, qe, rows):
    """the rows a query overlaps: same chromosome, row.start < q.end and row.end > q.start"""
    return [r for r in rows if r[0] == c and r[1] < qe and r[2] > qs]


def assignments(query, parts):
    """per query the index of the first partition with a hit, len(parts) for none"""
    out = []
    for c, qs, qe in query:
        a = len(parts)
        for pi, (_, rows) in enumerate(parts):
            if hits(c, qs, qe, rows):
                a = pi
                break
        out.append(a)
    return out


def calc_partitions(query, parts, bp_proportion=False):
    """-> (counts with intergenic last, total)"""
    if not bp_proportion:
        counts = [0] * (len(parts) + 1)
        for a in assignments(query, parts):
            counts[a] += 1
        return counts, len(query) & U32
    total = sum((qe - qs) & U32 for _, qs, qe in query) & U32
    counts, assigned = [], 0
    for _, rows in parts:
        bp = 0
        for c, qs, qe in query:
            for _, s, e in hits(c, qs, qe, rows):
                ol_start, ol_end = max(qs, s), min(qe, e)
                if ol_end > ol_start:
                    bp = (bp + ol_end - ol_start) & U32
        assigned = (assigned + bp) & U32
        counts.append(bp)
    counts.append(max(total - assigned, 0))
    return counts, total


# ---- calc_expected_partitions (partitions.rs:598-784) ----------------------------------------------------------------
LANCZOS = [0.99999999999980993, 676.5203681218851, -1259.1392167224028, 771.32342877765313, -176.61502916214059,
           12.507343278686905, -0.13857109526572012, 9.9843695780195716e-6, 1.5056327351493116e-7]


def ln_gamma(x):
    if x < 0.5:
        return math.log(math.pi / math.sin(math.pi * x)) - ln_gamma(1.0 - x)
    x -= 1.0
    total = LANCZOS[0]
    for i, c in enumerate(LANCZOS[1:]):
        total += c / (x + float(i) + 1.0)
    t = x + 7.5
    return 0.5 * math.log(2.0 * math.pi) + math.log(t) * (x + 0.5) - t + math.log(total)


def gamma_series(a, x, ln_gamma_a):
    total = term = 1.0 / a
    for n in range(1, 200):
        term *= x / (a + float(n))
        total += term
        if abs(term) < abs(total) * 1e-14:
            break
    return total * math.exp(-x + a * math.log(x) - ln_gamma_a)


def gamma_cf(a, x, ln_gamma_a):
    d = 1.0 / (x + 1.0 - a)
    c = 1.0 / 1e-30
    f = d
    for n in range(1, 200):
        an = -float(n) * (float(n) - a)
        bn = x + 2.0 * float(n) + 1.0 - a
        d = bn + an * d
        if abs(d) < 1e-30:
            d = 1e-30
        d = 1.0 / d
        c = bn + an / c
        if abs(c) < 1e-30:
            c = 1e-30
        delta = c * d
        f *= delta
        if abs(delta - 1.0) < 1e-14:
            break
    return min(max(f * math.exp(-x + a * math.log(x) - ln_gamma_a), 0.0), 1.0)


def regularized_gamma_lower(a, x):
    if x <= 0.0:
        return 0.0
    lg = ln_gamma(a)
    return gamma_series(a, x, lg) if x < a + 1.0 else 1.0 - gamma_cf(a, x, lg)


def chi_square_2x2(obs, exp, total):
    if total == 0.0 or exp == 0.0 or total - exp == 0.0:
        return 1.0
    non_obs, non_exp = total - obs, total - exp
    chi_sq = (obs - exp) ** 2 / exp + (non_obs - non_exp) ** 2 / non_exp
    return 1.0 - regularized_gamma_lower(0.5, chi_sq / 2.0)


def expected_rows(counts, total, partition_bp, genome_size):
    """-> (expected, log10OE, pvalue), one entry per count; partition_bp has one entry less (intergenic takes the rest)"""
    sizes = list(partition_bp) + [max(genome_size - sum(partition_bp), 0)]
    exp_, oe, pv = [], [], []
    for obs, bp in zip(counts, sizes):
        obs = float(obs)
        expected = (float(bp) / float(genome_size)) * float(total) if genome_size else float("nan")
        exp_.append(expected)
        oe.append(-math.inf if obs == 0.0 else math.inf if expected == 0.0 else math.log10(obs / expected))
        pv.append(chi_square_2x2(obs, expected, float(total)))
    return exp_, oe, pv


def calc_expected_partitions(query, parts, chrom_sizes, bp_proportion=False):
    counts, total = calc_partitions(query, parts, bp_proportion)
    partition_bp = [sum((e - s) & U32 for _, s, e in rows) for _, rows in parts]
    return (counts,) + expected_rows(counts, total, partition_bp, sum(chrom_sizes.values()))
