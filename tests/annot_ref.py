"""Plain-Python restatement of the reference's TSS / feature distances and GTF gene models (gtars-genomicdist/src/
models.rs:516-690, partitions.rs:123-340, stranded_region_set.rs:84-135; gtars-python/src/models/{tss_index,gene_model,
gda}.rs), the yardstick of tests/test_annot_cpu.py and tests/test_gpu_annot.py.

Regions are (chr, start, end) tuples with u32 coordinates; arithmetic wraps as in the reference's release build.  The
distances come in two forms, a brute-force O(n * m) one and a ``bisect`` one, which the CPU tests check against each
other.  Nothing here needs a choice the reference leaves open.
"""
import bisect
import gzip

U32 = 0xFFFFFFFF
I64_MAX = (1 << 63) - 1
GENE, EXON, THREE_UTR, FIVE_UTR, UTR, CDS = range(6)
FEATURES = {"gene": GENE, "exon": EXON, "three_prime_utr": THREE_UTR, "five_prime_utr": FIVE_UTR, "UTR": UTR, "CDS": CDS}
PLUS, MINUS, UNSTRANDED = 0, 1, 2


def midpoint(s, e):
    """Region::mid_point_with_mode(Bed): start + width / 2, width = end - start, both wrapping in u32"""
    return (s + ((e - s) & U32) // 2) & U32


def first_appearance_order(regs):
    """iter_chroms then iter_chr_regions: indices by chromosome of first appearance, set order within one"""
    rank = {}
    for c, _, _ in regs:
        rank.setdefault(c, len(rank))
    return sorted(range(len(regs)), key=lambda i: rank[regs[i][0]])


def build_index(regs):
    """TssIndex::from_region_set: chromosome -> sorted midpoints, duplicates kept"""
    idx = {}
    for c, s, e in regs:
        idx.setdefault(c, []).append(midpoint(s, e))
    for v in idx.values():
        v.sort()
    return idx


def distances(index, query):
    """(calc_tss_distances, feature_distances) with bisect, as the reference's binary search does it; absolute u32
    (U32 where the index lacks the chromosome) and signed feature - query (None there)"""
    out_abs, out_signed = [], []
    for i in first_appearance_order(query):
        c, s, e = query[i]
        mids = index.get(c)
        if mids is None:
            out_abs.append(U32)
            out_signed.append(None)
            continue
        t = midpoint(s, e)
        p = bisect.bisect_left(mids, t)
        if p < len(mids) and mids[p] == t:
            out_abs.append(0)
            out_signed.append(0.0)
            continue
        left = t - mids[p - 1] if p > 0 else None
        right = mids[p] - t if p < len(mids) else None
        if left is not None and (right is None or left <= right):
            out_abs.append(left)
            out_signed.append(float(-left))
        else:
            out_abs.append(right)
            out_signed.append(float(right))
    return out_abs, out_signed


def distances_brute(index_regs, query):
    """the same from every (query, feature) pair: the smallest |feature - query|, upstream on a tie"""
    mids = {}
    for c, s, e in index_regs:
        mids.setdefault(c, []).append(midpoint(s, e))
    out_abs, out_signed = [], []
    for i in first_appearance_order(query):
        c, s, e = query[i]
        if c not in mids:
            out_abs.append(U32)
            out_signed.append(None)
            continue
        t = midpoint(s, e)
        d = min(abs(m - t) for m in mids[c])
        out_abs.append(d)
        out_signed.append(float(-d) if (t - d) in mids[c] else float(d))
    return out_abs, out_signed


# ------------------------------------------------------------------------------------------------------- GTF reader
def rust_parse_u32(s):
    """<u32 as FromStr>::from_str: (value, None) or (None, the ParseIntError message)"""
    if s == "":
        return None, "cannot parse integer from empty string"
    body = s[1:] if s[0] == "+" else s
    if body == "":
        return None, "invalid digit found in string"
    v = 0
    for ch in body:
        if not "0" <= ch <= "9":
            return None, "invalid digit found in string"
        v = v * 10 + ord(ch) - 48
        if v > U32:
            return None, "number too large to fit in target type"
    return v, None


def read_lines(data: bytes):
    """BufRead::lines(): split at b"\\n", strip "\\n" or "\\r\\n", each line decoded as UTF-8 (ValueError otherwise)"""
    pos = 0
    while pos < len(data):
        nl = data.find(b"\n", pos)
        if nl < 0:
            raw, pos = data[pos:], len(data)
        else:
            raw, pos = data[pos:nl], nl + 1
            if raw.endswith(b"\r"):
                raw = raw[:-1]
        try:
            yield raw.decode("utf-8")
        except UnicodeDecodeError:
            raise ValueError("stream did not contain valid UTF-8") from None


def parse_gtf(data: bytes, filter_protein_coding=True, convert_ensembl_ucsc=True):
    """the reader of GeneModel::from_gtf: kept rows (chr, start, end, strand, feature) in file order"""
    rows = []
    for line in read_lines(data):
        if line.startswith("#"):
            continue
        f = line.split("\t")
        if len(f) < 9 or f[2] not in FEATURES:
            continue
        if filter_protein_coding and 'gene_biotype "protein_coding"' not in f[8] and 'gene_type "protein_coding"' not in f[8]:
            continue
        chr_ = f[0]
        if convert_ensembl_ucsc and not chr_.startswith("chr"):
            chr_ = "chr" + chr_
        start, err = rust_parse_u32(f[3])
        if err:
            raise ValueError("Parsing GTF start: " + err)
        end, err = rust_parse_u32(f[4])
        if err:
            raise ValueError("Parsing GTF end: " + err)
        c = f[6][:1]
        rows.append((chr_, max(start - 1, 0), end, PLUS if c == "+" else MINUS if c == "-" else UNSTRANDED, FEATURES[f[2]]))
    return rows


def read_gtf(path, filter_protein_coding=True, convert_ensembl_ucsc=True):
    with open(path, "rb") as fh:
        data = fh.read()
    if str(path).endswith(".gz"):
        data = gzip.decompress(data)  # every member, like MultiGzDecoder
    return parse_gtf(data, filter_protein_coding, convert_ensembl_ucsc)


def stranded_reduce(regs):
    """StrandedRegionSet::reduce of (chr, start, end, strand): stable sort by (chr bytewise, strand, start), merge while
    same chr and strand and start <= current end (the running max of the ends)"""
    if not regs:
        return []
    order = sorted(regs, key=lambda r: (r[0].encode(), r[3], r[1]))
    out = []
    c, s, e, st = order[0][:4]
    for r in order[1:]:
        if r[0] == c and r[3] == st and r[1] <= e:
            e = max(e, r[2])
        else:
            out.append((c, s, e, st))
            c, s, e, st = r[:4]
    out.append((c, s, e, st))
    return out


def gene_model(rows):
    """(genes, exons) of GeneModel::from_gtf: each a stranded reduce of its rows"""
    genes = stranded_reduce([r for r in rows if r[4] == GENE])
    exons = stranded_reduce([r for r in rows if r[4] == EXON])
    return genes, exons


def tss_regions(genes):
    """PyGenomicDistAnnotation::tss_index: [p, p + 1) with p = end.saturating_sub(1) on Minus, start otherwise"""
    out = []
    for c, s, e, st in genes:
        p = max(e - 1, 0) if st == MINUS else s
        out.append((c, p, (p + 1) & U32))
    return out


def reduce_unstranded(regs):
    """RegionSet::reduce of (chr, start, end, ...) ignoring the strand, sorted by (chr, start)"""
    return [(c, s, e) for c, s, e, _ in stranded_reduce([(r[0], r[1], r[2], 0) for r in regs])]
