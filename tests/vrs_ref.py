"""Plain-Python restatement of K18 (VRS allele identifiers), written from the rules and not from the library: hashlib and
base64 for the digests, a direct ``normalize`` over bytes, the VCF line rules.  No import of the library.

Rules restated (the reference's files are cited in DESIGN.md, K18):
  * sha512t24u = base64url, unpadded, of the first 24 bytes of SHA-512;
  * the SequenceLocation and Allele digests hash canonical JSON texts with sorted keys and no spaces;
  * normalize: check start + len(REF) against u64 and against the sequence, compare REF with the sequence upper-cased on
    both sides, trim the common prefix, then the common suffix, then roll left and right while the next base equals every
    non-empty trimmed allele at its circular index; the sequence is read upper-cased, alleles are used as given;
  * a VCF line yields alleles unless it is empty, starts with '#', has fewer than 5 tab-separated fields, or its POS is not
    a u64 >= 1; an ALT piece is kept unless it is empty, starts with '<', or is '*' or '.'."""
import base64
import gzip
import hashlib
import re

OK, START_OUT_OF_BOUNDS, REF_PAST_END, REF_MISMATCH, UNKNOWN_CHROMOSOME, BAD_ALLELE = range(6)
U64 = 1 << 64


def sha512t24u(data: bytes) -> str:
    return base64.urlsafe_b64encode(hashlib.sha512(data).digest()[:24]).decode("ascii")


def location_text(accession: str, start: int, end: int) -> bytes:
    return ('{"end":%d,"sequenceReference":{"refgetAccession":"%s","type":"SequenceReference"},"start":%d,"type":"SequenceLocation"}'
            % (end, accession, start)).encode()


def allele_text(loc_digest: str, sequence: bytes) -> bytes:
    return b'{"location":"' + loc_digest.encode() + b'","state":{"sequence":"' + sequence + b'","type":"LiteralSequenceExpression"},"type":"Allele"}'


def location_digest(accession: str, start: int, end: int) -> str:
    return sha512t24u(location_text(accession, start, end))


def vrs_digest(accession: str, start: int, end: int, sequence) -> str:
    sequence = sequence.encode() if isinstance(sequence, str) else bytes(sequence)
    return sha512t24u(allele_text(location_digest(accession, start, end), sequence))


def vrs_id(accession: str, start: int, end: int, sequence) -> str:
    return "ga4gh:VA." + vrs_digest(accession, start, end, sequence)


class NormalizeError(ValueError):
    def __init__(self, status, text):
        super().__init__(text)
        self.status = status


def normalize(sequence: bytes, start: int, ref: bytes, alt: bytes):
    """-> (new start, new end, new allele); NormalizeError otherwise"""
    n = len(sequence)
    s, e = start, start + len(ref)
    if e >= U64:
        raise NormalizeError(START_OUT_OF_BOUNDS, f"start position {start} exceeds sequence length {n}")
    if e > n:
        raise NormalizeError(REF_PAST_END, f"ref allele (start={start}, len={len(ref)}) extends past sequence length {n}")
    actual = sequence[s:e].upper()
    if ref.upper() != actual:
        raise NormalizeError(REF_MISMATCH, f"ref allele mismatch at interbase {start}: VCF says {ref.decode()}, reference has {actual.decode()}")
    while ref and alt and ref[0] == alt[0]:
        ref, alt, s = ref[1:], alt[1:], s + 1
    while ref and alt and ref[-1] == alt[-1]:
        ref, alt, e = ref[:-1], alt[:-1], e - 1
    alleles = [a for a in (ref, alt) if a]
    left = right = 0
    if alleles:
        while left < s:
            base = sequence[s - 1 - left:s - left].upper()[0]
            if any(a[-((left + 1) % len(a))] != base if (left + 1) % len(a) else a[0] != base for a in alleles):
                break
            left += 1
        while e + right < n:
            base = sequence[e + right:e + right + 1].upper()[0]
            if any(a[right % len(a)] != base for a in alleles):
                break
            right += 1
    return s - left, e + right, sequence[s - left:s].upper() + alt + sequence[e:e + right].upper()


def refget_digests(seqs: dict) -> dict:
    return {name: sha512t24u(s.upper()) for name, s in seqs.items()}


def alleles(seqs: dict, accessions: dict, rows):
    """rows of (chrom, start, ref, alt) -> (statuses, starts, ends, sequences, ids); a failed row has None id"""
    out = [], [], [], [], []
    for chrom, start, ref, alt in rows:
        if chrom not in seqs or chrom not in accessions:
            st, ns, ne, seq = UNKNOWN_CHROMOSOME, 0, 0, b""
        else:
            try:
                ns, ne, seq = normalize(seqs[chrom], start, ref, alt)
                st = OK
            except NormalizeError as err:
                st, ns, ne, seq = err.status, 0, 0, b""
        vid = vrs_id("SQ." + accessions[chrom], ns, ne, seq) if st == OK else None
        for col, v in zip(out, (st, ns, ne, seq, vid)):
            col.append(v)
    return out


def open_vcf_bytes(data: bytes) -> bytes:
    """plain, gzip or BGZF by the magic bytes (concatenated members are one stream)"""
    return gzip.decompress(data) if data[:2] == b"\x1f\x8b" else data


POS = re.compile(rb"\+?[0-9]+\Z")


def parse_vcf(text: bytes, known):
    """-> rows of (chrom, 0-based pos, ref, alt) in file order; ``known``: the chromosome names that are kept"""
    rows = []
    for line in text.split(b"\n"):
        line = line.rstrip(b"\r\n")
        if not line or line.startswith(b"#"):
            continue
        f = line.split(b"\t", 5)
        if len(f) < 5:
            continue
        if not POS.match(f[1]) or not 1 <= int(f[1]) < U64:
            continue
        chrom = f[0].decode()
        if chrom not in known:
            continue
        for alt in f[4].split(b","):
            if not alt or alt.startswith(b"<") or alt in (b"*", b"."):
                continue
            rows.append((chrom, int(f[1]) - 1, f[3], alt))
    return rows


def compute_vrs_ids(vcf_bytes: bytes, seqs: dict, accessions: dict):
    """-> rows of (chrom, pos, ref, alt, id); ValueError for the first allele that does not normalize"""
    out = []
    for chrom, pos, ref, alt in parse_vcf(open_vcf_bytes(vcf_bytes), set(seqs) & set(accessions)):
        try:
            ns, ne, seq = normalize(seqs[chrom], pos, ref, alt)
        except NormalizeError as err:
            raise ValueError(f"Failed to normalize variant at {chrom}:{pos + 1}: {err}") from None
        out.append((chrom, pos, ref.decode(), alt.decode(), vrs_id("SQ." + accessions[chrom], ns, ne, seq)))
    return out
