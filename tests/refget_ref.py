"""Plain-Python restatement of K21 (gtars_amd.refget): the FASTA record walk and the FAI rule (gtars-refget/src/digest/
fasta.rs:120-306), the alphabet table (alphabet.rs:194-304, 488-527), the collection digests (types.rs:204-347 over the
canonical JSON of algorithms.rs:59-110) and the substring rule (store/readonly.rs:1292-1352, store/export.rs:88-126).
hashlib, base64 and json only; nothing of the library is imported here."""
import base64
import hashlib
import json

DNA2BIT, DNA3BIT, DNAIO, PROTEIN, ASCII = range(5)
ALPHABET_NAMES = ("dna2bit", "dna3bit", "dnaio", "protein", "ASCII")
SUB_OK, SUB_NO_SEQUENCE, SUB_BAD_RANGE = 0, 1, 2
WS = b" \t\n\x0b\x0c\r"  # the ASCII part of char::is_whitespace

# The reference's arrays, restated as the bytes they map to a non-zero code (the arrays hold both letter cases; the guesser
# upper-cases before it looks a byte up, so the upper-case letters are what counts):
#   DNA_IUPAC_ENCODING_ARRAY: A C G T U R Y S W K M B D H V are non-zero, N is 0b0000
#   PROTEIN_ENCODING_ARRAY:   A is 0b00000; C D E F G H I K L M N P Q R S T V W Y * X - . are non-zero
IUPAC_NONZERO = b"ACGTURYSWKMBDHV"
PROTEIN_NONZERO = b"CDEFGHIKLMNPQRSTVWY*X-."


def class_of_upper(b: int) -> int:
    """get_minimum_alphabet_for_char, in its order of checks"""
    if b in b"ACGT":
        return DNA2BIT
    if b in b"NRY":
        return DNA3BIT
    if b in IUPAC_NONZERO or b == ord("N"):
        return DNAIO
    if b in PROTEIN_NONZERO or b in b"-*":
        return PROTEIN
    return ASCII


def upper(b: int) -> int:
    return b - 32 if 97 <= b <= 122 else b


# the class of every byte value: of its upper-cased form
CLASS_TABLE = bytes(class_of_upper(upper(b)) for b in range(256))
# ... stated: the 256 entries, 16 per row (4 = ASCII everywhere but at * - . and the letters)
CLASS_TABLE_STATED = bytes(
    [4] * 32 +
    [4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 3, 4, 4, 3, 3, 4] +          # 0x20: * - .
    [4] * 16 +
    #  @  A  B  C  D  E  F  G  H  I  J  K  L  M  N  O
    [4, 0, 2, 0, 2, 3, 3, 0, 2, 3, 4, 2, 3, 2, 1, 4] +
    #  P  Q  R  S  T  U  V  W  X  Y  Z
    [3, 3, 1, 2, 0, 2, 2, 2, 3, 1, 4, 4, 4, 4, 4, 4] +
    [4, 0, 2, 0, 2, 3, 3, 0, 2, 3, 4, 2, 3, 2, 1, 4] +          # lower case: as upper case
    [3, 3, 1, 2, 0, 2, 2, 2, 3, 1, 4, 4, 4, 4, 4, 4] +
    [4] * 128)
assert CLASS_TABLE == CLASS_TABLE_STATED


def guess_alphabet(data: bytes) -> int:
    """the most general class seen; an empty sequence is dna2bit"""
    return max((CLASS_TABLE[b] for b in data), default=DNA2BIT)


def sha512t24u(data: bytes) -> str:
    return base64.urlsafe_b64encode(hashlib.sha512(data).digest()[:24]).decode("ascii")


def md5(data: bytes) -> str:
    return hashlib.md5(data).hexdigest()


def ascii_upper(data: bytes) -> bytes:
    return bytes(upper(b) for b in data)


def walk_fasta(text: bytes, gzip_input: bool = False):
    """the records of a FASTA text in file order: dicts with name, description (None without one), sequence (upper-cased),
    length, sha512t24u, md5, alphabet and fai ((offset, line_bases, line_bytes), None for a record without a sequence line
    and for gzip input)"""
    recs, cur = [], None
    at = 0
    while at < len(text):
        nl = text.find(b"\n", at)
        end = len(text) if nl < 0 else nl + 1
        line = text[at:end]
        at = end
        if line[:1] == b">":
            header = line[1:].strip(WS)
            k = 0
            while k < len(header) and header[k] not in WS:
                k += 1
            cur = {"name": header[:k].decode("utf-8", "replace"),
                   "description": header[k + 1:].strip(WS).decode("utf-8", "replace") if k < len(header) else None,
                   "chunks": [], "fai": None, "offset": at}
            recs.append(cur)
        elif cur is not None and line.strip(WS):
            trimmed = line.rstrip(WS)
            if cur["fai"] is None:
                cur["fai"] = (cur["offset"], len(trimmed), len(line))
            cur["chunks"].append(trimmed)
    out = []
    for r in recs:
        seq = ascii_upper(b"".join(r["chunks"]))
        out.append({"name": r["name"], "description": r["description"], "sequence": seq, "length": len(seq), "sha512t24u": sha512t24u(seq),
                    "md5": md5(seq), "alphabet": guess_alphabet(seq), "fai": None if gzip_input else r["fai"]})
    return out


def canonical(value) -> bytes:
    """compact, keys sorted, integers in decimal, strings as serde_json writes them (UTF-8 passed through)"""
    return json.dumps(value, separators=(",", ":"), sort_keys=True, ensure_ascii=False).encode("utf-8")


def collection_digests(names, lengths, digests) -> dict:
    seqs = ["SQ." + d for d in digests]
    pairs = [{"length": n, "name": s} for s, n in zip(names, lengths)]
    lvl1 = {"names": sha512t24u(canonical(list(names))), "sequences": sha512t24u(canonical(seqs)),
            "lengths": sha512t24u(canonical(list(lengths)))}
    return {"top": sha512t24u(canonical({"names": lvl1["names"], "sequences": lvl1["sequences"]})), **lvl1,
            "name_length_pairs": sha512t24u(canonical(pairs)),
            "sorted_name_length_pairs": sha512t24u(canonical(sorted(sha512t24u(canonical(p)) for p in pairs))),
            "sorted_sequences": sha512t24u(canonical(sorted(seqs)))}


def digests_of_records(recs) -> dict:
    return collection_digests([r["name"] for r in recs], [r["length"] for r in recs], [r["sha512t24u"] for r in recs])


def substring(seq, start: int, end: int):
    """(status, bytes): start == end is the empty string wherever it lies, whatever the sequence; otherwise the row needs a
    sequence, start < end, start < len and end <= len.  A sequence the collection lacks is status 1 even for an empty range:
    the region calls look the name up first (export.rs:97-113)."""
    if seq is None:
        return SUB_NO_SEQUENCE, b""
    if start == end:
        return SUB_OK, b""
    if start >= len(seq) or end > len(seq) or start >= end:
        return SUB_BAD_RANGE, b""
    return SUB_OK, seq[start:end]


def last_by_name(recs) -> dict:
    """name -> record: a repeated name means its LAST record (the store's name map keeps one digest per name and a later
    insert replaces the value, store/readonly.rs:444-447)"""
    return {r["name"]: r for r in recs}


def region_substrings(recs, chroms, starts, ends):
    by = last_by_name(recs)
    return [substring(by[c]["sequence"] if c in by else None, s, e) for c, s, e in zip(chroms, starts, ends)]


def export_fasta_from_regions(recs, regions) -> bytes:
    """`>{chrom}:{start}-{end}` and the sequence per region (export.rs:293-327); every region must be valid"""
    out = []
    for (c, s, e), (st, seq) in zip(regions, region_substrings(recs, *zip(*regions))):
        assert st == SUB_OK, (c, s, e)
        out.append(b">%s:%d-%d\n%s\n" % (c.encode(), s, e, seq))
    return b"".join(out)
