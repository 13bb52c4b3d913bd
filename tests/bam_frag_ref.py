"""K26 restated in pure Python: BAM records with aux data, the aux walk of SAM specification section 4.2.4, and fragments_ref
-- the rule of DESIGN.md section 3 K26, statement by statement.  Built on bam_ref (unchanged); nothing here touches the
library.

A record is bam_ref's dict with one more key: aux, the bytes behind the qualities (default b"")."""
import struct

import bam_ref as R

REASONS = ("unplaced", "flag", "mapq", "mate_ref", "not_leftmost", "too_long", "no_barcode", "empty")
STATS = ("records",) + REASONS + ("kept_pairs", "fragments", "barcodes")
DEFAULTS = dict(barcode_tag="CB", min_mapq=30, max_fragment_length=2000, shift=(4, -5), require_flags=0x3, exclude_flags=0xB0C, sample="bulk")


class Malformed(Exception):
    """aux data that the walk cannot follow inside the record"""


# ---- writer ---------------------------------------------------------------------------------------------------------
def rec(aux=b"", **kw):
    r = R.rec(**kw)
    r["aux"] = bytes(aux)
    return r


def encode_record(r):
    """bam_ref.encode_record's bytes with the aux bytes appended and block_size rewritten"""
    base = R.encode_record(r)
    body = base[4:] + r.get("aux", b"")
    return struct.pack("<I", len(body)) + body


def bam_stream(refs, records, text=""):
    return R.encode_header(refs, text) + b"".join(encode_record(r) for r in records)


def write_bam(path, refs, records, cuts=None, block=0xFF00):
    data = R.bgzf_bytes(bam_stream(refs, records), cuts, True, block)
    with open(path, "wb") as f:
        f.write(data)
    return data


def _tag(tag):
    t = tag.encode() if isinstance(tag, str) else bytes(tag)
    assert len(t) == 2
    return t


def aux_A(tag, ch):
    return _tag(tag) + b"A" + bytes([ch if isinstance(ch, int) else ord(ch)])


def aux_int(tag, type_, v):
    return _tag(tag) + type_.encode() + struct.pack({"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[type_], v)


def aux_f(tag, v):
    return _tag(tag) + b"f" + struct.pack("<f", v)


def aux_Z(tag, value):
    v = value.encode() if isinstance(value, str) else bytes(value)
    assert 0 not in v
    return _tag(tag) + b"Z" + v + b"\0"


def aux_H(tag, hexdigits):
    return _tag(tag) + b"H" + hexdigits.encode() + b"\0"


def aux_B(tag, sub, values):
    fmt = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[sub]
    return _tag(tag) + b"B" + sub.encode() + struct.pack("<I", len(values)) + struct.pack("<%d%s" % (len(values), fmt), *values)


# ---- reader ---------------------------------------------------------------------------------------------------------
def parse_stream(s):
    """bam_ref.parse_stream, every record with its aux bytes: -> refs, records"""
    _text, refs, _first, offs, recs = R.parse_stream(s)
    for at, r in zip(offs, recs):
        bs = struct.unpack_from("<I", s, at)[0]
        l_name, n_cig, l_seq = s[at + 12], struct.unpack_from("<H", s, at + 16)[0], struct.unpack_from("<I", s, at + 20)[0]
        aux = 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
        r["aux"] = s[at + 4 + aux:at + 4 + bs] if aux <= bs else None  # (None: the aux area starts beyond block_size)
    return refs, recs


def read_bam(path):
    with open(path, "rb") as f:
        _blocks, stream = R.read_blocks(f.read())
    return parse_stream(stream)


# ---- the aux walk (SAM specification section 4.2.4) -----------------------------------------------------------------------
FIXED = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


def aux_value_size(aux, at, type_):
    """bytes of the value that starts at aux[at]; Malformed when it does not end inside aux"""
    left = len(aux) - at
    if type_ in FIXED:
        n = FIXED[type_]
    elif type_ in "ZH":
        nul = aux.find(b"\0", at)
        if nul < 0:
            raise Malformed("Z / H without NUL")
        n = nul - at + 1
    elif type_ == "B":
        if left < 5:
            raise Malformed("B header cut")
        sub = chr(aux[at])
        if sub not in FIXED or sub == "A":
            raise Malformed("unknown B subtype")
        n = 5 + struct.unpack_from("<I", aux, at + 1)[0] * FIXED[sub]
    else:
        raise Malformed("unknown type")
    if n > left:
        raise Malformed("value reaches past block_size")
    return n


def aux_entries(aux):
    """[(tag, type, value bytes)] of a whole aux area"""
    out, at = [], 0
    while at < len(aux):
        if len(aux) - at < 3:
            raise Malformed("entry header cut")
        tag, type_ = aux[at:at + 2], chr(aux[at + 2])
        n = aux_value_size(aux, at + 3, type_)
        out.append((tag, type_, aux[at + 3:at + 3 + n]))
        at += 3 + n
    return out


def find_barcode(aux, tag):
    """step 7: the first entry whose tag is `tag` decides -> the barcode's bytes, or None (no_barcode).  Entries behind it are
    not looked at; the ones up to it must be well-formed."""
    if aux is None:
        raise Malformed("aux start beyond block_size")
    at = 0
    while at < len(aux):
        if len(aux) - at < 3:
            raise Malformed("entry header cut")
        t, type_ = aux[at:at + 2], chr(aux[at + 2])
        n = aux_value_size(aux, at + 3, type_)
        if t == tag:
            if type_ == "Z" and n > 1:
                return aux[at + 3:at + 3 + n - 1]
            return None
        at += 3 + n
    return None


# ---- the rule ---------------------------------------------------------------------------------------------------------
def classify(refs, r, barcode_tag, min_mapq, max_fragment_length, shift, require_flags, exclude_flags, sample):
    """one record -> a reason (str) or the kept pair (ref, start, end, barcode bytes)"""
    if r["ref_id"] < 0:
        return "unplaced"
    if (r["flag"] & require_flags) != require_flags or r["flag"] & exclude_flags:
        return "flag"
    if r["mapq"] < min_mapq:
        return "mapq"
    if r["next_ref_id"] != r["ref_id"]:
        return "mate_ref"
    if r["tlen"] <= 0:
        return "not_leftmost"
    if r["tlen"] > max_fragment_length:
        return "too_long"
    if barcode_tag is None:
        barcode = sample.encode()
    else:
        barcode = find_barcode(r.get("aux", b""), _tag(barcode_tag))
        if barcode is None:
            return "no_barcode"
    start = max(r["pos"] + shift[0], 0)
    end = min(r["pos"] + r["tlen"] + shift[1], refs[r["ref_id"]][1])
    if start >= end:
        return "empty"
    return (r["ref_id"], start, end, barcode)


def fragments_ref(refs, records, **params):
    """-> rows [(ref, start, end, barcode id, count)], barcodes [bytes] in id order, stats dict, text bytes.  Malformed is
    raised for aux data the walk cannot follow."""
    p = dict(DEFAULTS, **params)
    stats = dict.fromkeys(STATS, 0)
    counts = {}
    for r in records:
        stats["records"] += 1
        out = classify(refs, r, **p)
        if isinstance(out, str):
            stats[out] += 1
        else:
            stats["kept_pairs"] += 1
            counts[out] = counts.get(out, 0) + 1
    barcodes = sorted({k[3] for k in counts})  # (bytes compare bytewise, a prefix before the longer string)
    ids = {b: i for i, b in enumerate(barcodes)}
    rows = [(ref, start, end, ids[b], counts[(ref, start, end, b)]) for ref, start, end, b in sorted(counts)]
    stats["fragments"], stats["barcodes"] = len(rows), len(barcodes)
    text = b"".join(b"%s\t%d\t%d\t%s\t%d\n" % (refs[ref][0].encode(), start, end, barcodes[b], c) for ref, start, end, b, c in rows)
    return rows, barcodes, stats, text
