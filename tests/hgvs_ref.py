"""K20 restated in plain Python, the way the reference computes it: a recursive-descent parser over the string as in
gtars-vrs/src/hgvs/parser.rs (nucleotide grammar; a protein expression stops behind its "p."), and the genome path of the
bridge as in bridge.rs:552-923 over the restatements of K18 and K19 (vrs_ref.normalize / vrs_id, reftx_ref.c_to_g / n_to_g),
with slices and bytes.translate where the library walks bytes.  No import of the library.  Statuses are the library's
(csrc/hgvs_core.h)."""
import reftx_ref as R
import vrs_ref as V

(OK, PARSE_ERROR, UNSUPPORTED_REFERENCE_TYPE, UNSUPPORTED_EDIT, TRANSCRIPT_NOT_FOUND, NO_MANE_TRANSCRIPT, UNKNOWN_CHROM, MAPPING_ERROR,
 OUT_OF_BOUNDS, INCONSISTENT_EDIT, REF_MISMATCH, NORMALIZE_ERROR) = range(12)
STATUS_NAMES = ("ok", "parse_error", "unsupported_reference_type", "unsupported_edit", "transcript_not_found", "no_mane_transcript",
                "unknown_chromosome", "mapping_error", "out_of_bounds", "inconsistent_edit", "ref_mismatch", "normalize_error")
IUPAC = set(b"ACGTUNacgtunRYSWKMBDHVryswkmbdhv")
I64 = 1 << 63
U64 = 1 << 64


class ParseError(ValueError):
    def __init__(self, pos, msg, text):
        super().__init__(f"HGVS parse error at position {pos}: {msg} (in: \"{text}\")")
        self.pos, self.msg = pos, msg


class Protein(Exception):
    """a p. expression: the accession and the gene are read, the rest is not"""

    def __init__(self, accession, gene):
        self.accession, self.gene = accession, gene


def _i64(v):
    """`as i64` of a u64, and a negation that wraps"""
    v &= U64 - 1
    return v - U64 if v >= I64 else v


class _Parser:
    def __init__(self, text: bytes):
        self.s, self.pos = text, 0

    def err(self, msg):
        return ParseError(self.pos, msg, self.s.decode("utf-8", "replace"))

    def peek(self):
        return self.s[self.pos] if self.pos < len(self.s) else None

    def eat(self, ch):
        if self.peek() == ord(ch):
            self.pos += 1
            return True
        return False

    def expect(self, ch, msg):
        if not self.eat(ch):
            raise self.err(msg)

    def keyword(self, kw):
        if self.s.startswith(kw, self.pos):
            self.pos += len(kw)
            return True
        return False

    def digits(self):
        start = self.pos
        while self.peek() is not None and 48 <= self.peek() <= 57:
            self.pos += 1
        return self.s[start:self.pos]

    def uint(self):
        d = self.digits()
        if not d:
            raise self.err("expected integer")
        if int(d) >= U64:
            raise self.err("invalid integer")
        return int(d)

    def run(self):
        start = self.pos
        while self.peek() in IUPAC:
            self.pos += 1
        return self.s[start:self.pos].decode()

    def position(self, rt):
        datum = "cds" if rt == "c" else "seq_start"
        if rt == "c" and self.eat("*"):
            datum = "cds_stop"
        neg = False
        if self.peek() == ord("-"):
            neg, self.pos = True, self.pos + 1
        elif self.peek() == ord("+"):
            self.pos += 1
        base = _i64(self.uint())
        base = _i64(-base) if neg else base
        offset = 0
        if self.peek() in (ord("+"), ord("-")):
            minus = self.peek() == ord("-")
            self.pos += 1
            offset = _i64(self.uint())
            offset = _i64(-offset) if minus else offset
        return {"base": base, "offset": offset, "datum": datum}

    def pair(self, rt):
        low = None if self.eat("?") else self.position(rt)
        self.expect("_", "expected `_` in uncertain position range")
        high = None if self.eat("?") else self.position(rt)
        return low, high

    def bound(self, rt, prefer_high):
        """one side of a location -> (PositionBound dict, its main position)"""
        if self.eat("("):
            low, high = self.pair(rt)
            self.expect(")", "expected `)` after uncertain position")
            main = (high or low) if prefer_high else (low or high)
            if main is None:
                raise self.err("both bounds unknown")
            return {"kind": "uncertain", "position": None, "low": low, "high": high}, main
        p = self.position(rt)
        return {"kind": "certain", "position": p, "low": None, "high": None}, p

    def location(self, rt):
        start, main = self.bound(rt, True)
        if not self.eat("_"):
            return "single", {"kind": "certain", "position": main, "low": None, "high": None}, None
        end, _ = self.bound(rt, False)
        return "range", start, end

    def edit(self):
        e = lambda kind, ref=None, alt=None: {"kind": kind, "ref": ref, "alt": alt}  # noqa: E731
        if self.eat("="):
            return e("identity")
        if self.eat("?"):
            return e("unknown")
        if self.keyword(b"delins"):
            alt = self.run()
            if not alt:
                raise self.err("expected nucleotide sequence")
            return e("delins", None, alt)
        if self.keyword(b"del"):
            ref = self.run() or None
            if self.keyword(b"ins"):
                alt = self.run()
                if not alt:
                    raise self.err("expected nucleotide sequence")
                return e("delins", ref, alt)
            if ref is None:
                self.digits()
            return e("deletion", ref)
        if self.keyword(b"dup"):
            return e("duplication", self.run() or None)
        if self.keyword(b"ins"):
            alt = self.run()
            if not alt:
                raise self.err("expected nucleotide sequence")
            return e("insertion", None, alt)
        if self.keyword(b"inv"):
            return e("inversion", self.run() or None)
        if self.keyword(b"copy"):
            return e("copy", None, "[%d]" % (self.uint() & 0xFFFFFFFF))
        ref = self.run()
        if not ref:
            raise self.err("expected edit")
        if self.eat("="):
            return e("identity")
        if self.eat("["):
            count = self.uint() & 0xFFFFFFFF
            self.expect("]", "expected `]` after repeat count")
            return e("repeat", None, "%s[%d]" % (ref, count))
        self.expect(">", "expected `>` in substitution")
        alt = self.run()
        if not alt:
            raise self.err("expected alternate allele")
        return e("substitution", ref, alt)

    def outer_uncertain(self):
        if self.peek() != ord("("):
            return False
        saved = self.pos
        self.pos += 1
        outer = False
        if self.peek() != ord("?"):
            if self.peek() in (ord("-"), ord("*")):
                self.pos += 1
            self.digits()
            if self.peek() in (ord("+"), ord("-")):
                self.pos += 1
                self.digits()
            outer = self.peek() != ord("_")
        self.pos = saved
        return outer

    def variant(self):
        start = self.pos
        while self.peek() is not None and self.peek() not in (ord(":"), ord("(")):
            self.pos += 1
        if self.pos == start:
            raise self.err("expected accession")
        accession, gene = self.s[start:self.pos].decode("utf-8", "replace"), None
        if self.eat("("):
            g = self.pos
            while self.peek() is not None and self.peek() != ord(")"):
                self.pos += 1
            if self.pos == g:
                raise self.err("expected gene symbol after `(`")
            gene = self.s[g:self.pos].decode("utf-8", "replace")
            self.expect(")", "expected `)` after gene symbol")
        self.expect(":", "expected `:` after accession")
        t = self.peek()
        if t is not None:
            self.pos += 1
        if t is None or chr(t) not in "gcnmrp":
            raise self.err("expected reference type (g/c/n/m/r/p)")
        rt = chr(t)
        self.expect(".", "expected `.` after reference type")
        if rt == "p":
            raise Protein(accession, gene)
        if self.peek() in (ord("="), ord("?")):
            kind, lo, hi, edit, uncertain = "whole_sequence", None, None, self.edit(), False
        elif self.outer_uncertain():
            self.pos += 1
            kind, lo, hi = self.location(rt)
            edit = self.edit()
            self.expect(")", "expected `)` to close uncertain posedit")
            uncertain = True
        else:
            kind, lo, hi = self.location(rt)
            edit = self.edit()
            uncertain = kind == "range" and "uncertain" in (lo["kind"], hi["kind"])
        if self.pos < len(self.s):
            raise self.err("trailing characters after variant")
        return {"accession": accession, "gene": gene, "reference_type": rt,
                "pos_edit": {"location_kind": kind, "start": lo, "end": hi, "edit": edit, "uncertain": uncertain}}


def parse(text):
    """the dict of HgvsVariant.to_dict(); ParseError, or Protein for a p. expression"""
    return _Parser(text if isinstance(text, bytes) else text.encode("utf-8")).variant()


# ---- the bridge -------------------------------------------------------------------------------------------------------------
PREFIXES = ("NC_", "NM_", "NR_", "NG_", "NW_", "NT_", "XM_", "XR_", "ENST", "ENSG", "chr")


def looks_like_gene_symbol(acc: str) -> bool:
    if "." in acc or acc == "MT" or acc.startswith(PREFIXES):
        return False
    for p in ("GL", "KI"):
        if acc.startswith(p) and acc[2:3].isdigit() and acc[2:3].isascii():
            return False
    return True


REVCOMP = bytes.maketrans(b"ACGTN", b"TGCAN")


def revcomp(b: bytes):
    """None for a byte outside ACGTN"""
    return None if b.strip(b"ACGTN") else b.translate(REVCOMP)[::-1]


_OWN = {}


def own_digests(seqs):
    """the assembly's own refget digests, hashed once per assembly object"""
    if id(seqs) not in _OWN or _OWN[id(seqs)][0] is not seqs:
        _OWN[id(seqs)] = (seqs, R.refget_digests(seqs))
    return _OWN[id(seqs)][1]


class Failure(Exception):
    def __init__(self, status, detail=0):
        self.status, self.detail = status, detail


def bridge_one(seqs: dict, accessions: dict, transcripts: list, text, aliases=None):
    """one expression over an assembly {name: bytes} (in the assembly's order), the accession table {name: digest} and a list of
    restatement transcripts -> {"status", "detail", "warning", "chrom" (name or None), "start", "end" (normalized), "id", and
    "span": (chromosome, start, end, strand) before normalization, once the positions are mapped}"""
    out = {"status": OK, "detail": 0, "warning": 0, "chrom": None, "start": 0, "end": 0, "id": None, "span": None}
    try:
        try:
            v = parse(text)
        except ParseError:
            raise Failure(PARSE_ERROR)
        except Protein:
            raise Failure(UNSUPPORTED_REFERENCE_TYPE)
        pe, rt = v["pos_edit"], v["reference_type"]
        out["warning"] = 1 if pe["uncertain"] else 0
        acc, tx = v["accession"], None
        if looks_like_gene_symbol(acc):
            tx = R.lookup_mane(transcripts, acc)
            if tx is None:
                raise Failure(NO_MANE_TRANSCRIPT)
            acc = tx["accession"]
        if rt == "g":
            chrom = acc if acc in seqs else (aliases or {}).get(acc)
            strand = 1
        elif rt in "cn":
            tx = tx or R.lookup(transcripts, acc)
            if tx is None:
                raise Failure(TRANSCRIPT_NOT_FOUND)
            own = own_digests(seqs)
            chrom = next((name for name in seqs if R.digest_bytes(own[name]) == tx["digest"]), None)
            strand = tx["strand"]
        else:
            raise Failure(UNSUPPORTED_REFERENCE_TYPE)
        if chrom is None:
            raise Failure(UNKNOWN_CHROM)
        edit, kind = pe["edit"], pe["location_kind"]
        if edit["kind"] in ("inversion", "unknown", "copy", "repeat") or kind == "whole_sequence" or \
                "uncertain" in (pe["start"]["kind"], (pe["end"] or pe["start"])["kind"]):
            raise Failure(UNSUPPORTED_EDIT)

        def where(p):
            if rt == "g":
                if p["base"] < 1:
                    raise Failure(INCONSISTENT_EDIT)
                return p["base"] - 1
            st, g = R.c_to_g(tx, p["base"], p["offset"], p["datum"] == "cds_stop") if rt == "c" else R.n_to_g(tx, p["base"], p["offset"])
            if st != R.OK:
                raise Failure(MAPPING_ERROR, st)
            return g

        a = where(pe["start"]["position"])
        if kind == "single":
            start, end = ((a + 1, a + 1) if strand > 0 else (a, a)) if edit["kind"] == "insertion" else (a, a + 1)
        else:
            b = where(pe["end"]["position"])
            if edit["kind"] == "insertion":
                if abs(a - b) != 1:
                    raise Failure(INCONSISTENT_EDIT)
                start = end = max(a, b)
            else:
                start, end = min(a, b), max(a, b) + 1
        seq = seqs[chrom]
        out["span"] = (chrom, start, end, strand)
        if end > len(seq):
            raise Failure(OUT_OF_BOUNDS)
        actual = seq[start:end].upper()
        oriented = lambda s: s.encode() if strand > 0 else revcomp(s.encode())  # noqa: E731
        if edit["kind"] in ("substitution", "insertion", "delins"):
            alt = oriented(edit["alt"])
            if alt is None:
                raise Failure(INCONSISTENT_EDIT)
        else:
            alt = {"deletion": b"", "duplication": actual + actual, "identity": actual}[edit["kind"]]
        if edit["ref"] is not None:
            want = oriented(edit["ref"])
            if want is None:
                raise Failure(INCONSISTENT_EDIT)
            if want != actual:
                raise Failure(REF_MISMATCH)
        if chrom not in accessions:
            raise Failure(NORMALIZE_ERROR, V.UNKNOWN_CHROMOSOME)
        try:
            ns, ne, allele = V.normalize(seq, start, actual, alt)
        except V.NormalizeError as e:
            raise Failure(NORMALIZE_ERROR, e.status)
        out.update(chrom=chrom, start=ns, end=ne, id=V.vrs_id("SQ." + accessions[chrom], ns, ne, allele))
    except Failure as f:
        out.update(status=f.status, detail=f.detail)
    return out


def bridge(seqs, accessions, transcripts, strings, aliases=None):
    return [bridge_one(seqs, accessions, transcripts, s, aliases) for s in strings]
