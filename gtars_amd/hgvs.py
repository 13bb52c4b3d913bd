"""HGVS expressions: ``gtars.vrs.hgvs`` (gtars-python/src/vrs/hgvs.rs, gtars-vrs/src/hgvs/{ast,parser,bridge}.rs).

The parser mirror keeps the reference's classes and results: ``ReferenceType``, ``Datum``, ``Position``, ``Edit``,
``PositionBound``, ``PosEdit``, ``HgvsVariant`` with ``to_dict()``, ``parse_hgvs`` and ``HgvsError``.  It is host code and needs no
device.  Protein expressions (``p.``) are not parsed: ``parse_hgvs`` raises HgvsError for them and the bridge answers
"unsupported reference type", which is what the reference's bridge answers for them too.  It is the one narrowing of the
parser.

``hgvs_to_vrs_id`` is the reference's call with other arguments: the reference's ``provider`` / ``refget`` /
``collection_digest`` have no counterpart here, so it takes the assembly and a ``ReadonlyTxStore`` (or ``BoundTxStore``; None
when every expression is ``g.``).  ``hgvs_to_vrs_ids`` is the additive batch call.  The strings are parsed and their
accessions looked up on the host threads; the rest runs on the device that holds the assembly's packed image
(csrc/hgvs.hip): one lane per row maps the positions, cuts the span and checks REF against the
assembly, REF and ALT are written eight bytes per lane, and the columns go straight into the kernels of ``gtars.vrs``.
``on_host=True`` runs the library's own host path instead: the same results, no device.  Without a device the default calls
raise NoDeviceError; there is no silent fallback.

``hgvs_to_transcript_vrs_id`` / ``hgvs_to_transcript_vrs_ids`` / ``hgvs_to_transcript_allele`` are the second bridge of the
reference (bridge.rs:226-534): the allele of a ``c.`` / ``n.`` expression anchored on the transcript's own refget accession,
"SQ." + sha512t24u of the mature mRNA derived from the assembly.  Coordinates, REF, ALT and the normalization are in mRNA
space and in transcript orientation; a roll crosses exon junctions and stops at the transcript's ends (csrc/hgvs_tx.hip,
DESIGN.md section 3, K23).  These take the assembly and the store in place of the reference's ``genome`` / ``tx_store``.

Only literal sequence states are computed; ``ReferenceLengthExpression`` states are not part of this module.
"""
from __future__ import annotations

import ctypes as C
from enum import Enum
from typing import Dict, List, Optional, Sequence

import numpy as np

from ._lib import check, lib, ptr
from .reftx import BoundTxStore, ReadonlyTxStore, TxStoreBuilder, _mapping_text, mature_mrna
from .seqstats import _genome_handle
from .vrs import VA_PREFIX, _accession_table, sha512t24u
from .vrs import STATUS_NAMES as _VRS_STATUS_NAMES


def _status_names():
    names, k = [], 0
    while True:
        s = lib.gtars_hgvs_status_name(k)
        if s is None:
            return tuple(names)
        names.append(s.decode("ascii"))
        k += 1


STATUS_NAMES = _status_names()
(OK, PARSE_ERROR, UNSUPPORTED_REFERENCE_TYPE, UNSUPPORTED_EDIT, TRANSCRIPT_NOT_FOUND, NO_MANE_TRANSCRIPT, UNKNOWN_CHROM, MAPPING_ERROR,
 OUT_OF_BOUNDS, INCONSISTENT_EDIT, REF_MISMATCH, NORMALIZE_ERROR) = range(12)
WARN_UNCERTAIN = 1
NONE_U32 = 0xFFFFFFFF


class HgvsError(Exception):
    pass


class ReferenceType(Enum):
    Coding = 0
    NonCoding = 1
    Genomic = 2
    Mitochondrial = 3
    Protein = 4
    Rna = 5

    def __repr__(self):
        return f"ReferenceType.{self.name}"


class Datum(Enum):
    SeqStart = 0
    Cds = 1
    CdsStop = 2

    def __repr__(self):
        return f"Datum.{self.name}"


_REF_TYPES = (ReferenceType.Genomic, ReferenceType.Coding, ReferenceType.NonCoding, ReferenceType.Mitochondrial, ReferenceType.Rna,
              ReferenceType.Protein)  # by the library's code
_REF_LETTER = {ReferenceType.Coding: "c", ReferenceType.NonCoding: "n", ReferenceType.Genomic: "g", ReferenceType.Mitochondrial: "m",
               ReferenceType.Protein: "p", ReferenceType.Rna: "r"}
_DATUMS = (Datum.SeqStart, Datum.Cds, Datum.CdsStop)
_DATUM_TEXT = {Datum.SeqStart: "seq_start", Datum.Cds: "cds", Datum.CdsStop: "cds_stop"}
_EDIT_KINDS = ("substitution", "deletion", "duplication", "insertion", "delins", "inversion", "identity", "unknown", "copy", "repeat")
E_SUB, E_DEL, E_DUP, E_INS, E_DELINS, E_INV, E_IDENTITY, E_UNKNOWN, E_COPY, E_REPEAT = range(10)
L_SINGLE, L_RANGE, L_WHOLE, L_UNCERTAIN_START, L_UNCERTAIN_END, L_UNCERTAIN_BOTH = range(6)
_HAS_GENE, _HAS_REF, _UNCERTAIN = 1, 2, 4


class Position:
    def __init__(self, base: int, offset: int, datum: Datum):
        self.base, self.offset, self.datum = base, offset, datum

    def to_dict(self) -> dict:
        return {"base": self.base, "offset": self.offset, "datum": _DATUM_TEXT[self.datum]}

    def __repr__(self):
        return f"Position(base={self.base}, offset={self.offset}, datum={self.datum.name})"


class Edit:
    """``kind``: "substitution", "deletion", "insertion", "delins", "duplication", "inversion", "identity", "unknown", "copy"
    or "repeat"; ``ref`` / ``alt`` as the expression has them, or None"""

    def __init__(self, kind: str, ref: Optional[str], alt: Optional[str]):
        self.kind, self.ref, self.alt = kind, ref, alt

    def to_dict(self) -> dict:
        return {"kind": self.kind, "ref": self.ref, "alt": self.alt}

    def __repr__(self):
        return f"Edit(kind={self.kind!r}, ref={self.ref!r}, alt={self.alt!r})"


class PositionBound:
    """one side of a location: ``kind`` "certain" with ``position``, or "uncertain" with ``low`` / ``high`` (None for ``?``)"""

    def __init__(self, kind: str, position: Optional[Position], low: Optional[Position], high: Optional[Position]):
        self.kind, self.position, self.low, self.high = kind, position, low, high

    def to_dict(self) -> dict:
        d = lambda p: None if p is None else p.to_dict()  # noqa: E731
        return {"kind": self.kind, "position": d(self.position), "low": d(self.low), "high": d(self.high)}

    def __repr__(self):
        return f"PositionBound(kind={self.kind!r}, position={self.position!r}, low={self.low!r}, high={self.high!r})"


class PosEdit:
    """``location_kind``: "single", "range" or "whole_sequence" """

    def __init__(self, location_kind: str, start: Optional[PositionBound], end: Optional[PositionBound], edit: Edit, uncertain: bool):
        self.location_kind, self.start, self.end, self.edit, self.uncertain = location_kind, start, end, edit, uncertain

    def to_dict(self) -> dict:
        return {"location_kind": self.location_kind, "start": None if self.start is None else self.start.to_dict(),
                "end": None if self.end is None else self.end.to_dict(), "edit": self.edit.to_dict(), "uncertain": self.uncertain}

    def __repr__(self):
        return (f"PosEdit(location_kind={self.location_kind!r}, start={self.start!r}, end={self.end!r}, edit={self.edit!r}, "
                f"uncertain={str(self.uncertain).lower()})")


class HgvsVariant:
    def __init__(self, accession: str, gene: Optional[str], reference_type: ReferenceType, pos_edit: PosEdit):
        self.accession, self.gene, self.reference_type, self.pos_edit = accession, gene, reference_type, pos_edit

    def to_dict(self) -> dict:
        return {"accession": self.accession, "gene": self.gene, "reference_type": _REF_LETTER[self.reference_type],
                "pos_edit": self.pos_edit.to_dict()}

    def __repr__(self):
        return f"HgvsVariant(accession={self.accession!r}, reference_type={self.reference_type!r}, pos_edit={self.pos_edit!r})"


# ---- the library's row ---------------------------------------------------------------------------------------------------
class _CPosition(C.Structure):
    _fields_ = [("base", C.c_int64), ("offset", C.c_int64), ("datum", C.c_uint8), ("present", C.c_uint8), ("reserved", C.c_uint8 * 6)]


class _CRow(C.Structure):
    _fields_ = [(name, C.c_uint32) for name in ("acc_off", "acc_len", "gene_off", "gene_len", "ref_off", "ref_len", "alt_off", "alt_len")] + \
               [("pos", _CPosition * 4), ("count", C.c_uint32), ("ref_type", C.c_uint8), ("loc", C.c_uint8), ("edit", C.c_uint8),
                ("flags", C.c_uint8)]


def _debug_str(s: str) -> str:
    """a str as Rust's {:?} writes it"""
    out = []
    for ch in s:
        if ch in '"\\':
            out.append("\\" + ch)
        elif ch == "\n":
            out.append("\\n")
        elif ch == "\r":
            out.append("\\r")
        elif ch == "\t":
            out.append("\\t")
        elif ch == "\0":
            out.append("\\0")
        elif not ch.isprintable():
            out.append("\\u{%x}" % ord(ch))
        else:
            out.append(ch)
    return '"' + "".join(out) + '"'


def _parse_row(s: str):
    """(status, row, bytes) of one expression; HgvsError for a parse failure"""
    b = str(s).encode("utf-8")
    row, status, at = _CRow(), C.c_uint8(), C.c_uint64()
    msg = C.create_string_buffer(96)
    check(lib.gtars_hgvs_parse(b, len(b), C.byref(row), C.byref(status), C.byref(at), msg, len(msg)))
    if status.value == PARSE_ERROR:
        raise HgvsError(f"HGVS parse error at position {at.value}: {msg.value.decode('ascii')} (in: {_debug_str(str(s))})")
    return status.value, row, b


def _span(b: bytes, off: int, n: int) -> str:
    return b[off:off + n].decode("utf-8", "replace")


def _position(p: _CPosition) -> Optional[Position]:
    return Position(p.base, p.offset, _DATUMS[p.datum]) if p.present else None


def _edit_of(row: _CRow, b: bytes) -> Edit:
    ref = _span(b, row.ref_off, row.ref_len) if row.flags & _HAS_REF else None
    alt = _span(b, row.alt_off, row.alt_len)
    k = row.edit
    if k == E_SUB or k == E_DELINS:
        return Edit(_EDIT_KINDS[k], ref, alt)
    if k in (E_DEL, E_DUP, E_INV):
        return Edit(_EDIT_KINDS[k], ref, None)
    if k == E_INS:
        return Edit(_EDIT_KINDS[k], None, alt)
    if k == E_COPY:
        return Edit("copy", None, f"[{row.count}]")
    if k == E_REPEAT:
        return Edit("repeat", None, f"{_span(b, row.ref_off, row.ref_len)}[{row.count}]")
    return Edit(_EDIT_KINDS[k], None, None)


def parse_hgvs(s: str) -> HgvsVariant:
    """the parsed expression; HgvsError "HGVS parse error at position N: message (in: "...")" for one that does not parse"""
    status, row, b = _parse_row(s)
    if status == UNSUPPORTED_REFERENCE_TYPE:
        raise HgvsError(f"protein expressions are not parsed (in: {_debug_str(str(s))})")
    certain = lambda p: PositionBound("certain", _position(p), None, None)  # noqa: E731
    uncertain = lambda lo, hi: PositionBound("uncertain", None, _position(lo), _position(hi))  # noqa: E731
    p = row.pos
    kind, start, end = {
        L_SINGLE: lambda: ("single", certain(p[0]), None),
        L_RANGE: lambda: ("range", certain(p[0]), certain(p[2])),
        L_WHOLE: lambda: ("whole_sequence", None, None),
        L_UNCERTAIN_START: lambda: ("range", uncertain(p[0], p[1]), certain(p[2])),
        L_UNCERTAIN_END: lambda: ("range", certain(p[0]), uncertain(p[2], p[3])),
        L_UNCERTAIN_BOTH: lambda: ("range", uncertain(p[0], p[1]), uncertain(p[2], p[3])),
    }[row.loc]()
    return HgvsVariant(_span(b, row.acc_off, row.acc_len), _span(b, row.gene_off, row.gene_len) if row.flags & _HAS_GENE else None,
                       _REF_TYPES[row.ref_type], PosEdit(kind, start, end, _edit_of(row, b), bool(row.flags & _UNCERTAIN)))


def looks_like_gene_symbol(accession: str) -> bool:
    """whether the bridge reads an accession as a bare gene symbol and resolves it through the MANE index (bridge.rs:552-589)"""
    return bool(lib.gtars_hgvs_looks_like_gene_symbol(str(accession).encode("utf-8")))


# ---- the bridge -----------------------------------------------------------------------------------------------------------
def _bound(genome, store) -> BoundTxStore:
    if isinstance(store, BoundTxStore):
        if store.genome is not genome:
            raise ValueError("the store is bound to another assembly")
        return store
    if store is None:  # g. only: a store without transcripts
        store = ReadonlyTxStore.from_bytes(TxStoreBuilder().to_bytes())
    return BoundTxStore(genome, store)


def _blob(strings: Sequence) -> tuple:
    enc = [s if isinstance(s, (bytes, bytearray)) else str(s).encode("utf-8") for s in strings]
    off = np.zeros(len(enc) + 1, dtype=np.uint64)
    if enc:
        off[1:] = np.cumsum([len(b) for b in enc], dtype=np.uint64)
    return np.frombuffer(b"".join(enc), dtype=np.uint8), off, enc


def _alias_table(genome, aliases: Optional[Dict[str, str]]):
    """name -> chromosome name of the assembly, as the library's three columns"""
    if not aliases:
        return np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), 0
    ids = {name: k for k, name in enumerate(genome.chrom_names)}
    keys = list(aliases)
    for k in keys:
        if aliases[k] not in ids:
            raise ValueError(f"alias {k!r} names {aliases[k]!r}, which is no chromosome of the assembly")
    pool, off, _ = _blob(keys)
    return pool, off, np.array([ids[aliases[k]] for k in keys], dtype=np.uint32), len(keys)


COLUMN_DTYPES = (("pre", np.uint8), ("kind", np.uint8), ("loc", np.uint8), ("edit", np.uint8), ("flags", np.uint8), ("tx", np.uint32),
                 ("base1", np.int64), ("off1", np.int64), ("base2", np.int64), ("off2", np.int64), ("text_off", np.uint64),
                 ("ref_off", np.uint32), ("ref_len", np.uint32), ("alt_off", np.uint32), ("alt_len", np.uint32))


class _CColumns(C.Structure):
    _fields_ = [(name, C.c_void_p) for name, _ in COLUMN_DTYPES] + [("text", C.c_void_p), ("text_bytes", C.c_uint64), ("n", C.c_uint64)]


def resolve(genome, store, strings: Sequence, aliases: Optional[Dict[str, str]] = None, threads: int = 0) -> dict:
    """the host half of the batch call: every string parsed and its accession looked up, as the columns the device entry takes
    (numpy arrays by the names of COLUMN_DTYPES, plus "text": the strings back to back as uint8)"""
    b = _bound(genome, store)
    text, off, _ = _blob(strings)
    n = len(off) - 1
    cols = {name: np.zeros(n, dtype=dt) for name, dt in COLUMN_DTYPES}
    c = _CColumns(**{name: cols[name].ctypes.data if n else None for name, _ in COLUMN_DTYPES})
    a_pool, a_off, a_chrom, n_alias = _alias_table(b.genome, aliases)
    check(lib.gtars_hgvs_resolve(b._h, ptr(text), ptr(off), n, ptr(a_pool), ptr(a_off), ptr(a_chrom), n_alias, int(threads), C.byref(c)))
    cols["text"] = text
    return cols


def ids_device(genome, store, d_cols: Dict[str, int], text_bytes: int, n: int, d_status: int = 0, d_detail: int = 0, d_warnings: int = 0,
               d_chrom: int = 0, d_start: int = 0, d_end: int = 0, d_digests: int = 0, stream: int = 0,
               accessions: Optional[Dict[str, str]] = None) -> None:
    """the bridge for resolved columns that are on the device already: ``d_cols`` maps the names of COLUMN_DTYPES and "text" to
    device pointers; outputs u8 statuses, details and warnings, u32 chromosome ids, u64 starts / ends, n * 32 digest bytes, any
    may be 0.  Queued on ``stream``, which is drained before the call returns.  The current device must be the assembly's.
    ``store``: a BoundTxStore that is kept between calls, or a ReadonlyTxStore."""
    b = _bound(genome, store)
    c = _CColumns(**{name: int(d_cols[name]) for name, _ in COLUMN_DTYPES}, text=int(d_cols["text"]), text_bytes=int(text_bytes), n=int(n))
    check(lib.gtars_hgvs_ids_device(b._h, C.byref(c), _accession_table(b.genome, accessions), C.c_void_p(d_status), C.c_void_p(d_detail),
                                    C.c_void_p(d_warnings), C.c_void_p(d_chrom), C.c_void_p(d_start), C.c_void_p(d_end),
                                    C.c_void_p(d_digests), C.c_void_p(stream)))


def hgvs_to_vrs_ids(genome, store, strings: Sequence, accessions: Optional[Dict[str, str]] = None, aliases: Optional[Dict[str, str]] = None,
                    on_host: bool = False, threads: int = 0) -> dict:
    """VRS identifiers of a batch of HGVS expressions over an assembly and a transcript store (None: ``g.`` only; a BoundTxStore
    is kept between calls): {"ids": "ga4gh:VA...." per string (None for one that failed), "statuses" (numpy u8, see
    STATUS_NAMES), "details" (the mapping status of ``gtars.reftx`` for status 7, the status of ``gtars.vrs`` for status 11),
    "warnings" (bit 0: uncertain expression), "chroms" (chromosome ids, 2^32 - 1 for a row that failed), "starts", "ends" (the
    normalized interval)}.  ``accessions``: chromosome name -> refget digest, default the assembly's own; ``aliases``: other
    names ``g.`` expressions may use -> chromosome name.  Never raises for data."""
    b = _bound(genome, store)
    _genome_handle(b.genome)
    text, off, _ = _blob(strings)
    n = len(off) - 1
    status, detail, warnings = (np.zeros(n, dtype=np.uint8) for _ in range(3))
    chrom = np.full(n, NONE_U32, dtype=np.uint32)
    ns, ne = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    digests = np.zeros(32 * n, dtype=np.uint8)
    a_pool, a_off, a_chrom, n_alias = _alias_table(b.genome, aliases)
    check(lib.gtars_hgvs_to_vrs(b._h, ptr(text), ptr(off), n, ptr(a_pool), ptr(a_off), ptr(a_chrom), n_alias,
                                _accession_table(b.genome, accessions), 1 if on_host else 0, int(threads), ptr(status), ptr(detail),
                                ptr(warnings), ptr(chrom), ptr(ns), ptr(ne), ptr(digests)))
    raw = digests.tobytes()
    ids: List[Optional[str]] = [VA_PREFIX + raw[32 * i:32 * i + 32].decode("ascii") if status[i] == 0 else None for i in range(n)]
    return {"ids": ids, "statuses": status, "details": detail, "warnings": warnings, "chroms": chrom, "starts": ns, "ends": ne}


def _unsupported_edit(row: _CRow) -> str:
    for kind, text in ((E_INV, "inv"), (E_UNKNOWN, "unknown"), (E_COPY, "copy"), (E_REPEAT, "repeat")):
        if row.edit == kind:
            return text
    return "whole-sequence edit" if row.loc == L_WHOLE else "uncertain position range"


def _failure_text(b: BoundTxStore, s: str, status: int, detail: int, aliases) -> str:
    """BridgeError's Display (bridge.rs:55-86) for a row that failed past the parser; the figures are derived again here, on
    the host, from the row itself"""
    st, row, raw = _parse_row(s)
    acc = _span(raw, row.acc_off, row.acc_len)
    if status == UNSUPPORTED_REFERENCE_TYPE:
        return f"unsupported reference type: {_REF_LETTER[_REF_TYPES[row.ref_type]].upper()} (v1 supports g., c., n.)"
    if status == NO_MANE_TRANSCRIPT:
        return f"provider error: No MANE Select transcript for gene: {acc}"
    store, genome = b.store, b.genome
    tx = None
    if looks_like_gene_symbol(acc):
        tx = store.lookup_mane(acc)
        acc = tx.accession
    if status == TRANSCRIPT_NOT_FOUND:
        return f"provider error: Transcript not found: {acc}"
    kind = row.ref_type  # 0 g, 1 c, 2 n
    if kind != 0 and tx is None:
        tx = store.lookup(acc)
    names = genome.chrom_names
    if status == UNKNOWN_CHROM:
        return f"chromosome accession {acc if kind == 0 else tx.chrom} not found in collection"
    if status == UNSUPPORTED_EDIT:
        return f"unsupported edit: {_unsupported_edit(row)}"
    if kind == 0:
        chrom = acc if acc in names else (aliases or {}).get(acc)
    else:
        chrom = {d: name for name, d in reversed(list(genome.refget_digests().items()))}.get(tx.chrom[3:])
    strand = 1 if kind == 0 or str(tx.strand) == "+" else -1

    def where(p):  # position_to_genomic_interbase: (interbase, None) or (None, the error's text)
        if kind == 0:
            return (p.base - 1, None) if p.base >= 1 else (None, f"inconsistent edit: g. position must be >= 1, got {p.base}")
        tx_i = np.array([store.index_of(acc)], dtype=np.uint32)
        kinds, poss, offs = np.array([kind - 1], dtype=np.uint8), np.array([p.base], dtype=np.int64), np.array([p.offset], dtype=np.int64)
        stars, out, code = np.array([1 if p.datum == 2 else 0], dtype=np.uint8), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint8)
        check(lib.gtars_txstore_map(store._h, ptr(tx_i), ptr(kinds), ptr(poss), ptr(offs), ptr(stars), 1, 1, ptr(out), ptr(code)))
        if code[0]:
            return None, "provider error: Mapping error: " + _mapping_text(int(code[0]), acc, p.base, p.offset)
        return int(out[0]), None

    a, err = where(row.pos[0])
    if err:
        return err
    if row.loc == L_SINGLE:
        start, end = ((a + 1, a + 1) if strand > 0 else (a, a)) if row.edit == E_INS else (a, a + 1)
    else:
        c, err = where(row.pos[2])
        if err:
            return err
        if row.edit == E_INS:
            if abs(a - c) != 1:
                return f"inconsistent edit: ins range positions are not adjacent: {a} and {c}"
            start = end = max(a, c)
        else:
            start, end = min(a, c), max(a, c) + 1
    if status == OUT_OF_BOUNDS:
        return f"coordinate {end} out of bounds for {chrom} (len={genome.chrom_sizes[chrom]})"
    ref = _span(raw, row.ref_off, row.ref_len) if row.flags & _HAS_REF else ""
    if status == INCONSISTENT_EDIT:
        alt = _span(raw, row.alt_off, row.alt_len) if row.edit in (E_SUB, E_INS, E_DELINS) else ""
        for allele in (alt, ref):  # (revcomp reads an allele from its end)
            bad = next((ch for ch in reversed(allele) if ch not in "ACGTN"), None)
            if bad is not None:
                return f"inconsistent edit: non-ACGTN base {bad!r} in HGVS allele"
    if status == REF_MISMATCH:
        actual = genome.sequence(chrom, start, end).decode("ascii", "replace").upper()
        return f"REF mismatch at {chrom}:{start}: HGVS says {ref}, sequence has {actual}"
    if status == NORMALIZE_ERROR:
        return "normalize error: " + ("chromosome is not in the assembly or has no accession" if detail == 4 else _VRS_STATUS_NAMES[detail])
    return f"bridge failed: {STATUS_NAMES[status]}"


def hgvs_to_vrs_id(hgvs_str: str, genome, store=None, accessions: Optional[Dict[str, str]] = None, aliases: Optional[Dict[str, str]] = None,
                   on_host: bool = False) -> str:
    """parse + bridge + normalize + digest of one expression: its "ga4gh:VA...." identifier, the one the equivalent VCF row
    gets from ``gtars.vrs``.  HgvsError for an expression that does not parse, ValueError with BridgeError's text for every
    other failure."""
    b = _bound(genome, store)
    _parse_row(hgvs_str)  # (HgvsError before anything else)
    r = hgvs_to_vrs_ids(genome, b, [hgvs_str], accessions, aliases, on_host, 1)
    if r["statuses"][0] != OK:
        raise ValueError(_failure_text(b, hgvs_str, int(r["statuses"][0]), int(r["details"][0]), aliases))
    return r["ids"][0]


# ---- the transcript-anchored bridge (K23) -----------------------------------------------------------------------------------
TX_NOT_EXONIC = 8  # the detail of MAPPING_ERROR for a position that is intronic or outside the mature mRNA


def transcript_ids_device(genome, store, d_cols: Dict[str, int], text_bytes: int, n: int, d_status: int = 0, d_detail: int = 0,
                          d_warnings: int = 0, d_tx: int = 0, d_start: int = 0, d_end: int = 0, d_digests: int = 0, d_anchors: int = 0,
                          stream: int = 0) -> None:
    """the transcript-anchored bridge for resolved columns that are on the device already (``d_cols`` as for ``ids_device``);
    outputs u8 statuses, details and warnings, u32 transcript numbers, u64 starts / ends on the mRNA, n * 32 digest bytes and
    n * 32 bytes of the anchors' digests, any may be 0.  Queued on ``stream``, which is drained before the call returns.  The
    current device must be the assembly's."""
    b = _bound(genome, store)
    c = _CColumns(**{name: int(d_cols[name]) for name, _ in COLUMN_DTYPES}, text=int(d_cols["text"]), text_bytes=int(text_bytes), n=int(n))
    check(lib.gtars_hgvs_transcript_ids_device(b._h, C.byref(c), C.c_void_p(d_status), C.c_void_p(d_detail), C.c_void_p(d_warnings),
                                               C.c_void_p(d_tx), C.c_void_p(d_start), C.c_void_p(d_end), C.c_void_p(d_digests),
                                               C.c_void_p(d_anchors), C.c_void_p(stream)))


def hgvs_to_transcript_vrs_ids(genome, store, strings: Sequence, on_host: bool = False, threads: int = 0) -> dict:
    """VRS identifiers of a batch of ``c.`` / ``n.`` expressions, anchored on the transcripts' mature mRNAs: {"ids":
    "ga4gh:VA...." per string (None for one that failed), "statuses" (see STATUS_NAMES), "details" (the mapping status of
    ``gtars.reftx`` for status 7 -- 8, TX_NOT_EXONIC: intronic or outside the mature mRNA --, the status of ``gtars.vrs`` for
    status 11), "warnings" (bit 0: uncertain expression), "transcripts" (numbers in the store, 2^32 - 1 for a row that
    failed), "accessions" ("SQ...." of the mRNA, None for a row that failed), "starts", "ends" (the normalized interval on the
    mRNA)}.  ``store``: a ReadonlyTxStore, or a BoundTxStore that is kept between calls.  Never raises for data."""
    b = _bound(genome, store)
    _genome_handle(b.genome)
    text, off, _ = _blob(strings)
    n = len(off) - 1
    status, detail, warnings = (np.zeros(n, dtype=np.uint8) for _ in range(3))
    tx = np.full(n, NONE_U32, dtype=np.uint32)
    ns, ne = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    digests, anchors = np.zeros(32 * n, dtype=np.uint8), np.zeros(32 * n, dtype=np.uint8)
    check(lib.gtars_hgvs_to_transcript_vrs(b._h, ptr(text), ptr(off), n, 1 if on_host else 0, int(threads), ptr(status), ptr(detail),
                                           ptr(warnings), ptr(tx), ptr(ns), ptr(ne), ptr(digests), ptr(anchors)))
    raw, raw_a = digests.tobytes(), anchors.tobytes()
    ok = [status[i] == 0 for i in range(n)]
    ids: List[Optional[str]] = [VA_PREFIX + raw[32 * i:32 * i + 32].decode("ascii") if ok[i] else None for i in range(n)]
    accs: List[Optional[str]] = ["SQ." + raw_a[32 * i:32 * i + 32].decode("ascii") if ok[i] else None for i in range(n)]
    return {"ids": ids, "statuses": status, "details": detail, "warnings": warnings, "transcripts": tx, "accessions": accs, "starts": ns,
            "ends": ne}


def _tx_parts(b: BoundTxStore, s: str):
    """build_transcript_allele_parts (bridge.rs:306-403) for one expression on the host, check for check: (accession, start,
    end, mRNA, ALT), or ValueError with BridgeError's Display"""
    st, row, raw = _parse_row(s)
    if st == UNSUPPORTED_REFERENCE_TYPE or row.ref_type not in (1, 2):
        raise ValueError(f"unsupported reference type: {_REF_LETTER[_REF_TYPES[row.ref_type]].upper()} (v1 supports g., c., n.)")
    store, acc = b.store, _span(raw, row.acc_off, row.acc_len)
    if looks_like_gene_symbol(acc):
        mane = store.lookup_mane(acc)
        if mane is None:
            raise ValueError(f"provider error: No MANE Select transcript for gene: {acc}")
        acc = mane.accession
    if row.edit in (E_INV, E_UNKNOWN, E_COPY, E_REPEAT) or row.loc > L_RANGE:
        raise ValueError("unsupported edit: " + ("ins position range" if row.edit == E_INS else _unsupported_edit(row)))
    index = store.index_of(acc)
    if index < 0:
        raise ValueError(f"provider error: Transcript not found: {acc}")

    def one(kind, pos, offset, star):
        tx_i, kinds = np.array([index], dtype=np.uint32), np.array([kind], dtype=np.uint8)
        poss, offs = np.array([pos], dtype=np.uint64).view(np.int64), np.array([offset], dtype=np.int64)
        stars, out, code = np.array([star], dtype=np.uint8), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint8)
        check(lib.gtars_txstore_map(store._h, ptr(tx_i), ptr(kinds), ptr(poss), ptr(offs), ptr(stars), 1, 1, ptr(out), ptr(code)))
        return int(out[0]), int(code[0])

    def forward(p):  # position_to_genomic_interbase
        g, code = one(row.ref_type - 1, p.base % (1 << 64), p.offset, 1 if p.datum == 2 else 0)
        if code:
            raise ValueError("provider error: Mapping error: " + _mapping_text(code, acc, p.base, p.offset))
        return g

    def back(g):  # map_g_to_tx
        off, code = one(2, g, 0, 0)
        if code == TX_NOT_EXONIC:
            raise ValueError(f"position {g} on {acc} is intronic or outside the mature mRNA (no transcript-mRNA coordinate)")
        if code:
            raise ValueError("provider error: Mapping error: " + _mapping_text(code, acc, g, 0))
        return off

    if row.loc == L_SINGLE:
        a = back(forward(row.pos[0]))
        start, end = (a + 1, a + 1) if row.edit == E_INS else (a, a + 1)
    else:
        ga, gb = forward(row.pos[0]), forward(row.pos[2])
        a, c = back(ga), back(gb)
        if row.edit == E_INS:
            if abs(a - c) != 1:
                raise ValueError(f"inconsistent edit: ins range positions are not adjacent on the transcript: offsets {a} and {c}")
            start = end = max(a, c)
        else:
            start, end = min(a, c), max(a, c) + 1
    try:
        mrna = mature_mrna(b.genome, b, acc, on_host=True)
    except ValueError as e:
        raise ValueError(f"refget error: {e}") from None
    if end > len(mrna):
        raise ValueError(f"coordinate {end} out of bounds for {acc} (len={len(mrna)})")
    actual = mrna[start:end]
    alt = {E_DEL: "", E_DUP: actual + actual, E_IDENTITY: actual}.get(row.edit)
    if alt is None:
        alt = _span(raw, row.alt_off, row.alt_len)
    if row.flags & _HAS_REF and _span(raw, row.ref_off, row.ref_len) != actual:
        raise ValueError(f"REF mismatch at {acc}:{start}: HGVS says {_span(raw, row.ref_off, row.ref_len)}, sequence has {actual}")
    return acc, start, end, mrna, alt


def hgvs_to_transcript_allele(hgvs_str: str, genome, store) -> dict:
    """the non-normalized VRS Allele of one ``c.`` / ``n.`` expression on its transcript's mature mRNA, as a dict:
    ``location.sequenceReference.refgetAccession`` ("SQ." + the digest of the derived mRNA), ``location.start`` / ``end``
    (0-based interbase on the mRNA) and ``state.sequence`` (ALT as written; the span once or twice for ``=`` and ``dup``).
    Host code: one expression, nothing to spread over a device.  HgvsError / ValueError as ``hgvs_to_transcript_vrs_id``."""
    b = _bound(genome, store)
    _, start, end, mrna, alt = _tx_parts(b, hgvs_str)
    return {"type": "Allele",
            "location": {"type": "SequenceLocation", "sequenceReference": {"type": "SequenceReference", "refgetAccession": "SQ." + sha512t24u(mrna)},
                         "start": start, "end": end},
            "state": {"type": "LiteralSequenceExpression", "sequence": alt}}


def hgvs_to_transcript_vrs_id(hgvs_str: str, genome, store, on_host: bool = False) -> str:
    """parse + bridge + normalize + digest of one expression on its transcript's mature mRNA: the "ga4gh:VA...." identifier
    whose location references "SQ." + the digest of the derived mRNA.  HgvsError for an expression that does not parse,
    ValueError with BridgeError's text for every other failure (a position that is intronic or outside the mature mRNA:
    "position N on ACC is intronic or outside the mature mRNA (no transcript-mRNA coordinate)")."""
    b = _bound(genome, store)
    _parse_row(hgvs_str)  # (HgvsError before anything else)
    r = hgvs_to_transcript_vrs_ids(genome, b, [hgvs_str], on_host, 1)
    if r["statuses"][0] != OK:
        _tx_parts(b, hgvs_str)  # (raises the failure's text: it makes the same checks in the same order)
        raise ValueError("normalize error: " + _VRS_STATUS_NAMES[int(r["details"][0])])  # what is left: K18 refused the allele
    return r["ids"][0]
