"""Transcripts: ``gtars.reftx`` (gtars-python/src/reftx/mod.rs, gtars-refget/src/transcripts/{models,builder,store,mapper,sequence}.rs).

The reference's classes keep their signatures and results: ``Strand``, ``ManeStatus``, ``Exon``, ``Transcript``,
``TxStoreBuilder`` (``add_transcript``, ``add_chrom_mapping``, ``load_cdot``, ``load_mane_summary``, ``build``),
``ReadonlyTxStore`` over a ``.reftx`` v2 file and ``CoordinateMapper``, with ``MappingError`` and ``TxStoreError``.  They are
host code and need no device.

The batch calls are additive.  ``CoordinateMapper.c_to_g_many`` / ``n_to_g_many`` / ``g_to_transcript_offset_many`` take
columns and return ``(values, statuses)``; ``mature_mrnas`` and ``transcript_accessions`` give the spliced mRNA of every
transcript and its ``SQ.`` accession.  They run on the device that holds the assembly's packed image (csrc/reftx.hip,
DESIGN.md section 3, K19): one lane per query, one lane per transcript digest, eight output bytes per lane for the
sequences.  ``on_host=True`` runs the library's own host path on its host threads instead: the same results, no device.
Without a device the default calls raise NoDeviceError; there is no silent fallback.

``ReftxProvider`` is not part of this module.  HGVS expressions over a store are ``gtars_amd.hgvs`` (``gtars.vrs.hgvs``).
"""
from __future__ import annotations

import ctypes as C
import gzip
import json
import os
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np

from ._lib import GtarsError, NoDeviceError, check, lib, ptr
from .seqstats import _genome_handle

MAP_STATUS_NAMES = ("ok", "transcript_not_found", "non_coding", "outside_cds", "outside_transcript", "five_prime_utr_overflow",
                    "three_prime_utr_overflow", "invalid_intronic_offset", "not_exonic", "bad_kind", "bad_exons")
SEQ_STATUS_NAMES = ("ok", "transcript_not_found", "sequence_not_found", "exon_past_end", "bad_exons")
KIND_C, KIND_N, KIND_G = 0, 1, 2
NONE_U32 = 0xFFFFFFFF


class MappingError(Exception):
    pass


class TxStoreError(Exception):
    pass


def _store_call(fn, *args):
    try:
        check(fn(*args))
    except NoDeviceError:
        raise
    except (ValueError, OSError, GtarsError) as e:
        raise TxStoreError(getattr(e, "message", None) or str(e)) from None


class Strand:
    """Strand.Plus / Strand.Minus; ``str()`` gives "+" / "-" """

    Plus: "Strand"
    Minus: "Strand"
    _FORWARD = ("+", "Plus", "forward", "Forward", "1", "+1")
    _REVERSE = ("-", "Minus", "reverse", "Reverse", "-1")

    def __init__(self, sign: int):
        self._sign = 1 if sign > 0 else -1

    @classmethod
    def from_str(cls, s: str) -> "Strand":
        if s in cls._FORWARD:
            return cls.Plus
        if s in cls._REVERSE:
            return cls.Minus
        raise ValueError(f'Unrecognized strand: "{s}"')

    def __eq__(self, other):
        if isinstance(other, Strand):
            return self._sign == other._sign
        if isinstance(other, int):  # (eq_int: Plus is 0, Minus is 1)
            return other == (0 if self._sign > 0 else 1)
        return NotImplemented

    def __hash__(self):
        return hash(self._sign)

    def __int__(self):
        return 0 if self._sign > 0 else 1

    def __repr__(self):
        return "Strand.Plus" if self._sign > 0 else "Strand.Minus"

    def __str__(self):
        return "+" if self._sign > 0 else "-"


Strand.Plus, Strand.Minus = Strand(1), Strand(-1)


def _strand_of(value) -> Strand:
    return value if isinstance(value, Strand) else Strand.from_str(str(value))


class ManeStatus:
    def __init__(self, select: bool = False, plus_clinical: bool = False):
        self.select, self.plus_clinical = bool(select), bool(plus_clinical)

    def to_dict(self) -> dict:
        return {"select": self.select, "plus_clinical": self.plus_clinical}

    def __repr__(self):
        return f"ManeStatus(select={self.select}, plus_clinical={self.plus_clinical})"


class Exon:
    def __init__(self, start: int, end: int):
        self.start, self.end = _u32(start), _u32(end)

    def to_dict(self) -> dict:
        return {"start": self.start, "end": self.end}

    def __repr__(self):
        return f"Exon(start={self.start}, end={self.end})"


def _u32(x) -> int:
    x = int(x)
    if not 0 <= x < 1 << 32:
        raise OverflowError("value must fit in u32")
    return x


class Transcript:
    """one record of a store: ``accession``, ``gene`` (None when empty), ``chrom`` ("SQ." + refget digest), ``strand``,
    ``cds_start`` / ``cds_end`` (None for a non-coding transcript), ``exons`` in genomic order, ``mane`` (None without a flag)"""

    def __init__(self, accession: str, gene: Optional[str], chrom: str, strand: Strand, cds_start: Optional[int], cds_end: Optional[int],
                 exons: List[Exon], mane: Optional[ManeStatus], transcript_length: int = 0, cds_length: int = 0):
        self.accession, self.gene, self.chrom, self.strand = accession, gene, chrom, strand
        self.cds_start, self.cds_end, self.exons, self.mane = cds_start, cds_end, exons, mane
        self.transcript_length, self.cds_length = transcript_length, cds_length

    @property
    def is_coding(self) -> bool:
        return self.cds_start is not None and self.cds_end is not None

    def to_dict(self) -> dict:
        return {"accession": self.accession, "gene": self.gene, "chrom": self.chrom, "strand": str(self.strand), "cds_start": self.cds_start,
                "cds_end": self.cds_end, "exons": [e.to_dict() for e in self.exons], "mane": self.mane.to_dict() if self.mane else None}

    def __repr__(self):
        return (f'Transcript(accession="{self.accession}", gene={self.gene!r}, chrom="{self.chrom}", strand={self.strand!r}, '
                f"exons={len(self.exons)})")


def _exon_pairs(exons: Iterable) -> np.ndarray:
    out = []
    for item in exons:
        if isinstance(item, Exon):
            out += [item.start, item.end]
        elif isinstance(item, dict):
            for key in ("start", "end"):
                if key not in item:
                    raise KeyError(f'Missing field "{key}"')
            out += [_u32(item["start"]), _u32(item["end"])]
        else:
            try:
                s, e = item
            except (TypeError, ValueError):
                raise TypeError("exons entries must be Exon, dict, or (start, end) tuple") from None
            out += [_u32(s), _u32(e)]
    return np.array(out, dtype=np.uint32)


def _opt_u32(x) -> int:
    return NONE_U32 if x is None else _u32(x)


def _text(x) -> bytes:
    return str(x).encode("utf-8")


def _open_text(path):
    path = os.fspath(path)
    return gzip.open(path, "rt", encoding="utf-8") if path.endswith(".gz") else open(path, "rt", encoding="utf-8")


class TxStoreBuilder:
    """stages transcripts and writes them as a ``.reftx`` v2 file"""

    def __init__(self):
        self._h = None
        h = C.c_void_p()
        check(lib.gtars_txbuilder_new(C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib.gtars_txbuilder_free(self._h)
                self._h = None
        except Exception:
            pass

    def __len__(self) -> int:
        return int(lib.gtars_txbuilder_len(self._h))

    def add_transcript(self, value) -> None:
        """a ``Transcript`` or a dict with the keys of ``Transcript.to_dict()``; ``gene``, ``cds_start``, ``cds_end`` and ``mane``
        may be missing or None.  KeyError for a missing field, ValueError for a strand that is none, TxStoreError for a
        ``chrom`` that is not "SQ." + base64url of 24 bytes."""
        if isinstance(value, Transcript):
            value = value.to_dict()
        elif not isinstance(value, dict):
            raise TypeError("add_transcript expects a Transcript or dict")
        for key in ("accession", "chrom", "strand", "exons"):
            if key not in value:
                raise KeyError(f'Missing field "{key}"')
        strand = _strand_of(value["strand"])
        mane = value.get("mane")
        if mane is None:
            flags = 0
        elif isinstance(mane, ManeStatus):
            flags = (1 if mane.select else 0) | (2 if mane.plus_clinical else 0)
        elif isinstance(mane, dict):
            flags = (1 if mane.get("select") else 0) | (2 if mane.get("plus_clinical") else 0)
        else:
            raise TypeError("mane must be ManeStatus or dict")
        exons = _exon_pairs(value["exons"])
        gene = value.get("gene")
        _store_call(lib.gtars_txbuilder_add, self._h, _text(value["accession"]), _text(gene) if gene is not None else b"", _text(value["chrom"]),
                    1 if strand == Strand.Plus else -1, _opt_u32(value.get("cds_start")), _opt_u32(value.get("cds_end")), flags, ptr(exons),
                    exons.size // 2)

    def add_chrom_mapping(self, name: str, accession: str) -> None:
        """chromosome name of a cdot file -> its "SQ." refget accession"""
        _store_call(lib.gtars_txbuilder_add_chrom_mapping, self._h, _text(name), _text(accession))

    def load_cdot(self, path) -> int:
        """the transcripts of a cdot JSON file (gzip when the name ends in ".gz") -> how many were staged.  Transcripts on a
        contig without a mapping, with a strand that is not 1 / -1 or without exons are skipped (builder.rs:146-208)."""
        try:
            with _open_text(path) as f:
                doc = json.load(f)
            transcripts = doc["transcripts"]
            count = 0
            added = C.c_int()
            for tx in transcripts.values():
                exons = np.array([[_u32(e[0]), _u32(e[1])] for e in tx["exons"]], dtype=np.uint32).reshape(-1)
                gene = tx.get("gene_name")
                strand = int(tx["strand"])
                check(lib.gtars_txbuilder_add_cdot(self._h, _text(tx["id"]), _text(gene) if gene is not None else b"", _text(tx["contig"]),
                                                   strand if -(1 << 63) <= strand < 1 << 63 else 0, _opt_u32(tx.get("cds_start")),
                                                   _opt_u32(tx.get("cds_end")), ptr(exons), exons.size // 2, C.byref(added)))
                count += added.value
            return count
        except (OSError, ValueError, KeyError, TypeError, IndexError, OverflowError, GtarsError) as e:
            raise TxStoreError(str(e)) from None

    def load_cdot_gz(self, path) -> int:
        return self.load_cdot(path)

    def load_mane_summary(self, path) -> int:
        """MANE flags from an NCBI MANE summary TSV (gzip when the name ends in ".gz") -> accession entries read.  Columns
        RefSeq_nuc, Ensembl_nuc and MANE_status by the header's names; "MANE Select" is 0x01, "MANE Plus Clinical" 0x03;
        affects transcripts that ``load_cdot`` stages afterwards (builder.rs:64-129)."""
        try:
            with _open_text(path) as f:
                lines = (line.rstrip("\n").rstrip("\r") for line in f)
                header = next((line for line in lines if line), None)
                if header is None:
                    raise TxStoreError("MANE summary is empty")
                columns = [c.strip() for c in header.lstrip("#").split("\t")]
                where = {}
                for name in ("RefSeq_nuc", "Ensembl_nuc", "MANE_status"):
                    if name not in columns:
                        raise TxStoreError(f"{name} column not found in MANE summary")
                    where[name] = columns.index(name)
                count = 0
                for line in lines:
                    if not line or line.startswith("#"):
                        continue
                    fields = line.split("\t")
                    if len(fields) <= max(where.values()):
                        continue
                    flags = {"MANE Select": 0x01, "MANE Plus Clinical": 0x03}.get(fields[where["MANE_status"]].strip())
                    if flags is None:
                        continue
                    for name in ("RefSeq_nuc", "Ensembl_nuc"):
                        acc = fields[where[name]].strip()
                        if acc:
                            check(lib.gtars_txbuilder_add_mane(self._h, _text(acc), flags))
                            count += 1
                return count
        except (OSError, ValueError, GtarsError) as e:
            raise TxStoreError(str(e)) from None

    def to_bytes(self) -> bytes:
        """the ``.reftx`` image ``build`` would write"""
        p, n = C.c_void_p(), C.c_uint64()
        _store_call(lib.gtars_txbuilder_bytes, self._h, C.byref(p), C.byref(n))
        try:
            return C.string_at(p, n.value)
        finally:
            lib.gtars_free(p)

    def build(self, out_path) -> None:
        """writes the store to a temporary file next to ``out_path`` and renames it; TxStoreError for an empty builder"""
        _store_call(lib.gtars_txbuilder_build, self._h, os.fspath(out_path).encode("utf-8"))


class ReadonlyTxStore:
    """a ``.reftx`` v2 file, read whole and decoded when it is opened; TxStoreError for a file that is no such store"""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def open(cls, path) -> "ReadonlyTxStore":
        h = C.c_void_p()
        _store_call(lib.gtars_txstore_open, os.fspath(path).encode("utf-8"), C.byref(h))
        return cls(h)

    @classmethod
    def from_bytes(cls, data: bytes) -> "ReadonlyTxStore":
        data = bytes(data)
        h = C.c_void_p()
        _store_call(lib.gtars_txstore_from_bytes, data, len(data), C.byref(h))
        return cls(h)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib.gtars_txstore_free(self._h)
                self._h = None
        except Exception:
            pass

    def __len__(self) -> int:
        return int(lib.gtars_txstore_len(self._h))

    def has_mane_index(self) -> bool:
        return bool(lib.gtars_txstore_has_mane(self._h))

    def index_of(self, accession: str) -> int:
        """the transcript's number in the store (the file's index order), -1: none"""
        return int(lib.gtars_txstore_lookup(self._h, _text(accession)))

    def indices_of(self, accessions: Sequence[str], threads: int = 0) -> np.ndarray:
        """u32 numbers of a batch of accessions, 2^32 - 1 for one the store lacks"""
        enc = [_text(a) for a in accessions]
        off = np.zeros(len(enc) + 1, dtype=np.uint64)
        if enc:
            off[1:] = np.cumsum([len(b) for b in enc], dtype=np.uint64)
        pool = np.frombuffer(b"".join(enc), dtype=np.uint8)
        idx = np.zeros(len(enc), dtype=np.uint32)
        check(lib.gtars_txstore_lookup_many(self._h, ptr(pool), ptr(off), len(enc), int(threads), ptr(idx)))
        return idx

    def transcript(self, i: int) -> Transcript:
        acc, gene, exons = C.c_void_p(), C.c_void_p(), C.c_void_p()
        chrom = C.create_string_buffer(33)
        strand = C.c_int()
        mane, cds_s, cds_e, length, cds_len = (C.c_uint32() for _ in range(5))
        n = C.c_uint64()
        check(lib.gtars_txstore_record(self._h, int(i), C.byref(acc), C.byref(gene), chrom, C.byref(strand), C.byref(mane), C.byref(cds_s),
                                       C.byref(cds_e), C.byref(length), C.byref(cds_len), C.byref(exons), C.byref(n)))
        pairs = np.ctypeslib.as_array(C.cast(exons, C.POINTER(C.c_uint32)), shape=(2 * n.value,)).tolist() if n.value else []
        gene_text = C.string_at(gene).decode("utf-8", "replace")
        return Transcript(C.string_at(acc).decode("utf-8", "replace"), gene_text or None, "SQ." + chrom.value.decode("ascii"),
                          Strand.Plus if strand.value > 0 else Strand.Minus, None if cds_s.value == NONE_U32 else cds_s.value,
                          None if cds_e.value == NONE_U32 else cds_e.value, [Exon(pairs[2 * k], pairs[2 * k + 1]) for k in range(n.value)],
                          ManeStatus(bool(mane.value & 1), bool(mane.value & 2)) if mane.value & 3 else None, length.value, cds_len.value)

    def lookup(self, accession: str) -> Optional[Transcript]:
        i = self.index_of(accession)
        return None if i < 0 else self.transcript(i)

    def lookup_mane(self, gene: str) -> Optional[Transcript]:
        """the MANE Select transcript of a gene symbol (case-insensitive)"""
        i = int(lib.gtars_txstore_lookup_mane(self._h, _text(gene)))
        return None if i < 0 else self.transcript(i)

    def get_chrom_accession(self, accession: str) -> Optional[str]:
        tx = self.lookup(accession)
        return None if tx is None else tx.chrom

    def get_strand(self, accession: str) -> Optional[Strand]:
        tx = self.lookup(accession)
        return None if tx is None else tx.strand

    def accessions(self) -> List[str]:
        """every accession in the store's order"""
        return [self.transcript(i).accession for i in range(len(self))]


class BoundTxStore:
    """a store matched against an assembly's refget digests: what the sequence calls and the device mapping calls work on.
    Keeps both alive."""

    def __init__(self, genome, store: ReadonlyTxStore, threads: int = 0):
        self._h = None
        self.genome, self.store = genome, store
        h = C.c_void_p()
        check(lib.gtars_txbind_new(store._h, _genome_handle(genome), int(threads), C.byref(h)))
        self._h = h

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib.gtars_txbind_free(self._h)
                self._h = None
        except Exception:
            pass

    def map(self, tx, kind, pos, offsets=None, star=None, on_host: bool = False, threads: int = 0):
        tx, kind, pos, offsets, star = _map_columns(tx, kind, pos, offsets, star)
        out, status = np.zeros(tx.size, dtype=np.uint64), np.zeros(tx.size, dtype=np.uint8)
        check(lib.gtars_txbind_map(self._h, ptr(tx), ptr(kind), ptr(pos), ptr(offsets) if offsets is not None else None,
                                   ptr(star) if star is not None else None, tx.size, 1 if on_host else 0, int(threads), ptr(out), ptr(status)))
        return out, status

    def map_device(self, d_tx: int, d_kind: int, d_pos: int, d_offset: int, d_star: int, n: int, d_out: int, d_status: int, stream: int = 0):
        """the mapping call for columns that are on the device already (u32 transcript numbers, u8 kinds, i64 positions, i64
        offsets or 0, u8 star flags or 0; outputs u64 values and u8 statuses), queued on ``stream``, which is drained before
        the call returns.  The current device must be the assembly's."""
        check(lib.gtars_tx_map_device(self._h, C.c_void_p(d_tx), C.c_void_p(d_kind), C.c_void_p(d_pos), C.c_void_p(d_offset), C.c_void_p(d_star),
                                      int(n), C.c_void_p(d_out), C.c_void_p(d_status), C.c_void_p(stream)))

    def digests_device(self, d_idx: int, n: int, d_status: int, d_digests: int, stream: int = 0):
        """sha512t24u of the mature mRNA of the transcripts numbered by a device column: u8 statuses and n * 32 digest bytes"""
        check(lib.gtars_tx_digests_device(self._h, C.c_void_p(d_idx), int(n), C.c_void_p(d_status), C.c_void_p(d_digests), C.c_void_p(stream)))

    def sequences(self, idx, want_digests: bool = True, want_sequences: bool = True, on_host: bool = False, threads: int = 0):
        """(statuses, digests or None, sequences or None) of the transcripts numbered ``idx``"""
        idx = np.ascontiguousarray(idx, dtype=np.uint32)
        n = idx.size
        status = np.zeros(n, dtype=np.uint8)
        digests = np.zeros(32 * n, dtype=np.uint8) if want_digests else None
        po, pb = C.c_void_p(), C.c_void_p()
        check(lib.gtars_txbind_sequences(self._h, ptr(idx), n, 1 if on_host else 0, int(threads), ptr(status),
                                         ptr(digests) if want_digests else None, C.byref(po) if want_sequences else None,
                                         C.byref(pb) if want_sequences else None))
        seqs = None
        if want_sequences:
            try:
                off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
                blob = C.string_at(pb, int(off[-1]))
            finally:
                lib.gtars_free(po)
                lib.gtars_free(pb)
            seqs = [blob[int(off[i]):int(off[i + 1])] for i in range(n)]
        texts = None
        if want_digests:
            raw = digests.tobytes()
            texts = [raw[32 * i:32 * i + 32].decode("ascii") if status[i] == 0 else None for i in range(n)]
        return status, texts, seqs


def _map_columns(tx, kind, pos, offsets, star):
    tx = np.ascontiguousarray(tx, dtype=np.uint32)
    n = tx.size
    kind = np.full(n, kind, dtype=np.uint8) if np.isscalar(kind) else np.ascontiguousarray(kind, dtype=np.uint8)
    pos = np.ascontiguousarray(pos, dtype=np.int64)
    offsets = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.int64)
    star = None if star is None else np.ascontiguousarray(star, dtype=np.uint8)
    for col in (kind, pos, offsets, star):
        if col is not None and col.size != n:
            raise ValueError("columns must have the same length")
    return tx, kind, pos, offsets, star


def _mapping_text(status: int, accession: str, pos: int, offset: int) -> str:
    return {1: f"Transcript not found: {accession}", 2: "Non-coding transcript has no CDS", 3: f"Position {pos} is outside CDS",
            4: f"Position {pos} is outside transcript", 5: f"5' UTR position c.{pos} extends beyond transcript start",
            6: f"3' UTR position c.*{pos} extends beyond transcript end",
            7: f"Intronic offset {offset} at transcript position {pos} is invalid (not at exon boundary)",
            10: f"Transcript {accession} has exons that are not ascending and disjoint"}.get(status, f"mapping failed with status {status}")


class CoordinateMapper:
    """``CoordinateMapper(store)``: the reference's scalar calls, on the host.  ``CoordinateMapper(store, genome)`` also binds the
    store to an assembly, whose device then runs the batch calls; without a genome the batch calls need ``on_host=True``."""

    def __init__(self, store: ReadonlyTxStore, genome=None):
        self.store = store
        self._bound = BoundTxStore(genome, store) if genome is not None else None

    # -- scalar calls ------------------------------------------------------------------------------------------------
    def _one(self, accession: str, index: int, kind: int, pos: int, offset: int, star: bool):
        tx = np.array([index if index >= 0 else NONE_U32], dtype=np.uint32)
        out, status = np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.uint8)
        # (named, so that the arrays outlive the call)
        kinds, poss = np.array([kind], dtype=np.uint8), np.array([pos], dtype=np.int64)
        offs, stars = np.array([offset], dtype=np.int64), np.array([1 if star else 0], dtype=np.uint8)
        check(lib.gtars_txstore_map(self.store._h, ptr(tx), ptr(kinds), ptr(poss), ptr(offs), ptr(stars), 1, 1, ptr(out), ptr(status)))
        if status[0] == 8:
            return None
        if status[0]:
            raise MappingError(_mapping_text(int(status[0]), accession, pos, offset))
        return int(out[0])

    @staticmethod
    def _i64(x) -> int:
        x = int(x)
        if not -(1 << 63) <= x < 1 << 63:
            raise OverflowError("position must fit in i64")
        return x

    def c_to_g(self, accession: str, c_pos: int, datum: Optional[int] = None, offset: int = 0) -> int:
        """HGVS c. position -> 0-based genomic position; ``datum=1`` reads ``c_pos`` as c.*N; ``offset``: the intronic offset"""
        return self._one(accession, self.store.index_of(accession), KIND_C, self._i64(c_pos), self._i64(offset), datum == 1)

    def n_to_g(self, accession: str, n_pos: int, offset: int = 0) -> int:
        return self._one(accession, self.store.index_of(accession), KIND_N, self._i64(n_pos), self._i64(offset), False)

    def g_to_transcript_offset(self, accession: str, g_pos: int) -> Optional[int]:
        """0-based genomic position -> 0-based offset on the mature mRNA, None when it lies in no exon"""
        g = int(g_pos)
        if not 0 <= g < 1 << 64:
            raise OverflowError("position must fit in u64")
        return self._one(accession, self.store.index_of(accession), KIND_G, g - (1 << 64) if g >= 1 << 63 else g, 0, False)

    def _full(self, accession: str, index: int, value: int) -> dict:
        tx = self.store.transcript(index)
        return {"chrom": tx.chrom, "chrom_accession": tx.chrom, "genomic_pos": value, "strand": tx.strand}

    def c_to_g_full(self, accession: str, c_pos: int, datum: Optional[int] = None) -> dict:
        """{"chrom", "chrom_accession" (both the "SQ." accession), "genomic_pos", "strand"}"""
        i = self.store.index_of(accession)
        return self._full(accession, i, self._one(accession, i, KIND_C, self._i64(c_pos), 0, datum == 1))

    def n_to_g_full(self, accession: str, n_pos: int) -> dict:
        i = self.store.index_of(accession)
        return self._full(accession, i, self._one(accession, i, KIND_N, self._i64(n_pos), 0, False))

    def c_to_g_by_gene(self, gene: str, c_pos: int, datum: Optional[int] = None) -> dict:
        """through the gene's MANE Select transcript; the dict also has "accession" """
        i = int(lib.gtars_txstore_lookup_mane(self.store._h, _text(gene)))
        if i < 0:
            raise MappingError(f"No MANE Select transcript for gene: {gene}")
        acc = self.store.transcript(i).accession
        d = self._full(acc, i, self._one(acc, i, KIND_C, self._i64(c_pos), 0, datum == 1))
        d["accession"] = acc
        return d

    # -- batch calls -------------------------------------------------------------------------------------------------
    def _many(self, accessions, kind, pos, offsets, star, on_host, threads):
        tx = self.store.indices_of(accessions, threads)
        if self._bound is not None:
            return self._bound.map(tx, kind, pos, offsets, star, on_host, threads)
        if not on_host:
            raise ValueError("the batch calls run on the device of an assembly: CoordinateMapper(store, genome), or on_host=True")
        tx, kind, pos, offsets, star = _map_columns(tx, kind, pos, offsets, star)
        out, status = np.zeros(tx.size, dtype=np.uint64), np.zeros(tx.size, dtype=np.uint8)
        check(lib.gtars_txstore_map(self.store._h, ptr(tx), ptr(kind), ptr(pos), ptr(offsets) if offsets is not None else None,
                                    ptr(star) if star is not None else None, tx.size, int(threads), ptr(out), ptr(status)))
        return out, status

    def c_to_g_many(self, accessions: Sequence[str], c_pos, offsets=None, datum=None, on_host: bool = False, threads: int = 0):
        """(values u64, statuses u8; 0 = ok, see MAP_STATUS_NAMES) of a batch of c. positions.  ``offsets``: intronic offsets;
        ``datum``: 1 where the position is c.*N (a scalar or a column).  Never raises for data."""
        star = None
        if datum is not None:
            star = (np.full(len(accessions), datum) if np.isscalar(datum) else np.asarray(datum)) == 1
        return self._many(accessions, KIND_C, c_pos, offsets, star, on_host, threads)

    def n_to_g_many(self, accessions: Sequence[str], n_pos, offsets=None, on_host: bool = False, threads: int = 0):
        return self._many(accessions, KIND_N, n_pos, offsets, None, on_host, threads)

    def g_to_transcript_offset_many(self, accessions: Sequence[str], g_pos, on_host: bool = False, threads: int = 0):
        """status 8: the position lies in no exon (the scalar call's None)"""
        g = np.ascontiguousarray(g_pos, dtype=np.uint64).view(np.int64)
        return self._many(accessions, KIND_G, g, None, None, on_host, threads)


def _bound(genome, store) -> BoundTxStore:
    return store if isinstance(store, BoundTxStore) else BoundTxStore(genome, store)


def mature_mrnas(genome, store, accessions: Optional[Sequence[str]] = None, on_host: bool = False, threads: int = 0,
                 with_status: bool = False):
    """the mature (spliced) mRNA reference sequence of a batch of transcripts (default: every transcript, in the store's
    order) as str; None for one that failed, or -- ``with_status`` -- (sequences, statuses; see SEQ_STATUS_NAMES).  ``store``:
    a ReadonlyTxStore, or a BoundTxStore that is kept between calls."""
    b = _bound(genome, store)
    idx = np.arange(len(b.store), dtype=np.uint32) if accessions is None else b.store.indices_of(accessions, threads)
    status, _, seqs = b.sequences(idx, want_digests=False, on_host=on_host, threads=threads)
    out = [s.decode("ascii") if st == 0 else None for s, st in zip(seqs, status)]
    return (out, status) if with_status else out


def mature_mrna(genome, store, accession: str, on_host: bool = False) -> str:
    """one transcript's mature mRNA; ValueError "Transcript not found: <accession>" or "Sequence not found: <digest>" """
    b = _bound(genome, store)
    seqs, status = mature_mrnas(genome, b, [accession], on_host=on_host, with_status=True)
    if status[0] == 0:
        return seqs[0]
    if status[0] == 1:
        raise ValueError(f"Transcript not found: {accession}")
    tx = b.store.lookup(accession)
    if status[0] == 2:
        raise ValueError(f"Sequence not found: {tx.chrom[3:]}")
    if status[0] == 3:
        raise ValueError(f"Transcript {accession} has an exon past the end of sequence {tx.chrom[3:]} (transcript / assembly mismatch)")
    raise ValueError(f"Transcript {accession} has exons that are not ascending and disjoint")


def transcript_accessions(genome, store, on_host: bool = False, threads: int = 0) -> Dict[str, str]:
    """accession -> "SQ." + sha512t24u of its mature mRNA, for every transcript whose sequence the assembly has"""
    b = _bound(genome, store)
    idx = np.arange(len(b.store), dtype=np.uint32)
    status, digests, _ = b.sequences(idx, want_sequences=False, on_host=on_host, threads=threads)
    names = b.store.accessions()
    return {names[i]: "SQ." + digests[i] for i in range(len(names)) if status[i] == 0}
