"""Refget: sequence digests, sequence collections and an in-memory store (gtars-python/py_src/gtars/refget/__init__.pyi,
gtars-refget/src/{digest,store}).

The reference's names keep their signatures and results: ``sha512t24u_digest``, ``md5_digest``, ``digest_sequence``,
``digest_fasta``, ``load_fasta``, ``compute_fai``, ``AlphabetType``, ``FaiMetadata``, ``FaiRecord``, ``SequenceMetadata``,
``SequenceRecord``, ``SeqColDigestLvl1``, ``SequenceCollectionMetadata``, ``SequenceCollection``, ``RetrievedSequence`` and
``RefgetStore.in_memory()``.  The scalar calls and ``compute_fai`` are host code and need no device.

``digest_fasta`` / ``load_fasta`` hash the records of a FASTA file on the device (csrc/refget.hip, DESIGN.md section 3,
K21): one lane per record computes sha512t24u, MD5 and the alphabet class in one pass; records longer than
``GTARS_REFGET_HOST_LEN`` bytes are hashed on the host threads meanwhile and never uploaded.  The store's region calls
(``substrings_from_regions``, ``export_fasta_from_regions``, ``substrings_many``) read a collection's packed device image,
built at the first such call.  ``on_host=True`` runs the library's own host path on its host threads instead: the same
results, no device.  Without a device the default calls raise NoDeviceError; there is no silent fallback.

``substrings_many``, ``digests_device`` and ``substrings_device`` are additive.  Not provided: persistence (``on_disk``,
``open_local``, ``write``), remote stores, encoded storage, aliases, FHR metadata, ``compare``, the attribute index,
``SequenceStream`` and ``ReadonlyRefgetStore``.  The module lives in ``gtars_amd`` only; ``gtars.refget`` is not registered.
"""
from __future__ import annotations

import ctypes as C
import glob as _glob
import gzip
import os
import re
from typing import Dict, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np

from ._lib import check, lib, ptr

KEEP_BYTES, ON_HOST, NO_DIGESTS = 1, 2, 4
SUB_STATUS_NAMES = ("ok", "sequence_not_found", "bad_range", "too_wide")
NONE_U32 = 0xFFFFFFFF


class AlphabetType:
    """AlphabetType.Dna2bit .. AlphabetType.Unknown; ``str()`` gives dna2bit, dna3bit, dnaio, protein, ASCII, Unknown"""

    _NAMES = ("Dna2bit", "Dna3bit", "DnaIupac", "Protein", "Ascii", "Unknown")
    _TEXT = ("dna2bit", "dna3bit", "dnaio", "protein", "ASCII", "Unknown")

    def __init__(self, value: int):
        self.value = int(value)

    @property
    def name(self) -> str:
        return self._NAMES[self.value]

    def __eq__(self, other):
        if isinstance(other, AlphabetType):
            return self.value == other.value
        if isinstance(other, int):
            return self.value == other
        return NotImplemented

    def __hash__(self):
        return hash(self.value)

    def __int__(self):
        return self.value

    def __repr__(self):
        return f"AlphabetType.{self.name}"

    def __str__(self):
        return self._TEXT[self.value]


for _i, _n in enumerate(AlphabetType._NAMES):
    setattr(AlphabetType, _n, AlphabetType(_i))


class FaiMetadata:
    def __init__(self, offset: int, line_bases: int, line_bytes: int):
        self.offset, self.line_bases, self.line_bytes = int(offset), int(line_bases), int(line_bytes)

    def __eq__(self, other):
        return isinstance(other, FaiMetadata) and (self.offset, self.line_bases, self.line_bytes) == (other.offset, other.line_bases, other.line_bytes)

    def __repr__(self):
        return f"FaiMetadata(offset={self.offset}, line_bases={self.line_bases}, line_bytes={self.line_bytes})"

    __str__ = __repr__


class FaiRecord:
    def __init__(self, name: str, length: int, fai: Optional[FaiMetadata]):
        self.name, self.length, self.fai = name, int(length), fai

    def __repr__(self):
        return f"FaiRecord(name={self.name!r}, length={self.length}, fai={self.fai!r})"

    __str__ = __repr__


class SequenceMetadata:
    def __init__(self, name: str, length: int, sha512t24u: str, md5: str, alphabet: AlphabetType, description: Optional[str] = None,
                 fai: Optional[FaiMetadata] = None):
        self.name, self.description, self.length = name, description, int(length)
        self.sha512t24u, self.md5, self.alphabet, self.fai = sha512t24u, md5, alphabet, fai

    def __repr__(self):
        return (f"SequenceMetadata(name={self.name!r}, length={self.length}, sha512t24u={self.sha512t24u!r}, md5={self.md5!r}, "
                f"alphabet={self.alphabet})")

    def __str__(self):
        return (f"SequenceMetadata for sequence {self.name}\n  length: {self.length}\n  sha512t24u: {self.sha512t24u}\n  md5: {self.md5}\n"
                f"  alphabet: {self.alphabet}")


class SequenceRecord:
    """``metadata`` and, when loaded, ``sequence``: the upper-cased bytes"""

    def __init__(self, metadata: SequenceMetadata, sequence: Optional[bytes] = None):
        self.metadata, self.sequence = metadata, sequence

    @property
    def is_loaded(self) -> bool:
        return self.sequence is not None

    def decode(self) -> Optional[str]:
        return None if self.sequence is None else self.sequence.decode("utf-8", "replace")

    def __repr__(self):
        return f"SequenceRecord(name={self.metadata.name!r}, length={self.metadata.length}, is_loaded={self.is_loaded})"

    def __str__(self):
        return f"SequenceRecord for {self.metadata.name} ({self.metadata.length} bp, {'loaded' if self.is_loaded else 'stub'})"


class SeqColDigestLvl1:
    def __init__(self, sequences_digest: str, names_digest: str, lengths_digest: str):
        self.sequences_digest, self.names_digest, self.lengths_digest = sequences_digest, names_digest, lengths_digest

    def __repr__(self):
        return (f"SeqColDigestLvl1(sequences_digest={self.sequences_digest!r}, names_digest={self.names_digest!r}, "
                f"lengths_digest={self.lengths_digest!r})")

    def __str__(self):
        return (f"SeqColDigestLvl1:\n  sequences_digest: {self.sequences_digest}\n  names_digest: {self.names_digest}\n"
                f"  lengths_digest: {self.lengths_digest}")


class SequenceCollectionMetadata:
    def __init__(self, digest, n_sequences, names_digest, sequences_digest, lengths_digest, name_length_pairs_digest=None,
                 sorted_name_length_pairs_digest=None, sorted_sequences_digest=None):
        self.digest, self.n_sequences = digest, int(n_sequences)
        self.names_digest, self.sequences_digest, self.lengths_digest = names_digest, sequences_digest, lengths_digest
        self.name_length_pairs_digest = name_length_pairs_digest
        self.sorted_name_length_pairs_digest = sorted_name_length_pairs_digest
        self.sorted_sequences_digest = sorted_sequences_digest

    def __repr__(self):
        return f"SequenceCollectionMetadata(digest={self.digest!r}, n_sequences={self.n_sequences})"

    def __str__(self):
        return f"SequenceCollectionMetadata for {self.digest} ({self.n_sequences} sequences)"


class _Handle:
    """owns one gtars_seqcol_t"""

    def __init__(self, h):
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib.gtars_seqcol_free(self.h)
                self.h = None
        except Exception:
            pass

    def __len__(self):
        return int(lib.gtars_seqcol_len(self.h))

    @classmethod
    def from_path(cls, path, flags: int, threads: int = 0) -> "_Handle":
        h = C.c_void_p()
        check(lib.gtars_seqcol_from_fasta(os.fspath(path).encode("utf-8"), int(flags), int(threads), C.byref(h)))
        return cls(h)

    @classmethod
    def from_bytes(cls, text: bytes, flags: int, threads: int = 0) -> "_Handle":
        h = C.c_void_p()
        check(lib.gtars_seqcol_from_fasta_bytes(text, len(text), int(flags), int(threads), C.byref(h)))
        return cls(h)

    def record(self, i: int, with_bytes: bool) -> SequenceRecord:
        name, desc, seq = C.c_void_p(), C.c_void_p(), C.c_void_p()
        length, off = C.c_uint64(), C.c_uint64()
        has_fai, alphabet = C.c_int(), C.c_int()
        bases, nbytes = C.c_uint32(), C.c_uint32()
        sha, md5 = C.create_string_buffer(33), C.create_string_buffer(33)
        check(lib.gtars_seqcol_record(self.h, int(i), C.byref(name), C.byref(desc), C.byref(length), C.byref(has_fai), C.byref(off),
                                      C.byref(bases), C.byref(nbytes), sha, md5, C.byref(alphabet), C.byref(seq)))
        fai = FaiMetadata(off.value, bases.value, nbytes.value) if has_fai.value else None
        meta = SequenceMetadata(C.string_at(name).decode("utf-8", "replace"), length.value, sha.value.decode("ascii"), md5.value.decode("ascii"),
                                AlphabetType(alphabet.value), C.string_at(desc).decode("utf-8", "replace") if desc.value else None, fai)
        data = None
        if with_bytes and (seq.value or length.value == 0):
            data = C.string_at(seq, length.value).upper() if length.value else b""
        return SequenceRecord(meta, data)

    def digests(self) -> List[str]:
        buf = C.create_string_buffer(7 * 33)
        check(lib.gtars_seqcol_digests(self.h, buf))
        return [buf.raw[33 * k:33 * k + 32].decode("ascii") for k in range(7)]

    def substrings(self, seq, start, end, on_host: bool, threads: int = 0):
        seq = np.ascontiguousarray(seq, dtype=np.uint32)
        start, end = np.ascontiguousarray(start, dtype=np.uint64), np.ascontiguousarray(end, dtype=np.uint64)
        n = seq.size
        if start.size != n or end.size != n:
            raise ValueError("columns must have the same length")
        status = np.zeros(n, dtype=np.uint8)
        po, pb = C.c_void_p(), C.c_void_p()
        check(lib.gtars_seqcol_substrings(self.h, ptr(seq), ptr(start), ptr(end), n, 1 if on_host else 0, int(threads), ptr(status),
                                          C.byref(po), C.byref(pb)))
        try:
            off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
            blob = C.string_at(pb, int(off[-1]))
        finally:
            lib.gtars_free(po)
            lib.gtars_free(pb)
        return status, off, blob


class SequenceCollection:
    """the records of one FASTA file (or one list of records) with the collection digests of the GA4GH seqcol specification"""

    def __init__(self, sequences: List[SequenceRecord], digest: str, lvl1: SeqColDigestLvl1, file_path: Optional[str] = None,
                 ancillary: Optional[Tuple[str, str, str]] = None, handle: Optional[_Handle] = None):
        self.sequences, self.digest, self.lvl1, self.file_path = sequences, digest, lvl1, file_path
        self._ancillary, self._handle = ancillary, handle

    @classmethod
    def from_records(cls, records: Sequence[SequenceRecord]) -> "SequenceCollection":
        """a collection over records that have their digests already (``digest_sequence``)"""
        d = _collection_digests([r.metadata.name for r in records], [r.metadata.length for r in records],
                                [r.metadata.sha512t24u for r in records])
        return cls(list(records), d[0], SeqColDigestLvl1(d[2], d[1], d[3]), None, (d[4], d[5], d[6]))

    def metadata(self) -> SequenceCollectionMetadata:
        anc = self._ancillary or (None, None, None)
        return SequenceCollectionMetadata(self.digest, len(self.sequences), self.lvl1.names_digest, self.lvl1.sequences_digest,
                                          self.lvl1.lengths_digest, *anc)

    def write_fasta(self, file_path, line_width: Optional[int] = None) -> None:
        width = 70 if line_width is None else int(line_width)
        for r in self.sequences:
            if r.sequence is None:
                raise IOError(f"Sequence '{r.metadata.name}' has no data loaded")
        with open(os.fspath(file_path), "wb") as f:
            for r in self.sequences:
                _write_record(f, r, width)

    def __len__(self) -> int:
        return len(self.sequences)

    def __getitem__(self, idx: int) -> SequenceRecord:
        return self.sequences[idx]

    def __iter__(self) -> Iterator[SequenceRecord]:
        return iter(self.sequences)

    def __repr__(self):
        return f"SequenceCollection(n_sequences={len(self.sequences)}, digest={self.digest!r})"

    def __str__(self):
        return f"SequenceCollection with {len(self.sequences)} sequences, digest: {self.digest}"


class RetrievedSequence:
    def __init__(self, sequence: str, chrom_name: str, start: int, end: int):
        self.sequence, self.chrom_name, self.start, self.end = sequence, chrom_name, int(start), int(end)

    def __eq__(self, other):
        return isinstance(other, RetrievedSequence) and (self.sequence, self.chrom_name, self.start, self.end) == (
            other.sequence, other.chrom_name, other.start, other.end)

    def __repr__(self):
        return f"RetrievedSequence(sequence={self.sequence!r}, chrom_name={self.chrom_name!r}, start={self.start}, end={self.end})"

    def __str__(self):
        return f"{self.chrom_name}|{self.start}-{self.end}: {self.sequence}"


def _write_record(f, r: SequenceRecord, width: int) -> None:
    m = r.metadata
    f.write((f">{m.name} {m.description}\n" if m.description is not None else f">{m.name}\n").encode("utf-8"))
    for at in range(0, len(r.sequence), width):
        f.write(r.sequence[at:at + width] + b"\n")


def _data(readable, what: str) -> bytes:
    if isinstance(readable, str):
        return readable.encode("utf-8")
    if isinstance(readable, (bytes, bytearray, memoryview)):
        return bytes(readable)
    raise TypeError(f"{what} expects str or bytes")


def sha512t24u_digest(readable: Union[str, bytes]) -> str:
    """the GA4GH digest of the bytes as given (no upper-casing): 32 base64url characters"""
    data = _data(readable, "sha512t24u_digest")
    out = C.create_string_buffer(33)
    check(lib.gtars_sha512t24u(data, len(data), out))
    return out.value.decode("ascii")


def md5_digest(readable: Union[str, bytes]) -> str:
    """MD5 of the bytes as given: 32 hex characters"""
    data = _data(readable, "md5_digest")
    out = C.create_string_buffer(33)
    check(lib.gtars_md5(data, len(data), out))
    return out.value.decode("ascii")


def guess_alphabet(readable: Union[str, bytes]) -> AlphabetType:
    """the most general alphabet class among the bytes, read upper-cased (additive)"""
    data = _data(readable, "guess_alphabet")
    return AlphabetType(lib.gtars_refget_alphabet(data, len(data)))


def alphabet_class_table() -> np.ndarray:
    """the class 0 .. 4 of every byte value (additive)"""
    out = np.zeros(256, dtype=np.uint8)
    lib.gtars_refget_class_table(ptr(out))
    return out


def digest_sequence(data: Union[str, bytes], name: Optional[str] = None, description: Optional[str] = None) -> SequenceRecord:
    """a loaded record over the upper-cased bytes, with its digests; host code"""
    seq = _data(data, "digest_sequence").upper()
    meta = SequenceMetadata("" if name is None else name, len(seq), sha512t24u_digest(seq), md5_digest(seq), guess_alphabet(seq), description)
    return SequenceRecord(meta, seq)


def _collection_digests(names, lengths, digests) -> List[str]:
    """[collection digest, names, sequences, lengths, name_length_pairs, sorted_name_length_pairs, sorted_sequences] of records
    that did not come from a FASTA text (whose digests the library computes itself): the canonical JSON of
    algorithms.rs:59-110 -- compact, keys sorted, UTF-8 as it is -- hashed by the library"""
    import json

    def canon(v):
        return json.dumps(v, separators=(",", ":"), sort_keys=True, ensure_ascii=False).encode("utf-8")

    seqs = ["SQ." + d for d in digests]
    pairs = [{"length": int(n), "name": s} for s, n in zip(names, lengths)]
    lvl = [sha512t24u_digest(canon(list(names))), sha512t24u_digest(canon(seqs)), sha512t24u_digest(canon([int(n) for n in lengths]))]
    top = sha512t24u_digest(canon({"names": lvl[0], "sequences": lvl[1]}))
    return [top, lvl[0], lvl[1], lvl[2], sha512t24u_digest(canon(pairs)),
            sha512t24u_digest(canon(sorted(sha512t24u_digest(canon(p)) for p in pairs))), sha512t24u_digest(canon(sorted(seqs)))]


def _collection_of(h: _Handle, path: Optional[str], loaded: bool) -> SequenceCollection:
    recs = [h.record(i, loaded) for i in range(len(h))]
    d = h.digests()
    return SequenceCollection(recs, d[0], SeqColDigestLvl1(d[2], d[1], d[3]), path, (d[4], d[5], d[6]), h if loaded else None)


def digest_fasta(fasta, on_host: bool = False, threads: int = 0) -> SequenceCollection:
    """the records of a FASTA file (plain or gzip) with their digests, sequence data not loaded"""
    path = os.fspath(fasta)
    return _collection_of(_Handle.from_path(path, ON_HOST if on_host else 0, threads), path, False)


def load_fasta(fasta, on_host: bool = False, threads: int = 0) -> SequenceCollection:
    """as ``digest_fasta``, with every record's upper-cased bytes loaded"""
    path = os.fspath(fasta)
    return _collection_of(_Handle.from_path(path, KEEP_BYTES | (ON_HOST if on_host else 0), threads), path, True)


def compute_fai(fasta) -> List[FaiRecord]:
    """name, length and FAI data of every record; host code.  ``fai`` is None for gzip input"""
    h = _Handle.from_path(os.fspath(fasta), NO_DIGESTS)
    out = []
    for i in range(len(h)):
        m = h.record(i, False).metadata
        out.append(FaiRecord(m.name, m.length, m.fai))
    return out


def _image_handle(records: Sequence[SequenceRecord]) -> _Handle:
    """a collection handle over loaded records, for the device image: one stand-in FASTA record per sequence"""
    parts = []
    for i, r in enumerate(records):
        if r.sequence is None:
            raise KeyError("Sequence data not loaded (stub only)")
        if r.sequence and (r.sequence[-1:].isspace() or b"\n" in r.sequence or b"\r" in r.sequence):
            raise ValueError(f"sequence '{r.metadata.name}' holds line breaks: it cannot be placed in a device image")
        parts.append(b">%d\n%s\n" % (i, r.sequence))
    return _Handle.from_bytes(b"".join(parts), KEEP_BYTES | NO_DIGESTS)


class RefgetStore:
    """``RefgetStore.in_memory()``: sequences by digest, collections by digest, names per collection"""

    def __init__(self):
        self._seqs: Dict[str, SequenceRecord] = {}
        self._md5: Dict[str, str] = {}
        self._cols: Dict[str, SequenceCollectionMetadata] = {}
        self._names: Dict[str, Dict[str, str]] = {}   # collection -> name -> sha512t24u (a repeated name: its last record)
        self._records: Dict[str, List[SequenceRecord]] = {}  # collection -> its records in order
        self._handles: Dict[str, _Handle] = {}

    @classmethod
    def in_memory(cls) -> "RefgetStore":
        return cls()

    # -- adding ----------------------------------------------------------------------------------------------------------
    def add_sequence(self, sequence: SequenceRecord, force: bool = False) -> None:
        key = sequence.metadata.sha512t24u
        if key in self._seqs and not force and (self._seqs[key].is_loaded or not sequence.is_loaded):
            return
        self._seqs[key] = sequence
        self._md5[sequence.metadata.md5] = key

    def add_sequence_collection(self, collection: SequenceCollection, force: bool = False) -> Tuple[SequenceCollectionMetadata, bool]:
        if collection.digest in self._cols and not force:
            return self._cols[collection.digest], False
        was_new = collection.digest not in self._cols
        meta = collection.metadata()
        if meta.name_length_pairs_digest is None:
            d = _collection_digests([r.metadata.name for r in collection], [r.metadata.length for r in collection],
                                    [r.metadata.sha512t24u for r in collection])
            meta.name_length_pairs_digest, meta.sorted_name_length_pairs_digest, meta.sorted_sequences_digest = d[4], d[5], d[6]
        self._cols[collection.digest] = meta
        names = self._names.setdefault(collection.digest, {})
        for r in collection:
            names[r.metadata.name] = r.metadata.sha512t24u
            self.add_sequence(r, force)
        self._records[collection.digest] = list(collection.sequences)
        self._handles.pop(collection.digest, None)
        if collection._handle is not None:
            self._handles[collection.digest] = collection._handle
        return meta, was_new

    def add_sequence_collection_from_fasta(self, file_path, force: bool = False, on_host: bool = False, threads: int = 0,
                                           **_ignored) -> Tuple[SequenceCollectionMetadata, bool]:
        return self.add_sequence_collection(load_fasta(file_path, on_host=on_host, threads=threads), force)

    def add_sequence_collections_from_fastas(self, fastas=(), file_list=None, force: bool = False, on_host: bool = False, threads: int = 0,
                                             **_ignored) -> List[Tuple[SequenceCollectionMetadata, bool]]:
        """``fastas``: a list of paths, or one glob pattern (expanded in sorted order; ValueError when nothing matches);
        ``file_list``: a text file of paths, blank lines and ``#`` lines ignored"""
        if isinstance(fastas, (str, os.PathLike)):
            pattern = os.fspath(fastas)
            paths = sorted(_glob.glob(pattern))
            if not paths:
                raise ValueError(f"glob pattern matched no files: {pattern}")
        else:
            paths = [os.fspath(p) for p in fastas]
        if file_list is not None:
            with open(os.fspath(file_list), "rt", encoding="utf-8") as f:
                for line in f:
                    line = line.strip()
                    if line and not line.startswith("#"):
                        paths.append(line)
        return [self.add_sequence_collection_from_fasta(p, force, on_host, threads) for p in paths]

    # -- collections -----------------------------------------------------------------------------------------------------
    def list_collections(self, *_args, **_kwargs) -> List[SequenceCollectionMetadata]:
        return [self._cols[k] for k in sorted(self._cols)]

    def get_collection_metadata(self, collection_digest: str) -> Optional[SequenceCollectionMetadata]:
        return self._cols.get(collection_digest)

    def is_collection_loaded(self, collection_digest: str) -> bool:
        return collection_digest in self._names

    def get_collection(self, collection_digest: str) -> SequenceCollection:
        """the collection with its records: one per name, in the order the names first appeared (the store keeps names in an
        insertion-ordered map, so a repeated name shows once, with its last record's digest)"""
        if collection_digest not in self._cols:
            raise KeyError(f"Collection not found: {collection_digest}")
        m = self._cols[collection_digest]
        recs = []
        for name, sha in self._names[collection_digest].items():
            r = self._seqs[sha]
            if r.metadata.name != name:
                md = r.metadata
                r = SequenceRecord(SequenceMetadata(name, md.length, md.sha512t24u, md.md5, md.alphabet, md.description, md.fai), r.sequence)
            recs.append(r)
        return SequenceCollection(recs, m.digest, SeqColDigestLvl1(m.sequences_digest, m.names_digest, m.lengths_digest), None,
                                  (m.name_length_pairs_digest, m.sorted_name_length_pairs_digest, m.sorted_sequences_digest))

    def iter_collections(self) -> List[SequenceCollection]:
        return [self.get_collection(k) for k in sorted(self._cols)]

    def get_collection_level1(self, digest: str) -> dict:
        if digest not in self._cols:
            raise KeyError(f"Collection not found: {digest}")
        m = self._cols[digest]
        return {"names": m.names_digest, "lengths": m.lengths_digest, "sequences": m.sequences_digest,
                "name_length_pairs": m.name_length_pairs_digest, "sorted_name_length_pairs": m.sorted_name_length_pairs_digest,
                "sorted_sequences": m.sorted_sequences_digest}

    def get_collection_level2(self, digest: str) -> dict:
        if digest not in self._cols:
            raise KeyError(f"Collection not found: {digest}")
        recs = self._records[digest]
        seqs = ["SQ." + r.metadata.sha512t24u for r in recs]
        return {"names": [r.metadata.name for r in recs], "lengths": [r.metadata.length for r in recs], "sequences": seqs,
                "name_length_pairs": [{"length": r.metadata.length, "name": r.metadata.name} for r in recs],
                "sorted_sequences": sorted(seqs)}

    # -- sequences -------------------------------------------------------------------------------------------------------
    def _key(self, digest: str) -> str:
        return self._md5.get(digest, digest)

    def list_sequences(self) -> List[SequenceMetadata]:
        return [self._seqs[k].metadata for k in sorted(self._seqs)]

    def get_sequence_metadata(self, seq_digest: str) -> Optional[SequenceMetadata]:
        r = self._seqs.get(self._key(seq_digest))
        return None if r is None else r.metadata

    def get_sequence(self, digest: str) -> SequenceRecord:
        """by sha512t24u or by MD5; KeyError for a digest the store lacks"""
        r = self._seqs.get(self._key(digest))
        if r is None:
            raise KeyError(f"Sequence not found: {digest}")
        return r

    def get_sequence_by_name(self, collection_digest: str, sequence_name: str) -> SequenceRecord:
        """a repeated name gives its LAST record: the store's name map keeps one digest per name, and a later insert replaces it"""
        if collection_digest not in self._names:
            raise KeyError("Collection not loaded. Call load_collection() or load_all_collections() first.")
        sha = self._names[collection_digest].get(sequence_name)
        if sha is None:
            raise KeyError(f"Sequence '{sequence_name}' not found in collection")
        return self._seqs[sha]

    def iter_sequences(self) -> List[SequenceRecord]:
        return [self._seqs[k] for k in sorted(self._seqs)]

    def get_substring(self, seq_digest: str, start: int, end: int) -> str:
        """bases [start, end) of one sequence; host code.  ``start == end`` is the empty string wherever it lies; KeyError for an
        unknown digest and for a range that is inverted or passes the sequence's end"""
        r = self._seqs.get(self._key(seq_digest))
        if r is None:
            raise KeyError(f"Sequence not found: {seq_digest}")
        start, end = int(start), int(end)
        if start == end:
            return ""
        if r.sequence is None:
            raise KeyError("Sequence data not loaded (stub only)")
        n = r.metadata.length
        if start < 0 or start >= n or end > n or start >= end:
            raise KeyError(f"Invalid substring range: start={start}, end={end}, sequence length={n}")
        return r.sequence[start:end].decode("utf-8", "replace")

    # -- regions ---------------------------------------------------------------------------------------------------------
    def _image(self, collection_digest: str) -> _Handle:
        if collection_digest not in self._records:
            raise KeyError("Collection not loaded. Call load_collection() or load_all_collections() first.")
        h = self._handles.get(collection_digest)
        if h is None:
            h = self._handles[collection_digest] = _image_handle(self._records[collection_digest])
        return h

    def _rows_of(self, collection_digest: str, chroms: Sequence[str]) -> np.ndarray:
        recs = self._records[collection_digest]
        last = {r.metadata.name: i for i, r in enumerate(recs)}  # (a repeated name: its last record)
        return np.array([last.get(c, NONE_U32) for c in chroms], dtype=np.uint32)

    def substrings_from_regions(self, collection_digest: str, bed_file_path, on_host: bool = False, threads: int = 0) -> List[RetrievedSequence]:
        """the sequence of every region of a BED file, from the collection's device image; a region that fails raises
        ValueError with the reference's message"""
        chroms, starts, ends = _read_bed(bed_file_path)
        return _regions(self, collection_digest, chroms, starts, ends, "Line", 2, on_host, threads)

    def export_fasta_from_regions(self, collection_digest: str, bed_file_path, output_file_path, on_host: bool = False, threads: int = 0) -> None:
        """one ``>{chrom}:{start}-{end}`` record per region; gzip when the name ends in ".gz" """
        out = os.fspath(output_file_path)
        parent = os.path.dirname(out)
        if parent:
            os.makedirs(parent, exist_ok=True)
        with (gzip.open(out, "wb") if out.endswith(".gz") else open(out, "wb")) as f:
            for rs in self.substrings_from_regions(collection_digest, bed_file_path, on_host, threads):
                f.write(f">{rs.chrom_name}:{rs.start}-{rs.end}\n{rs.sequence}\n".encode("utf-8"))

    def export_fasta(self, collection_digest: str, output_path, sequence_names: Optional[Sequence[str]] = None,
                     line_width: Optional[int] = None) -> None:
        if collection_digest not in self._names:
            raise KeyError(f"Collection not found: {collection_digest!r}")
        names = self._names[collection_digest]
        width = 80 if line_width is None else int(line_width)
        out = os.fspath(output_path)
        with (gzip.open(out, "wb") if out.endswith(".gz") else open(out, "wb")) as f:
            for name in (list(names) if sequence_names is None else sequence_names):
                if name not in names:
                    raise KeyError(f"Sequence '{name}' not found in collection")
                r = self._seqs[names[name]]
                if r.sequence is None:
                    raise KeyError(f"Sequence data not loaded for '{name}'. Call load_sequence() or load_all_sequences() first.")
                _write_record(f, r, width)

    def __len__(self) -> int:
        return len(self._seqs)

    def __iter__(self) -> Iterator[SequenceMetadata]:
        return iter(self.list_sequences())

    def __repr__(self):
        return f"RefgetStore(n_sequences={len(self._seqs)}, n_collections={len(self._cols)}, memory-only)"

    __str__ = __repr__


def _read_bed(path) -> Tuple[List[str], List[int], List[int]]:
    """parse_bedlike_file: tab-separated; a start or end that is no i32 counts as -1"""
    path = os.fspath(path)
    chroms, starts, ends = [], [], []

    def num(fields, k):
        v = int(fields[k]) if len(fields) > k and re.fullmatch(r"[+-]?[0-9]+", fields[k]) else -1
        return v if -(1 << 31) <= v < 1 << 31 else -1

    with (gzip.open(path, "rt", encoding="utf-8") if path.endswith(".gz") else open(path, "rt", encoding="utf-8")) as f:
        for line in f:
            fields = line.strip().split("\t")
            chroms.append(fields[0])
            starts.append(num(fields, 1))
            ends.append(num(fields, 2))
    return chroms, starts, ends


def _regions(store: RefgetStore, collection_digest: str, chroms, starts, ends, label: str, first: int, on_host: bool, threads: int):
    for i, (s, e) in enumerate(zip(starts, ends)):
        if s < 0 or e < 0:
            raise ValueError(f"{label} {i + first} has invalid start or end coordinates: start={s}, end={e}")
    seqs, status = substrings_many(store, collection_digest, chroms, starts, ends, on_host=on_host, threads=threads, with_status=True)
    bad = np.flatnonzero(status)
    if bad.size:
        i = int(bad[0])
        where = f"{label} {i + first}"
        if status[i] == 1:
            raise ValueError(f"{where}: sequence '{chroms[i]}' not found in collection '{collection_digest}': "
                             f"Sequence '{chroms[i]}' not found in collection")
        rec = store.get_sequence_by_name(collection_digest, chroms[i])
        raise ValueError(f"{where}: failed to get substring for digest '{rec.metadata.sha512t24u}' from {starts[i]} to {ends[i]}: "
                         f"Invalid substring range: start={starts[i]}, end={ends[i]}, sequence length={rec.metadata.length}")
    return [RetrievedSequence(q, c, s, e) for q, c, s, e in zip(seqs, chroms, starts, ends)]


def substrings_many(store: RefgetStore, collection_digest: str, chroms: Sequence[str], starts, ends, on_host: bool = False,
                    with_status: bool = False, threads: int = 0):
    """the upper-cased sequence of a batch of regions of one collection, from its packed device image (built at the first
    call): str per region, None for one that failed, or -- ``with_status`` -- (sequences, statuses; see SUB_STATUS_NAMES).
    A name the collection has twice means its last record.  Never raises for data."""
    h = store._image(collection_digest)
    rows = store._rows_of(collection_digest, chroms)
    status, off, blob = h.substrings(rows, starts, ends, on_host, threads)
    out = [blob[int(off[i]):int(off[i + 1])].decode("utf-8", "replace") if status[i] == 0 else None for i in range(len(rows))]
    return (out, status) if with_status else out


def digests_device(collection: Union[SequenceCollection, _Handle], d_digests: int = 0, d_md5: int = 0, d_class: int = 0, stream: int = 0) -> None:
    """sha512t24u, MD5 and alphabet class of every record of a loaded collection (``load_fasta``) into columns that are on the
    device already: n * 32 characters and n * 16 bytes (both 8-byte aligned), n classes; any may be 0.  Queued on ``stream``,
    which is drained before the call returns.  The current device must be the one that holds the collection's image."""
    check(lib.gtars_refget_digests_device(_handle_of(collection).h, C.c_void_p(d_digests), C.c_void_p(d_md5), C.c_void_p(d_class),
                                          C.c_void_p(stream)))


def substrings_device(collection: Union[SequenceCollection, _Handle], d_seq: int, d_start: int, d_end: int, n: int, d_status: int,
                      d_offsets: int, d_bytes: int, cap: int, stream: int = 0) -> int:
    """substrings for columns that are on the device already (u32 record numbers, u64 starts and ends; outputs u8 statuses,
    n + 1 u64 offsets, ``cap`` bytes) -> the bytes needed; CapacityError when that is more than ``cap``"""
    total = C.c_uint64()
    check(lib.gtars_refget_substrings_device(_handle_of(collection).h, C.c_void_p(d_seq), C.c_void_p(d_start), C.c_void_p(d_end), int(n),
                                             C.c_void_p(d_status), C.c_void_p(d_offsets), C.c_void_p(d_bytes), int(cap), C.byref(total),
                                             C.c_void_p(stream)))
    return int(total.value)


def digest_records(collection: Union[SequenceCollection, _Handle], on_host: bool = False, threads: int = 0):
    """(sha512t24u texts, MD5 hex texts, classes u8) of every record of a loaded collection, hashed again from its full
    device image (additive; ``digest_fasta`` is the call for a file)"""
    h = _handle_of(collection)
    n = len(h)
    text, md5, cls = np.zeros(32 * n, dtype=np.uint8), np.zeros(16 * n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    check(lib.gtars_seqcol_digest_records(h.h, 1 if on_host else 0, int(threads), ptr(text), ptr(md5), ptr(cls)))
    raw, m = text.tobytes(), md5.tobytes()
    return [raw[32 * i:32 * i + 32].decode("ascii") for i in range(n)], [m[16 * i:16 * i + 16].hex() for i in range(n)], cls


def _handle_of(collection) -> _Handle:
    if isinstance(collection, _Handle):
        return collection
    if collection._handle is None:
        collection._handle = _image_handle(collection.sequences)
    return collection._handle
