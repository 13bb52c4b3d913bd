"""Refget: sequence digests, sequence collections and an in-memory store (gtars-python/py_src/gtars/refget/__init__.pyi,
gtars-refget/src/{digest,store}).

The reference's names keep their signatures and results: ``sha512t24u_digest``, ``md5_digest``, ``digest_sequence``,
``digest_fasta``, ``load_fasta``, ``compute_fai``, ``AlphabetType``, ``FaiMetadata``, ``FaiRecord``, ``SequenceMetadata``,
``SequenceRecord``, ``SeqColDigestLvl1``, ``SequenceCollectionMetadata``, ``SequenceCollection``, ``RetrievedSequence`` and
``RefgetStore.in_memory()``.  The scalar calls and ``compute_fai`` are host code and need no device.

``digest_fasta`` / ``load_fasta`` hash the records of a FASTA file on the device (csrc/refget.hip, DESIGN.md section 3,
K21): one lane per record computes sha512t24u, MD5 and the alphabet class in one pass; records longer than
``GTARS_REFGET_HOST_LEN`` bytes are hashed on the host threads meanwhile and never uploaded.  The store's region calls
(``substrings_from_regions``, ``export_fasta_from_regions``, ``substrings_many``, ``get_substrings``) read a collection's device
image, built at the first such call.  ``on_host=True`` runs the library's own host path on its host threads instead: the same
results, no device.  Without a device the default calls raise NoDeviceError; there is no silent fallback.

The store persists: ``RefgetStore.on_disk`` / ``open_local`` / ``write`` / ``write_store_to_dir`` /
``enable_persistence`` read and write the reference's store directory -- ``rgstore.json``, ``sequences.rgsi``,
``collections.rgci``, ``collections/<digest>.rgsi`` and one ``.seq`` file per sequence -- byte for byte.  ``StorageMode.Encoded``
keeps every sequence bit-packed at the 2 / 3 / 4 / 5 / 8 bits of its alphabet class: ``SequenceRecord.sequence`` then holds the
packed bytes and ``decode()`` gives the text.  A collection's region calls read its packed image on the device, built once per
collection: by ``k_refget_pack`` from the raw image when the text is resident, straight from the ``.seq`` files when the records
are stubs (the files' bytes are uploaded as they are; the payload never passes through Python objects).  The scalar
``get_substring`` on a stub reads only the bytes of the file that hold the range and decodes them on the host.  The IUPAC tables
are the reference's and are no inverse pair: D comes back as H, H as V, U as T.

``RefgetStore.in_memory()`` stays a ``Raw`` store whose records hold text (the reference's in-memory default is ``Encoded``;
``enable_encoding()`` gives that).  ``substrings_many``, ``digests_device``, ``substrings_device``, ``packed_image``, the ``on_host`` / ``threads``
arguments and the scalar ``encode_sequence`` / ``decode_substring`` / ``byte_range_for_bases`` / ``bits_per_symbol`` are additive.  Not provided: remote stores, aliases, FHR metadata, ``compare``, the attribute index,
``SequenceStream`` and ``ReadonlyRefgetStore``.  The module lives in ``gtars_amd`` only; ``gtars.refget`` is not registered.
"""
from __future__ import annotations

import ctypes as C
import glob as _glob
import gzip
import hashlib
import json
import os
import re
import time
from typing import Dict, Iterator, List, Optional, Sequence, Tuple, Union

import numpy as np

from ._lib import check, cstr_array, lib, ptr

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


def _alphabet_of(text: str) -> AlphabetType:
    """the class an index file names; anything unknown is ``Unknown``"""
    return AlphabetType(AlphabetType._TEXT.index(text) if text in AlphabetType._TEXT else 5)


class StorageMode:
    """StorageMode.Raw: sequences as upper-case text; StorageMode.Encoded: bit-packed by alphabet class"""

    _NAMES = ("Raw", "Encoded")

    def __init__(self, value: int):
        self.value = int(value)

    @property
    def name(self) -> str:
        return self._NAMES[self.value]

    def __eq__(self, other):
        return self.value == other.value if isinstance(other, StorageMode) else NotImplemented

    def __hash__(self):
        return hash(self.value)

    def __repr__(self):
        return f"StorageMode.{self.name}"

    def __str__(self):
        return self.name


StorageMode.Raw, StorageMode.Encoded = StorageMode(0), StorageMode(1)


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
    """``metadata`` and, when loaded, ``sequence``: the upper-cased bytes, or -- in a store whose mode is ``Encoded`` -- the
    bytes bit-packed by ``metadata.alphabet`` (``encoded``); ``decode()`` gives the text of either"""

    def __init__(self, metadata: SequenceMetadata, sequence: Optional[bytes] = None, encoded: bool = False):
        self.metadata, self.sequence, self.encoded = metadata, sequence, bool(encoded) and sequence is not None

    @property
    def is_loaded(self) -> bool:
        return self.sequence is not None

    def decode(self) -> Optional[str]:
        if self.sequence is None:
            return None
        data = decode_substring(self.sequence, 0, self.metadata.length, self.metadata.alphabet) if self.encoded else self.sequence
        return data.decode("utf-8", "replace")

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

    @classmethod
    def from_seq_files(cls, paths: Sequence[str], lengths: Sequence[int], threads: int = 0) -> "_Handle":
        """the text ``.seq`` files of a Raw store as a collection with its bytes kept: read by the library"""
        arr, keep = cstr_array([os.fspath(p) for p in paths])
        length = np.ascontiguousarray(lengths, dtype=np.uint64)
        h = C.c_void_p()
        check(lib.gtars_seqcol_from_seq_files(C.cast(arr, C.c_void_p), ptr(length), len(keep), int(threads), C.byref(h)))
        return cls(h)

    @classmethod
    def from_buffers(cls, sequences: Sequence[bytes]) -> "_Handle":
        """loaded sequences as a collection with its bytes kept (no stand-in FASTA text)"""
        arr = (C.c_char_p * max(len(sequences), 1))(*sequences)
        length = np.array([len(q) for q in sequences], dtype=np.uint64)
        h = C.c_void_p()
        check(lib.gtars_seqcol_from_buffers(C.cast(arr, C.c_void_p), ptr(length), len(sequences), C.byref(h)))
        return cls(h)

    def write_files(self, paths: Sequence[Optional[str]], threads: int = 0) -> None:
        """every record's upper-cased bytes into its file (None: skipped), written by the library"""
        arr, _keep = cstr_array([None if p is None else os.fspath(p) for p in paths])
        check(lib.gtars_seqcol_write_files(self.h, C.cast(arr, C.c_void_p), int(threads)))

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


def _take_csr(po, pb, n: int):
    try:
        off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
        blob = C.string_at(pb, int(off[-1]))
    finally:
        lib.gtars_free(po)
        lib.gtars_free(pb)
    return off, blob


class _Pack:
    """owns one gtars_seqpack_t: a collection's bit-packed image (host copy, and the device image from the first device call)"""

    def __init__(self, h):
        self.h = h

    def __del__(self):
        try:
            if getattr(self, "h", None):
                lib.gtars_seqpack_free(self.h)
                self.h = None
        except Exception:
            pass

    def __len__(self):
        return int(lib.gtars_seqpack_len(self.h))

    @property
    def image_bytes(self) -> int:
        return int(lib.gtars_seqpack_image_bytes(self.h))

    @classmethod
    def from_handle(cls, handle: _Handle, classes: Optional[Sequence[int]] = None, on_host: bool = False, threads: int = 0) -> "_Pack":
        """packed from a collection's text: ``k_refget_pack`` over its raw device image, or the host threads"""
        cl = None if classes is None else np.ascontiguousarray([int(c) for c in classes], dtype=np.uint8)
        if cl is not None and cl.size != len(handle):
            raise ValueError("one alphabet class per record")
        h = C.c_void_p()
        check(lib.gtars_seqpack_from_seqcol(handle.h, None if cl is None else ptr(cl), 1 if on_host else 0, int(threads), C.byref(h)))
        return cls(h)

    @classmethod
    def from_files(cls, paths: Sequence[str], lengths: Sequence[int], classes: Sequence[int], threads: int = 0) -> "_Pack":
        """the ``.seq`` files of an Encoded store, read by the library and kept as they are"""
        arr, keep = cstr_array([os.fspath(p) for p in paths])
        length = np.ascontiguousarray(lengths, dtype=np.uint64)
        cl = np.ascontiguousarray([int(c) for c in classes], dtype=np.uint8)
        if length.size != len(keep) or cl.size != len(keep):
            raise ValueError("columns must have the same length")
        h = C.c_void_p()
        check(lib.gtars_seqpack_from_files(C.cast(arr, C.c_void_p), ptr(length), ptr(cl), len(keep), int(threads), C.byref(h)))
        return cls(h)

    @classmethod
    def from_buffers(cls, packed: Sequence[bytes], lengths: Sequence[int], classes: Sequence[int]) -> "_Pack":
        arr = (C.c_char_p * max(len(packed), 1))(*packed)
        size = np.array([len(q) for q in packed], dtype=np.uint64)
        length = np.ascontiguousarray(lengths, dtype=np.uint64)
        cl = np.ascontiguousarray([int(c) for c in classes], dtype=np.uint8)
        if length.size != len(packed) or cl.size != len(packed):
            raise ValueError("columns must have the same length")
        h = C.c_void_p()
        check(lib.gtars_seqpack_from_buffers(C.cast(arr, C.c_void_p), ptr(size), ptr(length), ptr(cl), len(packed), C.byref(h)))
        return cls(h)

    def record(self, i: int, padding: int = 0) -> Tuple[bytes, int, int]:
        """(packed bytes, length, alphabet class) of record i, from the host copy of the image; ``padding``: up to 16 of the
        image's bytes behind the record are returned with it"""
        data, size, length, cl = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_int()
        check(lib.gtars_seqpack_record(self.h, int(i), C.byref(data), C.byref(size), C.byref(length), C.byref(cl)))
        take = size.value + min(max(int(padding), 0), 16)
        return (C.string_at(data, take) if take else b""), int(length.value), int(cl.value)

    def write_files(self, paths: Sequence[Optional[str]], threads: int = 0) -> None:
        arr, _keep = cstr_array([None if p is None else os.fspath(p) for p in paths])
        check(lib.gtars_seqpack_write_files(self.h, C.cast(arr, C.c_void_p), int(threads)))

    def substrings(self, seq, start, end, on_host: bool, threads: int = 0):
        seq = np.ascontiguousarray(seq, dtype=np.uint32)
        start, end = np.ascontiguousarray(start, dtype=np.uint64), np.ascontiguousarray(end, dtype=np.uint64)
        n = seq.size
        if start.size != n or end.size != n:
            raise ValueError("columns must have the same length")
        status = np.zeros(n, dtype=np.uint8)
        po, pb = C.c_void_p(), C.c_void_p()
        check(lib.gtars_seqpack_substrings(self.h, ptr(seq), ptr(start), ptr(end), n, 1 if on_host else 0, int(threads), ptr(status),
                                           C.byref(po), C.byref(pb)))
        off, blob = _take_csr(po, pb, n)
        return status, off, blob

    def decode_records(self, on_host: bool = False, threads: int = 0):
        """(offsets, bytes): every record's text, decoded from the image"""
        po, pb = C.c_void_p(), C.c_void_p()
        check(lib.gtars_seqpack_decode_records(self.h, 1 if on_host else 0, int(threads), C.byref(po), C.byref(pb)))
        return _take_csr(po, pb, len(self))


def _class_of(alphabet: Union[AlphabetType, int]) -> int:
    return int(alphabet.value if isinstance(alphabet, AlphabetType) else alphabet)


def bits_per_symbol(alphabet: Union[AlphabetType, int]) -> int:
    """2 / 3 / 4 / 5 / 8 bits for Dna2bit / Dna3bit / DnaIupac / Protein / Ascii, 8 for Unknown"""
    return int(lib.gtars_refget_bits(_class_of(alphabet)))


def encode_sequence(data: Union[str, bytes], alphabet: Union[AlphabetType, int]) -> bytes:
    """the bytes bit-packed MSB first by the class's table (both letter cases alike): ceil(len * bits / 8) bytes; host code"""
    seq = _data(data, "encode_sequence")
    out = C.create_string_buffer(max((len(seq) * bits_per_symbol(alphabet) + 7) // 8, 1))
    size = C.c_uint64()
    check(lib.gtars_refget_encode(seq, len(seq), _class_of(alphabet), out, len(out.raw), C.byref(size)))
    return out.raw[:size.value]


def decode_substring(packed: bytes, start: int, end: int, alphabet: Union[AlphabetType, int], byte_offset: int = 0) -> bytes:
    """symbols [start, end) of an encoding of which ``packed`` holds the bytes from ``byte_offset`` on; bits outside those
    bytes read as zero, ``end <= start`` is empty; host code"""
    start, end = int(start), int(end)
    if end <= start:
        return b""
    packed = bytes(packed)
    out = C.create_string_buffer(end - start)
    check(lib.gtars_refget_decode(packed, len(packed), int(byte_offset), start, end, _class_of(alphabet), out))
    return out.raw


def byte_range_for_bases(start: int, end: int, bits: int) -> Tuple[int, int]:
    """the bytes [b0, b1) of an encoding that hold symbols [start, end)"""
    b0, b1 = C.c_uint64(), C.c_uint64()
    lib.gtars_refget_byte_range(int(start), int(end), int(bits), C.byref(b0), C.byref(b1))
    return int(b0.value), int(b1.value)


RGSI_HEADER = "#name\tlength\talphabet\tsha512t24u\tmd5\tdescription\n"
RGCI_HEADER = ("#digest\tn_sequences\tnames_digest\tsequences_digest\tlengths_digest\tname_length_pairs_digest\t"
               "sorted_name_length_pairs_digest\tsorted_sequences_digest\n")
DEFAULT_SEQDATA_PATH_TEMPLATE = "sequences/%s2/%s.seq"


def _rgsi_row(m: SequenceMetadata) -> str:
    return f"{m.name}\t{m.length}\t{m.alphabet}\t{m.sha512t24u}\t{m.md5}\t{m.description or ''}\n"


def _parse_rgsi_line(line: str) -> Optional[SequenceMetadata]:
    """parse_rgsi_line (types.rs:996-1031): 5 or 6 tab-separated columns, anything else is no row"""
    if not line.strip():
        return None
    parts = line.split("\t")
    if len(parts) not in (5, 6) or not re.fullmatch(r"\+?[0-9]+", parts[1]):
        return None
    return SequenceMetadata(parts[0], int(parts[1]), parts[3], parts[4], _alphabet_of(parts[2]), (parts[5] or None) if len(parts) == 6 else None)


def _lines(path) -> List[str]:
    with open(path, "rt", encoding="utf-8", newline="") as f:
        return [ln[:-1] if ln.endswith("\r") else ln for ln in f.read().split("\n")]


def _collection_rgsi_text(meta: "SequenceCollectionMetadata", records: Optional[Sequence["SequenceRecord"]]) -> str:
    """write_rgsi_impl (collection.rs:23-67)"""
    out = [f"##seqcol_digest={meta.digest}\n", f"##names_digest={meta.names_digest}\n", f"##sequences_digest={meta.sequences_digest}\n",
           f"##lengths_digest={meta.lengths_digest}\n"]
    for key in ("name_length_pairs_digest", "sorted_name_length_pairs_digest", "sorted_sequences_digest"):
        if getattr(meta, key) is not None:
            out.append(f"##{key}={getattr(meta, key)}\n")
    out.append(RGSI_HEADER)
    out += [_rgsi_row(r.metadata) for r in records or ()]
    return "".join(out)


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

    def write_collection_rgsi(self, file_path) -> None:
        """the collection's ``.rgsi`` file: its digests as ``##key=value`` lines (the ancillary ones when present), the column
        line, one row per record in order"""
        with open(os.fspath(file_path), "wt", encoding="utf-8", newline="") as f:
            f.write(_collection_rgsi_text(self.metadata(), self.sequences))

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


def read_rgsi_file(file_path) -> SequenceCollection:
    """a collection of stub records from an ``.rgsi`` file (read_rgsi_file, collection.rs:282-368): ``##key=value`` lines give
    the digests, other ``#`` lines are skipped, rows have 5 or 6 columns; level-1 digests the file lacks are computed from
    the rows, ancillary digests it lacks stay None"""
    path = os.fspath(file_path)
    head: Dict[str, str] = {}
    recs = []
    for line in _lines(path):
        if line.startswith("##"):
            key, eq, value = line[2:].partition("=")
            if eq:
                head[key] = value
        elif not line.startswith("#"):
            m = _parse_rgsi_line(line)
            if m is not None:
                recs.append(SequenceRecord(m))
    if not (head.get("sequences_digest") and head.get("names_digest") and head.get("lengths_digest")):
        col = SequenceCollection.from_records(recs)
        col.file_path = path
        return col
    lvl1 = SeqColDigestLvl1(head["sequences_digest"], head["names_digest"], head["lengths_digest"])
    digest = head.get("seqcol_digest") or sha512t24u_digest(
        json.dumps({"names": lvl1.names_digest, "sequences": lvl1.sequences_digest}, separators=(",", ":"), sort_keys=True).encode("utf-8"))
    return SequenceCollection(recs, digest, lvl1, path, (head.get("name_length_pairs_digest"), head.get("sorted_name_length_pairs_digest"),
                                                         head.get("sorted_sequences_digest")))


def _write_record(f, r: SequenceRecord, width: int) -> None:
    m = r.metadata
    data = r.decode().encode("utf-8") if r.encoded else r.sequence
    f.write((f">{m.name} {m.description}\n" if m.description is not None else f">{m.name}\n").encode("utf-8"))
    for at in range(0, len(data), width):
        f.write(data[at:at + width] + b"\n")


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


def _sanitize_relative_path(path: str) -> None:
    """sanitize_relative_path (readonly.rs:1891-1902)"""
    if path.startswith("/") or path.startswith("\\"):
        raise ValueError(f"Absolute paths not allowed: {path}")
    if ".." in path:
        raise ValueError(f"Directory traversal not allowed: {path}")
    if "\0" in path:
        raise ValueError("Null bytes not allowed in path")


def _expand_template(template: str, digest: str) -> str:
    return template.replace("%s2", digest[:2]).replace("%s4", digest[:4]).replace("%s", digest)


def _rfc3339_now() -> str:
    """UTC now with the fraction digits chrono's to_rfc3339 prints (none, 3, 6 or 9)"""
    ns = time.time_ns()
    frac = ns % 1_000_000_000
    text = time.strftime("%Y-%m-%dT%H:%M:%S", time.gmtime(ns // 1_000_000_000))
    if frac:
        text += "." + (f"{frac // 1_000_000:03d}" if frac % 1_000_000 == 0 else f"{frac // 1000:06d}" if frac % 1000 == 0 else f"{frac:09d}")
    return text + "+00:00"


class RefgetStore:
    """sequences by digest, collections by digest, names per collection: ``RefgetStore.in_memory()``, or disk-backed by a store
    directory (``on_disk``, ``open_local``), in storage mode ``Raw`` or ``Encoded``"""

    def __init__(self):
        self._seqs: Dict[str, SequenceRecord] = {}
        self._md5: Dict[str, str] = {}
        self._cols: Dict[str, SequenceCollectionMetadata] = {}
        self._names: Dict[str, Dict[str, str]] = {}   # collection -> name -> sha512t24u (a repeated name: its last record)
        self._records: Dict[str, List[SequenceRecord]] = {}  # collection -> its records in order
        self._handles: Dict[str, _Handle] = {}
        self._packs: Dict[str, _Pack] = {}               # collection -> its packed image (mode Encoded)
        self._mode = StorageMode.Raw
        self._path: Optional[str] = None                 # the store directory of a disk-backed store
        self._template: Optional[str] = None
        self._persist = False

    @classmethod
    def in_memory(cls) -> "RefgetStore":
        """a memory-only store in mode ``Raw``: records hold upper-case text.  (The reference's in-memory store starts in mode
        ``Encoded``; ``enable_encoding()`` switches this one.)"""
        return cls()

    @classmethod
    def on_disk(cls, cache_path) -> "RefgetStore":
        """the store at ``cache_path`` when it has an ``rgstore.json``; otherwise a new persisting store there in mode
        ``Encoded`` (``sequences/``, ``collections/`` and ``fhr/`` are created; the index files come with the first write)"""
        root = os.fspath(cache_path)
        if os.path.exists(os.path.join(root, "rgstore.json")):
            return cls.open_local(root)
        store = cls()
        store._mode, store._path, store._template, store._persist = StorageMode.Encoded, root, DEFAULT_SEQDATA_PATH_TEMPLATE, True
        for sub in ("sequences", "collections", "fhr"):
            os.makedirs(os.path.join(root, sub), exist_ok=True)
        return store

    @classmethod
    def open_local(cls, path) -> "RefgetStore":
        """a store directory opened for reading and writing (open_local, persistence.rs:370-431): sequences and collections
        come as stubs from ``sequences.rgsi`` and ``collections.rgci``; without an ``.rgci`` the ``collections/*.rgsi`` files
        are read instead.  A path of the manifest that is absolute or holds ``..`` or a NUL is refused (ValueError)."""
        root = os.fspath(path)
        manifest = os.path.join(root, "rgstore.json")
        try:
            with open(manifest, "rt", encoding="utf-8") as f:
                meta = json.load(f)
        except OSError as e:
            raise IOError(f"Failed to read rgstore.json from {manifest}") from e
        except ValueError as e:
            raise ValueError("Failed to parse store metadata") from e
        for key in ("seqdata_path_template", "sequence_index", "collection_index", "collections_path_template"):
            if meta.get(key) is not None:
                _sanitize_relative_path(meta[key])
        if meta.get("mode") not in StorageMode._NAMES:
            raise ValueError("Failed to parse store metadata")
        store = cls()
        store._mode = StorageMode(StorageMode._NAMES.index(meta["mode"]))
        store._path, store._template, store._persist = root, meta["seqdata_path_template"], True
        index = os.path.join(root, meta["sequence_index"])
        if os.path.exists(index):
            for line in _lines(index):
                m = None if line.startswith("#") else _parse_rgsi_line(line)
                if m is not None:
                    store._seqs[m.sha512t24u] = SequenceRecord(m)
                    store._md5[m.md5] = m.sha512t24u
        if meta.get("collection_index") is not None and os.path.exists(os.path.join(root, meta["collection_index"])):
            for line in _lines(os.path.join(root, meta["collection_index"])):
                parts = line.split("\t")
                # parse_rgci_line (types.rs:1042-1067)
                if line.startswith("#") or len(parts) < 5 or not re.fullmatch(r"\+?[0-9]+", parts[1]):
                    continue
                anc = [parts[k] if len(parts) > k and parts[k] else None for k in (5, 6, 7)]
                store._cols[parts[0]] = SequenceCollectionMetadata(parts[0], int(parts[1]), parts[2], parts[3], parts[4], *anc)
        if not store._cols:
            for file in sorted(_glob.glob(os.path.join(_glob.escape(os.path.join(root, "collections")), "*.rgsi"))):
                store._adopt(read_rgsi_file(file))
        return store

    # -- adding ----------------------------------------------------------------------------------------------------------
    def add_sequence(self, sequence: SequenceRecord, force: bool = False) -> None:
        key = sequence.metadata.sha512t24u
        if key in self._seqs and not force and (self._seqs[key].is_loaded or not sequence.is_loaded):
            return
        self._seqs[key] = sequence
        self._md5[sequence.metadata.md5] = key

    def _adopt(self, collection: SequenceCollection, force: bool = False) -> SequenceCollectionMetadata:
        """the collection's metadata, names and records into the maps"""
        meta = collection.metadata()
        if meta.name_length_pairs_digest is None and all(r.metadata.sha512t24u for r in collection):
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
        self._packs.pop(collection.digest, None)
        return meta

    def add_sequence_collection(self, collection: SequenceCollection, force: bool = False, on_host: bool = False,
                                threads: int = 0) -> Tuple[SequenceCollectionMetadata, bool]:
        """In mode ``Encoded`` the records are packed first (``k_refget_pack`` over the collection's raw device image, or the
        host threads with ``on_host``) and the store keeps the packed bytes.  A persisting store writes the ``.seq`` files, the
        collection's ``.rgsi`` and the index files, and keeps stubs."""
        if collection.digest in self._cols and not force:
            return self._cols[collection.digest], False
        was_new = collection.digest not in self._cols
        handle, pack, stored = collection._handle, None, collection
        loaded = len(collection) > 0 and all(r.is_loaded and not r.encoded for r in collection)
        if loaded and (self._persist or self._mode == StorageMode.Encoded):
            if handle is None:
                handle = _image_handle(collection.sequences)
            if self._mode == StorageMode.Encoded:
                pack = _Pack.from_handle(handle, [r.metadata.alphabet.value for r in collection], on_host, threads)
            if self._persist:
                paths = [self._seq_file(r.metadata.sha512t24u, make_dirs=True) for r in collection]
                (pack or handle).write_files(paths, threads)
                recs = [SequenceRecord(r.metadata) for r in collection]
            else:
                recs = [SequenceRecord(r.metadata, pack.record(i)[0], True) for i, r in enumerate(collection)]
            stored = SequenceCollection(recs, collection.digest, collection.lvl1, collection.file_path, collection._ancillary)
        meta = self._adopt(stored, force)
        if stored is collection:
            if handle is not None and self._mode == StorageMode.Raw:
                self._handles[collection.digest] = handle
        elif pack is not None:
            self._packs[collection.digest] = pack
        else:
            self._handles[collection.digest] = handle
        if self._persist:
            os.makedirs(os.path.join(self._path, "collections"), exist_ok=True)
            with open(os.path.join(self._path, "collections", f"{meta.digest}.rgsi"), "wt", encoding="utf-8", newline="") as f:
                f.write(_collection_rgsi_text(meta, self._records[meta.digest]))
            self._write_index_files()
        return meta, was_new

    def add_sequence_collection_from_fasta(self, file_path, force: bool = False, on_host: bool = False, threads: int = 0,
                                           **_ignored) -> Tuple[SequenceCollectionMetadata, bool]:
        return self.add_sequence_collection(load_fasta(file_path, on_host=on_host, threads=threads), force, on_host, threads)

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
        self.load_collection(collection_digest)
        m = self._cols[collection_digest]
        recs = []
        for name, sha in self._names[collection_digest].items():
            r = self._seqs[sha]
            if r.metadata.name != name:
                md = r.metadata
                r = SequenceRecord(SequenceMetadata(name, md.length, md.sha512t24u, md.md5, md.alphabet, md.description, md.fai), r.sequence,
                                   r.encoded)
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
        self.load_collection(digest)
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
        unknown digest and for a range that is inverted or passes the sequence's end.  A stub of a disk-backed store is served
        from its ``.seq`` file: only the bytes that hold the range are read (``byte_range_for_bases`` in mode ``Encoded``)."""
        r = self._seqs.get(self._key(seq_digest))
        if r is None:
            raise KeyError(f"Sequence not found: {seq_digest}")
        start, end = int(start), int(end)
        if start == end:
            return ""
        m = r.metadata
        path = None
        if r.sequence is None:
            path = self._seq_file(m.sha512t24u)
            if path is None or not os.path.exists(path):
                raise KeyError("Sequence data not loaded (stub only)")
        if start < 0 or start >= m.length or end > m.length or start >= end:
            raise KeyError(f"Invalid substring range: start={start}, end={end}, sequence length={m.length}")
        encoded = r.encoded if path is None else self._mode == StorageMode.Encoded
        b0, b1 = byte_range_for_bases(start, end, bits_per_symbol(m.alphabet)) if encoded else (start, end)
        if path is None:
            window = r.sequence[b0:b1]
        else:
            with open(path, "rb") as f:
                f.seek(b0)
                window = f.read(b1 - b0)
            if len(window) != b1 - b0:
                raise IOError(f"{path}: too short for bytes {b0} to {b1}")
        return (decode_substring(window, start, end, m.alphabet, b0) if encoded else window).decode("utf-8", "replace")

    def get_substrings(self, seq_digest: str, ranges: Sequence[Tuple[int, int]], on_host: bool = False, threads: int = 0) -> List[str]:
        """many ranges of ONE sequence (get_substrings, readonly.rs:1396-1433): every range is checked first (KeyError with the
        message of ``get_substring``; an empty range is fine wherever it lies), then all of them are read in one call from
        the device image of a loaded collection that holds the sequence, or one by one when no collection does"""
        r = self._seqs.get(self._key(seq_digest))
        if r is None:
            raise KeyError(f"Sequence not found: {seq_digest}")
        n = r.metadata.length
        ranges = [(int(a), int(b)) for a, b in ranges]
        for a, b in ranges:
            if a < 0 or (a != b and a >= n) or b > n or a > b:
                raise KeyError(f"Invalid substring range: start={a}, end={b}, sequence length={n}")
        sha = r.metadata.sha512t24u
        for col, recs in self._records.items():
            row = next((i for i, q in enumerate(recs) if q.metadata.sha512t24u == sha), None)
            if row is None:
                continue
            try:
                source = self._source(col)
            except KeyError:
                continue
            status, off, blob = source.substrings([row] * len(ranges), [a for a, _ in ranges], [b for _, b in ranges], on_host, threads)
            if status.any():
                raise KeyError(f"Invalid substring range: sequence length={n}")
            return [blob[int(off[i]):int(off[i + 1])].decode("utf-8", "replace") for i in range(len(ranges))]
        return [self.get_substring(seq_digest, a, b) for a, b in ranges]

    # -- persistence and storage mode ------------------------------------------------------------------------------------
    @property
    def storage_mode(self) -> StorageMode:
        return self._mode

    @property
    def is_persisting(self) -> bool:
        return self._persist

    @property
    def cache_path(self) -> Optional[str]:
        """the store directory; None for a memory-only store"""
        return self._path

    def _seq_file(self, sha: str, make_dirs: bool = False) -> Optional[str]:
        """the ``.seq`` file of a sequence: the template with %s2, %s4 and %s expanded in that order (expand_template,
        readonly.rs:1860-1871)"""
        if self._path is None or self._template is None:
            return None
        path = os.path.join(self._path, _expand_template(self._template, sha))
        if make_dirs:
            os.makedirs(os.path.dirname(path), exist_ok=True)
        return path

    def _resident(self, r: SequenceRecord) -> SequenceRecord:
        """the record that holds the data of ``r``'s sequence, if any does"""
        if r.is_loaded:
            return r
        q = self._seqs.get(r.metadata.sha512t24u)
        return q if q is not None and q.is_loaded else r

    def load_collection(self, digest: str) -> None:
        """the records of a collection that came as a stub from ``collections.rgci``, from its ``collections/<digest>.rgsi``"""
        if digest in self._names:
            return
        if digest not in self._cols:
            raise KeyError(f"Collection not found: {digest}")
        if self._path is None:
            raise KeyError(f"Collection not loaded: {digest}")
        col = read_rgsi_file(os.path.join(self._path, "collections", f"{digest}.rgsi"))
        meta = self._cols[digest]
        self._names[digest] = {}
        recs = []
        for r in col:
            m = r.metadata
            have = self._seqs.get(m.sha512t24u)
            if have is None:
                self._seqs[m.sha512t24u], self._md5[m.md5] = r, m.sha512t24u
            elif have.metadata.name == m.name:
                r = have
            self._names[digest][m.name] = m.sha512t24u
            recs.append(r)
        self._records[digest] = recs
        self._cols[digest] = meta

    def load_all_collections(self) -> None:
        for digest in sorted(self._cols):
            self.load_collection(digest)

    def load_sequence(self, digest: str) -> None:
        """a stub's data from its ``.seq`` file: packed bytes in mode ``Encoded``, text in mode ``Raw``"""
        r = self._seqs.get(self._key(digest))
        if r is None:
            raise KeyError(f"Sequence not found: {digest}")
        if r.is_loaded:
            return
        path = self._seq_file(r.metadata.sha512t24u)
        if path is None:
            raise KeyError("Sequence data not loaded (stub only)")
        encoded = self._mode == StorageMode.Encoded
        want = (r.metadata.length * bits_per_symbol(r.metadata.alphabet) + 7) // 8 if encoded else r.metadata.length
        try:
            with open(path, "rb") as f:
                data = f.read()
        except OSError as e:
            raise IOError(f"Failed to open seq file {path}") from e
        if len(data) != want:
            raise ValueError(f"{path}: {len(data)} bytes, the sequence needs {want}")
        r.sequence, r.encoded = data, encoded

    def load_all_sequences(self) -> None:
        for sha in sorted(self._seqs):
            self.load_sequence(sha)

    def _loaded_records(self) -> List[SequenceRecord]:
        """every loaded record object of the store, once"""
        seen, out = set(), []
        for r in list(self._seqs.values()) + [q for recs in self._records.values() for q in recs]:
            if r.is_loaded and id(r) not in seen:
                seen.add(id(r))
                out.append(r)
        return out

    def set_encoding_mode(self, new_mode: StorageMode, on_host: bool = False, threads: int = 0) -> None:
        """changes the mode and converts every resident sequence: ``Raw`` to ``Encoded`` packs the text with ``k_refget_pack``
        (one launch per conversion), ``Encoded`` to ``Raw`` decodes whole records from the packed image; ``on_host`` runs
        either on the host threads.  Stubs and files on disk are not touched."""
        if new_mode == self._mode:
            return
        recs = [r for r in self._loaded_records() if r.encoded != (new_mode == StorageMode.Encoded)]
        if recs:
            classes = [r.metadata.alphabet.value for r in recs]
            if new_mode == StorageMode.Encoded:
                pack = _Pack.from_handle(_Handle.from_buffers([r.sequence for r in recs]), classes, on_host, threads)
                for i, r in enumerate(recs):
                    r.sequence, r.encoded = pack.record(i)[0], True
            else:
                pack = _Pack.from_buffers([r.sequence for r in recs], [r.metadata.length for r in recs], classes)
                off, blob = pack.decode_records(on_host, threads)
                for i, r in enumerate(recs):
                    r.sequence, r.encoded = blob[int(off[i]):int(off[i + 1])], False
        self._handles.clear()
        self._packs.clear()
        self._mode = new_mode

    def enable_encoding(self, on_host: bool = False, threads: int = 0) -> None:
        self.set_encoding_mode(StorageMode.Encoded, on_host, threads)

    def disable_encoding(self, on_host: bool = False, threads: int = 0) -> None:
        self.set_encoding_mode(StorageMode.Raw, on_host, threads)

    def _write_sequence_files(self, root: str, template: str, threads: int = 0) -> List[SequenceRecord]:
        """the data of every loaded sequence into its ``.seq`` file under ``root``, written by the library -> those records"""
        recs, seen = [], set()
        for r in self._loaded_records():
            if r.metadata.sha512t24u not in seen and r.encoded == (self._mode == StorageMode.Encoded):
                seen.add(r.metadata.sha512t24u)
                recs.append(r)
        if recs:
            paths = [os.path.join(root, _expand_template(template, r.metadata.sha512t24u)) for r in recs]
            for path in paths:
                os.makedirs(os.path.dirname(path), exist_ok=True)
            if self._mode == StorageMode.Encoded:
                _Pack.from_buffers([r.sequence for r in recs], [r.metadata.length for r in recs],
                                   [r.metadata.alphabet.value for r in recs]).write_files(paths, threads)
            else:
                _Handle.from_buffers([r.sequence for r in recs]).write_files(paths, threads)
        return recs

    def _write_collection_files(self, root: str) -> None:
        os.makedirs(os.path.join(root, "collections"), exist_ok=True)
        for digest in sorted(self._cols):
            if digest not in self._records and self._path is not None:
                self.load_collection(digest)
            with open(os.path.join(root, "collections", f"{digest}.rgsi"), "wt", encoding="utf-8", newline="") as f:
                f.write(_collection_rgsi_text(self._cols[digest], self._records.get(digest)))

    def _write_indexes(self, root: str, template: str, with_digests: bool) -> None:
        """``sequences.rgsi`` (rows by sha512t24u), ``collections.rgci`` (rows by digest) and ``rgstore.json``
        (persistence.rs:114-285): pretty-printed with two spaces, absent options left out, no trailing newline"""
        seq_text = RGSI_HEADER + "".join(_rgsi_row(self._seqs[k].metadata) for k in sorted(self._seqs))
        col_text = RGCI_HEADER + "".join(
            "\t".join([m.digest, str(m.n_sequences), m.names_digest, m.sequences_digest, m.lengths_digest, m.name_length_pairs_digest or "",
                       m.sorted_name_length_pairs_digest or "", m.sorted_sequences_digest or ""]) + "\n"
            for m in (self._cols[k] for k in sorted(self._cols)))
        for name, text in (("sequences.rgsi", seq_text), ("collections.rgci", col_text)):
            with open(os.path.join(root, name), "wb") as f:
                f.write(text.encode("utf-8"))
        meta = {"version": 1, "seqdata_path_template": template, "collections_path_template": "collections/%s.rgsi",
                "sequence_index": "sequences.rgsi", "collection_index": "collections.rgci", "mode": self._mode.name,
                "created_at": _rfc3339_now(), "ancillary_digests": True, "attribute_index": False, "modified": _rfc3339_now()}
        if with_digests:
            meta["collections_digest"] = hashlib.sha256(col_text.encode("utf-8")).hexdigest()
            meta["sequences_digest"] = hashlib.sha256(seq_text.encode("utf-8")).hexdigest()
        with open(os.path.join(root, "rgstore.json"), "wb") as f:
            f.write(json.dumps(meta, indent=2, ensure_ascii=False).encode("utf-8"))

    def _write_index_files(self) -> None:
        self._write_indexes(self._path, self._template or DEFAULT_SEQDATA_PATH_TEMPLATE, True)

    def write(self) -> None:
        """the index files of a disk-backed store again; IOError for a store that is not"""
        if not self._persist:
            raise IOError("write() only works with disk-backed stores - use write_store_to_dir() instead")
        self._write_index_files()

    def write_store_to_dir(self, root_path, seqdata_path_template: Optional[str] = None, threads: int = 0) -> None:
        """the whole store into a directory (write_store_to_dir, readonly.rs:2135-2195): the ``.seq`` file of every loaded
        sequence in the store's mode (stubs have none to write), every collection's ``.rgsi``, the two index files and an
        ``rgstore.json`` without the index digests"""
        root = os.fspath(root_path)
        template = seqdata_path_template or self._template or DEFAULT_SEQDATA_PATH_TEMPLATE
        _sanitize_relative_path(template)
        for sub in ("sequences", "collections"):
            os.makedirs(os.path.join(root, sub), exist_ok=True)
        self._write_sequence_files(root, template, threads)
        self._write_collection_files(root)
        self._write_indexes(root, template, False)

    def enable_persistence(self, path, threads: int = 0) -> None:
        """makes the store disk-backed at ``path``: what is resident is written there and the records become stubs"""
        self._path, self._persist = os.fspath(path), True
        self._template = self._template or DEFAULT_SEQDATA_PATH_TEMPLATE
        for sub in ("sequences", "collections"):
            os.makedirs(os.path.join(self._path, sub), exist_ok=True)
        self._write_sequence_files(self._path, self._template, threads)
        for r in self._loaded_records():
            r.sequence, r.encoded = None, False
        self._handles.clear()
        self._packs.clear()
        self._write_collection_files(self._path)
        self._write_index_files()

    def disable_persistence(self) -> None:
        self._persist = False

    # -- regions ---------------------------------------------------------------------------------------------------------
    def _source(self, collection_digest: str) -> Union[_Handle, _Pack]:
        """the collection's device image, built once: in mode ``Raw`` K21's raw image (from the records' text, or the text
        ``.seq`` files of stubs); in mode ``Encoded`` the packed image (from the ``.seq`` files as they are when the store has
        them all, else from the records' packed bytes)"""
        if collection_digest not in self._records and collection_digest in self._cols and self._path is not None:
            self.load_collection(collection_digest)
        if collection_digest not in self._records:
            raise KeyError("Collection not loaded. Call load_collection() or load_all_collections() first.")
        cache = self._packs if self._mode == StorageMode.Encoded else self._handles
        if collection_digest in cache:
            return cache[collection_digest]
        recs = [self._resident(r) for r in self._records[collection_digest]]
        encoded = self._mode == StorageMode.Encoded
        paths = [self._seq_file(r.metadata.sha512t24u) for r in recs]
        lengths, classes = [r.metadata.length for r in recs], [r.metadata.alphabet.value for r in recs]
        if all(r.is_loaded and r.encoded == encoded for r in recs) and not encoded:
            source = _image_handle(recs)
        elif recs and all(p is not None and os.path.exists(p) for p in paths):
            source = _Pack.from_files(paths, lengths, classes) if encoded else _Handle.from_seq_files(paths, lengths)
        elif all(r.is_loaded and r.encoded == encoded for r in recs):
            source = _Pack.from_buffers([r.sequence for r in recs], lengths, classes)
        else:
            raise KeyError("Sequence data not loaded (stub only)")
        cache[collection_digest] = source
        return source

    _image = _source

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
        where = "memory-only" if self._path is None else f"mode={self._mode}, path={self._path!r}"
        return f"RefgetStore(n_sequences={len(self._seqs)}, n_collections={len(self._cols)}, {where})"

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
    h = store._source(collection_digest)
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


def substrings_device(collection: Union[SequenceCollection, _Handle, _Pack], d_seq: int, d_start: int, d_end: int, n: int, d_status: int,
                      d_offsets: int, d_bytes: int, cap: int, stream: int = 0) -> int:
    """substrings for columns that are on the device already (u32 record numbers, u64 starts and ends; outputs u8 statuses,
    n + 1 u64 offsets, ``cap`` bytes) -> the bytes needed; CapacityError when that is more than ``cap``.  A packed image
    (``packed_image``) is read through its decode tables, a collection through its raw image."""
    total = C.c_uint64()
    packed = isinstance(collection, _Pack)
    entry = lib.gtars_refget_packed_substrings_device if packed else lib.gtars_refget_substrings_device
    check(entry((collection if packed else _handle_of(collection)).h, C.c_void_p(d_seq), C.c_void_p(d_start), C.c_void_p(d_end), int(n),
                C.c_void_p(d_status), C.c_void_p(d_offsets), C.c_void_p(d_bytes), int(cap), C.byref(total), C.c_void_p(stream)))
    return int(total.value)


def packed_image(collection: Union[SequenceCollection, _Handle], classes: Optional[Sequence[int]] = None, on_host: bool = False,
                 threads: int = 0) -> _Pack:
    """the bit-packed image of a loaded collection (``load_fasta``), packed on the device by ``k_refget_pack`` (or on the host
    threads): ``record(i)``, ``substrings``, ``decode_records``, ``write_files``; additive"""
    if classes is None and isinstance(collection, SequenceCollection):
        classes = [r.metadata.alphabet.value for r in collection]
    return _Pack.from_handle(_handle_of(collection), classes, on_host, threads)


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
