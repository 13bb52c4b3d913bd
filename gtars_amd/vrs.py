"""GA4GH VRS allele identifiers: ``gtars.vrs`` (gtars-python/src/vrs/funcs.rs, gtars-vrs/src/{normalize,digest,vcf_core,vcf}.rs).

The reference's four functions keep their signatures and results: ``vrs_digest``, ``vrs_id``, ``normalize_allele`` and
``location_digest`` are host code and need no device.  The batch calls are additive: ``normalize_alleles`` and ``vrs_ids``
take alleles as columns, ``compute_vrs_ids`` takes a VCF file (plain, gzip or BGZF by its magic bytes); they run on the
device that holds the assembly's packed image (csrc/vrs.hip) -- one lane per allele normalizes
against the chromosome and computes the two SHA-512 digests.  ``on_host=True`` runs the library's own host path on its
host threads instead: the same results, no device.  Without a device the default calls raise NoDeviceError; there is no
silent fallback.

Only literal sequence states are computed.  ``ReferenceLengthExpression`` states, the refget store and sequence
collections are not part of this module.  The HGVS parser and the HGVS-to-VRS bridge are ``gtars_amd.hgvs``, which is
reachable from here as ``vrs.hgvs`` (``gtars.vrs.hgvs``), as in the reference; transcripts are ``gtars_amd.reftx``.
``transcript_vrs_ids`` is the batch call for alleles that lie on transcripts: they are normalized over the mature mRNAs, which
are derived from the assembly for the call (csrc/hgvs_tx.hip, K23).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from ._lib import check, lib, ptr
from .seqstats import _genome_handle

STATUS_NAMES = ("ok", "start_out_of_bounds", "ref_past_end", "ref_mismatch", "unknown_chromosome", "bad_allele")
VA_PREFIX = "ga4gh:VA."


def _u64(x) -> int:
    if not 0 <= int(x) < 1 << 64:
        raise OverflowError("position must fit in u64")
    return int(x)


def _bytes(x) -> bytes:
    return x if isinstance(x, (bytes, bytearray)) else str(x).encode("utf-8")


def sha512t24u(data) -> str:
    """the first 24 bytes of SHA-512 as base64url without padding (32 characters) of a str (UTF-8) or bytes"""
    b = bytes(_bytes(data))
    out = C.create_string_buffer(33)
    check(lib.gtars_sha512t24u(b, len(b), out))
    return out.value.decode("ascii")


def location_digest(seq_digest: str, start: int, end: int) -> str:
    """digest of the SequenceLocation {refgetAccession: seq_digest, start, end}; ``seq_digest`` as given, "SQ." included"""
    out = C.create_string_buffer(33)
    check(lib.gtars_vrs_location_digest(str(seq_digest).encode("utf-8"), _u64(start), _u64(end), out))
    return out.value.decode("ascii")


def vrs_digest(seq_digest: str, start: int, end: int, alt: str) -> str:
    """digest of the Allele with a literal sequence state, without the "ga4gh:VA." prefix"""
    b = str(alt).encode("utf-8")
    out = C.create_string_buffer(33)
    check(lib.gtars_vrs_allele_digest(str(seq_digest).encode("utf-8"), _u64(start), _u64(end), b, len(b), out))
    return out.value.decode("ascii")


def vrs_id(seq_digest: str, start: int, end: int, alt: str) -> str:
    """"ga4gh:VA." + vrs_digest"""
    return VA_PREFIX + vrs_digest(seq_digest, start, end, alt)


def normalize_allele(sequence: str, start: int, ref_allele: str, alt_allele: str) -> dict:
    """fully-justified normalization of one allele over ``sequence``: {"start", "end", "allele"}; ValueError with
    NormalizeError's text when it fails"""
    seq, ref, alt = _bytes(sequence), _bytes(ref_allele), _bytes(alt_allele)
    ns, ne, p, n = C.c_uint64(), C.c_uint64(), C.c_void_p(), C.c_uint64()
    check(lib.gtars_vrs_normalize(bytes(seq), len(seq), _u64(start), bytes(ref), len(ref), bytes(alt), len(alt), C.byref(ns), C.byref(ne),
                                  C.byref(p), C.byref(n)))
    try:
        allele = C.string_at(p, n.value)
    finally:
        lib.gtars_free(p)
    return {"start": ns.value, "end": ne.value, "allele": allele.decode("utf-8")}


def refget_digests(genome, threads: int = 0) -> Dict[str, str]:
    """``genome.refget_digests()``: chromosome name -> sha512t24u of its upper-cased bytes"""
    _genome_handle(genome)
    return genome.refget_digests(threads)


def _accession_table(genome, accessions: Optional[Dict[str, str]]):
    """the caller's name -> digest table as 32 bytes per chromosome id (a zero row: none), or None for the assembly's own"""
    if accessions is None:
        return None
    names = genome.chrom_names
    tab = bytearray(32 * len(names))
    for k, name in enumerate(names):
        d = accessions.get(name)
        if d is None:
            continue
        d = str(d)
        d = d[3:] if d.startswith("SQ.") else d
        b = d.encode("ascii")
        if len(b) != 32:
            raise ValueError(f"accession of {name!r} must be 32 digest characters, got {d!r}")
        tab[32 * k:32 * k + 32] = b
    return bytes(tab)


class _Columns:
    """alleles as the library's columns: chromosome ids, u64 starts, one byte pool with offsets and lengths"""

    def __init__(self, genome, chroms: Sequence, starts: Sequence[int], refs: Sequence, alts: Sequence):
        n = len(chroms)
        if not (len(starts) == len(refs) == len(alts) == n):
            raise ValueError("columns must have the same length")
        ids = {name: k for k, name in enumerate(genome.chrom_names)}
        # an unknown name is chromosome id 2^32 - 1: the row gets status 4
        self.chrom = np.array([c if isinstance(c, (int, np.integer)) else ids.get(c, 0xFFFFFFFF) for c in chroms], dtype=np.uint32)
        self.start = np.array([_u64(s) for s in starts], dtype=np.uint64)
        refs, alts = [bytes(_bytes(r)) for r in refs], [bytes(_bytes(a)) for a in alts]
        self.ref_len = np.array([len(r) for r in refs], dtype=np.uint32)
        self.alt_len = np.array([len(a) for a in alts], dtype=np.uint32)
        lens = np.empty(2 * n, dtype=np.uint64)
        lens[0::2], lens[1::2] = self.ref_len, self.alt_len
        off = np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens, dtype=np.uint64)])
        if int(off[-1]) > 0xFFFFFFF0:
            raise ValueError("the alleles of one call must fit 4 GiB")
        self.ref_off, self.alt_off = off[0:-1:2].astype(np.uint32), off[1::2].astype(np.uint32)
        self.pool = np.frombuffer(b"".join(x for pair in zip(refs, alts) for x in pair), dtype=np.uint8)
        self.n = n


def _run(genome, cols: _Columns, accessions, want_ids: bool, want_seqs: bool, on_host: bool, threads: int):
    h = _genome_handle(genome)
    n = cols.n
    status = np.zeros(n, dtype=np.uint8)
    ns, ne = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    digests = np.zeros(32 * n, dtype=np.uint8) if want_ids else None
    po, pb = C.c_void_p(), C.c_void_p()
    tab = _accession_table(genome, accessions)
    check(lib.gtars_vrs_alleles(h, tab, ptr(cols.chrom), ptr(cols.start), ptr(cols.pool), cols.pool.size, ptr(cols.ref_off),
                                ptr(cols.ref_len), ptr(cols.alt_off), ptr(cols.alt_len), n, 1 if on_host else 0, int(threads),
                                ptr(status), ptr(ns), ptr(ne), ptr(digests) if want_ids else None,
                                C.byref(po) if want_seqs else None, C.byref(pb) if want_seqs else None))
    seqs = None
    if want_seqs:
        try:
            off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
            blob = C.string_at(pb, int(off[-1]))
        finally:
            lib.gtars_free(po)
            lib.gtars_free(pb)
        seqs = [blob[int(off[i]):int(off[i + 1])] for i in range(n)]
    ids = None
    if want_ids:
        raw = digests.tobytes()
        ids = [VA_PREFIX + raw[32 * i:32 * i + 32].decode("ascii") if status[i] == 0 else None for i in range(n)]
    return status, ns, ne, seqs, ids


def normalize_alleles(genome, chroms, starts, refs, alts, on_host: bool = False, threads: int = 0) -> dict:
    """normalization of a batch against an assembly: {"starts", "ends", "statuses" (numpy; 0 = ok, see STATUS_NAMES),
    "sequences" (bytes per allele, empty for one that failed)}.  ``chroms``: names of the assembly or its chromosome ids;
    ``refs`` / ``alts``: str or bytes.  Never raises for data."""
    status, ns, ne, seqs, _ = _run(genome, _Columns(genome, chroms, starts, refs, alts), None, False, True, on_host, threads)
    return {"starts": ns, "ends": ne, "statuses": status, "sequences": seqs}


def vrs_ids(genome, chroms, starts, refs, alts, accessions: Optional[Dict[str, str]] = None, on_host: bool = False,
            threads: int = 0) -> dict:
    """{"ids": "ga4gh:VA...." per allele (None for one that failed), "statuses"}.  ``accessions``: chromosome name -> refget
    digest (with or without "SQ."); chromosomes it lacks get status 4.  Default: the assembly's own ``refget_digests()``."""
    status, _, _, _, ids = _run(genome, _Columns(genome, chroms, starts, refs, alts), accessions, True, False, on_host, threads)
    return {"ids": ids, "statuses": status}


def ids_device(genome, d_chrom: int, d_start: int, d_pool: int, pool_bytes: int, d_ref_off: int, d_ref_len: int, d_alt_off: int,
               d_alt_len: int, n: int, d_status: int = 0, d_new_start: int = 0, d_new_end: int = 0, d_digests: int = 0, stream: int = 0,
               accessions: Optional[Dict[str, str]] = None) -> None:
    """the batch call for columns that are on the device already (device pointers: u32 chromosome ids, u64 starts, the byte
    pool, u32 offsets and lengths; outputs u8 statuses, u64 starts / ends, n * 32 digest bytes, any may be 0), queued on
    ``stream``, which is drained before the call returns.  The current device must be the assembly's."""
    check(lib.gtars_vrs_ids_device(_genome_handle(genome), _accession_table(genome, accessions), C.c_void_p(d_chrom), C.c_void_p(d_start),
                                   C.c_void_p(d_pool), int(pool_bytes), C.c_void_p(d_ref_off), C.c_void_p(d_ref_len),
                                   C.c_void_p(d_alt_off), C.c_void_p(d_alt_len), int(n), C.c_void_p(d_status), C.c_void_p(d_new_start),
                                   C.c_void_p(d_new_end), C.c_void_p(d_digests), C.c_void_p(stream)))


def transcript_vrs_ids(genome, store, accessions_or_indices, starts, refs, alts, on_host: bool = False, threads: int = 0) -> dict:
    """VRS identifiers of alleles that lie on transcripts: allele i on the mature mRNA of transcript
    ``accessions_or_indices[i]`` (an accession of the store, or its number there) at 0-based interbase ``starts[i]``, REF and ALT
    in transcript orientation.  The mRNAs are derived from the assembly for the call, normalization is over the mRNA alone
    (csrc/hgvs_tx.hip, K23: the layer ``gtars.vrs.hgvs.hgvs_to_transcript_vrs_ids`` sits on).  {"ids" (None for an allele
    that failed), "statuses" (see STATUS_NAMES; 4: no such transcript, or the assembly cannot give its sequence),
    "accessions" ("SQ...." of the mRNA or None), "starts", "ends"}.  ``store``: a ReadonlyTxStore or a BoundTxStore."""
    from .hgvs import _bound  # (hgvs imports this module)

    b = _bound(genome, store)
    _genome_handle(b.genome)
    names = [a for a in accessions_or_indices if not isinstance(a, (int, np.integer))]
    found = dict(zip(names, b.store.indices_of(names, threads).tolist())) if names else {}
    cols = _Columns(b.genome, [a if isinstance(a, (int, np.integer)) else found[a] for a in accessions_or_indices], starts, refs, alts)
    n = cols.n
    status = np.zeros(n, dtype=np.uint8)
    ns, ne = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    digests, anchors = np.zeros(32 * n, dtype=np.uint8), np.zeros(32 * n, dtype=np.uint8)
    check(lib.gtars_vrs_transcript_ids(b._h, ptr(cols.chrom), ptr(cols.start), ptr(cols.pool), cols.pool.size, ptr(cols.ref_off),
                                       ptr(cols.ref_len), ptr(cols.alt_off), ptr(cols.alt_len), n, 1 if on_host else 0, int(threads),
                                       ptr(status), ptr(ns), ptr(ne), ptr(digests), ptr(anchors)))
    raw, raw_a = digests.tobytes(), anchors.tobytes()
    ids = [VA_PREFIX + raw[32 * i:32 * i + 32].decode("ascii") if status[i] == 0 else None for i in range(n)]
    accs = ["SQ." + raw_a[32 * i:32 * i + 32].decode("ascii") if status[i] == 0 else None for i in range(n)]
    return {"ids": ids, "statuses": status, "accessions": accs, "starts": ns, "ends": ne}


class VrsResults:
    """the alleles of a VCF file in file order, as columns: ``chrom``, ``pos`` (0-based), ``ref_allele``, ``alt_allele``,
    ``vrs_id`` (mirrors VrsResult, vcf_core.rs:89-97); ``len()`` and indexing give rows as dicts"""

    def __init__(self, chrom: List[str], pos: List[int], ref_allele: List[str], alt_allele: List[str], vrs_id: Optional[List[str]]):
        self.chrom, self.pos, self.ref_allele, self.alt_allele, self.vrs_id = chrom, pos, ref_allele, alt_allele, vrs_id

    def __len__(self) -> int:
        return len(self.chrom)

    def __getitem__(self, i: int) -> dict:
        return {"chrom": self.chrom[i], "pos": self.pos[i], "ref_allele": self.ref_allele[i], "alt_allele": self.alt_allele[i],
                "vrs_id": self.vrs_id[i] if self.vrs_id is not None else None}

    def __repr__(self) -> str:
        return f"VrsResults with {len(self)} alleles."


def _take_results(genome, r) -> VrsResults:
    try:
        n = int(lib.gtars_vrs_results_len(r))
        pc, pp_, pool, ro, rl, ao, al, pd = (C.c_void_p() for _ in range(8))
        nb = C.c_uint64()
        check(lib.gtars_vrs_results_columns(r, C.byref(pc), C.byref(pp_), C.byref(pool), C.byref(nb), C.byref(ro), C.byref(rl), C.byref(ao),
                                            C.byref(al), C.byref(pd)))

        def col(p, ctype):
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(n,)).tolist() if n else []

        names = genome.chrom_names
        blob = C.string_at(pool, nb.value) if nb.value else b""
        text = lambda o, k: blob[o:o + k].decode("utf-8", "replace")  # noqa: E731
        refs = [text(o, k) for o, k in zip(col(ro, C.c_uint32), col(rl, C.c_uint32))]
        alts = [text(o, k) for o, k in zip(col(ao, C.c_uint32), col(al, C.c_uint32))]
        ids = None
        if pd.value:
            raw = C.string_at(pd, 32 * n)
            ids = [VA_PREFIX + raw[32 * i:32 * i + 32].decode("ascii") for i in range(n)]
        return VrsResults([names[c] for c in col(pc, C.c_uint32)], col(pp_, C.c_uint64), refs, alts, ids)
    finally:
        lib.gtars_vrs_results_free(r)


def read_vcf_alleles(vcf_path, genome, accessions: Optional[Dict[str, str]] = None, threads: int = 0) -> VrsResults:
    """the alleles ``compute_vrs_ids`` would process, parsed on the host threads; ``vrs_id`` is None"""
    r = C.c_void_p()
    check(lib.gtars_vcf_read_alleles(_genome_handle(genome), os.fspath(vcf_path).encode("utf-8"), _accession_table(genome, accessions),
                                     int(threads), C.byref(r)))
    return _take_results(genome, r)


def compute_vrs_ids(vcf_path, genome, accessions: Optional[Dict[str, str]] = None, on_host: bool = False, threads: int = 0) -> VrsResults:
    """VRS identifiers of every real ALT allele of a VCF file (vcf_core.rs:126-189): rows whose chromosome the assembly (or
    ``accessions``) lacks are skipped; the first allele in file order that fails to normalize raises ValueError
    "Failed to normalize variant at chrom:pos: cause"."""
    r = C.c_void_p()
    check(lib.gtars_vrs_from_vcf(_genome_handle(genome), os.fspath(vcf_path).encode("utf-8"), _accession_table(genome, accessions),
                                 1 if on_host else 0, int(threads), C.byref(r)))
    return _take_results(genome, r)


# gtars.vrs.hgvs: the reference keeps the HGVS module under vrs and registers it in sys.modules (gtars-python/src/vrs/mod.rs);
# this file stays a single module, so the sub-module is registered by hand
import sys as _sys  # noqa: E402

from . import hgvs  # noqa: E402,F401

_sys.modules[__name__ + ".hgvs"] = hgvs
