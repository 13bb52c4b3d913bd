"""K23 restated in plain Python, the way the reference computes it (gtars-vrs/src/hgvs/bridge.rs:226-534): the mature mRNA as a
string from reftx_ref.mature, each position mapped c./n. -> genomic with reftx_ref.c_to_g / n_to_g and back with
reftx_ref.g_to_tx, the span and ALT rules on slices of that string, vrs_ref.normalize over the mRNA as ONE sequence and
vrs_ref.vrs_id over "SQ." + sha512t24u(mRNA).  The parser is hgvs_ref's.  No import of the library.  Statuses are the library's
(csrc/hgvs_core.h); a position that is intronic or outside the mature mRNA (the reference's OutsideMatureMrna) is
MAPPING_ERROR with detail reftx_ref.NOT_EXONIC."""
import hgvs_ref as HR
import reftx_ref as R
import vrs_ref as V
from hgvs_ref import (INCONSISTENT_EDIT, MAPPING_ERROR, NO_MANE_TRANSCRIPT, NORMALIZE_ERROR, OK, OUT_OF_BOUNDS, PARSE_ERROR,  # noqa: F401
                      REF_MISMATCH, TRANSCRIPT_NOT_FOUND, UNKNOWN_CHROM, UNSUPPORTED_EDIT, UNSUPPORTED_REFERENCE_TYPE, Failure)

OUTSIDE_TEXT = "position %d on %s is intronic or outside the mature mRNA (no transcript-mRNA coordinate)"


def accession_of(mrna: bytes) -> str:
    return "SQ." + V.sha512t24u(mrna)


def bridge_one(seqs: dict, transcripts: list, text):
    """one expression over an assembly {name: bytes} and a list of restatement transcripts -> {"status", "detail", "warning",
    "tx" (the transcript's accession or None), "accession" ("SQ." + digest of the mRNA, or None), "start", "end" (normalized,
    on the mRNA), "id", "span": (start, end, ALT) before normalization, "text": the reference's message for an intronic
    position}"""
    out = {"status": OK, "detail": 0, "warning": 0, "tx": None, "accession": None, "start": 0, "end": 0, "id": None, "span": None, "text": None}
    try:
        try:
            v = HR.parse(text)
        except HR.ParseError:
            raise Failure(PARSE_ERROR)
        except HR.Protein:
            raise Failure(UNSUPPORTED_REFERENCE_TYPE)
        pe, rt = v["pos_edit"], v["reference_type"]
        # build_transcript_allele_parts
        if rt not in "cn":
            raise Failure(UNSUPPORTED_REFERENCE_TYPE)
        out["warning"] = 1 if pe["uncertain"] else 0
        acc, tx = v["accession"], None
        if HR.looks_like_gene_symbol(acc):
            tx = R.lookup_mane(transcripts, acc)
            if tx is None:
                raise Failure(NO_MANE_TRANSCRIPT)
            acc = tx["accession"]
        edit, kind = pe["edit"], pe["location_kind"]

        def forward(p):  # position_to_genomic_interbase: the provider is asked here for the first time
            t = tx or R.lookup(transcripts, acc)
            if t is None:
                raise Failure(TRANSCRIPT_NOT_FOUND)
            st, g = R.c_to_g(t, p["base"], p["offset"], p["datum"] == "cds_stop") if rt == "c" else R.n_to_g(t, p["base"], p["offset"])
            if st != R.OK:
                raise Failure(MAPPING_ERROR, st)
            return g

        def back(g):  # map_g_to_tx
            st, off = R.g_to_tx(tx or R.lookup(transcripts, acc), g)
            if st == R.NOT_EXONIC:
                out["text"] = OUTSIDE_TEXT % (g, acc)
            if st != R.OK:
                raise Failure(MAPPING_ERROR, st)
            return off

        # transcript_interbase_span
        uncertain = kind == "whole_sequence" or "uncertain" in (pe["start"]["kind"], (pe["end"] or pe["start"])["kind"])
        if edit["kind"] == "insertion":
            if uncertain:
                raise Failure(UNSUPPORTED_EDIT)
            if kind == "single":
                start = end = back(forward(pe["start"]["position"])) + 1
            else:
                ga, gb = forward(pe["start"]["position"]), forward(pe["end"]["position"])
                a, b = back(ga), back(gb)
                if abs(a - b) != 1:
                    raise Failure(INCONSISTENT_EDIT)
                start = end = max(a, b)
        else:
            if edit["kind"] in ("inversion", "unknown", "copy", "repeat") or uncertain:
                raise Failure(UNSUPPORTED_EDIT)
            ga = forward(pe["start"]["position"])
            gb = forward(pe["end"]["position"]) if kind == "range" else ga
            lo, hi = back(min(ga, gb)), back(max(ga, gb))
            start, end = min(lo, hi), max(lo, hi) + 1
        tx = tx or R.lookup(transcripts, acc)
        # mature_mrna
        st, mrna = R.mature(seqs, tx)
        if st != R.SEQ_OK:
            raise {R.SEQ_NO_SEQUENCE: Failure(UNKNOWN_CHROM), R.SEQ_PAST_END: Failure(OUT_OF_BOUNDS)}.get(st, Failure(MAPPING_ERROR, R.BAD_EXONS))
        if end > len(mrna):
            raise Failure(OUT_OF_BOUNDS)
        actual = mrna[start:end]
        # compute_alt_transcript: verbatim, no complement
        if edit["kind"] in ("substitution", "insertion", "delins"):
            alt = edit["alt"].encode()
        else:
            alt = {"deletion": b"", "duplication": actual + actual, "identity": actual}[edit["kind"]]
        out["span"] = (start, end, alt)
        if edit["ref"] is not None and edit["ref"].encode() != actual:
            raise Failure(REF_MISMATCH)
        # finalize_transcript_vrs_id
        try:
            ns, ne, allele = V.normalize(mrna, start, actual, alt)
        except V.NormalizeError as e:
            raise Failure(NORMALIZE_ERROR, e.status)
        accession = accession_of(mrna)
        out.update(tx=acc, accession=accession, start=ns, end=ne, id=V.vrs_id(accession, ns, ne, allele))
    except Failure as f:
        out.update(status=f.status, detail=f.detail)
    return out


def bridge(seqs, transcripts, strings):
    return [bridge_one(seqs, transcripts, s) for s in strings]


def alleles(seqs: dict, transcripts: list, rows):
    """rows of (accession, start, ref, alt) on transcripts -> per row (status of vrs_ref, start, end, id, "SQ." accession)"""
    out = []
    for acc, start, ref, alt in rows:
        tx = R.lookup(transcripts, acc)
        st, mrna = R.mature(seqs, tx)
        if st != R.SEQ_OK:
            out.append((V.UNKNOWN_CHROMOSOME, 0, 0, None, None))
            continue
        try:
            ns, ne, allele = V.normalize(mrna, start, ref, alt)
        except V.NormalizeError as e:
            out.append((e.status, 0, 0, None, None))
            continue
        out.append((V.OK, ns, ne, V.vrs_id(accession_of(mrna), ns, ne, allele), accession_of(mrna)))
    return out
