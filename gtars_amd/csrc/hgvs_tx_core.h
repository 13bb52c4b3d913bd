// hgvs_tx_core.h -- the row rules of K23, the transcript-anchored HGVS-to-VRS bridge (gtars-vrs/src/hgvs/bridge.rs:226-534:
// build_transcript_allele_parts, transcript_interbase_span, compute_alt_transcript), as plain C++17 next to hgvs_core.h, so
// that hgvs.cpp, the kernels of hgvs_tx.hip and a stand-alone checking program share one text.  The allele lies on the
// transcript's own mature mRNA: coordinates are 0-based interbase offsets on it, every byte is in transcript orientation,
// and nothing is reverse-complemented.
#pragma once

#include "hgvs_core.h"

namespace gtars {

// the mature mRNA of one transcript read out of its chromosome a byte at a time; the exon is searched only when the
// position leaves the one that is open
struct TxMrnaCursor {
    TxExons x;
    const uint8_t *seq;  // the chromosome's first byte
    uint32_t k = 0;
    uint64_t ts = 0, te = 0;  // the open exon holds transcript positions [ts, te); none yet
    GT_TX_HD uint32_t at(uint64_t p) {
        if (p < ts || p >= te) {
            k = x.at(tx_exon_of(x, p));
            ts = x.ts[k], te = ts + (x.ge[k] - x.gs[k]);
        }
        return tx_base(x, seq, k, p - ts);
    }
};

// what the bridge leaves of one row before normalization: the span [start, start + ref_len) on the mature mRNA of
// transcript `tx`, whose bytes are REF, and the ALT's length and recipe (HGVS_ALT_TEXT or HGVS_ALT_SPAN)
struct HgvsTxSpan {
    uint8_t status = HGVS_OK, detail = 0, mode = HGVS_ALT_TEXT;
    uint32_t tx = TX_NONE;
    uint64_t start = 0, ref_len = 0, alt_len = 0;
};

// one position c. / n. -> genomic -> offset on the mature mRNA (position_to_genomic_interbase, then map_g_to_tx).  The
// second step's TX_NOT_EXONIC is the reference's OutsideMatureMrna: a mapping error with that detail.
GT_TX_HD uint8_t hgvs_tx_forward(const TxTables &t, uint32_t kind, uint32_t tx, int64_t base, int64_t off, uint32_t star, uint64_t *g,
                                 uint8_t *detail) {
    const uint8_t st = tx_map_one(t, tx, kind == HGVS_REF_C ? TX_KIND_C : TX_KIND_N, base, off, star, g);
    if (st == TX_OK) return HGVS_OK;
    *detail = st;
    return HGVS_MAPPING_ERROR;
}
GT_TX_HD uint8_t hgvs_tx_back(const TxTables &t, uint32_t tx, uint64_t g, uint64_t *p, uint8_t *detail) {
    const uint8_t st = tx_map_one(t, tx, TX_KIND_G, (int64_t)g, 0, 0, p);
    if (st == TX_OK) return HGVS_OK;
    *detail = st;
    return HGVS_MAPPING_ERROR;
}

// One row in the reference's order of checks: the reference type, the MANE lookup's result, the edits and location kinds
// range_and_edit_to_genomic refuses (before the provider is asked anything, so before an unknown transcript), the
// transcript, both positions forward, both back, the span rule, the transcript's sequence (mature_mrna's failures), the
// bounds against the transcript's length, compute_alt_transcript and the REF cross-check against the mRNA's bytes as
// written.  Reads the assembly only inside exons of a transcript whose seq_status is TXSEQ_OK.
GT_TX_HD HgvsTxSpan hgvs_tx_span_one(const TxTables &t, const HgvsGenome &g, const HgvsCols &c, uint64_t i) {
    HgvsTxSpan r;
    const uint32_t pre = c.pre[i], kind = c.kind[i], loc = c.loc[i], edit = c.edit[i], flags = c.flags[i], tx = c.tx[i];
    if (pre == HGVS_PARSE_ERROR || pre == HGVS_UNSUPPORTED_REFERENCE_TYPE) return r.status = (uint8_t)pre, r;
    // (columns that do not come from the parser: alleles outside the text are no expression)
    if (c.text_off[i] > c.text_bytes || (uint64_t)c.ref_off[i] + c.ref_len[i] > c.text_bytes - c.text_off[i] ||
        (uint64_t)c.alt_off[i] + c.alt_len[i] > c.text_bytes - c.text_off[i])
        return r.status = HGVS_PARSE_ERROR, r;
    if (kind != HGVS_REF_C && kind != HGVS_REF_N) return r.status = HGVS_UNSUPPORTED_REFERENCE_TYPE, r;
    if (pre == HGVS_NO_MANE_TRANSCRIPT) return r.status = HGVS_NO_MANE_TRANSCRIPT, r;
    if (edit == HGVS_EDIT_INV || edit >= HGVS_EDIT_UNKNOWN || loc > HGVS_LOC_RANGE) return r.status = HGVS_UNSUPPORTED_EDIT, r;
    if (pre != HGVS_OK) return r.status = (uint8_t)pre, r;
    if (tx >= t.n_tx) return r.status = HGVS_TRANSCRIPT_NOT_FOUND, r;
    uint64_t ga = 0, gb = 0, a = 0, b = 0, start, end;
    if ((r.status = hgvs_tx_forward(t, kind, tx, c.base1[i], c.off1[i], flags & HGVS_STAR1, &ga, &r.detail)) != HGVS_OK) return r;
    if (loc == HGVS_LOC_SINGLE) {
        if ((r.status = hgvs_tx_back(t, tx, ga, &a, &r.detail)) != HGVS_OK) return r;
        // an insertion sits between bases a and a + 1 of the transcript on either strand
        if (edit == HGVS_EDIT_INS) start = end = a + 1;
        else start = a, end = a + 1;
    } else {
        if ((r.status = hgvs_tx_forward(t, kind, tx, c.base2[i], c.off2[i], flags & HGVS_STAR2, &gb, &r.detail)) != HGVS_OK) return r;
        if ((r.status = hgvs_tx_back(t, tx, ga, &a, &r.detail)) != HGVS_OK) return r;
        if ((r.status = hgvs_tx_back(t, tx, gb, &b, &r.detail)) != HGVS_OK) return r;
        const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
        if (edit == HGVS_EDIT_INS) {
            // adjacent IN TRANSCRIPT SPACE: the two bases of an exon junction are far apart on the genome
            if (hi - lo != 1) return r.status = HGVS_INCONSISTENT_EDIT, r;
            start = end = hi;
        } else {
            start = lo, end = hi + 1;
        }
    }
    // mature_mrna
    const uint32_t ss = t.seq_status[tx];
    if (ss == TXSEQ_NO_SEQUENCE) return r.status = HGVS_UNKNOWN_CHROM, r;
    if (ss == TXSEQ_PAST_END) return r.status = HGVS_OUT_OF_BOUNDS, r;
    if (ss != TXSEQ_OK) return r.status = HGVS_MAPPING_ERROR, r.detail = TX_BAD_EXONS, r;
    if (end > t.len[tx]) return r.status = HGVS_OUT_OF_BOUNDS, r;
    const uint64_t span = end - start;
    // compute_alt_transcript: the alternate as written, or the span once (identity) or twice (dup)
    uint64_t alt_len = 0;
    uint8_t mode = HGVS_ALT_TEXT;
    if (edit == HGVS_EDIT_SUB || edit == HGVS_EDIT_INS || edit == HGVS_EDIT_DELINS) alt_len = c.alt_len[i];
    else if (edit == HGVS_EDIT_DUP) alt_len = 2 * span, mode = HGVS_ALT_SPAN;
    else if (edit == HGVS_EDIT_IDENTITY) alt_len = span, mode = HGVS_ALT_SPAN;
    // the REF cross-check: the parsed reference, byte for byte as written, against the mRNA
    if (flags & HGVS_HAS_REF) {
        const uint8_t *ref = c.text + c.text_off[i] + c.ref_off[i];
        const uint64_t n_ref = c.ref_len[i];
        if (n_ref != span) return r.status = HGVS_REF_MISMATCH, r;
        TxMrnaCursor m{tx_exons(t, tx), span ? g.seq_of(t.chrom[tx]) : nullptr};
        for (uint64_t k = 0; k < n_ref; ++k)
            if (ref[k] != m.at(start + k)) return r.status = HGVS_REF_MISMATCH, r;
    }
    r.tx = tx, r.start = start, r.ref_len = span, r.alt_len = alt_len, r.mode = mode;
    return r;
}

// byte k < ref_len + alt_len of a row's REF | ALT.  mrna: the first byte of the transcript's mature mRNA (upper case
// already), alt: the parsed alternate's first byte.
GT_TX_HD uint32_t hgvs_tx_pool_byte(const uint8_t *mrna, uint64_t start, uint64_t ref_len, uint32_t mode, const uint8_t *alt, uint64_t k) {
    if (k < ref_len) return mrna[start + k];
    const uint64_t j = k - ref_len;
    if (mode == HGVS_ALT_SPAN) return mrna[start + (j >= ref_len ? j - ref_len : j)];
    return alt[j];
}

}  // namespace gtars
