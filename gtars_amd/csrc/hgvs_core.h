// hgvs_core.h -- the rules of K20 as plain C++17 (no HIP includes, no library state), so that hgvs.cpp, the kernels of
// hgvs.hip and a stand-alone checking program share one text: the HGVS parser for the nucleotide grammar
// (gtars-vrs/src/hgvs/parser.rs, ast.rs) and the arithmetic of the HGVS-to-VRS bridge (bridge.rs:552-913) over the mapping
// tables of reftx_core.h.  Under hipcc the functions the kernels call are __host__ __device__; under a host compiler they
// are ordinary inline functions.
//
// Protein expressions (p.) are not parsed: the row gets its accession, gene and reference type and the status
// HGVS_UNSUPPORTED_REFERENCE_TYPE, which is what the bridge answers for them anyway.  It is the one narrowing of the parser.
#pragma once

#include <cstdint>
#include <cstring>

#include "reftx_core.h"

namespace gtars {

// per-row status of the bridge.  1 is HgvsError::Parse, 2 .. 11 are BridgeError's kinds as the genome path raises them
// (bridge.rs:55-86; Provider is split into its three causes)
enum : uint8_t {
    HGVS_OK = 0,
    HGVS_PARSE_ERROR = 1,
    HGVS_UNSUPPORTED_REFERENCE_TYPE = 2,  // m. r. p.
    HGVS_UNSUPPORTED_EDIT = 3,            // inv, unknown, copy, repeat, a whole-sequence edit, an uncertain position range
    HGVS_TRANSCRIPT_NOT_FOUND = 4,
    HGVS_NO_MANE_TRANSCRIPT = 5,
    HGVS_UNKNOWN_CHROM = 6,
    HGVS_MAPPING_ERROR = 7,    // detail: the TX_* code of reftx_core.h
    HGVS_OUT_OF_BOUNDS = 8,
    HGVS_INCONSISTENT_EDIT = 9,
    HGVS_REF_MISMATCH = 10,
    HGVS_NORMALIZE_ERROR = 11,  // detail: the VRS_* code of vrs_core.h
    HGVS_N_STATUS = 12,
};
inline const char *hgvs_status_name(uint32_t s) {
    static const char *const names[HGVS_N_STATUS] = {"ok", "parse_error", "unsupported_reference_type", "unsupported_edit",
                                                     "transcript_not_found", "no_mane_transcript", "unknown_chromosome", "mapping_error",
                                                     "out_of_bounds", "inconsistent_edit", "ref_mismatch", "normalize_error"};
    return s < HGVS_N_STATUS ? names[s] : nullptr;
}

enum : uint8_t { HGVS_REF_G = 0, HGVS_REF_C = 1, HGVS_REF_N = 2, HGVS_REF_M = 3, HGVS_REF_R = 4, HGVS_REF_P = 5 };
enum : uint8_t { HGVS_DATUM_SEQ_START = 0, HGVS_DATUM_CDS_START = 1, HGVS_DATUM_CDS_END = 2 };
enum : uint8_t {
    HGVS_LOC_SINGLE = 0,
    HGVS_LOC_RANGE = 1,
    HGVS_LOC_WHOLE = 2,
    HGVS_LOC_UNCERTAIN_START = 3,
    HGVS_LOC_UNCERTAIN_END = 4,
    HGVS_LOC_UNCERTAIN_BOTH = 5,
};
enum : uint8_t {
    HGVS_EDIT_SUB = 0,
    HGVS_EDIT_DEL = 1,
    HGVS_EDIT_DUP = 2,
    HGVS_EDIT_INS = 3,
    HGVS_EDIT_DELINS = 4,
    HGVS_EDIT_INV = 5,
    HGVS_EDIT_IDENTITY = 6,
    HGVS_EDIT_UNKNOWN = 7,
    HGVS_EDIT_COPY = 8,
    HGVS_EDIT_REPEAT = 9,
};
// flags of a row and of the columns; the two star bits exist in the columns only (a row has the datum of every position)
enum : uint8_t { HGVS_HAS_GENE = 1, HGVS_HAS_REF = 2, HGVS_UNCERTAIN = 4, HGVS_STAR1 = 8, HGVS_STAR2 = 16 };
enum : uint8_t { HGVS_WARN_UNCERTAIN = 1 };

// One parsed expression (gtars_hgvs_row of the C ABI).  Accession, gene, ref and alt are (offset, length) spans into the
// input text: nothing is copied.  pos[0] is the start (or its low bound), pos[1] the start's high bound, pos[2] the end (or
// its low bound), pos[3] the end's high bound; `present` is 0 for a position the location kind does not have and for "?".
// A repeat keeps its unit in the ref span (without HGVS_HAS_REF) and its count in `count`, a copy its count.
struct HgvsPosition {
    int64_t base, offset;
    uint8_t datum, present;
    uint8_t reserved[6];
};
struct HgvsRow {
    uint32_t acc_off, acc_len, gene_off, gene_len, ref_off, ref_len, alt_off, alt_len;
    HgvsPosition pos[4];
    uint32_t count;
    uint8_t ref_type, loc, edit, flags;
};

// is_iupac (parser.rs:571-579)
inline bool hgvs_is_iupac(uint8_t b) {
    switch (b) {
        case 'A': case 'C': case 'G': case 'T': case 'U': case 'N': case 'a': case 'c': case 'g': case 't': case 'u': case 'n':
        case 'R': case 'Y': case 'S': case 'W': case 'K': case 'M': case 'B': case 'D': case 'H': case 'V':
        case 'r': case 'y': case 's': case 'w': case 'k': case 'm': case 'b': case 'd': case 'h': case 'v':
            return true;
        default:
            return false;
    }
}

// The parser: parser.rs, method for method.  It reads text[0, n) and nothing else.  An error keeps the byte position the
// reference reports and one of its messages.
struct HgvsParser {
    const uint8_t *s;
    size_t n, pos = 0;
    const char *msg = nullptr;

    int peek() const { return pos < n ? s[pos] : -1; }
    bool fail(const char *m) {
        if (!msg) msg = m;
        return false;
    }
    bool expect(uint8_t b, const char *ctx) {
        if (peek() == b) return ++pos, true;
        return fail(ctx);
    }
    bool try_consume(uint8_t b) {
        if (peek() == b) return ++pos, true;
        return false;
    }
    bool try_keyword(const char *kw) {
        const size_t k = strlen(kw);
        if (n - pos >= k && memcmp(s + pos, kw, k) == 0) return pos += k, true;
        return false;
    }
    bool digit() const { return pos < n && s[pos] >= '0' && s[pos] <= '9'; }
    // str::parse::<u64> of a run of digits
    bool parse_uint(uint64_t *out) {
        const size_t start = pos;
        while (digit()) ++pos;
        if (pos == start) return fail("expected integer");
        uint64_t v = 0;
        for (size_t i = start; i < pos; ++i) {
            const uint64_t d = (uint64_t)(s[i] - '0');
            if (v > (UINT64_MAX - d) / 10) return fail("invalid integer");
            v = v * 10 + d;
        }
        *out = v;
        return true;
    }
    // (`as u32`: the count wraps)
    bool parse_count(uint32_t *out) {
        uint64_t v;
        if (!parse_uint(&v)) return false;
        *out = (uint32_t)v;
        return true;
    }
    // `as i64` and the negations wrap, as the reference's release build does
    bool parse_position(uint8_t rt, HgvsPosition *p) {
        p->datum = rt == HGVS_REF_C ? HGVS_DATUM_CDS_START : HGVS_DATUM_SEQ_START;
        if (rt == HGVS_REF_C && try_consume('*')) p->datum = HGVS_DATUM_CDS_END;
        bool neg = false;
        if (peek() == '-') neg = true, ++pos;
        else if (peek() == '+') ++pos;
        uint64_t v;
        if (!parse_uint(&v)) return false;
        p->base = (int64_t)(neg ? 0 - v : v);
        p->offset = 0;
        if (peek() == '+' || peek() == '-') {
            const bool minus = peek() == '-';
            ++pos;
            if (!parse_uint(&v)) return false;
            p->offset = (int64_t)(minus ? 0 - v : v);
        }
        p->present = 1;
        return true;
    }
    // `pos1_pos2`, `?_pos` or `pos_?` inside the parentheses of an uncertain position
    bool parse_uncertain_pair(uint8_t rt, HgvsPosition *low, HgvsPosition *high) {
        if (!try_consume('?') && !parse_position(rt, low)) return false;
        if (!expect('_', "expected `_` in uncertain position range")) return false;
        if (!try_consume('?') && !parse_position(rt, high)) return false;
        return true;
    }
    bool parse_location_range(uint8_t rt, HgvsRow *r) {
        bool start_uncertain = false, end_uncertain = false;
        if (try_consume('(')) {
            if (!parse_uncertain_pair(rt, &r->pos[0], &r->pos[1])) return false;
            if (!expect(')', "expected `)` after uncertain position")) return false;
            if (!r->pos[0].present && !r->pos[1].present) return fail("both bounds unknown");
            start_uncertain = true;
        } else if (!parse_position(rt, &r->pos[0])) {
            return false;
        }
        if (!try_consume('_')) {
            // (an uncertain start without an end is Single of its "main" position: the high bound, else the low one)
            if (start_uncertain) {
                if (r->pos[1].present) r->pos[0] = r->pos[1];
                r->pos[1] = HgvsPosition{};
            }
            r->loc = HGVS_LOC_SINGLE;
            return true;
        }
        if (try_consume('(')) {
            if (!parse_uncertain_pair(rt, &r->pos[2], &r->pos[3])) return false;
            if (!expect(')', "expected `)` after uncertain position")) return false;
            if (!r->pos[2].present && !r->pos[3].present) return fail("both bounds unknown");
            end_uncertain = true;
        } else if (!parse_position(rt, &r->pos[2])) {
            return false;
        }
        r->loc = start_uncertain ? (end_uncertain ? HGVS_LOC_UNCERTAIN_BOTH : HGVS_LOC_UNCERTAIN_START)
                                 : (end_uncertain ? HGVS_LOC_UNCERTAIN_END : HGVS_LOC_RANGE);
        return true;
    }
    // a run over is_iupac: its span; false when it is empty
    bool iupac_run(uint32_t *off, uint32_t *len) {
        const size_t start = pos;
        while (pos < n && hgvs_is_iupac(s[pos])) ++pos;
        *off = (uint32_t)start, *len = (uint32_t)(pos - start);
        return pos != start;
    }
    bool parse_edit(HgvsRow *r) {
        if (try_consume('=')) return r->edit = HGVS_EDIT_IDENTITY, true;
        if (try_consume('?')) return r->edit = HGVS_EDIT_UNKNOWN, true;
        if (try_keyword("delins")) {
            r->edit = HGVS_EDIT_DELINS;
            if (!iupac_run(&r->alt_off, &r->alt_len)) return fail("expected nucleotide sequence");
            return true;
        }
        if (try_keyword("del")) {
            if (iupac_run(&r->ref_off, &r->ref_len)) r->flags |= HGVS_HAS_REF;
            if (try_keyword("ins")) {
                r->edit = HGVS_EDIT_DELINS;
                if (!iupac_run(&r->alt_off, &r->alt_len)) return fail("expected nucleotide sequence");
                return true;
            }
            if (!(r->flags & HGVS_HAS_REF))
                while (digit()) ++pos;  // `delN`, a legacy count: consumed
            return r->edit = HGVS_EDIT_DEL, true;
        }
        if (try_keyword("dup")) {
            if (iupac_run(&r->ref_off, &r->ref_len)) r->flags |= HGVS_HAS_REF;
            return r->edit = HGVS_EDIT_DUP, true;
        }
        if (try_keyword("ins")) {
            r->edit = HGVS_EDIT_INS;
            if (!iupac_run(&r->alt_off, &r->alt_len)) return fail("expected nucleotide sequence");
            return true;
        }
        if (try_keyword("inv")) {
            if (iupac_run(&r->ref_off, &r->ref_len)) r->flags |= HGVS_HAS_REF;
            return r->edit = HGVS_EDIT_INV, true;
        }
        if (try_keyword("copy")) {
            r->edit = HGVS_EDIT_COPY;
            return parse_count(&r->count);
        }
        if (!iupac_run(&r->ref_off, &r->ref_len)) return fail("expected edit");
        if (try_consume('=')) {  // `G=`: the reference allele is dropped
            r->ref_off = r->ref_len = 0;
            return r->edit = HGVS_EDIT_IDENTITY, true;
        }
        if (try_consume('[')) {
            r->edit = HGVS_EDIT_REPEAT;
            if (!parse_count(&r->count)) return false;
            return expect(']', "expected `]` after repeat count");
        }
        if (!expect('>', "expected `>` in substitution")) return false;
        if (!iupac_run(&r->alt_off, &r->alt_len)) return fail("expected alternate allele");
        r->flags |= HGVS_HAS_REF;
        return r->edit = HGVS_EDIT_SUB, true;
    }
    // the look-ahead of parser.rs:135-170: `(` opens an outer wrapper unless what follows reads `?` or `number_`
    bool outer_uncertain() {
        if (peek() != '(') return false;
        const size_t saved = pos;
        ++pos;
        bool outer = false;
        if (peek() != '?') {
            if (peek() == '-' || peek() == '*') ++pos;
            while (digit()) ++pos;
            if (peek() == '+' || peek() == '-') {
                ++pos;
                while (digit()) ++pos;
            }
            outer = peek() != '_';
        }
        pos = saved;
        return outer;
    }
    // HGVS_OK, HGVS_PARSE_ERROR or -- p. -- HGVS_UNSUPPORTED_REFERENCE_TYPE
    uint8_t parse_variant(HgvsRow *r) {
        const size_t acc_start = pos;
        while (pos < n && s[pos] != ':' && s[pos] != '(') ++pos;
        if (pos == acc_start) return fail("expected accession"), HGVS_PARSE_ERROR;
        r->acc_off = (uint32_t)acc_start, r->acc_len = (uint32_t)(pos - acc_start);
        if (try_consume('(')) {
            const size_t g_start = pos;
            while (pos < n && s[pos] != ')') ++pos;
            if (pos == g_start) return fail("expected gene symbol after `(`"), HGVS_PARSE_ERROR;
            r->gene_off = (uint32_t)g_start, r->gene_len = (uint32_t)(pos - g_start), r->flags |= HGVS_HAS_GENE;
            if (!expect(')', "expected `)` after gene symbol")) return HGVS_PARSE_ERROR;
        }
        if (!expect(':', "expected `:` after accession")) return HGVS_PARSE_ERROR;
        const int t = peek();
        if (t >= 0) ++pos;  // (consume_byte: the position of this error lies behind the byte)
        switch (t) {
            case 'g': r->ref_type = HGVS_REF_G; break;
            case 'c': r->ref_type = HGVS_REF_C; break;
            case 'n': r->ref_type = HGVS_REF_N; break;
            case 'm': r->ref_type = HGVS_REF_M; break;
            case 'r': r->ref_type = HGVS_REF_R; break;
            case 'p': r->ref_type = HGVS_REF_P; break;
            default: return fail("expected reference type (g/c/n/m/r/p)"), HGVS_PARSE_ERROR;
        }
        if (!expect('.', "expected `.` after reference type")) return HGVS_PARSE_ERROR;
        if (r->ref_type == HGVS_REF_P) return HGVS_UNSUPPORTED_REFERENCE_TYPE;
        const uint8_t rt = r->ref_type;
        if (peek() == '=' || peek() == '?') {
            r->loc = HGVS_LOC_WHOLE;
            if (!parse_edit(r)) return HGVS_PARSE_ERROR;
        } else if (outer_uncertain()) {
            ++pos;
            if (!parse_location_range(rt, r) || !parse_edit(r)) return HGVS_PARSE_ERROR;
            if (!expect(')', "expected `)` to close uncertain posedit")) return HGVS_PARSE_ERROR;
            r->flags |= HGVS_UNCERTAIN;
        } else {
            if (!parse_location_range(rt, r) || !parse_edit(r)) return HGVS_PARSE_ERROR;
            if (r->loc >= HGVS_LOC_UNCERTAIN_START) r->flags |= HGVS_UNCERTAIN;
        }
        if (pos < n) return fail("trailing characters after variant"), HGVS_PARSE_ERROR;
        return HGVS_OK;
    }
};

// parse(): the status, and for HGVS_PARSE_ERROR the byte position and the message of the error (either may be null).
// Texts of 2^32 bytes and more are refused: the spans are u32.
inline uint8_t hgvs_parse(const char *text, size_t len, HgvsRow *out, size_t *err_pos = nullptr, const char **err_msg = nullptr) {
    *out = HgvsRow{};
    HgvsParser p{(const uint8_t *)text, len};
    uint8_t st;
    if (len >= 0xFFFFFFFFull) st = HGVS_PARSE_ERROR, p.fail("expression too long");
    else st = p.parse_variant(out);
    if (err_pos) *err_pos = st == HGVS_PARSE_ERROR ? p.pos : 0;
    if (err_msg) *err_msg = st == HGVS_PARSE_ERROR ? p.msg : nullptr;
    return st;
}

// looks_like_gene_symbol (bridge.rs:552-589)
inline bool hgvs_looks_like_gene_symbol(const char *acc, size_t n) {
    if (memchr(acc, '.', n)) return false;
    if (n == 2 && memcmp(acc, "MT", 2) == 0) return false;
    static const char *const prefixes[11] = {"NC_", "NM_", "NR_", "NG_", "NW_", "NT_", "XM_", "XR_", "ENST", "ENSG", "chr"};
    for (const char *p : prefixes) {
        const size_t k = strlen(p);
        if (n >= k && memcmp(acc, p, k) == 0) return false;
    }
    if (n >= 3 && (memcmp(acc, "GL", 2) == 0 || memcmp(acc, "KI", 2) == 0) && acc[2] >= '0' && acc[2] <= '9') return false;
    return true;
}

// ---- the bridge ------------------------------------------------------------------------------------------------------
// revcomp's table: exactly ACGTN, 0 for any other byte (lower case included)
GT_TX_HD uint32_t hgvs_complement(uint32_t b) { return b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : b == 'G' ? 'C' : b == 'N' ? 'N' : 0u; }

// The rows of a batch as columns, host vectors or device arrays (gtars_hgvs_columns of the C ABI has the same members).
// pre: what parsing and the accession lookup left (HGVS_OK, or the row's status); kind / loc / edit: the enums above;
// flags: HGVS_HAS_REF, HGVS_UNCERTAIN, HGVS_STAR1 / HGVS_STAR2 for a c.*N first / second position; tx: the transcript's
// index in the store for c. and n., the chromosome id of the assembly for g. (2^32 - 1: unknown); base1 / off1: the
// single position or the range's start, base2 / off2: the range's end; the alleles are text[text_off + ref_off, + ref_len)
// and text[text_off + alt_off, + alt_len).
struct HgvsCols {
    const uint8_t *pre = nullptr, *kind = nullptr, *loc = nullptr, *edit = nullptr, *flags = nullptr;
    const uint32_t *tx = nullptr;
    const int64_t *base1 = nullptr, *off1 = nullptr, *base2 = nullptr, *off2 = nullptr;
    const uint64_t *text_off = nullptr;
    const uint32_t *ref_off = nullptr, *ref_len = nullptr, *alt_off = nullptr, *alt_len = nullptr;
    const uint8_t *text = nullptr;
    uint64_t text_bytes = 0;
    uint64_t n = 0;
};

// the assembly as the bridge reads it: packed bytes, or one pointer per chromosome (seq_of)
struct HgvsGenome {
    const uint8_t *seq = nullptr;           // packed image, chromosome c at off[c] ...
    const uint64_t *off = nullptr;
    const uint8_t *const *chroms = nullptr; // ... or chromosome c at chroms[c]
    const uint64_t *len = nullptr;
    uint32_t n_chrom = 0;
    GT_TX_HD const uint8_t *seq_of(uint32_t c) const { return chroms ? chroms[c] : seq + off[c]; }
};

// how the ALT bytes of a row are made (HgvsSpan::mode)
enum : uint8_t { HGVS_ALT_TEXT = 0, HGVS_ALT_TEXT_REVCOMP = 1, HGVS_ALT_SPAN = 2 };

// what the bridge leaves of one row before normalization: the genomic span [start, start + ref_len) on `chrom`, whose
// upper-cased bytes are REF, and the ALT's length and recipe
struct HgvsSpan {
    uint8_t status = HGVS_OK, detail = 0, mode = HGVS_ALT_TEXT;
    uint32_t chrom = TX_NONE;
    uint64_t start = 0, ref_len = 0, alt_len = 0;
};

// position_to_genomic_interbase (bridge.rs:672-701) for the kinds the bridge supports
GT_TX_HD uint8_t hgvs_position_to_genomic(const TxTables &t, uint32_t kind, uint32_t tx, int64_t base, int64_t off, uint32_t star, uint64_t *ib,
                                          uint8_t *detail) {
    if (kind == HGVS_REF_G) {
        if (base < 1) return HGVS_INCONSISTENT_EDIT;
        *ib = (uint64_t)base - 1;
        return HGVS_OK;
    }
    const uint8_t st = tx_map_one(t, tx, kind == HGVS_REF_C ? TX_KIND_C : TX_KIND_N, base, off, star, ib);
    if (st == TX_OK) return HGVS_OK;
    *detail = st;
    return HGVS_MAPPING_ERROR;
}

// One row through resolve_chrom's last step, range_and_edit_to_genomic, the bounds check against the chromosome's own
// length, compute_alt and the REF cross-check (bridge.rs:625-667, 706-913), in the reference's order.  Reads the assembly
// only inside [start, start + ref_len) of a span that passed the bounds check.
GT_TX_HD HgvsSpan hgvs_span_one(const TxTables &t, const HgvsGenome &g, const HgvsCols &c, uint64_t i) {
    HgvsSpan r;
    const uint32_t kind = c.kind[i], loc = c.loc[i], edit = c.edit[i], flags = c.flags[i], tx = c.tx[i];
    if (c.pre[i] != HGVS_OK) return r.status = c.pre[i], r;
    // (columns that do not come from the parser: alleles outside the text are no expression)
    if (c.text_off[i] > c.text_bytes || (uint64_t)c.ref_off[i] + c.ref_len[i] > c.text_bytes - c.text_off[i] ||
        (uint64_t)c.alt_off[i] + c.alt_len[i] > c.text_bytes - c.text_off[i])
        return r.status = HGVS_PARSE_ERROR, r;
    if (kind > HGVS_REF_N) return r.status = HGVS_UNSUPPORTED_REFERENCE_TYPE, r;
    int strand = 1;
    uint32_t chrom;
    if (kind == HGVS_REF_G) {
        chrom = tx;
    } else {
        if (tx >= t.n_tx) return r.status = HGVS_TRANSCRIPT_NOT_FOUND, r;
        chrom = t.chrom[tx];
        strand = t.strand[tx];
    }
    if (chrom >= g.n_chrom) return r.status = HGVS_UNKNOWN_CHROM, r;
    if (edit == HGVS_EDIT_INV || edit >= HGVS_EDIT_UNKNOWN || loc > HGVS_LOC_RANGE) return r.status = HGVS_UNSUPPORTED_EDIT, r;
    uint64_t a = 0, b = 0, start, end;
    if ((r.status = hgvs_position_to_genomic(t, kind, tx, c.base1[i], c.off1[i], flags & HGVS_STAR1, &a, &r.detail)) != HGVS_OK) return r;
    if (loc == HGVS_LOC_SINGLE) {
        if (edit == HGVS_EDIT_INS) start = end = strand >= 0 ? a + 1 : a;
        else start = a, end = a + 1;
    } else {
        if ((r.status = hgvs_position_to_genomic(t, kind, tx, c.base2[i], c.off2[i], flags & HGVS_STAR2, &b, &r.detail)) != HGVS_OK) return r;
        const uint64_t lo = a < b ? a : b, hi = a < b ? b : a;
        if (edit == HGVS_EDIT_INS) {
            if (hi - lo != 1) return r.status = HGVS_INCONSISTENT_EDIT, r;
            start = end = hi;
        } else {
            start = lo, end = hi + 1;
        }
    }
    if (end > g.len[chrom]) return r.status = HGVS_OUT_OF_BOUNDS, r;
    const uint64_t span = end - start;
    const uint8_t *text = c.text + c.text_off[i];
    // compute_alt
    uint64_t alt_len = 0;
    uint8_t mode = HGVS_ALT_TEXT;
    if (edit == HGVS_EDIT_SUB || edit == HGVS_EDIT_INS || edit == HGVS_EDIT_DELINS) {
        alt_len = c.alt_len[i];
        if (strand < 0) {
            mode = HGVS_ALT_TEXT_REVCOMP;
            const uint8_t *alt = text + c.alt_off[i];
            for (uint64_t k = 0; k < alt_len; ++k)
                if (!hgvs_complement(alt[k])) return r.status = HGVS_INCONSISTENT_EDIT, r;
        }
    } else if (edit == HGVS_EDIT_DUP) {
        alt_len = 2 * span, mode = HGVS_ALT_SPAN;
    } else if (edit == HGVS_EDIT_IDENTITY) {
        alt_len = span, mode = HGVS_ALT_SPAN;
    }
    // the REF cross-check: the parsed reference, reverse-complemented on the reverse strand, against the span's bytes
    if (flags & HGVS_HAS_REF) {
        const uint8_t *ref = text + c.ref_off[i];
        const uint64_t n_ref = c.ref_len[i];
        if (strand < 0)
            for (uint64_t k = 0; k < n_ref; ++k)
                if (!hgvs_complement(ref[k])) return r.status = HGVS_INCONSISTENT_EDIT, r;
        if (n_ref != span) return r.status = HGVS_REF_MISMATCH, r;
        const uint8_t *seq = g.seq_of(chrom) + start;
        for (uint64_t k = 0; k < n_ref; ++k) {
            const uint32_t want = strand < 0 ? hgvs_complement(ref[n_ref - 1 - k]) : ref[k];
            if (want != tx_upper(seq[k])) return r.status = HGVS_REF_MISMATCH, r;
        }
    }
    r.chrom = chrom, r.start = start, r.ref_len = span, r.alt_len = alt_len, r.mode = mode;
    return r;
}

// byte k < ref_len + alt_len of a row's REF | ALT: REF is the span upper-cased; ALT is the parsed alternate as given, or
// read backwards through the complement, or the span once (identity) or twice (dup).  seq: the chromosome's first byte,
// alt: the parsed alternate's first byte.
GT_TX_HD uint32_t hgvs_pool_byte(const uint8_t *seq, uint64_t start, uint64_t ref_len, uint64_t alt_len, uint32_t mode, const uint8_t *alt,
                                 uint64_t k) {
    if (k < ref_len) return tx_upper(seq[start + k]);
    const uint64_t j = k - ref_len;
    if (mode == HGVS_ALT_SPAN) return tx_upper(seq[start + (j >= ref_len ? j - ref_len : j)]);
    if (mode == HGVS_ALT_TEXT_REVCOMP) return hgvs_complement(alt[alt_len - 1 - j]);
    return alt[j];
}

}  // namespace gtars
