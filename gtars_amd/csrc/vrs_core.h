// vrs_core.h -- the host-side rules of K18 as plain C++17 (no HIP, no library state), so that vrs.cpp, the host tail of
// the digest kernel and a stand-alone checking program share one text: allele normalization over bytes
// (gtars-vrs/src/normalize.rs:362-441), the two canonical digest texts (digest.rs:60-81) and the VCF line rules
// (vcf_core.rs:35-87).
#pragma once

#include <cstdint>
#include <cstring>
#include <string>

#include "sha512.h"

namespace gtars {

// per-allele status of the column calls: 1 .. 3 are NormalizeError's three kinds, 4 and 5 are the columns' own
enum : uint8_t {
    VRS_OK = 0,
    VRS_START_OUT_OF_BOUNDS = 1,  // start + len(REF) overflows u64
    VRS_REF_PAST_END = 2,         // start + len(REF) > the chromosome's length (a start beyond the chromosome ends here too)
    VRS_REF_MISMATCH = 3,         // REF differs from the assembly, both sides upper-cased
    VRS_NO_CHROM = 4,             // chromosome id outside the assembly, or no accession for it
    VRS_BAD_ALLELE = 5,           // REF or ALT does not lie inside the byte pool
};

inline uint8_t vrs_upper(uint8_t b) { return b >= 'a' && b <= 'z' ? (uint8_t)(b - 32) : b; }

// what normalization leaves: the normalized allele is seq[start, start + lroll) upper-cased, then alt[alt_skip, alt_skip +
// alt_len) as given, then seq[end - rroll, end) upper-cased
struct VrsNorm {
    uint8_t status = VRS_OK;
    uint64_t start = 0, end = 0;    // the new interbase interval
    uint64_t lroll = 0, rroll = 0;  // bases rolled left / right
    uint64_t alt_skip = 0, alt_len = 0;
    uint64_t seq_len() const { return lroll + alt_len + rroll; }
};

// normalize_ref over a chromosome's bytes.  The assembly is read through vrs_upper (the reference's store holds its
// sequences upper-cased, gtars-refget/src/fasta.rs:123); allele bytes are used as given.
inline VrsNorm vrs_normalize(const uint8_t *seq, uint64_t seq_len, uint64_t start, const uint8_t *ref, uint64_t ref_len,
                             const uint8_t *alt, uint64_t alt_len) {
    VrsNorm r;
    if (start + ref_len < start) {
        r.status = VRS_START_OUT_OF_BOUNDS;
        return r;
    }
    uint64_t s = start, e = start + ref_len;
    if (e > seq_len) {
        r.status = VRS_REF_PAST_END;
        return r;
    }
    for (uint64_t k = 0; k < ref_len; ++k)
        if (vrs_upper(ref[k]) != vrs_upper(seq[s + k])) {
            r.status = VRS_REF_MISMATCH;
            return r;
        }
    uint64_t rl = ref_len, al = alt_len, skip = 0;
    while (skip < rl && skip < al && ref[skip] == alt[skip]) ++skip;  // trim_left
    s += skip, rl -= skip, al -= skip;
    const uint8_t *rt = ref + skip, *at = alt + skip;
    uint64_t cut = 0;
    while (cut < rl && cut < al && rt[rl - 1 - cut] == at[al - 1 - cut]) ++cut;  // trim_right
    e -= cut, rl -= cut, al -= cut;
    uint64_t lroll = 0, rroll = 0;
    if (rl || al) {
        // roll_left: step d compares seq[s - 1 - d] with every non-empty allele at its circular index from the end
        uint64_t ir = rl ? rl - 1 : 0, ia = al ? al - 1 : 0;
        while (lroll < s) {
            const uint8_t base = vrs_upper(seq[s - 1 - lroll]);
            if ((rl && rt[ir] != base) || (al && at[ia] != base)) break;
            ++lroll;
            ir = ir ? ir - 1 : (rl ? rl - 1 : 0);
            ia = ia ? ia - 1 : (al ? al - 1 : 0);
        }
        ir = ia = 0;
        while (rroll < seq_len - e) {
            const uint8_t base = vrs_upper(seq[e + rroll]);
            if ((rl && rt[ir] != base) || (al && at[ia] != base)) break;
            ++rroll;
            if (rl && ++ir == rl) ir = 0;
            if (al && ++ia == al) ia = 0;
        }
    }
    r.start = s - lroll, r.end = e + rroll, r.lroll = lroll, r.rroll = rroll, r.alt_skip = skip, r.alt_len = al;
    return r;
}

// the normalized allele's bytes
inline std::string vrs_norm_sequence(const VrsNorm &r, const uint8_t *seq, const uint8_t *alt) {
    std::string out;
    out.reserve((size_t)r.seq_len());
    for (uint64_t k = 0; k < r.lroll; ++k) out.push_back((char)vrs_upper(seq[r.start + k]));
    out.append((const char *)alt + r.alt_skip, (size_t)r.alt_len);
    for (uint64_t k = 0; k < r.rroll; ++k) out.push_back((char)vrs_upper(seq[r.end - r.rroll + k]));
    return out;
}

// NormalizeError's Display (normalize.rs:306-330); the bytes of a mismatch as from_utf8_lossy would for ASCII
inline std::string vrs_error_text(uint8_t status, const uint8_t *seq, uint64_t seq_len, uint64_t start, const uint8_t *ref,
                                  uint64_t ref_len) {
    switch (status) {
        case VRS_START_OUT_OF_BOUNDS:
            return "start position " + std::to_string(start) + " exceeds sequence length " + std::to_string(seq_len);
        case VRS_REF_PAST_END:
            return "ref allele (start=" + std::to_string(start) + ", len=" + std::to_string(ref_len) + ") extends past sequence length " +
                   std::to_string(seq_len);
        case VRS_REF_MISMATCH: {
            std::string actual;
            for (uint64_t k = 0; k < ref_len; ++k) actual.push_back((char)vrs_upper(seq[start + k]));
            return "ref allele mismatch at interbase " + std::to_string(start) + ": VCF says " + std::string((const char *)ref, (size_t)ref_len) +
                   ", reference has " + actual;
        }
        case VRS_NO_CHROM: return "chromosome is not in the assembly or has no accession";
        case VRS_BAD_ALLELE: return "allele bytes lie outside the pool";
        default: return "";
    }
}

// ---- the two digest texts ---------------------------------------------------------------------------------------
// (literal writes, no JSON escaping: accessions are "SQ." + base64url, sequences are nucleotide letters, digest.rs:43-51)
constexpr const char *VRS_LOC_A = "{\"end\":";
constexpr const char *VRS_LOC_B = ",\"sequenceReference\":{\"refgetAccession\":\"";
constexpr const char *VRS_LOC_C = "\",\"type\":\"SequenceReference\"},\"start\":";
constexpr const char *VRS_LOC_D = ",\"type\":\"SequenceLocation\"}";
constexpr const char *VRS_AL_A = "{\"location\":\"";
constexpr const char *VRS_AL_B = "\",\"state\":{\"sequence\":\"";
constexpr const char *VRS_AL_C = "\",\"type\":\"LiteralSequenceExpression\"},\"type\":\"Allele\"}";

inline void vrs_location_digest(const char *accession, size_t acc_len, uint64_t start, uint64_t end, char out[32]) {
    std::string m = VRS_LOC_A + std::to_string(end) + VRS_LOC_B;
    m.append(accession, acc_len);
    m += VRS_LOC_C + std::to_string(start) + VRS_LOC_D;
    sha512t24u((const uint8_t *)m.data(), m.size(), out);
}

// the Allele message streamed from its five parts, nothing copied: head | left context | ALT | right context | tail
struct VrsAlleleSrc {
    const uint8_t *part[5];
    uint64_t left[5];
    bool upper[5];
    int k = 0;
    uint8_t next() {
        while (!left[k]) ++k;
        --left[k];
        const uint8_t b = *part[k]++;
        return upper[k] ? vrs_upper(b) : b;
    }
};

// digest of the Allele whose sequence is lctx (upper-cased) + alt + rctx (upper-cased)
inline void vrs_allele_digest(const char loc_digest[32], const uint8_t *lctx, uint64_t n_l, const uint8_t *alt, uint64_t n_a,
                              const uint8_t *rctx, uint64_t n_r, char out[32]) {
    std::string head = VRS_AL_A;
    head.append(loc_digest, 32);
    head += VRS_AL_B;
    const uint64_t n_tail = strlen(VRS_AL_C);
    VrsAlleleSrc src{{(const uint8_t *)head.data(), lctx, alt, rctx, (const uint8_t *)VRS_AL_C},
                     {head.size(), n_l, n_a, n_r, n_tail},
                     {false, true, false, true, false}};
    Sha512 s;
    sha512_stream(s, src, head.size() + n_l + n_a + n_r + n_tail);
    sha512t24u_text(s, out);
}

// ---- VCF lines --------------------------------------------------------------------------------------------------
struct VcfRecord {
    const char *chrom, *ref, *alts;
    size_t n_chrom, n_ref, n_alts;
    uint64_t pos;  // 0-based
};

// str::parse::<u64>: an optional '+', then one or more digits, no overflow
inline bool vcf_parse_u64(const char *p, size_t n, uint64_t &out) {
    size_t i = 0;
    if (i < n && p[i] == '+') ++i;
    if (i == n) return false;
    uint64_t v = 0;
    for (; i < n; ++i) {
        if (p[i] < '0' || p[i] > '9') return false;
        const uint64_t d = (uint64_t)(p[i] - '0');
        if (v > (UINT64_MAX - d) / 10) return false;
        v = v * 10 + d;
    }
    out = v;
    return true;
}

// parse_vcf_record (vcf_core.rs:65-87) on line[0, n) (the terminator may be included): false for a line that yields nothing
inline bool vcf_parse_line(const char *line, size_t n, VcfRecord &r) {
    while (n && (line[n - 1] == '\n' || line[n - 1] == '\r')) --n;
    if (!n || line[0] == '#') return false;
    // splitn(6, '\t'): fields 0 .. 4 end at a tab, or -- the last one present -- at the end of the line
    const char *f[5];
    size_t fl[5];
    size_t at = 0;
    for (int k = 0; k < 5; ++k) {
        if (at > n) return false;  // fewer than 5 fields
        const char *tab = at < n ? (const char *)memchr(line + at, '\t', n - at) : nullptr;
        f[k] = line + at;
        fl[k] = tab ? (size_t)(tab - (line + at)) : n - at;
        at = tab ? (size_t)(tab - line) + 1 : n + 1;
    }
    uint64_t pos1;
    if (!vcf_parse_u64(f[1], fl[1], pos1) || pos1 < 1) return false;
    r.chrom = f[0], r.n_chrom = fl[0];
    r.ref = f[3], r.n_ref = fl[3];
    r.alts = f[4], r.n_alts = fl[4];
    r.pos = pos1 - 1;
    return true;
}

// is_real_alt (vcf_core.rs:35-37)
inline bool vcf_is_real_alt(const char *a, size_t n) { return !(n == 0 || a[0] == '<' || (n == 1 && (a[0] == '*' || a[0] == '.'))); }

// f(alt, len) for every real ALT of the field, in order (str::split(','): an empty field has one empty piece)
template <class F>
inline void vcf_for_real_alts(const char *alts, size_t n, F &&f) {
    size_t at = 0;
    for (;;) {
        const char *c = at < n ? (const char *)memchr(alts + at, ',', n - at) : nullptr;
        const size_t len = c ? (size_t)(c - (alts + at)) : n - at;
        if (vcf_is_real_alt(alts + at, len)) f(alts + at, len);
        if (!c) break;
        at = (size_t)(c - alts) + 1;
    }
}

}  // namespace gtars
