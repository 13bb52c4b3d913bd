// bam_frag_core.h -- K26: the rule that turns ONE BAM record into a fragment or into the reason it gives none (DESIGN.md §3
// K26), stated once for the device kernel (bam.hip: k_bam_frag_rows) and a stand-alone checking program
// (tests/soak/bam_frag_host_check.cpp).  Plain C++17 header in the style of bed_text_core.h: no HIP include; under hipcc the
// functions are __host__ __device__, under a host compiler ordinary inline functions.
//
// A record is given as a pointer to its block_size field.  The caller guarantees that the 4 + block_size bytes behind it are
// readable and that block_size >= 32 (the host walk, bam.cpp: bam_walk); nothing outside those bytes is read here, whatever
// the record's own length fields say.  Byte loads only: a record starts at any address.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GT_BF_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GT_BF_HD inline
#endif

namespace gtars {

// what bam_frag_rule returns: the record is a kept pair, the first reason of the rule that applies, or malformed aux data
enum : int32_t {
    BF_MALFORMED = -1,
    BF_KEPT = 0,
    BF_UNPLACED = 1,
    BF_FLAG = 2,
    BF_MAPQ = 3,
    BF_MATE_REF = 4,
    BF_NOT_LEFTMOST = 5,
    BF_TOO_LONG = 6,
    BF_NO_BARCODE = 7,
    BF_EMPTY = 8,
    BF_N_OUTCOMES = 9
};

struct BamFragParams {
    uint8_t tag[2];       // the barcode tag
    uint32_t use_tag;     // 0: no barcode is looked for (every kept pair belongs to one sample)
    uint32_t min_mapq;
    uint32_t require_flags, exclude_flags;
    int64_t max_fragment_length;
    int64_t shift_left, shift_right;
};

struct BamFragRow {
    int32_t ref;
    uint32_t start, end;
    uint32_t cb_off, cb_len;  // the barcode's bytes: offset from the record's block_size field, length without the NUL
};

GT_BF_HD uint32_t bf_ld16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
GT_BF_HD uint32_t bf_ld32(const uint8_t *p) { return bf_ld16(p) | (bf_ld16(p + 2) << 16); }

// the value bytes of an aux entry of type `type` whose value starts at body[at] (SAM specification §4.2.4), *size; false:
// the entry is malformed -- an unknown type letter, a value or a B array that reaches past `end`, a Z / H without a NUL in
// front of `end`.  Only body[at, end) is read.
GT_BF_HD bool bam_aux_value_size(const uint8_t *body, uint64_t at, uint64_t end, uint8_t type, uint64_t *size) {
    uint64_t n;
    switch (type) {
        case 'A': case 'c': case 'C': n = 1; break;
        case 's': case 'S': n = 2; break;
        case 'i': case 'I': case 'f': n = 4; break;
        case 'Z': case 'H': {
            uint64_t k = at;
            while (k < end && body[k] != 0) ++k;
            if (k >= end) return false;
            n = k - at + 1;
            break;
        }
        case 'B': {
            if (end - at < 5) return false;
            const uint8_t sub = body[at];
            uint64_t each;
            if (sub == 'c' || sub == 'C') each = 1;
            else if (sub == 's' || sub == 'S') each = 2;
            else if (sub == 'i' || sub == 'I' || sub == 'f') each = 4;
            else return false;
            n = 5 + (uint64_t)bf_ld32(body + at + 1) * each;  // (at most 5 + 4 * (2^32 - 1): no overflow)
            break;
        }
        default: return false;
    }
    if (n > end - at) return false;
    *size = n;
    return true;
}

// Step 7 of the rule: the entries of body[aux, end) in file order; the first whose tag is `tag` decides.  BF_KEPT: its type
// is Z and its value is not empty, body[*off, *off + *len) is the value.  BF_NO_BARCODE: another type, an empty value, or
// no such entry.  BF_MALFORMED: an entry up to and including that one is malformed, or aux > end.
GT_BF_HD int32_t bam_aux_find(const uint8_t *body, uint64_t aux, uint64_t end, const uint8_t tag[2], uint64_t *off, uint32_t *len) {
    if (aux > end) return BF_MALFORMED;
    uint64_t at = aux;
    while (at < end) {
        if (end - at < 3) return BF_MALFORMED;
        const uint8_t t0 = body[at], t1 = body[at + 1], type = body[at + 2];
        uint64_t size;
        if (!bam_aux_value_size(body, at + 3, end, type, &size)) return BF_MALFORMED;
        if (t0 == tag[0] && t1 == tag[1]) {
            if (type != 'Z' || size <= 1) return BF_NO_BARCODE;
            *off = at + 3, *len = (uint32_t)(size - 1);
            return BF_KEPT;
        }
        at += 3 + size;
    }
    return BF_NO_BARCODE;
}

// The rule for one record (ISSUE K26 §1), tested in its order: the first reason that applies is returned.
// rec: the record's block_size field.  ref_len[n_ref]: the header's reference lengths.  BF_KEPT fills *row.
GT_BF_HD int32_t bam_frag_rule(const uint8_t *rec, const BamFragParams &p, const uint32_t *ref_len, uint32_t n_ref, BamFragRow *row) {
    const uint64_t bs = bf_ld32(rec);
    const uint8_t *body = rec + 4;
    const int32_t ref = (int32_t)bf_ld32(body);
    if (ref < 0) return BF_UNPLACED;
    const uint32_t flag = bf_ld16(body + 14);
    if ((flag & p.require_flags) != p.require_flags || (flag & p.exclude_flags)) return BF_FLAG;
    if ((uint32_t)body[9] < p.min_mapq) return BF_MAPQ;
    if ((int32_t)bf_ld32(body + 20) != ref) return BF_MATE_REF;
    const int64_t tlen = (int32_t)bf_ld32(body + 28);
    if (tlen <= 0) return BF_NOT_LEFTMOST;
    if (tlen > p.max_fragment_length) return BF_TOO_LONG;
    uint64_t cb_off = 0;
    uint32_t cb_len = 0;
    if (p.use_tag) {
        const uint64_t l_seq = bf_ld32(body + 16);
        const uint64_t aux = 32ull + body[8] + 4ull * bf_ld16(body + 12) + (l_seq + 1) / 2 + l_seq;
        const int32_t r = bam_aux_find(body, aux, bs, p.tag, &cb_off, &cb_len);
        if (r != BF_KEPT) return r;
    }
    if ((uint32_t)ref >= n_ref) return BF_MALFORMED;  // (the walk has refused such a file already)
    const int64_t pos = (int32_t)bf_ld32(body + 4);
    int64_t start = pos + p.shift_left, end = pos + tlen + p.shift_right;
    if (start < 0) start = 0;
    if (end > (int64_t)ref_len[ref]) end = (int64_t)ref_len[ref];
    if (start >= end) return BF_EMPTY;
    row->ref = ref, row->start = (uint32_t)start, row->end = (uint32_t)end;
    row->cb_off = (uint32_t)(4 + cb_off), row->cb_len = cb_len;
    return BF_KEPT;
}

}  // namespace gtars
