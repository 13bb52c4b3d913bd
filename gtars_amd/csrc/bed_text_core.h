// bed_text_core.h -- the text of a region set, stated once for the host paths (bed_text.cpp), the device kernels (K25,
// bed_text.hip) and a stand-alone checking program.  Plain C++17 header in the style of refget_core.h: no HIP include; under
// hipcc every function is __host__ __device__, under a host compiler an ordinary inline function.
//
// A set has four streams of bytes, each the concatenation of one piece per row (gtars-core/src/models/region_set.rs:282-306,
// region.rs:30-40):
//     CHR    the chromosome names joined by ','          START  the decimal starts joined by ','
//     END    the decimal ends joined by ','              LINE   chr \t start \t end [\t rest] \n  -- the BED text
// A row's piece carries its separator: a comma unless the row is the last of its set, '\n' always for LINE.  The bed digest
// ("identifier") is the MD5 of hex(md5 CHR) , hex(md5 START) , hex(md5 END); the file digest the MD5 of LINE.
#pragma once

#include <cstddef>
#include <cstdint>

#include "md5.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GT_BT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GT_BT_HD inline
#endif

namespace gtars {

enum : uint32_t { BED_CHR = 0, BED_START = 1, BED_END = 2, BED_LINE = 3 };

// the decimal digits of v: 1 .. 10
GT_BT_HD uint32_t bed_u32_width(uint32_t v) {
    uint32_t w = 1;
    if (v >= 10u) w = 2;
    if (v >= 100u) w = 3;
    if (v >= 1000u) w = 4;
    if (v >= 10000u) w = 5;
    if (v >= 100000u) w = 6;
    if (v >= 1000000u) w = 7;
    if (v >= 10000000u) w = 8;
    if (v >= 100000000u) w = 9;
    if (v >= 1000000000u) w = 10;
    return w;
}

// character k (0: the most significant) of the w = bed_u32_width(v) digits of v
GT_BT_HD uint8_t bed_u32_digit(uint32_t v, uint32_t w, uint32_t k) {
    for (uint32_t drop = w - 1 - k; drop; --drop) v /= 10u;
    return (uint8_t)('0' + v % 10u);
}

// one row as the streams see it; `last`: the last row of its set
struct BedRow {
    const uint8_t *name;
    const uint8_t *rest;
    uint32_t name_len, rest_len;  // (rest_len counts only when has_rest)
    uint32_t start, end;
    bool has_rest, last;
};

// the bytes of the row's piece of a stream, separator included
GT_BT_HD uint32_t bed_row_bytes(uint32_t kind, const BedRow &r) {
    const uint32_t sep = r.last ? 0u : 1u;
    if (kind == BED_CHR) return r.name_len + sep;
    if (kind == BED_START) return bed_u32_width(r.start) + sep;
    if (kind == BED_END) return bed_u32_width(r.end) + sep;
    return r.name_len + 1 + bed_u32_width(r.start) + 1 + bed_u32_width(r.end) + (r.has_rest ? 1 + r.rest_len : 0u) + 1;
}

// byte k < bed_row_bytes(kind, r) of that piece
GT_BT_HD uint8_t bed_row_byte(uint32_t kind, const BedRow &r, uint32_t k) {
    if (kind == BED_CHR) return k < r.name_len ? r.name[k] : (uint8_t)',';
    if (kind == BED_START || kind == BED_END) {
        const uint32_t v = kind == BED_START ? r.start : r.end, w = bed_u32_width(v);
        return k < w ? bed_u32_digit(v, w, k) : (uint8_t)',';
    }
    if (k < r.name_len) return r.name[k];
    k -= r.name_len;
    if (k == 0) return (uint8_t)'\t';
    k -= 1;
    const uint32_t ws = bed_u32_width(r.start);
    if (k < ws) return bed_u32_digit(r.start, ws, k);
    k -= ws;
    if (k == 0) return (uint8_t)'\t';
    k -= 1;
    const uint32_t we = bed_u32_width(r.end);
    if (k < we) return bed_u32_digit(r.end, we, k);
    k -= we;
    if (r.has_rest) {
        if (k == 0) return (uint8_t)'\t';
        k -= 1;
        if (k < r.rest_len) return r.rest[k];
    }
    return (uint8_t)'\n';
}

// The piece written out whole, for hosts that format rows into a buffer: dst receives bed_row_bytes(kind, r) bytes, the same
// ones bed_row_byte gives one at a time (the checking program compares the two at every digit-count edge).
GT_BT_HD uint32_t bed_u32_write(uint32_t v, uint8_t *dst) {
    const uint32_t w = bed_u32_width(v);
    for (uint32_t k = w; k--; v /= 10u) dst[k] = (uint8_t)('0' + v % 10u);
    return w;
}
GT_BT_HD uint32_t bed_bytes_write(const uint8_t *src, uint32_t n, uint8_t *dst) {
    for (uint32_t k = 0; k < n; ++k) dst[k] = src[k];
    return n;
}
GT_BT_HD uint32_t bed_row_write(uint32_t kind, const BedRow &r, uint8_t *dst) {
    uint8_t *p = dst;
    if (kind == BED_CHR) p += bed_bytes_write(r.name, r.name_len, p);
    else if (kind == BED_START) p += bed_u32_write(r.start, p);
    else if (kind == BED_END) p += bed_u32_write(r.end, p);
    if (kind != BED_LINE) {
        if (!r.last) *p++ = (uint8_t)',';
        return (uint32_t)(p - dst);
    }
    p += bed_bytes_write(r.name, r.name_len, p);
    *p++ = (uint8_t)'\t';
    p += bed_u32_write(r.start, p);
    *p++ = (uint8_t)'\t';
    p += bed_u32_write(r.end, p);
    if (r.has_rest) {
        *p++ = (uint8_t)'\t';
        p += bed_bytes_write(r.rest, r.rest_len, p);
    }
    *p++ = (uint8_t)'\n';
    return (uint32_t)(p - dst);
}

// the 98 bytes hex(c) , hex(s) , hex(e) of the identifier's message as a byte source of md5_stream: d = the three stream
// digests in md5_words form, six words
struct BedIdSrc {
    const uint64_t *d;
    uint32_t at;
    GT_BT_HD uint8_t next() {
        const uint32_t j = at / 33u, r = at % 33u;
        ++at;
        if (r == 32u) return (uint8_t)',';
        const uint32_t b = r >> 1;
        const uint32_t byte = (uint32_t)(d[2 * j + (b >> 3)] >> (8 * (b & 7u))) & 0xFFu;
        const uint32_t nib = (r & 1u) ? byte & 15u : byte >> 4;
        return (uint8_t)(nib < 10 ? '0' + nib : 'a' + (nib - 10));
    }
};
constexpr uint64_t BED_ID_MESSAGE_BYTES = 98;

// out[0 .. 1]: the identifier (md5_words form) of the three stream digests at d[0 .. 5]
GT_BT_HD void bed_identifier(const uint64_t *d, uint64_t out[2]) {
    Md5 s;
    BedIdSrc src{d, 0};
    md5_stream(s, src, BED_ID_MESSAGE_BYTES);
    md5_words(s, out);
}

}  // namespace gtars
