// refget_pack_core.h -- the bit arithmetic of K22 (the encoded storage mode of a refget store:
// gtars-refget/src/digest/alphabet.rs:114-123 and 130-383, digest/encoder.rs:99-130 and 175-252) that the kernels, the
// library's host path and a stand-alone checking program share.  Plain C++17: no HIP include; under hipcc the functions
// are __host__ __device__.
//
//   * bits per symbol of an alphabet class (alphabet.rs:114-123): 2, 3, 4, 5, 8, and 8 for Unknown.
//   * the encoding tables (alphabet.rs:130-142, 158-177, 194-230, 255-304), restated as arithmetic on the upper-cased
//     byte -- every table of the reference maps both letter cases alike: 2-bit T C A G = 0 .. 3, anything else 0; 3-bit
//     A C G T N R Y = 0 .. 6, ANYTHING ELSE 7; IUPAC one bit per base (A 1, C 2, G 4, T and U 8) with N = 0, anything else 0;
//     protein the position in ACDEFGHIKLMNPQRSTVWY*X-., anything else 0; 8-bit the upper-cased byte (the reference's table
//     is the identity, its FASTA reader upper-cases: fasta.rs:123).
//   * the decoding tables (alphabet.rs:145-152, 179-189, 234-253, 306-334) as four 8-character words per class.  IUPAC is
//     no inverse pair: code 13 (D) decodes to H, 14 (H) to V, 11 to D and U comes back as T.  That is the reference's
//     behaviour and is kept.
//   * packing, MSB first (encode_sequence, encoder.rs:99-117): symbol i of a record has bits [i b, i b + b) counted from
//     the top bit of byte 0; a record of len symbols is ceil(len b / 8) bytes, the unused low bits of the last byte zero.
//     rg_pack_group packs 64 symbols into b big-endian 64-bit words, symbols at and behind the record's end as ZERO BITS
//     whatever the table says of the byte found there (the 3-bit table maps a zero byte to 7).
//   * decoding: rg_decode_window is decode_substring_from_bytes_at_offset with the zero fill of the naive decoder
//     (encoder.rs:175-203, 365-379) for a window of the encoding; RgPackedRow reads a record of a packed image (every record
//     at a 16-byte-aligned offset, at least 16 zero bytes behind it) in aligned 64-bit words.
//   * byte_range_for_bases (encoder.rs:126-130).
#pragma once

#include <cstdint>
#include <cstring>

#include "refget_core.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GT_PK_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GT_PK_HD inline
#endif

namespace gtars {

GT_PK_HD uint32_t rg_bits_of(uint32_t cls) { return cls == RG_DNA2BIT ? 2u : cls == RG_DNA3BIT ? 3u : cls == RG_DNAIO ? 4u : cls == RG_PROTEIN ? 5u : 8u; }

// bytes of `len` symbols at `bits` each
GT_PK_HD uint64_t rg_packed_bytes(uint64_t len, uint32_t bits) { return (len * bits + 7) >> 3; }

// the position of `u` in s[0 .. n), `dflt` without one
template <unsigned N>
GT_PK_HD uint8_t rg_find(const char (&s)[N], uint8_t u, uint8_t dflt) {
    for (unsigned k = 0; k + 1 < N; ++k)
        if ((uint8_t)s[k] == u) return (uint8_t)k;
    return dflt;
}

// the code of a byte in the class's table
GT_PK_HD uint8_t rg_encode_byte(uint32_t cls, uint8_t byte) {
    const uint8_t u = refget_upper(byte);
    switch (cls) {
    case RG_DNA2BIT: return rg_find("TCAG", u, 0);
    case RG_DNA3BIT: return rg_find("ACGTNRY", u, 7);
    case RG_DNAIO: return u == 'U' ? (uint8_t)8 : u == '?' ? (uint8_t)0 : rg_find("NACMGRSKTWY?BDHV", u, 0);
    case RG_PROTEIN: return rg_find("ACDEFGHIKLMNPQRSTVWY*X-.", u, 0);
    default: return u;
    }
}

// eight characters as one word, the first in the low byte
constexpr uint64_t rg_word8(const char *s) {
    uint64_t w = 0;
    for (int k = 0; k < 8; ++k) w |= (uint64_t)(unsigned char)s[k] << (8 * k);
    return w;
}

// the class's decoding table for codes 0 .. 31 as four words of eight characters (the 8-bit classes decode to the code itself
// and need none).  Selected word by word, so that the table stays in registers on the device
struct RgDecode {
    uint64_t w0, w1, w2, w3;
};
GT_PK_HD RgDecode rg_decode_table(uint32_t cls) {
    RgDecode t;
    t.w0 = cls == RG_DNA2BIT ? rg_word8("TCAGNNNN") : cls == RG_DNA3BIT ? rg_word8("ACGTNRYX") : cls == RG_DNAIO ? rg_word8("NACMGRSK")
         : cls == RG_PROTEIN ? rg_word8("ACDEFGHI") : 0;
    t.w1 = cls == RG_DNAIO ? rg_word8("TWYDBHVV") : cls == RG_PROTEIN ? rg_word8("KLMNPQRS") : 0;
    t.w2 = cls == RG_PROTEIN ? rg_word8("TVWY*X-.") : 0;
    t.w3 = cls == RG_PROTEIN ? rg_word8("XXXXXXXX") : 0;
    return t;
}
GT_PK_HD uint8_t rg_decode_code(const RgDecode &t, uint32_t bits, uint32_t code) {
    if (bits == 8) return (uint8_t)code;
    // (masks, not selects: a select between two members becomes a load at a computed address, and the table leaves the registers)
    const uint64_t m8 = 0 - (uint64_t)((code >> 3) & 1u), m16 = 0 - (uint64_t)((code >> 4) & 1u);
    const uint64_t lo = t.w0 ^ ((t.w0 ^ t.w1) & m8), hi = t.w2 ^ ((t.w2 ^ t.w3) & m8);
    return (uint8_t)((lo ^ ((lo ^ hi) & m16)) >> (8 * (code & 7u)));
}

GT_PK_HD uint64_t rg_bswap64(uint64_t x) { return __builtin_bswap64(x); }

// Symbols [64 g, 64 g + 64) of a record as B words: in[j] holds the group's raw bytes [8 j, 8 j + 8), the first in the low
// byte; only the first `valid` of them belong to the record, the others count as zero bits.  enc(byte) is the class's
// table.  put(w, word) gets word w = 0 .. B - 1 of the group in MEMORY order (its first byte in the low byte).
template <uint32_t B, class Enc, class Put>
GT_PK_HD void rg_pack_group_b(const uint64_t (&in)[8], uint32_t valid, const Enc &enc, const Put &put) {
    uint64_t acc = 0;
    uint32_t nb = 0, w = 0;  // (acc holds nb < 64 bits)
#if defined(__clang__)
#pragma unroll
#endif
    for (uint32_t j = 0; j < 8; ++j) {
#if defined(__clang__)
#pragma unroll
#endif
        for (uint32_t k = 0; k < 8; ++k) {
            const uint64_t code = 8 * j + k < valid ? (uint64_t)enc((uint8_t)(in[j] >> (8 * k))) : 0;
            if (nb + B >= 64) {
                const uint32_t take = 64 - nb;  // 1 .. B bits of the code complete the word
                put(w++, rg_bswap64((acc << take) | (code >> (B - take))));
                nb = B - take;
                acc = code & ((1ull << nb) - 1);
            } else {
                acc = (acc << B) | code;
                nb += B;
            }
        }
    }
}
template <class Enc, class Put>
GT_PK_HD void rg_pack_group(uint32_t bits, const uint64_t (&in)[8], uint32_t valid, const Enc &enc, const Put &put) {
    switch (bits) {
    case 2: rg_pack_group_b<2>(in, valid, enc, put); break;
    case 3: rg_pack_group_b<3>(in, valid, enc, put); break;
    case 4: rg_pack_group_b<4>(in, valid, enc, put); break;
    case 5: rg_pack_group_b<5>(in, valid, enc, put); break;
    default: rg_pack_group_b<8>(in, valid, enc, put); break;
    }
}

// groups [g0, g1) of a record on the host (a group: 64 symbols, 8 b bytes): out[0, ceil(len b / 8)) is the record's encoding and
// nothing behind it is written; seq has no readable byte behind len
inline void rg_encode_groups(const uint8_t *seq, uint64_t len, uint32_t cls, uint8_t *out, uint64_t g0, uint64_t g1) {
    const uint32_t bits = rg_bits_of(cls);
    const uint64_t n_bytes = rg_packed_bytes(len, bits);
    uint8_t tab[256];
    for (int b = 0; b < 256; ++b) tab[b] = rg_encode_byte(cls, (uint8_t)b);
    for (uint64_t g = g0; g < g1 && 64 * g < len; ++g) {
        const uint32_t valid = (uint32_t)(len - 64 * g < 64 ? len - 64 * g : 64);
        uint64_t in[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        memcpy(in, seq + 64 * g, valid);
        rg_pack_group(bits, in, valid, [&](uint8_t b) { return tab[b]; },
                      [&](uint32_t w, uint64_t word) {
                          const uint64_t at = 8 * ((uint64_t)bits * g + w);
                          if (at < n_bytes) memcpy(out + at, &word, (size_t)(n_bytes - at < 8 ? n_bytes - at : 8));
                      });
    }
}
inline void rg_encode_record(const uint8_t *seq, uint64_t len, uint32_t cls, uint8_t *out) { rg_encode_groups(seq, len, cls, out, 0, (len + 63) >> 6); }

// byte_range_for_bases: the bytes [*b0, *b1) of the encoding that hold symbols [start, end)
GT_PK_HD void rg_byte_range(uint64_t start, uint64_t end, uint32_t bits, uint64_t *b0, uint64_t *b1) {
    *b0 = (start * bits) >> 3;
    *b1 = (end * bits + 7) >> 3;
}

// Symbols [start, end) of an encoding of which `packed` holds bytes [byte_offset, byte_offset + n_packed); bits outside the
// window read as zero; end <= start is the empty string.  -> the characters written (out: end - start of them)
inline uint64_t rg_decode_window(const uint8_t *packed, uint64_t n_packed, uint64_t byte_offset, uint64_t start, uint64_t end, uint32_t cls,
                                 uint8_t *out) {
    if (end <= start) return 0;
    const uint32_t bits = rg_bits_of(cls);
    const RgDecode t = rg_decode_table(cls);
    auto fetch = [&](uint64_t at) -> uint32_t { return at >= byte_offset && at - byte_offset < n_packed ? packed[at - byte_offset] : 0u; };
    for (uint64_t i = start; i < end; ++i) {
        const uint64_t p = i * bits, at = p >> 3;
        const uint32_t q = (uint32_t)(p & 7), pair = (fetch(at) << 8) | (q + bits > 8 ? fetch(at + 1) : 0u);
        out[i - start] = rg_decode_code(t, bits, (pair >> (16 - q - bits)) & ((1u << bits) - 1));
    }
    return end - start;
}

// One record of a packed image, read from symbol `start` on: byte(k) is the character of symbol start + k.  The record's
// base is 8-byte aligned and the 64-bit word behind the one that holds a symbol's first bit is readable (the image keeps 16
// zero bytes behind every record).  Two words are held, so ascending k costs one pair of loads per 64 bits.
struct RgPackedRow {
    const uint64_t *base;
    uint64_t start, at, hi, lo;  // `at`: the word pair held (none: all ones)
    uint32_t bits;
    RgDecode t;
    GT_PK_HD void open(const uint64_t *record, uint32_t cls, uint64_t first) {
        base = record, start = first, at = ~0ull, hi = lo = 0;
        bits = rg_bits_of(cls);
        t = rg_decode_table(cls);
    }
    GT_PK_HD uint32_t byte(uint64_t k) {
        const uint64_t p = (start + k) * bits, word = p >> 6;
        if (word != at) {
            at = word;
            hi = rg_bswap64(base[word]), lo = rg_bswap64(base[word + 1]);
        }
        const uint32_t q = (uint32_t)(p & 63);
        const uint64_t v = q + bits <= 64 ? hi >> (64 - q - bits) : (hi << (q + bits - 64)) | (lo >> (128 - q - bits));
        return rg_decode_code(t, bits, (uint32_t)v & ((1u << bits) - 1));
    }
};

// the layout of a packed image: record r at off[r] (a multiple of 16), its bytes, 16 .. 31 zero bytes.  -> the image's bytes
inline uint64_t rg_image_layout(const uint64_t *len, const uint8_t *cls, uint64_t n, uint64_t *off, uint64_t *n_bytes) {
    uint64_t at = 0;
    for (uint64_t r = 0; r < n; ++r) {
        off[r] = at;
        n_bytes[r] = rg_packed_bytes(len[r], rg_bits_of(cls[r]));
        at = (at + n_bytes[r] + 16 + 15) & ~15ull;
    }
    return at;
}

}  // namespace gtars
