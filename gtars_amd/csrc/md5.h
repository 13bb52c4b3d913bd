// md5.h -- one MD5 (RFC 1321) for the host and the device, in the style of sha512.h.  Plain header: no HIP includes; under
// hipcc every function is __host__ __device__, under a host compiler an ordinary inline function.
//
// The 16-word block is a ring of eight named 64-bit values, two little-endian message words each: md5_block's 64 steps are
// written out, so every index into the block is a compile-time constant and the block lives in registers.  Messages arrive
// eight bytes at a time -- md5_push shifts the ring by one pair, so a streaming producer needs no index of its own -- and
// md5_stream, the loop a message in memory goes through, pads by position.  The step constants are immediates.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GT_MD5_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GT_MD5_HD inline
#endif

namespace gtars {

struct Md5 {
    uint32_t h[4];  // the chaining value A B C D
    uint64_t m[8];  // the block being collected: m[0] holds words 0 (low half) and 1 once eight pairs have been pushed
};

GT_MD5_HD uint32_t md5_rotl(uint32_t x, int k) { return (x << k) | (x >> (32 - k)); }

GT_MD5_HD void md5_init(Md5 &s) {
    s.h[0] = 0x67452301u, s.h[1] = 0xefcdab89u, s.h[2] = 0x98badcfeu, s.h[3] = 0x10325476u;
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = 0; i < 8; ++i) s.m[i] = 0;
}

// appends eight message bytes (the first byte in the low byte of `pair`): the ring moves up by one
GT_MD5_HD void md5_push(Md5 &s, uint64_t pair) {
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = 0; i < 7; ++i) s.m[i] = s.m[i + 1];
    s.m[7] = pair;
}

// one compression: the chaining value h takes in a block given as eight pairs of words (a pair's first word in its low half)
GT_MD5_HD void md5_compress(uint32_t h[4], uint64_t m0, uint64_t m1, uint64_t m2, uint64_t m3, uint64_t m4, uint64_t m5, uint64_t m6,
                            uint64_t m7) {
    const uint32_t x0 = (uint32_t)m0, x1 = (uint32_t)(m0 >> 32), x2 = (uint32_t)m1, x3 = (uint32_t)(m1 >> 32);
    const uint32_t x4 = (uint32_t)m2, x5 = (uint32_t)(m2 >> 32), x6 = (uint32_t)m3, x7 = (uint32_t)(m3 >> 32);
    const uint32_t x8 = (uint32_t)m4, x9 = (uint32_t)(m4 >> 32), x10 = (uint32_t)m5, x11 = (uint32_t)(m5 >> 32);
    const uint32_t x12 = (uint32_t)m6, x13 = (uint32_t)(m6 >> 32), x14 = (uint32_t)m7, x15 = (uint32_t)(m7 >> 32);
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
#define GT_MD5_F(x, y, z) ((z) ^ ((x) & ((y) ^ (z))))
#define GT_MD5_G(x, y, z) ((y) ^ ((z) & ((x) ^ (y))))
#define GT_MD5_H(x, y, z) ((x) ^ (y) ^ (z))
#define GT_MD5_I(x, y, z) ((y) ^ ((x) | ~(z)))
#define GT_MD5_STEP(f, a, b, c, d, x, t, k) a = b + md5_rotl(a + f(b, c, d) + (x) + (t), k);
    GT_MD5_STEP(GT_MD5_F, a, b, c, d, x0, 0xd76aa478u, 7)
    GT_MD5_STEP(GT_MD5_F, d, a, b, c, x1, 0xe8c7b756u, 12)
    GT_MD5_STEP(GT_MD5_F, c, d, a, b, x2, 0x242070dbu, 17)
    GT_MD5_STEP(GT_MD5_F, b, c, d, a, x3, 0xc1bdceeeu, 22)
    GT_MD5_STEP(GT_MD5_F, a, b, c, d, x4, 0xf57c0fafu, 7)
    GT_MD5_STEP(GT_MD5_F, d, a, b, c, x5, 0x4787c62au, 12)
    GT_MD5_STEP(GT_MD5_F, c, d, a, b, x6, 0xa8304613u, 17)
    GT_MD5_STEP(GT_MD5_F, b, c, d, a, x7, 0xfd469501u, 22)
    GT_MD5_STEP(GT_MD5_F, a, b, c, d, x8, 0x698098d8u, 7)
    GT_MD5_STEP(GT_MD5_F, d, a, b, c, x9, 0x8b44f7afu, 12)
    GT_MD5_STEP(GT_MD5_F, c, d, a, b, x10, 0xffff5bb1u, 17)
    GT_MD5_STEP(GT_MD5_F, b, c, d, a, x11, 0x895cd7beu, 22)
    GT_MD5_STEP(GT_MD5_F, a, b, c, d, x12, 0x6b901122u, 7)
    GT_MD5_STEP(GT_MD5_F, d, a, b, c, x13, 0xfd987193u, 12)
    GT_MD5_STEP(GT_MD5_F, c, d, a, b, x14, 0xa679438eu, 17)
    GT_MD5_STEP(GT_MD5_F, b, c, d, a, x15, 0x49b40821u, 22)
    GT_MD5_STEP(GT_MD5_G, a, b, c, d, x1, 0xf61e2562u, 5)
    GT_MD5_STEP(GT_MD5_G, d, a, b, c, x6, 0xc040b340u, 9)
    GT_MD5_STEP(GT_MD5_G, c, d, a, b, x11, 0x265e5a51u, 14)
    GT_MD5_STEP(GT_MD5_G, b, c, d, a, x0, 0xe9b6c7aau, 20)
    GT_MD5_STEP(GT_MD5_G, a, b, c, d, x5, 0xd62f105du, 5)
    GT_MD5_STEP(GT_MD5_G, d, a, b, c, x10, 0x02441453u, 9)
    GT_MD5_STEP(GT_MD5_G, c, d, a, b, x15, 0xd8a1e681u, 14)
    GT_MD5_STEP(GT_MD5_G, b, c, d, a, x4, 0xe7d3fbc8u, 20)
    GT_MD5_STEP(GT_MD5_G, a, b, c, d, x9, 0x21e1cde6u, 5)
    GT_MD5_STEP(GT_MD5_G, d, a, b, c, x14, 0xc33707d6u, 9)
    GT_MD5_STEP(GT_MD5_G, c, d, a, b, x3, 0xf4d50d87u, 14)
    GT_MD5_STEP(GT_MD5_G, b, c, d, a, x8, 0x455a14edu, 20)
    GT_MD5_STEP(GT_MD5_G, a, b, c, d, x13, 0xa9e3e905u, 5)
    GT_MD5_STEP(GT_MD5_G, d, a, b, c, x2, 0xfcefa3f8u, 9)
    GT_MD5_STEP(GT_MD5_G, c, d, a, b, x7, 0x676f02d9u, 14)
    GT_MD5_STEP(GT_MD5_G, b, c, d, a, x12, 0x8d2a4c8au, 20)
    GT_MD5_STEP(GT_MD5_H, a, b, c, d, x5, 0xfffa3942u, 4)
    GT_MD5_STEP(GT_MD5_H, d, a, b, c, x8, 0x8771f681u, 11)
    GT_MD5_STEP(GT_MD5_H, c, d, a, b, x11, 0x6d9d6122u, 16)
    GT_MD5_STEP(GT_MD5_H, b, c, d, a, x14, 0xfde5380cu, 23)
    GT_MD5_STEP(GT_MD5_H, a, b, c, d, x1, 0xa4beea44u, 4)
    GT_MD5_STEP(GT_MD5_H, d, a, b, c, x4, 0x4bdecfa9u, 11)
    GT_MD5_STEP(GT_MD5_H, c, d, a, b, x7, 0xf6bb4b60u, 16)
    GT_MD5_STEP(GT_MD5_H, b, c, d, a, x10, 0xbebfbc70u, 23)
    GT_MD5_STEP(GT_MD5_H, a, b, c, d, x13, 0x289b7ec6u, 4)
    GT_MD5_STEP(GT_MD5_H, d, a, b, c, x0, 0xeaa127fau, 11)
    GT_MD5_STEP(GT_MD5_H, c, d, a, b, x3, 0xd4ef3085u, 16)
    GT_MD5_STEP(GT_MD5_H, b, c, d, a, x6, 0x04881d05u, 23)
    GT_MD5_STEP(GT_MD5_H, a, b, c, d, x9, 0xd9d4d039u, 4)
    GT_MD5_STEP(GT_MD5_H, d, a, b, c, x12, 0xe6db99e5u, 11)
    GT_MD5_STEP(GT_MD5_H, c, d, a, b, x15, 0x1fa27cf8u, 16)
    GT_MD5_STEP(GT_MD5_H, b, c, d, a, x2, 0xc4ac5665u, 23)
    GT_MD5_STEP(GT_MD5_I, a, b, c, d, x0, 0xf4292244u, 6)
    GT_MD5_STEP(GT_MD5_I, d, a, b, c, x7, 0x432aff97u, 10)
    GT_MD5_STEP(GT_MD5_I, c, d, a, b, x14, 0xab9423a7u, 15)
    GT_MD5_STEP(GT_MD5_I, b, c, d, a, x5, 0xfc93a039u, 21)
    GT_MD5_STEP(GT_MD5_I, a, b, c, d, x12, 0x655b59c3u, 6)
    GT_MD5_STEP(GT_MD5_I, d, a, b, c, x3, 0x8f0ccc92u, 10)
    GT_MD5_STEP(GT_MD5_I, c, d, a, b, x10, 0xffeff47du, 15)
    GT_MD5_STEP(GT_MD5_I, b, c, d, a, x1, 0x85845dd1u, 21)
    GT_MD5_STEP(GT_MD5_I, a, b, c, d, x8, 0x6fa87e4fu, 6)
    GT_MD5_STEP(GT_MD5_I, d, a, b, c, x15, 0xfe2ce6e0u, 10)
    GT_MD5_STEP(GT_MD5_I, c, d, a, b, x6, 0xa3014314u, 15)
    GT_MD5_STEP(GT_MD5_I, b, c, d, a, x13, 0x4e0811a1u, 21)
    GT_MD5_STEP(GT_MD5_I, a, b, c, d, x4, 0xf7537e82u, 6)
    GT_MD5_STEP(GT_MD5_I, d, a, b, c, x11, 0xbd3af235u, 10)
    GT_MD5_STEP(GT_MD5_I, c, d, a, b, x2, 0x2ad7d2bbu, 15)
    GT_MD5_STEP(GT_MD5_I, b, c, d, a, x9, 0xeb86d391u, 21)
#undef GT_MD5_STEP
#undef GT_MD5_F
#undef GT_MD5_G
#undef GT_MD5_H
#undef GT_MD5_I
    h[0] += a, h[1] += b, h[2] += c, h[3] += d;
}

// the chaining value takes in the sixteen words of s.m
GT_MD5_HD void md5_block(Md5 &s) { md5_compress(s.h, s.m[0], s.m[1], s.m[2], s.m[3], s.m[4], s.m[5], s.m[6], s.m[7]); }

// the number of 64-byte blocks of a message of len bytes (0x80 and the 8 length bytes included)
GT_MD5_HD uint64_t md5_blocks(uint64_t len) { return (len + 9 + 63) >> 6; }

// pair `c` (bytes 8 c .. 8 c + 7) of the padded message, given the pair `data` of the message with its bytes behind `len`
// cleared and 0x80 in place: the last pair of the last block is the bit length
GT_MD5_HD uint64_t md5_padded_pair(uint64_t data, uint64_t c, uint64_t len) { return c + 1 == 8 * md5_blocks(len) ? len << 3 : data; }

// The whole message in one loop with one compression site: `len` bytes come from src.next() in order, the padding (0x80,
// zeros, the bit length in the last 8 bytes) is generated by position.  Src: anything with `uint8_t next()`.  The digest is
// left in s.h[0 .. 3], little-endian words.  Messages stay below 2^61 bytes.
template <class Src>
GT_MD5_HD void md5_stream(Md5 &s, Src &src, uint64_t len) {
    md5_init(s);
    const uint64_t n_pairs = 8 * md5_blocks(len);
#if defined(__clang__)
#pragma unroll 1
#endif
    for (uint64_t c = 0; c < n_pairs; ++c) {
        uint64_t pair = 0;
#if defined(__clang__)
#pragma unroll 1
#endif
        for (int k = 0; k < 8; ++k) {
            const uint64_t pos = 8 * c + (uint64_t)k;
            uint8_t b = 0;
            if (pos < len) b = src.next();
            else if (pos == len) b = 0x80;
            pair |= (uint64_t)b << (8 * k);
        }
        md5_push(s, md5_padded_pair(pair, c, len));
        if ((c & 7) == 7) md5_block(s);
    }
}

// The same for a source that yields eight message bytes per call: `uint64_t pair(uint64_t c)` gives bytes [8 c, 8 c + 8),
// the first in the low byte; it is asked for c = 0, 1, ... in order and only while 8 c < len, and whatever it holds behind
// len is dropped here.  A block's eight pairs go straight to their places (constant indices: the block stays in registers).
// md5_tail_pairs goes on from a state that has taken in the first `first_block` blocks, all of them inside the message
// (64 * first_block <= len): the source is asked from pair 8 * first_block on.
template <class Src>
GT_MD5_HD void md5_tail_pairs(Md5 &s, Src &src, uint64_t len, uint64_t first_block) {
    const uint64_t n_blocks = md5_blocks(len);
#if defined(__clang__)
#pragma unroll 1
#endif
    for (uint64_t blk = first_block; blk < n_blocks; ++blk) {
#if defined(__clang__)
#pragma unroll
#endif
        for (int i = 0; i < 8; ++i) {
            const uint64_t c = (blk << 3) + (uint64_t)i, at = c << 3;
            uint64_t d = 0;
            if (at < len) {
                d = src.pair(c);
                const uint64_t rem = len - at;
                if (rem < 8) d = (d & ((1ull << (8 * rem)) - 1)) | (0x80ull << (8 * rem));
            } else if (at == len) {
                d = 0x80;
            }
            s.m[i] = md5_padded_pair(d, c, len);
        }
        md5_block(s);
    }
}
template <class Src>
GT_MD5_HD void md5_stream_pairs(Md5 &s, Src &src, uint64_t len) {
    md5_init(s);
    md5_tail_pairs(s, src, len, 0);
}

// the 16 digest bytes of a finished state
GT_MD5_HD void md5_bytes(const Md5 &s, uint8_t out[16]) {
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = 0; i < 16; ++i) out[i] = (uint8_t)(s.h[i >> 2] >> (8 * (i & 3)));
}

// the digest as two words, byte i of the digest in byte i of memory on a little-endian machine
GT_MD5_HD void md5_words(const Md5 &s, uint64_t out[2]) {
    out[0] = (uint64_t)s.h[0] | ((uint64_t)s.h[1] << 32);
    out[1] = (uint64_t)s.h[2] | ((uint64_t)s.h[3] << 32);
}

struct Md5Bytes {  // a message in memory
    const uint8_t *p;
    GT_MD5_HD uint8_t next() { return *p++; }
};

// md5 of n bytes: 16 digest bytes
GT_MD5_HD void md5(const uint8_t *p, size_t n, uint8_t out[16]) {
    Md5 s;
    Md5Bytes src{p};
    md5_stream(s, src, (uint64_t)n);
    md5_bytes(s, out);
}

// 32 lower-case hex characters of 16 digest bytes, not terminated
GT_MD5_HD void md5_hex(const uint8_t d[16], char out[32]) {
    for (int i = 0; i < 16; ++i) {
        const uint32_t hi = d[i] >> 4, lo = d[i] & 15u;
        out[2 * i] = (char)(hi < 10 ? '0' + hi : 'a' + (hi - 10));
        out[2 * i + 1] = (char)(lo < 10 ? '0' + lo : 'a' + (lo - 10));
    }
}

}  // namespace gtars
