// sha512.h -- one SHA-512 (FIPS 180-4) for the host and the device, and the GA4GH digest text on top of it: sha512t24u =
// the first 24 digest bytes in base64url without padding, 32 characters (gtars-vrs/src/digest.rs:89-96).  Plain header: no
// HIP includes; under hipcc every function is __host__ __device__, under a host compiler an ordinary inline function.
//
// The 16-word message schedule is a ring of sixteen named 64-bit values: sha512_block's rounds are unrolled in groups of
// sixteen, so every index into the ring is a compile-time constant and the ring lives in registers (a runtime-indexed W[]
// would go to scratch on the device).  Messages arrive a big-endian word at a time -- sha512_push shifts the ring by one word,
// so a streaming producer needs no index of its own -- and sha512_stream, the one loop every message goes through, pads by
// position.  Only the round constants are read from memory.  The issue's sha512_final is that loop's last block.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GT_SHA_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GT_SHA_HD inline
#endif

namespace gtars {

struct Sha512 {
    uint64_t h[8];   // the chaining value
    uint64_t w[16];  // the block being collected: w[0] is its first word once sixteen have been pushed
};

GT_SHA_HD uint64_t sha512_rotr(uint64_t x, int k) { return (x >> k) | (x << (64 - k)); }

GT_SHA_HD void sha512_init(Sha512 &s) {
    s.h[0] = 0x6a09e667f3bcc908ull, s.h[1] = 0xbb67ae8584caa73bull, s.h[2] = 0x3c6ef372fe94f82bull, s.h[3] = 0xa54ff53a5f1d36f1ull;
    s.h[4] = 0x510e527fade682d1ull, s.h[5] = 0x9b05688c2b3e6c1full, s.h[6] = 0x1f83d9abfb41bd6bull, s.h[7] = 0x5be0cd19137e2179ull;
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = 0; i < 16; ++i) s.w[i] = 0;
}

#define GT_SHA_ROUND(a, b, c, d, e, f, g, h, k, w)                                                                  \
    {                                                                                                               \
        const uint64_t t1 = h + (sha512_rotr(e, 14) ^ sha512_rotr(e, 18) ^ sha512_rotr(e, 41)) + ((e & f) ^ (~e & g)) + (k) + (w); \
        const uint64_t t2 = (sha512_rotr(a, 28) ^ sha512_rotr(a, 34) ^ sha512_rotr(a, 39)) + ((a & b) ^ (a & c) ^ (b & c));        \
        d += t1;                                                                                                    \
        h = t1 + t2;                                                                                                \
    }

// one compression: the chaining value takes in the sixteen words of s.w (which are used up)
GT_SHA_HD void sha512_block(Sha512 &s) {
    const uint64_t K[80] = {
        0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull,
        0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull,
        0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull, 0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull,
        0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
        0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull, 0x983e5152ee66dfabull,
        0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
        0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull,
        0x53380d139d95b3dfull, 0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
        0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull,
        0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull, 0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull,
        0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull,
        0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
        0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull,
        0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull,
        0x113f9804bef90daeull, 0x1b710b35131c471bull, 0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull,
        0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
    uint64_t a = s.h[0], b = s.h[1], c = s.h[2], d = s.h[3], e = s.h[4], f = s.h[5], g = s.h[6], h = s.h[7];
    uint64_t w0 = s.w[0], w1 = s.w[1], w2 = s.w[2], w3 = s.w[3], w4 = s.w[4], w5 = s.w[5], w6 = s.w[6], w7 = s.w[7];
    uint64_t w8 = s.w[8], w9 = s.w[9], w10 = s.w[10], w11 = s.w[11], w12 = s.w[12], w13 = s.w[13], w14 = s.w[14], w15 = s.w[15];
#define GT_SHA_S0(x) (sha512_rotr(x, 1) ^ sha512_rotr(x, 8) ^ ((x) >> 7))
#define GT_SHA_S1(x) (sha512_rotr(x, 19) ^ sha512_rotr(x, 61) ^ ((x) >> 6))
#define GT_SHA_16(k)                                   \
    GT_SHA_ROUND(a, b, c, d, e, f, g, h, (k)[0], w0)   \
    GT_SHA_ROUND(h, a, b, c, d, e, f, g, (k)[1], w1)   \
    GT_SHA_ROUND(g, h, a, b, c, d, e, f, (k)[2], w2)   \
    GT_SHA_ROUND(f, g, h, a, b, c, d, e, (k)[3], w3)   \
    GT_SHA_ROUND(e, f, g, h, a, b, c, d, (k)[4], w4)   \
    GT_SHA_ROUND(d, e, f, g, h, a, b, c, (k)[5], w5)   \
    GT_SHA_ROUND(c, d, e, f, g, h, a, b, (k)[6], w6)   \
    GT_SHA_ROUND(b, c, d, e, f, g, h, a, (k)[7], w7)   \
    GT_SHA_ROUND(a, b, c, d, e, f, g, h, (k)[8], w8)   \
    GT_SHA_ROUND(h, a, b, c, d, e, f, g, (k)[9], w9)   \
    GT_SHA_ROUND(g, h, a, b, c, d, e, f, (k)[10], w10) \
    GT_SHA_ROUND(f, g, h, a, b, c, d, e, (k)[11], w11) \
    GT_SHA_ROUND(e, f, g, h, a, b, c, d, (k)[12], w12) \
    GT_SHA_ROUND(d, e, f, g, h, a, b, c, (k)[13], w13) \
    GT_SHA_ROUND(c, d, e, f, g, h, a, b, (k)[14], w14) \
    GT_SHA_ROUND(b, c, d, e, f, g, h, a, (k)[15], w15)
    GT_SHA_16(K)
#if defined(__clang__)
#pragma unroll 1
#endif
    for (int j = 16; j < 80; j += 16) {
        w0 += GT_SHA_S1(w14) + w9 + GT_SHA_S0(w1);
        w1 += GT_SHA_S1(w15) + w10 + GT_SHA_S0(w2);
        w2 += GT_SHA_S1(w0) + w11 + GT_SHA_S0(w3);
        w3 += GT_SHA_S1(w1) + w12 + GT_SHA_S0(w4);
        w4 += GT_SHA_S1(w2) + w13 + GT_SHA_S0(w5);
        w5 += GT_SHA_S1(w3) + w14 + GT_SHA_S0(w6);
        w6 += GT_SHA_S1(w4) + w15 + GT_SHA_S0(w7);
        w7 += GT_SHA_S1(w5) + w0 + GT_SHA_S0(w8);
        w8 += GT_SHA_S1(w6) + w1 + GT_SHA_S0(w9);
        w9 += GT_SHA_S1(w7) + w2 + GT_SHA_S0(w10);
        w10 += GT_SHA_S1(w8) + w3 + GT_SHA_S0(w11);
        w11 += GT_SHA_S1(w9) + w4 + GT_SHA_S0(w12);
        w12 += GT_SHA_S1(w10) + w5 + GT_SHA_S0(w13);
        w13 += GT_SHA_S1(w11) + w6 + GT_SHA_S0(w14);
        w14 += GT_SHA_S1(w12) + w7 + GT_SHA_S0(w15);
        w15 += GT_SHA_S1(w13) + w8 + GT_SHA_S0(w0);
        GT_SHA_16(K + j)
    }
#undef GT_SHA_16
#undef GT_SHA_S0
#undef GT_SHA_S1
    s.h[0] += a, s.h[1] += b, s.h[2] += c, s.h[3] += d, s.h[4] += e, s.h[5] += f, s.h[6] += g, s.h[7] += h;
}
#undef GT_SHA_ROUND

// appends one big-endian word to the block: the ring moves up by one (register moves, no index)
GT_SHA_HD void sha512_push(Sha512 &s, uint64_t word) {
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = 0; i < 15; ++i) s.w[i] = s.w[i + 1];
    s.w[15] = word;
}

// The whole message in one loop with ONE compression site: `len` bytes come from src.next() in order, the padding (0x80, zeros,
// the bit length in the last 16 bytes) is generated by position.  Src: anything with `uint8_t next()`.  The digest is left in
// s.h[0 .. 7], big-endian words.  Messages stay below 2^61 bytes.
template <class Src>
GT_SHA_HD void sha512_stream(Sha512 &s, Src &src, uint64_t len) {
    sha512_init(s);
    const uint64_t n_blocks = (len + 17 + 127) >> 7;
#if defined(__clang__)
#pragma unroll 1
#endif
    for (uint64_t blk = 0; blk < n_blocks; ++blk) {
#if defined(__clang__)
#pragma unroll 1
#endif
        for (int wi = 0; wi < 16; ++wi) {
            uint64_t word = 0;
            const uint64_t at = (blk << 7) + 8 * (uint64_t)wi;
#if defined(__clang__)
#pragma unroll 1
#endif
            for (int k = 0; k < 8; ++k) {
                const uint64_t pos = at + (uint64_t)k;
                uint8_t b = 0;
                if (pos < len) b = src.next();
                else if (pos == len) b = 0x80;
                word = (word << 8) | b;
            }
            if (blk + 1 == n_blocks && wi == 15) word = len << 3;
            sha512_push(s, word);
        }
        sha512_block(s);
    }
}

struct Sha512Bytes {  // a message in memory
    const uint8_t *p;
    GT_SHA_HD uint8_t next() { return *p++; }
};

// base64url character of a 6-bit value
GT_SHA_HD char sha512_b64(uint32_t v) {
    return (char)(v < 26 ? 'A' + v : v < 52 ? 'a' + (v - 26) : v < 62 ? '0' + (v - 52) : v == 62 ? '-' : '_');
}

// the 32 characters of a finished state as four words of 8 characters, the first character in the top byte -- the form the
// device keeps a digest in between the two messages of an allele
GT_SHA_HD void sha512t24u_words(const Sha512 &s, uint64_t out[4]) {
    // 24 bytes = three state words = 192 bits = 32 groups of 6: word q of the text covers bits [48 q, 48 q + 48)
#if defined(__clang__)
#pragma unroll
#endif
    for (int q = 0; q < 4; ++q) {
        // 48 bits starting at bit 48 q of h[0] h[1] h[2]
        uint64_t bits48;
        if (q == 0) bits48 = s.h[0] >> 16;
        else if (q == 1) bits48 = ((s.h[0] & 0xFFFFull) << 32) | (s.h[1] >> 32);
        else if (q == 2) bits48 = ((s.h[1] & 0xFFFFFFFFull) << 16) | (s.h[2] >> 48);
        else bits48 = s.h[2] & 0xFFFFFFFFFFFFull;
        uint64_t text = 0;
#if defined(__clang__)
#pragma unroll
#endif
        for (int k = 0; k < 8; ++k) text = (text << 8) | (uint8_t)sha512_b64((uint32_t)(bits48 >> (42 - 6 * k)) & 63u);
        out[q] = text;
    }
}

GT_SHA_HD void sha512t24u_text(const Sha512 &s, char out[32]) {
    uint64_t t[4];
    sha512t24u_words(s, t);
#if defined(__clang__)
#pragma unroll
#endif
    for (int q = 0; q < 4; ++q)
        for (int k = 0; k < 8; ++k) out[8 * q + k] = (char)(t[q] >> (56 - 8 * k));
}

// sha512t24u of n bytes: 32 characters, not terminated
GT_SHA_HD void sha512t24u(const uint8_t *p, size_t n, char out[32]) {
    Sha512 s;
    Sha512Bytes src{p};
    sha512_stream(s, src, (uint64_t)n);
    sha512t24u_text(s, out);
}

}  // namespace gtars
