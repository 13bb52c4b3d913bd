// refget_pack_check.cpp -- refget_pack_core.h under the sanitizers, as a stand-alone program (tests/test_refget_store_cpu.py
// builds it with -fsanitize=address,undefined):
//   refget_pack_check [max_len]
// For every alphabet class and every length 0 .. max_len (300): a random sequence (both letter cases, bytes outside every
// table) in a heap block of exactly its size is encoded into a block of exactly ceil(len b / 8) bytes and compared with a
// bit-by-bit loop; then every [start, end) with end - start <= 17 is decoded three ways -- from the whole encoding, from a
// block that holds exactly byte_range_for_bases of it, and by RgPackedRow from an image block of the record's bytes plus its
// 16 .. 31 zero bytes -- against a loop over the naive codes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../gtars_amd/csrc/refget_pack_core.h"

using namespace gtars;

static int fails = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            if (++fails < 20) {           \
                fprintf(stderr, __VA_ARGS__); \
                fprintf(stderr, "\n");    \
            }                             \
        }                                 \
    } while (0)

static uint64_t rng_state = 0x2200;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

// the tables written out, independent of the header's arithmetic
static int naive_code(int cls, uint8_t b) {
    const uint8_t u = b >= 'a' && b <= 'z' ? b - 32 : b;
    auto pos = [&](const char *s) -> int {
        const char *p = u ? strchr(s, u) : nullptr;
        return p ? (int)(p - s) : -1;
    };
    switch (cls) {
    case 0: return pos("TCAG") < 0 ? 0 : pos("TCAG");
    case 1: return pos("ACGTNRY") < 0 ? 7 : pos("ACGTNRY");
    case 2: {
        const char *k = "ACGTURYSWKMBDHVN";
        const int v[] = {1, 2, 4, 8, 8, 5, 10, 6, 9, 7, 3, 12, 13, 14, 15, 0};
        return pos(k) < 0 ? 0 : v[pos(k)];
    }
    case 3: return pos("ACDEFGHIKLMNPQRSTVWY*X-.") < 0 ? 0 : pos("ACDEFGHIKLMNPQRSTVWY*X-.");
    default: return u;
    }
}
static uint8_t naive_char(int cls, int code) {
    switch (cls) {
    case 0: return (uint8_t)"TCAG"[code];
    case 1: return (uint8_t)"ACGTNRYX"[code];
    case 2: return (uint8_t)"NACMGRSKTWYDBHVV"[code];
    case 3: return code < 24 ? (uint8_t)"ACDEFGHIKLMNPQRSTVWY*X-."[code] : (uint8_t)'X';
    default: return (uint8_t)code;
    }
}

int main(int argc, char **argv) {
    const size_t max_len = argc > 1 ? (size_t)atol(argv[1]) : 300;
    const std::string letters = std::string("ACGTacgtNnRYryUuSWKMBDHVswkmbdhvEFILPQXefilpqx*-.Zz7 ") + '\0' + "\xc3\xa9\xff";
    size_t n_records = 0, n_ranges = 0;
    for (int cls = 0; cls < 6; ++cls) {
        const uint32_t bits = rg_bits_of((uint32_t)cls);
        CHECK(bits == (cls == 0 ? 2u : cls == 1 ? 3u : cls == 2 ? 4u : cls == 3 ? 5u : 8u), "class %d: %u bits", cls, bits);
        for (int b = 0; b < 256; ++b)
            CHECK(rg_encode_byte((uint32_t)cls, (uint8_t)b) == naive_code(cls, (uint8_t)b), "class %d byte %d: code %d", cls, b,
                  rg_encode_byte((uint32_t)cls, (uint8_t)b));
        const RgDecode t = rg_decode_table((uint32_t)cls);
        for (int code = 0; code < (1 << bits); ++code)
            CHECK(rg_decode_code(t, bits, (uint32_t)code) == naive_char(cls, code), "class %d code %d decodes to %d", cls, code,
                  rg_decode_code(t, bits, (uint32_t)code));
        for (size_t len = 0; len <= max_len; ++len, ++n_records) {
            uint8_t *seq = (uint8_t *)malloc(len ? len : 1);  // (exactly sized: nothing readable behind the sequence)
            for (size_t i = 0; i < len; ++i) seq[i] = (uint8_t)letters[rnd() % letters.size()];
            const size_t n_bytes = (size_t)rg_packed_bytes(len, bits);
            CHECK(n_bytes == (len * bits + 7) / 8, "class %d length %zu: %zu bytes", cls, len, n_bytes);
            uint8_t *enc = (uint8_t *)malloc(n_bytes ? n_bytes : 1);
            memset(enc, 0xAA, n_bytes);
            rg_encode_record(seq, len, (uint32_t)cls, enc);
            std::vector<uint8_t> want(n_bytes, 0);
            std::vector<int> codes(len);
            for (size_t i = 0; i < len; ++i) {
                codes[i] = naive_code(cls, seq[i]);
                for (uint32_t j = 0; j < bits; ++j) {
                    const size_t bit = i * bits + j;
                    want[bit >> 3] |= (uint8_t)(((codes[i] >> (bits - 1 - j)) & 1) << (7 - (bit & 7)));
                }
            }
            CHECK(!n_bytes || memcmp(enc, want.data(), n_bytes) == 0, "class %d length %zu: the encoding differs", cls, len);
            // the record as a packed image holds it
            const size_t span = (n_bytes + 16 + 15) & ~(size_t)15;
            uint64_t *image = (uint64_t *)aligned_alloc(16, span);
            memset(image, 0, span);
            memcpy(image, enc, n_bytes);
            uint8_t out[17], got[17];
            for (size_t start = 0; start <= len; ++start) {
                for (size_t end = start; end <= len && end - start <= 17; ++end, ++n_ranges) {
                    const size_t w = end - start;
                    for (size_t k = 0; k < w; ++k) out[k] = naive_char(cls, codes[start + k]);
                    CHECK(rg_decode_window(enc, n_bytes, 0, start, end, (uint32_t)cls, got) == w && memcmp(got, out, w) == 0,
                          "class %d length %zu [%zu, %zu): decode from the whole encoding", cls, len, start, end);
                    uint64_t b0, b1;
                    rg_byte_range(start, end, bits, &b0, &b1);
                    CHECK(b0 == start * bits / 8 && b1 == (end * bits + 7) / 8 && b1 <= n_bytes, "class %d [%zu, %zu): byte range", cls, start, end);
                    if (w) {
                        uint8_t *window = (uint8_t *)malloc((size_t)(b1 - b0));  // (exactly the bytes the range needs)
                        memcpy(window, enc + b0, (size_t)(b1 - b0));
                        CHECK(rg_decode_window(window, b1 - b0, b0, start, end, (uint32_t)cls, got) == w && memcmp(got, out, w) == 0,
                              "class %d length %zu [%zu, %zu): decode from its byte range", cls, len, start, end);
                        free(window);
                        RgPackedRow row;
                        row.open(image, (uint32_t)cls, start);
                        for (size_t k = 0; k < w; ++k) got[k] = (uint8_t)row.byte(k);
                        CHECK(memcmp(got, out, w) == 0, "class %d length %zu [%zu, %zu): RgPackedRow", cls, len, start, end);
                    }
                }
            }
            CHECK(rg_decode_window(enc, n_bytes, 0, 3, 3, (uint32_t)cls, got) == 0 && rg_decode_window(enc, n_bytes, 0, 5, 2, (uint32_t)cls, got) == 0,
                  "end <= start is the empty string");
            free(image), free(enc), free(seq);
        }
    }
    // the known answers
    uint8_t k2[1], k3[3];
    rg_encode_record((const uint8_t *)"ACGT", 4, RG_DNA2BIT, k2);
    CHECK(k2[0] == 0x9C, "ACGT at 2 bits: %02x", k2[0]);
    rg_encode_record((const uint8_t *)"ACGTNRYX", 8, RG_DNA3BIT, k3);
    CHECK(k3[0] == 0x05 && k3[1] == 0x39 && k3[2] == 0x77, "ACGTNRYX at 3 bits: %02x %02x %02x", k3[0], k3[1], k3[2]);
    if (fails) return 1;
    printf("ok: %zu records, %zu ranges\n", n_records, n_ranges);
    return 0;
}
