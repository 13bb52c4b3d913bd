// bed_text_host_check.cpp -- bed_text_core.h and md5_stream_pairs of md5.h under the sanitizers, as a stand-alone program
// (tests/test_regionset_digest_cpu.py builds it with -fsanitize=address,undefined and writes its input):
//   bed_text_host_check rows.tsv identifier file_digest
// rows.tsv: one row per line, chr \t start \t end [\t rest], in set order; the two digests are the restatement's answers.
//   * bed_u32_width / bed_u32_digit / bed_u32_write against snprintf at every digit-count edge and around it;
//   * for every row and stream kind, bed_row_byte byte by byte against bed_row_write into a block of exactly
//     bed_row_bytes bytes, with the row as the last of its set and not;
//   * md5_stream_pairs against md5_stream on every message length from 0 to 300, the message in an exactly sized block;
//   * the four streams of the rows, each in an exactly sized block, hashed both ways; the identifier and the file digest
//     against the expected ones.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../gtars_amd/csrc/bed_text_core.h"

using namespace gtars;

static int fails = 0;
#define CHECK(cond, ...)                   \
    do {                                   \
        if (!(cond)) {                     \
            ++fails;                       \
            fprintf(stderr, __VA_ARGS__);  \
            fprintf(stderr, "\n");         \
        }                                  \
    } while (0)

struct Row {
    std::string chr, rest;
    uint32_t start, end;
    bool has_rest;
};

static BedRow view(const Row &r, bool last) {
    BedRow b;
    b.name = (const uint8_t *)r.chr.data(), b.name_len = (uint32_t)r.chr.size();
    b.rest = (const uint8_t *)r.rest.data(), b.rest_len = (uint32_t)r.rest.size();
    b.start = r.start, b.end = r.end, b.has_rest = r.has_rest, b.last = last;
    return b;
}

// a source of md5_stream_pairs over a block of exactly len bytes: never reads behind it
struct BlockPairs {
    const uint8_t *p;
    uint64_t len;
    uint64_t pair(uint64_t c) const {
        uint64_t v = 0;
        memcpy(&v, p + 8 * c, (size_t)(len - 8 * c < 8 ? len - 8 * c : 8));
        return v;
    }
};

static std::string hex(const Md5 &s) {
    uint8_t d[16];
    char out[33];
    md5_bytes(s, d);
    md5_hex(d, out);
    out[32] = '\0';
    return out;
}

// both loops of md5.h over a message in an exactly sized heap block; returns the words
static void hash_block(const std::vector<uint8_t> &msg, uint64_t words[2], const char *what) {
    const size_t n = msg.size();
    uint8_t *block = (uint8_t *)malloc(n ? n : 1);
    if (n) memcpy(block, msg.data(), n);
    Md5 a, b;
    Md5Bytes bytes{block};
    md5_stream(a, bytes, n);
    BlockPairs pairs{block, n};
    md5_stream_pairs(b, pairs, n);
    CHECK(hex(a) == hex(b), "%s: md5_stream_pairs %s != md5_stream %s at %zu bytes", what, hex(b).c_str(), hex(a).c_str(), n);
    // the split the kernel makes: the blocks wholly inside the message taken in directly, the rest by md5_tail_pairs
    Md5 c;
    md5_init(c);
    const uint64_t full = n >> 6;
    for (uint64_t blk = 0; blk < full; ++blk) {
        memcpy(c.m, block + 64 * blk, 64);
        md5_block(c);
    }
    md5_tail_pairs(c, pairs, n, full);
    CHECK(hex(a) == hex(c), "%s: whole blocks + md5_tail_pairs %s != md5_stream %s at %zu bytes", what, hex(c).c_str(), hex(a).c_str(), n);
    md5_words(b, words);
    free(block);
}

int main(int argc, char **argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: bed_text_host_check rows.tsv identifier file_digest\n");
        return 2;
    }
    // digits
    const uint64_t edges[] = {0, 1, 9, 10, 11, 99, 100, 101, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000,
                              99999999, 100000000, 999999999, 1000000000, 1000000001, 4294967294ull, 4294967295ull};
    for (uint64_t e : edges) {
        const uint32_t v = (uint32_t)e;
        char want[16];
        const int w = snprintf(want, sizeof want, "%u", v);
        CHECK((int)bed_u32_width(v) == w, "width of %u: %u", v, bed_u32_width(v));
        uint8_t *got = (uint8_t *)malloc((size_t)w);
        CHECK((int)bed_u32_write(v, got) == w && !memcmp(got, want, (size_t)w), "bed_u32_write of %u", v);
        for (int k = 0; k < w; ++k) CHECK(bed_u32_digit(v, (uint32_t)w, (uint32_t)k) == (uint8_t)want[k], "digit %d of %u", k, v);
        free(got);
    }
    // padding edges of the pair loop
    for (size_t n = 0; n <= 300; ++n) {
        std::vector<uint8_t> msg(n);
        for (size_t i = 0; i < n; ++i) msg[i] = (uint8_t)(i * 131 + n);
        uint64_t w[2];
        hash_block(msg, w, "message");
    }
    // the rows
    std::vector<Row> rows;
    {
        std::ifstream f(argv[1], std::ios::binary);
        std::string ln;
        while (std::getline(f, ln)) {
            Row r;
            const size_t t1 = ln.find('\t'), t2 = ln.find('\t', t1 + 1), t3 = ln.find('\t', t2 + 1);
            r.chr = ln.substr(0, t1);
            r.start = (uint32_t)strtoull(ln.substr(t1 + 1, t2 - t1 - 1).c_str(), nullptr, 10);
            r.end = (uint32_t)strtoull(ln.substr(t2 + 1, t3 == std::string::npos ? std::string::npos : t3 - t2 - 1).c_str(), nullptr, 10);
            r.has_rest = t3 != std::string::npos;
            if (r.has_rest) r.rest = ln.substr(t3 + 1);
            rows.push_back(r);
        }
    }
    uint64_t digests[8];
    for (uint32_t kind = BED_CHR; kind <= BED_LINE; ++kind) {
        std::vector<uint8_t> stream;
        for (size_t i = 0; i < rows.size(); ++i) {
            for (int as_last = 0; as_last < 2; ++as_last) {
                const BedRow b = view(rows[i], as_last != 0);
                const uint32_t n = bed_row_bytes(kind, b);
                uint8_t *piece = (uint8_t *)malloc(n ? n : 1);
                CHECK(bed_row_write(kind, b, piece) == n, "row %zu kind %u: bed_row_write != bed_row_bytes", i, kind);
                for (uint32_t k = 0; k < n; ++k) CHECK(bed_row_byte(kind, b, k) == piece[k], "row %zu kind %u byte %u", i, kind, k);
                if ((as_last != 0) == (i + 1 == rows.size())) stream.insert(stream.end(), piece, piece + n);
                free(piece);
            }
        }
        hash_block(stream, &digests[2 * kind], "stream");
    }
    uint64_t id[2];
    bed_identifier(digests, id);
    uint8_t d[16];
    char text[33];
    text[32] = '\0';
    memcpy(d, id, 16), md5_hex(d, text);
    CHECK(!strcmp(text, argv[2]), "identifier %s, expected %s", text, argv[2]);
    memcpy(d, &digests[2 * BED_LINE], 16), md5_hex(d, text);
    CHECK(!strcmp(text, argv[3]), "file digest %s, expected %s", text, argv[3]);
    printf("bed_text_host_check: %zu rows, %d failure(s)\n", rows.size(), fails);
    return fails ? 1 : 0;
}
