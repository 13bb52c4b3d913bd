// refget_host_check.cpp -- md5.h and refget_core.h under the sanitizers, as a stand-alone program (tests/test_refget_cpu.py
// builds it with -fsanitize=address,undefined and writes its inputs):
//   refget_host_check messages.txt fasta.bin walks.txt
// messages.txt: per line a message in hex ("-": empty), then sha512t24u, MD5 and alphabet class of its upper-cased bytes and
// the MD5 of the bytes as they are.  Every message is copied into a heap block of exactly its size, so that a read past
// its end is an error, and goes through refget_hash (the combined loop), md5_stream and sha512_stream.
// walks.txt: per line a cut, the number of records of fasta.bin[0, cut) and per record length:sha512t24u:fai-offset ("-":
// no FAI).  The walk runs on an exactly sized copy of every prefix.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../gtars_amd/csrc/refget_core.h"

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

static std::string read_all(const char *path) {
    std::ifstream f(path, std::ios::binary);
    std::stringstream s;
    s << f.rdbuf();
    return s.str();
}

static std::vector<uint8_t> unhex(const std::string &h) {
    std::vector<uint8_t> out;
    if (h == "-") return out;
    auto v = [](char c) { return c <= '9' ? c - '0' : c - 'a' + 10; };
    for (size_t i = 0; i + 1 < h.size(); i += 2) out.push_back((uint8_t)(v(h[i]) << 4 | v(h[i + 1])));
    return out;
}

int main(int argc, char **argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: refget_host_check messages.txt fasta.bin walks.txt\n");
        return 2;
    }
    size_t n_messages = 0, n_walks = 0;
    {
        std::istringstream in(read_all(argv[1]));
        std::string hex, sha, md5_up, md5_raw;
        int cls;
        while (in >> hex >> sha >> md5_up >> cls >> md5_raw) {
            const std::vector<uint8_t> msg = unhex(hex);
            const size_t n = msg.size();
            uint8_t *block = (uint8_t *)malloc(n ? n : 1);  // (exactly sized: nothing readable behind the message)
            if (n) memcpy(block, msg.data(), n);
            RefgetDigest d;
            refget_digest_host(n ? block : nullptr, n, d);
            char hexed[32];
            md5_hex(d.md5, hexed);
            CHECK(std::string(d.text, 32) == sha, "length %zu: sha512t24u %.32s, expected %s", n, d.text, sha.c_str());
            CHECK(std::string(hexed, 32) == md5_up, "length %zu: md5 %.32s, expected %s", n, hexed, md5_up.c_str());
            CHECK(d.cls == cls, "length %zu: class %d, expected %d", n, d.cls, cls);
            uint8_t raw[16];
            md5(block, n, raw);
            md5_hex(raw, hexed);
            CHECK(std::string(hexed, 32) == md5_raw, "length %zu: md5_stream %.32s, expected %s", n, hexed, md5_raw.c_str());
            // the upper-cased bytes through the two streaming forms agree with the combined loop
            for (size_t i = 0; i < n; ++i) block[i] = refget_upper(block[i]);
            char text[32];
            sha512t24u(block, n, text);
            CHECK(memcmp(text, d.text, 32) == 0, "length %zu: sha512_stream and the combined loop differ", n);
            md5(block, n, raw);
            CHECK(memcmp(raw, d.md5, 16) == 0, "length %zu: md5_stream and the combined loop differ", n);
            uint32_t mask = 0;
            for (size_t i = 0; i < n; ++i) mask |= refget_class_bit(block[i]);
            CHECK(refget_guess(mask) == d.cls, "length %zu: the class differs byte by byte", n);
            free(block);
            ++n_messages;
        }
    }
    {
        const std::string fasta = read_all(argv[2]);
        std::istringstream in(read_all(argv[3]));
        std::string line;
        while (std::getline(in, line)) {
            std::istringstream fields(line);
            size_t cut, n_recs;
            fields >> cut >> n_recs;
            char *block = (char *)malloc(cut ? cut : 1);
            if (cut) memcpy(block, fasta.data(), cut);
            std::string blob;
            std::vector<RefgetRecord> recs;
            refget_walk_fasta(block, cut, blob, recs);
            free(block);
            CHECK(recs.size() == n_recs, "cut %zu: %zu records, expected %zu", cut, recs.size(), n_recs);
            for (size_t i = 0; i < recs.size() && i < n_recs; ++i) {
                std::string want;
                fields >> want;
                RefgetDigest d;
                refget_digest_host((const uint8_t *)blob.data() + recs[i].off, recs[i].len, d);
                const std::string got = std::to_string(recs[i].len) + ":" + std::string(d.text, 32) + ":" +
                                        (recs[i].has_fai ? std::to_string(recs[i].fai_offset) : std::string("-"));
                CHECK(got == want, "cut %zu record %zu: %s, expected %s", cut, i, got.c_str(), want.c_str());
            }
            ++n_walks;
        }
    }
    // the substring rule at its edges
    uint32_t bytes;
    CHECK(refget_sub_status(5, 5, 3, &bytes) == RG_SUB_OK && bytes == 0, "start == end past the end");
    CHECK(refget_sub_status(0, 3, 3, &bytes) == RG_SUB_OK && bytes == 3, "the whole sequence");
    CHECK(refget_sub_status(0, 4, 3, &bytes) == RG_SUB_BAD_RANGE && bytes == 0, "past the end");
    CHECK(refget_sub_status(2, 1, 3, &bytes) == RG_SUB_BAD_RANGE, "inverted");
    CHECK(refget_sub_status(3, 4, 3, &bytes) == RG_SUB_BAD_RANGE, "start at the end");
    CHECK(refget_sub_status(0, 1ull << 32, 1ull << 33, &bytes) == RG_SUB_TOO_WIDE && bytes == 0, "too wide");
    if (n_messages < 301 || n_walks < 2) {
        fprintf(stderr, "too few cases: %zu messages, %zu walks\n", n_messages, n_walks);
        return 1;
    }
    if (fails) return 1;
    printf("ok: %zu messages, %zu walks\n", n_messages, n_walks);
    return 0;
}
