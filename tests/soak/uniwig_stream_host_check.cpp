// uniwig_stream_host_check.cpp -- the parser header of the streaming uniwig (csrc/uniwig_stream_parse.h) under the host
// sanitizers, stand-alone:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -o check uniwig_stream_host_check.cpp -lz && ./check cases.txt
// cases.txt, one case per line:  <input as hex, "-" for empty> TAB <expected>
//   expected = "ok" followed by " <chrom as hex>:<start>:<end>:<score>" per row, or "err <message as hex>", or "err *" (any
//   error).  Every input is parsed from a heap block of exactly its size, so a read past either end is an ASan report.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>

#include "../../gtars_amd/csrc/uniwig_stream_parse.h"

static std::string to_hex(const std::string &s) {
    static const char *d = "0123456789abcdef";
    std::string out;
    for (unsigned char c : s) {
        out.push_back(d[c >> 4]);
        out.push_back(d[c & 15]);
    }
    return out;
}

static int nib(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s cases.txt\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    std::string line;
    size_t n_cases = 0, n_bad = 0;
    while (std::getline(in, line)) {
        const size_t tab = line.find('\t');
        if (tab == std::string::npos) continue;
        const std::string hex = line.substr(0, tab), want = line.substr(tab + 1);
        const size_t n = hex == "-" ? 0 : hex.size() / 2;
        unsigned char *block = (unsigned char *)malloc(n ? n : 1);
        for (size_t i = 0; i < n; ++i) block[i] = (unsigned char)(nib(hex[2 * i]) * 16 + nib(hex[2 * i + 1]));
        gtars::swparse::Rows rows;
        std::string err, got;
        // (n == 0: a one-byte block of which nothing may be read)
        if (gtars::swparse::parse_buffer(block, n, rows, err)) {
            got = "ok";
            for (size_t i = 0; i < rows.cid.size(); ++i)
                got += " " + to_hex(rows.names[rows.cid[i]]) + ":" + std::to_string(rows.start[i]) + ":" + std::to_string(rows.end[i]) + ":" +
                       std::to_string(rows.score[i]);
        } else {
            got = want == "err *" ? "err *" : "err " + to_hex(err);
            if (!rows.cid.empty() || !rows.names.empty()) got += " (rows kept)";
        }
        free(block);
        ++n_cases;
        if (got != want) {
            ++n_bad;
            fprintf(stderr, "case %zu (%s):\n  want %s\n  got  %s\n", n_cases, hex.c_str(), want.c_str(), got.c_str());
        }
    }
    printf("%zu cases, %zu wrong\n", n_cases, n_bad);
    return n_bad ? 1 : 0;
}
