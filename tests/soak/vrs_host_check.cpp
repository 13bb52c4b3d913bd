// vrs_host_check.cpp -- csrc/sha512.h and the VCF line rules of csrc/vrs_core.h alone, for a build with AddressSanitizer and
// UBSan (tests/test_vrs_cpu.py compiles and runs it; nothing of it is loaded into python).
//   vrs_host_check <digests file> <seed>
// The digests file holds one line per message length n = 0 .. 300: "n digest", digest = sha512t24u of the n bytes
// b[k] = (31 n + 7 k) mod 256, written by the test with hashlib.  Then the line parser is fed lines it must survive: random
// bytes, well-formed lines, and every truncation of those, each in an exactly sized heap block so that a read past the end
// is seen.  The normalizer runs over random short sequences the same way.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../gtars_amd/csrc/vrs_core.h"

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static int fail(const char *what, size_t n) {
    fprintf(stderr, "FAILED: %s (%zu)\n", what, n);
    return 1;
}

// the parser on an exact copy of the line; whatever it returns must lie inside the line
static bool parse_checked(const std::string &line, size_t &alts_seen) {
    char *copy = (char *)malloc(line.size() ? line.size() : 1);
    memcpy(copy, line.data(), line.size());
    gtars::VcfRecord r;
    const bool got = gtars::vcf_parse_line(copy, line.size(), r);
    bool ok = true;
    if (got) {
        const char *end = copy + line.size();
        ok = r.chrom >= copy && r.chrom + r.n_chrom <= end && r.ref >= copy && r.ref + r.n_ref <= end && r.alts >= copy &&
             r.alts + r.n_alts <= end;
        if (ok)
            gtars::vcf_for_real_alts(r.alts, r.n_alts, [&](const char *a, size_t n) {
                ok = ok && a >= r.alts && a + n <= r.alts + r.n_alts && n > 0 && a[0] != '<';
                ++alts_seen;
            });
    }
    free(copy);
    return ok;
}

int main(int argc, char **argv) {
    if (argc < 3) return fail("usage: vrs_host_check <digests file> <seed>", 0);
    rng_state = strtoull(argv[2], nullptr, 10);
    FILE *f = fopen(argv[1], "r");
    if (!f) return fail("cannot open the digests file", 0);
    size_t checked = 0;
    for (;;) {
        unsigned n;
        char want[64];
        if (fscanf(f, "%u %63s", &n, want) != 2) break;
        uint8_t *msg = (uint8_t *)malloc(n ? n : 1);
        for (unsigned k = 0; k < n; ++k) msg[k] = (uint8_t)(31 * n + 7 * k);
        char got[33] = {0};
        gtars::sha512t24u(msg, n, got);
        free(msg);
        if (strcmp(got, want) != 0) return fail("sha512t24u differs at length", n);
        ++checked;
    }
    fclose(f);
    if (checked != 301) return fail("expected 301 digests", checked);

    size_t lines = 0, parsed_alts = 0;
    const char *alphabet = "\t\t\t,<*.#\r\nACGTacgtN0123456789+-chr";
    const size_t n_alpha = strlen(alphabet);
    for (int round = 0; round < 400; ++round) {
        std::string line;
        if (round % 2 == 0) {
            const size_t n = rnd() % 80;
            for (size_t k = 0; k < n; ++k) line.push_back(rnd() % 4 ? alphabet[rnd() % n_alpha] : (char)rnd());
        } else {
            line = "chr" + std::to_string(rnd() % 30) + "\t" + std::to_string(rnd() % 100000) + "\trs" + std::to_string(rnd() % 1000) + "\t";
            for (size_t k = rnd() % 6; k-- > 0;) line.push_back("ACGT"[rnd() % 4]);
            line.push_back('\t');
            for (size_t a = rnd() % 5; a-- > 0;) {
                const int kind = (int)(rnd() % 6);
                line += kind == 0 ? "<DEL>" : kind == 1 ? "*" : kind == 2 ? "." : kind == 3 ? "" : std::string(1 + rnd() % 4, "ACGT"[rnd() % 4]);
                if (a) line.push_back(',');
            }
            if (rnd() % 2) line += "\t50\tPASS\tAC=1;AF=0.5";
            if (rnd() % 2) line += rnd() % 2 ? "\r\n" : "\n";
        }
        for (size_t cutoff = 0; cutoff <= line.size(); ++cutoff) {
            if (!parse_checked(line.substr(0, cutoff), parsed_alts)) return fail("the parser left the line", lines);
            ++lines;
        }
    }
    if (!parsed_alts) return fail("no well-formed line was parsed", lines);

    // the normalizer and the streamed Allele digest against the copied one
    size_t normalized = 0;
    for (int round = 0; round < 3000; ++round) {
        const size_t n = 1 + rnd() % 40;
        uint8_t *seq = (uint8_t *)malloc(n);
        const int letters = 1 + (int)(rnd() % 3);
        for (size_t k = 0; k < n; ++k) seq[k] = (uint8_t)"ACgt"[rnd() % letters];
        const uint64_t start = rnd() % (n + 2);
        const size_t rl = rnd() % 4, al = rnd() % 4;
        uint8_t *ref = (uint8_t *)malloc(rl ? rl : 1), *alt = (uint8_t *)malloc(al ? al : 1);
        for (size_t k = 0; k < rl; ++k) ref[k] = start + k < n && rnd() % 8 ? gtars::vrs_upper(seq[start + k]) : (uint8_t)'T';
        for (size_t k = 0; k < al; ++k) alt[k] = (uint8_t)"ACGT"[rnd() % letters];
        const gtars::VrsNorm r = gtars::vrs_normalize(seq, n, start, ref, rl, alt, al);
        if (r.status == gtars::VRS_OK) {
            if (r.start > r.end || r.end > n) return fail("normalized interval outside the sequence", (size_t)round);
            const std::string s = gtars::vrs_norm_sequence(r, seq, alt);
            char loc[32], streamed[33] = {0}, copied[33] = {0};
            gtars::vrs_location_digest("SQ.x", 4, r.start, r.end, loc);
            gtars::vrs_allele_digest(loc, seq + r.start, r.lroll, alt + r.alt_skip, r.alt_len, seq + (r.end - r.rroll), r.rroll, streamed);
            gtars::vrs_allele_digest(loc, nullptr, 0, (const uint8_t *)s.data(), s.size(), nullptr, 0, copied);
            if (strcmp(streamed, copied) != 0) return fail("streamed and copied digests differ", (size_t)round);
            ++normalized;
        } else {
            (void)gtars::vrs_error_text(r.status, seq, n, start, ref, rl);
        }
        free(seq), free(ref), free(alt);
    }
    if (!normalized) return fail("nothing normalized", 0);
    printf("all checks passed: %zu digests, %zu lines, %zu alleles normalized\n", checked, lines, normalized);
    return 0;
}
