// hgvs_host_check.cpp -- a stand-alone program (its own main) over csrc/hgvs_core.h, meant to be built with
// -fsanitize=address,undefined and run by tests/test_hgvs_cpu.py:
//   hgvs_host_check <seed>
//   * hgvs_parse on a list of valid expressions, on every prefix of each and on random byte flips, each text in a heap block of
//     exactly its bytes, so that a read past the end is a sanitizer report; every span of a row that parsed lies in the text;
//   * hgvs_span_one and hgvs_pool_byte on random transcripts over a random chromosome, the chromosome and the expression's
//     text in exactly sized blocks too: a row that passes has its span inside the chromosome, its REF bytes are the
//     chromosome's, and its ALT has the length and the bytes compute_alt would give.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../gtars_amd/csrc/hgvs_core.h"

using namespace gtars;

static int failures = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                \
        }                                                              \
    } while (0)

static const char *const VALID[] = {
    "NC_000007.14:g.140753336A>T", "NM_004333.6:c.1799T>A", "NM_004333.6:c.-14C>T", "NM_004333.6:c.*37A>G", "NM_004333.6:c.1798+5G>A",
    "NM_004333.6:c.1799-3T>A", "NM_004333.6:c.100delAGT", "NM_004333.6:c.100del", "NM_004333.6:c.100del3", "NM_004333.6:c.100_102dupATG",
    "NM_004333.6:c.100_101insATG", "NM_004333.6:c.100_102delinsCT", "NM_004333.6:c.100_102delAGTinsCT", "NM_004333.6:c.100=",
    "NM_004333.6:c.100G=", "NM_004333.6(BRAF):c.1799T>A", "BRAF:c.1799T>A", "NM_004333.6:c.(1799T>A)", "NC_000007.14:g.100_200inv",
    "NM_004333.6:c.(4_6)_246del", "NM_004333.6:c.4_(245_246)del", "NM_004333.6:c.(?_6)_(245_?)dup", "NC_000001.11:g.=", "NC_000001.11:g.?",
    "NC_000001.11:g.100_200copy3", "NC_000001.11:g.100CA[4]", "NR_1.1:n.5+3del", "NC_012920.1:m.3243A>G", "NM_1.1:r.76a>c", "NP_1.1:p.Val600Glu",
    "NM_1.1:c.*5_*7delinsacgtnRYK", "NM_1.1:c.+5A>T",
};

// parses a copy of text[0, n) that lives in a block of exactly n bytes
static uint8_t parse_exact(const char *text, size_t n, HgvsRow *row) {
    char *block = (char *)malloc(n ? n : 1);
    if (n) memcpy(block, text, n);
    size_t at = 0;
    const char *msg = nullptr;
    const uint8_t st = hgvs_parse(block, n, row, &at, &msg);
    EXPECT(st == HGVS_OK || st == HGVS_PARSE_ERROR || st == HGVS_UNSUPPORTED_REFERENCE_TYPE);
    EXPECT((st == HGVS_PARSE_ERROR) == (msg != nullptr));
    EXPECT(at <= n);
    if (st != HGVS_PARSE_ERROR) {
        EXPECT((uint64_t)row->acc_off + row->acc_len <= n && (uint64_t)row->gene_off + row->gene_len <= n);
        EXPECT((uint64_t)row->ref_off + row->ref_len <= n && (uint64_t)row->alt_off + row->alt_len <= n);
        EXPECT(row->acc_len > 0 && row->ref_type <= HGVS_REF_P && row->loc <= HGVS_LOC_UNCERTAIN_BOTH && row->edit <= HGVS_EDIT_REPEAT);
    }
    free(block);
    return st;
}

static void check_parser(std::mt19937_64 &rng) {
    for (const char *s : VALID) {
        const size_t n = strlen(s);
        HgvsRow row;
        const uint8_t st = parse_exact(s, n, &row);
        EXPECT(st == (strstr(s, ":p.") ? HGVS_UNSUPPORTED_REFERENCE_TYPE : HGVS_OK));
        for (size_t k = 0; k < n; ++k) parse_exact(s, k, &row);
        for (int round = 0; round < 200; ++round) {
            std::string t(s);
            const int flips = 1 + (int)(rng() % 3);
            for (int f = 0; f < flips; ++f) t[rng() % n] = (char)(rng() % 4 ? "()_?*+-=>[]:.0123456789ACGTacgtdelinsupvcopy"[rng() % 44] : (char)(rng() & 0xFF));
            parse_exact(t.data(), t.size(), &row);
        }
    }
    EXPECT(hgvs_looks_like_gene_symbol("BRAF", 4) && hgvs_looks_like_gene_symbol("KIT", 3) && hgvs_looks_like_gene_symbol("GL", 2));
    EXPECT(!hgvs_looks_like_gene_symbol("GL000220", 8) && !hgvs_looks_like_gene_symbol("MT", 2) && !hgvs_looks_like_gene_symbol("chr7", 4));
}

static TxRecord random_transcript(std::mt19937_64 &rng, uint32_t span) {
    TxRecord r;
    r.strand = rng() & 1 ? 1 : -1;
    const size_t n = 1 + rng() % 5;
    std::vector<uint32_t> cuts(2 * n);
    for (uint32_t &c : cuts) c = (uint32_t)(rng() % span);
    std::sort(cuts.begin(), cuts.end());
    for (size_t k = 0; k < n; ++k) r.exons.push_back(TxExon{cuts[2 * k], cuts[2 * k + 1]});
    if (rng() % 4) r.cds_start = r.exons.front().start, r.cds_end = r.exons.back().end;
    return r;
}

static void check_bridge(std::mt19937_64 &rng) {
    const uint32_t len = 300;
    uint8_t *chrom = (uint8_t *)malloc(len);
    for (uint32_t k = 0; k < len; ++k) chrom[k] = (uint8_t)"ACGTacgtN"[rng() % 9];
    const uint8_t *chroms[1] = {chrom};
    const uint64_t lens[1] = {len};
    HgvsGenome g;
    g.chroms = chroms, g.len = lens, g.n_chrom = 1;
    int passed = 0;
    for (int round = 0; round < 400; ++round) {
        std::vector<TxRecord> recs{random_transcript(rng, len + 20)};  // (an exon may reach past the chromosome)
        TxHostTables tables;
        EXPECT(tables.build(recs));
        tables.chrom[0] = 0;
        const TxTables t = tables.view();
        for (int q = 0; q < 60; ++q) {
            // one row of columns: the alleles in a text block of exactly their bytes
            const uint32_t n_ref = (uint32_t)(rng() % 4), n_alt = (uint32_t)(rng() % 12);
            uint8_t *text = (uint8_t *)malloc(n_ref + n_alt ? n_ref + n_alt : 1);
            for (uint32_t k = 0; k < n_ref + n_alt; ++k) text[k] = (uint8_t)"ACGTNacgtR"[rng() % (rng() % 8 ? 5 : 10)];
            const uint8_t pre = 0, kind = (uint8_t)(rng() % 3), loc = (uint8_t)(rng() % 7 ? rng() % 2 : 2 + rng() % 4);
            static const uint8_t bridged[6] = {HGVS_EDIT_SUB, HGVS_EDIT_DEL, HGVS_EDIT_DUP, HGVS_EDIT_INS, HGVS_EDIT_DELINS, HGVS_EDIT_IDENTITY};
            const uint8_t edit = (uint8_t)(rng() % 9 ? bridged[rng() % 6] : rng() % 10);
            const uint8_t flags = (uint8_t)((rng() % 3 ? 0 : HGVS_HAS_REF) | (rng() % 5 ? 0 : HGVS_STAR1) | (rng() % 5 ? 0 : HGVS_STAR2));
            const uint32_t tx = kind == HGVS_REF_G ? (rng() % 9 ? 0u : 7u) : (rng() % 9 ? 0u : 1u);
            const int64_t base1 = (int64_t)(rng() % 340) - 20, base2 = rng() % 3 ? base1 + (int64_t)(rng() % 5) - 1 : (int64_t)(rng() % 340) - 20;
            const int64_t off1 = rng() % 4 ? 0 : (int64_t)(rng() % 9) - 4, off2 = rng() % 4 ? 0 : (int64_t)(rng() % 9) - 4;
            const uint64_t text_off = 0;
            const uint32_t ref_off = 0, alt_off = n_ref;
            HgvsCols c;
            c.pre = &pre, c.kind = &kind, c.loc = &loc, c.edit = &edit, c.flags = &flags, c.tx = &tx;
            c.base1 = &base1, c.off1 = &off1, c.base2 = &base2, c.off2 = &off2, c.text_off = &text_off;
            c.ref_off = &ref_off, c.ref_len = &n_ref, c.alt_off = &alt_off, c.alt_len = &n_alt;
            c.text = text, c.text_bytes = n_ref + n_alt, c.n = 1;
            const HgvsSpan s = hgvs_span_one(t, g, c, 0);
            EXPECT(s.status < HGVS_N_STATUS && s.status != HGVS_PARSE_ERROR && s.status != HGVS_NORMALIZE_ERROR);
            EXPECT((s.status == HGVS_MAPPING_ERROR) == (s.detail != 0));
            if (s.status == HGVS_OK) {
                ++passed;
                EXPECT(s.chrom == 0 && s.start + s.ref_len <= len);
                const bool rev = kind != HGVS_REF_G && recs[0].strand < 0;
                const uint64_t want_alt = edit == HGVS_EDIT_DEL ? 0 : edit == HGVS_EDIT_DUP ? 2 * s.ref_len : edit == HGVS_EDIT_IDENTITY ? s.ref_len : n_alt;
                EXPECT(s.alt_len == want_alt);
                for (uint64_t k = 0; k < s.ref_len + s.alt_len; ++k) {
                    const uint32_t b = hgvs_pool_byte(chrom, s.start, s.ref_len, s.alt_len, s.mode, text + alt_off, k);
                    uint32_t want;
                    if (k < s.ref_len) want = tx_upper(chrom[s.start + k]);
                    else if (s.mode == HGVS_ALT_SPAN) want = tx_upper(chrom[s.start + (k - s.ref_len) % s.ref_len]);
                    else if (rev) want = hgvs_complement(text[alt_off + n_alt - 1 - (k - s.ref_len)]);
                    else want = text[alt_off + (k - s.ref_len)];
                    EXPECT(b == want && b != 0);
                }
                if (flags & HGVS_HAS_REF) EXPECT(n_ref == s.ref_len);
            }
            free(text);
        }
    }
    EXPECT(passed > 100);
    free(chrom);
}

int main(int argc, char **argv) {
    std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 1);
    check_parser(rng);
    check_bridge(rng);
    if (failures) {
        fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
