// reftx_host_check.cpp -- a stand-alone program (its own main) over csrc/reftx_core.h, meant to be built with
// -fsanitize=address,undefined and run by tests/test_reftx_cpu.py:
//   reftx_host_check <store.reftx> <seed>
//   * the .reftx decoder on every truncation of the file and on random byte flips, each in a heap block of exactly the bytes
//     it is given, so that a read past the end is a sanitizer report; a store that still decodes is looked up and mapped;
//   * the scalar mapper (binary searches) on random transcripts against a linear-scan copy of mapper.rs written here;
//   * the streamed digest of a mature sequence against the same sequence hashed from memory.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../gtars_amd/csrc/reftx_core.h"

using namespace gtars;

static int failures = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                \
        }                                                              \
    } while (0)

// decodes a copy of data[0, n) that lives in a block of exactly n bytes
static bool decode_exact(const uint8_t *data, size_t n, TxStoreData &out) {
    uint8_t *block = (uint8_t *)malloc(n ? n : 1);
    if (n) memcpy(block, data, n);
    std::string err;
    const bool ok = out.decode(block, n, err);
    EXPECT(ok || !err.empty());
    free(block);
    return ok;
}

// ---- mapper.rs with its linear scans ------------------------------------------------------------------------------------
struct Off {
    uint64_t ts, te, gs, ge;
};
static std::vector<Off> offsets_of(const TxRecord &r) {
    std::vector<Off> out;
    uint64_t pos = 0;
    const size_t n = r.exons.size();
    for (size_t j = 0; j < n; ++j) {
        const TxExon &e = r.exons[r.strand > 0 ? j : n - 1 - j];
        out.push_back({pos, pos + (e.end - e.start), e.start, e.end});
        pos += e.end - e.start;
    }
    return out;
}
static bool g2t(const TxRecord &r, const std::vector<Off> &o, uint64_t g, uint64_t *out) {
    for (const Off &e : o)
        if (g >= e.gs && g < e.ge) {
            *out = e.ts + (r.strand > 0 ? g - e.gs : e.ge - 1 - g);
            return true;
        }
    return false;
}
static bool t2g(const TxRecord &r, const std::vector<Off> &o, uint64_t p, uint64_t *out) {
    for (const Off &e : o)
        if (p >= e.ts && p < e.te) {
            *out = r.strand > 0 ? e.gs + (p - e.ts) : e.ge - 1 - (p - e.ts);
            return true;
        }
    return false;
}
static uint8_t linear_map(const TxRecord &r, uint32_t kind, int64_t pos, int64_t off, bool star, uint64_t *out) {
    *out = 0;
    const std::vector<Off> o = offsets_of(r);
    const uint64_t len = o.empty() ? 0 : o.back().te;
    if (kind == TX_KIND_G) return g2t(r, o, (uint64_t)pos, out) ? TX_OK : TX_NOT_EXONIC;
    uint64_t p;
    if (kind == TX_KIND_C) {
        uint64_t a, b;
        if (!r.is_coding() || r.cds_end == 0 || !g2t(r, o, r.cds_start, &a) || !g2t(r, o, r.cds_end - 1, &b)) return TX_NON_CODING;
        const uint64_t lo = std::min(a, b), hi = std::max(a, b) + 1;
        if (star) {
            if (pos <= 0 || hi + (uint64_t)(pos - 1) >= len) return TX_UTR3_OVERFLOW;
            p = hi + (uint64_t)(pos - 1);
        } else if (pos > 0) {
            p = lo + (uint64_t)pos - 1;
            if (p >= hi) return TX_OUTSIDE_CDS;
        } else if (pos < 0) {
            const uint64_t utr = 0 - (uint64_t)pos;
            if (utr > lo) return TX_UTR5_OVERFLOW;
            p = lo - utr;
        } else {
            return TX_OUTSIDE_CDS;
        }
    } else {
        if (pos <= 0 || (uint64_t)pos - 1 >= len) return TX_OUTSIDE_TRANSCRIPT;
        p = (uint64_t)pos - 1;
    }
    uint64_t anchor = 0;
    if (!t2g(r, o, p, &anchor)) return TX_OUTSIDE_TRANSCRIPT;
    if (off == 0) {
        *out = anchor;
        return TX_OK;
    }
    bool boundary = false;
    for (size_t i = 0; i < o.size(); ++i) {
        if (off > 0 && p + 1 == o[i].te && i + 1 < o.size()) boundary = true;
        if (off < 0 && p == o[i].ts && i > 0) boundary = true;
    }
    if (!boundary) return TX_INVALID_OFFSET;
    const uint64_t mag = off > 0 ? (uint64_t)off : 0 - (uint64_t)off;
    if ((off > 0) == (r.strand > 0)) {
        if (anchor + mag < anchor) return TX_INVALID_OFFSET;
        *out = anchor + mag;
    } else {
        if (mag > anchor) return TX_INVALID_OFFSET;
        *out = anchor - mag;
    }
    return TX_OK;
}

static TxRecord random_record(std::mt19937_64 &rng, uint32_t span) {
    TxRecord r;
    r.accession = "NM_" + std::to_string(rng() % 100000) + ".1";
    r.strand = rng() & 1 ? 1 : -1;
    const size_t n = 1 + rng() % 9;
    std::vector<uint32_t> cuts(2 * n);
    for (uint32_t &c : cuts) c = (uint32_t)(rng() % span);
    std::sort(cuts.begin(), cuts.end());
    for (size_t k = 0; k < n; ++k) {
        uint32_t s = cuts[2 * k], e = cuts[2 * k + 1];
        if (rng() % 6 == 0) e = s;
        if (k && rng() % 5 == 0) s = r.exons.back().end, e = std::max(e, s);
        r.exons.push_back({s, e});
    }
    if (rng() % 4) {
        r.cds_start = (uint32_t)(rng() % span), r.cds_end = (uint32_t)(rng() % span);
        if (rng() % 3) {  // the CDS ends on exon bases
            const TxExon &a = r.exons[rng() % n], &b = r.exons[rng() % n];
            if (a.start < a.end && b.start < b.end) r.cds_start = std::min(a.start, b.start), r.cds_end = std::max(a.end, b.end);
        }
    }
    return r;
}

static void check_mapper(std::mt19937_64 &rng) {
    const int64_t specials[] = {0, 1, -1, 2, INT64_MAX, INT64_MIN, INT64_MIN + 1, 1ll << 40, -(1ll << 40)};
    for (int round = 0; round < 300; ++round) {
        std::vector<TxRecord> recs;
        for (int k = 0; k < 8; ++k) recs.push_back(random_record(rng, round % 3 ? 80 : 5000));
        TxHostTables tab;
        EXPECT(tab.build(recs));
        const TxTables t = tab.view();
        for (uint32_t tx = 0; tx < recs.size(); ++tx) {
            EXPECT(!tab.bad[tx]);
            EXPECT(tab.len[tx] == recs[tx].transcript_length());
            const int64_t len = tab.len[tx];
            for (int q = 0; q < 200; ++q) {
                const uint32_t kind = (uint32_t)(rng() % 3);
                int64_t pos = rng() % 4 ? (int64_t)(rng() % (uint64_t)(2 * len + 8)) - len - 3 : specials[rng() % 9];
                if (kind == TX_KIND_G) pos = (int64_t)(rng() % 5100);
                const int64_t off = rng() % 2 ? 0 : specials[rng() % 9];
                const bool star = rng() % 5 == 0;
                uint64_t a, b;
                const uint8_t sa = tx_map_one(t, tx, kind, pos, off, star, &a), sb = linear_map(recs[tx], kind, pos, off, star, &b);
                EXPECT(sa == sb && a == b);
            }
        }
        uint64_t v;
        EXPECT(tx_map_one(t, (uint32_t)recs.size(), TX_KIND_N, 1, 0, 0, &v) == TX_NOT_FOUND && tx_map_one(t, TX_NONE, TX_KIND_C, 1, 0, 0, &v) == TX_NOT_FOUND);
        EXPECT(tx_map_one(t, 0, 3, 1, 0, 0, &v) == TX_BAD_KIND);
        // the streamed digest and the sequence in memory, over a chromosome of exactly the bytes the exons may reach
        const uint32_t span = round % 3 ? 80 : 5000;
        uint8_t *chrom = (uint8_t *)malloc(span);
        for (uint32_t i = 0; i < span; ++i) chrom[i] = (uint8_t)"ACGTNacgtnRYkm-"[rng() % 15];
        for (uint32_t tx = 0; tx < recs.size(); ++tx) {
            std::string seq;
            tx_sequence(t, tx, chrom, seq);
            char d1[32], d2[32];
            tx_digest(t, tx, chrom, d1);
            sha512t24u((const uint8_t *)seq.data(), seq.size(), d2);
            EXPECT(memcmp(d1, d2, 32) == 0 && seq.size() == tab.len[tx]);
            for (char c : seq) EXPECT(c != 0 && !(c >= 'a' && c <= 'z'));
        }
        free(chrom);
    }
    // exons that overlap or descend are refused, not searched
    TxRecord bad;
    bad.exons = {{10, 20}, {15, 30}};
    TxRecord worse;
    worse.exons = {{30, 20}};
    TxHostTables tab;
    EXPECT(tab.build({bad, worse}));
    uint64_t v;
    EXPECT(tab.bad[0] && tab.bad[1] && tx_map_one(tab.view(), 0, TX_KIND_N, 1, 0, 0, &v) == TX_BAD_EXONS);
}

int main(int argc, char **argv) {
    if (argc < 3) return fprintf(stderr, "usage: %s store.reftx seed\n", argv[0]), 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return fprintf(stderr, "cannot open %s\n", argv[1]), 2;
    std::vector<uint8_t> image;
    for (int c; (c = fgetc(f)) != EOF;) image.push_back((uint8_t)c);
    fclose(f);
    std::mt19937_64 rng(strtoull(argv[2], nullptr, 10));

    TxStoreData whole;
    EXPECT(decode_exact(image.data(), image.size(), whole));
    EXPECT(whole.recs.size() == 2);
    for (const TxRecord &r : whole.recs) EXPECT(whole.lookup(r.accession.data(), r.accession.size()) >= 0);
    EXPECT(whole.lookup("NM_NOPE.1", 9) < 0);
    // the encoder writes the bytes it read
    std::string again, err;
    EXPECT(tx_encode(whole.recs, again, err) && again.size() == image.size() && memcmp(again.data(), image.data(), image.size()) == 0);
    for (size_t n = 0; n < image.size(); ++n) {
        TxStoreData cut;
        EXPECT(!decode_exact(image.data(), n, cut));
    }
    size_t decoded = 0;
    for (int k = 0; k < 20000; ++k) {
        std::vector<uint8_t> bad = image;
        for (int flips = 1 + (int)(rng() % 3); flips; --flips) bad[rng() % bad.size()] = (uint8_t)rng();
        TxStoreData s;
        if (!decode_exact(bad.data(), bad.size(), s)) continue;
        ++decoded;
        TxHostTables tab;
        EXPECT(tab.build(s.recs));
        const TxTables t = tab.view();
        for (uint32_t tx = 0; tx < s.recs.size(); ++tx) {
            (void)s.lookup(s.recs[tx].accession.data(), s.recs[tx].accession.size());
            (void)s.lookup_mane(s.recs[tx].gene);
            uint64_t v;
            for (int64_t pos = -3; pos < 12; ++pos)
                for (uint32_t kind = 0; kind < 3; ++kind) (void)tx_map_one(t, tx, kind, kind == TX_KIND_G ? pos + 50 : pos, pos & 1 ? 1 : -1, pos == 2, &v);
        }
    }
    EXPECT(decoded > 100);
    check_mapper(rng);
    // base64url of 24 bytes, both ways
    uint8_t d[24], back[24];
    for (int i = 0; i < 24; ++i) d[i] = (uint8_t)rng();
    char text[36] = "SQ.";
    tx_digest_encode(d, text + 3);
    long got = 0;
    EXPECT(tx_digest_decode(text, 35, back, &got) && got == 24 && memcmp(d, back, 24) == 0);
    EXPECT(tx_digest_decode(text + 3, 32, back) && !tx_digest_decode(text, 34, back, &got) && !tx_digest_decode("SQ.notbase64!!!", 15, back, &got) && got == -1);
    if (failures) return fprintf(stderr, "%d check(s) failed\n", failures), 1;
    printf("ok: %zu flipped stores still decoded\n", decoded);
    return 0;
}
