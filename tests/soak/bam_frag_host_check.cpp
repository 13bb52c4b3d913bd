// bam_frag_host_check.cpp -- a stand-alone program (its own main) over csrc/bam_frag_core.h, meant to be built with
// -fsanitize=address,undefined and run by tests/test_bam_frag_cpu.py:
//   * the worked example of DESIGN.md §3 K26: every record's outcome and coordinates;
//   * the aux walk over every type, with the barcode tag first, last, twice, empty and with another type;
//   * records whose aux data is malformed, each in a heap block of exactly the record's bytes, so that a read past the end is
//     a sanitizer report: an unknown type, a Z without NUL, a value cut by the record's end, a B count of 0xFFFFFFFF, an aux
//     start past block_size, an l_seq of 0x7FFFFFFF -- and every truncation of a well-formed aux area.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../gtars_amd/csrc/bam_frag_core.h"

using namespace gtars;

static int failures = 0;
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                \
        }                                                              \
    } while (0)

static void put16(std::string &s, uint32_t v) { s.push_back((char)(v & 255)), s.push_back((char)(v >> 8 & 255)); }
static void put32(std::string &s, uint32_t v) { put16(s, v & 0xFFFF), put16(s, v >> 16); }

struct Rec {
    int32_t ref = 0, pos = 0, next_ref = 0, tlen = 0;
    uint32_t mapq = 60, flag = 99, l_seq = 4, n_cigar = 1;
    std::string name = "r", aux;
    // l_seq_field / block_size_delta: what the record CLAIMS, where that differs from what it holds
    std::string bytes(int64_t l_seq_field = -1, int64_t block_size_delta = 0) const {
        std::string b;
        put32(b, (uint32_t)ref), put32(b, (uint32_t)pos);
        b.push_back((char)(name.size() + 1)), b.push_back((char)mapq);
        put16(b, 4680), put16(b, n_cigar), put16(b, flag);
        put32(b, l_seq_field < 0 ? l_seq : (uint32_t)l_seq_field);
        put32(b, (uint32_t)next_ref), put32(b, 0xFFFFFFFFu), put32(b, (uint32_t)tlen);
        b += name, b.push_back('\0');
        for (uint32_t k = 0; k < n_cigar; ++k) put32(b, 10u << 4);
        b.append((l_seq + 1) / 2, '\x11'), b.append(l_seq, '\x1e');
        b += aux;
        std::string out;
        put32(out, (uint32_t)((int64_t)b.size() + block_size_delta));
        return out + b;
    }
};

static std::string Z(const char *tag, const std::string &v) { return std::string(tag) + "Z" + v + std::string(1, '\0'); }
static std::string B(const char *tag, char sub, uint32_t count, size_t each) {
    std::string s = std::string(tag) + "B" + std::string(1, sub);
    put32(s, count);
    s.append((size_t)count * each, '\x07');
    return s;
}

// the rule on a copy of `rec` that lives in a block of exactly its bytes
static int32_t run(const std::string &rec, const BamFragParams &p, BamFragRow *row, std::string *cb = nullptr) {
    static const uint32_t ref_len[2] = {1000, 500};
    uint8_t *block = (uint8_t *)malloc(rec.size());
    memcpy(block, rec.data(), rec.size());
    const int32_t r = bam_frag_rule(block, p, ref_len, 2, row);
    if (r == BF_KEPT && cb) cb->assign((const char *)block + row->cb_off, row->cb_len);
    free(block);
    return r;
}

static BamFragParams defaults() {
    BamFragParams p;
    p.tag[0] = 'C', p.tag[1] = 'B', p.use_tag = 1, p.min_mapq = 30, p.require_flags = 0x3, p.exclude_flags = 0xB0C;
    p.max_fragment_length = 2000, p.shift_left = 4, p.shift_right = -5;
    return p;
}

static void worked_example() {
    const BamFragParams p = defaults();
    struct Case {
        int32_t ref, pos, tlen;
        uint32_t flag, mapq;
        const char *cb;
        int32_t want;
        uint32_t start, end;
    };
    const Case cases[12] = {
        {0, 100, 200, 99, 60, "AAC-1", BF_KEPT, 104, 295},      {0, 100, 200, 99, 60, "AAC-1", BF_KEPT, 104, 295},
        {0, 100, 200, 99, 60, "AAA-1", BF_KEPT, 104, 295},      {0, 100, 150, 99, 60, "AAC-1", BF_KEPT, 104, 245},
        {0, 120, 200, 99, 10, nullptr, BF_MAPQ, 0, 0},          {0, 291, -200, 147, 60, "AAC-1", BF_NOT_LEFTMOST, 0, 0},
        {0, 990, 50, 99, 60, "AAC-1", BF_KEPT, 994, 1000},      {1, 0, 8, 99, 60, "AAC-1", BF_EMPTY, 0, 0},
        {1, 10, 3000, 99, 60, "AAC-1", BF_TOO_LONG, 0, 0},      {1, 20, 100, 99, 60, nullptr, BF_NO_BARCODE, 0, 0},
        {1, 30, 100, 99 | 0x400, 60, "AAC-1", BF_KEPT, 34, 125}, {-1, -1, 0, 0x4, 60, nullptr, BF_UNPLACED, 0, 0},
    };
    for (const Case &c : cases) {
        Rec r;
        r.ref = c.ref, r.pos = c.pos, r.next_ref = c.ref, r.tlen = c.tlen, r.flag = c.flag, r.mapq = c.mapq;
        if (c.cb) r.aux = Z("NM", "x") + Z("CB", c.cb);
        BamFragRow row;
        std::string cb;
        const int32_t got = run(r.bytes(), p, &row, &cb);
        EXPECT(got == c.want);
        if (got == BF_KEPT && c.want == BF_KEPT) EXPECT(row.ref == c.ref && row.start == c.start && row.end == c.end && cb == c.cb);
    }
    // the filters that the example does not reach
    Rec r;
    r.tlen = 100, r.aux = Z("CB", "A");
    BamFragRow row;
    r.flag = 0x41;  // not a proper pair
    EXPECT(run(r.bytes(), p, &row) == BF_FLAG);
    r.flag = 99 | 0x100;
    EXPECT(run(r.bytes(), p, &row) == BF_FLAG);
    r.flag = 99, r.next_ref = 1;
    EXPECT(run(r.bytes(), p, &row) == BF_MATE_REF);
    r.next_ref = 0, r.mapq = 255;
    EXPECT(run(r.bytes(), p, &row) == BF_KEPT);
    BamFragParams q = p;
    q.shift_left = -500, q.shift_right = 0, r.pos = 3;
    EXPECT(run(r.bytes(), q, &row) == BF_KEPT && row.start == 0 && row.end == 103);
    q.use_tag = 0, r.aux = "garbage";  // no tag is looked for: the aux area is never walked
    EXPECT(run(r.bytes(), q, &row) == BF_KEPT && row.cb_len == 0);
}

static void aux_layouts() {
    const BamFragParams p = defaults();
    Rec r;
    r.tlen = 100;
    BamFragRow row;
    std::string cb;
    const std::string every = std::string("XAAq") + std::string("XccZ") + std::string("XCC\x09") + std::string("XssAB") + std::string("XSSAB") +
                              std::string("XiiABCD") + std::string("XIIABCD") + std::string("XffABCD") + Z("XZ", "text with CB in it") +
                              Z("XH", "1AE301") + B("Bc", 'c', 3, 1) + B("BC", 'C', 0, 1) + B("Bs", 's', 2, 2) + B("BS", 'S', 5, 2) + B("Bi", 'i', 1, 4) +
                              B("BI", 'I', 7, 4) + B("Bf", 'f', 2, 4);
    r.aux = every + Z("CB", "TTT-1");
    EXPECT(run(r.bytes(), p, &row, &cb) == BF_KEPT && cb == "TTT-1");
    r.aux = Z("CB", "G") + every;
    EXPECT(run(r.bytes(), p, &row, &cb) == BF_KEPT && cb == "G");
    r.aux = every;
    EXPECT(run(r.bytes(), p, &row) == BF_NO_BARCODE);
    r.aux = "";
    EXPECT(run(r.bytes(), p, &row) == BF_NO_BARCODE);
    r.aux = Z("CB", "first") + Z("CB", "second");
    EXPECT(run(r.bytes(), p, &row, &cb) == BF_KEPT && cb == "first");
    r.aux = Z("CB", "") + Z("CB", "second");
    EXPECT(run(r.bytes(), p, &row) == BF_NO_BARCODE);
    r.aux = std::string("CBAx") + Z("CB", "second");
    EXPECT(run(r.bytes(), p, &row) == BF_NO_BARCODE);
    r.aux = Z("CR", "raw") + Z("CB", "cell");
    BamFragParams q = p;
    q.tag[1] = 'R';
    EXPECT(run(r.bytes(), q, &row, &cb) == BF_KEPT && cb == "raw");
    // every truncation of a well-formed aux area either still gives an answer or is malformed; nothing is read outside
    const std::string full = every + Z("CB", "TTT-1");
    int kept = 0, malformed = 0, none = 0;
    for (size_t n = 0; n <= full.size(); ++n) {
        r.aux = full.substr(0, n);
        const int32_t got = run(r.bytes(), p, &row);
        kept += got == BF_KEPT, malformed += got == BF_MALFORMED, none += got == BF_NO_BARCODE;
        EXPECT(got == BF_KEPT || got == BF_MALFORMED || got == BF_NO_BARCODE);
    }
    EXPECT(kept == 1 && none > 10 && malformed > 10);
}

static void malformed() {
    const BamFragParams p = defaults();
    Rec r;
    r.tlen = 100;
    BamFragRow row;
    r.aux = std::string("XQ?abc") + Z("CB", "A");  // an unknown type
    EXPECT(run(r.bytes(), p, &row) == BF_MALFORMED);
    r.aux = std::string("CBZno-nul-in-the-record");  // in the last bytes of a block of exactly the record's size
    EXPECT(run(r.bytes(), p, &row) == BF_MALFORMED);
    r.aux = std::string("XZZalso-none");
    EXPECT(run(r.bytes(), p, &row) == BF_MALFORMED);
    r.aux = std::string("XiiAB");  // a value cut by the record's end
    EXPECT(run(r.bytes(), p, &row) == BF_MALFORMED);
    r.aux = std::string("CB");  // an entry header cut
    EXPECT(run(r.bytes(), p, &row) == BF_MALFORMED);
    r.aux = std::string("XBBi") + std::string("\xff\xff\xff\xff", 4) + std::string(8, 'x');  // a B count of 0xFFFFFFFF
    EXPECT(run(r.bytes(), p, &row) == BF_MALFORMED);
    r.aux = std::string("XBBI") + std::string("\x03\0\0\0", 4) + std::string(11, 'x');  // 3 * 4 bytes announced, 11 there
    EXPECT(run(r.bytes(), p, &row) == BF_MALFORMED);
    r.aux = std::string("XBBZ") + std::string("\0\0\0\0", 4);  // an unknown subtype
    EXPECT(run(r.bytes(), p, &row) == BF_MALFORMED);
    r.aux = std::string("XBBc") + std::string("\0\0", 2);  // the count itself is cut
    EXPECT(run(r.bytes(), p, &row) == BF_MALFORMED);
    r.aux = Z("CB", "A");
    EXPECT(run(r.bytes(0x7FFFFFFF), p, &row) == BF_MALFORMED);  // l_seq of 0x7FFFFFFF
    EXPECT(run(r.bytes(0xFFFFFFFFll), p, &row) == BF_MALFORMED);
    EXPECT(run(r.bytes(r.l_seq + 40), p, &row) == BF_MALFORMED);  // an aux start past block_size
    r.n_cigar = 0xFFFF, r.l_seq = 0, r.aux = "";
    {
        // n_cigar_op says 65535 in a record that holds none: the aux start lies far past block_size
        Rec s = r;
        s.n_cigar = 0;
        std::string b = s.bytes();
        b[4 + 12] = (char)0xFF, b[4 + 13] = (char)0xFF;
        EXPECT(run(b, p, &row) == BF_MALFORMED);
    }
    // malformed aux data behind the entry that decides is not looked at; in a record that an earlier step drops, neither
    Rec ok;
    ok.tlen = 100, ok.aux = Z("CB", "A") + std::string("XQ?");
    EXPECT(run(ok.bytes(), p, &row) == BF_KEPT);
    ok.mapq = 3, ok.aux = "XQ?";
    EXPECT(run(ok.bytes(), p, &row) == BF_MAPQ);
}

int main() {
    worked_example();
    aux_layouts();
    malformed();
    if (failures) {
        fprintf(stderr, "%d failure(s)\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
