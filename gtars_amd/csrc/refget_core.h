// refget_core.h -- the rules of K21 (refget: gtars-refget/src/digest/{alphabet,fasta,types,algorithms}.rs, store/readonly.rs)
// that the kernels, the host path and a stand-alone checking program share.  Plain C++17: no HIP include; under hipcc the
// per-byte functions are __host__ __device__.
//
//   * the alphabet class of a byte and the guess (alphabet.rs:488-527), restated from the reference's encoding arrays:
//     after ASCII upper-casing A C G T need dna2bit; N R Y dna3bit; whatever DNA_IUPAC_ENCODING_ARRAY maps to non-zero
//     (U S W K M B D H V) dnaio; whatever PROTEIN_ENCODING_ARRAY maps to non-zero, '-' and '*' (E F I L P Q X * - .)
//     protein; everything else ASCII.  The guess is the most general class seen; an empty sequence is dna2bit.
//   * refget_hash: ONE pass over a sequence's bytes, eight at a time, that upper-cases them and feeds SHA-512 (sha512.h),
//     MD5 (md5.h) and the class mask.  The two hashes pad alike up to their length fields (0x80, zeros), so the padded
//     pair is built once.  Bytes behind the sequence's end never reach a hash or the mask, whatever the source returns
//     there.  Little-endian hosts only (a pair's first byte is its low byte).
//   * the substring rule of ReadonlyRefgetStore::get_substring (readonly.rs:1292-1352).
//   * host only: the FASTA record walk (parse_fasta_reader, fasta.rs:120-306) and the canonical JSON of the collection
//     digests (algorithms.rs:59-110, types.rs:204-347).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "md5.h"
#include "sha512.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GT_RG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define GT_RG_HD inline
#endif

namespace gtars {

enum : uint8_t { RG_DNA2BIT = 0, RG_DNA3BIT = 1, RG_DNAIO = 2, RG_PROTEIN = 3, RG_ASCII = 4, RG_UNKNOWN = 5 };
enum : uint8_t { RG_SUB_OK = 0, RG_SUB_NO_SEQUENCE = 1, RG_SUB_BAD_RANGE = 2, RG_SUB_TOO_WIDE = 3 };
constexpr uint32_t RG_NONE = 0xFFFFFFFFu;

// the bytes of `s` that lie in [base, base + 64) as a bit set
constexpr uint64_t rg_bits(const char *s, unsigned base) {
    uint64_t m = 0;
    for (; *s; ++s)
        if ((unsigned char)*s >= base && (unsigned char)*s < base + 64) m |= 1ull << ((unsigned char)*s - base);
    return m;
}
constexpr uint64_t RG_D2_HI = rg_bits("ACGT", 64), RG_D3_HI = rg_bits("NRY", 64), RG_IO_HI = rg_bits("USWKMBDHV", 64);
constexpr uint64_t RG_PR_HI = rg_bits("EFILPQX*-.", 64), RG_PR_LO = rg_bits("EFILPQX*-.", 0);

// 1 << class of an upper-cased byte
GT_RG_HD uint32_t refget_class_bit(uint8_t b) {
    const uint32_t s = b & 63u;
    const bool hi = (b & 0xC0u) == 0x40u, lo = b < 64;
    const uint32_t d2 = hi ? (uint32_t)(RG_D2_HI >> s) & 1u : 0u;
    const uint32_t d3 = hi ? (uint32_t)(RG_D3_HI >> s) & 1u : 0u;
    const uint32_t io = hi ? (uint32_t)(RG_IO_HI >> s) & 1u : 0u;
    const uint32_t pr = hi ? (uint32_t)(RG_PR_HI >> s) & 1u : lo ? (uint32_t)(RG_PR_LO >> s) & 1u : 0u;
    const uint32_t known = d2 | (d3 << 1) | (io << 2) | (pr << 3);
    return known ? known : 1u << RG_ASCII;
}

GT_RG_HD uint8_t refget_upper(uint8_t b) { return b >= 'a' && b <= 'z' ? (uint8_t)(b - 32) : b; }

// the class of a raw byte: of its upper-cased form (AlphabetGuesser::update)
GT_RG_HD uint8_t refget_class(uint8_t b) {
    const uint32_t bit = refget_class_bit(refget_upper(b));
    return (uint8_t)(bit & 16u ? 4 : bit & 8u ? 3 : bit & 4u ? 2 : bit & 2u ? 1 : 0);
}

// the guess of a mask of class bits: the most general class in it
GT_RG_HD uint8_t refget_guess(uint32_t mask) {
    return (uint8_t)(mask & 16u ? RG_ASCII : mask & 8u ? RG_PROTEIN : mask & 4u ? RG_DNAIO : mask & 2u ? RG_DNA3BIT : RG_DNA2BIT);
}

// eight bytes upper-cased at once: a byte in 'a' .. 'z' loses 0x20
GT_RG_HD uint64_t refget_upper8(uint64_t x) {
    const uint64_t ones = 0x0101010101010101ull, top = 0x8080808080808080ull;
    const uint64_t low7 = x & ~top;
    const uint64_t ge_a = low7 + (0x80 - 'a') * ones, gt_z = low7 + (0x80 - 'z' - 1) * ones;  // (no carry leaves a byte)
    return x - ((ge_a & ~gt_z & ~x & top) >> 2);
}

// sha512t24u, MD5 and the class mask of `len` bytes.  Src: `uint64_t pair(uint64_t c)` gives bytes [8 c, 8 c + 8) of the
// sequence, the first in the low byte; it is asked for c = 0, 1, ... in order, only while 8 c < len, and whatever it holds
// behind len is dropped here.
template <class Src>
GT_RG_HD void refget_hash(Src &src, uint64_t len, Sha512 &sh, Md5 &md, uint32_t &mask) {
    sha512_init(sh);
    md5_init(md);
    uint32_t seen = 0;
    const uint64_t n_sha = (len + 17 + 127) >> 7, n_md5 = 8 * md5_blocks(len);  // (16 n_sha >= n_md5)
#if defined(__clang__)
#pragma unroll 1
#endif
    for (uint64_t blk = 0; blk < n_sha; ++blk) {
#if defined(__clang__)
#pragma unroll 1
#endif
        for (int wi = 0; wi < 16; ++wi) {
            const uint64_t c = (blk << 4) + (uint64_t)wi, at = c << 3;
            uint64_t d = 0;
            if (at < len) {
                const uint64_t rem = len - at;
                d = refget_upper8(src.pair(c));
                uint32_t valid = 8;
                if (rem < 8) {
                    valid = (uint32_t)rem;
                    d = (d & ((1ull << (8 * rem)) - 1)) | (0x80ull << (8 * rem));
                }
#if defined(__clang__)
#pragma unroll
#endif
                for (uint32_t k = 0; k < 8; ++k)
                    if (k < valid) seen |= refget_class_bit((uint8_t)(d >> (8 * k)));
            } else if (at == len) {
                d = 0x80;
            }
            sha512_push(sh, blk + 1 == n_sha && wi == 15 ? len << 3 : __builtin_bswap64(d));
            // (the last eight words of SHA-512's ring are MD5's block, byte-swapped: MD5 keeps no ring of its own here; the one
            // pair the two hashes may differ in, a length field, is the eighth)
            if (c < n_md5 && (c & 7) == 7)
                md5_compress(md.h, __builtin_bswap64(sh.w[8]), __builtin_bswap64(sh.w[9]), __builtin_bswap64(sh.w[10]), __builtin_bswap64(sh.w[11]),
                             __builtin_bswap64(sh.w[12]), __builtin_bswap64(sh.w[13]), __builtin_bswap64(sh.w[14]), md5_padded_pair(d, c, len));
        }
        sha512_block(sh);
    }
    mask = seen;
}

// a sequence in host memory (no readable bytes behind it are assumed)
struct RefgetHostSrc {
    const uint8_t *p;
    uint64_t len;
    uint64_t pair(uint64_t c) const {
        const uint64_t at = c << 3;
        uint64_t v = 0;
        memcpy(&v, p + at, (size_t)(len - at < 8 ? len - at : 8));
        return v;
    }
};

// what one record's pass leaves: the 32 digest characters, the 16 MD5 bytes, the class
struct RefgetDigest {
    char text[32];
    uint8_t md5[16];
    uint8_t cls;
};

inline void refget_digest_host(const uint8_t *p, uint64_t len, RefgetDigest &out) {
    RefgetHostSrc src{p, len};
    Sha512 sh;
    Md5 md;
    uint32_t mask;
    refget_hash(src, len, sh, md, mask);
    sha512t24u_text(sh, out.text);
    md5_bytes(md, out.md5);
    out.cls = refget_guess(mask);
}

// get_substring's rule: [start, start) is the empty string wherever start lies; every other range needs
// start < end, start < len and end <= len.  -> status and the bytes of the row (rows wider than 2^32 - 1 bytes do not fit
// one call's u32 counts)
GT_RG_HD uint8_t refget_sub_status(uint64_t start, uint64_t end, uint64_t len, uint32_t *bytes) {
    *bytes = 0;
    if (start == end) return RG_SUB_OK;
    if (start >= len || end > len || start >= end) return RG_SUB_BAD_RANGE;
    if (end - start > 0xFFFFFFFFull) return RG_SUB_TOO_WIDE;
    *bytes = (uint32_t)(end - start);
    return RG_SUB_OK;
}

// ---- host only ------------------------------------------------------------------------------------------------------

inline bool rg_is_ws(char ch) { return ch == ' ' || (ch >= '\t' && ch <= '\r'); }  // (the ASCII part of char::is_whitespace)

// one record of a FASTA text, in file order; its sequence is blob[off, off + len): the trimmed lines back to back, as the
// file has them (not upper-cased)
struct RefgetRecord {
    std::string name, description;
    bool has_description = false;
    uint64_t off = 0, len = 0;
    bool has_fai = false;  // a record without a sequence line has none
    uint64_t fai_offset = 0;
    uint32_t line_bases = 0, line_bytes = 0;
};

// parse_fasta_reader: a header is a line whose FIRST byte is '>'; text before the first header is ignored; the name is the
// first whitespace-delimited token of the trimmed header, the description the trimmed rest (none without one); a sequence
// line is a line that is not blank, taken without its trailing whitespace; line_bases / line_bytes are those of the
// record's first sequence line (line_bytes with its line end), offset is the position just behind the header line.
// Records stay in file order, a repeated name stays a record of its own.
inline void refget_walk_fasta(const char *text, size_t n, std::string &blob, std::vector<RefgetRecord> &recs) {
    size_t at = 0;
    while (at < n) {
        const char *nl = (const char *)memchr(text + at, '\n', n - at);
        const size_t line_end = nl ? (size_t)(nl - text) + 1 : n;  // (read_line: the line end belongs to the line)
        const char *line = text + at;
        const size_t bytes_read = line_end - at;
        at = line_end;
        if (line[0] == '>') {
            size_t b = 1, e = bytes_read;
            while (b < e && rg_is_ws(line[b])) ++b;
            while (e > b && rg_is_ws(line[e - 1])) --e;
            size_t k = b;
            while (k < e && !rg_is_ws(line[k])) ++k;
            RefgetRecord r;
            r.name.assign(line + b, k - b);
            if (k < e) {
                size_t d = k + 1;
                while (d < e && rg_is_ws(line[d])) ++d;
                r.has_description = true;
                r.description.assign(line + d, e - d);
            }
            r.off = blob.size();
            r.fai_offset = at;
            recs.push_back(std::move(r));
            continue;
        }
        if (recs.empty()) continue;
        size_t e = bytes_read;
        while (e && rg_is_ws(line[e - 1])) --e;
        if (!e) continue;  // a blank line
        RefgetRecord &r = recs.back();
        if (!r.has_fai) r.has_fai = true, r.line_bases = (uint32_t)e, r.line_bytes = (uint32_t)bytes_read;
        blob.append(line, e);
        r.len += e;
    }
}

// serde_json's string: '"' and '\\' escaped, \b \f \n \r \t by name, other control bytes as \u00XX, the rest (UTF-8
// included) as it is
inline void rg_json_string(std::string &out, const std::string &s) {
    out.push_back('"');
    for (const char ch : s) {
        const unsigned char c = (unsigned char)ch;
        if (c == '"') out += "\\\"";
        else if (c == '\\') out += "\\\\";
        else if (c == '\b') out += "\\b";
        else if (c == '\f') out += "\\f";
        else if (c == '\n') out += "\\n";
        else if (c == '\r') out += "\\r";
        else if (c == '\t') out += "\\t";
        else if (c < 0x20) {
            const char hex[] = "0123456789abcdef";
            out += "\\u00";
            out.push_back(hex[c >> 4]);
            out.push_back(hex[c & 15]);
        } else out.push_back(ch);
    }
    out.push_back('"');
}

inline std::string rg_digest_of(const std::string &text) {
    char d[32];
    sha512t24u((const uint8_t *)text.data(), text.size(), d);
    return std::string(d, 32);
}

inline std::string rg_json_strings(const std::vector<std::string> &v) {
    std::string out = "[";
    for (size_t i = 0; i < v.size(); ++i) {
        if (i) out.push_back(',');
        rg_json_string(out, v[i]);
    }
    out.push_back(']');
    return out;
}

// the seven digests of a collection, 32 characters each
struct RefgetColDigests {
    std::string top, names, sequences, lengths, name_length_pairs, sorted_name_length_pairs, sorted_sequences;
};

// names / lengths / digests (32 characters, no prefix) of the records in order
inline void refget_collection_digests(const std::vector<std::string> &names, const std::vector<uint64_t> &lengths,
                                      const std::vector<std::string> &digests, RefgetColDigests &out) {
    const size_t n = names.size();
    std::vector<std::string> seqs(n), pairs(n), pair_digests(n);
    std::string len_json = "[";
    for (size_t i = 0; i < n; ++i) {
        seqs[i] = "SQ." + digests[i];
        if (i) len_json.push_back(',');
        len_json += std::to_string(lengths[i]);
        pairs[i] = "{\"length\":" + std::to_string(lengths[i]) + ",\"name\":";
        rg_json_string(pairs[i], names[i]);
        pairs[i].push_back('}');
        pair_digests[i] = rg_digest_of(pairs[i]);
    }
    len_json.push_back(']');
    out.sequences = rg_digest_of(rg_json_strings(seqs));
    out.names = rg_digest_of(rg_json_strings(names));
    out.lengths = rg_digest_of(len_json);
    std::string top = "{\"names\":";
    rg_json_string(top, out.names);
    top += ",\"sequences\":";
    rg_json_string(top, out.sequences);
    top.push_back('}');
    out.top = rg_digest_of(top);
    std::string nlp = "[";
    for (size_t i = 0; i < n; ++i) {
        if (i) nlp.push_back(',');
        nlp += pairs[i];
    }
    nlp.push_back(']');
    out.name_length_pairs = rg_digest_of(nlp);
    std::sort(pair_digests.begin(), pair_digests.end());
    out.sorted_name_length_pairs = rg_digest_of(rg_json_strings(pair_digests));
    std::sort(seqs.begin(), seqs.end());
    out.sorted_sequences = rg_digest_of(rg_json_strings(seqs));
}

}  // namespace gtars
