// reftx_core.h -- the rules of K19 as plain C++17 (no HIP includes, no library state), so that reftx.cpp, the kernels of
// reftx.hip, the host tail of the digest kernel and a stand-alone checking program share one text: the transcript model
// (gtars-refget/src/transcripts/models.rs), the .reftx v2 container (store.rs), the coordinate mapper (mapper.rs:239-475)
// and the byte rule of the mature mRNA (sequence.rs:36-127).  Under hipcc the functions the kernels call are
// __host__ __device__; under a host compiler they are ordinary inline functions.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "sha512.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GT_TX_HD __host__ __device__ inline
#else
#define GT_TX_HD inline
#endif

namespace gtars {

// per-query status of the mapping calls: 1 .. 7 are MappingError's kinds (mapper.rs:19-50; NoManeTranscript is the by-gene
// call's and has no row form), 8 is g_to_transcript_offset's None, 9 and 10 are the columns' own
enum : uint8_t {
    TX_OK = 0,
    TX_NOT_FOUND = 1,           // transcript index outside the store (an unknown accession is index 2^32 - 1)
    TX_NON_CODING = 2,          // c. on a transcript without CDS, or whose CDS ends do not lie in exons
    TX_OUTSIDE_CDS = 3,         // c.N past the CDS end, c.0
    TX_OUTSIDE_TRANSCRIPT = 4,  // n.N <= 0 or past the transcript's end
    TX_UTR5_OVERFLOW = 5,       // c.-N before the transcript's first base
    TX_UTR3_OVERFLOW = 6,       // c.*N with N <= 0 or past the transcript's last base
    TX_INVALID_OFFSET = 7,      // an intronic offset away from an exon boundary, or one that leaves u64
    TX_NOT_EXONIC = 8,          // g. -> transcript offset: the position lies in no exon
    TX_BAD_KIND = 9,
    TX_BAD_EXONS = 10,          // the transcript's exons are not ascending and disjoint (start <= end <= next start)
};
enum : uint8_t { TX_KIND_C = 0, TX_KIND_N = 1, TX_KIND_G = 2 };

// per-row status of the sequence calls
enum : uint8_t {
    TXSEQ_OK = 0,
    TXSEQ_NOT_FOUND = 1,    // transcript index outside the store
    TXSEQ_NO_SEQUENCE = 2,  // the assembly has no chromosome with the transcript's digest ("Sequence not found")
    TXSEQ_PAST_END = 3,     // an exon reaches past the chromosome's end (transcript / assembly mismatch)
    TXSEQ_BAD_EXONS = 4,
};

constexpr uint32_t TX_NONE = 0xFFFFFFFFu;

// The mapping tables of a store: host vectors or device arrays.  Exons stand in genomic order, transcript t's are
// [exon_off[t], exon_off[t + 1]); tx_start is the exon's first base in transcript coordinates (0-based), so for a
// reverse-strand transcript it descends with the index.  Ascending disjoint exons keep every sum below 2^32.
struct TxTables {
    const uint32_t *exon_off = nullptr;                                      // [n_tx + 1]
    const uint32_t *g_start = nullptr, *g_end = nullptr, *tx_start = nullptr;  // per exon
    const uint32_t *chrom = nullptr;                                         // [n_tx] chromosome id of the bound assembly, TX_NONE: none
    const int8_t *strand = nullptr;                                          // [n_tx] +1 / -1
    const uint32_t *cds_lo = nullptr, *cds_hi = nullptr;                     // [n_tx] the CDS in transcript coordinates, cds_lo TX_NONE: non-coding
    const uint32_t *len = nullptr;                                           // [n_tx] transcript length
    const uint8_t *bad = nullptr;                                            // [n_tx] 1: TX_BAD_EXONS
    const uint8_t *seq_status = nullptr;                                     // [n_tx] TXSEQ_* of the bound assembly
    uint32_t n_tx = 0;
};

// one transcript's exons in TRANSCRIPT order: j = 0 is the 5' exon
struct TxExons {
    const uint32_t *gs, *ge, *ts;
    uint32_t n;
    bool fwd;
    GT_TX_HD uint32_t at(uint32_t j) const { return fwd ? j : n - 1 - j; }
};
GT_TX_HD TxExons tx_exons(const TxTables &t, uint32_t tx) {
    const uint32_t e0 = t.exon_off[tx];
    return TxExons{t.g_start + e0, t.g_end + e0, t.tx_start + e0, t.exon_off[tx + 1] - e0, t.strand[tx] > 0};
}

// the exon that holds transcript position pos < length, as its index in transcript order: the last one that starts at or
// before pos (an empty exon shares its start with the exon behind it, so the last one is the one with bases)
GT_TX_HD uint32_t tx_exon_of(const TxExons &x, uint64_t pos) {
    uint32_t lo = 0, hi = x.n;
    while (hi - lo > 1) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        if (x.ts[x.at(m)] <= pos) lo = m;
        else hi = m;
    }
    return lo;
}

// genomic position -> transcript position (genomic_to_transcript_fast); false: in no exon
GT_TX_HD bool tx_from_genomic(const TxExons &x, uint64_t g, uint64_t *out) {
    if (!x.n || g < x.gs[0]) return false;
    uint32_t lo = 0, hi = x.n;  // the last exon in genomic order that starts at or before g
    while (hi - lo > 1) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        if (x.gs[m] <= g) lo = m;
        else hi = m;
    }
    if (g >= x.ge[lo]) return false;
    *out = (uint64_t)x.ts[lo] + (x.fwd ? g - x.gs[lo] : (uint64_t)x.ge[lo] - 1 - g);
    return true;
}

// One query (c_to_g_inner, n_to_g_inner, apply_offset_to_tx_pos, g_to_transcript_offset).  kind C: HGVS c.pos, c.*pos with
// `star`, intronic offset `off`; kind N: n.pos with `off`; kind G: pos is a 0-based genomic position (read as u64) and the
// result its 0-based offset on the mature mRNA.  *out is 0 unless the status is TX_OK.
GT_TX_HD uint8_t tx_map_one(const TxTables &t, uint32_t tx, uint32_t kind, int64_t pos, int64_t off, uint32_t star, uint64_t *out) {
    *out = 0;
    if (tx >= t.n_tx) return TX_NOT_FOUND;
    if (kind > TX_KIND_G) return TX_BAD_KIND;
    if (t.bad[tx]) return TX_BAD_EXONS;
    const TxExons x = tx_exons(t, tx);
    const uint64_t len = t.len[tx];
    if (kind == TX_KIND_G) {
        uint64_t r;
        if (!tx_from_genomic(x, (uint64_t)pos, &r)) return TX_NOT_EXONIC;
        *out = r;
        return TX_OK;
    }
    uint64_t p;
    if (kind == TX_KIND_C) {
        const uint64_t lo = t.cds_lo[tx], hi = t.cds_hi[tx];
        if (lo == TX_NONE) return TX_NON_CODING;
        if (star) {
            if (pos <= 0) return TX_UTR3_OVERFLOW;
            p = hi + ((uint64_t)pos - 1);  // (hi < 2^32, pos < 2^63: no carry out of u64)
            if (p >= len) return TX_UTR3_OVERFLOW;
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
        if (pos <= 0) return TX_OUTSIDE_TRANSCRIPT;
        p = (uint64_t)pos - 1;
        if (p >= len) return TX_OUTSIDE_TRANSCRIPT;
    }
    const uint32_t j = tx_exon_of(x, p), k = x.at(j);
    const uint64_t ts = x.ts[k], te = ts + (x.ge[k] - x.gs[k]);
    const uint64_t anchor = x.fwd ? (uint64_t)x.gs[k] + (p - ts) : (uint64_t)x.ge[k] - 1 - (p - ts);
    if (off == 0) {
        *out = anchor;
        return TX_OK;
    }
    // is_exon_boundary: the last base of an exon that is not the last for a positive offset, the first base of an exon that
    // is not the first for a negative one (empty exons next to this one change neither answer)
    const bool positive = off > 0;
    if (positive ? !(p + 1 == te && j + 1 < x.n) : !(p == ts && j > 0)) return TX_INVALID_OFFSET;
    const uint64_t mag = positive ? (uint64_t)off : 0 - (uint64_t)off;
    if (positive == x.fwd) {
        if (anchor + mag < anchor) return TX_INVALID_OFFSET;  // checked_add
        *out = anchor + mag;
    } else {
        if (mag > anchor) return TX_INVALID_OFFSET;  // checked_sub
        *out = anchor - mag;
    }
    return TX_OK;
}

GT_TX_HD uint32_t tx_upper(uint32_t b) { return b - 97u < 26u ? b - 32u : b; }
// reverse_complement's table over upper-cased bytes: anything outside ACGTN is N
GT_TX_HD uint32_t tx_complement(uint32_t b) {
    return b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : b == 'G' ? 'C' : 'N';
}

// byte k < length of a transcript's mature sequence, and the streaming form: the exons forward as the chromosome has them
// (upper-cased), or backward with the complement.  seq: the chromosome's first byte.
GT_TX_HD uint32_t tx_base(const TxExons &x, const uint8_t *seq, uint32_t k_exon, uint64_t within) {
    return x.fwd ? tx_upper(seq[(uint64_t)x.gs[k_exon] + within]) : tx_complement(tx_upper(seq[(uint64_t)x.ge[k_exon] - 1 - within]));
}
struct TxSeqSrc {  // a sha512_stream source; next() is called length times
    TxExons x;
    const uint8_t *seq;
    uint32_t j = 0;        // next exon in transcript order
    uint32_t left = 0;     // bytes left in the current one
    uint64_t pos = 0;      // forward: the next byte; reverse: one behind the next byte
    GT_TX_HD uint8_t next() {
        while (left == 0) {
            const uint32_t k = x.at(j++);
            left = x.ge[k] - x.gs[k];
            pos = x.fwd ? x.gs[k] : x.ge[k];
        }
        --left;
        uint32_t b;
        if (x.fwd) b = tx_upper(seq[pos++]);
        else b = tx_complement(tx_upper(seq[--pos]));
        return (uint8_t)b;
    }
};

// ---- the model and the container: host only --------------------------------------------------------------------------
struct TxExon {
    uint32_t start, end;  // 0-based half-open
};
struct TxRecord {
    std::string accession, gene;
    uint8_t chrom_digest[24] = {};
    int8_t strand = 1;
    uint8_t mane = 0;  // bit 0 MANE Select, bit 1 MANE Plus Clinical
    uint32_t cds_start = TX_NONE, cds_end = TX_NONE;  // TX_NONE: none
    std::vector<TxExon> exons;
    bool is_coding() const { return cds_start != TX_NONE && cds_end != TX_NONE; }
    uint32_t transcript_length() const {
        uint32_t n = 0;
        for (const TxExon &e : exons) n += e.end - e.start;
        return n;
    }
    uint32_t cds_length() const {
        if (!is_coding()) return 0;
        uint32_t n = 0;
        for (const TxExon &e : exons) {
            const uint32_t s = std::max(e.start, cds_start), t = std::min(e.end, cds_end);
            if (s < t) n += t - s;
        }
        return n;
    }
};

inline uint64_t tx_fnv1a(const void *data, size_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t *)data)[i]) * 0x100000001b3ull;
    return h;
}
inline std::string tx_ascii_upper(const std::string &s) {
    std::string u = s;
    for (char &c : u)
        if (c >= 'a' && c <= 'z') c = (char)(c - 32);
    return u;
}

// base64url without padding <-> 24 bytes ("SQ." is optional in front).  False: not base64url, or not 24 bytes; *n_bytes
// (may be null) is how many bytes the text decodes to, or -1 for a character outside the alphabet / an impossible length.
inline bool tx_digest_decode(const char *text, size_t n, uint8_t out[24], long *n_bytes = nullptr) {
    if (n >= 3 && memcmp(text, "SQ.", 3) == 0) text += 3, n -= 3;
    while (n && text[n - 1] == '=') --n;  // (padding is tolerated)
    if (n_bytes) *n_bytes = -1;
    if (n % 4 == 1) return false;
    uint32_t acc = 0, bits = 0;
    uint8_t buf[24];
    size_t got = 0;
    for (size_t i = 0; i < n; ++i) {
        const char c = text[i];
        int v;
        if (c >= 'A' && c <= 'Z') v = c - 'A';
        else if (c >= 'a' && c <= 'z') v = c - 'a' + 26;
        else if (c >= '0' && c <= '9') v = c - '0' + 52;
        else if (c == '-') v = 62;
        else if (c == '_') v = 63;
        else return false;
        acc = (acc << 6) | (uint32_t)v, bits += 6;
        if (bits >= 8) {
            bits -= 8;
            if (got < 24) buf[got] = (uint8_t)(acc >> bits);
            ++got;
        }
    }
    if (n_bytes) *n_bytes = (long)got;
    if (got != 24) return false;
    memcpy(out, buf, 24);
    return true;
}
inline void tx_digest_encode(const uint8_t d[24], char out[32]) {
    for (int q = 0; q < 8; ++q) {
        const uint32_t v = ((uint32_t)d[3 * q] << 16) | ((uint32_t)d[3 * q + 1] << 8) | d[3 * q + 2];
        for (int k = 0; k < 4; ++k) out[4 * q + k] = sha512_b64((v >> (18 - 6 * k)) & 63u);
    }
}

// The .reftx v2 image: 40-byte header (RFTX, version 2, record count, index offset, MANE index offset, 8 reserved), the
// records in ascending FNV-1a order of their accessions, the accession index (hash, record offset), then -- only when a
// record is MANE Select -- a count and the index keyed by the upper-cased gene, ascending too.  Empty string: `err` says why.
constexpr size_t TX_HEADER = 40, TX_INDEX_ENTRY = 16;
inline void tx_put(std::string &out, uint64_t v, int bytes) {
    for (int i = 0; i < bytes; ++i) out.push_back((char)(v >> (8 * i)));
}
inline bool tx_encode(const std::vector<TxRecord> &recs, std::string &out, std::string &err) {
    std::vector<std::pair<uint64_t, size_t>> order(recs.size());
    for (size_t i = 0; i < recs.size(); ++i) order[i] = {tx_fnv1a(recs[i].accession.data(), recs[i].accession.size()), i};
    std::stable_sort(order.begin(), order.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    out.assign(TX_HEADER, '\0');
    std::vector<std::pair<uint64_t, uint64_t>> index, mane;
    for (const auto &o : order) {
        const TxRecord &r = recs[o.second];
        if (r.accession.size() > 255 || r.gene.size() > 255) {
            const bool acc = r.accession.size() > 255;
            const std::string &s = acc ? r.accession : r.gene;
            err = std::string(acc ? "accession \"" : "gene \"") + s + "\" is " + std::to_string(s.size()) + " bytes; exceeds 255-byte .reftx limit";
            return false;
        }
        if (r.exons.size() > 65535) {
            err = "transcript \"" + r.accession + "\" has " + std::to_string(r.exons.size()) + " exons; exceeds 65535-exon .reftx limit";
            return false;
        }
        const uint64_t at = out.size();
        index.push_back({o.first, at});
        if (r.mane & 1) {
            const std::string g = tx_ascii_upper(r.gene);
            mane.push_back({tx_fnv1a(g.data(), g.size()), at});
        }
        out.push_back((char)r.accession.size());
        out += r.accession;
        out.push_back((char)r.gene.size());
        out += r.gene;
        out.append((const char *)r.chrom_digest, 24);
        out.push_back((char)r.strand);
        out.push_back((char)r.mane);
        tx_put(out, r.cds_start, 4), tx_put(out, r.cds_end, 4);
        tx_put(out, r.exons.size(), 2);
        for (const TxExon &e : r.exons) tx_put(out, e.start, 4), tx_put(out, e.end, 4);
    }
    const uint64_t index_off = out.size();
    for (const auto &e : index) tx_put(out, e.first, 8), tx_put(out, e.second, 8);
    uint64_t mane_off = 0;
    if (!mane.empty()) {
        std::stable_sort(mane.begin(), mane.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
        mane_off = out.size();
        tx_put(out, mane.size(), 8);
        for (const auto &e : mane) tx_put(out, e.first, 8), tx_put(out, e.second, 8);
    }
    std::string head;
    head += "RFTX";
    tx_put(head, 2, 4), tx_put(head, recs.size(), 8), tx_put(head, index_off, 8), tx_put(head, mane_off, 8), tx_put(head, 0, 8);
    out.replace(0, TX_HEADER, head);
    return true;
}

// A decoded store.  Decoding reads `n` bytes at `data` and nothing else: every length is checked against what is left before
// it is used.  Unlike the reference, which decodes a record when it is looked up and answers None for one it cannot read, the
// whole file is decoded when it is opened and a record that does not fit is an error of the open.
struct TxStoreData {
    std::vector<TxRecord> recs;                        // in index order
    std::vector<uint64_t> hash;                        // [recs] ascending
    std::vector<std::pair<uint64_t, uint32_t>> mane;   // (hash of the upper-cased gene, record), ascending
    bool has_mane = false;

    static uint64_t le(const uint8_t *p, int bytes) {
        uint64_t v = 0;
        for (int i = 0; i < bytes; ++i) v |= (uint64_t)p[i] << (8 * i);
        return v;
    }
    // one record at data[at, bound); false: it does not fit
    static bool read_record(const uint8_t *data, uint64_t at, uint64_t bound, TxRecord &r) {
        uint64_t left = bound - at;
        const uint8_t *p = data + at;
        auto take = [&](uint64_t k) -> const uint8_t * {
            if (k > left) return nullptr;
            const uint8_t *q = p;
            p += k, left -= k;
            return q;
        };
        const uint8_t *q;
        if (!(q = take(1))) return false;
        const uint64_t n_acc = *q;
        if (!(q = take(n_acc))) return false;
        r.accession.assign((const char *)q, n_acc);
        if (!(q = take(1))) return false;
        const uint64_t n_gene = *q;
        if (!(q = take(n_gene))) return false;
        r.gene.assign((const char *)q, n_gene);
        if (!(q = take(24))) return false;
        memcpy(r.chrom_digest, q, 24);
        if (!(q = take(2))) return false;
        r.strand = (int8_t)q[0], r.mane = q[1];
        if (r.strand != 1 && r.strand != -1) return false;
        if (!(q = take(10))) return false;
        r.cds_start = (uint32_t)le(q, 4), r.cds_end = (uint32_t)le(q + 4, 4);
        const uint64_t n_exons = le(q + 8, 2);
        if (!(q = take(8 * n_exons))) return false;
        r.exons.resize(n_exons);
        for (uint64_t i = 0; i < n_exons; ++i) r.exons[i] = TxExon{(uint32_t)le(q + 8 * i, 4), (uint32_t)le(q + 8 * i + 4, 4)};
        return true;
    }
    bool decode(const uint8_t *data, uint64_t n, std::string &err) {
        if (n < TX_HEADER) return err = "File too small for header", false;
        if (memcmp(data, "RFTX", 4) != 0) return err = "Invalid magic number: expected RFTX", false;
        const uint64_t version = le(data + 4, 4);
        if (version != 2) return err = "Unsupported format version: " + std::to_string(version), false;
        const uint64_t count = le(data + 8, 8), index_off = le(data + 16, 8), mane_off = le(data + 24, 8);
        if (index_off < TX_HEADER || index_off > n || count > (n - index_off) / TX_INDEX_ENTRY)
            return err = "Truncated .reftx file: the accession index does not fit", false;
        const uint64_t index_end = index_off + count * TX_INDEX_ENTRY;
        uint64_t n_mane = 0;
        if (mane_off) {
            if (mane_off < index_end || mane_off > n || n - mane_off < 8) return err = "Truncated .reftx file: the MANE index does not fit", false;
            n_mane = le(data + mane_off, 8);
            if (n_mane > (n - mane_off - 8) / TX_INDEX_ENTRY) return err = "Truncated .reftx file: the MANE index does not fit", false;
        }
        if (count >= 0xFFFFFFFFull) return err = "too many transcripts in one .reftx file", false;
        recs.assign((size_t)count, TxRecord());
        hash.assign((size_t)count, 0);
        std::vector<std::pair<uint64_t, uint32_t>> by_offset((size_t)count);
        for (uint64_t i = 0; i < count; ++i) {
            const uint8_t *e = data + index_off + i * TX_INDEX_ENTRY;
            hash[i] = le(e, 8);
            const uint64_t at = le(e + 8, 8);
            if (i && hash[i] < hash[i - 1]) return err = "Corrupt .reftx file: the accession index is not sorted", false;
            if (at < TX_HEADER || at > index_off || !read_record(data, at, index_off, recs[i]))
                return err = "Truncated .reftx file: record " + std::to_string(i) + " does not fit", false;
            by_offset[i] = {at, (uint32_t)i};
        }
        std::sort(by_offset.begin(), by_offset.end());
        has_mane = mane_off != 0;
        mane.assign((size_t)n_mane, {0, 0});
        for (uint64_t i = 0; i < n_mane; ++i) {
            const uint8_t *e = data + mane_off + 8 + i * TX_INDEX_ENTRY;
            const uint64_t h = le(e, 8), at = le(e + 8, 8);
            auto it = std::lower_bound(by_offset.begin(), by_offset.end(), std::make_pair(at, (uint32_t)0));
            if (it == by_offset.end() || it->first != at) return err = "Corrupt .reftx file: a MANE entry points at no record", false;
            if (i && h < mane[i - 1].first) return err = "Corrupt .reftx file: the MANE index is not sorted", false;
            mane[i] = {h, it->second};
        }
        return true;
    }
    // record index of an accession, -1: none (the entries of one hash are neighbours: the reference's linear probe)
    int64_t lookup(const char *acc, size_t n) const {
        const uint64_t h = tx_fnv1a(acc, n);
        for (size_t i = (size_t)(std::lower_bound(hash.begin(), hash.end(), h) - hash.begin()); i < hash.size() && hash[i] == h; ++i)
            if (recs[i].accession.size() == n && memcmp(recs[i].accession.data(), acc, n) == 0) return (int64_t)i;
        return -1;
    }
    int64_t lookup_mane(const std::string &gene) const {
        const std::string g = tx_ascii_upper(gene);
        const uint64_t h = tx_fnv1a(g.data(), g.size());
        auto it = std::lower_bound(mane.begin(), mane.end(), std::make_pair(h, (uint32_t)0));
        for (; it != mane.end() && it->first == h; ++it)
            if (tx_ascii_upper(recs[it->second].gene) == g) return (int64_t)it->second;
        return -1;
    }
};

// the mapping tables of a decoded store as host vectors (chrom / seq_status are the binding's and start out "none")
struct TxHostTables {
    std::vector<uint32_t> exon_off, g_start, g_end, tx_start, chrom, cds_lo, cds_hi, len;
    std::vector<int8_t> strand;
    std::vector<uint8_t> bad, seq_status;
    TxTables view() const {
        TxTables t;
        t.exon_off = exon_off.data(), t.g_start = g_start.data(), t.g_end = g_end.data(), t.tx_start = tx_start.data();
        t.chrom = chrom.data(), t.strand = strand.data(), t.cds_lo = cds_lo.data(), t.cds_hi = cds_hi.data(), t.len = len.data();
        t.bad = bad.data(), t.seq_status = seq_status.data(), t.n_tx = (uint32_t)len.size();
        return t;
    }
    // false: more than 2^32 - 1 exons
    bool build(const std::vector<TxRecord> &recs) {
        const size_t n = recs.size();
        size_t total = 0;
        for (const TxRecord &r : recs) total += r.exons.size();
        if (total >= 0xFFFFFFFFull) return false;
        exon_off.assign(n + 1, 0);
        g_start.resize(total), g_end.resize(total), tx_start.resize(total);
        chrom.assign(n, TX_NONE), cds_lo.assign(n, TX_NONE), cds_hi.assign(n, TX_NONE), len.assign(n, 0), strand.assign(n, 1);
        bad.assign(n, 0), seq_status.assign(n, TXSEQ_NO_SEQUENCE);
        size_t at = 0;
        for (size_t t = 0; t < n; ++t) {
            const TxRecord &r = recs[t];
            const size_t ne = r.exons.size();
            strand[t] = r.strand;
            bool ok = true;
            for (size_t k = 0; k < ne; ++k) {
                g_start[at + k] = r.exons[k].start, g_end[at + k] = r.exons[k].end;
                ok &= r.exons[k].start <= r.exons[k].end && (k == 0 || r.exons[k - 1].end <= r.exons[k].start);
            }
            bad[t] = !ok;
            if (ok) {
                uint32_t pos = 0;
                for (size_t j = 0; j < ne; ++j) {
                    const size_t k = r.strand > 0 ? j : ne - 1 - j;
                    tx_start[at + k] = pos;
                    pos += r.exons[k].end - r.exons[k].start;
                }
                len[t] = pos;
            }
            at += ne;
            exon_off[t + 1] = (uint32_t)at;
        }
        // cds_tx_bounds: both CDS ends through the exons; the smaller transcript position is the CDS start on either strand
        const TxTables v = view();
        for (size_t t = 0; t < n; ++t) {
            const TxRecord &r = recs[t];
            if (bad[t] || !r.is_coding() || r.cds_end == 0) continue;
            const TxExons x = tx_exons(v, (uint32_t)t);
            uint64_t a, b;
            if (!tx_from_genomic(x, r.cds_start, &a) || !tx_from_genomic(x, r.cds_end - 1, &b)) continue;
            cds_lo[t] = (uint32_t)std::min(a, b), cds_hi[t] = (uint32_t)std::max(a, b) + 1;
        }
        return true;
    }
};

// a transcript's mature sequence and its sha512t24u on the host (seq: the chromosome's first byte)
inline void tx_sequence(const TxTables &t, uint32_t tx, const uint8_t *seq, std::string &out) {
    TxSeqSrc src{tx_exons(t, tx), seq};
    out.resize(t.len[tx]);
    for (char &c : out) c = (char)src.next();
}
inline void tx_digest(const TxTables &t, uint32_t tx, const uint8_t *seq, char out[32]) {
    TxSeqSrc src{tx_exons(t, tx), seq};
    Sha512 s;
    sha512_stream(s, src, t.len[tx]);
    sha512t24u_text(s, out);
}

}  // namespace gtars
