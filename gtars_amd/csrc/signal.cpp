// signal.cpp -- signal matrices on the host (SignalMatrix, gtars-genomicdist/src/signal.rs:33-354: the TSV reader and
// the packed SIGM format) and the library calls of K13 on top of signal.hip: calc_summary_signal (signal.rs:356-454).
// Declared in include/gtars_amd_host.h, where the readers' rules are written down.  Region sets are read through their
// public accessors.
#include <cerrno>
#include <charconv>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/gtars_amd_debug.h"
#include "../../include/gtars_amd_host.h"
#include "guard.h"
#include "signal.h"

using gtars::fail;
using gtars::guarded;

struct gtars_signal {
    std::vector<std::string> names;  // chromosome id -> name, ids in order of first appearance
    std::unordered_map<std::string, uint32_t> id;
    std::vector<uint32_t> chrom, start, end;  // the rows, in file order
    std::vector<double> values;               // [rows * conditions], row-major
    std::vector<std::string> cond;
    std::mutex mu;  // guards the lazy device image
    gtars::SignalDevice *dev = nullptr;
    ~gtars_signal() { gtars::signal_free(dev); }
    void push(const std::string &chr, uint32_t s, uint32_t e) {
        auto it = id.find(chr);
        if (it == id.end()) {
            it = id.emplace(chr, (uint32_t)names.size()).first;
            names.push_back(chr);
        }
        chrom.push_back(it->second);
        start.push_back(s);
        end.push_back(e);
    }
};

namespace {

constexpr uint32_t SIGM_MAGIC = 0x5349474D, SIGM_VERSION = 2;
uint32_t g_sort_elems = gtars::SIGNAL_SORT_ELEMS;  // gtars_debug_signal_sort_elems

struct Bytes {  // of gtars_read_file
    char *p = nullptr;
    uint64_t n = 0;
    ~Bytes() { gtars_free(p); }
};

struct Span {
    const char *p;
    size_t n;
};

// the pieces of [p, p + n) between the separators (str::split: n + 1 pieces for n separators)
void split(const char *p, size_t n, char sep, std::vector<Span> &out) {
    out.clear();
    size_t a = 0;
    for (size_t i = 0; i <= n; ++i)
        if (i == n || p[i] == sep) {
            out.push_back(Span{p + a, i - a});
            a = i + 1;
        }
}

// u32::from_str: an optional '+', then digits only, at least one; overflow fails
bool parse_u32(Span s, uint32_t &out) {
    size_t i = s.n && s.p[0] == '+' ? 1 : 0;
    if (i == s.n) return false;
    uint64_t v = 0;
    for (; i < s.n; ++i) {
        if (s.p[i] < '0' || s.p[i] > '9') return false;
        v = v * 10 + (uint64_t)(s.p[i] - '0');
        if (v > 0xFFFFFFFFull) return false;
    }
    out = (uint32_t)v;
    return true;
}

bool ieq(const char *p, size_t n, const char *word) {
    if (strlen(word) != n) return false;
    for (size_t i = 0; i < n; ++i)
        if ((p[i] | 0x20) != word[i]) return false;
    return true;
}

// f64::from_str: an optional sign, then inf / infinity / nan in any case, or digits with an optional '.' (at least one
// digit on either side of it) and an optional exponent [eE][+-]digits; nothing else, nothing around it.  Correctly rounded.
bool parse_f64(Span s, double &out) {
    const char *p = s.p;
    size_t n = s.n;
    bool neg = false;
    if (n && (p[0] == '+' || p[0] == '-')) neg = p[0] == '-', ++p, --n;
    if (!n) return false;
    double v;
    if (ieq(p, n, "inf") || ieq(p, n, "infinity")) {
        v = std::numeric_limits<double>::infinity();
    } else if (ieq(p, n, "nan")) {
        const uint64_t bits = 0x7FF8000000000000ull;
        memcpy(&v, &bits, 8);
    } else {
        size_t i = 0, digits = 0;
        while (i < n && p[i] >= '0' && p[i] <= '9') ++i, ++digits;
        if (i < n && p[i] == '.') {
            ++i;
            while (i < n && p[i] >= '0' && p[i] <= '9') ++i, ++digits;
        }
        if (!digits) return false;
        if (i < n && (p[i] == 'e' || p[i] == 'E')) {
            ++i;
            if (i < n && (p[i] == '+' || p[i] == '-')) ++i;
            const size_t e0 = i;
            while (i < n && p[i] >= '0' && p[i] <= '9') ++i;
            if (i == e0) return false;
        }
        if (i != n) return false;
        const std::from_chars_result r = std::from_chars(p, p + n, v, std::chars_format::general);
        if (r.ec == std::errc::result_out_of_range) {
            // too large or too small for the format: infinity, or zero / a subnormal, as the reference rounds them
            const std::string z(p, n);
            v = strtod(z.c_str(), nullptr);
        } else if (r.ec != std::errc() || r.ptr != p + n) {
            return false;
        }
    }
    out = neg ? -v : v;
    return true;
}

inline uint64_t le(const unsigned char *p, int bytes) {
    uint64_t v = 0;
    for (int k = bytes - 1; k >= 0; --k) v = v << 8 | p[k];
    return v;
}
inline void put_le(std::string &s, uint64_t v, int bytes) {
    for (int k = 0; k < bytes; ++k) s.push_back((char)(v >> (8 * k) & 0xFF));
}

gtars_status sigm_error(const std::string &msg) { return fail(GTARS_ERR_PARSE, "Signal matrix error: " + msg); }

gtars_status parse_tsv(const char *p, size_t n, gtars_signal &m) {
    std::vector<Span> lines, fields, parts;
    split(p, n, '\n', lines);
    // BufRead::lines: a line ends at '\n', and a '\r' in front of that '\n' goes with it; the text behind the last '\n' is a
    // line as it stands unless it is empty
    for (size_t k = 0; k + 1 < lines.size(); ++k)
        if (lines[k].n && lines[k].p[lines[k].n - 1] == '\r') --lines[k].n;
    if (lines.back().n == 0) lines.pop_back();
    if (lines.empty()) return sigm_error("Empty signal matrix file");
    split(lines[0].p, lines[0].n, '\t', fields);
    if (fields.size() < 2) return sigm_error("Signal matrix must have at least 2 columns");
    for (size_t k = 1; k < fields.size(); ++k) m.cond.emplace_back(fields[k].p, fields[k].n);
    const size_t nc = m.cond.size();
    std::vector<double> row(nc);
    for (size_t li = 1; li < lines.size(); ++li) {
        split(lines[li].p, lines[li].n, '\t', fields);
        split(fields[0].p, fields[0].n, '_', parts);
        uint32_t s, e;
        if (parts.size() != 3 || !parse_u32(parts[1], s) || !parse_u32(parts[2], e)) continue;
        if (fields.size() < 1 + nc) continue;
        bool ok = true;
        for (size_t k = 0; k < nc && ok; ++k) ok = parse_f64(fields[1 + k], row[k]);
        if (!ok) continue;
        m.push(std::string(parts[0].p, parts[0].n), s, e);
        m.values.insert(m.values.end(), row.begin(), row.end());
    }
    if (m.start.empty()) return sigm_error("No valid rows in signal matrix");
    return GTARS_OK;
}

gtars_status parse_sigm(const unsigned char *p, uint64_t size, gtars_signal &m) {
    uint64_t pos = 0;
    bool short_file = false;
    auto take = [&](uint64_t k) -> const unsigned char * {  // null: truncated
        if (short_file || k > size - pos) {
            short_file = true;
            return nullptr;
        }
        const unsigned char *q = p + pos;
        pos += k;
        return q;
    };
    auto u = [&](int bytes) -> uint64_t {
        const unsigned char *q = take((uint64_t)bytes);
        return q ? le(q, bytes) : 0;
    };
    const uint64_t magic = u(4);
    if (short_file) return sigm_error("Unexpected end of file");
    if (magic != SIGM_MAGIC) return sigm_error("Invalid signal matrix file format — regenerate with 'gtars prep'");
    const uint64_t version = u(4);
    if (short_file) return sigm_error("Unexpected end of file");
    if (version != SIGM_VERSION)
        return sigm_error("Unsupported signal matrix format version " + std::to_string(version) + " (expected " +
                          std::to_string(SIGM_VERSION) + ") — regenerate with 'gtars prep'");
    const uint64_t n_regions = u(4), n_cond = u(4), n_strings = u(4);
    if (short_file) return sigm_error("Unexpected end of file");
    std::vector<std::string> table;
    for (uint64_t k = 0; k < n_strings; ++k) {
        const uint64_t len = u(4);
        const unsigned char *q = take(len);
        if (short_file) return sigm_error("Unexpected end of file");
        table.emplace_back((const char *)q, (size_t)len);
    }
    const uint64_t n_names = u(4);
    if (short_file) return sigm_error("Unexpected end of file");
    if (n_names != n_cond) return sigm_error("Condition name count mismatch");
    const unsigned char *cond_ids = take(n_cond * 2), *chr_ids = take(n_regions * 2), *starts = take(n_regions * 4),
                        *ends = take(n_regions * 4);
    if (n_cond && n_regions > size / 8 / n_cond) short_file = true;  // (the product below would not fit the file, or 64 bits)
    const unsigned char *vals = take(n_regions * n_cond * 8);
    if (short_file) return sigm_error("Unexpected end of file");
    for (uint64_t k = 0; k < n_cond; ++k) {
        const uint64_t sid = le(cond_ids + 2 * k, 2);
        if (sid >= table.size()) return sigm_error("Condition name id " + std::to_string(sid) + " outside the string table");
        m.cond.push_back(table[(size_t)sid]);
    }
    for (uint64_t i = 0; i < n_regions; ++i) {
        const uint64_t sid = le(chr_ids + 2 * i, 2);
        if (sid >= table.size()) return sigm_error("Chromosome id " + std::to_string(sid) + " outside the string table");
        m.push(table[(size_t)sid], (uint32_t)le(starts + 4 * i, 4), (uint32_t)le(ends + 4 * i, 4));
    }
    m.values.resize((size_t)(n_regions * n_cond));
    for (size_t k = 0; k < m.values.size(); ++k) {
        const uint64_t bits = le(vals + 8 * k, 8);
        memcpy(&m.values[k], &bits, 8);
    }
    return GTARS_OK;
}

// the handle's device image, built at the first summary on the device current then
gtars_status device_image(gtars_signal *m, gtars::SignalDevice **out) {
    std::lock_guard<std::mutex> lk(m->mu);
    if (!m->dev)
        if (const gtars_status e = gtars::signal_build(m->chrom.data(), m->start.data(), m->end.data(), m->start.size(),
                                                       (uint32_t)m->names.size(), m->values.data(), (uint32_t)m->cond.size(), &m->dev))
            return e;
    *out = m->dev;
    return GTARS_OK;
}

gtars_status hand_over(gtars::SignalSummary &r, uint32_t **qidx, double **values, double **stats, uint64_t *n_rows) {
    *n_rows = r.n_rows;
    if (qidx) *qidx = r.qidx, r.qidx = nullptr;
    if (values) *values = r.values, r.values = nullptr;
    *stats = r.stats, r.stats = nullptr;
    return GTARS_OK;
}

}  // namespace

extern "C" {

gtars_status gtars_signal_from_tsv(const char *path, gtars_signal_t **out) {
    return guarded([&]() -> gtars_status {
        if (!path || !out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        Bytes b;
        if (const gtars_status e = gtars_read_file(path, &b.p, &b.n)) return e;
        auto m = std::make_unique<gtars_signal>();
        if (const gtars_status e = parse_tsv(b.p, (size_t)b.n, *m)) return e;
        *out = m.release();
        return GTARS_OK;
    });
}

gtars_status gtars_signal_load_bin(const char *path, gtars_signal_t **out) {
    return guarded([&]() -> gtars_status {
        if (!path || !out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        FILE *f = fopen(path, "rb");
        if (!f) return fail(GTARS_ERR_IO, std::string("Failed to open file: \"") + path + "\": " + strerror(errno));
        std::string data;
        std::vector<char> buf(1 << 20);
        size_t k;
        while ((k = fread(buf.data(), 1, buf.size(), f)) > 0) data.append(buf.data(), k);
        const bool bad = ferror(f) != 0;
        fclose(f);
        if (bad) return fail(GTARS_ERR_IO, std::string("Failed to read file: \"") + path + "\"");
        auto m = std::make_unique<gtars_signal>();
        if (const gtars_status e = parse_sigm((const unsigned char *)data.data(), data.size(), *m)) return e;
        *out = m.release();
        return GTARS_OK;
    });
}

gtars_status gtars_signal_save_bin(const gtars_signal_t *m, const char *path) {
    return guarded([&]() -> gtars_status {
        if (!m || !path) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        // the string table: chromosome names in order of first appearance, then the condition names it lacks
        std::vector<const std::string *> table;
        std::unordered_map<std::string, uint32_t> at;
        for (const std::string &s : m->names) at.emplace(s, (uint32_t)table.size()), table.push_back(&s);
        for (const std::string &s : m->cond)
            if (at.emplace(s, (uint32_t)table.size()).second) table.push_back(&s);
        if (table.size() > 65536) return fail(GTARS_ERR_INVALID_ARG, "signal matrix: more than 65536 distinct names");
        const size_t n = m->start.size(), nc = m->cond.size();
        std::string b;
        put_le(b, SIGM_MAGIC, 4);
        put_le(b, SIGM_VERSION, 4);
        put_le(b, n, 4);
        put_le(b, nc, 4);
        put_le(b, table.size(), 4);
        for (const std::string *s : table) {
            put_le(b, s->size(), 4);
            b += *s;
        }
        put_le(b, nc, 4);
        for (const std::string &s : m->cond) put_le(b, at[s], 2);
        b.reserve(b.size() + n * 10 + m->values.size() * 8);
        for (size_t i = 0; i < n; ++i) put_le(b, m->chrom[i], 2);
        for (size_t i = 0; i < n; ++i) put_le(b, m->start[i], 4);
        for (size_t i = 0; i < n; ++i) put_le(b, m->end[i], 4);
        for (const double v : m->values) {
            uint64_t bits;
            memcpy(&bits, &v, 8);
            put_le(b, bits, 8);
        }
        FILE *f = fopen(path, "wb");
        if (!f) return fail(GTARS_ERR_IO, std::string("Failed to create file: \"") + path + "\": " + strerror(errno));
        const bool ok = fwrite(b.data(), 1, b.size(), f) == b.size();
        const bool closed = fclose(f) == 0;
        if (!ok || !closed) return fail(GTARS_ERR_IO, std::string("Failed to write file: \"") + path + "\"");
        return GTARS_OK;
    });
}

gtars_status gtars_signal_from_arrays(const char *const *chrom_names, uint32_t n_chrom, const uint32_t *chrom, const uint32_t *start,
                                      const uint32_t *end, uint64_t n, const double *values, const char *const *condition_names,
                                      uint32_t n_conditions, gtars_signal_t **out) {
    return guarded([&]() -> gtars_status {
        if (!out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        if (!n || !n_conditions) return fail(GTARS_ERR_INVALID_ARG, "signal matrix without rows or conditions");
        if (!chrom_names || !chrom || !start || !end || !values || !condition_names) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (n > 0xFFFFF000ull) return fail(GTARS_ERR_INVALID_ARG, "signal matrix too large (" + std::to_string(n) + " rows)");
        auto m = std::make_unique<gtars_signal>();
        for (uint32_t k = 0; k < n_conditions; ++k) {
            if (!condition_names[k]) return fail(GTARS_ERR_INVALID_ARG, "NULL condition name");
            m->cond.emplace_back(condition_names[k]);
        }
        std::vector<std::string> dict(n_chrom);
        for (uint32_t c = 0; c < n_chrom; ++c) {
            if (!chrom_names[c]) return fail(GTARS_ERR_INVALID_ARG, "NULL chromosome name");
            dict[c] = chrom_names[c];
        }
        m->chrom.reserve(n), m->start.reserve(n), m->end.reserve(n);
        for (uint64_t i = 0; i < n; ++i) {
            if (chrom[i] >= n_chrom) return fail(GTARS_ERR_INVALID_ARG, "signal matrix: chromosome id out of range");
            m->push(dict[chrom[i]], start[i], end[i]);
        }
        m->values.assign(values, values + n * n_conditions);
        *out = m.release();
        return GTARS_OK;
    });
}

void gtars_signal_free(gtars_signal_t *m) { delete m; }
uint64_t gtars_signal_n_regions(const gtars_signal_t *m) { return m ? m->start.size() : 0; }
uint32_t gtars_signal_n_conditions(const gtars_signal_t *m) { return m ? (uint32_t)m->cond.size() : 0; }
const char *gtars_signal_condition_name(const gtars_signal_t *m, uint32_t i) {
    return m && i < m->cond.size() ? m->cond[i].c_str() : nullptr;
}
uint32_t gtars_signal_n_chrom(const gtars_signal_t *m) { return m ? (uint32_t)m->names.size() : 0; }
const char *gtars_signal_chrom_name(const gtars_signal_t *m, uint32_t id) {
    return m && id < m->names.size() ? m->names[id].c_str() : nullptr;
}
const uint32_t *gtars_signal_chrom_ids(const gtars_signal_t *m) { return m ? m->chrom.data() : nullptr; }
const uint32_t *gtars_signal_starts(const gtars_signal_t *m) { return m ? m->start.data() : nullptr; }
const uint32_t *gtars_signal_ends(const gtars_signal_t *m) { return m ? m->end.data() : nullptr; }
const double *gtars_signal_values(const gtars_signal_t *m) { return m ? m->values.data() : nullptr; }

int gtars_signal_device(const gtars_signal_t *m) {
    if (!m) return -1;
    std::lock_guard<std::mutex> lk(const_cast<gtars_signal_t *>(m)->mu);
    return gtars::signal_device(m->dev);
}

gtars_status gtars_signal_summary_device(gtars_signal_t *m, const uint32_t *d_chrom, const uint32_t *d_start, const uint32_t *d_end,
                                         uint64_t n, void *stream, uint32_t **qidx, double **values, double **stats, uint64_t *n_rows) {
    return guarded([&]() -> gtars_status {
        if (!m || !stats || !n_rows) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (qidx) *qidx = nullptr;
        if (values) *values = nullptr;
        *stats = nullptr, *n_rows = 0;
        if (!n) return GTARS_OK;
        gtars::SignalDevice *dev;
        if (const gtars_status e = device_image(m, &dev)) return e;
        gtars::SignalSummary r;
        if (const gtars_status e = gtars::signal_summary_device(*dev, d_chrom, d_start, d_end, n, qidx && values, g_sort_elems, r, stream))
            return e;
        return hand_over(r, qidx, values, stats, n_rows);
    });
}

gtars_status gtars_signal_summary(gtars_signal_t *m, const gtars_regionset_t *rs, uint32_t **qidx, double **values, double **stats,
                                  uint64_t *n_rows) {
    return guarded([&]() -> gtars_status {
        if (!m || !rs || !qidx || !values || !stats || !n_rows) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *qidx = nullptr, *values = nullptr, *stats = nullptr, *n_rows = 0;
        const uint64_t n = gtars_regionset_len(rs);
        if (!n) return GTARS_OK;
        // the set's chromosome ids on the matrix's dictionary; a chromosome the matrix lacks gives no hits
        const uint32_t nc = gtars_regionset_n_chrom(rs);
        std::vector<uint32_t> seg_of(nc, GTARS_UNKNOWN_CHROM);
        bool any = false;
        for (uint32_t k = 0; k < nc; ++k) {
            auto it = m->id.find(gtars_regionset_chrom_name(rs, k));
            if (it != m->id.end()) seg_of[k] = it->second, any = true;
        }
        if (!any) return GTARS_OK;
        const uint32_t *cid = gtars_regionset_chrom_ids(rs);
        std::vector<uint32_t> qc(n);
        for (uint64_t i = 0; i < n; ++i) qc[i] = seg_of[cid[i]];
        gtars::SignalDevice *dev;
        if (const gtars_status e = device_image(m, &dev)) return e;
        gtars::SignalSummary r;
        if (const gtars_status e =
                gtars::signal_summary(*dev, qc.data(), gtars_regionset_starts(rs), gtars_regionset_ends(rs), n, g_sort_elems, r))
            return e;
        return hand_over(r, qidx, values, stats, n_rows);
    });
}

uint32_t gtars_debug_signal_sort_elems(uint32_t elems) {
    const uint32_t before = g_sort_elems;
    g_sort_elems = elems ? elems : gtars::SIGNAL_SORT_ELEMS;
    return before;
}

uint32_t gtars_debug_signal_split_hits(void) { return gtars::SIGNAL_SPLIT_HITS; }

}  // extern "C"
