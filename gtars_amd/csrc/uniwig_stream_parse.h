// uniwig_stream_parse.h -- the text side of the streaming uniwig (K24): parse_bed_line and the line loop of
// gtars-uniwig/src/stream.rs:57-112, 516-596 over a whole buffer, plain or gzip.  Header only and free of the library's
// other headers (zlib and the standard library), so that a stand-alone program can run it under the sanitizers
// (tests/soak/uniwig_stream_host_check.cpp).
//
// Rules (each one a line of stream.rs):
//   * a buffer that starts with 1f 8b is gzip; only its FIRST member is decoded (flate2::bufread::GzDecoder), whatever
//     follows it is ignored;
//   * the text must be UTF-8 (read_line into a String);
//   * a line ends at '\n'; every trailing '\n' and '\r' is cut; an empty line and a line whose FIRST byte is '#' are
//     skipped; then the line is trimmed (Unicode White_Space, as str::trim) and skipped if it is empty or starts with
//     "track" or "browser";
//   * fields are split on any run of white space; fewer than 3 is an error; start and end parse as i32 (an optional sign,
//     digits), the error text carries the reference's message;
//   * score = fields[4].parse::<i32>().unwrap_or(1).max(0) when there are 5 fields or more, else 1.
// The first bad line fails the whole parse: nothing is kept.
#pragma once

#include <zlib.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

namespace gtars {
namespace swparse {

struct Rows {
    std::vector<std::string> names;  // chromosome names in first-seen order
    std::vector<uint32_t> cid;       // index into names, per row
    std::vector<int32_t> start, end;
    std::vector<uint32_t> score;  // 0 .. 2^31 - 1
};

// bytes of the white-space character at p (p < e), 0 if there is none: char::is_whitespace
inline size_t ws_len(const unsigned char *p, const unsigned char *e) {
    const unsigned char c = p[0];
    if (c == ' ' || (c >= 0x09 && c <= 0x0D)) return 1;
    if (c == 0xC2 && e - p >= 2) return (p[1] == 0x85 || p[1] == 0xA0) ? 2 : 0;
    if (e - p < 3) return 0;
    if (c == 0xE1) return (p[1] == 0x9A && p[2] == 0x80) ? 3 : 0;
    if (c == 0xE2) {
        if (p[1] == 0x80) return ((p[2] >= 0x80 && p[2] <= 0x8A) || p[2] == 0xA8 || p[2] == 0xA9 || p[2] == 0xAF) ? 3 : 0;
        return (p[1] == 0x81 && p[2] == 0x9F) ? 3 : 0;
    }
    if (c == 0xE3) return (p[1] == 0x80 && p[2] == 0x80) ? 3 : 0;
    return 0;
}

inline bool valid_utf8(const unsigned char *p, const unsigned char *e) {
    while (p < e) {
        const unsigned char c = *p;
        if (c < 0x80) {
            ++p;
            continue;
        }
        size_t n;
        unsigned lo = 0x80, hi = 0xBF;
        if (c >= 0xC2 && c <= 0xDF) n = 1;
        else if (c >= 0xE0 && c <= 0xEF) n = 2, lo = c == 0xE0 ? 0xA0 : 0x80, hi = c == 0xED ? 0x9F : 0xBF;
        else if (c >= 0xF0 && c <= 0xF4) n = 3, lo = c == 0xF0 ? 0x90 : 0x80, hi = c == 0xF4 ? 0x8F : 0xBF;
        else return false;
        if ((size_t)(e - p) <= n) return false;
        if (p[1] < lo || p[1] > hi) return false;
        for (size_t k = 2; k <= n; ++k)
            if ((p[k] & 0xC0) != 0x80) return false;
        p += n + 1;
    }
    return true;
}

// i32::from_str; on failure *why is the text of the ParseIntError
inline bool parse_i32(const unsigned char *p, const unsigned char *e, int32_t *out, const char **why) {
    if (p == e) return *why = "cannot parse integer from empty string", false;
    bool neg = false;
    if (*p == '+' || *p == '-') {
        neg = *p == '-';
        ++p;
        if (p == e) return *why = "invalid digit found in string", false;
    }
    int64_t v = 0;
    bool over = false;
    for (; p < e; ++p) {
        if (*p < '0' || *p > '9') return *why = "invalid digit found in string", false;
        if (!over) {
            v = v * 10 + (*p - '0');
            if (v > 2147483648ll) over = true;
        }
    }
    if (neg) v = -v;
    if (over || v > 2147483647ll || v < -2147483648ll)
        return *why = neg ? "number too small to fit in target type" : "number too large to fit in target type", false;
    *out = (int32_t)v;
    return true;
}

// the first member of a gzip buffer
inline bool gunzip_first_member(const unsigned char *p, size_t n, std::string &out, std::string &err) {
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, 16 + MAX_WBITS) != Z_OK) return err = "cannot set up the gzip decoder", false;
    std::vector<unsigned char> chunk(1u << 16);
    size_t at = 0;
    int rc = Z_OK;
    while (rc != Z_STREAM_END) {
        if (z.avail_in == 0 && at < n) {
            const size_t take = n - at < (1u << 30) ? n - at : (1u << 30);
            z.next_in = const_cast<unsigned char *>(p + at);
            z.avail_in = (uInt)take;
            at += take;
        }
        z.next_out = chunk.data();
        z.avail_out = (uInt)chunk.size();
        rc = inflate(&z, Z_NO_FLUSH);
        if (rc != Z_OK && rc != Z_STREAM_END) {
            err = rc == Z_BUF_ERROR ? "gzip input ends inside its first member" : "corrupt gzip input";
            inflateEnd(&z);
            return false;
        }
        out.append((const char *)chunk.data(), chunk.size() - z.avail_out);
    }
    inflateEnd(&z);
    return true;
}

inline bool starts_with(const unsigned char *p, const unsigned char *e, const char *word) {
    const size_t n = strlen(word);
    return (size_t)(e - p) >= n && memcmp(p, word, n) == 0;
}

// one line without its terminator: 1 a row was appended, 0 skipped, -1 error
inline int parse_line(const unsigned char *p, const unsigned char *e, Rows &rows, std::unordered_map<std::string, uint32_t> &ids,
                      std::string &err) {
    if (p == e || *p == '#') return 0;
    for (size_t k; p < e && (k = ws_len(p, e)); p += k) {}
    // (trailing white space: the last character is found from the front, the line is short)
    const unsigned char *last = p;
    for (const unsigned char *q = p; q < e;) {
        const size_t k = ws_len(q, e);
        q += k ? k : 1;
        if (!k) last = q;
    }
    // a multi-byte character that is no white space: `last` sits behind its first byte only; extend over its tail
    while (last < e && (*last & 0xC0) == 0x80) ++last;
    e = last;
    if (p == e) return 0;
    if (starts_with(p, e, "track") || starts_with(p, e, "browser")) return 0;
    const unsigned char *f0[5], *f1[5];
    size_t nf = 0;
    for (const unsigned char *q = p; q < e;) {
        size_t k = ws_len(q, e);
        if (k) {
            q += k;
            continue;
        }
        const unsigned char *b = q;
        while (q < e && !ws_len(q, e)) ++q;
        if (nf < 5) f0[nf] = b, f1[nf] = q;
        ++nf;
    }
    const std::string trimmed((const char *)p, (size_t)(e - p));
    if (nf < 3) return err = "BED line has fewer than 3 fields: '" + trimmed + "'", -1;
    int32_t s, t, sc = 1;
    const char *why = "";
    if (!parse_i32(f0[1], f1[1], &s, &why))
        return err = "Cannot parse start '" + std::string((const char *)f0[1], (size_t)(f1[1] - f0[1])) + "': " + why, -1;
    if (!parse_i32(f0[2], f1[2], &t, &why))
        return err = "Cannot parse end '" + std::string((const char *)f0[2], (size_t)(f1[2] - f0[2])) + "': " + why, -1;
    if (nf >= 5) {
        if (!parse_i32(f0[4], f1[4], &sc, &why)) sc = 1;
        if (sc < 0) sc = 0;
    }
    std::string name((const char *)f0[0], (size_t)(f1[0] - f0[0]));
    auto it = ids.find(name);
    uint32_t id;
    if (it == ids.end()) {
        id = (uint32_t)rows.names.size();
        ids.emplace(name, id);
        rows.names.push_back(std::move(name));
    } else {
        id = it->second;
    }
    rows.cid.push_back(id);
    rows.start.push_back(s);
    rows.end.push_back(t);
    rows.score.push_back((uint32_t)sc);
    return 1;
}

// the whole input; false: err holds the message and rows is empty
inline bool parse_buffer(const unsigned char *data, size_t n, Rows &rows, std::string &err) {
    rows = Rows();
    std::string plain;
    if (n >= 2 && data[0] == 0x1f && data[1] == 0x8b) {
        if (!gunzip_first_member(data, n, plain, err)) return false;
        data = (const unsigned char *)plain.data();
        n = plain.size();
    }
    if (!valid_utf8(data, data + n)) return err = "stream did not contain valid UTF-8", false;
    std::unordered_map<std::string, uint32_t> ids;
    const unsigned char *p = data, *end = data + n;
    while (p < end) {
        const unsigned char *nl = (const unsigned char *)memchr(p, '\n', (size_t)(end - p));
        const unsigned char *stop = nl ? nl : end, *e = stop;
        while (e > p && (e[-1] == '\r' || e[-1] == '\n')) --e;
        if (parse_line(p, e, rows, ids, err) < 0) {
            rows = Rows();
            return false;
        }
        p = nl ? nl + 1 : end;
    }
    return true;
}

}  // namespace swparse
}  // namespace gtars
