// bed_text.cpp -- the host layer of K25 (RegionSet.identifier / file_digest / to_bed / to_bed_gz, RegionSetList.identifier;
// gtars-core/src/models/region_set.rs:240-330, region_set_list.rs:85-98): the host paths over the text of bed_text_core.h --
// the same header the kernels of bed_text.hip compile -- and the calls that gather a list of handles into the columns the
// device pipeline takes.  Declared in include/gtars_amd_host.h (the entry on device columns in include/gtars_amd.h).
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <memory>
#include <string>
#include <vector>

#include "../../include/gtars_amd_host.h"
#include "bed_text.h"
#include "bed_text_core.h"
#include "guard.h"
#include "host_threads.h"

namespace gtars {
unsigned host_threads_for(unsigned cap);
}  // namespace gtars
using gtars::BedRow;
using gtars::fail;
using gtars::guarded;

namespace {

unsigned threads_of(uint32_t threads) {
    const unsigned most = gtars::host_threads_for(0xFFFFFFFFu);
    return threads ? std::min<unsigned>(threads, most) : most;
}

// a handle through its public columns
struct SetView {
    const gtars_regionset_t *rs;
    size_t n;
    const uint32_t *chrom, *start, *end;
    std::vector<const uint8_t *> name;
    std::vector<uint32_t> name_len;
    explicit SetView(const gtars_regionset_t *s)
        : rs(s), n((size_t)gtars_regionset_len(s)), chrom(gtars_regionset_chrom_ids(s)), start(gtars_regionset_starts(s)),
          end(gtars_regionset_ends(s)) {
        const uint32_t n_names = gtars_regionset_n_chrom(s);
        for (uint32_t c = 0; c < n_names; ++c) {
            const char *nm = gtars_regionset_chrom_name(s, c);
            name.push_back((const uint8_t *)nm), name_len.push_back((uint32_t)strlen(nm));
        }
    }
    BedRow row(size_t i, uint32_t kind) const {
        BedRow r;
        r.name = name[chrom[i]], r.name_len = name_len[chrom[i]];
        r.start = start[i], r.end = end[i];
        r.rest = nullptr, r.rest_len = 0, r.has_rest = false, r.last = i + 1 == n;
        if (kind == gtars::BED_LINE)
            if (const char *rest = gtars_regionset_rest(rs, i)) r.rest = (const uint8_t *)rest, r.rest_len = (uint32_t)strlen(rest), r.has_rest = true;
        return r;
    }
};

// one stream of a set, eight bytes per call for md5_stream_pairs: rows are written into a buffer a few at a time
struct HostStreamSrc {
    const SetView &v;
    uint32_t kind;
    size_t next_row = 0, pos = 0, have = 0;
    std::vector<uint8_t> buf;
    static constexpr size_t FILL = 1u << 16;
    void refill() {
        memmove(buf.data(), buf.data() + pos, have - pos);
        have -= pos, pos = 0;
        while (have < FILL && next_row < v.n) {
            const BedRow r = v.row(next_row++, kind);
            const size_t need = have + gtars::bed_row_bytes(kind, r);
            if (buf.size() < need) buf.resize(need + FILL);
            have += gtars::bed_row_write(kind, r, buf.data() + have);
        }
    }
    uint64_t pair(uint64_t) {
        if (have - pos < 8) refill();
        const size_t k = std::min<size_t>(8, have - pos);
        uint64_t d = 0;
        memcpy(&d, buf.data() + pos, k);
        pos += k;
        return d;
    }
};

// the MD5 (md5_words form) of one stream of a set
void stream_md5(const SetView &v, uint32_t kind, uint64_t out[2]) {
    uint64_t len = 0;
    for (size_t i = 0; i < v.n; ++i) len += gtars::bed_row_bytes(kind, v.row(i, kind));
    HostStreamSrc src{v, kind};
    src.buf.resize(2 * HostStreamSrc::FILL);
    gtars::Md5 s;
    gtars::md5_stream_pairs(s, src, len);
    gtars::md5_words(s, out);
}

// one digest per set on the host threads: out[2 * n]
void host_digests(const std::vector<SetView> &views, int what, unsigned threads, uint64_t *out) {
    const size_t n = views.size();
    if (what == GTARS_BED_FILE_DIGEST) {
        gtars::parallel_for(n, threads, 1, [&](size_t s) { stream_md5(views[s], gtars::BED_LINE, out + 2 * s); });
        return;
    }
    std::vector<uint64_t> part(6 * n);
    gtars::parallel_for(3 * n, threads, 1, [&](size_t t) { stream_md5(views[t / 3], (uint32_t)(t % 3), &part[2 * t]); });
    for (size_t s = 0; s < n; ++s) gtars::bed_identifier(&part[6 * s], out + 2 * s);
}

void hex_of(const uint64_t words[2], char *out32) {
    uint8_t d[16];
    memcpy(d, words, 16);  // (md5_words: byte i of the digest in byte i of memory)
    gtars::md5_hex(d, out32);
}

// the LINE text of a set, formatted on the host threads
void host_text(const SetView &v, unsigned threads, std::string &out) {
    constexpr size_t BLOCK = 4096;
    const size_t n_blocks = (v.n + BLOCK - 1) / BLOCK;
    std::vector<uint64_t> at(n_blocks + 1, 0);
    gtars::parallel_for(n_blocks, threads, 1, [&](size_t b) {
        uint64_t bytes = 0;
        for (size_t i = b * BLOCK; i < std::min(v.n, (b + 1) * BLOCK); ++i) bytes += gtars::bed_row_bytes(gtars::BED_LINE, v.row(i, gtars::BED_LINE));
        at[b + 1] = bytes;
    });
    for (size_t b = 0; b < n_blocks; ++b) at[b + 1] += at[b];
    out.resize((size_t)at[n_blocks]);
    uint8_t *dst = (uint8_t *)&out[0];
    gtars::parallel_for(n_blocks, threads, 1, [&](size_t b) {
        uint8_t *p = dst + at[b];
        for (size_t i = b * BLOCK; i < std::min(v.n, (b + 1) * BLOCK); ++i) p += gtars::bed_row_write(gtars::BED_LINE, v.row(i, gtars::BED_LINE), p);
    });
}

// The sets as the chunks of columns the device pipeline takes.  The names table of a chunk is every set's own table one
// after the other, a set's ids rebased by the names before it.
struct Stager {
    const std::vector<SetView> &views;
    bool line;
    unsigned threads;
    // (the row columns are written whole by the copy below: no value-initialisation of a gigabyte on one thread)
    template <class T>
    struct Raw {
        std::unique_ptr<T[]> p;
        size_t cap = 0;
        T *take(size_t n) {
            if (n > cap || !p) p.reset(new T[std::max<size_t>(n, 1)]), cap = n;
            return p.get();
        }
    };
    std::vector<uint64_t> set_off, name_off;
    std::vector<uint8_t> names;
    Raw<uint32_t> chrom_, start_, end_;
    Raw<uint64_t> rest_off_;
    Raw<uint8_t> rest_, has_rest_;
    void operator()(uint64_t s0, uint64_t s1, gtars::BedCols &c) {
        const size_t n_sets = (size_t)(s1 - s0);
        set_off.assign(n_sets + 1, 0);
        std::vector<uint32_t> name_base(n_sets + 1, 0);
        std::vector<uint64_t> rest_base(n_sets + 1, 0);
        name_off.assign(1, 0), names.clear();
        for (size_t k = 0; k < n_sets; ++k) {
            const SetView &v = views[s0 + k];
            set_off[k + 1] = set_off[k] + v.n;
            name_base[k + 1] = name_base[k] + (uint32_t)v.name.size();
            for (size_t j = 0; j < v.name.size(); ++j) {
                names.insert(names.end(), v.name[j], v.name[j] + v.name_len[j]);
                name_off.push_back(names.size());
            }
        }
        const size_t n = (size_t)set_off[n_sets];
        uint32_t *chrom = chrom_.take(n), *start = start_.take(n), *end = end_.take(n);
        uint64_t *rest_off = nullptr;
        uint8_t *rest = nullptr, *has_rest = nullptr;
        if (line) {
            has_rest = has_rest_.take(n), rest_off = rest_off_.take(n + 1);
            gtars::parallel_for(n_sets, threads, 1, [&](size_t k) {
                const SetView &v = views[s0 + k];
                uint64_t bytes = 0;
                for (size_t i = 0; i < v.n; ++i)
                    if (const char *r = gtars_regionset_rest(v.rs, i)) bytes += strlen(r);
                rest_base[k + 1] = bytes;
            });
            for (size_t k = 0; k < n_sets; ++k) rest_base[k + 1] += rest_base[k];
            rest = rest_.take((size_t)rest_base[n_sets]);
        }
        gtars::parallel_for(n_sets, threads, 1, [&](size_t k) {
            const SetView &v = views[s0 + k];
            const size_t at = (size_t)set_off[k];
            for (size_t i = 0; i < v.n; ++i) chrom[at + i] = v.chrom[i] + name_base[k];
            if (v.n) memcpy(&start[at], v.start, v.n * sizeof(uint32_t)), memcpy(&end[at], v.end, v.n * sizeof(uint32_t));
            if (!line) return;
            uint64_t o = rest_base[k];
            for (size_t i = 0; i < v.n; ++i) {
                const char *r = gtars_regionset_rest(v.rs, i);
                const size_t len = r ? strlen(r) : 0;
                has_rest[at + i] = r != nullptr;
                rest_off[at + i] = o;
                if (len) memcpy(&rest[(size_t)o], r, len);
                o += len;
            }
        });
        if (line) rest_off[n] = rest_base[n_sets];
        c.set_off = set_off.data(), c.n_sets = n_sets;
        c.chrom = chrom, c.start = start, c.end = end;
        c.name_off = name_off.data(), c.names = names.data(), c.n_names = name_base[n_sets];
        c.rest_off = rest_off, c.rest = rest, c.has_rest = has_rest;
    }
};

// one digest per set (what) or the LINE text of all sets (BED_WHAT_TEXT) on the device
gtars_status device_run(const std::vector<SetView> &views, int what, unsigned threads, uint64_t *out, std::string *text) {
    const size_t n = views.size();
    const bool line = what != GTARS_BED_IDENTIFIER;
    std::vector<uint64_t> set_off(n + 1, 0), bound(n, 0);
    uint64_t max_name = 0;
    for (const SetView &v : views)
        for (uint32_t l : v.name_len) max_name = std::max<uint64_t>(max_name, l);
    gtars::parallel_for(n, threads, 1, [&](size_t s) {
        const SetView &v = views[s];
        uint64_t rest_bytes = 0;
        for (size_t i = 0; line && i < v.n; ++i)
            if (const char *r = gtars_regionset_rest(v.rs, i)) rest_bytes += strlen(r);
        bound[s] = gtars::bed_text_bound(what, v.n, rest_bytes, max_name);
    });
    for (size_t s = 0; s < n; ++s) set_off[s + 1] = set_off[s] + views[s].n;
    Stager stage{views, line, threads, {}, {}, {}, {}, {}, {}, {}, {}, {}};
    return gtars::bed_text_run_host_cols(set_off.data(), n, bound, std::ref(stage), what, out, text, threads);
}

gtars_status views_of(const gtars_regionset_t *const *sets, uint64_t n, std::vector<SetView> &views) {
    if (n && !sets) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    views.reserve((size_t)n);
    for (uint64_t k = 0; k < n; ++k) {
        if (!sets[k]) return fail(GTARS_ERR_INVALID_ARG, "NULL region set");
        views.emplace_back(sets[k]);
    }
    return GTARS_OK;
}

gtars_status list_digests(const gtars_regionset_t *const *sets, uint64_t n, int what, int on_host, uint32_t threads, std::vector<uint64_t> &out) {
    if (what != GTARS_BED_IDENTIFIER && what != GTARS_BED_FILE_DIGEST)
        return fail(GTARS_ERR_INVALID_ARG, "what must be GTARS_BED_IDENTIFIER or GTARS_BED_FILE_DIGEST");
    std::vector<SetView> views;
    if (const gtars_status e = views_of(sets, n, views)) return e;
    out.assign(2 * (size_t)n, 0);
    if (on_host) {
        host_digests(views, what, threads_of(threads), out.data());
        return GTARS_OK;
    }
    return device_run(views, what, threads_of(threads), out.data(), nullptr);
}

gtars_status single_digest(const gtars_regionset_t *rs, int what, char *out33) {
    if (!rs || !out33) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    std::vector<SetView> views;
    views.emplace_back(rs);
    uint64_t d[2];
    host_digests(views, what, std::min(threads_of(0), 4u), d);  // (three slow streams: a single set stays on the host)
    hex_of(d, out33), out33[32] = '\0';
    return GTARS_OK;
}

gtars_status text_of(const gtars_regionset_t *rs, bool on_host, std::string &text) {
    std::vector<SetView> views;
    views.emplace_back(rs);
    text.clear();
    if (on_host) {
        host_text(views[0], threads_of(0), text);
        return GTARS_OK;
    }
    return device_run(views, gtars::BED_WHAT_TEXT, threads_of(0), nullptr, &text);
}

// `text` as one gzip member at the best compression level
gtars_status gzip_of(const std::string &text, std::string &out) {
    z_stream z;
    memset(&z, 0, sizeof z);
    if (deflateInit2(&z, Z_BEST_COMPRESSION, Z_DEFLATED, 15 + 16, 8, Z_DEFAULT_STRATEGY) != Z_OK) return fail(GTARS_ERR_INTERNAL, "zlib: deflateInit2");
    out.resize(1u << 16);
    size_t fed = 0;  // (zlib counts a call's input and output in 32 bits: both go through in pieces)
    int rc;
    do {
        if (z.avail_in == 0 && fed < text.size()) {
            const size_t piece = std::min<size_t>(text.size() - fed, 1u << 30);
            z.next_in = (Bytef *)text.data() + fed, z.avail_in = (uInt)piece;
            fed += piece;
        }
        if (z.total_out == out.size()) out.resize(2 * out.size());
        z.next_out = (Bytef *)&out[0] + z.total_out;
        z.avail_out = (uInt)std::min<size_t>(out.size() - z.total_out, 1u << 30);
        rc = deflate(&z, fed == text.size() ? Z_FINISH : Z_NO_FLUSH);
        if (rc == Z_STREAM_ERROR) {
            deflateEnd(&z);
            return fail(GTARS_ERR_INTERNAL, "zlib: deflate");
        }
    } while (rc != Z_STREAM_END);
    out.resize(z.total_out);
    deflateEnd(&z);
    return GTARS_OK;
}

}  // namespace

namespace gtars {

gtars_status write_text_file(const std::string &text, const char *path, bool gz) {
    std::string packed;
    if (gz)
        if (const gtars_status e = gzip_of(text, packed)) return e;
    const std::string &bytes = gz ? packed : text;
    std::error_code ec;
    const std::filesystem::path parent = std::filesystem::path(path).parent_path();
    if (!parent.empty()) std::filesystem::create_directories(parent, ec);
    FILE *f = fopen(path, "wb");
    if (!f) return fail(GTARS_ERR_IO, std::string("cannot create ") + path);
    const bool ok = fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    if (fclose(f) != 0 || !ok) return fail(GTARS_ERR_IO, std::string("cannot write ") + path);
    return GTARS_OK;
}

}  // namespace gtars

extern "C" {

gtars_status gtars_regionset_identifier(const gtars_regionset_t *rs, char *out33) {
    return guarded([&]() -> gtars_status { return single_digest(rs, GTARS_BED_IDENTIFIER, out33); });
}

gtars_status gtars_regionset_file_digest(const gtars_regionset_t *rs, char *out33) {
    return guarded([&]() -> gtars_status { return single_digest(rs, GTARS_BED_FILE_DIGEST, out33); });
}

gtars_status gtars_regionset_bed_text(const gtars_regionset_t *rs, int on_host, char **out, uint64_t *len) {
    return guarded([&]() -> gtars_status {
        if (!rs || !out || !len) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr, *len = 0;
        std::string text;
        if (const gtars_status e = text_of(rs, on_host != 0, text)) return e;
        char *p = (char *)malloc(text.size() + 1);
        if (!p) return fail(GTARS_ERR_INTERNAL, "out of host memory");
        memcpy(p, text.data(), text.size()), p[text.size()] = '\0';
        *out = p, *len = text.size();
        return GTARS_OK;
    });
}

gtars_status gtars_regionset_write_bed(const gtars_regionset_t *rs, const char *path, int gz) {
    return guarded([&]() -> gtars_status {
        if (!rs || !path) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        std::string text;
        if (const gtars_status e = text_of(rs, gtars_regionset_len(rs) < gtars::bed_text_device_rows(), text)) return e;
        return gtars::write_text_file(text, path, gz != 0);
    });
}

gtars_status gtars_regionset_list_digests(const gtars_regionset_t *const *sets, uint64_t n, int what, int on_host, uint32_t threads, char *out) {
    return guarded([&]() -> gtars_status {
        if (n && !out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        std::vector<uint64_t> d;
        if (const gtars_status e = list_digests(sets, n, what, on_host, threads, d)) return e;
        for (uint64_t s = 0; s < n; ++s) hex_of(&d[2 * s], out + 32 * s);
        return GTARS_OK;
    });
}

// RegionSetList::identifier (region_set_list.rs:85-98): the member identifiers sorted as strings, concatenated, hashed
gtars_status gtars_regionset_list_identifier(const gtars_regionset_t *const *sets, uint64_t n, int on_host, uint32_t threads, char *out33) {
    return guarded([&]() -> gtars_status {
        if (!out33) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        std::vector<uint64_t> d;
        if (const gtars_status e = list_digests(sets, n, GTARS_BED_IDENTIFIER, on_host, threads, d)) return e;
        std::vector<std::string> ids((size_t)n, std::string(32, '\0'));
        for (uint64_t s = 0; s < n; ++s) hex_of(&d[2 * s], &ids[s][0]);
        std::sort(ids.begin(), ids.end());
        std::string all;
        for (const std::string &id : ids) all += id;
        uint8_t digest[16];
        gtars::md5((const uint8_t *)all.data(), all.size(), digest);
        gtars::md5_hex(digest, out33), out33[32] = '\0';
        return GTARS_OK;
    });
}

gtars_status gtars_bed_digests_device(const uint64_t *set_off, uint64_t n_sets, const uint32_t *d_chrom, const uint32_t *d_start,
                                      const uint32_t *d_end, const uint64_t *d_name_off, const uint8_t *d_names, uint32_t n_names,
                                      const uint64_t *d_rest_off, const uint8_t *d_rest, const uint8_t *d_has_rest, int what, uint8_t *d_digests,
                                      void *stream) {
    return guarded([&]() -> gtars_status {
        if (what != GTARS_BED_IDENTIFIER && what != GTARS_BED_FILE_DIGEST)
            return fail(GTARS_ERR_INVALID_ARG, "what must be GTARS_BED_IDENTIFIER or GTARS_BED_FILE_DIGEST");
        gtars::BedCols c;
        c.set_off = set_off, c.n_sets = n_sets, c.chrom = d_chrom, c.start = d_start, c.end = d_end;
        c.name_off = d_name_off, c.names = d_names, c.n_names = n_names, c.rest_off = d_rest_off, c.rest = d_rest, c.has_rest = d_has_rest;
        return gtars::bed_text_run_device(c, what, (uint64_t *)d_digests, nullptr, threads_of(0), stream);
    });
}

}  // extern "C"
