// assembly.cpp -- genome assemblies on the host (GenomeAssembly / BinaryGenomeAssembly, gtars-genomicdist/src/
// models.rs:145-413) and the library calls of K12 on top of seqstats.hip: calc_gc_content / calc_dinucl_freq
// (statistics.rs:331-483).  Declared in include/gtars_amd_host.h, where the readers' rules are written down.  Region
// sets are read through their public accessors.  The device counts integers; the divisions are done here, in f64, in the
// reference's order of operations.
#include <sys/stat.h>

#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/gtars_amd_host.h"
#include "assembly.h"
#include "guard.h"
#include "seqstats.h"

using gtars::fail;
using gtars::guarded;
using gtars::MallocArray;

// the handle's device image, built at the first call on the device current then
gtars_status gtars::assembly_device_image(gtars_assembly *a, gtars::Assembly **out) {
    std::lock_guard<std::mutex> lk(a->mu);
    if (!a->dev) {
        std::vector<const uint8_t *> seq(a->names.size());
        for (size_t c = 0; c < seq.size(); ++c) seq[c] = (const uint8_t *)a->blob.data() + a->off[c];
        if (const gtars_status e = gtars::assembly_build(seq.data(), a->len.data(), (uint32_t)seq.size(), &a->dev)) return e;
    }
    *out = a->dev;
    return GTARS_OK;
}

namespace {

using gtars::assembly_device_image;

inline bool is_ws(char ch) { return ch == ' ' || (ch >= '\t' && ch <= '\r'); }

struct File {
    FILE *f = nullptr;
    ~File() {
        if (f) fclose(f);
    }
};

gtars_status open_regular(const std::string &path, const char *mode, File &out) {
    struct stat sb;
    if (mode[0] == 'r' && stat(path.c_str(), &sb) == 0 && !S_ISREG(sb.st_mode))
        return fail(GTARS_ERR_IO, "Failed to open file: \"" + path + "\": not a regular file");
    out.f = fopen(path.c_str(), mode);
    if (!out.f) return fail(GTARS_ERR_IO, "Failed to open file: \"" + path + "\": " + strerror(errno));
    return GTARS_OK;
}

// the records of a FASTA file in file order: name, and the sequence as blob[off, off + len)
struct FastaRecord {
    std::string name;
    uint64_t off, len;
};

gtars_status read_fasta(const std::string &path, std::string &blob, std::vector<FastaRecord> &recs) {
    File in;
    if (const gtars_status e = open_regular(path, "rb", in)) return e;
    struct stat sb;
    if (fstat(fileno(in.f), &sb) == 0 && sb.st_size > 0) blob.reserve((size_t)sb.st_size);
    struct Line {
        char *p = nullptr;
        size_t cap = 0;
        ~Line() { free(p); }
    } line;
    bool first = true;
    for (;;) {
        const ssize_t got = getline(&line.p, &line.cap, in.f);
        if (got < 0) break;
        size_t n = (size_t)got;
        if (first && n && line.p[0] != '>')
            return fail(GTARS_ERR_PARSE, "Error reading genome file: Expected > at record start: " + path);
        first = false;
        while (n && is_ws(line.p[n - 1])) --n;
        if (n && line.p[0] == '>') {
            size_t k = 1;
            while (k < n && !is_ws(line.p[k])) ++k;
            recs.push_back(FastaRecord{std::string(line.p + 1, k - 1), blob.size(), 0});
        } else if (n) {
            blob.append(line.p, n);
            recs.back().len += n;
        }
    }
    if (ferror(in.f)) return fail(GTARS_ERR_IO, "Error reading genome file: \"" + path + "\": " + strerror(errno));
    return GTARS_OK;
}

inline uint64_t le(const unsigned char *p, int bytes) {
    uint64_t v = 0;
    for (int k = bytes - 1; k >= 0; --k) v = v << 8 | p[k];
    return v;
}
inline void put_le(std::string &s, uint64_t v, int bytes) {
    for (int k = 0; k < bytes; ++k) s.push_back((char)(v >> (8 * k) & 0xFF));
}

// std::str::from_utf8's rules: no overlong forms, no surrogates, nothing above U+10FFFF
bool valid_utf8(const unsigned char *p, size_t n) {
    size_t i = 0;
    while (i < n) {
        const unsigned c = p[i];
        if (c < 0x80) {
            ++i;
            continue;
        }
        size_t k;
        unsigned lo = 0x80, hi = 0xBF;
        if (c >= 0xC2 && c <= 0xDF) k = 1;
        else if (c == 0xE0) k = 2, lo = 0xA0;
        else if (c == 0xED) k = 2, hi = 0x9F;
        else if (c >= 0xE1 && c <= 0xEF) k = 2;
        else if (c == 0xF0) k = 3, lo = 0x90;
        else if (c >= 0xF1 && c <= 0xF3) k = 3;
        else if (c == 0xF4) k = 3, hi = 0x8F;
        else return false;
        if (i + k >= n) return false;
        if (p[i + 1] < lo || p[i + 1] > hi) return false;
        for (size_t j = 2; j <= k; ++j)
            if (p[i + j] < 0x80 || p[i + j] > 0xBF) return false;
        i += k + 1;
    }
    return true;
}

// the rows of rs the reference's loops reach, in their order (iter_chroms: chromosomes by first appearance, set order
// within one), with the assembly's chromosome ids; src = the row of rs
struct Rows {
    std::vector<uint32_t> chrom, start, end;
    std::vector<uint64_t> src;
};

gtars_status select_rows(const gtars_assembly *a, const gtars_regionset_t *rs, bool ignore_unk, Rows &r) {
    const uint64_t n = gtars_regionset_len(rs);
    const uint32_t nc = gtars_regionset_n_chrom(rs);
    const uint32_t *cid = gtars_regionset_chrom_ids(rs), *st = gtars_regionset_starts(rs), *en = gtars_regionset_ends(rs);
    std::vector<uint32_t> rank(nc, UINT32_MAX);  // first-appearance rank of a dictionary id
    std::vector<uint64_t> at;                    // rows per rank, then the rank's next output slot
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t &k = rank[cid[i]];
        if (k == UINT32_MAX) {
            k = (uint32_t)at.size();
            at.push_back(0);
        }
        ++at[k];
    }
    uint64_t sum = 0;
    for (uint64_t &v : at) {
        const uint64_t c = v;
        v = sum;
        sum += c;
    }
    std::vector<uint64_t> order(n);
    for (uint64_t i = 0; i < n; ++i) order[at[rank[cid[i]]]++] = i;
    std::vector<int64_t> aid(nc, -1);
    for (uint32_t k = 0; k < nc; ++k) {
        auto it = a->id.find(gtars_regionset_chrom_name(rs, k));
        if (it != a->id.end()) aid[k] = it->second;
    }
    for (uint64_t j = 0; j < n; ++j) {
        const uint64_t i = order[j];
        const int64_t c = aid[cid[i]];
        const bool ok = c >= 0 && (uint64_t)en[i] <= a->len[(size_t)c] && st[i] <= en[i];
        if (!ok) {
            if (ignore_unk) continue;
            const std::string chr = gtars_regionset_chrom_name(rs, cid[i]);
            const std::string why =
                c < 0 ? "Unknown chromosome found in region set: " + chr
                      : "Invalid range: start=" + std::to_string(st[i]) + ", end=" + std::to_string(en[i]) + " for chromosome " + chr +
                            " with length " + std::to_string(a->len[(size_t)c]);
            return fail(GTARS_ERR_INVALID_ARG, "Error getting sequence for region " + chr + ":" + std::to_string(st[i]) + "-" +
                                                   std::to_string(en[i]) + ": " + why);
        }
        r.chrom.push_back((uint32_t)c);
        r.start.push_back(st[i]);
        r.end.push_back(en[i]);
        r.src.push_back(i);
    }
    return GTARS_OK;
}

gtars_status counts_of(gtars_assembly *a, const Rows &r, int mode, std::vector<uint32_t> &counts) {
    const uint64_t n = r.src.size();
    counts.assign(n * (mode == GTARS_SEQ_GC ? 1 : 16), 0);
    if (!n) return GTARS_OK;
    gtars::Assembly *dev;
    if (const gtars_status e = assembly_device_image(a, &dev)) return e;
    return gtars::seqstats_counts(*dev, r.chrom.data(), r.start.data(), r.end.data(), n, mode, counts.data());
}

}  // namespace

extern "C" {

gtars_status gtars_assembly_from_fasta(const char *path, gtars_assembly_t **out) {
    return guarded([&]() -> gtars_status {
        if (!path || !out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        auto a = std::make_unique<gtars_assembly>();
        std::vector<FastaRecord> recs;
        if (const gtars_status e = read_fasta(path, a->blob, recs)) return e;
        for (const FastaRecord &r : recs) a->put(r.name, r.off, r.len);
        *out = a.release();
        return GTARS_OK;
    });
}

gtars_status gtars_assembly_from_fab(const char *path, gtars_assembly_t **out) {
    return guarded([&]() -> gtars_status {
        if (!path || !out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        auto a = std::make_unique<gtars_assembly>();
        {
            File in;
            if (const gtars_status e = open_regular(path, "rb", in)) return e;
            struct stat sb;
            if (fstat(fileno(in.f), &sb) == 0 && sb.st_size > 0) a->blob.reserve((size_t)sb.st_size);
            std::vector<char> buf(1 << 20);
            size_t k;
            while ((k = fread(buf.data(), 1, buf.size(), in.f)) > 0) a->blob.append(buf.data(), k);
            if (ferror(in.f)) return fail(GTARS_ERR_IO, std::string("Failed to read .fab file '") + path + "': " + strerror(errno));
        }
        const unsigned char *p = (const unsigned char *)a->blob.data();
        const uint64_t size = a->blob.size();
        if (size < 9) return fail(GTARS_ERR_PARSE, "Invalid .fab file: too short");
        if (memcmp(p, "GFAB", 4) != 0) return fail(GTARS_ERR_PARSE, "Invalid .fab file: bad magic bytes");
        if (p[4] != 1) return fail(GTARS_ERR_PARSE, "Unsupported .fab version: " + std::to_string(p[4]) + " (expected 1)");
        const uint64_t n_chroms = le(p + 5, 4);
        uint64_t pos = 9;
        for (uint64_t c = 0; c < n_chroms; ++c) {
            if (pos + 2 > size) return fail(GTARS_ERR_PARSE, "Invalid .fab file: truncated index");
            const uint64_t name_len = le(p + pos, 2);
            pos += 2;
            if (pos + name_len + 16 > size) return fail(GTARS_ERR_PARSE, "Invalid .fab file: truncated index entry");
            if (!valid_utf8(p + pos, (size_t)name_len)) return fail(GTARS_ERR_PARSE, "Invalid .fab file: non-UTF8 chromosome name");
            const std::string name((const char *)p + pos, (size_t)name_len);
            pos += name_len;
            const uint64_t o = le(p + pos, 8), l = le(p + pos + 8, 8);
            pos += 16;
            a->put(name, o, l);
        }
        // (the reference makes this check per query; every entry is checked, also one a later entry of its name replaces)
        for (size_t c = 0; c < a->names.size(); ++c)
            if (a->off[c] > size || a->len[c] > size - a->off[c])
                return fail(GTARS_ERR_PARSE, "Corrupted .fab file: sequence data for " + a->names[c] + " extends beyond file boundary");
        *out = a.release();
        return GTARS_OK;
    });
}

gtars_status gtars_fab_write_from_fasta(const char *fasta_path, const char *out_path) {
    return guarded([&]() -> gtars_status {
        if (!fasta_path || !out_path) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        std::string blob;
        std::vector<FastaRecord> recs;
        if (const gtars_status e = read_fasta(fasta_path, blob, recs)) return e;
        uint64_t header = 4 + 1 + 4;
        for (const FastaRecord &r : recs) {
            if (r.name.size() > 0xFFFF) return fail(GTARS_ERR_INVALID_ARG, "chromosome name longer than 65535 bytes");
            header += 2 + r.name.size() + 8 + 8;
        }
        if (recs.size() > 0xFFFFFFFFull) return fail(GTARS_ERR_INVALID_ARG, "too many records");
        std::string head("GFAB");
        head.push_back((char)1);
        put_le(head, recs.size(), 4);
        uint64_t at = header;
        for (const FastaRecord &r : recs) {
            put_le(head, r.name.size(), 2);
            head += r.name;
            put_le(head, at, 8);
            put_le(head, r.len, 8);
            at += r.len;
        }
        File o;
        o.f = fopen(out_path, "wb");
        if (!o.f) return fail(GTARS_ERR_IO, std::string("Failed to create .fab file '") + out_path + "': " + strerror(errno));
        // (the records' sequences lie back to back in blob, in file order)
        if (fwrite(head.data(), 1, head.size(), o.f) != head.size() || fwrite(blob.data(), 1, blob.size(), o.f) != blob.size() ||
            fflush(o.f) != 0)
            return fail(GTARS_ERR_IO, std::string("Failed to write .fab file '") + out_path + "': " + strerror(errno));
        return GTARS_OK;
    });
}

void gtars_assembly_free(gtars_assembly_t *a) { delete a; }
uint32_t gtars_assembly_n_chrom(const gtars_assembly_t *a) { return a ? (uint32_t)a->names.size() : 0; }
const char *gtars_assembly_chrom_name(const gtars_assembly_t *a, uint32_t id) {
    return a && id < a->names.size() ? a->names[id].c_str() : nullptr;
}
uint64_t gtars_assembly_chrom_len(const gtars_assembly_t *a, uint32_t id) { return a && id < a->len.size() ? a->len[id] : 0; }
int gtars_assembly_contains(const gtars_assembly_t *a, const char *name) { return a && name && a->id.count(name) ? 1 : 0; }

gtars_status gtars_assembly_sequence(const gtars_assembly_t *a, const char *name, uint64_t start, uint64_t end, const uint8_t **out) {
    return guarded([&]() -> gtars_status {
        if (!a || !name || !out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        auto it = a->id.find(name);
        if (it == a->id.end()) return fail(GTARS_ERR_INVALID_ARG, std::string("Unknown chromosome found in region set: ") + name);
        const uint64_t l = a->len[it->second];
        if (!(end <= l && start <= end))
            return fail(GTARS_ERR_INVALID_ARG, "Invalid range: start=" + std::to_string(start) + ", end=" + std::to_string(end) +
                                                   " for chromosome " + name + " with length " + std::to_string(l));
        *out = (const uint8_t *)a->blob.data() + a->off[it->second] + start;
        return GTARS_OK;
    });
}

int gtars_assembly_device(const gtars_assembly_t *a) {
    if (!a) return -1;
    std::lock_guard<std::mutex> lk(const_cast<gtars_assembly_t *>(a)->mu);
    return gtars::assembly_device(a->dev);
}

// include/gtars_amd_debug.h: forge the device id the image records (tests of the device-affinity checks on a one-GPU box)
int gtars_debug_set_assembly_device(void *assembly, int device) {
    gtars_assembly_t *a = (gtars_assembly_t *)assembly;
    if (!a) return -1;
    std::lock_guard<std::mutex> lk(a->mu);
    return a->dev ? gtars::assembly_set_device(a->dev, device) : -1;
}

uint64_t gtars_debug_seq_stage_blocks(void) { return gtars::assembly_stage_blocks(); }

uint32_t gtars_seqstats_piece_bytes(void) { return gtars::SEQ_PIECE; }

gtars_status gtars_seqstats_counts_device(gtars_assembly_t *a, const uint32_t *d_chrom, const uint32_t *d_start,
                                          const uint32_t *d_end, uint64_t n, int mode, uint32_t *d_out, void *stream) {
    return guarded([&]() -> gtars_status {
        if (!a) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (mode != GTARS_SEQ_GC && mode != GTARS_SEQ_DINUCL)
            return fail(GTARS_ERR_INVALID_ARG, "seqstats: unknown mode " + std::to_string(mode));
        if (!n) return GTARS_OK;
        gtars::Assembly *dev;
        if (const gtars_status e = assembly_device_image(a, &dev)) return e;
        return gtars::seqstats_counts_device(*dev, d_chrom, d_start, d_end, n, mode, d_out, stream);
    });
}

gtars_status gtars_seqstats_gc(gtars_assembly_t *a, const gtars_regionset_t *rs, int ignore_unk, double **gc, uint64_t *n_out) {
    return guarded([&]() -> gtars_status {
        if (!a || !rs || !gc || !n_out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *gc = nullptr, *n_out = 0;
        Rows r;
        if (const gtars_status e = select_rows(a, rs, ignore_unk != 0, r)) return e;
        std::vector<uint32_t> counts;
        if (const gtars_status e = counts_of(a, r, GTARS_SEQ_GC, counts)) return e;
        const uint64_t n = r.src.size();
        MallocArray<double> o;
        if (!o.alloc(n)) return fail(GTARS_ERR_INTERNAL, "out of host memory");
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t total = r.end[i] - r.start[i];
            o.p[i] = total ? (double)counts[i] / (double)total : 0.0;
        }
        *gc = o.release();
        *n_out = n;
        return GTARS_OK;
    });
}

gtars_status gtars_seqstats_dinucl(gtars_assembly_t *a, const gtars_regionset_t *rs, int raw_counts, int ignore_unk,
                                   uint64_t **row_index, double **freq, uint64_t *n_out) {
    return guarded([&]() -> gtars_status {
        if (!a || !rs || !row_index || !freq || !n_out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *row_index = nullptr, *freq = nullptr, *n_out = 0;
        Rows r;
        if (const gtars_status e = select_rows(a, rs, ignore_unk != 0, r)) return e;
        std::vector<uint32_t> counts;
        if (const gtars_status e = counts_of(a, r, GTARS_SEQ_DINUCL, counts)) return e;
        const uint64_t n = r.src.size();
        MallocArray<uint64_t> idx;
        MallocArray<double> o;
        if (!idx.alloc(n) || !o.alloc(n * 16)) return fail(GTARS_ERR_INTERNAL, "out of host memory");
        for (uint64_t i = 0; i < n; ++i) {
            idx.p[i] = r.src[i];
            const uint32_t *c = &counts[i * 16];
            uint64_t total = 0;
            for (int k = 0; k < 16; ++k) total += c[k];
            for (int k = 0; k < 16; ++k)
                o.p[i * 16 + k] = raw_counts ? (double)c[k] : total ? ((double)c[k] / (double)total) * 100.0 : 0.0;
        }
        *row_index = idx.release();
        *freq = o.release();
        *n_out = n;
        return GTARS_OK;
    });
}

}  // extern "C"
