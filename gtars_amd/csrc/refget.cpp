// refget.cpp -- the host layer of K21 (gtars_amd.refget; gtars-refget/src/digest, store/readonly.rs): the FASTA reader on
// top of the record walk of refget_core.h, the sequence-collection handle with its per-record digests and collection
// digests, the host paths, and the column calls on top of refget.hip.  Declared in include/gtars_amd_host.h (the two
// entries on device columns in include/gtars_amd.h).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/gtars_amd_host.h"
#include "assembly.h"
#include "guard.h"
#include "host_threads.h"
#include "refget.h"
#include "refget_core.h"
#include "refget_seqcol.h"

namespace gtars {
unsigned host_threads_for(unsigned cap);
bool read_file_by_magic(const std::string &path, std::string &out, std::string &err);
}  // namespace gtars
using gtars::fail;
using gtars::guarded;

namespace {

unsigned threads_of(uint32_t threads) {
    const unsigned most = gtars::host_threads_for(0xFFFFFFFFu);
    return threads ? std::min<unsigned>(threads, most) : most;
}

template <class T>
T *malloc_copy(const T *src, size_t n) {
    T *p = (T *)malloc((n ? n : 1) * sizeof(T));
    if (p && n) memcpy(p, src, n * sizeof(T));
    return p;
}

// every record's digests: on the host threads, or -- the rows up to GTARS_REFGET_HOST_LEN bytes -- on the device, from an
// image of those rows alone, while the host threads hash the longer ones
gtars_status digest_records(gtars_seqcol &c, const std::string &blob, bool on_host, unsigned threads) {
    const size_t n = c.recs.size();
    c.digests.assign(n, gtars::RefgetDigest());
    const uint8_t *base = (const uint8_t *)blob.data();
    auto one = [&](size_t i) { gtars::refget_digest_host(base + c.recs[i].off, c.recs[i].len, c.digests[i]); };
    if (on_host) {
        gtars::parallel_for(n, threads, 1, one);
        return GTARS_OK;
    }
    const uint64_t host_len = gtars::refget_host_len();
    std::vector<size_t> on_dev, on_cpu;
    for (size_t i = 0; i < n; ++i) (c.recs[i].len <= host_len ? on_dev : on_cpu).push_back(i);
    std::vector<const uint8_t *> seq(on_dev.size());
    std::vector<uint64_t> len(on_dev.size());
    for (size_t k = 0; k < on_dev.size(); ++k) seq[k] = base + c.recs[on_dev[k]].off, len[k] = c.recs[on_dev[k]].len;
    gtars::Assembly *image = nullptr;
    if (const gtars_status e = gtars::assembly_build(seq.data(), len.data(), (uint32_t)on_dev.size(), &image)) return e;
    struct Free {
        gtars::Assembly *p;
        ~Free() { gtars::assembly_free(p); }
    } owner{image};
    std::vector<char> text(on_dev.size() * 32);
    std::vector<uint8_t> md5(on_dev.size() * 16), cls(on_dev.size());
    gtars::RefgetDigestCall call;
    call.n = on_dev.size(), call.digest = text.data(), call.md5 = md5.data(), call.cls = cls.data();
    call.h_seq = seq.data(), call.h_len = len.data(), call.threads = threads;
    call.meanwhile = [&]() { gtars::parallel_for(on_cpu.size(), threads, 1, [&](size_t k) { one(on_cpu[k]); }); };
    if (const gtars_status e = gtars::refget_digest_run(*image, call)) return e;
    for (size_t k = 0; k < on_dev.size(); ++k) {
        gtars::RefgetDigest &d = c.digests[on_dev[k]];
        memcpy(d.text, &text[k * 32], 32), memcpy(d.md5, &md5[k * 16], 16), d.cls = cls[k];
    }
    return GTARS_OK;
}

gtars_status collection_from(const char *text, size_t n, bool gzip, int flags, uint32_t threads, gtars_seqcol_t **out) {
    auto c = std::make_unique<gtars_seqcol>();
    c->gzip = gzip;
    std::string &blob = c->a.blob;
    gtars::refget_walk_fasta(text, n, blob, c->recs);
    if (c->recs.size() > 0x7FFFFFF0u) return fail(GTARS_ERR_INVALID_ARG, "refget: too many records");
    if (!(flags & GTARS_SEQCOL_NO_DIGESTS)) {
        if (const gtars_status e = digest_records(*c, blob, (flags & GTARS_SEQCOL_ON_HOST) != 0, threads_of(threads))) return e;
        c->has_digests = true;
        std::vector<std::string> names, digests;
        std::vector<uint64_t> lengths;
        for (size_t i = 0; i < c->recs.size(); ++i) {
            names.push_back(c->recs[i].name);
            lengths.push_back(c->recs[i].len);
            digests.emplace_back(c->digests[i].text, 32);
        }
        gtars::refget_collection_digests(names, lengths, digests, c->col);
    }
    if (flags & GTARS_SEQCOL_KEEP_BYTES) {
        c->has_bytes = true;
        for (size_t i = 0; i < c->recs.size(); ++i) {
            const gtars::RefgetRecord &r = c->recs[i];
            c->a.id[r.name] = (uint32_t)i;  // (the last record of a name)
            c->a.names.push_back(r.name), c->a.off.push_back(r.off), c->a.len.push_back(r.len);
        }
    } else {
        std::string().swap(blob);
    }
    *out = c.release();
    return GTARS_OK;
}

gtars_status need_bytes(const gtars_seqcol_t *c) {
    return c->has_bytes ? GTARS_OK : fail(GTARS_ERR_INVALID_ARG, "refget: the collection was read without its sequence data");
}

}  // namespace

extern "C" {

gtars_status gtars_md5(const void *data, uint64_t n, char *out33) {
    return guarded([&]() -> gtars_status {
        if ((!data && n) || !out33) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        uint8_t d[16];
        gtars::md5((const uint8_t *)data, (size_t)n, d);
        gtars::md5_hex(d, out33);
        out33[32] = '\0';
        return GTARS_OK;
    });
}

int gtars_refget_alphabet(const void *data, uint64_t n) {
    uint32_t mask = 0;
    for (uint64_t i = 0; data && i < n; ++i) mask |= 1u << gtars::refget_class(((const uint8_t *)data)[i]);
    return gtars::refget_guess(mask);
}

void gtars_refget_class_table(uint8_t *out256) {
    for (int b = 0; out256 && b < 256; ++b) out256[b] = gtars::refget_class((uint8_t)b);
}

uint32_t gtars_refget_host_len(void) { return gtars::refget_host_len(); }

gtars_status gtars_seqcol_from_fasta(const char *path, int flags, uint32_t threads, gtars_seqcol_t **out) {
    return guarded([&]() -> gtars_status {
        if (!path || !out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        bool gzip = false;
        if (FILE *f = fopen(path, "rb")) {
            unsigned char magic[2] = {0, 0};
            gzip = fread(magic, 1, 2, f) == 2 && magic[0] == 0x1f && magic[1] == 0x8b;
            fclose(f);
        }
        std::string text, err;
        if (!gtars::read_file_by_magic(path, text, err)) return fail(GTARS_ERR_IO, err);
        return collection_from(text.data(), text.size(), gzip, flags, threads, out);
    });
}

gtars_status gtars_seqcol_from_fasta_bytes(const void *text, uint64_t n, int flags, uint32_t threads, gtars_seqcol_t **out) {
    return guarded([&]() -> gtars_status {
        if ((!text && n) || !out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        return collection_from((const char *)text, (size_t)n, false, flags, threads, out);
    });
}

void gtars_seqcol_free(gtars_seqcol_t *c) { delete c; }
uint64_t gtars_seqcol_len(const gtars_seqcol_t *c) { return c ? c->recs.size() : 0; }
int gtars_seqcol_is_gzip(const gtars_seqcol_t *c) { return c && c->gzip; }
gtars_assembly_t *gtars_seqcol_assembly(gtars_seqcol_t *c) { return c && c->has_bytes ? &c->a : nullptr; }

gtars_status gtars_seqcol_record(const gtars_seqcol_t *c, uint64_t i, const char **name, const char **description, uint64_t *length,
                                 int *has_fai, uint64_t *fai_offset, uint32_t *line_bases, uint32_t *line_bytes, char *sha33, char *md5_33,
                                 int *alphabet, const uint8_t **bytes) {
    return guarded([&]() -> gtars_status {
        if (!c || !name || !description || !length || !has_fai || !fai_offset || !line_bases || !line_bytes || !sha33 || !md5_33 || !alphabet ||
            !bytes)
            return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (i >= c->recs.size()) return fail(GTARS_ERR_INVALID_ARG, "record index out of range");
        const gtars::RefgetRecord &r = c->recs[(size_t)i];
        *name = r.name.c_str(), *description = r.has_description ? r.description.c_str() : nullptr, *length = r.len;
        // (no FAI for gzip input: its offsets would be those of the inflated text)
        *has_fai = r.has_fai && !c->gzip, *fai_offset = r.fai_offset, *line_bases = r.line_bases, *line_bytes = r.line_bytes;
        sha33[0] = md5_33[0] = '\0';
        *alphabet = gtars::RG_UNKNOWN;
        if (c->has_digests) {
            const gtars::RefgetDigest &d = c->digests[(size_t)i];
            memcpy(sha33, d.text, 32), sha33[32] = '\0';
            gtars::md5_hex(d.md5, md5_33), md5_33[32] = '\0';
            *alphabet = d.cls;
        }
        *bytes = c->has_bytes ? (const uint8_t *)c->a.blob.data() + r.off : nullptr;
        return GTARS_OK;
    });
}

gtars_status gtars_seqcol_digests(const gtars_seqcol_t *c, char *out7x33) {
    return guarded([&]() -> gtars_status {
        if (!c || !out7x33) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (!c->has_digests) return fail(GTARS_ERR_INVALID_ARG, "refget: the collection was read without digests");
        const std::string *all[7] = {&c->col.top,  &c->col.names, &c->col.sequences, &c->col.lengths, &c->col.name_length_pairs,
                                     &c->col.sorted_name_length_pairs, &c->col.sorted_sequences};
        for (int k = 0; k < 7; ++k) memcpy(out7x33 + 33 * k, all[k]->c_str(), 33);
        return GTARS_OK;
    });
}

gtars_status gtars_seqcol_substrings(gtars_seqcol_t *c, const uint32_t *seq, const uint64_t *start, const uint64_t *end, uint64_t n, int on_host,
                                     uint32_t threads, uint8_t *status, uint64_t **offsets, uint8_t **bytes) {
    return guarded([&]() -> gtars_status {
        if (!c || (n && (!seq || !start || !end)) || !offsets || !bytes) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *offsets = nullptr, *bytes = nullptr;
        if (const gtars_status e = need_bytes(c)) return e;
        std::vector<uint64_t> off(1, 0);
        std::vector<uint8_t> out;
        if (on_host) {
            std::vector<uint32_t> cnt((size_t)n);
            off.resize((size_t)n + 1);
            for (uint64_t i = 0; i < n; ++i) {
                const uint8_t st = seq[i] < c->recs.size() ? gtars::refget_sub_status(start[i], end[i], c->recs[seq[i]].len, &cnt[i])
                                                           : (cnt[i] = 0, (uint8_t)gtars::RG_SUB_NO_SEQUENCE);
                if (status) status[i] = st;
                off[i + 1] = off[i] + cnt[i];
            }
            out.resize((size_t)off[n]);
            const uint8_t *base = (const uint8_t *)c->a.blob.data();
            gtars::parallel_for((size_t)n, threads_of(threads), 1024, [&](size_t i) {
                if (!cnt[i]) return;
                const uint8_t *src = base + c->recs[seq[i]].off + start[i];
                uint8_t *dst = out.data() + off[i];
                for (uint32_t k = 0; k < cnt[i]; ++k) dst[k] = gtars::refget_upper(src[k]);
            });
        } else if (n) {
            gtars::Assembly *image;
            if (const gtars_status e = gtars::assembly_device_image(&c->a, &image)) return e;
            gtars::RefgetSubCall call;
            call.seq = seq, call.start = start, call.end = end, call.n = n, call.status = status, call.off = &off, call.bytes = &out;
            if (const gtars_status e = gtars::refget_sub_run(*image, call)) return e;
        }
        off.resize((size_t)n + 1, off.back());
        *offsets = malloc_copy(off.data(), off.size());
        *bytes = malloc_copy(out.data(), out.size());
        if (!*offsets || !*bytes) {
            free(*offsets), free(*bytes);
            *offsets = nullptr, *bytes = nullptr;
            return fail(GTARS_ERR_INTERNAL, "out of host memory");
        }
        return GTARS_OK;
    });
}

gtars_status gtars_seqcol_digest_records(gtars_seqcol_t *c, int on_host, uint32_t threads, char *digests, uint8_t *md5, uint8_t *alphabet) {
    return guarded([&]() -> gtars_status {
        if (!c) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (const gtars_status e = need_bytes(c)) return e;
        const size_t n = c->recs.size();
        if (on_host) {
            const uint8_t *base = (const uint8_t *)c->a.blob.data();
            gtars::parallel_for(n, threads_of(threads), 1, [&](size_t i) {
                gtars::RefgetDigest d;
                gtars::refget_digest_host(base + c->recs[i].off, c->recs[i].len, d);
                if (digests) memcpy(digests + 32 * i, d.text, 32);
                if (md5) memcpy(md5 + 16 * i, d.md5, 16);
                if (alphabet) alphabet[i] = d.cls;
            });
            return GTARS_OK;
        }
        if (!n) return GTARS_OK;
        gtars::Assembly *image;
        if (const gtars_status e = gtars::assembly_device_image(&c->a, &image)) return e;
        std::vector<const uint8_t *> h_seq(n);
        for (size_t i = 0; i < n; ++i) h_seq[i] = (const uint8_t *)c->a.blob.data() + c->a.off[i];
        gtars::RefgetDigestCall call;
        call.n = n, call.digest = digests, call.md5 = md5, call.cls = alphabet;
        call.h_seq = h_seq.data(), call.h_len = c->a.len.data(), call.threads = threads_of(threads);
        return gtars::refget_digest_run(*image, call);
    });
}

gtars_status gtars_refget_digests_device(gtars_seqcol_t *c, char *d_digests, uint8_t *d_md5, uint8_t *d_class, void *stream) {
    return guarded([&]() -> gtars_status {
        if (!c) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (const gtars_status e = need_bytes(c)) return e;
        const size_t n = c->recs.size();
        if (!n) return GTARS_OK;
        gtars::Assembly *image;
        if (const gtars_status e = gtars::assembly_device_image(&c->a, &image)) return e;
        std::vector<const uint8_t *> h_seq(n);
        for (size_t i = 0; i < n; ++i) h_seq[i] = (const uint8_t *)c->a.blob.data() + c->a.off[i];
        gtars::RefgetDigestCall call;
        call.n = n, call.digest = d_digests, call.md5 = d_md5, call.cls = d_class, call.on_device = true, call.stream = stream;
        call.h_seq = h_seq.data(), call.h_len = c->a.len.data(), call.threads = threads_of(0);
        return gtars::refget_digest_run(*image, call);
    });
}

gtars_status gtars_refget_substrings_device(gtars_seqcol_t *c, const uint32_t *d_seq, const uint64_t *d_start, const uint64_t *d_end, uint64_t n,
                                            uint8_t *d_status, uint64_t *d_offsets, uint8_t *d_bytes, uint64_t cap, uint64_t *total,
                                            void *stream) {
    return guarded([&]() -> gtars_status {
        if (!c) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (const gtars_status e = need_bytes(c)) return e;
        gtars::Assembly *image;
        if (const gtars_status e = gtars::assembly_device_image(&c->a, &image)) return e;
        gtars::RefgetSubCall call;
        call.seq = d_seq, call.start = d_start, call.end = d_end, call.n = n, call.status = d_status, call.on_device = true, call.stream = stream;
        call.d_off = d_offsets, call.d_bytes = d_bytes, call.cap = cap, call.total = total;
        return gtars::refget_sub_run(*image, call);
    });
}

}  // extern "C"
