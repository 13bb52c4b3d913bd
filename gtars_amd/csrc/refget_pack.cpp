// refget_pack.cpp -- the host layer of K22 (the encoded storage mode and the `.seq` files of a refget store:
// gtars-refget/src/digest/encoder.rs, store/readonly.rs:1528-1568, store/persistence.rs:37-59): the scalar calls on
// refget_pack_core.h, the packed-image handle with its host copy and its lazy device image, the `.seq` file readers and
// writers, the host paths, and the column calls on top of refget_pack.hip.  Declared in include/gtars_amd_host.h (the
// entry on device columns in include/gtars_amd.h).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/gtars_amd_host.h"
#include "assembly.h"
#include "guard.h"
#include "host_threads.h"
#include "refget_pack.h"
#include "refget_seqcol.h"

namespace gtars {
unsigned host_threads_for(unsigned cap);
}  // namespace gtars
using gtars::fail;
using gtars::guarded;

// The packed image of a collection: its host copy (laid out as the device image is, rg_image_layout) and, from the first
// device call on, the device image.
struct gtars_seqpack {
    std::vector<uint64_t> len, off, n_bytes;
    std::vector<uint8_t> cls;
    std::vector<uint64_t> image;  // (u64: the records' bases are 8-byte aligned for RgPackedRow)
    uint64_t bytes = 0;
    std::mutex mu;  // guards the lazy device image
    gtars::PackedImage *dev = nullptr;
    ~gtars_seqpack() { gtars::packed_free(dev); }
    uint8_t *at(size_t r) { return (uint8_t *)image.data() + off[r]; }
    const uint8_t *at(size_t r) const { return (const uint8_t *)image.data() + off[r]; }
    void layout(const uint64_t *length, const uint8_t *alphabet, size_t n) {
        len.assign(length, length + n), cls.assign(alphabet, alphabet + n);
        off.resize(n), n_bytes.resize(n);
        bytes = gtars::rg_image_layout(len.data(), cls.data(), n, off.data(), n_bytes.data());
        image.assign((size_t)(bytes >> 3), 0);
    }
};

namespace {

constexpr uint64_t PK_MAX_N = 0x7FFFFFF0u;
constexpr uint64_t PK_CHUNK_GROUPS = 1u << 14;  // 2^20 symbols per host task

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

gtars_status check_classes(const uint8_t *alphabet, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i)
        if (alphabet[i] > gtars::RG_UNKNOWN) return fail(GTARS_ERR_INVALID_ARG, "refget: alphabet class out of range");
    return GTARS_OK;
}

// the whole file into dst[0, want); a file of another size is a parse error that names it
gtars_status read_exact(const char *path, uint8_t *dst, uint64_t want, const char *what) {
    FILE *f = fopen(path, "rb");
    if (!f) return fail(GTARS_ERR_IO, std::string("cannot open ") + path);
    struct Close {
        FILE *f;
        ~Close() { fclose(f); }
    } closer{f};
    if (fseek(f, 0, SEEK_END) != 0) return fail(GTARS_ERR_IO, std::string("cannot read ") + path);
    const long size = ftell(f);
    if (size < 0 || (uint64_t)size != want)
        return fail(GTARS_ERR_PARSE, std::string(path) + ": " + std::to_string(size) + " bytes, " + what + " needs " + std::to_string(want));
    rewind(f);
    if (want && fread(dst, 1, (size_t)want, f) != want) return fail(GTARS_ERR_IO, std::string("cannot read ") + path);
    return GTARS_OK;
}

gtars_status write_whole(const char *path, const uint8_t *src, uint64_t n) {
    FILE *f = fopen(path, "wb");
    if (!f) return fail(GTARS_ERR_IO, std::string("cannot create ") + path);
    const bool ok = !n || fwrite(src, 1, (size_t)n, f) == n;
    if (fclose(f) != 0 || !ok) return fail(GTARS_ERR_IO, std::string("cannot write ") + path);
    return GTARS_OK;
}

// body(i) -> status for every i on the host threads; the first failure's status (its message is the thread's own, so it is
// taken along and recorded again on the calling thread)
template <class F>
gtars_status for_each_status(size_t n, unsigned threads, F &&body) {
    std::mutex mu;
    gtars_status first = GTARS_OK;
    std::string message;
    gtars::parallel_for(n, threads, 1, [&](size_t i) {
        const gtars_status e = body(i);
        if (!e) return;
        std::lock_guard<std::mutex> lock(mu);
        if (!first) first = e, message = gtars_last_error();
    });
    return first ? fail(first, message) : GTARS_OK;
}

// the pack's device image, built at the first call on the device current then
gtars_status device_image(gtars_seqpack *p, gtars::PackedImage **out) {
    std::lock_guard<std::mutex> lock(p->mu);
    if (!p->dev) {
        if (const gtars_status e = gtars::packed_upload((const uint8_t *)p->image.data(), p->bytes, p->off.data(), p->len.data(), p->cls.data(),
                                                         (uint32_t)p->len.size(), &p->dev))
            return e;
    }
    *out = p->dev;
    return GTARS_OK;
}

// rows on the host threads: statuses, the scanned offsets, the decoded bytes
void host_substrings(const gtars_seqpack &p, const uint32_t *seq, const uint64_t *start, const uint64_t *end, uint64_t n, unsigned threads,
                     uint8_t *status, std::vector<uint64_t> &off, std::vector<uint8_t> &out) {
    std::vector<uint32_t> cnt((size_t)n);
    off.assign((size_t)n + 1, 0);
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t st =
            seq[i] < p.len.size() ? gtars::refget_sub_status(start[i], end[i], p.len[seq[i]], &cnt[i]) : (cnt[i] = 0, (uint8_t)gtars::RG_SUB_NO_SEQUENCE);
        if (status) status[i] = st;
        off[i + 1] = off[i] + cnt[i];
    }
    out.resize((size_t)off[n]);
    gtars::parallel_for((size_t)n, threads, 256, [&](size_t i) {
        if (!cnt[i]) return;
        gtars::RgPackedRow row;
        row.open((const uint64_t *)p.at(seq[i]), p.cls[seq[i]], start[i]);
        uint8_t *dst = out.data() + off[i];
        for (uint32_t k = 0; k < cnt[i]; ++k) dst[k] = (uint8_t)row.byte(k);
    });
}

gtars_status hand_over(const std::vector<uint64_t> &off, const std::vector<uint8_t> &out, uint64_t **offsets, uint8_t **bytes) {
    *offsets = malloc_copy(off.data(), off.size());
    *bytes = malloc_copy(out.data(), out.size());
    if (!*offsets || !*bytes) {
        free(*offsets), free(*bytes);
        *offsets = nullptr, *bytes = nullptr;
        return fail(GTARS_ERR_INTERNAL, "out of host memory");
    }
    return GTARS_OK;
}

gtars_status substrings(gtars_seqpack *p, const uint32_t *seq, const uint64_t *start, const uint64_t *end, uint64_t n, int on_host,
                        uint32_t threads, uint8_t *status, uint64_t **offsets, uint8_t **bytes) {
    std::vector<uint64_t> off(1, 0);
    std::vector<uint8_t> out;
    if (on_host) {
        host_substrings(*p, seq, start, end, n, threads_of(threads), status, off, out);
    } else if (n) {
        gtars::PackedImage *image;
        if (const gtars_status e = device_image(p, &image)) return e;
        gtars::RefgetSubCall call;
        call.seq = seq, call.start = start, call.end = end, call.n = n, call.status = status, call.off = &off, call.bytes = &out;
        if (const gtars_status e = gtars::packed_sub_run(*image, call)) return e;
    }
    off.resize((size_t)n + 1, off.back());
    return hand_over(off, out, offsets, bytes);
}

// a collection over n raw sequences whose bytes fill(i, dst) puts into the blob; names are the record numbers
template <class Fill>
gtars_status seqcol_of(const uint64_t *length, uint64_t n, unsigned threads, Fill &&fill, gtars_seqcol_t **out) {
    if (n > PK_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "refget: too many records");
    auto c = std::make_unique<gtars_seqcol>();
    uint64_t total = 0;
    c->recs.resize((size_t)n);
    for (size_t i = 0; i < n; ++i) {
        gtars::RefgetRecord &r = c->recs[i];
        r.name = std::to_string(i), r.off = total, r.len = length[i];
        total += length[i];
    }
    c->a.blob.resize((size_t)total);
    if (const gtars_status e = for_each_status((size_t)n, threads, [&](size_t i) { return fill(i, (uint8_t *)&c->a.blob[0] + c->recs[i].off); }))
        return e;
    c->has_bytes = true;
    for (size_t i = 0; i < n; ++i) {
        const gtars::RefgetRecord &r = c->recs[i];
        c->a.id[r.name] = (uint32_t)i;
        c->a.names.push_back(r.name), c->a.off.push_back(r.off), c->a.len.push_back(r.len);
    }
    *out = c.release();
    return GTARS_OK;
}

}  // namespace

extern "C" {

uint32_t gtars_refget_bits(int alphabet) { return gtars::rg_bits_of((uint32_t)alphabet); }

gtars_status gtars_refget_encode(const void *seq, uint64_t n, int alphabet, uint8_t *out, uint64_t cap, uint64_t *n_bytes) {
    return guarded([&]() -> gtars_status {
        if ((!seq && n) || !n_bytes) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (alphabet < 0 || alphabet > gtars::RG_UNKNOWN) return fail(GTARS_ERR_INVALID_ARG, "refget: alphabet class out of range");
        *n_bytes = gtars::rg_packed_bytes(n, gtars::rg_bits_of((uint32_t)alphabet));
        if (*n_bytes > cap || (*n_bytes && !out))
            return fail(GTARS_ERR_CAPACITY, "refget: the encoding does not fit: need " + std::to_string(*n_bytes));
        gtars::rg_encode_record((const uint8_t *)seq, n, (uint32_t)alphabet, out);
        return GTARS_OK;
    });
}

gtars_status gtars_refget_decode(const uint8_t *packed, uint64_t n_packed, uint64_t byte_offset, uint64_t start, uint64_t end, int alphabet,
                                 uint8_t *out) {
    return guarded([&]() -> gtars_status {
        if ((!packed && n_packed) || (!out && end > start)) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (alphabet < 0 || alphabet > gtars::RG_UNKNOWN) return fail(GTARS_ERR_INVALID_ARG, "refget: alphabet class out of range");
        gtars::rg_decode_window(packed, n_packed, byte_offset, start, end, (uint32_t)alphabet, out);
        return GTARS_OK;
    });
}

void gtars_refget_byte_range(uint64_t start, uint64_t end, uint32_t bits, uint64_t *b0, uint64_t *b1) {
    if (b0 && b1) gtars::rg_byte_range(start, end, bits, b0, b1);
}

gtars_status gtars_seqpack_from_seqcol(gtars_seqcol_t *c, const uint8_t *alphabet, int on_host, uint32_t threads, gtars_seqpack_t **out) {
    return guarded([&]() -> gtars_status {
        if (!c || !out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        if (!c->has_bytes) return fail(GTARS_ERR_INVALID_ARG, "refget: the collection was read without its sequence data");
        const size_t n = c->recs.size();
        std::vector<uint8_t> cls(n);
        if (alphabet) cls.assign(alphabet, alphabet + n);
        else if (c->has_digests)
            for (size_t i = 0; i < n; ++i) cls[i] = c->digests[i].cls;
        else return fail(GTARS_ERR_INVALID_ARG, "refget: the collection has no alphabet classes and none were given");
        if (const gtars_status e = check_classes(cls.data(), n)) return e;
        auto p = std::make_unique<gtars_seqpack>();
        p->layout(c->a.len.data(), cls.data(), n);
        if (on_host) {
            // one task per 2^20 symbols of a record: a task's groups end on whole 64-bit words of the encoding
            std::vector<std::pair<uint32_t, uint64_t>> tasks;
            for (size_t r = 0; r < n; ++r)
                for (uint64_t g = 0; 64 * g < p->len[r]; g += PK_CHUNK_GROUPS) tasks.emplace_back((uint32_t)r, g);
            const uint8_t *base = (const uint8_t *)c->a.blob.data();
            gtars::parallel_for(tasks.size(), threads_of(threads), 1, [&](size_t t) {
                const uint32_t r = tasks[t].first;
                gtars::rg_encode_groups(base + c->a.off[r], p->len[r], p->cls[r], p->at(r), tasks[t].second, tasks[t].second + PK_CHUNK_GROUPS);
            });
        } else if (n) {
            gtars::Assembly *raw;
            if (const gtars_status e = gtars::assembly_device_image(&c->a, &raw)) return e;
            if (const gtars_status e = gtars::packed_from_raw(*raw, p->off.data(), p->len.data(), p->cls.data(), (uint32_t)n, p->bytes,
                                                              (uint8_t *)p->image.data(), &p->dev))
                return e;
        }
        *out = p.release();
        return GTARS_OK;
    });
}

gtars_status gtars_seqpack_from_files(const char *const *paths, const uint64_t *length, const uint8_t *alphabet, uint64_t n, uint32_t threads,
                                      gtars_seqpack_t **out) {
    return guarded([&]() -> gtars_status {
        if (!out || (n && (!paths || !length || !alphabet))) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        if (n > PK_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "refget: too many records");
        if (const gtars_status e = check_classes(alphabet, n)) return e;
        auto p = std::make_unique<gtars_seqpack>();
        p->layout(length, alphabet, (size_t)n);
        // the bytes as the files have them: nothing is decoded here
        if (const gtars_status e = for_each_status((size_t)n, threads_of(threads), [&](size_t i) {
                return paths[i] ? read_exact(paths[i], p->at(i), p->n_bytes[i], "the packed record") : fail(GTARS_ERR_INVALID_ARG, "NULL argument");
            }))
            return e;
        *out = p.release();
        return GTARS_OK;
    });
}

gtars_status gtars_seqpack_from_buffers(const uint8_t *const *packed, const uint64_t *n_packed, const uint64_t *length, const uint8_t *alphabet,
                                        uint64_t n, gtars_seqpack_t **out) {
    return guarded([&]() -> gtars_status {
        if (!out || (n && (!packed || !n_packed || !length || !alphabet))) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        if (n > PK_MAX_N) return fail(GTARS_ERR_INVALID_ARG, "refget: too many records");
        if (const gtars_status e = check_classes(alphabet, n)) return e;
        auto p = std::make_unique<gtars_seqpack>();
        p->layout(length, alphabet, (size_t)n);
        for (size_t i = 0; i < n; ++i) {
            if (n_packed[i] != p->n_bytes[i])
                return fail(GTARS_ERR_PARSE, "record " + std::to_string(i) + ": " + std::to_string(n_packed[i]) + " bytes, the packed record needs " +
                                                 std::to_string(p->n_bytes[i]));
            if (n_packed[i]) memcpy(p->at(i), packed[i], (size_t)n_packed[i]);
        }
        *out = p.release();
        return GTARS_OK;
    });
}

void gtars_seqpack_free(gtars_seqpack_t *p) { delete p; }
uint64_t gtars_seqpack_len(const gtars_seqpack_t *p) { return p ? p->len.size() : 0; }
int gtars_seqpack_device(const gtars_seqpack_t *p) { return p ? gtars::packed_device(p->dev) : -1; }
uint64_t gtars_seqpack_image_bytes(const gtars_seqpack_t *p) { return p ? p->bytes : 0; }

gtars_status gtars_seqpack_record(const gtars_seqpack_t *p, uint64_t i, const uint8_t **bytes, uint64_t *n_bytes, uint64_t *length, int *alphabet) {
    return guarded([&]() -> gtars_status {
        if (!p || !bytes || !n_bytes || !length || !alphabet) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (i >= p->len.size()) return fail(GTARS_ERR_INVALID_ARG, "record index out of range");
        *bytes = p->at((size_t)i), *n_bytes = p->n_bytes[(size_t)i], *length = p->len[(size_t)i], *alphabet = p->cls[(size_t)i];
        return GTARS_OK;
    });
}

gtars_status gtars_seqpack_write_files(const gtars_seqpack_t *p, const char *const *paths, uint32_t threads) {
    return guarded([&]() -> gtars_status {
        if (!p || (!paths && !p->len.empty())) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        // (a NULL path: the record is not written)
        return for_each_status(p->len.size(), threads_of(threads),
                               [&](size_t i) { return paths[i] ? write_whole(paths[i], p->at(i), p->n_bytes[i]) : GTARS_OK; });
    });
}

gtars_status gtars_seqpack_substrings(gtars_seqpack_t *p, const uint32_t *seq, const uint64_t *start, const uint64_t *end, uint64_t n,
                                      int on_host, uint32_t threads, uint8_t *status, uint64_t **offsets, uint8_t **bytes) {
    return guarded([&]() -> gtars_status {
        if (!p || (n && (!seq || !start || !end)) || !offsets || !bytes) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *offsets = nullptr, *bytes = nullptr;
        return substrings(p, seq, start, end, n, on_host, threads, status, offsets, bytes);
    });
}

gtars_status gtars_seqpack_decode_records(gtars_seqpack_t *p, int on_host, uint32_t threads, uint64_t **offsets, uint8_t **bytes) {
    return guarded([&]() -> gtars_status {
        if (!p || !offsets || !bytes) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *offsets = nullptr, *bytes = nullptr;
        const size_t n = p->len.size();
        std::vector<uint32_t> seq(n);
        std::vector<uint64_t> start(n, 0);
        std::vector<uint8_t> status(n);
        for (size_t i = 0; i < n; ++i) seq[i] = (uint32_t)i;
        if (const gtars_status e = substrings(p, seq.data(), start.data(), p->len.data(), n, on_host, threads, status.data(), offsets, bytes))
            return e;
        for (size_t i = 0; i < n; ++i)
            if (status[i]) {
                free(*offsets), free(*bytes);
                *offsets = nullptr, *bytes = nullptr;
                return fail(GTARS_ERR_INVALID_ARG, "refget: record " + std::to_string(i) + " is too long to decode in one call");
            }
        return GTARS_OK;
    });
}

gtars_status gtars_refget_packed_substrings_device(gtars_seqpack_t *p, const uint32_t *d_seq, const uint64_t *d_start, const uint64_t *d_end,
                                                   uint64_t n, uint8_t *d_status, uint64_t *d_offsets, uint8_t *d_bytes, uint64_t cap,
                                                   uint64_t *total, void *stream) {
    return guarded([&]() -> gtars_status {
        if (!p) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        gtars::PackedImage *image;
        if (const gtars_status e = device_image(p, &image)) return e;
        gtars::RefgetSubCall call;
        call.seq = d_seq, call.start = d_start, call.end = d_end, call.n = n, call.status = d_status, call.on_device = true, call.stream = stream;
        call.d_off = d_offsets, call.d_bytes = d_bytes, call.cap = cap, call.total = total;
        return gtars::packed_sub_run(*image, call);
    });
}

gtars_status gtars_seqcol_from_seq_files(const char *const *paths, const uint64_t *length, uint64_t n, uint32_t threads, gtars_seqcol_t **out) {
    return guarded([&]() -> gtars_status {
        if (!out || (n && (!paths || !length))) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        return seqcol_of(length, n, threads_of(threads), [&](size_t i, uint8_t *dst) {
            return paths[i] ? read_exact(paths[i], dst, length[i], "the sequence") : fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        }, out);
    });
}

gtars_status gtars_seqcol_from_buffers(const uint8_t *const *seq, const uint64_t *length, uint64_t n, gtars_seqcol_t **out) {
    return guarded([&]() -> gtars_status {
        if (!out || (n && (!seq || !length))) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        return seqcol_of(length, n, 1, [&](size_t i, uint8_t *dst) {
            if (length[i]) memcpy(dst, seq[i], (size_t)length[i]);
            return GTARS_OK;
        }, out);
    });
}

gtars_status gtars_seqcol_write_files(const gtars_seqcol_t *c, const char *const *paths, uint32_t threads) {
    return guarded([&]() -> gtars_status {
        if (!c || (!paths && !c->recs.empty())) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (!c->has_bytes) return fail(GTARS_ERR_INVALID_ARG, "refget: the collection was read without its sequence data");
        return for_each_status(c->recs.size(), threads_of(threads), [&](size_t i) {
            if (!paths[i]) return (gtars_status)GTARS_OK;
            const gtars::RefgetRecord &r = c->recs[i];
            std::vector<uint8_t> up((size_t)r.len);
            const uint8_t *src = (const uint8_t *)c->a.blob.data() + r.off;
            for (size_t k = 0; k < up.size(); ++k) up[k] = gtars::refget_upper(src[k]);
            return write_whole(paths[i], up.data(), r.len);
        });
    });
}

}  // extern "C"
