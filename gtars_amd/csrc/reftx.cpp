// reftx.cpp -- the host layer of K19 (gtars.reftx; gtars-refget/src/transcripts, gtars-python/src/reftx/mod.rs): the store
// builder with its cdot / MANE skip rules (builder.rs:64-208), the .reftx file, the scalar and column mapping calls on the
// host, the binding of a store to an assembly and the column calls on top of reftx.hip.  Declared in
// include/gtars_amd_host.h.  The rules themselves are reftx_core.h.
#include <sys/stat.h>
#include <unistd.h>

#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/gtars_amd_host.h"
#include "assembly.h"
#include "guard.h"
#include "host_threads.h"
#include "reftx.h"
#include "reftx_core.h"

namespace gtars {
unsigned host_threads_for(unsigned cap);
}  // namespace gtars
using gtars::fail;
using gtars::guarded;

struct gtars_txbuilder {
    std::vector<gtars::TxRecord> recs;
    std::unordered_map<std::string, std::array<uint8_t, 24>> chrom_to_digest;
    std::unordered_map<std::string, uint8_t> mane_flags;  // by full and by base accession
};

struct gtars_txstore {
    gtars::TxStoreData data;
    gtars::TxHostTables tables;  // chrom / seq_status unset: those belong to a binding
};

struct gtars_txbind {
    const gtars_txstore *store = nullptr;
    gtars_assembly *assembly = nullptr;
    gtars::TxHostTables tables;
    std::vector<const uint8_t *> h_seq;
    std::mutex mu;  // guards the lazy device tables
    gtars::TxDevice *dev = nullptr;
    ~gtars_txbind() { gtars::tx_device_free(dev); }
};

namespace {

unsigned threads_of(uint32_t threads) {
    const unsigned most = gtars::host_threads_for(0xFFFFFFFFu);
    return threads ? std::min<unsigned>(threads, most) : most;
}

// decode_chrom_digest (reftx/mod.rs:282-300)
gtars_status chrom_digest_of(const char *text, uint8_t out[24]) {
    long got = -1;
    if (gtars::tx_digest_decode(text, strlen(text), out, &got)) return GTARS_OK;
    if (got < 0) return fail(GTARS_ERR_INVALID_ARG, std::string("Invalid base64url chrom accession \"") + text + "\"");
    return fail(GTARS_ERR_INVALID_ARG, "Chrom accession must decode to 24 bytes, got " + std::to_string(got) + " (input: \"" + text + "\")");
}

void set_exons(gtars::TxRecord &r, const uint32_t *exons, uint64_t n_exons) {
    r.exons.resize((size_t)n_exons);
    for (uint64_t k = 0; k < n_exons; ++k) r.exons[k] = gtars::TxExon{exons[2 * k], exons[2 * k + 1]};
}

gtars_status store_from(const uint8_t *data, uint64_t n, gtars_txstore **out) {
    auto s = std::make_unique<gtars_txstore>();
    std::string err;
    if (!s->data.decode(data, n, err)) return fail(GTARS_ERR_PARSE, err);
    if (!s->tables.build(s->data.recs)) return fail(GTARS_ERR_CAPACITY, "reftx: the store has more than 2^32 - 2 exons");
    *out = s.release();
    return GTARS_OK;
}

void map_on_host(const gtars::TxTables &t, const uint32_t *tx, const uint8_t *kind, const int64_t *pos, const int64_t *off, const uint8_t *star,
                 uint64_t n, unsigned threads, uint64_t *out, uint8_t *status) {
    gtars::parallel_for((size_t)n, threads, 4096,
                        [&](size_t i) { status[i] = gtars::tx_map_one(t, tx[i], kind[i], pos[i], off ? off[i] : 0, star ? star[i] : 0u, &out[i]); });
}

gtars_status device_tables(gtars_txbind *b, gtars::Assembly **image, gtars::TxDevice **dev) {
    if (const gtars_status e = gtars::assembly_device_image(b->assembly, image)) return e;
    std::lock_guard<std::mutex> lk(b->mu);
    if (!b->dev)
        if (const gtars_status e = gtars::tx_device_build(**image, b->tables, &b->dev)) return e;
    *dev = b->dev;
    return GTARS_OK;
}

template <class T>
T *malloc_copy(const T *src, size_t n) {
    T *p = (T *)malloc((n ? n : 1) * sizeof(T));
    if (p && n) memcpy(p, src, n * sizeof(T));
    return p;
}

}  // namespace

namespace gtars {
TxBindParts tx_bind_parts(gtars_txbind *b) { return TxBindParts{&b->store->data, b->assembly, &b->tables, b->h_seq.data()}; }
gtars_status tx_bind_device(gtars_txbind *b, Assembly **image, TxDevice **dev) { return device_tables(b, image, dev); }
}  // namespace gtars

extern "C" {

gtars_status gtars_txbuilder_new(gtars_txbuilder_t **out) {
    return guarded([&]() -> gtars_status {
        if (!out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = new gtars_txbuilder();
        return GTARS_OK;
    });
}
void gtars_txbuilder_free(gtars_txbuilder_t *b) { delete b; }
uint64_t gtars_txbuilder_len(const gtars_txbuilder_t *b) { return b ? b->recs.size() : 0; }

gtars_status gtars_txbuilder_add(gtars_txbuilder_t *b, const char *accession, const char *gene, const char *chrom_accession, int strand,
                                 uint32_t cds_start, uint32_t cds_end, uint32_t mane_flags, const uint32_t *exons, uint64_t n_exons) {
    return guarded([&]() -> gtars_status {
        if (!b || !accession || !chrom_accession || (!exons && n_exons)) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (strand != 1 && strand != -1) return fail(GTARS_ERR_INVALID_ARG, "strand must be +1 or -1");
        gtars::TxRecord r;
        if (const gtars_status e = chrom_digest_of(chrom_accession, r.chrom_digest)) return e;
        r.accession = accession, r.gene = gene ? gene : "";
        r.strand = (int8_t)strand, r.mane = (uint8_t)(mane_flags & 3), r.cds_start = cds_start, r.cds_end = cds_end;
        set_exons(r, exons, n_exons);
        b->recs.push_back(std::move(r));
        return GTARS_OK;
    });
}

gtars_status gtars_txbuilder_add_chrom_mapping(gtars_txbuilder_t *b, const char *name, const char *chrom_accession) {
    return guarded([&]() -> gtars_status {
        if (!b || !name || !chrom_accession) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        std::array<uint8_t, 24> d;
        if (const gtars_status e = chrom_digest_of(chrom_accession, d.data())) return e;
        b->chrom_to_digest[name] = d;
        return GTARS_OK;
    });
}

gtars_status gtars_txbuilder_add_mane(gtars_txbuilder_t *b, const char *accession, uint32_t flags) {
    return guarded([&]() -> gtars_status {
        if (!b || !accession) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        const std::string acc = accession;
        b->mane_flags[acc] = (uint8_t)flags;
        const size_t dot = acc.find('.');
        if (dot != std::string::npos) b->mane_flags[acc.substr(0, dot)] = (uint8_t)flags;
        return GTARS_OK;
    });
}

gtars_status gtars_txbuilder_add_cdot(gtars_txbuilder_t *b, const char *id, const char *gene, const char *contig, int64_t strand,
                                      uint32_t cds_start, uint32_t cds_end, const uint32_t *exons, uint64_t n_exons, int *added) {
    return guarded([&]() -> gtars_status {
        if (!b || !id || !contig || (!exons && n_exons) || !added) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *added = 0;
        const auto chrom = b->chrom_to_digest.find(contig);
        if (chrom == b->chrom_to_digest.end() || (strand != 1 && strand != -1) || n_exons == 0) return GTARS_OK;
        gtars::TxRecord r;
        r.accession = id, r.gene = gene ? gene : "";
        memcpy(r.chrom_digest, chrom->second.data(), 24);
        r.strand = (int8_t)strand, r.cds_start = cds_start, r.cds_end = cds_end;
        auto flags = b->mane_flags.find(r.accession);
        if (flags == b->mane_flags.end()) flags = b->mane_flags.find(r.accession.substr(0, r.accession.find('.')));
        r.mane = flags == b->mane_flags.end() ? 0 : flags->second;
        set_exons(r, exons, n_exons);
        b->recs.push_back(std::move(r));
        *added = 1;
        return GTARS_OK;
    });
}

gtars_status gtars_txbuilder_bytes(const gtars_txbuilder_t *b, uint8_t **out, uint64_t *n) {
    return guarded([&]() -> gtars_status {
        if (!b || !out || !n) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr, *n = 0;
        std::string image, err;
        if (!gtars::tx_encode(b->recs, image, err)) return fail(GTARS_ERR_INVALID_ARG, err);
        *out = malloc_copy((const uint8_t *)image.data(), image.size());
        if (!*out) return fail(GTARS_ERR_INTERNAL, "out of host memory");
        *n = image.size();
        return GTARS_OK;
    });
}

gtars_status gtars_txbuilder_build(const gtars_txbuilder_t *b, const char *path) {
    return guarded([&]() -> gtars_status {
        if (!b || !path) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (b->recs.empty()) return fail(GTARS_ERR_EMPTY, "No transcripts to write");
        std::string image, err;
        if (!gtars::tx_encode(b->recs, image, err)) return fail(GTARS_ERR_INVALID_ARG, err);
        // a temporary file in the destination's directory, complete and flushed before it takes the name
        const std::string dest = path;
        const size_t slash = dest.rfind('/');
        const std::string tmp = (slash == std::string::npos ? std::string("./") : dest.substr(0, slash + 1)) + ".reftx.XXXXXX";
        std::vector<char> name(tmp.begin(), tmp.end());
        name.push_back('\0');
        const int fd = mkstemp(name.data());
        if (fd < 0) return fail(GTARS_ERR_IO, "creating temp file in the directory of " + dest);
        bool ok = true;
        for (size_t at = 0; ok && at < image.size();) {
            const ssize_t w = write(fd, image.data() + at, image.size() - at);
            if (w <= 0) ok = false;
            else at += (size_t)w;
        }
        ok = ok && fchmod(fd, 0644) == 0 && fsync(fd) == 0;  // (mkstemp's mode is 0600)
        ok = (close(fd) == 0) && ok;
        if (ok && rename(name.data(), dest.c_str()) != 0) ok = false;
        if (!ok) {
            unlink(name.data());
            return fail(GTARS_ERR_IO, "failed to atomically publish " + dest);
        }
        return GTARS_OK;
    });
}

gtars_status gtars_txstore_open(const char *path, gtars_txstore_t **out) {
    return guarded([&]() -> gtars_status {
        if (!path || !out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        FILE *f = fopen(path, "rb");
        if (!f) return fail(GTARS_ERR_IO, std::string("cannot open ") + path);
        std::string blob;
        char buf[1 << 16];
        size_t got;
        while ((got = fread(buf, 1, sizeof buf, f)) > 0) blob.append(buf, got);
        const bool bad = ferror(f);
        fclose(f);
        if (bad) return fail(GTARS_ERR_IO, std::string("cannot read ") + path);
        return store_from((const uint8_t *)blob.data(), blob.size(), out);
    });
}

gtars_status gtars_txstore_from_bytes(const uint8_t *data, uint64_t n, gtars_txstore_t **out) {
    return guarded([&]() -> gtars_status {
        if ((!data && n) || !out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        return store_from(data, n, out);
    });
}

void gtars_txstore_free(gtars_txstore_t *s) { delete s; }
uint64_t gtars_txstore_len(const gtars_txstore_t *s) { return s ? s->data.recs.size() : 0; }
int gtars_txstore_has_mane(const gtars_txstore_t *s) { return s && s->data.has_mane; }
int64_t gtars_txstore_lookup(const gtars_txstore_t *s, const char *accession) {
    return s && accession ? s->data.lookup(accession, strlen(accession)) : -1;
}
int64_t gtars_txstore_lookup_mane(const gtars_txstore_t *s, const char *gene) {
    try {
        return s && gene ? s->data.lookup_mane(gene) : -1;
    } catch (const std::exception &) {
        return -1;
    }
}

gtars_status gtars_txstore_lookup_many(const gtars_txstore_t *s, const uint8_t *pool, const uint64_t *offsets, uint64_t n, uint32_t threads,
                                       uint32_t *idx) {
    return guarded([&]() -> gtars_status {
        if (!s || (n && (!offsets || !idx)) || (n && !pool && offsets[n])) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        gtars::parallel_for((size_t)n, threads_of(threads), 4096, [&](size_t i) {
            const int64_t at = s->data.lookup((const char *)pool + offsets[i], (size_t)(offsets[i + 1] - offsets[i]));
            idx[i] = at < 0 ? gtars::TX_NONE : (uint32_t)at;
        });
        return GTARS_OK;
    });
}

gtars_status gtars_txstore_record(const gtars_txstore_t *s, uint64_t i, const char **accession, const char **gene, char *chrom33, int *strand,
                                  uint32_t *mane_flags, uint32_t *cds_start, uint32_t *cds_end, uint32_t *length, uint32_t *cds_length,
                                  const uint32_t **exons, uint64_t *n_exons) {
    return guarded([&]() -> gtars_status {
        if (!s || !accession || !gene || !chrom33 || !strand || !mane_flags || !cds_start || !cds_end || !length || !cds_length || !exons || !n_exons)
            return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (i >= s->data.recs.size()) return fail(GTARS_ERR_INVALID_ARG, "transcript index out of range");
        const gtars::TxRecord &r = s->data.recs[(size_t)i];
        *accession = r.accession.c_str(), *gene = r.gene.c_str();
        gtars::tx_digest_encode(r.chrom_digest, chrom33);
        chrom33[32] = '\0';
        *strand = r.strand, *mane_flags = r.mane, *cds_start = r.cds_start, *cds_end = r.cds_end;
        *length = r.transcript_length(), *cds_length = r.cds_length();
        static_assert(sizeof(gtars::TxExon) == 8, "exons leave as (start, end) pairs of u32");
        *exons = r.exons.empty() ? nullptr : &r.exons[0].start, *n_exons = r.exons.size();
        return GTARS_OK;
    });
}

gtars_status gtars_txstore_map(const gtars_txstore_t *s, const uint32_t *tx, const uint8_t *kind, const int64_t *pos, const int64_t *offset,
                               const uint8_t *star, uint64_t n, uint32_t threads, uint64_t *out, uint8_t *status) {
    return guarded([&]() -> gtars_status {
        if (!s || (n && (!tx || !kind || !pos || !out || !status))) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        map_on_host(s->tables.view(), tx, kind, pos, offset, star, n, threads_of(threads), out, status);
        return GTARS_OK;
    });
}

gtars_status gtars_txbind_new(const gtars_txstore_t *s, gtars_assembly_t *a, uint32_t threads, gtars_txbind_t **out) {
    return guarded([&]() -> gtars_status {
        if (!s || !a || !out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        const char *digests;
        if (const gtars_status e = gtars_assembly_refget_digests(a, threads, &digests)) return e;
        auto b = std::make_unique<gtars_txbind>();
        b->store = s, b->assembly = a, b->tables = s->tables;
        const size_t nc = a->names.size();
        std::map<std::string, uint32_t> by_digest;  // (a digest two chromosomes share names the first)
        for (size_t c = 0; c < nc; ++c) {
            uint8_t d[24];
            if (gtars::tx_digest_decode(digests + c * 33, 32, d)) by_digest.emplace(std::string((const char *)d, 24), (uint32_t)c);
            b->h_seq.push_back((const uint8_t *)a->blob.data() + a->off[c]);
        }
        gtars::TxHostTables &t = b->tables;
        for (size_t i = 0; i < s->data.recs.size(); ++i) {
            const gtars::TxRecord &r = s->data.recs[i];
            const auto it = by_digest.find(std::string((const char *)r.chrom_digest, 24));
            t.chrom[i] = it == by_digest.end() ? gtars::TX_NONE : it->second;
            uint8_t st = gtars::TXSEQ_OK;
            if (t.bad[i]) st = gtars::TXSEQ_BAD_EXONS;
            else if (t.len[i] == 0) st = gtars::TXSEQ_OK;  // (concat_regions answers "" before it looks the chromosome up)
            else if (it == by_digest.end()) st = gtars::TXSEQ_NO_SEQUENCE;
            else
                for (const gtars::TxExon &e : r.exons)
                    if (e.start < e.end && e.end > a->len[it->second]) st = gtars::TXSEQ_PAST_END;
            t.seq_status[i] = st;
        }
        *out = b.release();
        return GTARS_OK;
    });
}
void gtars_txbind_free(gtars_txbind_t *b) { delete b; }

gtars_status gtars_txbind_map(gtars_txbind_t *b, const uint32_t *tx, const uint8_t *kind, const int64_t *pos, const int64_t *offset,
                              const uint8_t *star, uint64_t n, int on_host, uint32_t threads, uint64_t *out, uint8_t *status) {
    return guarded([&]() -> gtars_status {
        if (!b || (n && (!tx || !kind || !pos || !out || !status))) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (on_host) {
            map_on_host(b->tables.view(), tx, kind, pos, offset, star, n, threads_of(threads), out, status);
            return GTARS_OK;
        }
        if (!n) return GTARS_OK;
        gtars::Assembly *image;
        gtars::TxDevice *dev;
        if (const gtars_status e = device_tables(b, &image, &dev)) return e;
        gtars::TxMapCall call;
        call.tx = tx, call.kind = kind, call.pos = pos, call.off = offset, call.star = star, call.n = n, call.out = out, call.status = status;
        return gtars::tx_map_run(*image, *dev, call);
    });
}

gtars_status gtars_tx_map_device(gtars_txbind_t *b, const uint32_t *d_tx, const uint8_t *d_kind, const int64_t *d_pos, const int64_t *d_offset,
                                 const uint8_t *d_star, uint64_t n, uint64_t *d_out, uint8_t *d_status, void *stream) {
    return guarded([&]() -> gtars_status {
        if (!b) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (!n) return GTARS_OK;
        gtars::Assembly *image;
        gtars::TxDevice *dev;
        if (const gtars_status e = device_tables(b, &image, &dev)) return e;
        gtars::TxMapCall call;
        call.tx = d_tx, call.kind = d_kind, call.pos = d_pos, call.off = d_offset, call.star = d_star, call.n = n;
        call.out = d_out, call.status = d_status, call.on_device = true, call.stream = stream;
        return gtars::tx_map_run(*image, *dev, call);
    });
}

gtars_status gtars_txbind_sequences(gtars_txbind_t *b, const uint32_t *idx, uint64_t n, int on_host, uint32_t threads, uint8_t *status,
                                    char *digests, uint64_t **seq_offsets, uint8_t **seq_bytes) {
    return guarded([&]() -> gtars_status {
        if (!b || (n && !idx) || (seq_offsets == nullptr) != (seq_bytes == nullptr)) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (seq_offsets) *seq_offsets = nullptr, *seq_bytes = nullptr;
        const unsigned nt = threads_of(threads);
        const gtars::TxTables t = b->tables.view();
        std::vector<uint64_t> off(1, 0);
        std::vector<uint8_t> bytes;
        if (on_host) {
            std::vector<std::string> seqs(seq_offsets ? (size_t)n : 0);
            gtars::parallel_for((size_t)n, nt, 16, [&](size_t i) {
                const uint32_t tx = idx[i];
                const uint8_t st = tx < t.n_tx ? t.seq_status[tx] : (uint8_t)gtars::TXSEQ_NOT_FOUND;
                if (status) status[i] = st;
                if (digests) memset(digests + i * 32, 0, 32);
                if (st != gtars::TXSEQ_OK) return;
                const uint8_t *seq = t.len[tx] ? b->h_seq[t.chrom[tx]] : nullptr;
                if (digests) gtars::tx_digest(t, tx, seq, digests + i * 32);
                if (seq_offsets) gtars::tx_sequence(t, tx, seq, seqs[i]);
            });
            for (const std::string &s : seqs) {
                bytes.insert(bytes.end(), s.begin(), s.end());
                off.push_back(bytes.size());
            }
        } else if (n) {
            gtars::Assembly *image;
            gtars::TxDevice *dev;
            if (const gtars_status e = device_tables(b, &image, &dev)) return e;
            gtars::TxSeqCall call;
            call.idx = idx, call.n = n, call.status = status, call.digest = digests, call.h_tables = &t, call.h_seq = b->h_seq.data(), call.threads = nt;
            if (seq_offsets) call.seq_off = &off, call.seq_bytes = &bytes;
            if (const gtars_status e = gtars::tx_seq_run(*image, *dev, call)) return e;
        }
        if (seq_offsets) {
            off.resize((size_t)n + 1, off.back());
            *seq_offsets = malloc_copy(off.data(), off.size());
            *seq_bytes = malloc_copy(bytes.data(), bytes.size());
            if (!*seq_offsets || !*seq_bytes) {
                free(*seq_offsets), free(*seq_bytes);
                *seq_offsets = nullptr, *seq_bytes = nullptr;
                return fail(GTARS_ERR_INTERNAL, "out of host memory");
            }
        }
        return GTARS_OK;
    });
}

gtars_status gtars_tx_digests_device(gtars_txbind_t *b, const uint32_t *d_idx, uint64_t n, uint8_t *d_status, char *d_digests, void *stream) {
    return guarded([&]() -> gtars_status {
        if (!b) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (!n) return GTARS_OK;
        gtars::Assembly *image;
        gtars::TxDevice *dev;
        if (const gtars_status e = device_tables(b, &image, &dev)) return e;
        const gtars::TxTables t = b->tables.view();
        gtars::TxSeqCall call;
        call.idx = d_idx, call.n = n, call.status = d_status, call.digest = d_digests, call.on_device = true, call.stream = stream;
        call.h_tables = &t, call.h_seq = b->h_seq.data(), call.threads = threads_of(0);
        return gtars::tx_seq_run(*image, *dev, call);
    });
}

}  // extern "C"
