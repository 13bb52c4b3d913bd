// vrs.cpp -- the host layer of K18 (VRS allele identifiers, gtars-vrs): the scalar calls of gtars.vrs (host code, no
// device), the refget digests of an assembly, the VCF reader (vcf.rs:56-73, vcf_core.rs:65-87) and the column / file calls
// on top of vrs.hip.  Declared in include/gtars_amd_host.h.  The rules themselves are vrs_core.h.
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/gtars_amd_host.h"
#include "assembly.h"
#include "guard.h"
#include "host_threads.h"
#include "vrs.h"
#include "vrs_core.h"

namespace gtars {
bool read_file_by_magic(const std::string &path, std::string &out, std::string &err);
unsigned host_threads_for(unsigned cap);
}  // namespace gtars
using gtars::fail;
using gtars::guarded;

struct gtars_vrs_results {
    std::vector<uint32_t> chrom;  // chromosome id of the assembly
    std::vector<uint64_t> pos;    // 0-based
    std::string pool;             // REF and ALT bytes; the ALTs of one line share its REF
    std::vector<uint32_t> ref_off, ref_len, alt_off, alt_len;
    std::vector<char> digest;     // 32 per allele; empty: parsed only
};

namespace {

unsigned threads_of(uint32_t threads) {
    const unsigned most = gtars::host_threads_for(0xFFFFFFFFu);
    return threads ? std::min<unsigned>(threads, most) : most;
}

const uint8_t *chrom_bytes(const gtars_assembly *a, size_t c) { return (const uint8_t *)a->blob.data() + a->off[c]; }

// sha512t24u of every chromosome's upper-cased bytes, one chromosome per host task, kept on the handle
gtars_status refget_digests(gtars_assembly *a, unsigned threads, const char **out) {
    std::lock_guard<std::mutex> lk(a->digest_mu);
    if (!a->refget_done) {
        const size_t nc = a->names.size();
        a->refget.assign(nc * 33, '\0');
        gtars::parallel_for(nc, threads, 1, [&](size_t c) {
            struct Upper {
                const uint8_t *p;
                uint8_t next() { return gtars::vrs_upper(*p++); }
            } src{chrom_bytes(a, c)};
            gtars::Sha512 s;
            gtars::sha512_stream(s, src, a->len[c]);
            gtars::sha512t24u_text(s, &a->refget[c * 33]);
        });
        a->refget_done = true;
    }
    *out = a->refget.data();
    return GTARS_OK;
}

// the accession table of a call as 32 characters per chromosome (a zero row: none): the caller's, or the assembly's own
gtars_status accession_table(gtars_assembly *a, const char *given, unsigned threads, std::vector<char> &tab) {
    const size_t nc = a->names.size();
    tab.assign(nc * 32 + 1, '\0');
    if (given) {
        memcpy(tab.data(), given, nc * 32);
        return GTARS_OK;
    }
    const char *own;
    if (const gtars_status e = refget_digests(a, threads, &own)) return e;
    for (size_t c = 0; c < nc; ++c) memcpy(&tab[c * 32], own + c * 33, 32);
    return GTARS_OK;
}

gtars_status check_lengths(const gtars_assembly *a) {
    for (size_t c = 0; c < a->names.size(); ++c)
        if (a->len[c] > 0xFFFFFFF0ull) return fail(GTARS_ERR_INVALID_ARG, "vrs: chromosome " + a->names[c] + " is longer than 2^32 - 16 bases");
    return GTARS_OK;
}

struct Columns {
    const uint32_t *chrom;
    const uint64_t *start;
    const uint8_t *pool;
    uint64_t pool_bytes;
    const uint32_t *ref_off, *ref_len, *alt_off, *alt_len;
    uint64_t n;
};

// the library's own host path: what the device computes, allele by allele on the host threads
void alleles_on_host(const gtars_assembly *a, const char *acc, const Columns &k, unsigned threads, uint8_t *status, uint64_t *new_start,
                     uint64_t *new_end, char *digest, std::vector<std::string> *seqs) {
    const size_t nc = a->names.size();
    if (seqs) seqs->assign((size_t)k.n, std::string());
    gtars::parallel_for((size_t)k.n, threads, 256, [&](size_t i) {
        gtars::VrsNorm r;
        const uint32_t c = k.chrom[i];
        if (c >= nc || (acc && acc[(size_t)c * 32] == 0)) r.status = gtars::VRS_NO_CHROM;
        else if ((uint64_t)k.ref_off[i] + k.ref_len[i] > k.pool_bytes || (uint64_t)k.alt_off[i] + k.alt_len[i] > k.pool_bytes)
            r.status = gtars::VRS_BAD_ALLELE;
        else
            r = gtars::vrs_normalize(chrom_bytes(a, c), a->len[c], k.start[i], k.pool + k.ref_off[i], k.ref_len[i], k.pool + k.alt_off[i],
                                     k.alt_len[i]);
        const bool ok = r.status == gtars::VRS_OK;
        if (status) status[i] = r.status;
        if (new_start) new_start[i] = ok ? r.start : 0;
        if (new_end) new_end[i] = ok ? r.end : 0;
        if (digest) {
            char *d = digest + i * 32;
            memset(d, 0, 32);
            if (ok) {
                char accession[35] = {'S', 'Q', '.'}, loc[32];
                memcpy(accession + 3, acc + (size_t)c * 32, 32);
                gtars::vrs_location_digest(accession, 35, r.start, r.end, loc);
                const uint8_t *seq = chrom_bytes(a, c);
                gtars::vrs_allele_digest(loc, seq + r.start, r.lroll, k.pool + k.alt_off[i] + r.alt_skip, r.alt_len, seq + (r.end - r.rroll),
                                         r.rroll, d);
            }
        }
        if (seqs && ok) (*seqs)[i] = gtars::vrs_norm_sequence(r, chrom_bytes(a, c), k.pool + k.alt_off[i]);
    });
}

template <class T>
T *malloc_copy(const T *src, size_t n) {
    T *p = (T *)malloc((n ? n : 1) * sizeof(T));
    if (p && n) memcpy(p, src, n * sizeof(T));
    return p;
}

// the alleles of a VCF text in file order.  Parsing is threaded over chunks cut at line starts; a chunk collects its own
// columns and pool, the chunks are joined in order.
struct Chunk {
    std::vector<uint32_t> chrom, ref_off, ref_len, alt_off, alt_len;
    std::vector<uint64_t> pos;
    std::string pool;
};

void parse_chunk(const gtars_assembly *a, const char *acc, const char *text, size_t begin, size_t end, Chunk &out) {
    std::string last_name;
    int64_t last_id = -1;
    bool have_last = false;
    size_t at = begin;
    while (at < end) {
        const char *nl = (const char *)memchr(text + at, '\n', end - at);
        const size_t stop = nl ? (size_t)(nl - text) + 1 : end;
        gtars::VcfRecord rec;
        if (gtars::vcf_parse_line(text + at, stop - at, rec)) {
            if (!have_last || last_name.size() != rec.n_chrom || memcmp(last_name.data(), rec.chrom, rec.n_chrom) != 0) {
                last_name.assign(rec.chrom, rec.n_chrom);
                have_last = true;
                auto it = a->id.find(last_name);
                last_id = it == a->id.end() ? -1 : (int64_t)it->second;
                if (last_id >= 0 && acc && acc[(size_t)last_id * 32] == 0) last_id = -1;  // no accession: skipped like an unknown name
            }
            if (last_id >= 0) {
                bool ref_stored = false;
                uint32_t ref_off = 0;
                gtars::vcf_for_real_alts(rec.alts, rec.n_alts, [&](const char *alt, size_t n_alt) {
                    if (!ref_stored) {
                        ref_off = (uint32_t)out.pool.size();
                        out.pool.append(rec.ref, rec.n_ref);
                        ref_stored = true;
                    }
                    out.chrom.push_back((uint32_t)last_id);
                    out.pos.push_back(rec.pos);
                    out.ref_off.push_back(ref_off);
                    out.ref_len.push_back((uint32_t)rec.n_ref);
                    out.alt_off.push_back((uint32_t)out.pool.size());
                    out.alt_len.push_back((uint32_t)n_alt);
                    out.pool.append(alt, n_alt);
                });
            }
        }
        at = stop;
    }
}

gtars_status read_vcf(const gtars_assembly *a, const char *acc, const char *path, unsigned threads, gtars_vrs_results &r) {
    std::string text, err;
    if (!gtars::read_file_by_magic(path, text, err)) return fail(GTARS_ERR_IO, err);
    const unsigned parts = (unsigned)std::max<size_t>(1, std::min<size_t>((size_t)threads * 4, text.size() >> 16));
    const std::vector<size_t> cut = gtars::cut_at_lines(text.data(), text.size(), parts);
    std::vector<Chunk> chunks(parts);
    gtars::parallel_for(parts, threads, 1, [&](size_t p) { parse_chunk(a, acc, text.data(), cut[p], cut[p + 1], chunks[p]); });
    size_t n = 0, bytes = 0;
    for (const Chunk &c : chunks) n += c.chrom.size(), bytes += c.pool.size();
    if (bytes > 0xFFFFFFF0ull) return fail(GTARS_ERR_CAPACITY, "VCF: the alleles of one call must fit 4 GiB; split the file");
    r.chrom.reserve(n), r.pos.reserve(n), r.ref_off.reserve(n), r.ref_len.reserve(n), r.alt_off.reserve(n), r.alt_len.reserve(n);
    r.pool.reserve(bytes);
    for (const Chunk &c : chunks) {
        const uint32_t base = (uint32_t)r.pool.size();
        r.pool += c.pool;
        r.chrom.insert(r.chrom.end(), c.chrom.begin(), c.chrom.end());
        r.pos.insert(r.pos.end(), c.pos.begin(), c.pos.end());
        r.ref_len.insert(r.ref_len.end(), c.ref_len.begin(), c.ref_len.end());
        r.alt_len.insert(r.alt_len.end(), c.alt_len.begin(), c.alt_len.end());
        for (uint32_t o : c.ref_off) r.ref_off.push_back(base + o);
        for (uint32_t o : c.alt_off) r.alt_off.push_back(base + o);
    }
    return GTARS_OK;
}

Columns columns_of(const gtars_vrs_results &r) {
    return Columns{r.chrom.data(), r.pos.data(), (const uint8_t *)r.pool.data(), r.pool.size(), r.ref_off.data(), r.ref_len.data(),
                   r.alt_off.data(), r.alt_len.data(), r.chrom.size()};
}

gtars::VrsCall call_of(const Columns &k) {
    gtars::VrsCall call;
    call.chrom = k.chrom, call.start = k.start, call.pool = k.pool, call.pool_bytes = k.pool_bytes;
    call.ref_off = k.ref_off, call.ref_len = k.ref_len, call.alt_off = k.alt_off, call.alt_len = k.alt_len, call.n = k.n;
    return call;
}

void text33(const char digest[32], char *out33) {
    memcpy(out33, digest, 32);
    out33[32] = '\0';
}

}  // namespace

namespace gtars {
void vrs_run_on_host(const gtars_assembly *a, const VrsCall &call) {
    const Columns k{call.chrom, call.start, call.pool, call.pool_bytes, call.ref_off, call.ref_len, call.alt_off, call.alt_len, call.n};
    alleles_on_host(a, call.accessions, k, call.threads, call.status, call.new_start, call.new_end, call.digest, nullptr);
}
gtars_status vrs_accession_table(gtars_assembly *a, const char *given, unsigned threads, std::vector<char> &tab) {
    return accession_table(a, given, threads, tab);
}
gtars_status vrs_check_lengths(const gtars_assembly *a) { return check_lengths(a); }
}  // namespace gtars

extern "C" {

gtars_status gtars_sha512t24u(const void *data, uint64_t n, char *out33) {
    return guarded([&]() -> gtars_status {
        if ((!data && n) || !out33) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        char d[32];
        gtars::sha512t24u((const uint8_t *)data, (size_t)n, d);
        text33(d, out33);
        return GTARS_OK;
    });
}

gtars_status gtars_vrs_location_digest(const char *accession, uint64_t start, uint64_t end, char *out33) {
    return guarded([&]() -> gtars_status {
        if (!accession || !out33) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        char d[32];
        gtars::vrs_location_digest(accession, strlen(accession), start, end, d);
        text33(d, out33);
        return GTARS_OK;
    });
}

gtars_status gtars_vrs_allele_digest(const char *accession, uint64_t start, uint64_t end, const char *sequence, uint64_t sequence_len,
                                     char *out33) {
    return guarded([&]() -> gtars_status {
        if (!accession || (!sequence && sequence_len) || !out33) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        char loc[32], d[32];
        gtars::vrs_location_digest(accession, strlen(accession), start, end, loc);
        gtars::vrs_allele_digest(loc, nullptr, 0, (const uint8_t *)sequence, sequence_len, nullptr, 0, d);
        text33(d, out33);
        return GTARS_OK;
    });
}

gtars_status gtars_vrs_normalize(const uint8_t *sequence, uint64_t sequence_len, uint64_t start, const uint8_t *ref, uint64_t ref_len,
                                 const uint8_t *alt, uint64_t alt_len, uint64_t *new_start, uint64_t *new_end, uint8_t **allele,
                                 uint64_t *allele_len) {
    return guarded([&]() -> gtars_status {
        if ((!sequence && sequence_len) || (!ref && ref_len) || (!alt && alt_len) || !new_start || !new_end || !allele || !allele_len)
            return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *allele = nullptr, *allele_len = 0;
        const gtars::VrsNorm r = gtars::vrs_normalize(sequence, sequence_len, start, ref, ref_len, alt, alt_len);
        if (r.status) return fail(GTARS_ERR_INVALID_ARG, gtars::vrs_error_text(r.status, sequence, sequence_len, start, ref, ref_len));
        const std::string s = gtars::vrs_norm_sequence(r, sequence, alt);
        *allele = malloc_copy((const uint8_t *)s.data(), s.size());
        if (!*allele) return fail(GTARS_ERR_INTERNAL, "out of host memory");
        *new_start = r.start, *new_end = r.end, *allele_len = s.size();
        return GTARS_OK;
    });
}

gtars_status gtars_assembly_refget_digests(gtars_assembly_t *a, uint32_t threads, const char **out) {
    return guarded([&]() -> gtars_status {
        if (!a || !out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        return refget_digests(a, threads_of(threads), out);
    });
}

gtars_status gtars_vrs_alleles(gtars_assembly_t *a, const char *accessions, const uint32_t *chrom, const uint64_t *start,
                               const uint8_t *pool, uint64_t pool_bytes, const uint32_t *ref_off, const uint32_t *ref_len,
                               const uint32_t *alt_off, const uint32_t *alt_len, uint64_t n, int on_host, uint32_t threads,
                               uint8_t *status, uint64_t *new_start, uint64_t *new_end, char *digests, uint64_t **seq_offsets,
                               uint8_t **seq_bytes) {
    return guarded([&]() -> gtars_status {
        if (!a || (seq_offsets == nullptr) != (seq_bytes == nullptr)) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (n && (!chrom || !start || !ref_off || !ref_len || !alt_off || !alt_len || (!pool && pool_bytes)))
            return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (seq_offsets) *seq_offsets = nullptr, *seq_bytes = nullptr;
        if (const gtars_status e = check_lengths(a)) return e;
        const unsigned nt = threads_of(threads);
        std::vector<char> tab;
        if (digests || accessions)
            if (const gtars_status e = accession_table(a, accessions, nt, tab)) return e;
        const char *acc = tab.empty() ? nullptr : tab.data();
        const Columns k{chrom, start, pool, pool_bytes, ref_off, ref_len, alt_off, alt_len, n};
        std::vector<uint64_t> off(1, 0);
        std::vector<uint8_t> bytes;
        if (on_host) {
            std::vector<std::string> seqs;
            alleles_on_host(a, acc, k, nt, status, new_start, new_end, digests, seq_offsets ? &seqs : nullptr);
            for (const std::string &s : seqs) {
                bytes.insert(bytes.end(), s.begin(), s.end());
                off.push_back(bytes.size());
            }
        } else if (n) {
            gtars::Assembly *dev;
            if (const gtars_status e = gtars::assembly_device_image(a, &dev)) return e;
            std::vector<const uint8_t *> h_seq(a->names.size());
            for (size_t c = 0; c < h_seq.size(); ++c) h_seq[c] = chrom_bytes(a, c);
            gtars::VrsCall call = call_of(k);
            call.accessions = acc, call.h_seq = h_seq.data(), call.threads = nt;
            call.status = status, call.new_start = new_start, call.new_end = new_end, call.digest = digests;
            if (seq_offsets) call.seq_off = &off, call.seq_bytes = &bytes;
            if (const gtars_status e = gtars::vrs_run(*dev, call)) return e;
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

gtars_status gtars_vrs_ids_device(gtars_assembly_t *a, const char *accessions, const uint32_t *d_chrom, const uint64_t *d_start,
                                  const uint8_t *d_pool, uint64_t pool_bytes, const uint32_t *d_ref_off, const uint32_t *d_ref_len,
                                  const uint32_t *d_alt_off, const uint32_t *d_alt_len, uint64_t n, uint8_t *d_status,
                                  uint64_t *d_new_start, uint64_t *d_new_end, char *d_digests, void *stream) {
    return guarded([&]() -> gtars_status {
        if (!a) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (const gtars_status e = check_lengths(a)) return e;
        if (!n) return GTARS_OK;
        const unsigned nt = threads_of(0);
        std::vector<char> tab;
        if (d_digests || accessions)
            if (const gtars_status e = accession_table(a, accessions, nt, tab)) return e;
        gtars::Assembly *dev;
        if (const gtars_status e = gtars::assembly_device_image(a, &dev)) return e;
        std::vector<const uint8_t *> h_seq(a->names.size());
        for (size_t c = 0; c < h_seq.size(); ++c) h_seq[c] = chrom_bytes(a, c);
        gtars::VrsCall call = call_of(Columns{d_chrom, d_start, d_pool, pool_bytes, d_ref_off, d_ref_len, d_alt_off, d_alt_len, n});
        call.on_device = true, call.stream = stream;
        call.accessions = tab.empty() ? nullptr : tab.data(), call.h_seq = h_seq.data(), call.threads = nt;
        call.status = d_status, call.new_start = d_new_start, call.new_end = d_new_end, call.digest = d_digests;
        return gtars::vrs_run(*dev, call);
    });
}

gtars_status gtars_vcf_read_alleles(gtars_assembly_t *a, const char *path, const char *accessions, uint32_t threads,
                                    gtars_vrs_results_t **out) {
    return guarded([&]() -> gtars_status {
        if (!a || !path || !out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        auto r = std::make_unique<gtars_vrs_results>();
        if (const gtars_status e = read_vcf(a, accessions, path, threads_of(threads), *r)) return e;
        *out = r.release();
        return GTARS_OK;
    });
}

gtars_status gtars_vrs_from_vcf(gtars_assembly_t *a, const char *path, const char *accessions, int on_host, uint32_t threads,
                                gtars_vrs_results_t **out) {
    return guarded([&]() -> gtars_status {
        if (!a || !path || !out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        if (const gtars_status e = check_lengths(a)) return e;
        const unsigned nt = threads_of(threads);
        std::vector<char> tab;
        if (const gtars_status e = accession_table(a, accessions, nt, tab)) return e;
        auto r = std::make_unique<gtars_vrs_results>();
        if (const gtars_status e = read_vcf(a, tab.data(), path, nt, *r)) return e;
        const Columns k = columns_of(*r);
        std::vector<uint8_t> status((size_t)k.n);
        r->digest.assign((size_t)k.n * 32, '\0');
        if (on_host) {
            alleles_on_host(a, tab.data(), k, nt, status.data(), nullptr, nullptr, r->digest.data(), nullptr);
        } else if (k.n) {
            gtars::Assembly *dev;
            if (const gtars_status e = gtars::assembly_device_image(a, &dev)) return e;
            std::vector<const uint8_t *> h_seq(a->names.size());
            for (size_t c = 0; c < h_seq.size(); ++c) h_seq[c] = chrom_bytes(a, c);
            gtars::VrsCall call = call_of(k);
            call.accessions = tab.data(), call.h_seq = h_seq.data(), call.threads = nt;
            call.status = status.data(), call.digest = r->digest.data();
            if (const gtars_status e = gtars::vrs_run(*dev, call)) return e;
        }
        // the reference stops at the first allele that fails to normalize (vcf_core.rs:162-163): the cause is derived again
        // here, on the host, from the row itself
        for (size_t i = 0; i < k.n; ++i)
            if (status[i]) {
                const uint32_t c = k.chrom[i];
                return fail(GTARS_ERR_INVALID_ARG, "Failed to normalize variant at " + a->names[c] + ":" + std::to_string(k.start[i] + 1) + ": " +
                                                       gtars::vrs_error_text(status[i], chrom_bytes(a, c), a->len[c], k.start[i],
                                                                             k.pool + k.ref_off[i], k.ref_len[i]));
            }
        *out = r.release();
        return GTARS_OK;
    });
}

void gtars_vrs_results_free(gtars_vrs_results_t *r) { delete r; }
uint64_t gtars_vrs_results_len(const gtars_vrs_results_t *r) { return r ? r->chrom.size() : 0; }

gtars_status gtars_vrs_results_columns(const gtars_vrs_results_t *r, const uint32_t **chrom, const uint64_t **pos, const uint8_t **pool,
                                       uint64_t *pool_bytes, const uint32_t **ref_off, const uint32_t **ref_len, const uint32_t **alt_off,
                                       const uint32_t **alt_len, const char **digests) {
    return guarded([&]() -> gtars_status {
        if (!r || !chrom || !pos || !pool || !pool_bytes || !ref_off || !ref_len || !alt_off || !alt_len || !digests)
            return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *chrom = r->chrom.data(), *pos = r->pos.data(), *pool = (const uint8_t *)r->pool.data(), *pool_bytes = r->pool.size();
        *ref_off = r->ref_off.data(), *ref_len = r->ref_len.data(), *alt_off = r->alt_off.data(), *alt_len = r->alt_len.data();
        *digests = r->digest.empty() ? nullptr : r->digest.data();
        return GTARS_OK;
    });
}

}  // extern "C"
