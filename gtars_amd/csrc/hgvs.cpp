// hgvs.cpp -- the host layer of K20 (gtars.vrs.hgvs; gtars-vrs/src/hgvs/{parser,bridge}.rs, gtars-python/src/vrs/hgvs.rs): the
// scalar parse, the batch parse and accession lookup on the host threads, the library's host path of the bridge and the
// batch calls on top of hgvs.hip; and the same for K23, the transcript-anchored bridge (hgvs_tx.hip, bridge.rs:226-534).
// Declared in include/gtars_amd_host.h.  The rules themselves are hgvs_core.h and hgvs_tx_core.h.
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/gtars_amd_host.h"
#include "assembly.h"
#include "guard.h"
#include "hgvs.h"
#include "hgvs_core.h"
#include "hgvs_tx_core.h"
#include "host_threads.h"
#include "vrs.h"
#include "vrs_core.h"

namespace gtars {
unsigned host_threads_for(unsigned cap);
}  // namespace gtars
using gtars::fail;
using gtars::guarded;

static_assert(sizeof(gtars_hgvs_row) == sizeof(gtars::HgvsRow) && sizeof(gtars_hgvs_position) == sizeof(gtars::HgvsPosition),
              "the row of the C ABI is the parser's");

namespace {

unsigned threads_of(uint32_t threads) {
    const unsigned most = gtars::host_threads_for(0xFFFFFFFFu);
    return threads ? std::min<unsigned>(threads, most) : most;
}

gtars::HgvsCols view_of(const gtars_hgvs_columns &c) {
    gtars::HgvsCols v;
    v.pre = c.pre, v.kind = c.kind, v.loc = c.loc, v.edit = c.edit, v.flags = c.flags, v.tx = c.tx;
    v.base1 = c.base1, v.off1 = c.off1, v.base2 = c.base2, v.off2 = c.off2, v.text_off = c.text_off;
    v.ref_off = c.ref_off, v.ref_len = c.ref_len, v.alt_off = c.alt_off, v.alt_len = c.alt_len;
    v.text = c.text, v.text_bytes = c.text_bytes, v.n = c.n;
    return v;
}

bool columns_complete(const gtars_hgvs_columns &c) {
    return c.pre && c.kind && c.loc && c.edit && c.flags && c.tx && c.base1 && c.off1 && c.base2 && c.off2 && c.text_off && c.ref_off &&
           c.ref_len && c.alt_off && c.alt_len;
}

// the caller's aliases of chromosome names
using Aliases = std::unordered_map<std::string, uint32_t>;
gtars_status aliases_of(const uint8_t *pool, const uint64_t *offsets, const uint32_t *chrom, uint64_t n, Aliases &out) {
    if (n && (!offsets || !chrom || (!pool && offsets[n]))) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    for (uint64_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return fail(GTARS_ERR_INVALID_ARG, "hgvs: alias offsets must ascend");
        out.emplace(std::string((const char *)pool + offsets[i], (size_t)(offsets[i + 1] - offsets[i])), chrom[i]);
    }
    return GTARS_OK;
}

// parse() and resolve_chrom_for_variant's lookups (bridge.rs:625-667) for expression i, into row i of the columns
void resolve_row(const gtars::TxBindParts &p, const Aliases &aliases, const char *s, size_t len, uint64_t text_off, const gtars_hgvs_columns &c,
                 size_t i) {
    gtars::HgvsRow row;
    uint8_t st = gtars::hgvs_parse(s, len, &row);
    uint32_t tx = gtars::TX_NONE;
    if (st == gtars::HGVS_OK) {
        const char *acc = s + row.acc_off;
        size_t n_acc = row.acc_len;
        int64_t idx = -1;
        const bool gene = gtars::hgvs_looks_like_gene_symbol(acc, n_acc);
        if (gene) {
            idx = p.store->lookup_mane(std::string(acc, n_acc));
            if (idx < 0) st = gtars::HGVS_NO_MANE_TRANSCRIPT;
            else acc = p.store->recs[(size_t)idx].accession.data(), n_acc = p.store->recs[(size_t)idx].accession.size();
        }
        if (st == gtars::HGVS_OK) {
            if (row.ref_type == gtars::HGVS_REF_G) {
                const std::string name(acc, n_acc);
                const auto it = p.assembly->id.find(name);
                if (it != p.assembly->id.end()) tx = it->second;
                else if (const auto al = aliases.find(name); al != aliases.end()) tx = al->second;
            } else if (row.ref_type == gtars::HGVS_REF_C || row.ref_type == gtars::HGVS_REF_N) {
                if (!gene) idx = p.store->lookup(acc, n_acc);
                if (idx < 0) st = gtars::HGVS_TRANSCRIPT_NOT_FOUND;
                else tx = (uint32_t)idx;
            }
        }
    }
    c.pre[i] = st, c.kind[i] = row.ref_type, c.loc[i] = row.loc, c.edit[i] = row.edit;
    c.flags[i] = (uint8_t)((row.flags & (gtars::HGVS_HAS_REF | gtars::HGVS_UNCERTAIN)) |
                           (row.pos[0].datum == gtars::HGVS_DATUM_CDS_END ? gtars::HGVS_STAR1 : 0) |
                           (row.pos[2].datum == gtars::HGVS_DATUM_CDS_END ? gtars::HGVS_STAR2 : 0));
    c.tx[i] = tx;
    c.base1[i] = row.pos[0].base, c.off1[i] = row.pos[0].offset, c.base2[i] = row.pos[2].base, c.off2[i] = row.pos[2].offset;
    c.text_off[i] = text_off;
    c.ref_off[i] = row.ref_off, c.ref_len[i] = row.ref_len, c.alt_off[i] = row.alt_off, c.alt_len[i] = row.alt_len;
}

gtars_status resolve(gtars_txbind_t *b, const uint8_t *text, const uint64_t *offsets, uint64_t n, const Aliases &aliases, unsigned threads,
                     gtars_hgvs_columns &c) {
    for (uint64_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) return fail(GTARS_ERR_INVALID_ARG, "hgvs: text offsets must ascend");
    const gtars::TxBindParts p = gtars::tx_bind_parts(b);
    c.text = text, c.text_bytes = n ? offsets[n] : 0, c.n = n;
    gtars::parallel_for((size_t)n, threads, 2048, [&](size_t i) {
        resolve_row(p, aliases, (const char *)text + offsets[i], (size_t)(offsets[i + 1] - offsets[i]), offsets[i], c, i);
    });
    return GTARS_OK;
}

struct Outputs {
    uint8_t *status, *detail, *warnings;
    uint32_t *chrom;
    uint64_t *start, *end;
    char *digest;
};

// the library's host path of hgvs_run: the same functions of hgvs_core.h row by row, then K18's host path
gtars_status run_on_host(const gtars::TxBindParts &p, const gtars::HgvsCols &c, const char *acc, unsigned threads, const Outputs &o) {
    const size_t n = (size_t)c.n;
    const gtars::TxTables t = p.tables->view();
    gtars::HgvsGenome g;
    g.chroms = p.h_seq, g.len = p.assembly->len.data(), g.n_chrom = (uint32_t)p.assembly->names.size();
    std::vector<gtars::HgvsSpan> spans(n);
    gtars::parallel_for(n, threads, 1024, [&](size_t i) { spans[i] = gtars::hgvs_span_one(t, g, c, i); });
    std::vector<uint64_t> off(n + 1, 0);
    for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + (spans[i].status == gtars::HGVS_OK ? spans[i].ref_len + spans[i].alt_len : 0);
    if (off[n] > 0xFFFFFFF0ull) return fail(GTARS_ERR_CAPACITY, "hgvs: the alleles of one call must fit 4 GiB; split the batch");
    std::vector<uint8_t> pool((size_t)off[n]), status(n), vrs_status(n);
    std::vector<uint32_t> chrom(n), ref_off(n), ref_len(n), alt_off(n), alt_len(n);
    std::vector<uint64_t> start(n), ns(n), ne(n);
    gtars::parallel_for(n, threads, 256, [&](size_t i) {
        const gtars::HgvsSpan &s = spans[i];
        const bool ok = s.status == gtars::HGVS_OK;
        status[i] = s.status;
        chrom[i] = ok ? s.chrom : gtars::TX_NONE, start[i] = ok ? s.start : 0;
        ref_len[i] = ok ? (uint32_t)s.ref_len : 0, alt_len[i] = ok ? (uint32_t)s.alt_len : 0;
        ref_off[i] = (uint32_t)off[i], alt_off[i] = (uint32_t)(off[i] + ref_len[i]);
        if (!ok) return;
        const uint8_t *seq = g.seq_of(s.chrom), *alt = c.text + c.text_off[i] + c.alt_off[i];
        uint8_t *dst = pool.data() + off[i];
        for (uint64_t k = 0; k < s.ref_len + s.alt_len; ++k) dst[k] = (uint8_t)gtars::hgvs_pool_byte(seq, s.start, s.ref_len, s.alt_len, s.mode, alt, k);
    });
    gtars::VrsCall v;
    v.chrom = chrom.data(), v.start = start.data(), v.pool = pool.data(), v.pool_bytes = pool.size();
    v.ref_off = ref_off.data(), v.ref_len = ref_len.data(), v.alt_off = alt_off.data(), v.alt_len = alt_len.data(), v.n = n;
    v.accessions = acc, v.threads = threads;
    v.status = vrs_status.data(), v.new_start = ns.data(), v.new_end = ne.data(), v.digest = o.digest;
    gtars::vrs_run_on_host(p.assembly, v);
    for (size_t i = 0; i < n; ++i) {
        uint8_t st = status[i], detail = spans[i].detail;
        if (st == gtars::HGVS_OK && vrs_status[i] != gtars::VRS_OK) st = gtars::HGVS_NORMALIZE_ERROR, detail = vrs_status[i];
        if (o.status) o.status[i] = st;
        if (o.detail) o.detail[i] = detail;
        if (o.warnings) o.warnings[i] = (c.flags[i] & gtars::HGVS_UNCERTAIN) ? (uint8_t)gtars::HGVS_WARN_UNCERTAIN : (uint8_t)0;
        if (o.chrom) o.chrom[i] = chrom[i];
        if (o.start) o.start[i] = ns[i];
        if (o.end) o.end[i] = ne[i];
    }
    return GTARS_OK;
}

// the device path of one batch: host columns (on_device false) or resident ones
gtars_status run_on_device(gtars_txbind_t *b, const gtars::TxBindParts &p, const gtars::HgvsCols &c, const char *acc, unsigned threads,
                           bool on_device, void *stream, const Outputs &o) {
    gtars::Assembly *image;
    gtars::TxDevice *dev;
    if (const gtars_status e = gtars::tx_bind_device(b, &image, &dev)) return e;
    gtars::HgvsCall call;
    call.cols = c, call.on_device = on_device, call.stream = stream;
    call.accessions = acc, call.h_seq = p.h_seq, call.threads = threads;
    call.status = o.status, call.detail = o.detail, call.warnings = o.warnings, call.chrom = o.chrom;
    call.start = o.start, call.end = o.end, call.digest = o.digest;
    return gtars::hgvs_run(*image, *dev, call);
}

// ---- K23: the transcript-anchored bridge ------------------------------------------------------------------------------
struct TxOutputs {
    uint8_t *status, *detail, *warnings;
    uint32_t *tx;
    uint64_t *start, *end;
    char *digest, *anchor;
};

constexpr size_t TX_HOST_BLOCK = 256;           // rows a host thread takes at a time
constexpr uint64_t TX_MAX_POOL = 0xFFFFFFF0ull;  // as on the device

// a thread's open transcript: its mature mRNA and "SQ." + its digest, derived once per run of equal transcript ids
struct OpenTranscript {
    uint32_t tx = gtars::TX_NONE;
    std::string mrna;
    char acc[35] = {'S', 'Q', '.'};
    void open(const gtars::TxTables &t, const uint8_t *const *h_seq, uint32_t want) {
        if (want == tx) return;
        gtars::tx_sequence(t, want, t.len[want] ? h_seq[t.chrom[want]] : nullptr, mrna);
        gtars::sha512t24u((const uint8_t *)mrna.data(), mrna.size(), acc + 3);
        tx = want;
    }
    const uint8_t *bytes() const { return (const uint8_t *)mrna.data(); }
};

// normalize_ref over the open mRNA and the two digests (finalize_transcript_vrs_id); the status of vrs_core.h
uint8_t finish_on_host(const OpenTranscript &m, uint64_t start, const uint8_t *ref, uint64_t ref_len, const uint8_t *alt, uint64_t alt_len,
                       uint64_t *ns, uint64_t *ne, char *digest) {
    const gtars::VrsNorm r = gtars::vrs_normalize(m.bytes(), m.mrna.size(), start, ref, ref_len, alt, alt_len);
    if (r.status != gtars::VRS_OK) return r.status;
    *ns = r.start, *ne = r.end;
    if (digest) {
        char loc[32];
        gtars::vrs_location_digest(m.acc, 35, r.start, r.end, loc);
        gtars::vrs_allele_digest(loc, m.bytes() + r.start, r.lroll, alt + r.alt_skip, r.alt_len, m.bytes() + (r.end - r.rroll), r.rroll, digest);
    }
    return gtars::VRS_OK;
}

// the library's host path of hgvs_tx_run: hgvs_tx_span_one row by row, then vrs_normalize and the digest writers over the
// transcript's mRNA
gtars_status run_tx_on_host(const gtars::TxBindParts &p, const gtars::HgvsCols &c, unsigned threads, const TxOutputs &o) {
    const size_t n = (size_t)c.n;
    const gtars::TxTables t = p.tables->view();
    gtars::HgvsGenome g;
    g.chroms = p.h_seq, g.len = p.assembly->len.data(), g.n_chrom = (uint32_t)p.assembly->names.size();
    std::atomic<bool> too_long{false};
    gtars::parallel_for((n + TX_HOST_BLOCK - 1) / TX_HOST_BLOCK, threads, 1, [&](size_t blk) {
        OpenTranscript m;
        std::vector<uint8_t> pool;
        for (size_t i = blk * TX_HOST_BLOCK; i < std::min(n, (blk + 1) * TX_HOST_BLOCK); ++i) {
            const gtars::HgvsTxSpan s = gtars::hgvs_tx_span_one(t, g, c, i);
            uint8_t st = s.status, detail = s.detail;
            uint64_t ns = 0, ne = 0;
            char digest[32] = {}, anchor[32] = {};
            if (st == gtars::HGVS_OK && s.ref_len + s.alt_len > TX_MAX_POOL) too_long.store(true), st = gtars::HGVS_OUT_OF_BOUNDS;
            const uint32_t tx = st == gtars::HGVS_OK ? s.tx : gtars::TX_NONE;
            if (st == gtars::HGVS_OK) {
                m.open(t, p.h_seq, s.tx);
                pool.resize((size_t)(s.ref_len + s.alt_len));
                const uint8_t *alt = c.text + c.text_off[i] + c.alt_off[i];
                for (uint64_t k = 0; k < s.ref_len + s.alt_len; ++k)
                    pool[k] = (uint8_t)gtars::hgvs_tx_pool_byte(m.bytes(), s.start, s.ref_len, s.mode, alt, k);
                const uint8_t vs = finish_on_host(m, s.start, pool.data(), s.ref_len, pool.data() + s.ref_len, s.alt_len, &ns, &ne, digest);
                if (vs != gtars::VRS_OK) st = gtars::HGVS_NORMALIZE_ERROR, detail = vs;
                else memcpy(anchor, m.acc + 3, 32);
            }
            if (o.status) o.status[i] = st;
            if (o.detail) o.detail[i] = detail;
            if (o.warnings) o.warnings[i] = (c.flags[i] & gtars::HGVS_UNCERTAIN) ? (uint8_t)gtars::HGVS_WARN_UNCERTAIN : (uint8_t)0;
            if (o.tx) o.tx[i] = tx;
            if (o.start) o.start[i] = ns;
            if (o.end) o.end[i] = ne;
            if (o.digest) memcpy(o.digest + i * 32, digest, 32);  // (zero bytes unless the row passed)
            if (o.anchor) memcpy(o.anchor + i * 32, anchor, 32);
        }
    });
    if (too_long.load()) return fail(GTARS_ERR_CAPACITY, "hgvs: the alleles of one call must fit 4 GiB; split the batch");
    return GTARS_OK;
}

gtars_status run_tx_on_device(gtars_txbind_t *b, const gtars::TxBindParts &p, const gtars::HgvsCols &c, unsigned threads, bool on_device,
                              void *stream, const TxOutputs &o) {
    gtars::Assembly *image;
    gtars::TxDevice *dev;
    if (const gtars_status e = gtars::tx_bind_device(b, &image, &dev)) return e;
    const gtars::TxTables t = p.tables->view();
    gtars::HgvsTxCall call;
    call.cols = c, call.on_device = on_device, call.stream = stream;
    call.host.h_tables = &t, call.host.h_seq = p.h_seq, call.host.threads = threads;
    call.status = o.status, call.detail = o.detail, call.warnings = o.warnings, call.tx = o.tx;
    call.start = o.start, call.end = o.end, call.digest = o.digest, call.anchor = o.anchor;
    return gtars::hgvs_tx_run(*image, *dev, call);
}

// the host path of vrs_tx_run: K18's checks in K18's order, over the transcript's mRNA
void tx_alleles_on_host(const gtars::TxBindParts &p, const gtars::VrsTxCall &k, unsigned threads) {
    const size_t n = (size_t)k.n;
    const gtars::TxTables t = p.tables->view();
    gtars::parallel_for((n + TX_HOST_BLOCK - 1) / TX_HOST_BLOCK, threads, 1, [&](size_t blk) {
        OpenTranscript m;
        for (size_t i = blk * TX_HOST_BLOCK; i < std::min(n, (blk + 1) * TX_HOST_BLOCK); ++i) {
            const uint32_t tx = k.tx[i];
            uint8_t st = gtars::VRS_OK;
            uint64_t ns = 0, ne = 0;
            char digest[32] = {}, anchor[32] = {};
            if (tx >= t.n_tx || t.seq_status[tx] != gtars::TXSEQ_OK) st = gtars::VRS_NO_CHROM;
            else if ((uint64_t)k.ref_off[i] + k.ref_len[i] > k.pool_bytes || (uint64_t)k.alt_off[i] + k.alt_len[i] > k.pool_bytes)
                st = gtars::VRS_BAD_ALLELE;
            else {
                m.open(t, p.h_seq, tx);
                st = finish_on_host(m, k.start[i], k.pool + k.ref_off[i], k.ref_len[i], k.pool + k.alt_off[i], k.alt_len[i], &ns, &ne, digest);
                if (st == gtars::VRS_OK) memcpy(anchor, m.acc + 3, 32);
            }
            if (k.status) k.status[i] = st;
            if (k.new_start) k.new_start[i] = ns;
            if (k.new_end) k.new_end[i] = ne;
            if (k.digest) memcpy(k.digest + i * 32, digest, 32);  // (zero bytes unless the row passed)
            if (k.anchor) memcpy(k.anchor + i * 32, anchor, 32);
        }
    });
}

}  // namespace

extern "C" {

const char *gtars_hgvs_status_name(uint32_t status) { return gtars::hgvs_status_name(status); }

gtars_status gtars_hgvs_parse(const char *text, uint64_t len, gtars_hgvs_row *row, uint8_t *status, uint64_t *err_pos, char *err_text,
                              uint64_t err_cap) {
    return guarded([&]() -> gtars_status {
        if ((!text && len) || !row || !status) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        size_t at = 0;
        const char *msg = nullptr;
        *status = gtars::hgvs_parse(text, (size_t)len, (gtars::HgvsRow *)row, &at, &msg);
        if (err_pos) *err_pos = at;
        if (err_text && err_cap) {
            strncpy(err_text, msg ? msg : "", (size_t)err_cap - 1);
            err_text[err_cap - 1] = '\0';
        }
        return GTARS_OK;
    });
}

int gtars_hgvs_looks_like_gene_symbol(const char *accession) { return accession && gtars::hgvs_looks_like_gene_symbol(accession, strlen(accession)); }

gtars_status gtars_hgvs_resolve(gtars_txbind_t *b, const uint8_t *text, const uint64_t *offsets, uint64_t n, const uint8_t *alias_pool,
                                const uint64_t *alias_offsets, const uint32_t *alias_chrom, uint64_t n_alias, uint32_t threads,
                                gtars_hgvs_columns *out) {
    return guarded([&]() -> gtars_status {
        if (!b || !out || (n && (!offsets || (!text && offsets[n]) || !columns_complete(*out)))) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        Aliases aliases;
        if (const gtars_status e = aliases_of(alias_pool, alias_offsets, alias_chrom, n_alias, aliases)) return e;
        return resolve(b, text, offsets, n, aliases, threads_of(threads), *out);
    });
}

gtars_status gtars_hgvs_to_vrs(gtars_txbind_t *b, const uint8_t *text, const uint64_t *offsets, uint64_t n, const uint8_t *alias_pool,
                               const uint64_t *alias_offsets, const uint32_t *alias_chrom, uint64_t n_alias, const char *accessions,
                               int on_host, uint32_t threads, uint8_t *status, uint8_t *detail, uint8_t *warnings, uint32_t *chrom,
                               uint64_t *start, uint64_t *end, char *digests) {
    return guarded([&]() -> gtars_status {
        if (!b || (n && (!offsets || (!text && offsets[n])))) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        const gtars::TxBindParts p = gtars::tx_bind_parts(b);
        if (const gtars_status e = gtars::vrs_check_lengths(p.assembly)) return e;
        if (!n) return GTARS_OK;
        const unsigned nt = threads_of(threads);
        Aliases aliases;
        if (const gtars_status e = aliases_of(alias_pool, alias_offsets, alias_chrom, n_alias, aliases)) return e;
        std::vector<char> tab;
        if (const gtars_status e = gtars::vrs_accession_table(p.assembly, accessions, nt, tab)) return e;
        const size_t k = (size_t)n;
        std::vector<uint8_t> bytes(5 * k);
        std::vector<uint32_t> words(5 * k);
        std::vector<int64_t> longs(4 * k);
        std::vector<uint64_t> text_off(k);
        gtars_hgvs_columns c{};
        c.pre = bytes.data(), c.kind = c.pre + k, c.loc = c.kind + k, c.edit = c.loc + k, c.flags = c.edit + k;
        c.tx = words.data(), c.ref_off = c.tx + k, c.ref_len = c.ref_off + k, c.alt_off = c.ref_len + k, c.alt_len = c.alt_off + k;
        c.base1 = longs.data(), c.off1 = c.base1 + k, c.base2 = c.off1 + k, c.off2 = c.base2 + k;
        c.text_off = text_off.data();
        if (const gtars_status e = resolve(b, text, offsets, n, aliases, nt, c)) return e;
        const Outputs o{status, detail, warnings, chrom, start, end, digests};
        if (on_host) return run_on_host(p, view_of(c), tab.data(), nt, o);
        return run_on_device(b, p, view_of(c), tab.data(), nt, false, nullptr, o);
    });
}

gtars_status gtars_hgvs_ids_device(gtars_txbind_t *b, const gtars_hgvs_columns *d_cols, const char *accessions, uint8_t *d_status,
                                   uint8_t *d_detail, uint8_t *d_warnings, uint32_t *d_chrom, uint64_t *d_start, uint64_t *d_end,
                                   char *d_digests, void *stream) {
    return guarded([&]() -> gtars_status {
        if (!b || !d_cols) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        const gtars::TxBindParts p = gtars::tx_bind_parts(b);
        if (const gtars_status e = gtars::vrs_check_lengths(p.assembly)) return e;
        if (!d_cols->n) return GTARS_OK;
        if (!columns_complete(*d_cols)) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        const unsigned nt = threads_of(0);
        std::vector<char> tab;
        if (const gtars_status e = gtars::vrs_accession_table(p.assembly, accessions, nt, tab)) return e;
        return run_on_device(b, p, view_of(*d_cols), tab.data(), nt, true, stream, Outputs{d_status, d_detail, d_warnings, d_chrom, d_start, d_end, d_digests});
    });
}

gtars_status gtars_hgvs_to_transcript_vrs(gtars_txbind_t *b, const uint8_t *text, const uint64_t *offsets, uint64_t n, int on_host,
                                          uint32_t threads, uint8_t *status, uint8_t *detail, uint8_t *warnings, uint32_t *tx, uint64_t *start,
                                          uint64_t *end, char *digests, char *anchors) {
    return guarded([&]() -> gtars_status {
        if (!b || (n && (!offsets || (!text && offsets[n])))) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (!n) return GTARS_OK;
        const gtars::TxBindParts p = gtars::tx_bind_parts(b);
        const unsigned nt = threads_of(threads);
        const size_t k = (size_t)n;
        std::vector<uint8_t> bytes(5 * k);
        std::vector<uint32_t> words(5 * k);
        std::vector<int64_t> longs(4 * k);
        std::vector<uint64_t> text_off(k);
        gtars_hgvs_columns c{};
        c.pre = bytes.data(), c.kind = c.pre + k, c.loc = c.kind + k, c.edit = c.loc + k, c.flags = c.edit + k;
        c.tx = words.data(), c.ref_off = c.tx + k, c.ref_len = c.ref_off + k, c.alt_off = c.ref_len + k, c.alt_len = c.alt_off + k;
        c.base1 = longs.data(), c.off1 = c.base1 + k, c.base2 = c.off1 + k, c.off2 = c.base2 + k;
        c.text_off = text_off.data();
        if (const gtars_status e = resolve(b, text, offsets, n, Aliases(), nt, c)) return e;
        const TxOutputs o{status, detail, warnings, tx, start, end, digests, anchors};
        if (on_host) return run_tx_on_host(p, view_of(c), nt, o);
        return run_tx_on_device(b, p, view_of(c), nt, false, nullptr, o);
    });
}

gtars_status gtars_hgvs_transcript_ids_device(gtars_txbind_t *b, const gtars_hgvs_columns *d_cols, uint8_t *d_status, uint8_t *d_detail,
                                              uint8_t *d_warnings, uint32_t *d_tx, uint64_t *d_start, uint64_t *d_end, char *d_digests,
                                              char *d_anchors, void *stream) {
    return guarded([&]() -> gtars_status {
        if (!b || !d_cols) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (!d_cols->n) return GTARS_OK;
        if (!columns_complete(*d_cols)) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        return run_tx_on_device(b, gtars::tx_bind_parts(b), view_of(*d_cols), threads_of(0), true, stream,
                                TxOutputs{d_status, d_detail, d_warnings, d_tx, d_start, d_end, d_digests, d_anchors});
    });
}

gtars_status gtars_vrs_transcript_ids(gtars_txbind_t *b, const uint32_t *tx, const uint64_t *start, const uint8_t *pool, uint64_t pool_bytes,
                                      const uint32_t *ref_off, const uint32_t *ref_len, const uint32_t *alt_off, const uint32_t *alt_len,
                                      uint64_t n, int on_host, uint32_t threads, uint8_t *status, uint64_t *new_start, uint64_t *new_end,
                                      char *digests, char *anchors) {
    return guarded([&]() -> gtars_status {
        if (!b) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (n && (!tx || !start || !ref_off || !ref_len || !alt_off || !alt_len || (!pool && pool_bytes)))
            return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        if (!n) return GTARS_OK;
        const gtars::TxBindParts p = gtars::tx_bind_parts(b);
        const gtars::TxTables t = p.tables->view();
        gtars::VrsTxCall call;
        call.tx = tx, call.start = start, call.pool = pool, call.pool_bytes = pool_bytes;
        call.ref_off = ref_off, call.ref_len = ref_len, call.alt_off = alt_off, call.alt_len = alt_len, call.n = n;
        call.host.h_tables = &t, call.host.h_seq = p.h_seq, call.host.threads = threads_of(threads);
        call.status = status, call.new_start = new_start, call.new_end = new_end, call.digest = digests, call.anchor = anchors;
        if (on_host) return tx_alleles_on_host(p, call, call.host.threads), GTARS_OK;
        gtars::Assembly *image;
        gtars::TxDevice *dev;
        if (const gtars_status e = gtars::tx_bind_device(b, &image, &dev)) return e;
        return gtars::vrs_tx_run(*image, *dev, call);
    });
}

}  // extern "C"
