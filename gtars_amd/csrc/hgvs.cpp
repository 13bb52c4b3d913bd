// hgvs.cpp -- the host layer of K20 (gtars.vrs.hgvs; gtars-vrs/src/hgvs/{parser,bridge}.rs, gtars-python/src/vrs/hgvs.rs): the
// scalar parse, the batch parse and accession lookup on the host threads, the library's host path of the bridge and the
// batch calls on top of hgvs.hip.  Declared in include/gtars_amd_host.h.  The rules themselves are hgvs_core.h.
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

}  // extern "C"
