// partitions.cpp -- partition lists on the host and the library calls of K14 on top of partitions.hip: calc_partitions
// and the arithmetic of calc_expected_partitions (gtars-genomicdist/src/partitions.rs:493-784).  Declared in
// include/gtars_amd_host.h.  Region sets are read through their public accessors.
#include <cmath>
#include <limits>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/gtars_amd_host.h"
#include "guard.h"
#include "partitions.h"

using gtars::fail;
using gtars::guarded;

struct gtars_partition_list {
    struct Part {
        std::string name;
        std::vector<uint32_t> chrom, start, end;  // the set's rows in set order, chrom = id in `names`
    };
    std::vector<Part> parts;
    std::vector<std::string> names;  // chromosome id -> name, in order of first appearance over the sets
    std::unordered_map<std::string, uint32_t> id;
    std::mutex mu;  // guards the lazy device index
    gtars::PartDevice *dev = nullptr;
    ~gtars_partition_list() { gtars::part_free(dev); }
};

namespace {

// the handle's device index, built at the first count on the device current then
gtars_status device_index(gtars_partition_list *pl, gtars::PartDevice **out) {
    std::lock_guard<std::mutex> lk(pl->mu);
    if (!pl->dev) {
        std::vector<gtars::PartCols> cols;
        for (const auto &p : pl->parts) cols.push_back(gtars::PartCols{p.chrom.data(), p.start.data(), p.end.data(), p.start.size()});
        if (const gtars_status e = gtars::part_build(cols, (uint32_t)pl->names.size(), &pl->dev)) return e;
    }
    *out = pl->dev;
    return GTARS_OK;
}

// the device's u64 sums as the reference's release-build u32 arithmetic (partitions.rs:506-592)
void finish_counts(const std::vector<uint64_t> &raw, size_t np, uint64_t n, bool bp, uint32_t *counts, uint32_t *total) {
    if (!bp) {
        for (size_t k = 0; k <= np; ++k) counts[k] = (uint32_t)raw[k];
        *total = (uint32_t)n;
        return;
    }
    uint32_t assigned = 0;
    for (size_t k = 0; k < np; ++k) assigned += counts[k] = (uint32_t)raw[k];
    *total = (uint32_t)raw[np];
    counts[np] = *total > assigned ? *total - assigned : 0;  // saturating_sub
}

// ---- chi_square_2x2 and what it stands on (partitions.rs:663-784), f64 throughout
double ln_gamma(double x) {
    static const double kCoeffs[9] = {0.99999999999980993,  676.5203681218851,     -1259.1392167224028,
                                      771.32342877765313,   -176.61502916214059,   12.507343278686905,
                                      -0.13857109526572012, 9.9843695780195716e-6, 1.5056327351493116e-7};
    const double pi = 3.14159265358979323846;
    if (x < 0.5) return std::log(pi / std::sin(pi * x)) - ln_gamma(1.0 - x);
    x -= 1.0;
    double sum = kCoeffs[0];
    for (int i = 0; i < 8; ++i) sum += kCoeffs[i + 1] / (x + (double)i + 1.0);
    const double t = x + 7.5;
    return 0.5 * std::log(2.0 * pi) + std::log(t) * (x + 0.5) - t + std::log(sum);
}

double gamma_series(double a, double x, double ln_gamma_a) {
    double sum = 1.0 / a, term = 1.0 / a;
    for (int n = 1; n < 200; ++n) {
        term *= x / (a + (double)n);
        sum += term;
        if (std::fabs(term) < std::fabs(sum) * 1e-14) break;
    }
    return sum * std::exp(-x + a * std::log(x) - ln_gamma_a);
}

double gamma_cf(double a, double x, double ln_gamma_a) {
    double d = 1.0 / (x + 1.0 - a), c = 1.0 / 1e-30, f = d;
    for (int n = 1; n < 200; ++n) {
        const double an = -(double)n * ((double)n - a), bn = x + 2.0 * (double)n + 1.0 - a;
        d = bn + an * d;
        if (std::fabs(d) < 1e-30) d = 1e-30;
        d = 1.0 / d;
        c = bn + an / c;
        if (std::fabs(c) < 1e-30) c = 1e-30;
        const double delta = c * d;
        f *= delta;
        if (std::fabs(delta - 1.0) < 1e-14) break;
    }
    const double r = f * std::exp(-x + a * std::log(x) - ln_gamma_a);
    return r < 0.0 ? 0.0 : r > 1.0 ? 1.0 : r;  // f64::clamp (a NaN stays)
}

double regularized_gamma_lower(double a, double x) {
    if (x < 0.0 || x == 0.0) return 0.0;
    const double lg = ln_gamma(a);
    return x < a + 1.0 ? gamma_series(a, x, lg) : 1.0 - gamma_cf(a, x, lg);
}

double chi_square_2x2(double obs, double exp, double total) {
    if (total == 0.0 || exp == 0.0 || total - exp == 0.0) return 1.0;
    const double non_obs = total - obs, non_exp = total - exp;
    const double chi = (obs - exp) * (obs - exp) / exp + (non_obs - non_exp) * (non_obs - non_exp) / non_exp;
    return 1.0 - regularized_gamma_lower(0.5, chi / 2.0);
}

}  // namespace

extern "C" {

gtars_status gtars_partition_list_from_sets(const char *const *names, const gtars_regionset_t *const *sets, uint32_t n,
                                            gtars_partition_list_t **out) {
    return guarded([&]() -> gtars_status {
        if (!out || (n && (!names || !sets))) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        if (n > gtars::PART_MAX) return fail(GTARS_ERR_INVALID_ARG, "more than " + std::to_string(gtars::PART_MAX) + " partitions");
        auto pl = std::make_unique<gtars_partition_list>();
        pl->parts.resize(n);
        for (uint32_t k = 0; k < n; ++k) {
            if (!names[k] || !sets[k]) return fail(GTARS_ERR_INVALID_ARG, "NULL partition name or set");
            gtars_partition_list::Part &p = pl->parts[k];
            p.name = names[k];
            const gtars_regionset_t *rs = sets[k];
            const uint32_t nc = gtars_regionset_n_chrom(rs);
            std::vector<uint32_t> map(nc);
            for (uint32_t c = 0; c < nc; ++c) {
                const std::string nm = gtars_regionset_chrom_name(rs, c);
                auto it = pl->id.find(nm);
                if (it == pl->id.end()) {
                    it = pl->id.emplace(nm, (uint32_t)pl->names.size()).first;
                    pl->names.push_back(nm);
                }
                map[c] = it->second;
            }
            const uint64_t m = gtars_regionset_len(rs);
            const uint32_t *cid = gtars_regionset_chrom_ids(rs), *s = gtars_regionset_starts(rs), *e = gtars_regionset_ends(rs);
            p.chrom.resize(m);
            for (uint64_t i = 0; i < m; ++i) p.chrom[i] = map[cid[i]];
            p.start.assign(s, s + m);
            p.end.assign(e, e + m);
        }
        *out = pl.release();
        return GTARS_OK;
    });
}

void gtars_partition_list_free(gtars_partition_list_t *pl) { delete pl; }
uint32_t gtars_partition_list_len(const gtars_partition_list_t *pl) { return pl ? (uint32_t)pl->parts.size() : 0; }
const char *gtars_partition_list_name(const gtars_partition_list_t *pl, uint32_t i) {
    return pl && i < pl->parts.size() ? pl->parts[i].name.c_str() : nullptr;
}
uint32_t gtars_partition_list_n_chrom(const gtars_partition_list_t *pl) { return pl ? (uint32_t)pl->names.size() : 0; }
const char *gtars_partition_list_chrom_name(const gtars_partition_list_t *pl, uint32_t id) {
    return pl && id < pl->names.size() ? pl->names[id].c_str() : nullptr;
}

gtars_status gtars_partition_list_set(const gtars_partition_list_t *pl, uint32_t i, gtars_regionset_t **out) {
    return guarded([&]() -> gtars_status {
        if (!pl || !out) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        *out = nullptr;
        if (i >= pl->parts.size()) return fail(GTARS_ERR_INVALID_ARG, "partition index out of range");
        const gtars_partition_list::Part &p = pl->parts[i];
        std::vector<const char *> chr(p.chrom.size());
        for (size_t k = 0; k < chr.size(); ++k) chr[k] = pl->names[p.chrom[k]].c_str();
        return gtars_regionset_from_arrays(chr.data(), p.start.data(), p.end.data(), nullptr, chr.size(), out);
    });
}

gtars_status gtars_partition_list_sizes(const gtars_partition_list_t *pl, uint64_t *out) {
    if (!pl || (!out && !pl->parts.empty())) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    for (size_t k = 0; k < pl->parts.size(); ++k) {
        const gtars_partition_list::Part &p = pl->parts[k];
        uint64_t bp = 0;
        for (size_t i = 0; i < p.start.size(); ++i) bp += (uint32_t)(p.end[i] - p.start[i]);
        out[k] = bp;
    }
    return GTARS_OK;
}

int gtars_partition_list_device(const gtars_partition_list_t *pl) {
    if (!pl) return -1;
    std::lock_guard<std::mutex> lk(const_cast<gtars_partition_list_t *>(pl)->mu);
    return gtars::part_device(pl->dev);
}

gtars_status gtars_partitions_count(gtars_partition_list_t *pl, const gtars_regionset_t *query, int bp_proportion, uint32_t *counts,
                                    uint32_t *total, uint8_t *assignments) {
    return guarded([&]() -> gtars_status {
        if (!pl || !query || !counts || !total) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        const size_t np = pl->parts.size();
        const uint64_t n = gtars_regionset_len(query);
        std::vector<uint64_t> raw(np + 1, 0);
        if (n) {
            const uint32_t nc = gtars_regionset_n_chrom(query);
            std::vector<uint32_t> seg_of(nc, GTARS_UNKNOWN_CHROM);
            for (uint32_t k = 0; k < nc; ++k) {
                auto it = pl->id.find(gtars_regionset_chrom_name(query, k));
                if (it != pl->id.end()) seg_of[k] = it->second;
            }
            gtars::PartDevice *dev;
            if (const gtars_status e = device_index(pl, &dev)) return e;
            if (const gtars_status e = gtars::part_count(dev, gtars_regionset_chrom_ids(query), gtars_regionset_starts(query),
                                                         gtars_regionset_ends(query), n, seg_of, bp_proportion != 0, raw.data(), assignments))
                return e;
        } else if (bp_proportion && assignments) {
            return fail(GTARS_ERR_INVALID_ARG, "per-query assignments exist in priority mode only");
        }
        finish_counts(raw, np, n, bp_proportion != 0, counts, total);
        return GTARS_OK;
    });
}

gtars_status gtars_partitions_count_device(gtars_partition_list_t *pl, const uint32_t *d_chrom, const uint32_t *d_start,
                                           const uint32_t *d_end, uint64_t n, int bp_proportion, void *stream, uint32_t *counts,
                                           uint32_t *total, uint8_t *d_assignments) {
    return guarded([&]() -> gtars_status {
        if (!pl || !counts || !total) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        const size_t np = pl->parts.size();
        std::vector<uint64_t> raw(np + 1, 0);
        if (n) {
            gtars::PartDevice *dev;
            if (const gtars_status e = device_index(pl, &dev)) return e;
            if (const gtars_status e =
                    gtars::part_count_device(dev, d_chrom, d_start, d_end, n, bp_proportion != 0, raw.data(), d_assignments, stream))
                return e;
        } else if (bp_proportion && d_assignments) {
            return fail(GTARS_ERR_INVALID_ARG, "per-query assignments exist in priority mode only");
        }
        finish_counts(raw, np, n, bp_proportion != 0, counts, total);
        return GTARS_OK;
    });
}

gtars_status gtars_partition_expected(const uint32_t *observed, const uint64_t *partition_bp, uint32_t n_partitions, uint32_t total,
                                      uint64_t genome_size, double *expected, double *log10_oe, double *pvalue) {
    if (!observed || !expected || !log10_oe || !pvalue || (n_partitions && !partition_bp)) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
    uint64_t sum = 0;
    for (uint32_t k = 0; k < n_partitions; ++k) sum += partition_bp[k];
    const double query_total = (double)total, inf = std::numeric_limits<double>::infinity();
    for (uint32_t k = 0; k <= n_partitions; ++k) {
        const uint64_t bp = k < n_partitions ? partition_bp[k] : genome_size > sum ? genome_size - sum : 0;  // saturating_sub
        const double obs = (double)observed[k], exp = ((double)bp / (double)genome_size) * query_total;
        expected[k] = exp;
        log10_oe[k] = obs == 0.0 ? -inf : exp == 0.0 ? inf : std::log10(obs / exp);
        pvalue[k] = chi_square_2x2(obs, exp, query_total);
    }
    return GTARS_OK;
}

}  // extern "C"
