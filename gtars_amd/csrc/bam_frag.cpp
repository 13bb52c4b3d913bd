// bam_frag.cpp -- the host layer of K26: the result handle's accessors, the fragment text from the row
// columns, and the file writer (the one to_bed / to_bed_gz use).  Plain C++: the device pipeline is in bam.hip.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "bam_frag.h"
#include "bed_text.h"
#include "bed_text_core.h"
#include "guard.h"
#include "host_threads.h"

namespace gtars {

gtars_status bam_frag_text(const std::vector<std::string> &ref_names, const std::vector<std::string> &barcodes, const int32_t *ref,
                           const uint32_t *start, const uint32_t *end, const uint32_t *barcode, const uint32_t *count, uint64_t n, unsigned threads,
                           std::string &text) {
    text.clear();
    if (!n) return GTARS_OK;
    for (uint64_t i = 0; i < n; ++i)
        if (ref[i] < 0 || (size_t)ref[i] >= ref_names.size() || barcode[i] >= barcodes.size())
            return fail(GTARS_ERR_INVALID_ARG, "fragment row " + std::to_string(i) + " names no reference or no barcode");
    // the rows in pieces of 64 Ki: a piece's bytes are counted, then every piece is filled at its offset
    const uint64_t piece = 1u << 16, n_pieces = (n + piece - 1) / piece;
    threads = std::max(threads, 1u);
    std::vector<uint64_t> off(n_pieces + 1, 0);
    parallel_for((size_t)n_pieces, threads, 1, [&](size_t k) {
        uint64_t bytes = 0;
        for (uint64_t i = k * piece; i < std::min(n, (k + 1) * piece); ++i)
            bytes += ref_names[ref[i]].size() + barcodes[barcode[i]].size() + bed_u32_width(start[i]) + bed_u32_width(end[i]) +
                     bed_u32_width(count[i]) + 5;
        off[k + 1] = bytes;
    });
    for (uint64_t k = 0; k < n_pieces; ++k) off[k + 1] += off[k];
    text.resize(off[n_pieces]);
    parallel_for((size_t)n_pieces, threads, 1, [&](size_t k) {
        char *p = &text[off[k]];
        auto put_str = [&](const std::string &s, char sep) {
            memcpy(p, s.data(), s.size());
            p += s.size();
            *p++ = sep;
        };
        auto put_u32 = [&](uint32_t v, char sep) {
            const uint32_t w = bed_u32_width(v);
            for (uint32_t d = w; d-- > 0; v /= 10u) p[d] = (char)('0' + v % 10u);
            p += w;
            *p++ = sep;
        };
        for (uint64_t i = k * piece; i < std::min(n, (k + 1) * piece); ++i) {
            put_str(ref_names[ref[i]], '\t');
            put_u32(start[i], '\t');
            put_u32(end[i], '\t');
            put_str(barcodes[barcode[i]], '\t');
            put_u32(count[i], '\n');
        }
    });
    return GTARS_OK;
}

namespace {

bool ends_in_gz(const char *path) {
    const size_t l = strlen(path);
    return l >= 3 && memcmp(path + l - 3, ".gz", 3) == 0;
}

gtars_status write_rows(const char *path, const std::vector<std::string> &ref_names, const std::vector<std::string> &barcodes, const int32_t *ref,
                        const uint32_t *start, const uint32_t *end, const uint32_t *barcode, const uint32_t *count, uint64_t n) {
    std::string text;
    if (const gtars_status e = bam_frag_text(ref_names, barcodes, ref, start, end, barcode, count, n, gtars_host_threads(16), text)) return e;
    return write_text_file(text, path, ends_in_gz(path));
}

}  // namespace
}  // namespace gtars

using gtars::fail;
using gtars::guarded;

extern "C" {

void gtars_bam_frag_params_default(gtars_bam_frag_params *p) {
    if (!p) return;
    memset(p, 0, sizeof *p);
    p->barcode_tag[0] = 'C', p->barcode_tag[1] = 'B', p->use_barcode_tag = 1, p->sample = "bulk";
    p->min_mapq = 30, p->max_fragment_length = 2000, p->shift_left = 4, p->shift_right = -5;
    p->require_flags = 0x3, p->exclude_flags = 0xB0C;
}

uint64_t gtars_bam_frags_len(const gtars_bam_frags_t *f) { return f ? f->ref.size() : 0; }
const int32_t *gtars_bam_frags_ref(const gtars_bam_frags_t *f) { return f ? f->ref.data() : nullptr; }
const uint32_t *gtars_bam_frags_start(const gtars_bam_frags_t *f) { return f ? f->start.data() : nullptr; }
const uint32_t *gtars_bam_frags_end(const gtars_bam_frags_t *f) { return f ? f->end.data() : nullptr; }
const uint32_t *gtars_bam_frags_barcode(const gtars_bam_frags_t *f) { return f ? f->barcode.data() : nullptr; }
const uint32_t *gtars_bam_frags_count(const gtars_bam_frags_t *f) { return f ? f->count.data() : nullptr; }
uint64_t gtars_bam_frags_n_barcodes(const gtars_bam_frags_t *f) { return f ? f->barcodes.size() : 0; }
const char *gtars_bam_frags_barcode_name(const gtars_bam_frags_t *f, uint64_t i, uint64_t *len) {
    if (!f || i >= f->barcodes.size()) return nullptr;
    if (len) *len = f->barcodes[i].size();
    return f->barcodes[i].c_str();
}
void gtars_bam_frags_stats(const gtars_bam_frags_t *f, uint64_t *out12) {
    if (f && out12) memcpy(out12, f->stats, sizeof f->stats);
}
void gtars_bam_frags_free(gtars_bam_frags_t *f) { delete f; }

gtars_status gtars_bam_frags_write(const gtars_bam_frags_t *f, const gtars_bam_t *b, const char *path) {
    return guarded([&]() -> gtars_status {
        if (!f || !b || !path) return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        std::vector<std::string> refs;
        for (uint32_t i = 0; i < gtars_bam_n_ref(b); ++i) refs.emplace_back(gtars_bam_ref_name(b, i));
        return gtars::write_rows(path, refs, f->barcodes, f->ref.data(), f->start.data(), f->end.data(), f->barcode.data(), f->count.data(),
                                 f->ref.size());
    });
}

gtars_status gtars_fragments_write_text(const char *path, const char *const *ref_names, uint32_t n_ref, const char *const *barcodes,
                                        uint64_t n_barcodes, const int32_t *ref, const uint32_t *start, const uint32_t *end,
                                        const uint32_t *barcode, const uint32_t *count, uint64_t n) {
    return guarded([&]() -> gtars_status {
        if (!path || (n_ref && !ref_names) || (n_barcodes && !barcodes) || (n && (!ref || !start || !end || !barcode || !count)))
            return fail(GTARS_ERR_INVALID_ARG, "NULL argument");
        std::vector<std::string> refs, bcs;
        for (uint32_t i = 0; i < n_ref; ++i) refs.emplace_back(ref_names[i] ? ref_names[i] : "");
        for (uint64_t i = 0; i < n_barcodes; ++i) bcs.emplace_back(barcodes[i] ? barcodes[i] : "");
        return gtars::write_rows(path, refs, bcs, ref, start, end, barcode, count, n);
    });
}

}  // extern "C"
