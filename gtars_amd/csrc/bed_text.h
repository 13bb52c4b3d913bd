// bed_text.h -- K25 between its host layer (bed_text.cpp) and its device pipeline (bed_text.hip): the text streams of
// bed_text_core.h over a batch of region sets given as concatenated columns.
#pragma once

#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/gtars_amd.h"

namespace gtars {

// A batch of sets as concatenated columns: set b = the rows [set_off[b], set_off[b + 1]), set_off[0] = 0.  chrom[i] names a
// row of the names table (a byte CSR: name c = names[name_off[c] .. name_off[c + 1])); the ids of every set are rebased
// into that one table.  The rest columns serve GTARS_BED_FILE_DIGEST and the text alone and may be null otherwise: row i's
// rest = rest[rest_off[i] .. rest_off[i + 1]) where has_rest[i].  set_off is always host memory; the other columns are
// host or device memory as the call says.
struct BedCols {
    const uint64_t *set_off = nullptr;
    uint64_t n_sets = 0;
    const uint32_t *chrom = nullptr, *start = nullptr, *end = nullptr;
    const uint64_t *name_off = nullptr;
    const uint8_t *names = nullptr;
    uint32_t n_names = 0;
    const uint64_t *rest_off = nullptr;
    const uint8_t *rest = nullptr, *has_rest = nullptr;
};

// `text` to the file at `path` (its directory is created): as it is, or as one gzip member at the best compression level --
// what to_bed / to_bed_gz write, and K26's fragment files
gtars_status write_text_file(const std::string &text, const char *path, bool gz);

constexpr int BED_WHAT_TEXT = 2;  // (behind GTARS_BED_IDENTIFIER = 0 and GTARS_BED_FILE_DIGEST = 1 of gtars_amd.h)

// the switches of K25
uint64_t bed_digest_host_len();   // GTARS_BED_DIGEST_HOST_LEN; 0: the rule of the batch (bed_text.hip)
uint64_t bed_text_bytes();        // GTARS_BED_TEXT_BYTES
uint64_t bed_text_device_rows();  // GTARS_BED_TEXT_DEVICE_ROWS

// an upper bound of the text bytes of a set of `rows` rows with `rest_bytes` bytes of rest, names up to max_name bytes
inline uint64_t bed_text_bound(int what, uint64_t rows, uint64_t rest_bytes, uint64_t max_name) {
    return what == 0 ? rows * (max_name + 1 + 11 + 11) : rows * (max_name + 1 + 11 + 11 + 1) + rest_bytes;
}

// the list cut into chunks of whole sets: `cut` ascends from 0 to n_sets; a chunk's bound stays below `limit` unless it is
// one set, and its rows below max_rows (a set with more rows than that is GTARS_ERR_INVALID_ARG)
gtars_status bed_plan_chunks(const std::vector<uint64_t> &bound, const uint64_t *set_off, uint64_t limit, uint64_t max_rows,
                             std::vector<uint64_t> &cut);

// The columns are device memory, on the calling thread's device; the work is queued on `stream`, which is drained.  what =
// identifier or file digest: d_out[2 * n_sets] receives one digest per set in md5_words form (8-byte aligned device
// memory).  what = BED_WHAT_TEXT: *text receives the LINE stream of all rows (n_sets == 1 is what to_bed writes).
gtars_status bed_text_run_device(const BedCols &cols, int what, uint64_t *d_out, std::string *text, unsigned threads, void *stream);

// The same over host columns that the caller stages chunk by chunk: stage(s0, s1, c) fills `c` with host columns of the
// sets [s0, s1) alone (set_off rebased to 0, c.n_sets = s1 - s0), valid until the next call of stage.  bound[b]: the text
// bound of set b.  out[2 * n_sets] (host) / *text as above.  Runs on the current device's null stream.
using BedStage = std::function<void(uint64_t s0, uint64_t s1, BedCols &c)>;
gtars_status bed_text_run_host_cols(const uint64_t *set_off, uint64_t n_sets, const std::vector<uint64_t> &bound, const BedStage &stage, int what,
                                    uint64_t *out, std::string *text, unsigned threads);

}  // namespace gtars
