// tokbatch.h -- internal interface of tokbatch.hip (K15: a batch of region sets encoded as B independent
// Tokenizer::tokenize calls in one device pass) for the host layer.  Plain C++: host.cpp includes it without the HIP headers.
// Chromosomes are ids of the index's dictionary.
#pragma once

#include <cstdint>
#include <cstdlib>

#include "../../include/gtars_amd.h"

namespace gtars {

constexpr uint64_t TOKBATCH_MAX_SETS = 0xFFFFF000ull;  // one lane per set, and the device scan takes that many counts
constexpr uint32_t TOKBATCH_PACK_TILE = 1024;          // output ids a workgroup of k_set_pack packs per step

// what tokbatch_encode allocates for its caller (malloc; whoever takes a pointer out sets it to null here)
struct TokBatchOut {
    uint64_t *offsets = nullptr;    // [n_sets + 1]
    uint32_t *ids = nullptr;        // [total]
    uint32_t *input_ids = nullptr;  // [n_sets * width]
    uint8_t *mask = nullptr;        // [n_sets * width]
    uint64_t total = 0, longest = 0, width = 0;
    TokBatchOut() = default;
    TokBatchOut(const TokBatchOut &) = delete;
    TokBatchOut &operator=(const TokBatchOut &) = delete;
    ~TokBatchOut() {
        free(offsets);
        free(ids);
        free(input_ids);
        free(mask);
    }
};

// set_offsets[0 .. n_sets]: starts at 0, never descends, ends at n -- else GTARS_ERR_INVALID_ARG
gtars_status tokbatch_check_offsets(const uint64_t *set_offsets, uint64_t n_sets, uint64_t n);

// Host columns of n query rows, set b = rows [set_offsets[b], set_offsets[b + 1]); on the index's device.
//   ragged: out.offsets / out.ids / out.total -- per set what Tokenizer::tokenize (tokenizer.rs:140-163) gives for it alone,
//           [unk_id] for a set without any id, then the first max_length ids (0: all of them)
//   padded: out.input_ids / out.mask / out.width -- row b = the set's ids and pad_id on the given side (GTARS_PAD_RIGHT /
//           GTARS_PAD_LEFT); width_or_0 == 0: the longest set, else that width, which must hold the longest set
gtars_status tokbatch_encode(const gtars_index_t *ix, const uint32_t *chrom, const uint32_t *start, const uint32_t *end, uint64_t n,
                             const uint64_t *set_offsets, uint64_t n_sets, uint32_t unk_id, uint64_t max_length, bool ragged,
                             bool padded, uint64_t width_or_0, int side, uint32_t pad_id, TokBatchOut &out);

}  // namespace gtars
