// bam.h -- K17: BAM input.  The host half (bam.cpp, plain C++: the BGZF container, the inflate on the
// host threads, the BAM header and the walk over the records' block_size chain) and what the device half (bam.hip: the
// window pipeline, k_bam_decode and the QC kernels) needs from it.  No HIP types here.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "../../include/gtars_amd_host.h"
#include "bgzf.h"
#include "guard.h"

namespace gtars {

struct BamRef {
    std::string name;
    uint32_t len;
};

struct BamFile {
    std::string path;
    std::string raw;  // the file, followed by 16 zero bytes the decoder may read into
    uint64_t n_raw = 0;
    std::vector<BamBlock> blocks;
    uint64_t n_bytes = 0;  // inflated
    std::string text;      // header text
    std::vector<BamRef> refs;
    std::vector<uint8_t> mito;  // per reference: counted as mitochondrial by the QC
    uint64_t first_record = 0;  // inflated offset of the first record
};

gtars_status bam_open(const std::string &path, BamFile &f);

// blocks [b0, b1) inflated to dst, block b at dst + (uoff[b] - uoff[b0]); every block's length and CRC-32 are checked.
// threads: 0 = the library's budget; always capped by it.
gtars_status bam_inflate(const BamFile &f, uint64_t b0, uint64_t b1, uint8_t *dst, unsigned threads);

// the running state of the record walk over consecutive byte ranges of one file: what the coordinate-sorted domain needs
struct BamWalk {
    uint64_t n_records = 0;
    int32_t last_ref = 0;  // refID of the last record (0 before the first: ids ascend from 0; -1 once the unplaced tail began)
};
// the runs of equal refID among the records one bam_walk call found: run k = records [start[k], start[k + 1]) of that call
struct BamSegs {
    std::vector<uint32_t> start;
    std::vector<int32_t> ref;
};
// The records of data[begin, n): offs receives each record's offset (of its block_size field) as `base + offset in data`
// truncated to T; *consumed = where the first incomplete record starts (n if none).  final: an incomplete record is an error.
// refID must not descend, -1 only at the end, and lie in [-1, n_ref).
gtars_status bam_walk(const uint8_t *data, uint64_t n, uint64_t begin, bool final, int64_t n_ref, BamWalk &w, std::vector<uint32_t> *offs32,
                      std::vector<uint64_t> *offs64, uint64_t base, uint64_t *consumed, BamSegs *segs = nullptr);

bool bam_is_mito(const std::string &name);

}  // namespace gtars
