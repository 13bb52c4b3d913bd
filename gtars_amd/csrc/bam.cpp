// bam.cpp -- K17, host half: the BGZF container and the BAM framing.  Written from the SAM/BAM format
// specification (sections 4.1 "The BGZF compression format" and 4.2 "The BAM format").  Host threads only inflate; every
// field of a record behind its block_size and refID is read on the device (bam.hip).
#include "bam.h"

#include <zlib.h>

#include <cerrno>
#include <cstdio>
#include <cstring>
#include <mutex>

#include "host_threads.h"
#include "inflate_fast.h"

namespace gtars {

namespace {

inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t le32(const uint8_t *p) { return le16(p) | (le16(p + 2) << 16); }

std::string blk(uint64_t i) { return "BGZF block " + std::to_string(i); }

// One pass over the file, nothing is decoded.
gtars_status block_table(BamFile &f) {
    const uint8_t *p = (const uint8_t *)f.raw.data();
    const uint64_t n = f.n_raw;
    uint64_t at = 0, uoff = 0;
    while (at < n) {
        const uint64_t i = f.blocks.size();
        BamBlock b;
        uint64_t bsize = 0;
        switch (bgzf_member_at(p, n, at, uoff, b, &bsize)) {
            case BgzfFrame::ok: break;
            case BgzfFrame::truncated:
                return fail(GTARS_ERR_PARSE, f.path + ": " + blk(i) + " is truncated (" + std::to_string(n - at) + " bytes left in the file)");
            case BgzfFrame::no_magic:
                return fail(GTARS_ERR_PARSE, f.path + ": " + blk(i) + " at offset " + std::to_string(at) + " does not start with the gzip magic");
            case BgzfFrame::flags: return fail(GTARS_ERR_PARSE, f.path + ": " + blk(i) + " has gzip flags other than FEXTRA: not BGZF");
            case BgzfFrame::extra_past_end: return fail(GTARS_ERR_PARSE, f.path + ": " + blk(i) + ": the extra field runs past the end of the file");
            case BgzfFrame::no_bc: return fail(GTARS_ERR_PARSE, f.path + ": " + blk(i) + " has no BC subfield (gzip, but not BGZF)");
            case BgzfFrame::past_end:
                return fail(GTARS_ERR_PARSE, f.path + ": " + blk(i) + " runs past the end of the file (BSIZE " + std::to_string(bsize) + " at offset " +
                                                 std::to_string(at) + ", file of " + std::to_string(n) + " bytes)");
            case BgzfFrame::bsize_small: return fail(GTARS_ERR_PARSE, f.path + ": " + blk(i) + ": BSIZE is smaller than the member's header and trailer");
            case BgzfFrame::isize_large:
                return fail(GTARS_ERR_PARSE, f.path + ": " + blk(i) + ": ISIZE " + std::to_string(le32(p + at + bsize + 1 - 4)) + " > 65536");
        }
        f.blocks.push_back(b);
        uoff += b.isize;
        at += b.csize;
    }
    f.n_bytes = uoff;
    return GTARS_OK;
}

// block b into dst (b.isize bytes): inflate_fast.h first, zlib for what it refuses -- and for what it got wrong, so that the
// message of a damaged block is zlib's verdict.  The fast decoder writes up to a margin past what it produced, so it decodes
// into a buffer of the thread and the block is copied from there: a neighbour's bytes are another thread's.
bool inflate_block(const BamFile &f, uint64_t i, uint8_t *dst, std::string &err) {
    const BamBlock &b = f.blocks[i];
    const uint8_t *in = (const uint8_t *)f.raw.data() + b.coff + b.doff;
    const size_t in_n = b.csize - b.doff - 8;
    thread_local std::string scratch;
    size_t used = 0, done = 0;
    if (fastinf::inflate_raw(in, in_n, &used, scratch, done) && done == b.isize && used <= in_n &&
        (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)scratch.data(), (uInt)done) == b.crc) {
        if (done) memcpy(dst, scratch.data(), done);
        return true;
    }
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, -MAX_WBITS) != Z_OK) {
        err = blk(i) + ": cannot initialise zlib";
        return false;
    }
    uint8_t out[BGZF_MAX_ISIZE + 1];
    z.next_in = (Bytef *)in;
    z.avail_in = (uInt)in_n;
    z.next_out = out;
    z.avail_out = sizeof out;
    const int r = inflate(&z, Z_FINISH);
    const size_t got = sizeof out - z.avail_out;
    const std::string zmsg = z.msg ? z.msg : "";
    inflateEnd(&z);
    if (r != Z_STREAM_END) {
        err = blk(i) + (r == Z_BUF_ERROR && got > b.isize ? ": inflates to more than its ISIZE " + std::to_string(b.isize)
                                                          : ": invalid deflate stream" + (zmsg.empty() ? "" : " (" + zmsg + ")"));
        return false;
    }
    if (got != b.isize) {
        err = blk(i) + ": inflated to " + std::to_string(got) + " bytes, ISIZE says " + std::to_string(b.isize);
        return false;
    }
    if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), out, (uInt)got) != b.crc) {
        err = blk(i) + ": CRC-32 mismatch";
        return false;
    }
    if (got) memcpy(dst, out, got);
    return true;
}

}  // namespace

bool bam_is_mito(const std::string &name) {
    std::string l = name;
    for (char &c : l)
        if (c >= 'A' && c <= 'Z') c = (char)(c - 'A' + 'a');
    return l == "chrm" || l == "mt" || l == "chrmt" || l.find("rcrsd") != std::string::npos;
}

gtars_status bam_inflate(const BamFile &f, uint64_t b0, uint64_t b1, uint8_t *dst, unsigned threads) {
    if (b0 > b1 || b1 > f.blocks.size()) return fail(GTARS_ERR_INVALID_ARG, "block range out of bounds");
    if (b0 == b1) return GTARS_OK;
    const unsigned budget = gtars_host_threads(0);
    const unsigned nt = threads ? std::min(threads, budget) : budget;
    const uint64_t base = f.blocks[b0].uoff;
    std::mutex mx;
    uint64_t bad = UINT64_MAX;
    std::string bad_msg;
    parallel_for((size_t)(b1 - b0), nt, 8, [&](size_t k) {
        std::string err;
        if (!inflate_block(f, b0 + k, dst + (f.blocks[b0 + k].uoff - base), err)) {
            std::lock_guard<std::mutex> lk(mx);
            if (b0 + k < bad) bad = b0 + k, bad_msg = err;
        }
    });
    if (bad != UINT64_MAX) return fail(GTARS_ERR_PARSE, f.path + ": " + bad_msg);
    return GTARS_OK;
}

gtars_status bam_open(const std::string &path, BamFile &f) {
    f.path = path;
    FILE *fp = fopen(path.c_str(), "rb");
    if (!fp) return fail(GTARS_ERR_IO, "Failed to open file: \"" + path + "\": " + strerror(errno));
    char buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, fp)) > 0) f.raw.append(buf, k);
    fclose(fp);
    f.n_raw = f.raw.size();
    f.raw.append(16, '\0');
    if (gtars_status st = block_table(f)) return st;

    // the header: as many leading blocks as it takes
    std::vector<uint8_t> h;
    uint64_t next = 0;
    gtars_status st = GTARS_OK;
    auto need = [&](uint64_t upto) {  // -> h holds upto bytes
        while (h.size() < upto) {
            if (next == f.blocks.size()) {
                st = fail(GTARS_ERR_PARSE, path + ": the BAM header is truncated (the data ends after " + std::to_string(h.size()) + " bytes)");
                return false;
            }
            const size_t at = h.size();
            h.resize(at + f.blocks[next].isize);
            if ((st = bam_inflate(f, next, next + 1, h.data() + at, 1))) return false;
            ++next;
        }
        return true;
    };
    if (!need(4)) return st;
    if (memcmp(h.data(), "BAM\1", 4)) return fail(GTARS_ERR_PARSE, path + ": not a BAM file (the inflated data does not start with the magic BAM\\1)");
    if (!need(8)) return st;
    const uint64_t l_text = le32(h.data() + 4);
    if (!need(8 + l_text + 4)) return st;
    f.text.assign((const char *)h.data() + 8, l_text);
    while (!f.text.empty() && f.text.back() == '\0') f.text.pop_back();
    uint64_t at = 8 + l_text;
    const int64_t n_ref = (int32_t)le32(h.data() + at);
    at += 4;
    if (n_ref < 0) return fail(GTARS_ERR_PARSE, path + ": negative n_ref in the BAM header");
    for (int64_t r = 0; r < n_ref; ++r) {
        if (!need(at + 4)) return st;
        const uint64_t l_name = le32(h.data() + at);
        if (!need(at + 4 + l_name + 4)) return st;
        std::string name((const char *)h.data() + at + 4, l_name);
        while (!name.empty() && name.back() == '\0') name.pop_back();
        f.refs.push_back(BamRef{name, le32(h.data() + at + 4 + l_name)});
        f.mito.push_back(bam_is_mito(name));
        at += 8 + l_name;
    }
    f.first_record = at;
    return GTARS_OK;
}

gtars_status bam_walk(const uint8_t *data, uint64_t n, uint64_t begin, bool final, int64_t n_ref, BamWalk &w, std::vector<uint32_t> *offs32,
                      std::vector<uint64_t> *offs64, uint64_t base, uint64_t *consumed, BamSegs *segs) {
    uint64_t at = begin, k = 0;
    while (at < n) {
        if (n - at < 4) break;
        const uint64_t bs = le32(data + at);
        if (bs < 32) return fail(GTARS_ERR_PARSE, "BAM record " + std::to_string(w.n_records) + ": block_size " + std::to_string(bs) + " < 32");
        if (n - at - 4 < bs) break;
        const int32_t ref = (int32_t)le32(data + at + 4);
        if (ref < -1 || ref >= n_ref)
            return fail(GTARS_ERR_PARSE, "BAM record " + std::to_string(w.n_records) + ": refID " + std::to_string(ref) + " is not in the header");
        if (ref != w.last_ref) {
            if (w.last_ref == -1 || (ref != -1 && ref < w.last_ref))
                return fail(GTARS_ERR_PARSE, "BAM record " + std::to_string(w.n_records) + ": refID " + std::to_string(ref) + " follows refID " +
                                                 std::to_string(w.last_ref) + ": only coordinate-sorted BAM files are read");
            w.last_ref = ref;
        }
        if (segs && (segs->ref.empty() || segs->ref.back() != ref)) segs->start.push_back((uint32_t)k), segs->ref.push_back(ref);
        ++k;
        if (offs32) offs32->push_back((uint32_t)(base + at));
        if (offs64) offs64->push_back(base + at);
        ++w.n_records;
        at += 4 + bs;
    }
    if (final && at < n)
        return fail(GTARS_ERR_PARSE, "BAM record " + std::to_string(w.n_records) + " runs past the end of the data (" + std::to_string(n - at) +
                                         " bytes left)");
    *consumed = at;
    return GTARS_OK;
}

}  // namespace gtars
