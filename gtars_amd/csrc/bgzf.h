// bgzf.h -- the BGZF framing (SAM/BAM specification section 4.1): a gzip file whose members carry their own compressed size in a
// "BC" subfield of the extra field and inflate to at most 64 KiB.  ONE parser of a member's frame for the BAM reader (bam.cpp:
// block_table, which turns a refusal into its message) and for the fragment pipeline's loader (host.cpp: bgzf_member_table, for
// which a refusal means "not BGZF: the file goes through the ordinary gzip reader").  Nothing is decoded.  Plain C++.
#pragma once

#include <cstdint>

namespace gtars {

constexpr uint32_t BGZF_MAX_ISIZE = 65536;

// One BGZF block: where it lies in the file, what its trailer promises, and where its bytes go in the inflated stream.  The
// table is what a device decoder needs: thousands of independent members of <= 64 KiB with both sizes known before a byte is
// decoded.
struct BamBlock {
    uint64_t coff;   // of the member's first byte in the file
    uint32_t csize;  // BSIZE + 1: the whole member
    uint32_t doff;   // of the raw deflate stream inside the member (behind the gzip header)
    uint32_t isize;  // inflated bytes (trailer), <= BGZF_MAX_ISIZE
    uint32_t crc;    // CRC-32 of the inflated bytes (trailer)
    uint64_t uoff;   // prefix sum of isize: the block's first byte in the inflated stream
};

// why the bytes at `at` are not a BGZF member (in the order the checks are made)
enum class BgzfFrame { ok, truncated, no_magic, flags, extra_past_end, no_bc, past_end, bsize_small, isize_large };

inline uint32_t bgzf_le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t bgzf_le32(const uint8_t *p) { return bgzf_le16(p) | (bgzf_le16(p + 2) << 16); }

// the member that starts at p[at] of a file of n bytes -> b (uoff as given); the next member starts at at + b.csize.
// *bsize: the BC subfield's value, once it has been read (for the caller's message).
inline BgzfFrame bgzf_member_at(const uint8_t *p, uint64_t n, uint64_t at, uint64_t uoff, BamBlock &b, uint64_t *bsize) {
    if (n - at < 18) return BgzfFrame::truncated;
    if (p[at] != 0x1f || p[at + 1] != 0x8b || p[at + 2] != 8) return BgzfFrame::no_magic;
    if (p[at + 3] != 4) return BgzfFrame::flags;  // FEXTRA and nothing else
    const uint64_t xlen = bgzf_le16(p + at + 10), x0 = at + 12, x1 = x0 + xlen;
    if (x1 + 8 > n) return BgzfFrame::extra_past_end;
    bool have = false;
    for (uint64_t x = x0; x + 4 <= x1;) {
        const uint64_t slen = bgzf_le16(p + x + 2);
        if (p[x] == 'B' && p[x + 1] == 'C' && slen == 2 && x + 6 <= x1) {
            *bsize = bgzf_le16(p + x + 4);
            have = true;
            break;
        }
        x += 4 + slen;
    }
    if (!have) return BgzfFrame::no_bc;
    const uint64_t csize = *bsize + 1, doff = 12 + xlen;
    if (at + csize > n) return BgzfFrame::past_end;
    if (csize < doff + 8) return BgzfFrame::bsize_small;
    const uint32_t isize = bgzf_le32(p + at + csize - 4);
    if (isize > BGZF_MAX_ISIZE) return BgzfFrame::isize_large;
    b = BamBlock{at, (uint32_t)csize, (uint32_t)doff, isize, bgzf_le32(p + at + csize - 8), uoff};
    return BgzfFrame::ok;
}

}  // namespace gtars
