// refget.h -- internal interface of refget.hip (K21: sequence digests and substrings of a sequence collection whose packed
// image is resident on the device; gtars-refget/src/digest, store/readonly.rs) for the host layer.
// Plain C++: refget.cpp includes it without the HIP headers.
#pragma once

#include <cstdint>
#include <functional>
#include <vector>

#include "refget_core.h"
#include "seqstats.h"

namespace gtars {

// sha512t24u, MD5 and alphabet class of EVERY row of an image (refget_hash, refget_core.h), n = the image's rows.  The
// result columns are device memory of the image's device (on_device) or host memory; each may be null.
struct RefgetDigestCall {
    uint64_t n = 0;
    bool on_device = false;
    void *stream = nullptr;   // on_device only
    char *digest = nullptr;   // n * 32 characters, 8-byte aligned when on the device
    uint8_t *md5 = nullptr;   // n * 16 bytes, 8-byte aligned when on the device
    uint8_t *cls = nullptr;   // n
    // HOST, for the rows longer than GTARS_REFGET_HOST_LEN (the host tail): the rows' bytes and lengths, threads
    const uint8_t *const *h_seq = nullptr;
    const uint64_t *h_len = nullptr;
    unsigned threads = 1;
    // runs on the calling thread once the kernel is queued, before the stream is drained (may be empty)
    std::function<void()> meanwhile;
};
gtars_status refget_digest_run(const Assembly &a, const RefgetDigestCall &call);

// One batch of substrings [start, end) of rows of an image (refget_sub_status, refget_core.h): per row a status and, for
// status 0, its bytes upper-cased, as a byte CSR.  seq: the image's row, RG_NONE for a sequence the collection lacks.
struct RefgetSubCall {
    const uint32_t *seq = nullptr;
    const uint64_t *start = nullptr, *end = nullptr;
    uint64_t n = 0;
    bool on_device = false;
    void *stream = nullptr;
    uint8_t *status = nullptr;
    // host callers: the CSR as vectors
    std::vector<uint64_t> *off = nullptr;
    std::vector<uint8_t> *bytes = nullptr;
    // device callers: n + 1 offsets and a byte column of `cap` bytes (8-byte aligned); *total is set on the host, and a
    // total above cap is GTARS_ERR_CAPACITY ("need N") with nothing written to d_bytes
    uint64_t *d_off = nullptr;
    uint8_t *d_bytes = nullptr;
    uint64_t cap = 0, *total = nullptr;
};
gtars_status refget_sub_run(const Assembly &a, const RefgetSubCall &call);

// The same call over any image whose rows have the device column len[n_seq] on `device` (K22's packed image, refget_pack.hip):
// statuses, counts and offsets as above; `fill` queues the launch that writes out[0, total) from the device columns seq /
// start (the call's rows) and the scanned offsets off[0 .. n].
using RefgetFill = std::function<gtars_status(const uint32_t *seq, const uint64_t *start, const uint64_t *off, uint32_t n, uint64_t total,
                                              uint8_t *out, void *stream)>;
gtars_status refget_sub_run_over(const uint64_t *d_len, uint32_t n_seq, int device, const RefgetSubCall &call, const RefgetFill &fill);

// the configured GTARS_REFGET_HOST_LEN: rows longer than this are hashed on the host threads
uint32_t refget_host_len();

}  // namespace gtars
