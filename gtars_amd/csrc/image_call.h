// image_call.h -- the frame of one call over the packed genome image (seqstats.hip, vrs.hip, reftx.hip, hgvs.hip).  Such a
// call comes in two forms: host columns, run on the image's device on the null stream, or the caller's device columns and
// stream, which must belong to the image's device (the entry checks that with require_handle_device, in its own order of
// argument checks, before it builds the frame).
#pragma once

#include "common.h"
#include "seqstats.h"

namespace gtars {

struct ImageCall {
    const bool dev;     // the caller's columns are device memory
    DeviceScope scope;  // (before the frame: the frame drains before the device is put back); the entry checks scope.st
    StreamFrame fr;
    ImageCall(const AssemblyParts &ap, bool on_device, void *stream)
        : dev(on_device), scope(on_device ? -1 : ap.device), fr(on_device ? (hipStream_t)stream : nullptr) {}

    // an input column: the caller's pointer when it is device memory (or null: an optional column), an upload otherwise
    template <class T>
    gtars_status in(const T *src, size_t n, const T **d) {
        if (dev || !src) {
            *d = src;
            return GTARS_OK;
        }
        T *up;
        GT_TRY(fr.upload(&up, src, n));
        *d = up;
        return GTARS_OK;
    }
    // a result column: the caller's device column where it gave one, one of the frame's otherwise ...
    template <class T>
    gtars_status out(T *given, size_t n, T **col) {
        if (dev && given) {
            *col = given;
            return GTARS_OK;
        }
        return fr.alloc(col, n);
    }
    // ... which a host caller that asked for the column gets back (queued: valid after the frame's drain)
    template <class T>
    gtars_status back(T *given, const T *col, size_t n) {
        return !dev && given ? fr.download(given, col, n) : GTARS_OK;
    }
    // the digest column: 32 text bytes per row for the caller, four u64 per row for the kernels
    gtars_status digests_out(char *given, size_t n, u64 **col) { return out((u64 *)given, 4 * n, col); }
    gtars_status digests_back(char *given, const u64 *col, size_t n) { return back(given, (const char *)col, 32 * n); }
    // one pinned host word for a value the device hands back
    template <class T>
    gtars_status host_word(T **h) {
        *h = (T *)fr.host(sizeof(T));
        return *h ? GTARS_OK : fail(GTARS_ERR_INTERNAL, "out of host memory");
    }
};

// the kernels store a digest as u64: a device digest column must be 8-byte aligned (`entry`: the message's prefix)
inline gtars_status digests_aligned(const char *entry, bool on_device, const char *digest) {
    if (on_device && digest && ((uintptr_t)digest & 7))
        return fail(GTARS_ERR_INVALID_ARG, std::string(entry) + ": the device digests must be 8-byte aligned");
    return GTARS_OK;
}

}  // namespace gtars
