// refget_pack.h -- internal interface of refget_pack.hip (K22: the bit-packed image of a sequence collection on the device,
// packed there from the raw image and read by the substring fill; gtars-refget/src/digest/encoder.rs, store/readonly.rs)
// for the host layer.  Plain C++: refget_store.cpp includes it without the HIP headers.
#pragma once

#include <cstdint>

#include "refget.h"
#include "refget_pack_core.h"

namespace gtars {

// The packed image on a device: ONE byte buffer -- record r at the 16-byte-aligned offset off[r], ceil(len[r] b / 8) bytes
// with b from cls[r], at least 16 zero bytes behind every record -- and the columns off / len / cls (rg_image_layout).
struct PackedImage;

// the image from its host copy (`bytes` of it, laid out by rg_image_layout), on the current device
gtars_status packed_upload(const uint8_t *image, uint64_t bytes, const uint64_t *off, const uint64_t *len, const uint8_t *cls, uint32_t n,
                           PackedImage **out);
// the image packed on the device of the raw image `raw` (K12's layout, n rows of len[r] bytes) by k_refget_pack; the host
// copy lands in image[0, bytes)
gtars_status packed_from_raw(const Assembly &raw, const uint64_t *off, const uint64_t *len, const uint8_t *cls, uint32_t n, uint64_t bytes,
                             uint8_t *image, PackedImage **out);
void packed_free(PackedImage *p);
int packed_device(const PackedImage *p);
uint64_t packed_device_bytes(const PackedImage *p);

// substrings of the image's records, decoded: RefgetSubCall as for the raw image (refget.h), the fill profiled as
// k_refget_fill_packed
gtars_status packed_sub_run(const PackedImage &p, const RefgetSubCall &call);

}  // namespace gtars
