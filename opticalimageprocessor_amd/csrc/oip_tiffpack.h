// oip_tiffpack.h -- what the two device encoders of TIFF streams (tifflzw.hip, tiffdeflate.hip) do after their coders: the streams
// lie in fixed slots of the scratch and are packed behind one another into the payload, at even offsets as the host writers place them.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace {

// stream k of this launch: slot -> payload + off[k] (even), (len + 1) / 2 two-byte units; an odd length's pad byte is zero
__global__ __launch_bounds__(256) void tiff_pack_kernel(const uint8_t *__restrict__ slots, size_t slot_bytes, const unsigned *__restrict__ len,
                                                        const unsigned long long *__restrict__ off, long strip0, long nstrips,
                                                        uint8_t *__restrict__ payload)
{
    const long k = strip0 + blockIdx.x;
    if (k >= nstrips) return;
    const unsigned n = len[k];
    const uint16_t *src = reinterpret_cast<const uint16_t *>(slots + (size_t)blockIdx.x * slot_bytes);
    uint16_t *dst = reinterpret_cast<uint16_t *>(payload + off[k]);
    const unsigned units = (n + 1) / 2;
    for (unsigned i = threadIdx.x; i < units; i += 256) {
        uint16_t v = src[i];
        if (2 * i + 1 >= n) v &= 0x00ffu;
        dst[i] = v;
    }
}

}  // namespace
