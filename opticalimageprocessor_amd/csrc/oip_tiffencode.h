// oip_tiffencode.h -- what the two device encoders of TIFF streams (oip_tiff_lzw_strips_u16 in tifflzw.hip,
// oip_tiff_deflate_strips_u16 in tiffdeflate.hip) do around their coder kernels, the mirror of oip_tiffdecode.h: the argument
// checks, the call's own or the caller's scratch, launch by launch the coder into fixed slots, the lengths coming down, the offsets
// going up and the streams packed behind one another into the payload, at even offsets as the host writers place them.
#pragma once

#include "oip_internal.h"
#include "oip_tiffstreams.h"

#include <cstdint>
#include <vector>

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

// the scratch of one call (plan_tiff_encode, oip_tiffstreams.h), as the kernels see it
struct OipTiffSlots {
    void *tables;                                // the codec's, for the streams of one launch
    uint8_t *slots;                              // stream i of a launch: slots + i * slot_bytes
    size_t slot_bytes;
    long nstrips;                                // of the image
    unsigned *len;                               // [nstrips] what the coder wrote; indexed by the stream's number in the image
    size_t launch_bytes;                         // tables and slots: what a launch writes, from `tables` on
};

// fn: the entry point, for its messages; launch(s0, ns, OipTiffSlots): the codec's coder for streams [s0, s0 + ns) on ctx->stream,
// under the codec's encode scope; OIP_OK or what oip_fail returned
template <typename Launch>
inline int oip_tiff_encode(oip_ctx *ctx, const char *fn, const OipTiffCodec &codec, const uint16_t *d_img, long rows, int width, int spp, long rows_per_strip,
                           uint8_t *d_payload, size_t payload_cap, uint64_t *strip_off, uint64_t *strip_len, size_t *payload_bytes, void *d_scratch,
                           size_t scratch_bytes, Launch launch)
{
    if (!d_img || !d_payload || !strip_off || !strip_len || !payload_bytes) return oip_fail(ctx, OIP_E_INVALID, "%s: bad argument", fn);
    const OipTiffEncodePlan p = plan_tiff_encode(codec, rows, width, spp, rows_per_strip);
    if (p.refusal) return oip_fail(ctx, OIP_E_INVALID, "%s: %s", fn, p.refusal);
    const int align = spp == 4 ? codec.image_align4 : codec.image_align;
    if (((uintptr_t)d_img) & (uintptr_t)(align - 1)) return oip_fail(ctx, OIP_E_INVALID, "%s: image not %d-byte aligned", fn, align);
    if ((((uintptr_t)d_payload) & 1)) return oip_fail(ctx, OIP_E_INVALID, "%s: payload not 2-byte aligned", fn);
    if (payload_cap < p.worst_bytes) return oip_fail(ctx, OIP_E_INVALID, "%s: payload buffer too small", fn);
    OipDeviceBlock own;                          // scratch of this call's own when the caller brought none
    if (d_scratch) {
        if (scratch_bytes < p.scratch_bytes || (((uintptr_t)d_scratch) & 7)) return oip_fail(ctx, OIP_E_INVALID, "%s: scratch too small or misaligned", fn);
    } else {
        OIP_HIP(ctx, own.alloc(p.scratch_bytes));
        d_scratch = own.p;
    }
    const OipTiffSlots t{(char *)d_scratch + p.o_tables, reinterpret_cast<uint8_t *>((char *)d_scratch + p.o_slots), p.slot_bytes,
                         p.nstrips, reinterpret_cast<unsigned *>((char *)d_scratch + p.o_len), p.o_len};
    unsigned long long *d_off = reinterpret_cast<unsigned long long *>((char *)d_scratch + p.o_off);
    std::vector<unsigned> len((size_t)p.nstrips);
    std::vector<unsigned long long> off((size_t)p.nstrips);
    size_t pos = 0;
    for (long s0 = 0; s0 < p.nstrips; s0 += p.per_launch) {
        const long ns = p.nstrips - s0 < p.per_launch ? p.nstrips - s0 : p.per_launch;
        const int rc = launch(s0, ns, t);
        if (rc != OIP_OK) return rc;
        OIP_HIP(ctx, hipGetLastError());
        OIP_HIP(ctx, hipMemcpyAsync(len.data() + s0, t.len + s0, (size_t)ns * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
        OIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (long k = s0; k < s0 + ns; ++k)      // (LZW: cannot fire -- its shortest stream is 5 bytes and the slot is its worst case)
            if (len[(size_t)k] == 0 || len[(size_t)k] > p.slot_bytes) return oip_fail(ctx, OIP_E_RUNTIME, "%s: strip %ld was not encoded", fn, k);
        pos = place_streams(len.data() + s0, (size_t)ns, pos, off.data() + s0);
        if (((pos + 1) & ~(size_t)1) > payload_cap) return oip_fail(ctx, OIP_E_INVALID, "%s: payload buffer too small", fn);
        OIP_HIP(ctx, hipMemcpyAsync(d_off + s0, off.data() + s0, (size_t)ns * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
        {
            OipProfScope prof(ctx, codec.pack_scope);
            hipLaunchKernelGGL(tiff_pack_kernel, dim3((unsigned)ns), dim3(256), 0, ctx->stream, t.slots, p.slot_bytes, t.len, d_off, s0, p.nstrips, d_payload);
        }
        OIP_HIP(ctx, hipGetLastError());
        OIP_HIP(ctx, hipStreamSynchronize(ctx->stream));                          // the slots and off[] are reused by the next launch
    }
    for (long k = 0; k < p.nstrips; ++k) { strip_off[k] = off[(size_t)k]; strip_len[k] = len[(size_t)k]; }
    *payload_bytes = pos;
    return OIP_OK;
}
