// oip_tiffdecode.h -- what the two device decoders of TIFF streams (oip_tiff_lzw_decode_u16 in tifflzw.hip,
// oip_tiff_deflate_decode_u16 in tiffdeflate.hip) do around their kernels: the argument checks, the per-call device scratch with
// the streams' offsets and lengths going up and what they decoded to coming down, and the verdict strip by strip.
#pragma once

#include "oip_internal.h"
#include "oip_tiffstreams.h"

#include <cstdint>
#include <vector>

// the scratch of one call (tiff_decode_layout, oip_tiffstreams.h), as the kernels see it
struct OipTiffStreams {
    void *tables;
    const unsigned long long *off, *len;         // [nstrips] stream offsets inside the file buffer, byte counts
    unsigned *got;                               // [nstrips] bytes a stream decoded to
    int *status;                                 // [nstrips] 0, or the codec's reason
};

// predictor 2 of 4-sample pixels, both decoders: four 16-bit adds in one register -- the low 15 bits of every field carry on their
// own, the top bits by xor
__device__ __forceinline__ unsigned long long padd16(unsigned long long a, unsigned long long b)
{
    const unsigned long long m = 0x7fff7fff7fff7fffull;
    return ((a & m) + (b & m)) ^ ((a ^ b) & ~m);
}

// fn: the entry point, for its messages; limit: a stream and what it decodes to are smaller than this; launch(OipTiffStreams): the
// codec's kernels on ctx->stream; codec, reason(status): the words for a stream the kernels refused
template <typename Launch>
inline int oip_tiff_decode(oip_ctx *ctx, const char *fn, const char *codec, const char *(*reason)(int), uint64_t limit, size_t table_bytes,
                           const uint8_t *d_file, size_t file_bytes, const uint64_t *strip_off, const uint64_t *strip_len, long nstrips, long rows,
                           int width, int spp, long rows_per_strip, int predictor, const uint16_t *d_img, Launch launch)
{
    if (!d_file || !strip_off || !strip_len || !d_img || nstrips <= 0 || rows <= 0 || width <= 0 || spp <= 0 || spp > 16 || rows_per_strip <= 0 ||
        (predictor != 1 && predictor != 2))
        return oip_fail(ctx, OIP_E_INVALID, "%s: bad argument", fn);
    if (nstrips != (rows + rows_per_strip - 1) / rows_per_strip) return oip_fail(ctx, OIP_E_INVALID, "%s: strip count does not match RowsPerStrip", fn);
    const size_t rowBytes = (size_t)width * spp * 2;
    if ((size_t)rows_per_strip * rowBytes >= limit) return oip_fail(ctx, OIP_E_INVALID, "%s: strip of 4 GiB or more", fn);
    if (spp == 4 && predictor == 2 && (((uintptr_t)d_img) & 7)) return oip_fail(ctx, OIP_E_INVALID, "%s: image not 8-byte aligned", fn);
    for (long k = 0; k < nstrips; ++k)
        if (strip_off[k] > file_bytes || strip_len[k] > file_bytes - strip_off[k] || strip_len[k] >= limit)
            return oip_fail(ctx, OIP_E_INVALID, "%s: strip %ld outside the buffer", fn, k);
    const OipTiffDecodeLayout l = tiff_decode_layout(table_bytes, (size_t)nstrips);
    OipDeviceBlock scratch;
    OIP_HIP(ctx, scratch.alloc(l.bytes));
    unsigned long long *d_off = reinterpret_cast<unsigned long long *>((char *)scratch.p + l.o_off);
    unsigned long long *d_len = reinterpret_cast<unsigned long long *>((char *)scratch.p + l.o_len);
    unsigned *d_got = reinterpret_cast<unsigned *>((char *)scratch.p + l.o_got);
    int *d_status = reinterpret_cast<int *>((char *)scratch.p + l.o_status);
    static_assert(sizeof(uint64_t) == sizeof(unsigned long long), "strip tables are copied as they are");
    if (hipMemcpyAsync(d_off, strip_off, (size_t)nstrips * 8, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(d_len, strip_len, (size_t)nstrips * 8, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
        return oip_fail(ctx, OIP_E_DEVICE, "%s: copying the strip tables failed", fn);
    launch(OipTiffStreams{scratch.p, d_off, d_len, d_got, d_status});
    std::vector<unsigned> got((size_t)nstrips);
    std::vector<int> status((size_t)nstrips);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(got.data(), d_got, (size_t)nstrips * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(status.data(), d_status, (size_t)nstrips * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess)
        return oip_fail(ctx, OIP_E_DEVICE, "%s: decoding failed on the device", fn);
    for (long k = 0; k < nstrips; ++k) {
        const size_t want = (size_t)tiff_strip_span(k, rows, rows_per_strip).nr * rowBytes;
        if (status[(size_t)k] != 0) return oip_fail(ctx, OIP_E_RUNTIME, "corrupt %s stream (%s) in strip %ld", codec, reason(status[(size_t)k]), k);
        if (got[(size_t)k] != want) return oip_fail(ctx, OIP_E_RUNTIME, "strip %ld decodes to %u bytes, %zu expected", k, got[(size_t)k], want);
    }
    return OIP_OK;
}
