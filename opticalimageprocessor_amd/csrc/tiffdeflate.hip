// tiffdeflate.hip -- the Deflate strips and tiles of a TIFF file (compression 8 / 32946) inflated on the GPU.
//
// The sibling of the LZW decoder in tifflzw.hip, behind the same reader (oip_host.hpp::read_tiff_to_device), with another shape:
// a lane of its own per strip does not carry over, because a decoder's Huffman tables plus its 32 KiB of history do not fit 64
// times into a CU.  Here a stream is a WAVE, in a single-wave workgroup:
//   - the history is a 32 KiB ring in LDS; matches read the ring, never the image in HBM;
//   - the Huffman tables (10-bit literal/length and 8-bit distance primaries, canonical counts for the longer codes) are in LDS
//     and rebuilt per dynamic block, the primaries by the 64 lanes;
//   - 2 KiB of input are staged in LDS at a time, loaded coalesced;
//   - every lane holds the same bit buffer and decodes the same symbol (table reads are broadcasts); lane 0 stores a literal, the
//     lanes copy a match together, and the ring goes to the image in 16-byte words whenever 16 KiB of it are new -- with the
//     Adler-32 of the bytes as they leave.
// About 38 KiB of LDS a workgroup: four resident waves per CU.  The decoder itself is csrc/oip_inflate.h, the code the host's
// threads run and the sanitizers have seen; this file gives it its lanes.  Predictor 2 is undone by a second kernel, a wave per
// image row (rows are independent; mod-2^16 sums in any order give the same bytes).
//
// The other direction, the Deflate strips and tiles of a product (oip_tiff_deflate_strips_u16, below the decoder): the encoder of
// csrc/oip_deflate.h with the same shape -- a stream is a wave in a single-wave workgroup.  The 32 KiB input ring, the 4096-entry
// hash table, the block's token record (two bits per position, a word per match), the histograms, the codes and the 512-byte
// bit buffer are LDS, about 66 KiB a workgroup: two resident waves per CU.  The lanes stage the input (the predictor-2
// differences of the image's rows, made while they are staged: the image is only read), hash and compare the 64 positions of a
// round, count the literals, rank the symbols by frequency, and place a block's codes by a prefix sum of their bit counts; one
// lane walks a round's 64 candidates and builds the code lengths.  Nothing of a stream is kept in HBM but its output: the streams
// land in fixed slots of the stored bound's size and oip_tiffencode.h packs them, as for LZW.
#include "oip_internal.h"
#include "oip_deflate.h"
#include "oip_inflate.h"
#include "oip_tiffdecode.h"
#include "oip_tiffencode.h"

#include <cstdint>
#include <memory>
#include <vector>

namespace {

constexpr long kStreamsPerLaunch = 1L << 20;

struct WaveLane {
    __device__ unsigned lane() const { return threadIdx.x; }
    __device__ unsigned nlanes() const { return 64; }
    __device__ void sync() const { __syncthreads(); }
    __device__ unsigned sum(unsigned v) const
    {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        return v;
    }
    __device__ unsigned uni(unsigned v) const { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }
};

struct DeflateJob {
    const uint8_t *file;
    const unsigned long long *off, *len;         // [nstrips]: stream offsets inside `file`, byte counts
    long rows;
    int width, spp;
    long rps, nstrips, strip0;
    uint16_t *img;
    unsigned *got;                               // [nstrips] bytes a stream decoded to
    int *status;                                 // [nstrips] oipinflate::Status
};

__global__ __launch_bounds__(64) void deflate_decode_kernel(DeflateJob j)
{
    __shared__ oipinflate::Shared sh;
    const long k = j.strip0 + blockIdx.x;
    if (k >= j.nstrips) return;
    const size_t rowBytes = (size_t)j.width * j.spp * 2;
    const OipStripSpan span = tiff_strip_span(k, j.rows, j.rps);
    const long r0 = span.r0, nr = span.nr;
    uint8_t *out = reinterpret_cast<uint8_t *>(j.img) + (size_t)r0 * rowBytes;
    const unsigned cap = (unsigned)((size_t)nr * rowBytes);
    WaveLane lanes;
    // (the stream's place and size are the same in every lane of the workgroup: scalar registers)
    const unsigned long long off = ((unsigned long long)lanes.uni((unsigned)(j.off[k] >> 32)) << 32) | lanes.uni((unsigned)j.off[k]);
    oipinflate::Decoder<WaveLane> d(lanes, sh, j.file + off, lanes.uni((unsigned)j.len[k]), out, cap);
    unsigned got = 0;
    const int st = d.run(&got);
    if (threadIdx.x == 0) { j.got[k] = got; j.status[k] = st; }
}

// Predictor 2 undone: a wave per row, 64 pixels a round, an inclusive scan (padd16, oip_tiffdecode.h) across the lanes plus the carry
// of the rounds before.
// FIELDS = 4: a pixel is four samples in one 64-bit word; 1: one sample.  Rows of a stream that failed are left as they are.
template <int FIELDS>
__global__ __launch_bounds__(64) void deflate_unpredict_kernel(uint16_t *img, long rows, int width, long rps, const unsigned *got, const int *status)
{
    const long r = blockIdx.x;
    if (r >= rows) return;
    const long k = r / rps;
    const long nr = tiff_strip_span(k, rows, rps).nr;
    if (status[k] != 0 || (size_t)got[k] != (size_t)nr * width * FIELDS * 2) return;
    uint16_t *row = img + (size_t)r * width * FIELDS;
    const int lane = threadIdx.x;
    unsigned long long carry = 0;
    for (int x0 = 0; x0 < width; x0 += 64) {
        const int x = x0 + lane;
        unsigned long long v = 0;
        if (x < width) v = FIELDS == 4 ? reinterpret_cast<const unsigned long long *>(row)[x] : (unsigned long long)row[x];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long t = __shfl_up(v, d, 64);
            if (lane >= d) v = padd16(v, t);
        }
        v = padd16(v, carry);
        if (x < width) {
            if (FIELDS == 4) reinterpret_cast<unsigned long long *>(row)[x] = v;
            else row[x] = (uint16_t)v;
        }
        carry = __shfl(v, 63, 64);                                             // (lanes past the row's end added zeros)
    }
}

// any other number of samples: lane c of the row's wave walks channel c
__global__ __launch_bounds__(64) void deflate_unpredict_any_kernel(uint16_t *img, long rows, int width, int spp, long rps, const unsigned *got, const int *status)
{
    const long r = blockIdx.x;
    if (r >= rows || (int)threadIdx.x >= spp) return;
    const long k = r / rps;
    const long nr = tiff_strip_span(k, rows, rps).nr;
    if (status[k] != 0 || (size_t)got[k] != (size_t)nr * width * spp * 2) return;
    uint16_t *row = img + (size_t)r * width * spp + threadIdx.x;
    unsigned prev = row[0];
    for (long x = 1; x < width; ++x) { prev = (prev + row[x * spp]) & 0xffffu; row[x * spp] = (uint16_t)prev; }
}

// ---- encode --------------------------------------------------------------------------------------------------------------------
struct WaveLaneEnc : WaveLane {
    __device__ unsigned scan(unsigned v) const                                 // exclusive prefix sum over the 64 lanes
    {
        unsigned s = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned t = __shfl_up(s, d, 64);
            if ((int)threadIdx.x >= d) s += t;
        }
        return s - v;
    }
    __device__ void amax(unsigned *p, unsigned v) const { atomicMax(p, v); }
    __device__ void inc(unsigned *p) const { atomicAdd(p, 1u); }
    __device__ void aor(unsigned *p, unsigned v) const { atomicOr(p, v); }
};

// byte i of a strip's stream: the little-endian bytes of (sample - the same channel of the previous pixel) mod 2^16, rows restarting
struct PredictorSource {
    const uint16_t *img;                         // the strip's first sample
    unsigned rowSamples, spp;
    __device__ unsigned at(unsigned i) const
    {
        const unsigned s = i >> 1;
        unsigned v = img[s];
        if (s % rowSamples >= spp) v -= img[s - spp];
        return (v >> (8 * (i & 1u))) & 255u;
    }
};

struct DeflateEncJob {
    const uint16_t *img;
    long rows;
    int width, spp;
    long rps, nstrips, strip0;
    uint8_t *slots;
    size_t slot_bytes;                           // >= stored_bound of a full strip
    unsigned *len;                               // [nstrips]; 0: the encoder refused (cannot happen with slots of the stored bound)
};

__global__ __launch_bounds__(64) void deflate_encode_kernel(DeflateEncJob j)
{
    extern __shared__ __align__(16) unsigned char lds[];
    oipdeflate::Shared &sh = *reinterpret_cast<oipdeflate::Shared *>(lds);
    const long k = j.strip0 + blockIdx.x;
    if (k >= j.nstrips) return;
    const size_t rowSamples = (size_t)j.width * j.spp;
    const OipStripSpan span = tiff_strip_span(k, j.rows, j.rps);
    const long r0 = span.r0, nr = span.nr;
    WaveLaneEnc lanes;
    const PredictorSource src{j.img + (size_t)r0 * rowSamples, (unsigned)rowSamples, (unsigned)j.spp};
    const unsigned n = (unsigned)((size_t)nr * rowSamples * 2);
    oipdeflate::Encoder<WaveLaneEnc, PredictorSource> e(lanes, sh, src, n, j.slots + (size_t)blockIdx.x * j.slot_bytes, (unsigned)oipdeflate::stored_bound(n));
    unsigned size = 0;
    const int st = e.run(&size);
    if (threadIdx.x == 0) j.len[k] = st == oipdeflate::kOk ? size : 0u;
}

}  // namespace

// (oip_tiff_decode's refusals and two of its own: the row kernels take a row per workgroup, so fewer than 2^31 rows, and address the
// image as u16 whatever the number of samples, so a 2-byte aligned image; the LZW decoder needs neither)
extern "C" int oip_tiff_deflate_decode_u16(oip_ctx *ctx, const uint8_t *d_file, size_t file_bytes, const uint64_t *strip_off,
                                           const uint64_t *strip_len, long nstrips, long rows, int width, int spp, long rows_per_strip,
                                           int predictor, uint16_t *d_img)
{
    OIP_CHECK_CTX(ctx);
    if (rows >= ((long)1 << 31)) return oip_fail(ctx, OIP_E_INVALID, "oip_tiff_deflate_decode_u16: 2^31 rows or more");
    if (((uintptr_t)d_img) & 1) return oip_fail(ctx, OIP_E_INVALID, "oip_tiff_deflate_decode_u16: image not 2-byte aligned");
    return oip_tiff_decode(ctx, "oip_tiff_deflate_decode_u16", kOipTiffDeflate.name, oipinflate::status_text, oipinflate::kMaxStream, 0, d_file, file_bytes, strip_off,
                           strip_len, nstrips, rows, width, spp, rows_per_strip, predictor, d_img, [&](const OipTiffStreams &t) {
        for (long s0 = 0; s0 < nstrips; s0 += kStreamsPerLaunch) {
            const long ns = nstrips - s0 < kStreamsPerLaunch ? nstrips - s0 : kStreamsPerLaunch;
            DeflateJob j{d_file, t.off, t.len, rows, width, spp, rows_per_strip, nstrips, s0, d_img, t.got, t.status};
            OipProfScope prof(ctx, "deflate_decode_kernel");
            hipLaunchKernelGGL(deflate_decode_kernel, dim3((unsigned)ns), dim3(64), 0, ctx->stream, j);
        }
        if (predictor == 2 && width > 1) {
            OipProfScope prof(ctx, "deflate_unpredict_kernel");
            if (spp == 4) hipLaunchKernelGGL(deflate_unpredict_kernel<4>, dim3((unsigned)rows), dim3(64), 0, ctx->stream, d_img, rows, width, rows_per_strip, t.got, t.status);
            else if (spp == 1) hipLaunchKernelGGL(deflate_unpredict_kernel<1>, dim3((unsigned)rows), dim3(64), 0, ctx->stream, d_img, rows, width, rows_per_strip, t.got, t.status);
            else hipLaunchKernelGGL(deflate_unpredict_any_kernel, dim3((unsigned)rows), dim3(64), 0, ctx->stream, d_img, rows, width, spp, rows_per_strip, t.got, t.status);
        }
    });
}

extern "C" size_t oip_deflate_stream_host(const uint8_t *src, size_t n, uint8_t *dst, size_t cap)
{
    if ((!src && n) || !dst) return 0;
    std::unique_ptr<oipdeflate::Shared> work(new oipdeflate::Shared);
    return oipdeflate::deflate_host(src, n, dst, cap, work.get());
}

extern "C" size_t oip_tiff_deflate_worst_bytes(long rows, int width, int spp, long rows_per_strip)
{
    return plan_tiff_encode(kOipTiffDeflate, rows, width, spp, rows_per_strip).worst_bytes;
}

extern "C" size_t oip_tiff_deflate_scratch_bytes(long rows, int width, int spp, long rows_per_strip)
{
    return plan_tiff_encode(kOipTiffDeflate, rows, width, spp, rows_per_strip).scratch_bytes;
}

extern "C" int oip_tiff_deflate_strips_u16(oip_ctx *ctx, const uint16_t *d_img, long rows, int width, int spp, long rows_per_strip,
                                           uint8_t *d_payload, size_t payload_cap, uint64_t *strip_off, uint64_t *strip_len,
                                           size_t *payload_bytes, void *d_scratch, size_t scratch_bytes)
{
    OIP_CHECK_CTX(ctx);
    return oip_tiff_encode(ctx, "oip_tiff_deflate_strips_u16", kOipTiffDeflate, d_img, rows, width, spp, rows_per_strip, d_payload, payload_cap, strip_off,
                           strip_len, payload_bytes, d_scratch, scratch_bytes, [&](long s0, long ns, const OipTiffSlots &t) {
        const size_t lds = sizeof(oipdeflate::Shared);
        static_assert(sizeof(oipdeflate::Shared) <= 80 * 1024, "two workgroups of the encoder per CU");
        // (above the 64 KiB a kernel gets without it; once a call, as before the launches of a call had one driver)
        if (s0 == 0) OIP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(deflate_encode_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        DeflateEncJob j{d_img, rows, width, spp, rows_per_strip, t.nstrips, s0, t.slots, t.slot_bytes, t.len};
        OipProfScope prof(ctx, kOipTiffDeflate.encode_scope);
        hipLaunchKernelGGL(deflate_encode_kernel, dim3((unsigned)ns), dim3(64), lds, ctx->stream, j);
        return (int)OIP_OK;
    });
}
