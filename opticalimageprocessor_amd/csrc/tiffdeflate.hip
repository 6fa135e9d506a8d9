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
#include "oip_internal.h"
#include "oip_inflate.h"
#include "oip_tiffdecode.h"

#include <cstdint>
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
    const long r0 = k * j.rps;
    long nr = j.rows - r0;
    if (nr > j.rps) nr = j.rps;
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

// four 16-bit adds in one register: the low 15 bits of every field carry on their own, the top bits by xor (as tifflzw.hip)
__device__ __forceinline__ unsigned long long padd16(unsigned long long a, unsigned long long b)
{
    const unsigned long long m = 0x7fff7fff7fff7fffull;
    return ((a & m) + (b & m)) ^ ((a ^ b) & ~m);
}

// Predictor 2 undone: a wave per row, 64 pixels a round, an inclusive scan across the lanes plus the carry of the rounds before.
// FIELDS = 4: a pixel is four samples in one 64-bit word; 1: one sample.  Rows of a stream that failed are left as they are.
template <int FIELDS>
__global__ __launch_bounds__(64) void deflate_unpredict_kernel(uint16_t *img, long rows, int width, long rps, const unsigned *got, const int *status)
{
    const long r = blockIdx.x;
    if (r >= rows) return;
    const long k = r / rps;
    const long nr = rows - k * rps < rps ? rows - k * rps : rps;
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
    const long nr = rows - k * rps < rps ? rows - k * rps : rps;
    if (status[k] != 0 || (size_t)got[k] != (size_t)nr * width * spp * 2) return;
    uint16_t *row = img + (size_t)r * width * spp + threadIdx.x;
    unsigned prev = row[0];
    for (long x = 1; x < width; ++x) { prev = (prev + row[x * spp]) & 0xffffu; row[x * spp] = (uint16_t)prev; }
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
    return oip_tiff_decode(ctx, "oip_tiff_deflate_decode_u16", "Deflate", oipinflate::status_text, oipinflate::kMaxStream, 0, d_file, file_bytes, strip_off,
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
