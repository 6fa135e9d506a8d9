// overview.hip -- the device side of `oip overviews` and `oip stitch --overviews`: one level of a reduced-resolution
// pyramid, the 2 x 2 average of a u16 strip or product that skips no data.  The reference has no counterpart (it leaves
// pyramids to gdaladdo); the siblings here are quicklook.hip and rrc.hip, whose layout the kernel follows.
//
//   level k, sample (y, x, c):  the up-to-four samples (2y + j, 2x + i, c), j, i in {0, 1}, of level k - 1 that lie inside it;
//                               n: those with v >= valid_min, S: their sum;  q = n == 0 ? 0 : (S + n / 2) / n
//
// Exact integers, so any evaluation order gives the same bytes; with valid_min = 0 a full block is (S + 2) >> 2; every output
// is 0 or >= valid_min (a mean of values >= valid_min), so data never becomes no data and no data appears only where all
// inputs were no data.  A level is defined from the level above it, as gdaladdo -r average does it, NOT from the image: the
// two differ by 1 DN on about a quarter of the samples.
//
// Layout / mapping.  HBM-bound: 2 B per source sample in, 0.5 B out.  A lane owns 16 bytes of two consecutive lines -- 8
// columns at spp = 1, 2 pixels at spp = 4 -- and produces 4 output samples from them (4 columns, or the 4 channels of one
// pixel: sample 4 * lane + j of the output line either way), stored as one 8-byte word where the output allows it.  Two line
// pairs (four 16-byte loads) are in flight per lane.  The full-block case with valid_min = 0 divides by a shift; the others
// by their own n (a constant 3 at most).  All offsets are 64 bit: a strip has more than 2^31 samples.  grid.y cuts the lines
// into ranges that are multiples of 64 lines, so no 2 x 2 block is shared between workgroups: no atomics, and the result
// depends neither on the launch geometry nor on how the caller cuts the lines into calls (at even lines).
// A partial last lane still loads its 16 bytes: window start and pitch are multiples of 8 samples (host-checked), so they lie
// inside the line; the surplus samples never enter a sum.
//
// Anything the vector form cannot take (a pitch that is not a multiple of 8 samples, a window that does not start on a 16-byte
// boundary) goes to the lane-per-output-sample kernel: 2-byte loads, same result.
#include "oip_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kPairs = 2;                    // line pairs in flight per lane
constexpr int kRangeLines = 64;              // a workgroup's line range is a multiple of this (and so even)

// S and n of one output sample; e: the sample lies inside the level
__device__ __forceinline__ void take(unsigned v, bool e, unsigned vm, unsigned &S, unsigned &n)
{
    const bool ok = e && v >= vm;
    S += ok ? v : 0u;
    n += ok ? 1u : 0u;
}
__device__ __forceinline__ unsigned quotient(unsigned S, unsigned n)
{
    return n == 4 ? (S + 2) >> 2 : (n == 3 ? (S + 1) / 3u : (n == 2 ? (S + 1) >> 1 : S));      // n == 0: S == 0
}

template <int SPP, bool VM0>
__global__ __launch_bounds__(kBlock) void halve_u16_kernel(const uint16_t *__restrict__ src, long pitch, int w, long rows, unsigned vm,
                                                           uint16_t *__restrict__ dst, long dst_pitch, int dst_vec, long rows_per_block)
{
    const long lane = (long)blockIdx.x * kBlock + threadIdx.x;
    const long s0 = lane * 8;                                  // first sample of the lane in its line
    const long ns = (long)w * SPP;                             // samples of a line that belong to the image
    if (s0 >= ns) return;
    const int nlive = ns - s0 < 8 ? (int)(ns - s0) : 8;        // samples of the lane inside the line
    const int nout = SPP == 4 ? 4 : (nlive + 1) / 2;           // output samples of the lane
    const long r0 = (long)blockIdx.y * rows_per_block;
    long r1 = r0 + rows_per_block;
    if (r1 > rows) r1 = rows;

    // one output line of the lane from its 16 bytes of the two source lines
    auto emit = [&](uint4 top, uint4 bot, bool has_bot, uint16_t *o) {
        const unsigned tp[4] = {top.x, top.y, top.z, top.w}, bp[4] = {bot.x, bot.y, bot.z, bot.w};
        unsigned a[8], b[8], v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a[2 * i] = tp[i] & 0xffffu;
            a[2 * i + 1] = tp[i] >> 16;
            b[2 * i] = bp[i] & 0xffffu;
            b[2 * i + 1] = bp[i] >> 16;
        }
        if (VM0 && nlive == 8 && has_bot) {                    // full blocks, every sample counts
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i0 = SPP == 1 ? 2 * j : j, i1 = SPP == 1 ? 2 * j + 1 : j + 4;
                v[j] = (a[i0] + a[i1] + b[i0] + b[i1] + 2) >> 2;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i0 = SPP == 1 ? 2 * j : j, i1 = SPP == 1 ? 2 * j + 1 : j + 4;
                unsigned S = 0, n = 0;
                take(a[i0], i0 < nlive, vm, S, n);
                take(a[i1], i1 < nlive, vm, S, n);
                take(b[i0], has_bot && i0 < nlive, vm, S, n);
                take(b[i1], has_bot && i1 < nlive, vm, S, n);
                v[j] = quotient(S, n);
            }
        }
        if (dst_vec && nout == 4) {
            *reinterpret_cast<uint2 *>(o) = make_uint2(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nout) o[j] = (uint16_t)v[j];
        }
    };

    const uint16_t *s = src + r0 * pitch + s0;
    uint16_t *d = dst + (r0 / 2) * dst_pitch + lane * 4;
    long r = r0;
    for (; r + 2 * kPairs <= r1; r += 2 * kPairs) {
        uint4 q[2 * kPairs];
#pragma unroll
        for (int u = 0; u < 2 * kPairs; ++u) q[u] = *reinterpret_cast<const uint4 *>(s + u * pitch);
#pragma unroll
        for (int p = 0; p < kPairs; ++p) emit(q[2 * p], q[2 * p + 1], true, d + p * dst_pitch);
        s += 2 * kPairs * pitch;
        d += kPairs * dst_pitch;
    }
    for (; r < r1; r += 2) {                                   // the range's last lines: fewer than 2 * kPairs, the last one maybe alone
        const bool has_bot = r + 1 < r1;                       // (uniform over the grid row)
        const uint4 top = *reinterpret_cast<const uint4 *>(s);
        uint4 bot = make_uint4(0, 0, 0, 0);
        if (has_bot) bot = *reinterpret_cast<const uint4 *>(s + pitch);
        emit(top, bot, has_bot, d);
        s += 2 * pitch;
        d += dst_pitch;
    }
}

// any pitch / alignment: a lane owns one sample of the output line (channel c of column ox) and walks the line pairs of its range
__global__ __launch_bounds__(kBlock) void halve_u16_sample_kernel(const uint16_t *__restrict__ src, long pitch, int w, long rows, int spp,
                                                                  unsigned vm, uint16_t *__restrict__ dst, long dst_pitch, long rows_per_block)
{
    const long t = (long)blockIdx.x * kBlock + threadIdx.x;
    const long ow = (w + 1) / 2;
    if (t >= ow * spp) return;
    const long ox = t / spp, c = t - ox * spp;
    const bool has_right = 2 * ox + 1 < w;
    const long r0 = (long)blockIdx.y * rows_per_block;
    long r1 = r0 + rows_per_block;
    if (r1 > rows) r1 = rows;
    const uint16_t *s = src + r0 * pitch + 2 * ox * spp + c;
    uint16_t *d = dst + (r0 / 2) * dst_pitch + t;
    for (long r = r0; r < r1; r += 2) {
        const bool has_bot = r + 1 < r1;
        unsigned S = 0, n = 0;
        take(s[0], true, vm, S, n);
        if (has_right) take(s[spp], true, vm, S, n);
        if (has_bot) {
            take(s[pitch], true, vm, S, n);
            if (has_right) take(s[pitch + spp], true, vm, S, n);
        }
        *d = (uint16_t)quotient(S, n);
        s += 2 * pitch;
        d += dst_pitch;
    }
}

}  // namespace

extern "C" int oip_halve_u16(oip_ctx *ctx, const uint16_t *d_src, long src_pitch, int w, long rows, int spp, int valid_min, uint16_t *d_dst,
                             long dst_pitch)
{
    OIP_CHECK_CTX(ctx);
    if (w < 1 || rows < 0 || rows >= (1L << 31) || (spp != 1 && spp != 4) || (long)w * spp >= (1L << 31) || valid_min < 0 || valid_min > 65535 ||
        !d_src || !d_dst || d_dst == d_src || ((uintptr_t)d_src & 1) || ((uintptr_t)d_dst & 1))
        return oip_fail(ctx, OIP_E_INVALID, "oip_halve_u16: bad argument");
    const long ns = (long)w * spp, on = (long)((w + 1) / 2) * spp;
    if (src_pitch < ns || dst_pitch < on) return oip_fail(ctx, OIP_E_INVALID, "oip_halve_u16: a pitch is shorter than its line");
    if (rows == 0) return OIP_OK;
    // the vector form: 16-byte loads that stay inside the pitch
    const bool vec = src_pitch % 8 == 0 && ((uintptr_t)d_src & 15) == 0 && (ns + 7) / 8 * 8 <= src_pitch;
    OipProfScope prof(ctx, vec ? "halve_u16_kernel" : "halve_u16_sample_kernel");
    const unsigned vm = (unsigned)valid_min;
    long rpb;
    int gy;
    if (vec) {
        const int gx = (int)(((ns + 7) / 8 + kBlock - 1) / kBlock);
        oip_row_blocks(ctx, gx, rows, 8, kRangeLines, &rpb, &gy);
        const int dst_vec = dst_pitch % 4 == 0 && ((uintptr_t)d_dst & 7) == 0;          // 8-byte stores of 4 output samples
        const dim3 grid(gx, gy);
#define OIP_HALVE_LAUNCH(SPP, VM0)                                                                                                   \
    hipLaunchKernelGGL((halve_u16_kernel<SPP, VM0>), grid, dim3(kBlock), 0, ctx->stream, d_src, src_pitch, w, rows, vm, d_dst, dst_pitch, \
                       dst_vec, rpb)
        if (spp == 1) {
            if (vm == 0) OIP_HALVE_LAUNCH(1, true);
            else OIP_HALVE_LAUNCH(1, false);
        } else {
            if (vm == 0) OIP_HALVE_LAUNCH(4, true);
            else OIP_HALVE_LAUNCH(4, false);
        }
#undef OIP_HALVE_LAUNCH
    } else {
        const int gx = (int)((on + kBlock - 1) / kBlock);
        oip_row_blocks(ctx, gx, rows, 16, kRangeLines, &rpb, &gy);
        hipLaunchKernelGGL(halve_u16_sample_kernel, dim3(gx, gy), dim3(kBlock), 0, ctx->stream, d_src, src_pitch, w, rows, spp, vm, d_dst,
                           dst_pitch, rpb);
    }
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}
