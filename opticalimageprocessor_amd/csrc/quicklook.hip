// quicklook.hip -- the device side of `oip quicklook`: an F x F box decimation of a u16 strip or product (the one pass over
// the full-size raster), the histogram of a decimated plane and the 16 -> 8 bit look-up that writes the browse image.  The
// reference has no counterpart (it leaves looking at its products to other packages); the siblings here are colstats.hip and
// rrc.hip, whose layout the decimator follows.
//
//   q = (S + n / 2) / n      S: exact integer sum of the samples of one channel inside the image within an F x F block,
//                            n: their count (partial blocks at the right and bottom edges use their own n)
//
// Decimator, layout / mapping.  HBM-bound, read-only: 2 B per sample in, 2 / F^2 B out.  A lane owns 16 bytes of a line --
// 8 columns at spp = 1, 2 pixels at spp = 4 -- and sums them down the F lines of an output row in 32-bit registers (64 lines
// of 65535 fit), four 16-byte loads in flight.  The horizontal sum: at spp = 1, F <= 8 it stays in the lane (8 / F outputs
// per lane); otherwise the F * spp / 8 neighbouring lanes that share a block add up through xor shuffles (2, 4 or 8 lanes at
// spp = 1, up to 32 at spp = 4: always inside one wave, a block of 256 lanes starts on a multiple of every group size) and
// the group's first lane stores.  A full block divides by a shift; an edge block by its own n.  grid.y cuts the lines into
// ranges that are multiples of 64 lines, so no F x F block is shared between workgroups: no atomics, and the result depends
// neither on the launch geometry nor on how the caller cuts the lines into calls (at multiples of F).
// A partial last lane group still loads its 16 bytes: window start and pitch are multiples of 8 samples (host-checked), so
// they lie inside the line; the surplus columns are zeroed before the horizontal sum.
//
// Anything the vector form cannot take (a pitch that is not a multiple of 8 samples, a window that does not start on a
// 16-byte boundary: a BIL band of a 30000-sample line starts at byte 15000) goes to the block-per-lane kernel: 2-byte loads,
// a lane walks the F x F block of one output sample.
//
// Histogram.  Its input is a decimated plane (tens of Mpix at most), so it is not tuned to the roofline; what it must not do
// is serialise on one address.  Counts are privatised in LDS: a workgroup owns one half of the value range (32768 32-bit
// bins = 128 of the CU's 160 KB), grid.y = 2 covers both, and a lane adds a run of equal values with one LDS atomic.  A
// workgroup then adds its non-zero bins to d_hist with 64-bit vector atomics, consecutive lanes on consecutive addresses.
#include <algorithm>

#include "oip_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kRowsInFlight = 4;
constexpr int kRangeLines = 64;              // a workgroup's line range is a multiple of this (and so of every F)

template <int F> struct Log2 { static constexpr int v = 1 + Log2<F / 2>::v; };
template <> struct Log2<1> { static constexpr int v = 0; };

// one output sample from its block sum; cols x lines samples of the image lie in the block
template <int F>
__device__ __forceinline__ unsigned box_quotient(unsigned sum, int cols, int lines)
{
    if (cols == F && lines == F) return (sum + F * F / 2) >> (2 * Log2<F>::v);
    const unsigned n = (unsigned)(cols * lines);
    return (sum + n / 2) / n;
}

template <int F, int SPP>
__global__ __launch_bounds__(kBlock) void decimate_box_u16_kernel(const uint16_t *__restrict__ src, long pitch, int w, long rows,
                                                                  uint16_t *__restrict__ dst, long dst_pitch, size_t dst_plane,
                                                                  long rows_per_block)
{
    constexpr int G = F < kRowsInFlight ? kRowsInFlight : F;   // lines per step: G / F output rows
    constexpr int NO = G / F;
    constexpr int LG = F * SPP / 8 > 0 ? F * SPP / 8 : 1;      // lanes that share a block
    constexpr int NV = SPP == 4 ? 4 : (F < 8 ? 8 / F : 1);     // values a lane (group) stores per output row
    const int lane = blockIdx.x * kBlock + threadIdx.x;
    const long s0 = (long)lane * 8;                            // first sample of the lane in its line
    const long ns = (long)w * SPP;                             // samples of a line that belong to the image
    const bool live = s0 < ns;
    const long r0 = (long)blockIdx.y * rows_per_block;
    long r1 = r0 + rows_per_block;
    if (r1 > rows) r1 = rows;
    // where the lane's values go: at spp = 1 output columns ox .. ox + NV - 1, at spp = 4 column ox of planes 0 .. 3
    const int px0 = (int)(s0 / SPP);
    const int ox = px0 / F;
    const int ow = (w + F - 1) / F;
    const bool writer = (threadIdx.x & (LG - 1)) == 0;

    unsigned col[NO][8];
    auto clear = [&]() {
#pragma unroll
        for (int o = 0; o < NO; ++o)
#pragma unroll
            for (int i = 0; i < 8; ++i) col[o][i] = 0;
    };
    auto line = [&](uint4 q, int o) {
        const unsigned p[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            col[o][2 * i] += p[i] & 0xffffu;
            col[o][2 * i + 1] += p[i] >> 16;
        }
    };
    // output row `oy` of this call from col[o]; `lines` source lines went into it.  Every lane of the block comes here (shuffles).
    auto emit = [&](int o, long oy, int lines) {
        unsigned v[NV];
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (s0 + i >= ns) col[o][i] = 0;                   // surplus columns of the last lane group
        if (SPP == 4) {
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = col[o][c] + col[o][4 + c];
        } else {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                v[j] = 0;
#pragma unroll
                for (int i = 0; i < 8 / NV; ++i) v[j] += col[o][j * (8 / NV) + i];
            }
        }
#pragma unroll
        for (int m = 1; m < LG; m <<= 1)
#pragma unroll
            for (int j = 0; j < NV; ++j) v[j] += __shfl_xor(v[j], m);
        if (!writer) return;
        uint16_t *d = dst + oy * dst_pitch;
        if (SPP == 4) {
            if (ox < ow) {
                const int cols = w - ox * F < F ? w - ox * F : F;
#pragma unroll
                for (int c = 0; c < 4; ++c) d[(size_t)c * dst_plane + ox] = (uint16_t)box_quotient<F>(v[c], cols, lines);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int x = ox + j;
                if (x < ow) {
                    const int cols = w - x * F < F ? w - x * F : F;
                    d[x] = (uint16_t)box_quotient<F>(v[j], cols, lines);
                }
            }
        }
    };

    const uint16_t *s = src + r0 * pitch + s0;
    long r = r0;
    for (; r + G <= r1; r += G) {
        clear();
        if (live) {
            // four lines in flight and no more: unrolled or interleaved further the kernel passes 64 registers, and the resident
            // set of 8 workgroups per CU that the grid is cut for no longer fits
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
            for (int c = 0; c < G; c += kRowsInFlight) {
                uint4 q[kRowsInFlight];
#pragma unroll
                for (int u = 0; u < kRowsInFlight; ++u) q[u] = *reinterpret_cast<const uint4 *>(s + (c + u) * pitch);
#pragma unroll
                for (int u = 0; u < kRowsInFlight; ++u) line(q[u], NO == 1 ? 0 : u / F);      // NO > 1: G == kRowsInFlight, c == 0
            }
        }
        s += G * pitch;
#pragma unroll
        for (int o = 0; o < NO; ++o) emit(o, r / F + o, F);
    }
    if (r < r1) {                                              // the image's last lines: fewer than G of them
        clear();
        const int left = (int)(r1 - r);
        if (live)
            for (int u = 0; u < left; ++u) {
                const uint4 q = *reinterpret_cast<const uint4 *>(s + u * pitch);
#pragma unroll
                for (int o = 0; o < NO; ++o)
                    if (u / F == o) line(q, o);
            }
#pragma unroll
        for (int o = 0; o < NO; ++o) {
            const int lines = left - o * F < F ? left - o * F : F;
            if (lines > 0) emit(o, r / F + o, lines);          // (uniform over the block: every lane takes part or none)
        }
    }
}

// any pitch / alignment: a lane owns one output sample (column ox of plane c) of the row block
__global__ __launch_bounds__(kBlock) void decimate_box_u16_block_kernel(const uint16_t *__restrict__ src, long pitch, int w, long rows,
                                                                        int spp, int F, uint16_t *__restrict__ dst, long dst_pitch,
                                                                        size_t dst_plane, long rows_per_block)
{
    const int ow = (w + F - 1) / F;
    const int t = blockIdx.x * kBlock + threadIdx.x;           // t = c * ow + ox: a wave reads one channel of neighbouring blocks
    if (t >= ow * spp) return;
    const int c = t / ow, ox = t - c * ow;
    const int cols = w - ox * F < F ? w - ox * F : F;
    const long r0 = (long)blockIdx.y * rows_per_block;
    long r1 = r0 + rows_per_block;
    if (r1 > rows) r1 = rows;
    for (long r = r0; r < r1; r += F) {
        const int lines = r1 - r < F ? (int)(r1 - r) : F;
        const uint16_t *s = src + r * pitch + (long)ox * F * spp + c;
        unsigned sum = 0;
        for (int u = 0; u < lines; ++u) {
            for (int i = 0; i < cols; ++i) sum += s[(long)i * spp];
            s += pitch;
        }
        const unsigned n = (unsigned)(cols * lines);
        dst[(size_t)c * dst_plane + (r / F) * dst_pitch + ox] = (uint16_t)((sum + n / 2) / n);
    }
}

template <int SPP>
void launch_decimate(oip_ctx *ctx, int F, dim3 grid, const uint16_t *src, long pitch, int w, long rows, uint16_t *dst, long dst_pitch,
                     size_t dst_plane, long rpb)
{
#define OIP_DECIMATE_CASE(f)                                                                                                      \
    case f:                                                                                                                       \
        hipLaunchKernelGGL((decimate_box_u16_kernel<f, SPP>), grid, dim3(kBlock), 0, ctx->stream, src, pitch, w, rows, dst, dst_pitch, \
                           dst_plane, rpb);                                                                                       \
        break
    switch (F) {
        OIP_DECIMATE_CASE(2);
        OIP_DECIMATE_CASE(4);
        OIP_DECIMATE_CASE(8);
        OIP_DECIMATE_CASE(16);
        OIP_DECIMATE_CASE(32);
        OIP_DECIMATE_CASE(64);
    }
#undef OIP_DECIMATE_CASE
}

// ---- histogram ------------------------------------------------------------------------------------------------------
constexpr int kHistBlock = 1024;
constexpr int kHistHalf = 32768;             // bins of a workgroup: one half of the value range
constexpr int kHistSpan = 4 * kHistBlock;    // pixels of a line that a work item covers

// a work item: kHistSpan consecutive pixels of one line; workgroup b takes the items b, b + gridDim.x, ...
__global__ __launch_bounds__(kHistBlock) void histogram_u16_kernel(const uint16_t *__restrict__ img, long pitch, int w, long items,
                                                                   int spans, unsigned long long *__restrict__ hist)
{
    __shared__ unsigned bins[kHistHalf];
    const unsigned base = blockIdx.y * kHistHalf;
    for (int i = threadIdx.x; i < kHistHalf; i += kHistBlock) bins[i] = 0;
    __syncthreads();
    unsigned cur = 0, run = 0;               // a run of equal values of this lane, not yet added
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const long row = it / spans;
        const int x0 = (int)(it - row * spans) * kHistSpan;
        const uint16_t *s = img + row * pitch;
#pragma unroll
        for (int k = 0; k < kHistSpan / kHistBlock; ++k) {
            const int x = x0 + k * kHistBlock + threadIdx.x;
            if (x < w) {
                const unsigned v = s[x];
                if (v == cur) {
                    ++run;
                } else {
                    if (run && cur - base < (unsigned)kHistHalf) atomicAdd(&bins[cur - base], run);
                    cur = v;
                    run = 1;
                }
            }
        }
    }
    if (run && cur - base < (unsigned)kHistHalf) atomicAdd(&bins[cur - base], run);
    __syncthreads();
    for (int i = threadIdx.x; i < kHistHalf; i += kHistBlock) {
        const unsigned n = bins[i];
        if (n) atomicAdd(hist + base + i, (unsigned long long)n);
    }
}

// ---- 16 -> 8 bit look-up, planes -> interleaved -------------------------------------------------------------------------
struct LutPlanes { const uint16_t *p[3]; };

template <int NCH>
__global__ __launch_bounds__(kBlock) void apply_lut_u8_kernel(LutPlanes planes, long pitch, int w, long rows, const uint8_t *__restrict__ luts,
                                                              uint8_t *__restrict__ out)
{
    const int x = blockIdx.x * kBlock + threadIdx.x;
    if (x >= w) return;
    for (long r = blockIdx.y; r < rows; r += gridDim.y) {
        uint8_t *o = out + ((size_t)r * w + x) * NCH;
#pragma unroll
        for (int c = 0; c < NCH; ++c) o[c] = luts[c * 65536 + planes.p[c][r * pitch + x]];
    }
}

}  // namespace

extern "C" int oip_decimate_box_u16(oip_ctx *ctx, const uint16_t *d_src, long pitch, int w, long rows, int spp, int factor, uint16_t *d_dst,
                                    long dst_pitch, size_t dst_plane_stride)
{
    OIP_CHECK_CTX(ctx);
    const bool pow2 = factor == 2 || factor == 4 || factor == 8 || factor == 16 || factor == 32 || factor == 64;
    if (w <= 0 || rows < 0 || rows >= (1L << 31) || (spp != 1 && spp != 4) || !pow2 || (long)w * spp >= (1L << 31) || pitch < (long)w * spp || !d_src ||
        !d_dst || ((uintptr_t)d_src & 1) || ((uintptr_t)d_dst & 1))
        return oip_fail(ctx, OIP_E_INVALID, "oip_decimate_box_u16: bad argument");
    const int ow = (w + factor - 1) / factor;
    const long oh = (rows + factor - 1) / factor;
    if (dst_pitch < ow || (spp == 4 && oh > 0 && dst_plane_stride < (size_t)(oh - 1) * dst_pitch + ow))
        return oip_fail(ctx, OIP_E_INVALID, "oip_decimate_box_u16: output pitch or plane stride too small");
    if (rows == 0) return OIP_OK;
    const bool vec = pitch % 8 == 0 && ((uintptr_t)d_src & 15) == 0;
    OipProfScope prof(ctx, vec ? "decimate_box_u16_kernel" : "decimate_box_u16_block_kernel");
    long rpb;
    int gy;
    if (vec) {
        const int gx = (int)((((long)w * spp + 7) / 8 + kBlock - 1) / kBlock);
        oip_row_blocks(ctx, gx, rows, 8, kRangeLines, &rpb, &gy);
        if (spp == 1) launch_decimate<1>(ctx, factor, dim3(gx, gy), d_src, pitch, w, rows, d_dst, dst_pitch, dst_plane_stride, rpb);
        else launch_decimate<4>(ctx, factor, dim3(gx, gy), d_src, pitch, w, rows, d_dst, dst_pitch, dst_plane_stride, rpb);
    } else {
        const int gx = (ow * spp + kBlock - 1) / kBlock;
        oip_row_blocks(ctx, gx, rows, 16, kRangeLines, &rpb, &gy);
        hipLaunchKernelGGL(decimate_box_u16_block_kernel, dim3(gx, gy), dim3(kBlock), 0, ctx->stream, d_src, pitch, w, rows, spp, factor, d_dst,
                           dst_pitch, dst_plane_stride, rpb);
    }
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}

extern "C" int oip_histogram_u16(oip_ctx *ctx, const uint16_t *d_img, long pitch, int w, long rows, uint64_t *d_hist)
{
    OIP_CHECK_CTX(ctx);
    if (w <= 0 || rows < 0 || rows >= (1L << 31) || pitch < w || !d_img || !d_hist || ((uintptr_t)d_img & 1) || ((uintptr_t)d_hist & 7))
        return oip_fail(ctx, OIP_E_INVALID, "oip_histogram_u16: bad argument");
    if (rows == 0) return OIP_OK;
    const int spans = (w + kHistSpan - 1) / kHistSpan;
    const long items = rows * spans;
    // a workgroup's 32-bit bins hold its share of the pixels: at most 2^19 items of kHistSpan pixels = 2^31
    long gx = std::max<long>(ctx->cu_count, (items + (1L << 19) - 1) >> 19);
    if (gx > items) gx = items;
    OipProfScope prof(ctx, "histogram_u16_kernel");
    hipLaunchKernelGGL(histogram_u16_kernel, dim3((unsigned)gx, 2), dim3(kHistBlock), 0, ctx->stream, d_img, pitch, w, items, spans,
                       reinterpret_cast<unsigned long long *>(d_hist));
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}

extern "C" int oip_apply_lut_u8(oip_ctx *ctx, const uint16_t *const *d_planes, long pitch, int w, long rows, int nch, const uint8_t *d_luts,
                                uint8_t *d_out)
{
    OIP_CHECK_CTX(ctx);
    if (w <= 0 || rows < 0 || rows >= (1L << 31) || pitch < w || (nch != 1 && nch != 3) || !d_planes || !d_luts || !d_out)
        return oip_fail(ctx, OIP_E_INVALID, "oip_apply_lut_u8: bad argument");
    LutPlanes pl = {{nullptr, nullptr, nullptr}};
    for (int c = 0; c < nch; ++c) {
        if (!d_planes[c] || ((uintptr_t)d_planes[c] & 1)) return oip_fail(ctx, OIP_E_INVALID, "oip_apply_lut_u8: bad plane pointer");
        pl.p[c] = d_planes[c];
    }
    if (rows == 0) return OIP_OK;
    const dim3 grid((w + kBlock - 1) / kBlock, (unsigned)std::min<long>(rows, 4096));
    OipProfScope prof(ctx, "apply_lut_u8_kernel");
    if (nch == 1) hipLaunchKernelGGL(apply_lut_u8_kernel<1>, grid, dim3(kBlock), 0, ctx->stream, pl, pitch, w, rows, d_luts, d_out);
    else hipLaunchKernelGGL(apply_lut_u8_kernel<3>, grid, dim3(kBlock), 0, ctx->stream, pl, pitch, w, rows, d_luts, d_out);
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}
