// seam.hip -- seam balancing and feathering of the strip stitch on gfx950 (`oip stitch --balance / --feather`).  The
// reference has no counterpart: IMO::StitchBigRaw (imageop.h:340-351) cuts hard at the seam, and stitch.hip restates that.
//
// After prestitch the last 2*fold columns of image 1 and the first 2*fold columns of image 2 see the same ground.  Lines are
// handled in SAMPLE units as StitchTiff does (Ws = W*spp, fs = fold*spp; the channel of sample index j is j % spp), and an
// overlap pair is  a = left[r][Ws - 2fs + j],  b = right[r][j],  j in [0, 2fs).
//
//   oip_seam_moments_u16     per channel  n, Sa, Sb, Saa, Sbb, Sab  over the pairs whose two samples are both valid,
//                            exact integers ADDED into a (6, spp) uint64 array
//   oip_stitch_balanced_u16  the stitch with image 2 balanced (b' = (G b + O) in Q16), a linear blend of half-width h pixels
//                            around the seam and "no data" (a sample below valid_min) handled inside it
//   oip_seam_moments_blocks_u16    the totals per block of B lines, (nb, 6, spp), all blocks in one launch   } `--balance-lines`:
//   oip_stitch_balanced_lines_u16  the balanced stitch with a (G, O) per line and channel from tables in HBM } see their kernels
//
// Moments: layout / mapping.  The overlap is a few hundred samples wide and as tall as the strip, so a lane owns ONE overlap
// sample j and walks lines: the 64 lanes of a wave read 128 contiguous bytes of a line of either image, the four waves of a
// block take every fourth line of the block's line range, four lines in flight per wave.  Both windows start wherever
// Ws - 2fs and the line pitch put them -- in general on a 2-byte boundary only, a different one on every line when Ws is
// odd -- so the loads are 2-byte loads and no alignment case exists.  (The pass reads 2*2fs of the 2*Ws samples per line the
// stitch moves: about 1 % of its bytes at the product geometries.)  A lane's channel is j % spp = lane % spp (64 % spp == 0),
// a loop constant.  A lane sees at most 65536 lines per launch, so n, Sa and Sb of a lane fit 32 bits; the three
// products need 64 (`S += (uint64_t)(x * y)` on the exact 32-bit product, the form colstats.hip settled on).
// Reduction: xor shuffles over the lanes of a wave that share a channel, the four waves through LDS, then 6*spp 64-bit
// integer vector atomics per block (global_atomic_add_x2, no return) into d_acc: totals do not depend on the launch
// geometry and add over calls.  The line ranges are sized for about one resident set of blocks (8 per CU).
//
// Stitch: stitch_rows_kernel's structure.  A lane owns one aligned 16-byte store of the output (8 samples), reads are
// funnel-shifted for odd source alignment, 4 chunks in flight per lane.  With the output line a multiple of 8 samples a
// chunk starts at channel 0, so the lane's four (G, O) pairs are loop constants.  Three kinds of chunk:
//   left of the blend zone    copy of image 1                                   (as stitch_rows_kernel)
//   right of it               copy of image 2, one 64-bit multiply-add, a shift and a clamp per sample
//   touching it (or the seam) per sample: both images' samples, the blend's division        (2h*spp/8 + 2 chunks of a line at most)
// Anything the vector form cannot take (an output line that is not a multiple of 8 samples, misaligned bases, an odd sample
// count) goes to the per-sample kernel, as in oip_stitch_rows_u16.  With G = 65536, O = 0, h = 0 both kernels write
// oip_stitch_rows_u16's bytes.
#include "oip_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kRowsInFlight = 4;
constexpr long kMaxLaneRows = 65536;         // 65536 * 65535 < 2^32: n, Sa, Sb of a lane in 32 bits

// ---- moments -------------------------------------------------------------------------------------------------------
template <bool MASK>
__device__ __forceinline__ void seam_pair(unsigned a, unsigned b, unsigned vmin, unsigned vspan, unsigned &n, unsigned &sa, unsigned &sb,
                                          unsigned long long &saa, unsigned long long &sbb, unsigned long long &sab)
{
    if (MASK) {
        const bool ok = (a - vmin <= vspan) && (b - vmin <= vspan);
        a = ok ? a : 0u;
        b = ok ? b : 0u;
        n += ok ? 1u : 0u;
    }
    sa += a;
    sb += b;
    saa += (unsigned long long)(a * a);      // a, b < 2^16: the 32-bit products are exact
    sbb += (unsigned long long)(b * b);
    sab += (unsigned long long)(a * b);
}

// grid.x: groups of 64 overlap samples; grid.y: line ranges of rows_per_block lines.  The shuffles reduce over the lanes
// that share a channel: all 64 at spp 1, the 16 with the same lane % 4 at spp 4.
template <bool MASK, int SPP>
__global__ __launch_bounds__(kBlock) void seam_moments_kernel(const uint16_t *__restrict__ left, const uint16_t *__restrict__ right, long Ws,
                                                             long L, int fs2, unsigned vmin, unsigned vspan,
                                                             unsigned long long *__restrict__ acc, long rows_per_block)
{
    __shared__ unsigned long long sh[kWaves][6][SPP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    const long r0 = (long)blockIdx.y * rows_per_block;
    long r1 = r0 + rows_per_block;
    if (r1 > L) r1 = L;
    unsigned n = 0, sa = 0, sb = 0;
    unsigned long long saa = 0, sbb = 0, sab = 0;
    if (j < fs2) {
        const uint16_t *pa = left + (Ws - fs2) + j, *pb = right + j;      // + r * Ws: inside line r of either raster
        long r = r0 + wave;
        for (; r + (kRowsInFlight - 1) * kWaves < r1; r += kRowsInFlight * kWaves) {
            unsigned a[kRowsInFlight], b[kRowsInFlight];
#pragma unroll
            for (int u = 0; u < kRowsInFlight; ++u) {
                a[u] = pa[(r + u * kWaves) * Ws];
                b[u] = pb[(r + u * kWaves) * Ws];
            }
#pragma unroll
            for (int u = 0; u < kRowsInFlight; ++u) seam_pair<MASK>(a[u], b[u], vmin, vspan, n, sa, sb, saa, sbb, sab);
        }
        for (; r < r1; r += kWaves) seam_pair<MASK>(pa[r * Ws], pb[r * Ws], vmin, vspan, n, sa, sb, saa, sbb, sab);
        if (!MASK) n = (unsigned)((r1 - r0 - wave + kWaves - 1) / kWaves);      // the lines this wave took
    }
    unsigned long long v[6] = {n, sa, sb, saa, sbb, sab};
#pragma unroll
    for (int off = 32; off >= SPP; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 6; ++k) v[k] += __shfl_xor(v[k], off, 64);
    }
    if (lane < SPP) {
#pragma unroll
        for (int k = 0; k < 6; ++k) sh[wave][k][lane] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 6 * SPP) {
        const int k = threadIdx.x / SPP, c = threadIdx.x % SPP;
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) t += sh[w][k][c];
        atomicAdd(acc + k * SPP + c, t);
    }
}

// The totals of every line block of B lines in ONE launch (`oip stitch --balance-lines`): block k < nb - 1 covers lines
// [k B, (k + 1) B), the last one [(nb - 1) B, L), and its six totals go to plane k of acc, (nb, 6, SPP).  Lane mapping, line
// walk and reduction are seam_moments_kernel's.  A line RANGE (at most rows_per_range lines, never across a block boundary)
// is what a workgroup reduces and adds: full blocks are cut into ranges_per_block ranges each, the last block into whatever
// it needs, and the workgroups of a column group (blockIdx.y) take the ranges with a grid stride, so the grid does not grow
// with nb.  The 32-bit partials start again with every range: a lane sees at most 65536 lines between two reductions.
template <bool MASK, int SPP>
__global__ __launch_bounds__(kBlock) void seam_moments_blocks_kernel(const uint16_t *__restrict__ left, const uint16_t *__restrict__ right,
                                                                    long Ws, long L, int fs2, unsigned vmin, unsigned vspan,
                                                                    unsigned long long *__restrict__ acc, long B, long nb,
                                                                    long rows_per_range, long ranges_per_block, long nranges)
{
    __shared__ unsigned long long sh[kWaves][6][SPP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.y * 64 + lane;
    const uint16_t *pa = left + (Ws - fs2) + j, *pb = right + j;      // + r * Ws: inside line r of either raster (j < fs2)
    const long full = (nb - 1) * ranges_per_block;                    // the ranges of the blocks in front of the last one
    for (long y = blockIdx.x; y < nranges; y += gridDim.x) {
        const long k = y < full ? y / ranges_per_block : nb - 1;
        const long s = y < full ? y - k * ranges_per_block : y - full;
        const long end = k < nb - 1 ? (k + 1) * B : L;
        const long r0 = k * B + s * rows_per_range;
        long r1 = r0 + rows_per_range;
        if (r1 > end) r1 = end;
        unsigned n = 0, sa = 0, sb = 0;
        unsigned long long saa = 0, sbb = 0, sab = 0;
        if (j < fs2) {
            long r = r0 + wave;
            for (; r + (kRowsInFlight - 1) * kWaves < r1; r += kRowsInFlight * kWaves) {
                unsigned a[kRowsInFlight], b[kRowsInFlight];
#pragma unroll
                for (int u = 0; u < kRowsInFlight; ++u) {
                    a[u] = pa[(r + u * kWaves) * Ws];
                    b[u] = pb[(r + u * kWaves) * Ws];
                }
#pragma unroll
                for (int u = 0; u < kRowsInFlight; ++u) seam_pair<MASK>(a[u], b[u], vmin, vspan, n, sa, sb, saa, sbb, sab);
            }
            for (; r < r1; r += kWaves) seam_pair<MASK>(pa[r * Ws], pb[r * Ws], vmin, vspan, n, sa, sb, saa, sbb, sab);
            if (!MASK) n = (unsigned)((r1 - r0 - wave + kWaves - 1) / kWaves);      // the lines this wave took (r1 > r0)
        }
        unsigned long long v[6] = {n, sa, sb, saa, sbb, sab};
#pragma unroll
        for (int off = 32; off >= SPP; off >>= 1) {
#pragma unroll
            for (int m = 0; m < 6; ++m) v[m] += __shfl_xor(v[m], off, 64);
        }
        if (lane < SPP) {
#pragma unroll
            for (int m = 0; m < 6; ++m) sh[wave][m][lane] = v[m];
        }
        __syncthreads();
        if (threadIdx.x < 6 * SPP) {
            const int m = threadIdx.x / SPP, c = threadIdx.x % SPP;
            unsigned long long t = 0;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) t += sh[w][m][c];
            atomicAdd(acc + (k * 6 + m) * SPP + c, t);
        }
        __syncthreads();                                              // sh is written again in the next trip
    }
}

// ---- balanced stitch -----------------------------------------------------------------------------------------------
// b' = clamp((G b + O + 32768) >> 16, 0, 65535), 64-bit, arithmetic shift.  t >> 16 lies in 0..65535 exactly when the high
// dword of t is zero; a negative high dword clamps to 0, a positive one to 65535.  orr = O + 32768 as 64 bits.
__device__ __forceinline__ unsigned balance_px(unsigned b, int G, long long orr)
{
    const long long t = (long long)G * (long long)(int)b + orr;
    const int hi = (int)(t >> 32);
    const unsigned lo = (unsigned)t;
    return hi == 0 ? lo >> 16 : (hi < 0 ? 0u : 65535u);
}

struct SeamGeom {
    long Ws;           // samples per input line
    int half;          // Ws - fs: samples an output line takes from either image
    int off_b;         // Ws - 2 fs: output sample x pairs with sample x - off_b of image 2
    int z0, z1;        // the blend zone in output samples: [half - h*spp, half + h*spp)
    int spp_shift;     // log2(spp)
    unsigned h2, h4;   // 2h, 4h
    unsigned vmin;     // samples below it are "no data" inside the blend zone
};

// output sample x of line r, any x; G / orr: those of channel x % spp
__device__ __forceinline__ unsigned seam_sample(const uint16_t *__restrict__ left, const uint16_t *__restrict__ right, const SeamGeom &g,
                                                long r, int x, int G, long long orr)
{
    if (x < g.z0) return left[r * g.Ws + x];
    const unsigned b = right[r * g.Ws + (x - g.off_b)];
    const unsigned bb = balance_px(b, G, orr);
    if (x >= g.z1) return bb;
    const unsigned a = left[r * g.Ws + x];
    if (a < g.vmin) return bb;
    if (b < g.vmin) return a;
    const unsigned wr = 2u * (unsigned)((x - g.z0) >> g.spp_shift) + 1u, wl = g.h4 - wr;
    return (wl * a + wr * bb + g.h2) / g.h4;          // 4h * 65535 + 2h < 2^32: h <= 16384, host-checked
}

// 8 consecutive u16 starting at element index `e` of `p` (e may be odd), as 4 dwords; the dwords covering the span are
// clamped to the last one that holds a valid element (stitch.hip's load8_u16)
__device__ __forceinline__ uint4 seam_load8(const uint16_t *__restrict__ p, long e, long n_elems)
{
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
    const long d0 = e >> 1, dmax = (n_elems - 1) >> 1;
    uint32_t w[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const long di = d0 + i;
        w[i] = q[di > dmax ? dmax : di];
    }
    uint4 o;
    if (e & 1) {
        o.x = __builtin_amdgcn_alignbit(w[1], w[0], 16);
        o.y = __builtin_amdgcn_alignbit(w[2], w[1], 16);
        o.z = __builtin_amdgcn_alignbit(w[3], w[2], 16);
        o.w = __builtin_amdgcn_alignbit(w[4], w[3], 16);
    } else {
        o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3];
    }
    return o;
}

// requires: out base 16-byte aligned, (2*half) % 8 == 0, left/right bases 4-byte aligned, Ws * L even.
// gq[k] / oq[k]: gain and offset + 32768 of channel k % spp, k = 0..3 (slot i of a chunk is channel i % spp)
__global__ __launch_bounds__(kBlock) void stitch_balanced_kernel(const uint16_t *__restrict__ left, const uint16_t *__restrict__ right,
                                                                 uint16_t *__restrict__ out, SeamGeom g, long L,
                                                                 const int *__restrict__ gain, const int *__restrict__ offset, int spp)
{
    int G[4];
    long long orr[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        G[k] = gain[k & (spp - 1)];
        orr[k] = (long long)offset[k & (spp - 1)] + 32768;
    }
    const int cpr = (2 * g.half) / 8;             // chunks per output line
    const long nchunks = (long)cpr * L;
    const long n_elems = g.Ws * L;
    constexpr int U = 4;
    const long stride = (long)gridDim.x * kBlock;
    for (long f0 = (long)blockIdx.x * kBlock + threadIdx.x; f0 < nchunks; f0 += stride * U) {
        uint4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long f = f0 + u * stride;
            if (f >= nchunks) break;
            const long r = f / cpr;
            const int x0 = (int)(f - r * cpr) * 8;
            if (x0 + 8 <= g.z0) {
                v[u] = seam_load8(left, r * g.Ws + x0, n_elems);
            } else if (x0 >= g.z1) {
                const uint4 q = seam_load8(right, r * g.Ws + (x0 - g.off_b), n_elems);
                v[u].x = balance_px(q.x & 0xffffu, G[0], orr[0]) | (balance_px(q.x >> 16, G[1], orr[1]) << 16);
                v[u].y = balance_px(q.y & 0xffffu, G[2], orr[2]) | (balance_px(q.y >> 16, G[3], orr[3]) << 16);
                v[u].z = balance_px(q.z & 0xffffu, G[0], orr[0]) | (balance_px(q.z >> 16, G[1], orr[1]) << 16);
                v[u].w = balance_px(q.w & 0xffffu, G[2], orr[2]) | (balance_px(q.w >> 16, G[3], orr[3]) << 16);
            } else {
                unsigned t[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) t[i] = seam_sample(left, right, g, r, x0 + i, G[i & 3], orr[i & 3]);
                v[u].x = t[0] | (t[1] << 16); v[u].y = t[2] | (t[3] << 16);
                v[u].z = t[4] | (t[5] << 16); v[u].w = t[6] | (t[7] << 16);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long f = f0 + u * stride;
            if (f >= nchunks) break;
            reinterpret_cast<uint4 *>(out)[f] = v[u];
        }
    }
}

__global__ __launch_bounds__(kBlock) void stitch_balanced_scalar_kernel(const uint16_t *__restrict__ left, const uint16_t *__restrict__ right,
                                                                        uint16_t *__restrict__ out, SeamGeom g, long L,
                                                                        const int *__restrict__ gain, const int *__restrict__ offset, int spp)
{
    const long ow = 2L * g.half;
    const long n = ow * L;
    const long stride = (long)gridDim.x * kBlock;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const long r = i / ow;
        const int x = (int)(i - r * ow);
        const int c = x & (spp - 1);
        out[i] = (uint16_t)seam_sample(left, right, g, r, x, gain[c], (long long)offset[c] + 32768);
    }
}

// ---- balanced stitch, one (G, O) per line and channel --------------------------------------------------------------
// stitch_balanced_kernel with the pairs of line r read from per-line tables (entry r * SPP + c) instead of kept as loop
// constants.  Per lane: a chunk left of the blend zone is the same pure copy and reads no table; any other chunk loads the SPP
// pairs of its own line next to its image samples -- one dword from either table at SPP 1, one 16-byte load from either at
// SPP 4 -- which the thousands of chunks of a line share through L2.  The arithmetic is balance_px / seam_sample, so equal
// pairs on every line give stitch_balanced_kernel's bytes.
// requires: stitch_balanced_kernel's alignments, and at SPP 4 table bases 16-byte aligned.
template <int SPP>
__device__ __forceinline__ void seam_line_pairs(const int *__restrict__ gain, const int *__restrict__ offset, long r, int (&G)[4], long long (&orr)[4])
{
    if (SPP == 4) {
        const int4 g4 = reinterpret_cast<const int4 *>(gain)[r], o4 = reinterpret_cast<const int4 *>(offset)[r];
        G[0] = g4.x; G[1] = g4.y; G[2] = g4.z; G[3] = g4.w;
        orr[0] = (long long)o4.x + 32768; orr[1] = (long long)o4.y + 32768; orr[2] = (long long)o4.z + 32768; orr[3] = (long long)o4.w + 32768;
    } else {
        const int g1 = gain[r];
        const long long o1 = (long long)offset[r] + 32768;
#pragma unroll
        for (int k = 0; k < 4; ++k) { G[k] = g1; orr[k] = o1; }
    }
}

template <int SPP>
__global__ __launch_bounds__(kBlock) void stitch_balanced_lines_kernel(const uint16_t *__restrict__ left, const uint16_t *__restrict__ right,
                                                                       uint16_t *__restrict__ out, SeamGeom g, long L,
                                                                       const int *__restrict__ gain, const int *__restrict__ offset)
{
    const int cpr = (2 * g.half) / 8;             // chunks per output line
    const long nchunks = (long)cpr * L;
    const long n_elems = g.Ws * L;
    constexpr int U = 4;
    const long stride = (long)gridDim.x * kBlock;
    for (long f0 = (long)blockIdx.x * kBlock + threadIdx.x; f0 < nchunks; f0 += stride * U) {
        uint4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long f = f0 + u * stride;
            if (f >= nchunks) break;
            const long r = f / cpr;
            const int x0 = (int)(f - r * cpr) * 8;
            if (x0 + 8 <= g.z0) {
                v[u] = seam_load8(left, r * g.Ws + x0, n_elems);
                continue;
            }
            int G[4];
            long long orr[4];
            seam_line_pairs<SPP>(gain, offset, r, G, orr);
            if (x0 >= g.z1) {
                const uint4 q = seam_load8(right, r * g.Ws + (x0 - g.off_b), n_elems);
                v[u].x = balance_px(q.x & 0xffffu, G[0], orr[0]) | (balance_px(q.x >> 16, G[1], orr[1]) << 16);
                v[u].y = balance_px(q.y & 0xffffu, G[2], orr[2]) | (balance_px(q.y >> 16, G[3], orr[3]) << 16);
                v[u].z = balance_px(q.z & 0xffffu, G[0], orr[0]) | (balance_px(q.z >> 16, G[1], orr[1]) << 16);
                v[u].w = balance_px(q.w & 0xffffu, G[2], orr[2]) | (balance_px(q.w >> 16, G[3], orr[3]) << 16);
            } else {
                unsigned t[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) t[i] = seam_sample(left, right, g, r, x0 + i, G[i & 3], orr[i & 3]);
                v[u].x = t[0] | (t[1] << 16); v[u].y = t[2] | (t[3] << 16);
                v[u].z = t[4] | (t[5] << 16); v[u].w = t[6] | (t[7] << 16);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long f = f0 + u * stride;
            if (f >= nchunks) break;
            reinterpret_cast<uint4 *>(out)[f] = v[u];
        }
    }
}

__global__ __launch_bounds__(kBlock) void stitch_balanced_lines_scalar_kernel(const uint16_t *__restrict__ left, const uint16_t *__restrict__ right,
                                                                              uint16_t *__restrict__ out, SeamGeom g, long L,
                                                                              const int *__restrict__ gain, const int *__restrict__ offset, int spp)
{
    const long ow = 2L * g.half;
    const long n = ow * L;
    const long stride = (long)gridDim.x * kBlock;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const long r = i / ow;
        const int x = (int)(i - r * ow);
        if (x < g.z0) {                                               // a copy: no table entry is read
            out[i] = left[r * g.Ws + x];
            continue;
        }
        const long e = r * spp + (x & (spp - 1));
        out[i] = (uint16_t)seam_sample(left, right, g, r, x, gain[e], (long long)offset[e] + 32768);
    }
}

}  // namespace

extern "C" int oip_seam_moments_u16(oip_ctx *ctx, const uint16_t *d_left, const uint16_t *d_right, int Ws, long L, int fs, int spp,
                                    int valid_min, int valid_max, uint64_t *d_acc)
{
    OIP_CHECK_CTX(ctx);
    if (!d_left || !d_right || !d_acc || ((uintptr_t)d_acc & 7) || ((uintptr_t)d_left & 1) || ((uintptr_t)d_right & 1) || (spp != 1 && spp != 4) ||
        Ws <= 0 || Ws % spp != 0 || fs <= 0 || fs % spp != 0 || 2L * fs > Ws || L < 0 || L >= (1L << 31) || valid_min < 0 || valid_max > 65535 ||
        valid_min > valid_max)
        return oip_fail(ctx, OIP_E_INVALID, "oip_seam_moments_u16: bad argument");
    if ((unsigned long long)(2 * fs / spp) * (unsigned long long)L > (1ull << 32))
        return oip_fail(ctx, OIP_E_INVALID, "oip_seam_moments_u16: more than 2^32 pairs per channel");
    if (L == 0) return OIP_OK;
    OipProfScope prof(ctx, "seam_moments_kernel");
    const int fs2 = 2 * fs;
    const int gx = (fs2 + 63) / 64;
    // about 8 blocks per CU over the whole grid; a range between 64 and kWaves * kMaxLaneRows lines
    long want = (long)ctx->cu_count * 8 / gx;
    if (want < 1) want = 1;
    long rpb = (L + want - 1) / want;
    if (rpb < 64) rpb = 64;
    if (rpb > kWaves * kMaxLaneRows) rpb = kWaves * kMaxLaneRows;
    const int gy = (int)((L + rpb - 1) / rpb);
    const bool mask = !(valid_min == 0 && valid_max == 65535);
    const unsigned vmin = (unsigned)valid_min, vspan = (unsigned)(valid_max - valid_min);
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(d_acc);
    const dim3 grid(gx, gy), block(kBlock);
#define OIP_SEAM_LAUNCH(M, S) \
    hipLaunchKernelGGL((seam_moments_kernel<M, S>), grid, block, 0, ctx->stream, d_left, d_right, (long)Ws, L, fs2, vmin, vspan, acc, rpb)
    if (spp == 1) { if (mask) OIP_SEAM_LAUNCH(true, 1); else OIP_SEAM_LAUNCH(false, 1); }
    else          { if (mask) OIP_SEAM_LAUNCH(true, 4); else OIP_SEAM_LAUNCH(false, 4); }
#undef OIP_SEAM_LAUNCH
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}

extern "C" int oip_stitch_balanced_u16(oip_ctx *ctx, const uint16_t *d_left, const uint16_t *d_right, uint16_t *d_out, int Ws, long L, int fs,
                                       int spp, const int32_t *d_gain_q16, const int32_t *d_offset_q16, int feather, int valid_min)
{
    OIP_CHECK_CTX(ctx);
    if (!d_left || !d_right || !d_out || !d_gain_q16 || !d_offset_q16 || ((uintptr_t)d_gain_q16 & 3) || ((uintptr_t)d_offset_q16 & 3) ||
        ((uintptr_t)d_left & 1) || ((uintptr_t)d_right & 1) || ((uintptr_t)d_out & 1) || (spp != 1 && spp != 4) || Ws <= 0 || Ws % spp != 0 ||
        fs < 0 || fs % spp != 0 || fs >= Ws || L < 0 || feather < 0 || (long)feather * spp > fs || valid_min > 65535)
        return oip_fail(ctx, OIP_E_INVALID, "oip_stitch_balanced_u16: bad argument");
    if (feather > 16384) return oip_fail(ctx, OIP_E_UNSUPPORTED, "oip_stitch_balanced_u16: feather above 16384 pixels (the blend's 32-bit numerator)");
    if (L == 0) return OIP_OK;
    OipProfScope prof(ctx, "stitch_balanced_kernel");
    SeamGeom g;
    g.Ws = Ws;
    g.half = Ws - fs;
    g.off_b = Ws - 2 * fs;
    g.z0 = g.half - feather * spp;
    g.z1 = g.half + feather * spp;
    g.spp_shift = spp == 4 ? 2 : 0;
    g.h2 = 2u * (unsigned)feather;
    g.h4 = 4u * (unsigned)feather;
    g.vmin = valid_min < 0 ? 0u : (unsigned)valid_min;
    const int ow = 2 * g.half;
    const bool fast = (ow % 8 == 0) && (((uintptr_t)d_out & 15) == 0) && (((uintptr_t)d_left & 3) == 0) && (((uintptr_t)d_right & 3) == 0) &&
                      ((long)Ws * L >= 16 && ((long)Ws * L) % 2 == 0);
    // one resident set of blocks (8 per CU), grid-stride over the rest
    const long cap = (long)ctx->cu_count * 8;
    if (fast) {
        const long nchunks = (long)(ow / 8) * L;
        long blocks = (nchunks + (long)kBlock * 4 - 1) / ((long)kBlock * 4);
        if (blocks > cap) blocks = cap;
        hipLaunchKernelGGL(stitch_balanced_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, d_left, d_right, d_out, g, L,
                           d_gain_q16, d_offset_q16, spp);
    } else {
        const long n = (long)ow * L;
        long blocks = (n + kBlock - 1) / kBlock;
        if (blocks > cap) blocks = cap;
        hipLaunchKernelGGL(stitch_balanced_scalar_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, d_left, d_right, d_out, g, L,
                           d_gain_q16, d_offset_q16, spp);
    }
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}

extern "C" int oip_seam_moments_blocks_u16(oip_ctx *ctx, const uint16_t *d_left, const uint16_t *d_right, int Ws, long L, int fs, int spp,
                                           int valid_min, int valid_max, long block_lines, uint64_t *d_acc)
{
    OIP_CHECK_CTX(ctx);
    if (!d_left || !d_right || !d_acc || ((uintptr_t)d_acc & 7) || ((uintptr_t)d_left & 1) || ((uintptr_t)d_right & 1) || (spp != 1 && spp != 4) ||
        Ws <= 0 || Ws % spp != 0 || fs <= 0 || fs % spp != 0 || 2L * fs > Ws || L < 0 || L >= (1L << 31) || valid_min < 0 || valid_max > 65535 ||
        valid_min > valid_max || block_lines < 1)
        return oip_fail(ctx, OIP_E_INVALID, "oip_seam_moments_blocks_u16: bad argument");
    if ((unsigned long long)(2 * fs / spp) * (unsigned long long)L > (1ull << 32))
        return oip_fail(ctx, OIP_E_INVALID, "oip_seam_moments_blocks_u16: more than 2^32 pairs per channel");
    if (L == 0) return OIP_OK;
    const int fs2 = 2 * fs;
    const int gx = (fs2 + 63) / 64;
    if (gx > 65535) return oip_fail(ctx, OIP_E_UNSUPPORTED, "oip_seam_moments_blocks_u16: an overlap of more than 65535 * 64 samples");
    OipProfScope prof(ctx, "seam_moments_blocks_kernel");
    const long B = block_lines;
    const long nb = L / B > 1 ? L / B : 1;
    const long last = L - (nb - 1) * B;                              // B .. 2B - 1 lines, or all L of them
    // ranges as oip_seam_moments_u16 sizes them (about 8 blocks per CU over the whole grid, 64 .. kWaves * kMaxLaneRows lines),
    // then cut at the block boundaries
    long want = (long)ctx->cu_count * 8 / gx;
    if (want < 1) want = 1;
    long rpr = (L + want - 1) / want;
    if (rpr < 64) rpr = 64;
    if (rpr > kWaves * kMaxLaneRows) rpr = kWaves * kMaxLaneRows;
    const long per_block = nb > 1 ? (B - 1) / rpr + 1 : 0;           // (B <= L where it is used)
    const long nranges = (nb - 1) * per_block + (last - 1) / rpr + 1;
    const long gy = nranges < want ? nranges : want;                  // one resident set; the rest by grid stride
    const bool mask = !(valid_min == 0 && valid_max == 65535);
    const unsigned vmin = (unsigned)valid_min, vspan = (unsigned)(valid_max - valid_min);
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(d_acc);
    const dim3 grid((unsigned)gy, (unsigned)gx), block(kBlock);
#define OIP_SEAM_LAUNCH(M, S)                                                                                                                     \
    hipLaunchKernelGGL((seam_moments_blocks_kernel<M, S>), grid, block, 0, ctx->stream, d_left, d_right, (long)Ws, L, fs2, vmin, vspan, acc, B, nb, \
                       rpr, per_block, nranges)
    if (spp == 1) { if (mask) OIP_SEAM_LAUNCH(true, 1); else OIP_SEAM_LAUNCH(false, 1); }
    else          { if (mask) OIP_SEAM_LAUNCH(true, 4); else OIP_SEAM_LAUNCH(false, 4); }
#undef OIP_SEAM_LAUNCH
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}

extern "C" int oip_stitch_balanced_lines_u16(oip_ctx *ctx, const uint16_t *d_left, const uint16_t *d_right, uint16_t *d_out, int Ws, long L, int fs,
                                             int spp, const int32_t *d_line_gain_q16, const int32_t *d_line_offset_q16, int feather, int valid_min)
{
    OIP_CHECK_CTX(ctx);
    if (!d_left || !d_right || !d_out || !d_line_gain_q16 || !d_line_offset_q16 || ((uintptr_t)d_line_gain_q16 & 3) ||
        ((uintptr_t)d_line_offset_q16 & 3) || ((uintptr_t)d_left & 1) || ((uintptr_t)d_right & 1) || ((uintptr_t)d_out & 1) ||
        (spp != 1 && spp != 4) || Ws <= 0 || Ws % spp != 0 || fs < 0 || fs % spp != 0 || fs >= Ws || L < 0 || feather < 0 ||
        (long)feather * spp > fs || valid_min > 65535)
        return oip_fail(ctx, OIP_E_INVALID, "oip_stitch_balanced_lines_u16: bad argument");
    if (feather > 16384)
        return oip_fail(ctx, OIP_E_UNSUPPORTED, "oip_stitch_balanced_lines_u16: feather above 16384 pixels (the blend's 32-bit numerator)");
    if (L == 0) return OIP_OK;
    OipProfScope prof(ctx, "stitch_balanced_lines_kernel");
    SeamGeom g;
    g.Ws = Ws;
    g.half = Ws - fs;
    g.off_b = Ws - 2 * fs;
    g.z0 = g.half - feather * spp;
    g.z1 = g.half + feather * spp;
    g.spp_shift = spp == 4 ? 2 : 0;
    g.h2 = 2u * (unsigned)feather;
    g.h4 = 4u * (unsigned)feather;
    g.vmin = valid_min < 0 ? 0u : (unsigned)valid_min;
    const int ow = 2 * g.half;
    const bool tables16 = spp == 1 || ((((uintptr_t)d_line_gain_q16 | (uintptr_t)d_line_offset_q16) & 15) == 0);
    const bool fast = (ow % 8 == 0) && (((uintptr_t)d_out & 15) == 0) && (((uintptr_t)d_left & 3) == 0) && (((uintptr_t)d_right & 3) == 0) &&
                      ((long)Ws * L >= 16 && ((long)Ws * L) % 2 == 0) && tables16;
    // one resident set of blocks (8 per CU), grid-stride over the rest
    const long cap = (long)ctx->cu_count * 8;
    if (fast) {
        const long nchunks = (long)(ow / 8) * L;
        long blocks = (nchunks + (long)kBlock * 4 - 1) / ((long)kBlock * 4);
        if (blocks > cap) blocks = cap;
        if (spp == 1)
            hipLaunchKernelGGL(stitch_balanced_lines_kernel<1>, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, d_left, d_right, d_out, g, L,
                               d_line_gain_q16, d_line_offset_q16);
        else
            hipLaunchKernelGGL(stitch_balanced_lines_kernel<4>, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, d_left, d_right, d_out, g, L,
                               d_line_gain_q16, d_line_offset_q16);
    } else {
        const long n = (long)ow * L;
        long blocks = (n + kBlock - 1) / kBlock;
        if (blocks > cap) blocks = cap;
        hipLaunchKernelGGL(stitch_balanced_lines_scalar_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, d_left, d_right, d_out, g, L,
                           d_line_gain_q16, d_line_offset_q16, spp);
    }
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}
