// seam.hip -- the moments of the overlap of two strips on gfx950: what `oip stitch --balance / --balance-lines` fits its gains
// and offsets to (the balanced stitch itself is in stitch.hip).  The reference has no counterpart.
//
// After prestitch the last 2*fold columns of image 1 and the first 2*fold columns of image 2 see the same ground.  Lines are
// handled in SAMPLE units as StitchTiff does (Ws = W*spp, fs = fold*spp; the channel of sample index j is j % spp), and an
// overlap pair is  a = left[r][Ws - 2fs + j],  b = right[r][j],  j in [0, 2fs).
//
//   oip_seam_moments_u16         per channel  n, Sa, Sb, Saa, Sbb, Sab  over the pairs whose two samples are both valid,
//                                exact integers ADDED into a (6, spp) uint64 array
//   oip_seam_moments_blocks_u16  the same per block of B lines, (nb, 6, spp): block k < nb - 1 covers lines [k B, (k + 1) B),
//                                the last one [(nb - 1) B, L)
//
// One kernel: the strip's totals are the block totals with one block of L lines, launched under its own profiler name.
//
// Layout / mapping.  The overlap is a few hundred samples wide and as tall as the strip, so a lane owns ONE overlap sample j
// and walks lines: the 64 lanes of a wave read 128 contiguous bytes of a line of either image, the four waves of a workgroup
// take every fourth line of a line range, four lines in flight per wave.  Both windows start wherever Ws - 2fs and the line
// pitch put them -- in general on a 2-byte boundary only, a different one on every line when Ws is odd -- so the loads are
// 2-byte loads and no alignment case exists.  (The pass reads 2*2fs of the 2*Ws samples per line the stitch moves: about 1 %
// of its bytes at the product geometries.)  A lane's channel is j % spp = lane % spp (64 % spp == 0), a loop constant.
// A line RANGE (at most rows_per_range lines, never across a block boundary) is what a workgroup reduces and adds.  The ranges
// are sized for about one resident set of workgroups (8 per CU over the whole grid, 64 .. 4 * 65536 lines) and then cut at the
// block boundaries: full blocks into ranges_per_block ranges each, the last block into whatever it needs.  grid.x: groups of
// 64 overlap samples; grid.y: the workgroups of a column group, which take the ranges with a grid stride, so the grid does not
// grow with nb.  A lane sees at most 65536 lines between two reductions, so its n, Sa and Sb fit 32 bits and start again
// with every range; the three products need 64 (`S += (uint64_t)(x * y)` on the exact 32-bit product, the form colstats.hip
// settled on).
// Reduction: xor shuffles over the lanes of a wave that share a channel, the four waves through LDS, then 6*spp 64-bit
// integer vector atomics per range (global_atomic_add_x2, no return) into plane k of d_acc: totals do not depend on the launch
// geometry and add over calls.
#include "oip_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kRowsInFlight = 4;
constexpr long kMaxLaneRows = 65536;         // 65536 * 65535 < 2^32: n, Sa, Sb of a lane in 32 bits

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

// The shuffles reduce over the lanes that share a channel: all 64 at spp 1, the 16 with the same lane % 4 at spp 4.
template <bool MASK, int SPP>
__global__ __launch_bounds__(kBlock) void seam_moments_blocks_kernel(const uint16_t *__restrict__ left, const uint16_t *__restrict__ right,
                                                                    long Ws, long L, int fs2, unsigned vmin, unsigned vspan,
                                                                    unsigned long long *__restrict__ acc, long B, long nb,
                                                                    long rows_per_range, long ranges_per_block, long nranges)
{
    __shared__ unsigned long long sh[kWaves][6][SPP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    const uint16_t *pa = left + (Ws - fs2) + j, *pb = right + j;      // + r * Ws: inside line r of either raster (j < fs2)
    const long full = (nb - 1) * ranges_per_block;                    // the ranges of the blocks in front of the last one
    for (long y = blockIdx.y; y < nranges; y += gridDim.y) {
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

// Both entries: `fn` and `scope` are the entry's name in a refusal and in the profiler; the strip entry passes B = L.
int seam_moments(oip_ctx *ctx, const char *fn, const char *scope, const uint16_t *d_left, const uint16_t *d_right, int Ws, long L, int fs,
                 int spp, int valid_min, int valid_max, long B, uint64_t *d_acc)
{
    if (!d_left || !d_right || !d_acc || ((uintptr_t)d_acc & 7) || ((uintptr_t)d_left & 1) || ((uintptr_t)d_right & 1) || (spp != 1 && spp != 4) ||
        Ws <= 0 || Ws % spp != 0 || fs <= 0 || fs % spp != 0 || 2L * fs > Ws || L < 0 || L >= (1L << 31) || valid_min < 0 || valid_max > 65535 ||
        valid_min > valid_max)
        return oip_fail(ctx, OIP_E_INVALID, "%s: bad argument", fn);
    if ((unsigned long long)(2 * fs / spp) * (unsigned long long)L > (1ull << 32))
        return oip_fail(ctx, OIP_E_INVALID, "%s: more than 2^32 pairs per channel", fn);
    if (L == 0) return OIP_OK;
    OipProfScope prof(ctx, scope);
    const int fs2 = 2 * fs;
    const int gx = (fs2 + 63) / 64;
    const long nb = L / B > 1 ? L / B : 1;
    const long last = L - (nb - 1) * B;                              // B .. 2B - 1 lines, or all L of them
    // about 8 workgroups per CU over the whole grid; a range between 64 and kWaves * kMaxLaneRows lines, then cut at the block
    // boundaries
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
    const dim3 grid((unsigned)gx, (unsigned)gy), block(kBlock);
#define OIP_SEAM_LAUNCH(M, S)                                                                                                                     \
    hipLaunchKernelGGL((seam_moments_blocks_kernel<M, S>), grid, block, 0, ctx->stream, d_left, d_right, (long)Ws, L, fs2, vmin, vspan, acc, B, nb, \
                       rpr, per_block, nranges)
    if (spp == 1) { if (mask) OIP_SEAM_LAUNCH(true, 1); else OIP_SEAM_LAUNCH(false, 1); }
    else          { if (mask) OIP_SEAM_LAUNCH(true, 4); else OIP_SEAM_LAUNCH(false, 4); }
#undef OIP_SEAM_LAUNCH
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}

}  // namespace

extern "C" int oip_seam_moments_u16(oip_ctx *ctx, const uint16_t *d_left, const uint16_t *d_right, int Ws, long L, int fs, int spp,
                                    int valid_min, int valid_max, uint64_t *d_acc)
{
    OIP_CHECK_CTX(ctx);
    return seam_moments(ctx, "oip_seam_moments_u16", "seam_moments_kernel", d_left, d_right, Ws, L, fs, spp, valid_min, valid_max, L, d_acc);
}

extern "C" int oip_seam_moments_blocks_u16(oip_ctx *ctx, const uint16_t *d_left, const uint16_t *d_right, int Ws, long L, int fs, int spp,
                                           int valid_min, int valid_max, long block_lines, uint64_t *d_acc)
{
    OIP_CHECK_CTX(ctx);
    if (block_lines < 1) return oip_fail(ctx, OIP_E_INVALID, "oip_seam_moments_blocks_u16: bad argument");
    return seam_moments(ctx, "oip_seam_moments_blocks_u16", "seam_moments_blocks_kernel", d_left, d_right, Ws, L, fs, spp, valid_min, valid_max,
                        block_lines, d_acc);
}
