// noise.hip -- per-block noise keys of a u16 raster on gfx950: the one pass over a strip or product from which `oip noise`
// derives the sensor's noise-level function (sigma against signal level).  The reference has no counterpart.
//
// The raster is cut into B x B blocks (B = 8 or 16) anchored at the window's first sample.  Per block and channel, in exact
// integers (include/oip_c.h states them): the sum, the sum of squares and the four quadrant sums give the sample variance and
// the F ratio of between-quadrant to within-quadrant mean squares; a block with a sample outside the valid range, or with an F
// ratio above 4 (an edge, a ramp), gets a sentinel key, every other block the key (level << 8 | sigma in quarter DN).  The
// existing oip_histogram_u16 over a key plane is then the (level x sigma) table of the band.
//
// Layout / mapping.  HBM-bound, read-only: 2 B per sample in, 2 B per block and channel out (1/64 or 1/256 of the read).  A
// lane owns one 16-byte vector (8 samples) of each of the B lines of a block line, so adjacent lanes read adjacent 16 bytes,
// and V = B * spp / 8 adjacent lanes share a block: 1 at spp 1 B 8 (all five sums stay in the lane), 2 at spp 1 B 16, 4 and 8
// at spp 4, where a vector holds two pixels of four channels.  The V partial sums meet in a butterfly of wave shuffles (V
// divides 64: a block never straddles a wave); lane c of the block then finishes channel c.  grid.y walks the block lines with
// a stride of gridDim.y, so that the resident workgroups read neighbouring lines and a raster of any height fits the grid.
//
// Anything the vector form cannot take (a pitch that is not a multiple of 8 samples, a window that does not start on a 16-byte
// boundary) goes to the block-per-lane kernel: 2-byte loads, the same keys.
#include "oip_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kPerCu = 8;                    // workgroups per CU over the whole grid
constexpr unsigned kKeyNoData = 0x00FFu, kKeyStructured = 0x01FFu;

// the key of one block and channel from its quadrant sums q[0..3] (top-left, top-right, bottom-left, bottom-right), its sum of
// squares and whether it holds a sample outside the valid range.  n = B * B; every product fits 64 bits (oip_c.h).
template <int B>
__device__ __forceinline__ unsigned noise_key(const unsigned q[4], unsigned long long S2, bool nodata, int level_shift)
{
    constexpr unsigned long long n = (unsigned long long)B * B;
    constexpr unsigned den = (unsigned)(n * (n - 1) / 16);               // 16 D / (n (n - 1)) = D / den: 252 or 4080
    if (nodata) return kKeyNoData;
    const unsigned long long S1 = (unsigned long long)q[0] + q[1] + q[2] + q[3];
    const unsigned long long S1sq = S1 * S1;
    const unsigned long long D = n * S2 - S1sq;
    const unsigned long long Q = (unsigned long long)q[0] * q[0] + (unsigned long long)q[1] * q[1] + (unsigned long long)q[2] * q[2] +
                                 (unsigned long long)q[3] * q[3];
    const unsigned long long E = 4 * Q - S1sq;
    if (E * (n - 4) > 12 * (D - E)) return kKeyStructured;
    unsigned level = (unsigned)(S1 / n) >> level_shift;
    if (level > 255u) level = 255u;
    unsigned sq = 254u;
    if (D < 65025ull * den) {                                            // otherwise isqrt >= 255: the cap
        const unsigned t = (unsigned)D / den;                            // < 65025: exact in f32
        unsigned r = (unsigned)__fsqrt_rn((float)t);
        if (r * r > t) --r;
        if ((r + 1) * (r + 1) <= t) ++r;
        sq = r < 254u ? r : 254u;
    }
    return level << 8 | sq;
}

template <int SPP, int B>
__global__ __launch_bounds__(kBlock) void noise_blocks_u16_kernel(const uint16_t *__restrict__ img, long pitch, int nbx, long nby, unsigned vmin,
                                                                  unsigned vmax, int level_shift, uint16_t *__restrict__ keys, long key_pitch,
                                                                  size_t key_plane_stride)
{
    constexpr int V = B * SPP / 8;           // lanes (16-byte vectors) per block
    constexpr int C = SPP;
    constexpr int LR = V == 1 ? 2 : 1;       // V == 1: the lane's vector holds both the left and the right half of the block
    const int vx = blockIdx.x * kBlock + threadIdx.x;
    const int bx = vx / V, g = vx % V;
    const bool active = bx < nbx;            // (an inactive lane loads nothing and still takes part in the shuffles)
    const int side = V > 1 && g >= V / 2 ? 1 : 0;
    for (long by = blockIdx.y; by < nby; by += gridDim.y) {
        unsigned t[C][2][LR], mn[C], mx[C];
        unsigned long long s2[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            mn[c] = 0xffffffffu; mx[c] = 0u; s2[c] = 0ull;
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int k = 0; k < LR; ++k) t[c][h][k] = 0u;
        }
        if (active) {
            // vx * 8 + 8 <= nbx * B * SPP <= w * spp <= pitch: the vector lies inside the line
            const uint16_t *s = img + by * B * pitch + (long)vx * 8;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                uint4 v[B / 2];
#pragma unroll
                for (int j = 0; j < B / 2; ++j) v[j] = *reinterpret_cast<const uint4 *>(s + (long)(h * (B / 2) + j) * pitch);
#pragma unroll
                for (int j = 0; j < B / 2; ++j) {
                    const unsigned p[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const unsigned u = (i & 1) ? p[i >> 1] >> 16 : p[i >> 1] & 0xffffu;
                        const int c = SPP == 4 ? (i & 3) : 0;
                        const int k = V == 1 ? (i >> 2) : 0;
                        t[c][h][k] += u;
                        s2[c] += (unsigned long long)(u * u);            // u < 2^16: the 32-bit product is exact
                        mn[c] = u < mn[c] ? u : mn[c];
                        mx[c] = u > mx[c] ? u : mx[c];
                    }
                }
            }
        }
        // quadrant sums of the lane's share, then the sums of the block over its V lanes
        unsigned q[C][4];
        int bad[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            bad[c] = active && (mn[c] < vmin || mx[c] > vmax) ? 1 : 0;
            if (V == 1) {
                q[c][0] = t[c][0][0]; q[c][1] = t[c][0][LR - 1]; q[c][2] = t[c][1][0]; q[c][3] = t[c][1][LR - 1];
            } else {
                q[c][0] = side ? 0u : t[c][0][0]; q[c][1] = side ? t[c][0][0] : 0u;
                q[c][2] = side ? 0u : t[c][1][0]; q[c][3] = side ? t[c][1][0] : 0u;
            }
        }
#pragma unroll
        for (int m = 1; m < V; m <<= 1) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
#pragma unroll
                for (int k = 0; k < 4; ++k) q[c][k] += __shfl_xor(q[c][k], m);
                s2[c] += __shfl_xor(s2[c], m);
                bad[c] |= __shfl_xor(bad[c], m);
            }
        }
        // lane c of the block finishes channel c (V >= C)
        if (active && g < C) {
            unsigned qq[4] = {q[0][0], q[0][1], q[0][2], q[0][3]};
            unsigned long long ss = s2[0];
            int bb = bad[0];
#pragma unroll
            for (int c = 1; c < C; ++c)
                if (g == c) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) qq[k] = q[c][k];
                    ss = s2[c];
                    bb = bad[c];
                }
            keys[(size_t)g * key_plane_stride + by * key_pitch + bx] = (uint16_t)noise_key<B>(qq, ss, bb != 0, level_shift);
        }
    }
}

// any pitch / alignment: a lane owns one block and channel
template <int B>
__global__ __launch_bounds__(kBlock) void noise_blocks_u16_any_kernel(const uint16_t *__restrict__ img, long pitch, int nbx, long nby, int spp,
                                                                      unsigned vmin, unsigned vmax, int level_shift,
                                                                      uint16_t *__restrict__ keys, long key_pitch, size_t key_plane_stride)
{
    const long i = (long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (long)nbx * spp) return;
    const int bx = (int)(i / spp), c = (int)(i % spp);
    for (long by = blockIdx.y; by < nby; by += gridDim.y) {
        const uint16_t *s = img + by * B * pitch + (long)bx * B * spp + c;
        unsigned q[4] = {0u, 0u, 0u, 0u}, mn = 0xffffffffu, mx = 0u;
        unsigned long long s2 = 0ull;
#pragma unroll
        for (int h = 0; h < 2; ++h)
            for (int j = 0; j < B / 2; ++j) {
                const uint16_t *l = s + (long)(h * (B / 2) + j) * pitch;
#pragma unroll
                for (int x = 0; x < B; ++x) {
                    const unsigned u = l[x * spp];
                    q[2 * h + (x >= B / 2 ? 1 : 0)] += u;
                    s2 += (unsigned long long)(u * u);
                    mn = u < mn ? u : mn;
                    mx = u > mx ? u : mx;
                }
            }
        keys[(size_t)c * key_plane_stride + by * key_pitch + bx] = (uint16_t)noise_key<B>(q, s2, mn < vmin || mx > vmax, level_shift);
    }
}

}  // namespace

extern "C" int oip_noise_blocks_u16(oip_ctx *ctx, const uint16_t *d_src, long pitch, int w, long rows, int spp, int block, int level_shift,
                                    int valid_min, int valid_max, uint16_t *d_keys, long key_pitch, size_t key_plane_stride)
{
    OIP_CHECK_CTX(ctx);
    if ((block != 8 && block != 16) || (spp != 1 && spp != 4) || level_shift < 0 || level_shift > 8 || valid_min < 0 || valid_max > 65535 ||
        valid_min > valid_max || w < 0 || rows < 0 || pitch < (long)w * spp || !d_src || !d_keys || ((uintptr_t)d_src & 1) || ((uintptr_t)d_keys & 1) ||
        key_pitch < w / block)
        return oip_fail(ctx, OIP_E_INVALID, "oip_noise_blocks_u16: bad argument");
    const int nbx = w / block;
    const long nby = rows / block;
    if (nbx == 0 || nby == 0) return OIP_OK;
    if (spp == 4 && key_plane_stride < (size_t)((nby - 1) * key_pitch + nbx))
        return oip_fail(ctx, OIP_E_INVALID, "oip_noise_blocks_u16: the key planes overlap");
    const unsigned vmin = (unsigned)valid_min, vmax = (unsigned)valid_max;
    const bool vec = pitch % 8 == 0 && ((uintptr_t)d_src & 15) == 0;
    OipProfScope prof(ctx, vec ? "noise_blocks_u16_kernel" : "noise_blocks_u16_any_kernel");
    const long lanes = vec ? (long)nbx * (block * spp / 8) : (long)nbx * spp;
    const int gx = (int)((lanes + kBlock - 1) / kBlock);
    long gy = (long)ctx->cu_count * kPerCu / gx;
    if (gy < 1) gy = 1;
    if (gy > nby) gy = nby;
    if (gy > 65535) gy = 65535;
    const dim3 grid(gx, (unsigned)gy), wg(kBlock);
#define OIP_NOISE_LAUNCH(S, Bk)                                                                                                                   \
    hipLaunchKernelGGL((noise_blocks_u16_kernel<S, Bk>), grid, wg, 0, ctx->stream, d_src, pitch, nbx, nby, vmin, vmax, level_shift, d_keys, \
                       key_pitch, key_plane_stride)
    if (vec) {
        if (spp == 1 && block == 8) OIP_NOISE_LAUNCH(1, 8);
        else if (spp == 1) OIP_NOISE_LAUNCH(1, 16);
        else if (block == 8) OIP_NOISE_LAUNCH(4, 8);
        else OIP_NOISE_LAUNCH(4, 16);
    } else if (block == 8) {
        hipLaunchKernelGGL(noise_blocks_u16_any_kernel<8>, grid, wg, 0, ctx->stream, d_src, pitch, nbx, nby, spp, vmin, vmax, level_shift, d_keys,
                           key_pitch, key_plane_stride);
    } else {
        hipLaunchKernelGGL(noise_blocks_u16_any_kernel<16>, grid, wg, 0, ctx->stream, d_src, pitch, nbx, nby, spp, vmin, vmax, level_shift, d_keys,
                           key_pitch, key_plane_stride);
    }
#undef OIP_NOISE_LAUNCH
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}
