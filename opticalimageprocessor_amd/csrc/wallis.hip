// wallis.hip -- the two full-size passes of the Wallis filter ("dodging", `oip wallis`) on gfx950: the moments n, S1, S2 of every
// B x B block of a u16 raster, and the point transform out = (G v + 256 O + 32768) >> 16 with G and O interpolated bilinearly
// between the nodes at the blocks' centres.  The step between them (moments -> node gains and offsets) is host code:
// oip_wallis_fit in host.cpp.  The reference has no counterpart.  include/oip_c.h states every byte.
//
// Moments.  HBM-bound, read-only: 2 B per sample in, 24 B per block and channel out.  The layout is noise.hip's: a lane owns one
// 16-byte vector (8 samples: 2 pixels at spp 4) of each line of a block line, adjacent lanes read adjacent 16 bytes, and
// V = B * spp / 8 adjacent lanes share a block (4 .. 128).  A lane keeps n and S1 of its share in 32 bits (256 lines * 8 samples *
// 65535 < 2^27) and S2 in 64.  The V partial sums meet in a butterfly of wave shuffles; with V = 128 (spp 4, B 256 alone) a block
// spans two waves, whose totals meet in LDS; at spp 4, B 128 it is one whole wave.  A workgroup of 256 lanes holds whole blocks (V divides 256), the first lane of a
// block STORES its 3 * spp entries: no atomics, and nothing depends on the launch geometry.  The block's S1 fits 32 bits
// (65536 * 65535 < 2^32).  grid.y walks the block lines with a stride of gridDim.y.  The last vector of a line that is no
// multiple of 8 samples is read sample by sample: nothing outside the window is touched.
//
// Apply.  2 B in, 2 B out per sample; bound by integer arithmetic, not by HBM (profiles/wallis_speed.md).  A workgroup owns 256
// vectors and walks consecutive rounds of 8 lines.  Per round a lane issues its 8 loads, then stage 1: lane i < 144 owns one
// (node column, table, channel) of the node columns the workgroup's pixels lie between (at most 66 columns at spp 1, 18 at spp
// 4), keeps its two node lines in registers (read again every B lines) and writes the value interpolated along the strip for each
// line into one half of a double-buffered LDS table; one barrier per round.  Stage 2: a lane reads the values of its two node
// columns (all samples of a vector share them: B / 2 pixels are a multiple of a vector's), forms each channel's interpolation
// across the line at its first pixel and steps it per pixel, and transforms.  The gain's interpolation fits 32 bits (G <= 2^20,
// t <= 256: below 2^29), the offset's (|O| < 2^29) takes two 32 x 32 -> 64-bit products per channel and line, the transform one
// per sample and 32-bit arithmetic from there.  The three counters of a lane meet in LDS and a workgroup adds each to HBM once.
//
// Anything the vector forms cannot take (a pitch or a line that is not a multiple of 8 samples, a base that is not on a 16-byte
// boundary) goes to the plain kernels: 2-byte accesses, everything in 64-bit integers as the header writes it, the same bytes.
#include "oip_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kPerCu = 8;                    // workgroups per CU over the whole grid
constexpr int kLines = 8;                    // lines a lane has in flight
constexpr int kMaxE = 144;                   // values of stage 1 per line: node columns * 2 tables * spp

using u64 = unsigned long long;

// ---- moments -----------------------------------------------------------------------------------------------------------------
// the samples i < lim of one vector into the lane's sums; sample i belongs to channel i % SPP
template <int SPP>
__device__ __forceinline__ void moments_add(const uint4 &v, int lim, unsigned vmin, unsigned vspan, unsigned n[SPP], unsigned s1[SPP], u64 s2[SPP])
{
    const unsigned d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const unsigned u = (i & 1) ? d[i >> 1] >> 16 : d[i >> 1] & 0xffffu;
        const bool ok = u - vmin <= vspan && i < lim;                    // vmin <= u <= vmax, unsigned
        const unsigned t = ok ? u : 0u;
        const int c = SPP == 4 ? (i & 3) : 0;
        n[c] += ok ? 1u : 0u;
        s1[c] += t;
        s2[c] += (u64)(t * t);                                           // t < 2^16: the 32-bit product is exact
    }
}

template <int SPP, int B>
__global__ __launch_bounds__(kBlock) void block_moments_u16_kernel(const uint16_t *__restrict__ img, long pitch, int w, long rows, long nby, unsigned vmin,
                                                                   unsigned vspan, u64 *__restrict__ acc, long acc_pitch, size_t plane)
{
    constexpr int V = B * SPP / 8;                           // lanes (16-byte vectors) per block
    constexpr int VW = V < 64 ? V : 64;                      // ... of them in one wave
    constexpr int C = SPP;
    const long line = (long)w * SPP;                         // samples of a line
    const int nvec = (int)((line + 7) / 8), gw = (w + B - 1) / B;
    const int vx = blockIdx.x * kBlock + threadIdx.x;
    const bool active = vx < nvec;                           // (an inactive lane loads nothing and still takes part in the shuffles)
    const bool whole = (long)vx * 8 + 8 <= line;             // the vector lies inside the line
    const int lim = active ? (int)(line - (long)vx * 8 < 8 ? line - (long)vx * 8 : 8) : 0;
    const int bx = vx / V;
    for (long by = blockIdx.y; by < nby; by += gridDim.y) {
        const int nl = rows - by * B < B ? (int)(rows - by * B) : B;
        unsigned n[C], s1[C];
        u64 s2[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            n[c] = 0u; s1[c] = 0u; s2[c] = 0ull;
        }
        if (active) {
            const uint16_t *src = img + by * B * pitch + (long)vx * 8;
            for (int h = 0; h < nl; h += kLines) {
                uint4 v[kLines];
#pragma unroll
                for (int j = 0; j < kLines; ++j) {
                    v[j] = make_uint4(0u, 0u, 0u, 0u);
                    if (h + j < nl) {
                        const uint16_t *l = src + (long)(h + j) * pitch;
                        if (whole) {
                            v[j] = *reinterpret_cast<const uint4 *>(l);
                        } else {
                            unsigned t[8];
#pragma unroll
                            for (int i = 0; i < 8; ++i) t[i] = i < lim ? (unsigned)l[i] : 0u;
                            v[j] = make_uint4(t[0] | t[1] << 16, t[2] | t[3] << 16, t[4] | t[5] << 16, t[6] | t[7] << 16);
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < kLines; ++j)
                    if (h + j < nl) {
                        if (whole) moments_add<SPP>(v[j], 8, vmin, vspan, n, s1, s2);
                        else moments_add<SPP>(v[j], lim, vmin, vspan, n, s1, s2);
                    }
            }
        }
#pragma unroll
        for (int m = 1; m < VW; m <<= 1) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                n[c] += __shfl_xor(n[c], m);
                s1[c] += __shfl_xor(s1[c], m);
                s2[c] += __shfl_xor(s2[c], m);
            }
        }
        u64 *out = acc + by * acc_pitch + bx;
        if constexpr (V <= 64) {
            if (active && vx % V == 0 && bx < gw) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    out[(size_t)(0 * C + c) * plane] = n[c];
                    out[(size_t)(1 * C + c) * plane] = s1[c];
                    out[(size_t)(2 * C + c) * plane] = s2[c];
                }
            }
        } else {
            // a block is two whole waves, 2 k and 2 k + 1 of the workgroup: their totals meet in LDS (the other instantiations hold none)
            __shared__ u64 sh[kBlock / 64][3 * C];
            const int wave = threadIdx.x >> 6;
            if ((threadIdx.x & 63) == 0) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    sh[wave][0 * C + c] = n[c];
                    sh[wave][1 * C + c] = s1[c];
                    sh[wave][2 * C + c] = s2[c];
                }
            }
            __syncthreads();
            if ((threadIdx.x & 127) == 0 && active && bx < gw) {
#pragma unroll
                for (int k = 0; k < 3 * C; ++k) out[(size_t)k * plane] = sh[wave][k] + sh[wave + 1][k];
            }
            __syncthreads();                                 // the next block line writes sh again
        }
    }
}

// any pitch / alignment: a lane owns one block and channel
__global__ __launch_bounds__(kBlock) void block_moments_u16_any_kernel(const uint16_t *__restrict__ img, long pitch, int w, long rows, long nby, int spp, int B,
                                                                       unsigned vmin, unsigned vspan, u64 *__restrict__ acc, long acc_pitch, size_t plane)
{
    const int gw = (w + B - 1) / B;
    const long i = (long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (long)gw * spp) return;
    const int bx = (int)(i / spp), c = (int)(i % spp);
    const int cw = w - bx * B < B ? w - bx * B : B;
    for (long by = blockIdx.y; by < nby; by += gridDim.y) {
        const int nl = rows - by * B < B ? (int)(rows - by * B) : B;
        const uint16_t *s = img + by * B * pitch + (long)bx * B * spp + c;
        u64 n = 0ull, s1 = 0ull, s2 = 0ull;
        for (int j = 0; j < nl; ++j) {
            const uint16_t *l = s + (long)j * pitch;
            for (int x = 0; x < cw; ++x) {
                const unsigned u = l[x * spp];
                if (u - vmin <= vspan) {
                    n += 1ull;
                    s1 += u;
                    s2 += (u64)(u * u);
                }
            }
        }
        u64 *out = acc + by * acc_pitch + bx;
        out[(size_t)(0 * spp + c) * plane] = n;
        out[(size_t)(1 * spp + c) * plane] = s1;
        out[(size_t)(2 * spp + c) * plane] = s2;
    }
}

// ---- apply -------------------------------------------------------------------------------------------------------------------
// the node below position p of an axis of n nodes B = 1 << lb apart, the first at B / 2 (include/oip_c.h); >> floors
__device__ __forceinline__ long node_below(long p, int lb, long n)
{
    const long k = (p - (1L << lb >> 1)) >> lb, top = n - 2 > 0 ? n - 2 : 0;
    return k < 0 ? 0 : k > top ? top : k;
}
// ... and the weight t in 0..B of the node above it
__device__ __forceinline__ int node_weight(long p, long k, int lb)
{
    const long t = p - (1L << lb >> 1) - (k << lb);
    return t < 0 ? 0 : t > (1L << lb) ? (1 << lb) : (int)t;
}
__device__ __forceinline__ long long node_mix(long long a, long long b, int t, int lb) { return (a * ((1 << lb) - t) + b * t + (1 << lb >> 1)) >> lb; }

// out of one sample; the lane's three counters
__device__ __forceinline__ unsigned wallis_sample(unsigned v, long long G, long long O, unsigned vmin, unsigned vspan, unsigned cmax, unsigned cnt[3])
{
    if (v - vmin > vspan) return v;                                     // no data and saturation pass through
    const long long q = (G * (long long)v + 256 * O + 32768) >> 16;
    cnt[0] += 1u;
    if (q < (long long)vmin) {
        cnt[1] += 1u;
        return vmin;
    }
    if (q > (long long)cmax) {
        cnt[2] += 1u;
        return cmax;
    }
    return (unsigned)q;
}

// the same with G in 0..2^20 and |O| < 2^29 as 32-bit values.  With S = G v + 32768 (below 2^37) and 256 O a multiple of 256,
// floor((S + 256 O) / 65536) = floor((floor(S / 256) + O) / 256): one 32 x 32 -> 64-bit multiply-add, then 32-bit arithmetic
// (S >> 8 < 2^29, the sum below 2^30 in magnitude)
__device__ __forceinline__ unsigned wallis_sample32(unsigned v, unsigned G, int O, unsigned vmin, unsigned vspan, unsigned cmax, unsigned cnt[3])
{
    const bool valid = v - vmin <= vspan;
    const unsigned s8 = (unsigned)(((unsigned long long)G * v + 32768ull) >> 8);
    const int q = ((int)s8 + O) >> 8;
    const bool low = valid && q < (int)vmin, high = valid && q > (int)cmax;
    cnt[0] += valid ? 1u : 0u;
    cnt[1] += low ? 1u : 0u;
    cnt[2] += high ? 1u : 0u;
    const unsigned r = (unsigned)min(max(q, (int)vmin), (int)cmax);
    return valid ? r : v;                                               // no data and saturation pass through
}

// the three counters of a workgroup into d_stats; every lane of the workgroup arrives here
__device__ __forceinline__ void wallis_flush(const u64 cnt[3], u64 *__restrict__ stats)
{
    __shared__ u64 tot[3];
    if (threadIdx.x < 3) tot[threadIdx.x] = 0ull;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (cnt[k]) atomicAdd(&tot[k], cnt[k]);
    __syncthreads();
    if (stats && threadIdx.x < 3 && tot[threadIdx.x]) atomicAdd(stats + threadIdx.x, tot[threadIdx.x]);
}

// lines of W * SPP samples, a multiple of 8, src and dst on 16-byte boundaries.  Workgroup (x, y) owns the vectors 256 x .. 256 x +
// 255 of `chunk` consecutive rounds of kLines lines.
template <int SPP>
__global__ __launch_bounds__(kBlock) void wallis_apply_u16_kernel(const uint16_t *src, uint16_t *dst, long row0, long rows, long chunk, int W, int lb,
                                                                  const int32_t *__restrict__ gain, const int32_t *__restrict__ offset, int gw, long gh,
                                                                  unsigned vmin, unsigned vspan, unsigned cmax, u64 *__restrict__ stats)
{
    constexpr int PPV = 8 / SPP;                             // pixels per vector
    __shared__ int sh[2][kLines][kMaxE];                     // [round & 1][line][(column * 2 + table) * SPP + channel]
    const int B = 1 << lb, half = B >> 1;
    const long line = (long)W * SPP;
    const int nvec = (int)(line / 8);
    const int vx0 = blockIdx.x * kBlock, vx = vx0 + threadIdx.x;
    const bool active = vx < nvec;
    // the node columns the workgroup's pixels lie between: ka .. kb, at most 2048 / (SPP * B) + 2 of them
    const int pa = vx0 * PPV;
    const int pb = (vx0 + kBlock) * PPV - 1 < W - 1 ? (vx0 + kBlock) * PPV - 1 : W - 1;
    const int ka = (int)node_below(pa, lb, gw);
    const int kl = (int)node_below(pb, lb, gw);
    const int kb = kl + 1 < gw - 1 ? kl + 1 : gw - 1;
    const int ne = (kb - ka + 1) * 2 * SPP;                  // <= kMaxE
    // stage 1: lane idx < ne owns one (column, table, channel) of the workgroup; it keeps the two nodes its lines lie between in
    // registers and reads them again only when a line passes a node (every B lines)
    const int idx = threadIdx.x;
    const bool lister = idx < ne;
    const int32_t *T = (((idx / SPP) & 1) ? offset : gain) + (long)(ka + (lister ? idx / (2 * SPP) : 0)) * SPP + idx % SPP;
    const long node_line = (long)gw * SPP;
    long kc = -1;
    int na = 0, nb = 0;
    // stage 2: the lane's two node columns; the weight of its first pixel and the step to the next (0 where the table is constant,
    // else 1: B / 2 pixels are a multiple of a vector's, so a vector never straddles the first or last node)
    const int px0 = (active ? vx : vx0) * PPV;
    const int k0 = (int)node_below(px0, lb, gw), k1 = k0 + 1 < gw - 1 ? k0 + 1 : gw - 1;
    const int e0 = (k0 - ka) * 2 * SPP, e1 = (k1 - ka) * 2 * SPP;
    const int t0 = node_weight(px0, k0, lb), dt = node_weight(px0 + 1, k0, lb) - t0;
    unsigned cnt[3] = {0u, 0u, 0u};
    u64 total[3] = {0ull, 0ull, 0ull};
    const long rounds = (rows + kLines - 1) / kLines;
    const long r0 = (long)blockIdx.y * chunk, r1 = r0 + chunk < rounds ? r0 + chunk : rounds;
    for (long rd = r0; rd < r1; ++rd) {
        const long g0 = rd * kLines;
        const int nl = rows - g0 < kLines ? (int)(rows - g0) : kLines;
        int(*tab)[kMaxE] = sh[rd & 1];
        // the round's loads go out before stage 1
        const long at = g0 * line + (long)vx * 8;
        uint4 v[kLines];
        if (active) {
#pragma unroll
            for (int j = 0; j < kLines; ++j)
                if (j < nl) v[j] = *reinterpret_cast<const uint4 *>(src + at + (long)j * line);
        }
        if (lister) {
#pragma unroll
            for (int j = 0; j < kLines; ++j)
                if (j < nl) {
                    const long y = row0 + g0 + j;
                    const long ky = node_below(y, lb, gh);
                    if (ky != kc) {                          // (the same for every lane: it depends on the line alone)
                        const long ky1 = ky + 1 < gh - 1 ? ky + 1 : gh - 1;
                        kc = ky;
                        na = T[ky * node_line];
                        nb = T[ky1 * node_line];
                    }
                    const int ty = node_weight(y, ky, lb);
                    tab[j][idx] = (int)(((long long)na * (B - ty) + (long long)nb * ty + half) >> lb);     // between na and nb: it fits
                }
        }
        // one barrier per round: the other half of sh is written only behind the next one, when every lane has left this round
        __syncthreads();
        if (active) {
#pragma unroll
            for (int j = 0; j < kLines; ++j)
                if (j < nl) {
                    const unsigned d[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
                    unsigned o[8];
                    // per channel the interpolation before its division, at the first pixel, and its step per pixel:
                    // V0 (B - t) + V1 t + B / 2 with t = t0 + p dt.  G <= 2^20 and t <= 256: below 2^29; |O| < 2^29: below 2^38
                    unsigned gu[SPP], gs[SPP];
                    long long ou[SPP], os[SPP];
#pragma unroll
                    for (int c = 0; c < SPP; ++c) {
                        const unsigned G0 = (unsigned)tab[j][e0 + c], G1 = (unsigned)tab[j][e1 + c];
                        const int O0 = tab[j][e0 + SPP + c], O1 = tab[j][e1 + SPP + c];
                        gu[c] = G0 * (unsigned)(B - t0) + G1 * (unsigned)t0 + (unsigned)half;
                        gs[c] = dt ? G1 - G0 : 0u;           // (modulo 2^32: the sums below are exact)
                        ou[c] = (long long)O0 * (B - t0) + (long long)O1 * t0 + half;
                        os[c] = dt ? (long long)O1 - O0 : 0ll;
                    }
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int p = i / SPP, c = i % SPP;
                        const unsigned u = (i & 1) ? d[i >> 1] >> 16 : d[i >> 1] & 0xffffu;
                        const unsigned Gx = gu[c] >> lb;
                        const int Ox = (int)(ou[c] >> lb);
                        o[i] = wallis_sample32(u, Gx, Ox, vmin, vspan, cmax, cnt);
                        if (p + 1 < PPV) {                   // the channel's next pixel
                            gu[c] += gs[c];
                            ou[c] += os[c];
                        }
                    }
                    *reinterpret_cast<uint4 *>(dst + at + (long)j * line) =
                        make_uint4(o[0] | o[1] << 16, o[2] | o[3] << 16, o[4] | o[5] << 16, o[6] | o[7] << 16);
                }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {                        // (a lane's 64 samples of a round fit 32 bits, its share of a strip need not)
            total[k] += cnt[k];
            cnt[k] = 0u;
        }
    }
    wallis_flush(total, stats);
}

// any line length / alignment: a lane per sample, the header's formulas as they stand
__global__ __launch_bounds__(kBlock) void wallis_apply_u16_any_kernel(const uint16_t *src, uint16_t *dst, long row0, long rows, int W, int spp, int lb,
                                                                      const int32_t *__restrict__ gain, const int32_t *__restrict__ offset, int gw, long gh,
                                                                      unsigned vmin, unsigned vspan, unsigned cmax, u64 *__restrict__ stats)
{
    const long line = (long)W * spp, count = rows * line;
    unsigned cnt[3] = {0u, 0u, 0u};
    u64 total[3] = {0ull, 0ull, 0ull};
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < count; i += (long)gridDim.x * kBlock) {
        const long r = i / line;
        const int xs = (int)(i - r * line), x = xs / spp, c = xs - x * spp;
        const long y = row0 + r;
        const long ky = node_below(y, lb, gh), ky1 = ky + 1 < gh - 1 ? ky + 1 : gh - 1;
        const long kx = node_below(x, lb, gw), kx1 = kx + 1 < gw - 1 ? kx + 1 : gw - 1;
        const int ty = node_weight(y, ky, lb), tx = node_weight(x, kx, lb);
        long long V[2];
#pragma unroll
        for (int tab = 0; tab < 2; ++tab) {
            const int32_t *T = tab ? offset : gain;
            const long long a = node_mix(T[(ky * gw + kx) * spp + c], T[(ky1 * gw + kx) * spp + c], ty, lb);
            const long long b = node_mix(T[(ky * gw + kx1) * spp + c], T[(ky1 * gw + kx1) * spp + c], ty, lb);
            V[tab] = node_mix(a, b, tx, lb);
        }
        dst[i] = (uint16_t)wallis_sample(src[i], V[0], V[1], vmin, vspan, cmax, cnt);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            total[k] += cnt[k];
            cnt[k] = 0u;
        }
    }
    wallis_flush(total, stats);
}

int log2_block(int block) { return block == 32 ? 5 : block == 64 ? 6 : block == 128 ? 7 : block == 256 ? 8 : 0; }

}  // namespace

extern "C" int oip_block_moments_u16(oip_ctx *ctx, const uint16_t *d_src, long pitch, int w, long rows, int spp, int block, int valid_min, int valid_max,
                                     uint64_t *d_acc, long acc_pitch, size_t acc_plane_stride)
{
    OIP_CHECK_CTX(ctx);
    if (!log2_block(block) || (spp != 1 && spp != 4) || w < 0 || rows < 0 || pitch < (long)w * spp || !d_src || !d_acc || ((uintptr_t)d_src & 1) ||
        ((uintptr_t)d_acc & 7) || valid_min < 0 || valid_max > 65535 || valid_min > valid_max || acc_pitch < (w + block - 1) / block)
        return oip_fail(ctx, OIP_E_INVALID, "oip_block_moments_u16: bad argument");
    const int gw = (w + block - 1) / block;
    const long nby = (rows + block - 1) / block;
    if (gw == 0 || nby == 0) return OIP_OK;
    if (acc_plane_stride < (size_t)((nby - 1) * acc_pitch + gw)) return oip_fail(ctx, OIP_E_INVALID, "oip_block_moments_u16: the planes overlap");
    const unsigned vmin = (unsigned)valid_min, vspan = (unsigned)(valid_max - valid_min);
    const bool vec = pitch % 8 == 0 && ((uintptr_t)d_src & 15) == 0;
    OipProfScope prof(ctx, vec ? "block_moments_u16_kernel" : "block_moments_u16_any_kernel");
    const long lanes = vec ? ((long)w * spp + 7) / 8 : (long)gw * spp;
    const int gx = (int)((lanes + kBlock - 1) / kBlock);
    long gy = (long)ctx->cu_count * kPerCu / gx;
    if (gy < 1) gy = 1;
    if (gy > nby) gy = nby;
    if (gy > 65535) gy = 65535;
    const dim3 grid(gx, (unsigned)gy), wg(kBlock);
    u64 *acc = reinterpret_cast<u64 *>(d_acc);
#define OIP_MOMENTS_LAUNCH(S, Bk) \
    hipLaunchKernelGGL((block_moments_u16_kernel<S, Bk>), grid, wg, 0, ctx->stream, d_src, pitch, w, rows, nby, vmin, vspan, acc, acc_pitch, acc_plane_stride)
    if (vec) {
        if (spp == 1 && block == 32) OIP_MOMENTS_LAUNCH(1, 32);
        else if (spp == 1 && block == 64) OIP_MOMENTS_LAUNCH(1, 64);
        else if (spp == 1 && block == 128) OIP_MOMENTS_LAUNCH(1, 128);
        else if (spp == 1) OIP_MOMENTS_LAUNCH(1, 256);
        else if (block == 32) OIP_MOMENTS_LAUNCH(4, 32);
        else if (block == 64) OIP_MOMENTS_LAUNCH(4, 64);
        else if (block == 128) OIP_MOMENTS_LAUNCH(4, 128);
        else OIP_MOMENTS_LAUNCH(4, 256);
    } else {
        hipLaunchKernelGGL(block_moments_u16_any_kernel, grid, wg, 0, ctx->stream, d_src, pitch, w, rows, nby, spp, block, vmin, vspan, acc, acc_pitch,
                           acc_plane_stride);
    }
#undef OIP_MOMENTS_LAUNCH
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}

extern "C" int oip_wallis_apply_u16(oip_ctx *ctx, const uint16_t *d_src, uint16_t *d_dst, long row0, long rows, int W, long L, int spp, int block,
                                    const int32_t *d_gain_q16, const int32_t *d_offset_q8, int gw, long gh, int valid_min, int valid_max, int clamp_max,
                                    uint64_t *d_stats)
{
    OIP_CHECK_CTX(ctx);
    const int lb = log2_block(block);
    if (!lb || (spp != 1 && spp != 4) || W < 1 || L < 1 || row0 < 0 || rows < 0 || row0 > L || rows > L - row0 || !d_src || !d_dst || !d_gain_q16 ||
        !d_offset_q8 || ((uintptr_t)d_src & 1) || ((uintptr_t)d_dst & 1) || ((uintptr_t)d_gain_q16 & 3) || ((uintptr_t)d_offset_q8 & 3) ||
        ((uintptr_t)d_stats & 7) || valid_min < 0 || valid_max > 65535 || valid_min > valid_max || clamp_max < valid_min || clamp_max > 65535 ||
        gw != (W + block - 1) / block || gh != (L + block - 1) / block)
        return oip_fail(ctx, OIP_E_INVALID, "oip_wallis_apply_u16: bad argument");
    if (rows == 0) return OIP_OK;
    const unsigned vmin = (unsigned)valid_min, vspan = (unsigned)(valid_max - valid_min), cmax = (unsigned)clamp_max;
    const long line = (long)W * spp;
    const bool vec = line % 8 == 0 && (((uintptr_t)d_src | (uintptr_t)d_dst) & 15) == 0;
    OipProfScope prof(ctx, vec ? "wallis_apply_u16_kernel" : "wallis_apply_u16_any_kernel");
    u64 *stats = reinterpret_cast<u64 *>(d_stats);
    const dim3 wg(kBlock);
    if (vec) {
        const int gx = (int)((line / 8 + kBlock - 1) / kBlock);
        const long rounds = (rows + kLines - 1) / kLines;
        long gy = (long)ctx->cu_count * kPerCu / gx;
        if (gy < 1) gy = 1;
        if (gy > rounds) gy = rounds;
        if (gy > 65535) gy = 65535;
        const long chunk = (rounds + gy - 1) / gy;             // consecutive rounds per workgroup
        const dim3 grid(gx, (unsigned)((rounds + chunk - 1) / chunk));
        if (spp == 1)
            hipLaunchKernelGGL(wallis_apply_u16_kernel<1>, grid, wg, 0, ctx->stream, d_src, d_dst, row0, rows, chunk, W, lb, d_gain_q16, d_offset_q8, gw, gh,
                               vmin, vspan, cmax, stats);
        else
            hipLaunchKernelGGL(wallis_apply_u16_kernel<4>, grid, wg, 0, ctx->stream, d_src, d_dst, row0, rows, chunk, W, lb, d_gain_q16, d_offset_q8, gw, gh,
                               vmin, vspan, cmax, stats);
    } else {
        long g = (rows * line + kBlock - 1) / kBlock;
        const long cap = (long)ctx->cu_count * kPerCu;
        if (g > cap) g = cap;
        hipLaunchKernelGGL(wallis_apply_u16_any_kernel, dim3((unsigned)g), wg, 0, ctx->stream, d_src, d_dst, row0, rows, W, spp, lb, d_gain_q16, d_offset_q8,
                           gw, gh, vmin, vspan, cmax, stats);
    }
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}
