// convolve.hip -- fixed-point 2-D convolution of u16 rasters on gfx950: the MTF-compensation filter of `oip mtfc`.  The
// reference has no counterpart.  include/oip_c.h states the arithmetic (oip_convolve_u16); tests/_mtfc_ref.py restates it.
//
//   out = clamp((sum_{j,i} taps[j][i] * n'(j,i) + 2048) >> 12, valid_min, 65535)      Q12 taps, correlation form,
//                                                                                     replicate border, no-data rules
//
// Everything is integer and exact.  sum |taps| <= 32767 (host-checked) bounds |acc + 2048| by 32767 * 65535 + 2048
// = 2 147 387 393 < 2^31, so the sum lives in one int32; a tap (|t| < 2^15) and a sample (< 2^16) are both 24-bit
// operands, so a multiply-add is ONE full-rate v_mad_i32_i24 (a plain 32-bit multiply is quarter rate).
//
// Layout / mapping.  Lines are handled in SAMPLE units (Ws = W * spp; the channel of sample s is s % spp, its pixel s / spp;
// a horizontal neighbour is spp samples away).  A block of 256 lanes owns a tile of kTileW = 512 samples x kTileH = 16
// lines.  The tile plus its halo (ry lines above and below, rx * spp samples left and right rounded up to 8 = HP) goes to
// LDS once, in 16-byte chunks: an aligned global_load_dwordx4 where the chunk lies inside the line, eight clamped 2-byte loads
// where it crosses the image border (pixel index clamped, channel kept) -- the replicate border costs nothing in the
// arithmetic.  Lines are clamped the same way and fetched from the resident window [src_row0, src_row0 + src_rows).  Only
// the lines and chunks that the tile's output needs are touched (a last tile has fewer lines; the window holds no more).
// Then a lane owns ONE aligned 16-byte store: 8 consecutive samples of a line; a wave takes a line, the four waves every
// fourth line of the tile.  Per kernel line j the lane reads its 8 + 2 HP samples from LDS as ds_read_b128 (3 at spp 1, up
// to 5 at spp 4; lanes read consecutive 16 bytes: conflict-free), unpacks them once and runs KX * 8 multiply-adds with
// compile-time register indices; the taps come from the kernel arguments through scalar loads.  KX and spp are template
// parameters (they fix the register window), ky is a run-time loop.
//
// No data.  n' = n < valid_min ? centre : n  costs a compare and a select per multiply-add, and real images hold no-data only
// in the black borders that prestitch and the aligner leave.  While a tile is filled each lane keeps the packed minimum of
// what it loads (v_pk_min_u16, one per dword); the barrier behind the fill ORs "some sample is below valid_min" over the
// block, and a tile without such a sample -- always so at valid_min 0 -- runs the loop without the two extra instructions.
// Both forms give the same bytes.
//
// A line that is not a multiple of 8 samples, or bases that are not 16-byte aligned, take the same kernel with ALIGNED =
// false: 2-byte loads into the same LDS image, the same arithmetic, 2-byte stores.
//
// One tile per block, no grid-stride loop: the grid is tiles_x * tiles_y in x (368 750 blocks at 30000 x 100000).  LDS:
// (16 + 8) lines x (512 + 2 HP) samples x 2 bytes <= 26 112 bytes per block.
#include "oip_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTileW = 512;                  // samples: 64 lanes x 8
constexpr int kTileH = 16;                   // lines
constexpr int kMaxK = 9;
constexpr int kMaxRows = kTileH + kMaxK - 1;

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

struct ConvArgs {
    const uint16_t *src;
    uint16_t *dst;
    long Ws, L;                              // samples per line, lines of the raster
    long src_row0, out_row0, out_rows;
    int W;                                   // pixels per line
    int ky;
    int vmin;
    int tiles_x;
    int taps[kMaxK * kMaxK];                 // row-major ky x KX
};

__device__ __forceinline__ unsigned pk_min_u16(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(us2, a), __builtin_bit_cast(us2, b)));
}

// the 8 output samples of one lane on one line.  win: the lane's first LDS sample of the tile's LDS line `lr`
// (= output line - first output line of the tile; kernel line j reads LDS line lr + j)
template <int SPP, int KX, bool MASK>
__device__ __forceinline__ uint4 conv_lane(const uint16_t *win, int pitch, int ky, int vmin, const int *__restrict__ taps)
{
    constexpr int RX = KX / 2, HP = (RX * SPP + 7) / 8 * 8, NW = 8 + 2 * HP;
    const int ry = ky >> 1;
    int ctr[8], acc[8];
    {
        const uint4 c = *reinterpret_cast<const uint4 *>(win + ry * pitch + HP);
        ctr[0] = c.x & 0xffffu; ctr[1] = c.x >> 16; ctr[2] = c.y & 0xffffu; ctr[3] = c.y >> 16;
        ctr[4] = c.z & 0xffffu; ctr[5] = c.z >> 16; ctr[6] = c.w & 0xffffu; ctr[7] = c.w >> 16;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 2048;
    for (int j = 0; j < ky; ++j) {
        int w[NW];
#pragma unroll
        for (int c = 0; c < NW / 8; ++c) {
            const uint4 q = *reinterpret_cast<const uint4 *>(win + j * pitch + c * 8);
            w[c * 8 + 0] = q.x & 0xffffu; w[c * 8 + 1] = q.x >> 16; w[c * 8 + 2] = q.y & 0xffffu; w[c * 8 + 3] = q.y >> 16;
            w[c * 8 + 4] = q.z & 0xffffu; w[c * 8 + 5] = q.z >> 16; w[c * 8 + 6] = q.w & 0xffffu; w[c * 8 + 7] = q.w >> 16;
        }
#pragma unroll
        for (int i = 0; i < KX; ++i) {
            const int t = taps[j * KX + i];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                int n = w[HP + k + (i - RX) * SPP];
                if (MASK) n = n < vmin ? ctr[k] : n;
                acc[k] = __mul24(t, n) + acc[k];
            }
        }
    }
    unsigned o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        int v = acc[k] >> 12;                                    // arithmetic shift: floor
        v = v < vmin ? vmin : (v > 65535 ? 65535 : v);
        if (MASK) v = ctr[k] < vmin ? ctr[k] : v;
        o[k] = (unsigned)v;
    }
    return make_uint4(o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16));
}

// ALIGNED requires: Ws % 8 == 0, src and dst 16-byte aligned
template <int SPP, int KX, bool ALIGNED>
__global__ __launch_bounds__(kBlock) void convolve_u16_kernel(const ConvArgs a)
{
    constexpr int RX = KX / 2, HP = (RX * SPP + 7) / 8 * 8, PITCH = kTileW + 2 * HP, NCH = PITCH / 8, SH = SPP == 4 ? 2 : 0;
    __shared__ uint4 tile4[kMaxRows * NCH];
    const int ry = a.ky >> 1;
    const long ty = (long)blockIdx.x / a.tiles_x;
    const int tx = (int)((long)blockIdx.x - ty * a.tiles_x);
    const long y0 = a.out_row0 + ty * kTileH;                    // first output line of the tile (global)
    const long left = a.out_row0 + a.out_rows - y0;
    const int rows = left < kTileH ? (int)left : kTileH;         // output lines of the tile, >= 1
    const long x0 = (long)tx * kTileW;                           // first output sample of the tile
    const long wleft = a.Ws - x0;
    const int cols = wleft < kTileW ? (int)wleft : kTileW;       // output samples of the tile, >= 1
    const int nch = (cols + 2 * HP + 7) >> 3;                    // chunks of an LDS line that are read later
    const int nfill = (rows + 2 * ry) * NCH;

    // ---- the tile and its halo -> LDS -------------------------------------------------------------------------------------
    unsigned lo = 0xffffffffu;
    for (int e = threadIdx.x; e < nfill; e += kBlock) {
        const int r = e / NCH, c = e - r * NCH;
        if (c >= nch) continue;
        long v = y0 - ry + r;
        v = v < 0 ? 0 : (v > a.L - 1 ? a.L - 1 : v);             // inside [src_row0, src_row0 + src_rows): host-checked
        const uint16_t *line = a.src + (v - a.src_row0) * a.Ws;
        const long s = x0 - HP + c * 8;
        uint4 q;
        if (ALIGNED && s >= 0 && s + 8 <= a.Ws) {
            q = *reinterpret_cast<const uint4 *>(line + s);
        } else {
            unsigned t[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const long ss = s + k;
                long p = ss >> SH;                               // arithmetic shift: the floor for ss < 0 as well
                p = p < 0 ? 0 : (p > a.W - 1 ? a.W - 1 : p);
                t[k] = line[(p << SH) + (ss & (SPP - 1))];
            }
            q = make_uint4(t[0] | (t[1] << 16), t[2] | (t[3] << 16), t[4] | (t[5] << 16), t[6] | (t[7] << 16));
        }
        lo = pk_min_u16(pk_min_u16(lo, q.x), pk_min_u16(q.y, pk_min_u16(q.z, q.w)));
        tile4[e] = q;
    }
    const int nodata = (int)(lo & 0xffffu) < a.vmin || (int)(lo >> 16) < a.vmin;
    const bool mask = __syncthreads_or(nodata) != 0;

    // ---- a wave per line, a lane per 16 bytes of it -----------------------------------------------------------------------
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane * 8 >= cols) return;
    const uint16_t *tile = reinterpret_cast<const uint16_t *>(tile4);
    for (int r = wave; r < rows; r += kWaves) {
        const uint16_t *win = tile + r * PITCH + lane * 8;
        const uint4 o = mask ? conv_lane<SPP, KX, true>(win, PITCH, a.ky, a.vmin, a.taps)
                             : conv_lane<SPP, KX, false>(win, PITCH, a.ky, a.vmin, a.taps);
        uint16_t *out = a.dst + (y0 - a.out_row0 + r) * a.Ws + x0 + lane * 8;
        if (ALIGNED) {
            *reinterpret_cast<uint4 *>(out) = o;                 // cols % 8 == 0: the whole chunk is inside the line
        } else {
            const unsigned d[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (lane * 8 + k < cols) out[k] = (uint16_t)(d[k >> 1] >> ((k & 1) * 16));
        }
    }
}

template <int SPP, bool ALIGNED>
void launch_kx(int kx, unsigned blocks, hipStream_t stream, const ConvArgs &a)
{
    switch (kx) {
        case 1: hipLaunchKernelGGL((convolve_u16_kernel<SPP, 1, ALIGNED>), dim3(blocks), dim3(kBlock), 0, stream, a); break;
        case 3: hipLaunchKernelGGL((convolve_u16_kernel<SPP, 3, ALIGNED>), dim3(blocks), dim3(kBlock), 0, stream, a); break;
        case 5: hipLaunchKernelGGL((convolve_u16_kernel<SPP, 5, ALIGNED>), dim3(blocks), dim3(kBlock), 0, stream, a); break;
        case 7: hipLaunchKernelGGL((convolve_u16_kernel<SPP, 7, ALIGNED>), dim3(blocks), dim3(kBlock), 0, stream, a); break;
        default: hipLaunchKernelGGL((convolve_u16_kernel<SPP, 9, ALIGNED>), dim3(blocks), dim3(kBlock), 0, stream, a); break;
    }
}

}  // namespace

extern "C" int oip_convolve_u16(oip_ctx *ctx, const uint16_t *d_src, long src_row0, long src_rows, uint16_t *d_dst, long out_row0, long out_rows,
                                int W, long L, int spp, const int32_t *taps, int ky, int kx, int valid_min)
{
    OIP_CHECK_CTX(ctx);
    if (!d_src || !d_dst || !taps || ((uintptr_t)d_src & 1) || ((uintptr_t)d_dst & 1) || (spp != 1 && spp != 4) || W < 1 || L < 1 ||
        ky < 1 || kx < 1 || ky > kMaxK || kx > kMaxK || ky % 2 == 0 || kx % 2 == 0 || valid_min < 0 || valid_min > 65535 || src_row0 < 0 ||
        src_rows < 0 || out_row0 < 0 || out_rows < 0 || out_rows > L || out_row0 > L - out_rows)
        return oip_fail(ctx, OIP_E_INVALID, "oip_convolve_u16: bad argument");
    if ((const uint16_t *)d_dst == d_src) return oip_fail(ctx, OIP_E_INVALID, "oip_convolve_u16: the call is not in place (d_dst == d_src)");
    long sum = 0;
    for (int i = 0; i < ky * kx; ++i) sum += taps[i] < 0 ? -(long)taps[i] : (long)taps[i];
    if (sum > 32767) return oip_fail(ctx, OIP_E_INVALID, "oip_convolve_u16: sum |taps| = %ld above 32767 (the int32 accumulator)", sum);
    if (out_rows == 0) return OIP_OK;
    const int ry = ky / 2;
    const long first = out_row0 - ry < 0 ? 0 : out_row0 - ry;
    const long last = out_row0 + out_rows - 1 + ry > L - 1 ? L - 1 : out_row0 + out_rows - 1 + ry;
    if (first < src_row0 || last >= src_row0 + src_rows)
        return oip_fail(ctx, OIP_E_INVALID, "oip_convolve_u16: source lines [%ld, %ld] needed, [%ld, %ld) resident", first, last, src_row0,
                        src_row0 + src_rows);
    ConvArgs a;
    a.src = d_src;
    a.dst = d_dst;
    a.Ws = (long)W * spp;
    a.L = L;
    a.src_row0 = src_row0;
    a.out_row0 = out_row0;
    a.out_rows = out_rows;
    a.W = W;
    a.ky = ky;
    a.vmin = valid_min;
    const long tiles_x = (a.Ws + kTileW - 1) / kTileW, tiles_y = (out_rows + kTileH - 1) / kTileH;
    if (tiles_x * tiles_y >= (1L << 31)) return oip_fail(ctx, OIP_E_UNSUPPORTED, "oip_convolve_u16: more than 2^31 tiles in one call");
    a.tiles_x = (int)tiles_x;
    for (int i = 0; i < kMaxK * kMaxK; ++i) a.taps[i] = i < ky * kx ? taps[i] : 0;
    const bool aligned = a.Ws % 8 == 0 && ((uintptr_t)d_src & 15) == 0 && ((uintptr_t)d_dst & 15) == 0;
    const unsigned blocks = (unsigned)(tiles_x * tiles_y);
    OipProfScope prof(ctx, "convolve_u16_kernel");
    if (spp == 1) { if (aligned) launch_kx<1, true>(kx, blocks, ctx->stream, a); else launch_kx<1, false>(kx, blocks, ctx->stream, a); }
    else          { if (aligned) launch_kx<4, true>(kx, blocks, ctx->stream, a); else launch_kx<4, false>(kx, blocks, ctx->stream, a); }
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}
