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
// Layout / mapping: the tile, grid and LDS layout of oip_tile.h, with ry = ky / 2 and rx = KX / 2.  Per kernel line j the lane
// reads its 8 + 2 HP samples from LDS (3 ds_read_b128 at spp 1, up to 5 at spp 4), unpacks them once and runs KX * 8
// multiply-adds with compile-time register indices; the taps come from the kernel arguments through scalar loads.  KX and spp
// are template parameters (they fix the register window), ky is a run-time loop.
//
// No data.  n' = n < valid_min ? centre : n  costs a compare and a select per multiply-add, and real images hold no-data only
// in the black borders that prestitch and the aligner leave: only a tile that oip_tile_has_nodata() reports runs the loop with
// the two extra instructions.  Both forms give the same bytes.
#include "oip_tile.h"

namespace {

constexpr int kBlock = kOipTileBlock;
constexpr int kMaxK = 9;
constexpr int kMaxRows = kOipTileH + kMaxK - 1;

struct ConvArgs : OipTileArgs {
    int taps[kMaxK * kMaxK];                 // row-major ky x KX
    int ky;
};

// the 8 output samples of one lane on one line.  win: as oip_tile_lines() hands it over
template <int SPP, int KX, bool MASK>
__device__ __forceinline__ uint4 conv_lane(const uint16_t *win, int ky, int vmin, const int *__restrict__ taps)
{
    constexpr int RX = KX / 2, HP = oip_tile_hp(SPP, RX), PITCH = oip_tile_pitch(HP), NC = 1 + 2 * HP / 8;
    const int ry = ky >> 1;
    int ctr[8], acc[8];
    oip_unpack8(*reinterpret_cast<const uint4 *>(win + ry * PITCH + HP), ctr);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 2048;
    for (int j = 0; j < ky; ++j) {
        int w[NC][8];
#pragma unroll
        for (int c = 0; c < NC; ++c) oip_unpack8(*reinterpret_cast<const uint4 *>(win + j * PITCH + c * 8), w[c]);
#pragma unroll
        for (int i = 0; i < KX; ++i) {
            const int t = taps[j * KX + i];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int at = HP + k + (i - RX) * SPP;
                int n = w[at >> 3][at & 7];
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
    return oip_pack8(o);
}

template <int SPP, int KX, bool ALIGNED>
__global__ __launch_bounds__(kBlock) void convolve_u16_kernel(const ConvArgs a)
{
    constexpr int HP = oip_tile_hp(SPP, KX / 2);
    __shared__ uint4 tile4[kMaxRows * oip_tile_nch(HP)];
    const OipTile t = oip_tile_of(a, blockIdx.x, SPP, HP, a.ky >> 1);
    const bool mask = oip_tile_has_nodata(oip_tile_fill<SPP, HP, ALIGNED>(tile4, a, t, a.ky >> 1, OipTileEdge()), a.vmin);
    oip_tile_lines<HP, ALIGNED>(tile4, a, t, [&](const uint16_t *win, int) {
        return mask ? conv_lane<SPP, KX, true>(win, a.ky, a.vmin, a.taps) : conv_lane<SPP, KX, false>(win, a.ky, a.vmin, a.taps);
    });
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
    const char *fn = "oip_convolve_u16";
    if (!taps || ky < 1 || kx < 1 || ky > kMaxK || kx > kMaxK || ky % 2 == 0 || kx % 2 == 0) return oip_fail(ctx, OIP_E_INVALID, "%s: bad argument", fn);
    const OipTilePlan p = oip_tile_plan(d_src, src_row0, src_rows, d_dst, out_row0, out_rows, W, L, spp, valid_min, ky / 2, 1, W);
    if (const int rc = oip_tile_refusal(ctx, fn, p, OIP_TILE_IN_PLACE)) return rc;
    long sum = 0;
    for (int i = 0; i < ky * kx; ++i) sum += taps[i] < 0 ? -(long)taps[i] : (long)taps[i];
    if (sum > 32767) return oip_fail(ctx, OIP_E_INVALID, "%s: sum |taps| = %ld above 32767 (the int32 accumulator)", fn, sum);
    if (const int rc = oip_tile_refusal(ctx, fn, p)) return rc;
    if (!p.blocks) return OIP_OK;
    ConvArgs a;
    static_cast<OipTileArgs &>(a) = p.args;
    a.ky = ky;
    for (int i = 0; i < kMaxK * kMaxK; ++i) a.taps[i] = i < ky * kx ? taps[i] : 0;
    OipProfScope prof(ctx, "convolve_u16_kernel");
    if (spp == 1) { if (p.aligned) launch_kx<1, true>(kx, p.blocks, ctx->stream, a); else launch_kx<1, false>(kx, p.blocks, ctx->stream, a); }
    else          { if (p.aligned) launch_kx<4, true>(kx, p.blocks, ctx->stream, a); else launch_kx<4, false>(kx, p.blocks, ctx->stream, a); }
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}
