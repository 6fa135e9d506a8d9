// rescale.hip -- the device side of `oip rescale`: a u16 raster resampled to another pixel grid by a separable polyphase filter
// whose tables the host built (include/oip_c.h: oip_rescale_u16; tables: oip_rescale_taps, arithmetic: oip_rescaleplan.h).  The
// reference has no counterpart; the siblings are remap.hip (whole-pixel shifts) and warp.hip (a displacement field at unchanged size).
//
//   s' = s - 32768
//   v(y, xs)  = clamp((sum_k ty[y][k] s'(clampL(fy[y] + k), xs) + 8192) >> 14, -32768, 32767)
//   out(y, x) = clamp(((sum_k tx[x][k] v(y, clampW(fx[x] + k)) + 8192) >> 14) + 32768, 0, 65535)
//
// One launch per call, one kernel, exact integers: any tile and any cut into windows give the same bytes.
//
// Layout / mapping.  A workgroup of 256 lanes owns th x tw output pixels; the host plan (oip_rescale_tile) shrinks the tile with
// the ratio so that the LDS image stays below 40 KiB (four workgroups a CU).  Four stages, a barrier between them:
//   fill    the source region of the tile (sh lines x pitch samples) goes to LDS in 16-byte chunks: a global_load_dwordx4
//           where the chunk is aligned and inside the line, eight clamped 2-byte loads otherwise (the replicate border, and
//           every chunk of a raster whose lines or base are not multiples of 16 bytes).  LDS column 0 is the region's first
//           sample rounded down to a multiple of 8, so aligned chunks stay aligned.  The taps of the tile's columns go to LDS
//           too, transposed (tap k of consecutive columns in consecutive halfwords).
//   lines   a wave takes an output line, a lane two neighbouring samples of the region (one ds_read_b32 per tap and pair); the
//           line's taps are wave-uniform.  The clamped intermediate is written to LDS as u16 (v + 32768).
//   across  a lane takes an output pixel (all its channels: one ds_read_u16 or ds_read_b64 per tap) and four output lines, so
//           that a tap read from LDS serves four multiply-adds per channel; results go to the output tile in LDS.
//   store   the output tile leaves in 16-byte stores where the output lines and base allow it, in 2-byte stores otherwise.
// All operands are below 2^16: the products are v_mad_i32_i24's.  The sums run on s and v + 32768 as they lie in LDS, in
// unsigned 32-bit arithmetic; the bias 32768 * 16384 (the taps of a row sum to 16384) is taken off at the end, which is exact
// modulo 2^32 and the true sum fits 32 bits.
//
// No data (valid_min > 0).  `lines` keeps the minimum of what a sample's column segment holds and stores "below valid_min" as a
// byte beside the intermediate; `across` ORs the bytes along the row of taps; a flagged output sample takes the nearest source
// sample, which lies inside the region.  With valid_min == 0 the kernel is compiled without any of it.
//
// Tables are the caller's.  first[] is used relative to the tile's first entry and clamped into the region, source lines are
// clamped into the resident window: tables that oip_rescale_taps did not build give unspecified samples, never an access
// outside the rasters.  All offsets are 64 bit.
#include "oip_internal.h"
#include "oip_rescaleplan.h"
#include "oip_tile.h"

#include <type_traits>

namespace {

struct RescaleArgs {
    const uint16_t *src;                     // line src_row0 of the source
    uint16_t *dst;                           // line out_row0 of the output
    const int *fx, *fy;
    const int16_t *tx, *ty;
    long Ws, Wos;                            // samples of a source and of an output line
    long L, Lo;
    long row_lo, row_hi;                     // source lines a tile may read: the resident ones inside the image
    long src_row0, out_row0, out_rows;
    int W, Wo;
    int Kx, Ky, vmin;
    int tiles_x;
    int src_wide, dst_wide;                  // 16-byte loads / stores apply
    OipRescaleTile t;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

constexpr unsigned kBias = 32768u << 14;

// f(std::integral_constant<int, K>) for the row lengths that get a loop of their own, f(<0>) for the others
template <class F> __device__ __forceinline__ void oip_rescale_by_k(int K, F f)
{
    switch (K) {
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 6: f(std::integral_constant<int, 6>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        default: f(std::integral_constant<int, 0>{}); break;
    }
}

template <int SPP, bool NODATA>
__global__ __launch_bounds__(kOipRescaleBlock) void rescale_u16_kernel(const RescaleArgs a)
{
    extern __shared__ uint4 lds4[];
    const int pitch = a.t.pitch, th = a.t.th, tw = a.t.tw, tws = tw * SPP, Kx = a.Kx, Ky = a.Ky;
    uint16_t *S = reinterpret_cast<uint16_t *>(lds4);            // sh x pitch
    uint16_t *M = S + a.t.sh * pitch;                            // th x pitch
    uint16_t *O = M + th * pitch;                                // th x tws
    int16_t *TX = reinterpret_cast<int16_t *>(O + th * tws);     // Kx x tw
    int *FX = reinterpret_cast<int *>(TX + Kx * tw);             // tw
    uint8_t *F = reinterpret_cast<uint8_t *>(FX + tw);           // th x pitch (NODATA)

    const int tid = threadIdx.x;
    const long tyi = blockIdx.x / a.tiles_x;
    const int txi = (int)(blockIdx.x - tyi * a.tiles_x);
    const long y0 = a.out_row0 + tyi * th;
    const long yleft = a.out_row0 + a.out_rows - y0;
    const int rows = yleft < th ? (int)yleft : th;
    const int x0 = txi * tw;
    const int cols = a.Wo - x0 < tw ? a.Wo - x0 : tw;
    const int sy0 = a.fy[y0], sx0 = a.fx[x0];
    const long g0 = (long)sx0 * SPP;
    const int pad = a.src_wide ? (int)(g0 & 7) : 0;              // (two's complement: the floor modulus for g0 < 0 as well)
    const long gs0 = g0 - pad;                                   // the sample of the line that LDS column 0 holds

    // ---- fill
    for (int e = tid; e < cols * Kx; e += kOipRescaleBlock) {
        const int i = e / Kx, k = e - i * Kx;
        TX[k * tw + i] = a.tx[(long)x0 * Kx + e];
    }
    for (int i = tid; i < cols; i += kOipRescaleBlock) FX[i] = clampi(a.fx[x0 + i] - sx0, 0, a.t.sw - Kx);
    {
        const int nsr = clampi(a.fy[y0 + rows - 1] + Ky - sy0, Ky, a.t.sh);
        const int nss = pad + clampi(a.fx[x0 + cols - 1] + Kx - sx0, Kx, a.t.sw) * SPP;
        const int nch = (nss + 7) >> 3;
        for (int e = tid; e < nsr * nch; e += kOipRescaleBlock) {
            const int r = e / nch, c = e - r * nch;
            long line = (long)sy0 + r;
            line = line < a.row_lo ? a.row_lo : (line > a.row_hi ? a.row_hi : line);
            const uint16_t *p = a.src + (line - a.src_row0) * a.Ws;
            const long g = gs0 + c * 8;
            uint4 q;
            if (a.src_wide && g >= 0 && g + 8 <= a.Ws) {
                q = *reinterpret_cast<const uint4 *>(p + g);
            } else {
                unsigned v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const long s = g + k;
                    long px = SPP == 4 ? s >> 2 : s;             // arithmetic shift: the floor for s < 0 as well
                    px = px < 0 ? 0 : (px > a.W - 1 ? a.W - 1 : px);
                    v[k] = p[px * SPP + (s & (SPP - 1))];
                }
                q = oip_pack8(v);
            }
            lds4[(r * pitch >> 3) + c] = q;
        }
    }
    __syncthreads();

    // ---- lines
    {
        const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        const int npairs = pitch >> 1;
        const unsigned *S2 = reinterpret_cast<const unsigned *>(S);
        unsigned *M2 = reinterpret_cast<unsigned *>(M);
        // (K as a constant for the common rows of 4, 6 and 8 taps: the loop unrolls, LDS offsets become immediates and the
        // line's taps are fetched once)
        oip_rescale_by_k(Ky, [&](auto kc) {
            constexpr int KC = decltype(kc)::value;
            const int ky = KC ? KC : Ky;
            constexpr int UN = KC ? KC : 2;
            for (int r = wave; r < rows; r += kOipRescaleBlock / 64) {
                const long y = y0 + r;
                const int ry = clampi(a.fy[y] - sy0, 0, a.t.sh - Ky);
                const int16_t *tp = a.ty + y * Ky;
                for (int cp = lane; cp < npairs; cp += 64) {
                    unsigned acc0 = 0, acc1 = 0, lo = 0xffffffffu;
                    const unsigned *s = S2 + (ry * pitch >> 1) + cp;
#pragma unroll UN
                    for (int k = 0; k < ky; ++k) {
                        const unsigned v = s[k * (pitch >> 1)];
                        const int t = tp[k];
                        acc0 += (unsigned)__mul24(t, (int)(v & 0xffffu));
                        acc1 += (unsigned)__mul24(t, (int)(v >> 16));
                        if (NODATA) lo = oip_pk_min_u16(lo, v);
                    }
                    const int v0 = clampi(((int)(acc0 - kBias) + 8192) >> 14, -32768, 32767) + 32768;
                    const int v1 = clampi(((int)(acc1 - kBias) + 8192) >> 14, -32768, 32767) + 32768;
                    M2[(r * pitch >> 1) + cp] = (unsigned)v0 | ((unsigned)v1 << 16);
                    if (NODATA) {
                        const unsigned f0 = (int)(lo & 0xffffu) < a.vmin, f1 = (int)(lo >> 16) < a.vmin;
                        reinterpret_cast<uint16_t *>(F)[(r * pitch >> 1) + cp] = (uint16_t)(f0 | (f1 << 8));
                    }
                }
            }
        });
    }
    __syncthreads();

    // ---- across
    {
        const int ngroups = (rows + kOipRescaleLines - 1) / kOipRescaleLines;
        oip_rescale_by_k(Kx, [&](auto kc) {
            constexpr int KC = decltype(kc)::value;
            const int kx = KC ? KC : Kx;
            constexpr int UN = KC ? KC : 2;
            for (int it = tid; it < cols * ngroups; it += kOipRescaleBlock) {
                const int gq = it / cols, i = it - gq * cols;
                const int r0 = gq * kOipRescaleLines;
                const int base = pad + FX[i] * SPP;
                int rr[kOipRescaleLines];
#pragma unroll
                for (int u = 0; u < kOipRescaleLines; ++u) rr[u] = (r0 + u < rows ? r0 + u : rows - 1) * pitch + base;
                unsigned acc[kOipRescaleLines][SPP];
                unsigned flag[kOipRescaleLines][SPP];
#pragma unroll
                for (int u = 0; u < kOipRescaleLines; ++u)
#pragma unroll
                    for (int c = 0; c < SPP; ++c) acc[u][c] = 0, flag[u][c] = 0;
#pragma unroll UN
                for (int k = 0; k < kx; ++k) {
                    const int t = TX[k * tw + i];
#pragma unroll
                    for (int u = 0; u < kOipRescaleLines; ++u) {
                        if constexpr (SPP == 1) {
                            acc[u][0] += (unsigned)__mul24(t, (int)M[rr[u] + k]);
                            if (NODATA) flag[u][0] |= F[rr[u] + k];
                        } else {
                            const uint2 m = *reinterpret_cast<const uint2 *>(M + rr[u] + 4 * k);
                            acc[u][0] += (unsigned)__mul24(t, (int)(m.x & 0xffffu));
                            acc[u][1] += (unsigned)__mul24(t, (int)(m.x >> 16));
                            acc[u][2] += (unsigned)__mul24(t, (int)(m.y & 0xffffu));
                            acc[u][3] += (unsigned)__mul24(t, (int)(m.y >> 16));
                            if (NODATA) {
                                const unsigned f = *reinterpret_cast<const unsigned *>(F + rr[u] + 4 * k);
                                flag[u][0] |= f & 0xffu, flag[u][1] |= (f >> 8) & 0xffu, flag[u][2] |= (f >> 16) & 0xffu, flag[u][3] |= f >> 24;
                            }
                        }
                    }
                }
                int nx = 0;
                if (NODATA) nx = pad + clampi((int)(oip_rescale_nearest(a.W, a.Wo, x0 + i) - sx0), 0, a.t.sw - 1) * SPP;
#pragma unroll
                for (int u = 0; u < kOipRescaleLines; ++u) {
                    if (r0 + u >= rows) break;
                    int ny = 0;
                    if (NODATA) ny = clampi((int)(oip_rescale_nearest(a.L, a.Lo, y0 + r0 + u) - sy0), 0, a.t.sh - 1) * pitch;
#pragma unroll
                    for (int c = 0; c < SPP; ++c) {
                        int o = clampi((((int)(acc[u][c] - kBias) + 8192) >> 14) + 32768, 0, 65535);
                        if (NODATA && flag[u][c]) o = S[ny + nx + c];
                        O[(r0 + u) * tws + i * SPP + c] = (uint16_t)o;
                    }
                }
            }
        });
    }
    __syncthreads();

    // ---- store
    uint16_t *d = a.dst + (y0 - a.out_row0) * a.Wos + (long)x0 * SPP;
    const int cs = cols * SPP;
    if (a.dst_wide) {                                            // (Wos and tws are multiples of 8, so cs is one)
        const int nch = cs >> 3;
        for (int e = tid; e < rows * nch; e += kOipRescaleBlock) {
            const int r = e / nch, c = e - r * nch;
            *reinterpret_cast<uint4 *>(d + r * a.Wos + c * 8) = *reinterpret_cast<const uint4 *>(O + r * tws + c * 8);
        }
    } else {
        for (int e = tid; e < rows * cs; e += kOipRescaleBlock) {
            const int r = e / cs, c = e - r * cs;
            d[r * a.Wos + c] = O[r * tws + c];
        }
    }
}

}  // namespace

extern "C" int oip_rescale_u16(oip_ctx *ctx, const uint16_t *d_src, long src_row0, long src_rows, int W, long L, int spp, uint16_t *d_dst, long out_row0,
                               long out_rows, int Wo, long Lo, const int *d_first_x, const int16_t *d_taps_x, int Kx, const int *d_first_y,
                               const int16_t *d_taps_y, int Ky, int valid_min)
{
    OIP_CHECK_CTX(ctx);
    const char *fn = "oip_rescale_u16";
    auto bad_k = [](int K) { return K < 2 || K > kOipRescaleMaxK || (K & 1); };
    if (!d_src || !d_dst || ((uintptr_t)d_src & 1) || ((uintptr_t)d_dst & 1) || !d_first_x || !d_taps_x || !d_first_y || !d_taps_y || (spp != 1 && spp != 4) ||
        W < 1 || L < 1 || Wo < 1 || Lo < 1 || L >= (1L << 31) || Lo >= (1L << 31) || (long)W * spp >= (1L << 31) || (long)Wo * spp >= (1L << 31) ||
        bad_k(Kx) || bad_k(Ky) || valid_min < 0 || valid_min > 65535 || src_row0 < 0 || src_rows < 0 || src_row0 > L || src_rows > L - src_row0 ||
        out_row0 < 0 || out_rows < 0 || out_rows > Lo || out_row0 > Lo - out_rows)
        return oip_fail(ctx, OIP_E_INVALID, "%s: bad argument", fn);
    if ((const uint16_t *)d_dst == d_src) return oip_fail(ctx, OIP_E_INVALID, "%s: the call is not in place (d_dst == d_src)", fn);
    for (int axis = 0; axis < 2; ++axis)
        if (const char *why = oip_rescale_axis_refusal(axis ? L : W, axis ? Lo : Wo)) return oip_fail(ctx, OIP_E_INVALID, "%s: %s", fn, why);
    if (out_rows == 0) return OIP_OK;
    long need0 = 0, needs = 0;
    oip_rescale_src_range_impl(L, Lo, Ky, out_row0, out_rows, &need0, &needs);
    if (need0 < src_row0 || need0 + needs > src_row0 + src_rows) {
        OipTilePlan p = {};
        p.refused = OIP_TILE_WINDOW;
        p.window[0] = need0, p.window[1] = need0 + needs - 1, p.window[2] = src_row0, p.window[3] = src_row0 + src_rows;
        return oip_tile_refusal(ctx, fn, p);
    }
    RescaleArgs a = {};
    a.t = oip_rescale_tile(W, Wo, L, Lo, spp, Kx, Ky, valid_min > 0);
    if (a.t.lds > kOipRescaleLds) return oip_fail(ctx, OIP_E_UNSUPPORTED, "%s: no tile fits %d bytes of LDS", fn, kOipRescaleLds);
    const long tiles_x = ((long)Wo + a.t.tw - 1) / a.t.tw, tiles_y = (out_rows + a.t.th - 1) / a.t.th;
    if (tiles_x * tiles_y >= (1L << 31)) return oip_fail(ctx, OIP_E_UNSUPPORTED, "%s: more than 2^31 tiles in one call", fn);
    a.src = d_src, a.dst = d_dst, a.fx = d_first_x, a.fy = d_first_y, a.tx = d_taps_x, a.ty = d_taps_y;
    a.Ws = (long)W * spp, a.Wos = (long)Wo * spp, a.L = L, a.Lo = Lo;
    a.row_lo = src_row0, a.row_hi = src_row0 + src_rows - 1;
    a.src_row0 = src_row0, a.out_row0 = out_row0, a.out_rows = out_rows;
    a.W = W, a.Wo = Wo, a.Kx = Kx, a.Ky = Ky, a.vmin = valid_min, a.tiles_x = (int)tiles_x;
    a.src_wide = a.Ws % 8 == 0 && ((uintptr_t)d_src & 15) == 0;
    a.dst_wide = a.Wos % 8 == 0 && ((uintptr_t)d_dst & 15) == 0;
    OipProfScope prof(ctx, "rescale_u16_kernel");
    const dim3 grid((unsigned)(tiles_x * tiles_y)), block(kOipRescaleBlock);
    const bool nd = valid_min > 0;
    if (spp == 1 && !nd) hipLaunchKernelGGL((rescale_u16_kernel<1, false>), grid, block, a.t.lds, ctx->stream, a);
    else if (spp == 1) hipLaunchKernelGGL((rescale_u16_kernel<1, true>), grid, block, a.t.lds, ctx->stream, a);
    else if (!nd) hipLaunchKernelGGL((rescale_u16_kernel<4, false>), grid, block, a.t.lds, ctx->stream, a);
    else hipLaunchKernelGGL((rescale_u16_kernel<4, true>), grid, block, a.t.lds, ctx->stream, a);
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}
