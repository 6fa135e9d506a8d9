// denoise.hip -- Lee's sigma filter with a pilot estimate on u16 rasters on gfx950: the noise-model-driven smoother of
// `oip denoise`.  The reference has no counterpart.  include/oip_c.h states the arithmetic (oip_sigma_filter_u16);
// tests/_denoise_ref.py restates it.
//
//   pilot    c1  = mean, half up, of the 3 x 3 neighbours within thr[ch][c >> 8] of the centre c
//   out      = mean, half up, of the (2r+1) x (2r+1) neighbours within thr[ch][c1 >> 8] of c1, if at least min_members
//              of them are; c otherwise.  Both ranges are cut at [valid_min, 65535]; a centre below valid_min passes through.
//
// Everything is integer and exact: a sum of at most 49 samples is below 2^22 and their count below 2^6, so both live in ONE
// int32 as S | m << 24 -- a sample is unpacked from LDS as n | 1 << 24 once and a member is one add.
//
// Layout / mapping: the tile, grid and LDS layout of oip_tile.h with ry = rx = R; the fill's minimum is not used (no tile form
// without the no-data rules).  The spp x 256 threshold table (2 KB at spp 4) is copied to LDS beside the tile; a sample reads
// it twice, by c >> 8 and c1 >> 8.  LDS with the table: 21.6 KB at R = 2, spp 1; 26.0 KB at R = 3, spp 4.
//
// Per neighbour and output sample: d = n - lo (unsigned wrap), d <= hi - lo, select n | 1 << 24 or 0, add: four vector
// instructions (v_sub, v_cmp, v_cndmask, v_add).  The packed 16-bit forms do not pay: v_pk_sub_u16 / v_pk_min_u16 exist, but a
// packed compare that yields a per-half mask does not, and the sums need 32 bits anyway.  The pilot is 9 such steps, the
// second stage (2R+1)^2; the two means are (2 S + m) / (2 m) by an f32 reciprocal and one exact correction step (the quotient
// is a u16 mean, so the f32 estimate is within 2^-6 of it).  R and spp are template parameters: they fix the register window.
//
// Counters (d_stats): a lane keeps the four in registers, a wave adds them by shuffles, the four waves meet in LDS and four
// lanes issue one 64-bit atomicAdd each per block.  STATS is a template parameter: without d_stats none of that is compiled.
#include "oip_tile.h"

namespace {

constexpr int kBlock = kOipTileBlock;
constexpr int kOne = 1 << 24;                // the member count's unit in an accumulator

struct SigmaArgs : OipTileArgs {
    const uint16_t *thr;                     // spp x 256
    unsigned long long *stats;               // 4, or NULL
    int minm;
};

// the NW samples of a lane's window on one LDS line, each as n | 1 << 24
template <int NW>
__device__ __forceinline__ void load_line(const uint16_t *p, int (&w)[NW])
{
#pragma unroll
    for (int c = 0; c < NW / 8; ++c) {
        const uint4 q = *reinterpret_cast<const uint4 *>(p + c * 8);
        const unsigned d[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            w[c * 8 + 2 * e] = (int)((d[e] & 0xffffu) | kOne);
            w[c * 8 + 2 * e + 1] = (int)((d[e] >> 16) | kOne);
        }
    }
}

// (2 S + m) / (2 m) of acc = S | m << 24, S the sum of m u16 samples: their mean, half up.  The f32 estimate of the quotient
// (< 2^16; operands below 2^24 are exact, the reciprocal and the product err by less than 2^-22 relative) is within 2^-6 of
// it, so its truncation is off by at most one either way.  m = 0 gives some number and no fault; the caller discards it.
__device__ __forceinline__ int mean_half_up(int acc)
{
    const int m = acc >> 24, num = 2 * (acc & (kOne - 1)) + m, den = 2 * m;
    int q = (int)((float)num * __builtin_amdgcn_rcpf((float)den));
    const int r = num - __mul24(q, den);
    q += (r >= den ? 1 : 0) - (r < 0 ? 1 : 0);
    return q;
}

// [lo, hi] = [c - T, c + T] cut at [vmin, 65535], as lo + (1 << 24) and hi - lo for the range test on n | 1 << 24
__device__ __forceinline__ void range_of(int c, int T, int vmin, int *lo, int *rng)
{
    const int l = c - T < vmin ? vmin : c - T, h = c + T > 65535 ? 65535 : c + T;
    *lo = l + kOne;
    *rng = h - l;
}

// the 8 output samples of one lane on one line.  win, nk: as oip_tile_lines() hands them over.
// st: [0] centres >= vmin, [1] of those left alone, [2] sum of m over the filtered, [3] samples changed
template <int SPP, int R, bool STATS>
__device__ __forceinline__ uint4 sigma_lane(const uint16_t *win, const uint16_t *tab, int vmin, int minm, int nk, unsigned (&st)[4])
{
    constexpr int HP = oip_tile_hp(SPP, R), NW = 8 + 2 * HP, PITCH = oip_tile_pitch(HP);
    int w[NW], ctr[8], lo[8], rng[8], acc[8];
    load_line<NW>(win + R * PITCH, w);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int c = w[HP + k] & 0xffff;
        ctr[k] = c;
        range_of(c, tab[(k & (SPP - 1)) * 256 + (c >> 8)], vmin, &lo[k], &rng[k]);
        if (c < vmin) { lo[k] = c + kOne; rng[k] = 0; }          // no data: the pilot is the centre alone, the result is discarded
        acc[k] = 0;
    }
    // ---- stage 1: the pilot over 3 x 3 --------------------------------------------------------------------------------------
#pragma unroll
    for (int jj = 0; jj < 3; ++jj) {
        if (jj > 0) load_line<NW>(win + (R + 2 * jj - 3) * PITCH, w);      // the centre line (it is loaded), then the one above and below
#pragma unroll
        for (int i = -1; i <= 1; ++i)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int n = w[HP + k + i * SPP];
                acc[k] += (unsigned)(n - lo[k]) <= (unsigned)rng[k] ? n : 0;
            }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int c1 = mean_half_up(acc[k]);
        range_of(c1, tab[(k & (SPP - 1)) * 256 + (c1 >> 8)], vmin, &lo[k], &rng[k]);
        acc[k] = 0;
    }
    // ---- stage 2: (2R+1) x (2R+1) -------------------------------------------------------------------------------------------
    for (int j = 0; j <= 2 * R; ++j) {
        load_line<NW>(win + j * PITCH, w);
#pragma unroll
        for (int i = -R; i <= R; ++i)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int n = w[HP + k + i * SPP];
                acc[k] += (unsigned)(n - lo[k]) <= (unsigned)rng[k] ? n : 0;
            }
    }
    unsigned o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int m = acc[k] >> 24, c = ctr[k];
        const bool alive = c >= vmin, filt = m >= minm;
        const int v = alive && filt ? mean_half_up(acc[k]) : c;
        o[k] = (unsigned)v;
        if (STATS && alive && k < nk) {
            st[0] += 1;
            st[1] += filt ? 0 : 1;
            st[2] += filt ? (unsigned)m : 0;
            st[3] += v != c ? 1 : 0;
        }
    }
    return oip_pack8(o);
}

template <int SPP, int R, bool ALIGNED, bool STATS>
__global__ __launch_bounds__(kBlock) void sigma_filter_u16_kernel(const SigmaArgs a)
{
    constexpr int HP = oip_tile_hp(SPP, R);
    __shared__ uint4 tile4[(kOipTileH + 2 * R) * oip_tile_nch(HP)];
    __shared__ uint16_t tab[SPP * 256];
    __shared__ unsigned wsum[kOipTileWaves][4];
    const OipTile t = oip_tile_of(a, blockIdx.x, SPP, HP, R);
#pragma unroll
    for (int c = 0; c < SPP; ++c) tab[c * 256 + threadIdx.x] = a.thr[c * 256 + threadIdx.x];
    oip_tile_fill<SPP, HP, ALIGNED>(tile4, a, t, R, OipTileEdge());
    __syncthreads();
    unsigned st[4] = {0, 0, 0, 0};
    oip_tile_lines<HP, ALIGNED>(tile4, a, t,
                                [&](const uint16_t *win, int nk) { return sigma_lane<SPP, R, STATS>(win, tab, a.vmin, a.minm, nk, st); });
    if (!STATS) return;

    // ---- counters: lanes -> wave (shuffles) -> block (LDS) -> one atomic per counter ---------------------------------------
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        unsigned v = st[i];                                      // a lane's <= 32 samples x <= 49 members: a wave's sum is below 2^17
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) wsum[wave][i] = v;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned v = 0;
#pragma unroll
        for (int w = 0; w < kOipTileWaves; ++w) v += wsum[w][threadIdx.x];
        if (v) atomicAdd(a.stats + threadIdx.x, (unsigned long long)v);
    }
}

template <int SPP, int R>
void launch_sigma(bool aligned, unsigned blocks, hipStream_t stream, const SigmaArgs &a)
{
    if (a.stats) {
        if (aligned) hipLaunchKernelGGL((sigma_filter_u16_kernel<SPP, R, true, true>), dim3(blocks), dim3(kBlock), 0, stream, a);
        else hipLaunchKernelGGL((sigma_filter_u16_kernel<SPP, R, false, true>), dim3(blocks), dim3(kBlock), 0, stream, a);
    } else {
        if (aligned) hipLaunchKernelGGL((sigma_filter_u16_kernel<SPP, R, true, false>), dim3(blocks), dim3(kBlock), 0, stream, a);
        else hipLaunchKernelGGL((sigma_filter_u16_kernel<SPP, R, false, false>), dim3(blocks), dim3(kBlock), 0, stream, a);
    }
}

template <int SPP>
void launch_radius(int radius, bool aligned, unsigned blocks, hipStream_t stream, const SigmaArgs &a)
{
    switch (radius) {
        case 1: launch_sigma<SPP, 1>(aligned, blocks, stream, a); break;
        case 2: launch_sigma<SPP, 2>(aligned, blocks, stream, a); break;
        default: launch_sigma<SPP, 3>(aligned, blocks, stream, a); break;
    }
}

}  // namespace

extern "C" int oip_sigma_filter_u16(oip_ctx *ctx, const uint16_t *d_src, long src_row0, long src_rows, uint16_t *d_dst, long out_row0, long out_rows,
                                    int W, long L, int spp, int radius, const uint16_t *d_thr, int min_members, int valid_min, uint64_t *d_stats)
{
    OIP_CHECK_CTX(ctx);
    const char *fn = "oip_sigma_filter_u16";
    if (!d_thr || ((uintptr_t)d_thr & 1) || ((uintptr_t)d_stats & 7) || radius < 1 || radius > 3 || min_members < 1 ||
        min_members > (2 * radius + 1) * (2 * radius + 1))
        return oip_fail(ctx, OIP_E_INVALID, "%s: bad argument", fn);
    const OipTilePlan p = oip_tile_plan(d_src, src_row0, src_rows, d_dst, out_row0, out_rows, W, L, spp, valid_min, radius, 1, W);
    if (const int rc = oip_tile_refusal(ctx, fn, p)) return rc;
    if (!p.blocks) return OIP_OK;
    SigmaArgs a;
    static_cast<OipTileArgs &>(a) = p.args;
    a.thr = d_thr;
    a.stats = reinterpret_cast<unsigned long long *>(d_stats);
    a.minm = min_members;
    OipProfScope prof(ctx, "sigma_filter_u16_kernel");
    if (spp == 1) launch_radius<1>(radius, p.aligned, p.blocks, ctx->stream, a);
    else launch_radius<4>(radius, p.aligned, p.blocks, ctx->stream, a);
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}
