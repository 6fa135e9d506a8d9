// despike.hip -- repair of a raw strip on gfx950 before anything resamples it: listed bad columns are interpolated, isolated
// impulse pixels are replaced by a conditional 3 x 3 median (`oip despike`).  The reference has no counterpart.
// include/oip_c.h states the arithmetic (oip_despike_u16); tests/_despike_ref.py restates it.
//
//   c(v, x)  = src[v][x], or for a listed column the rounded linear interpolation between its good neighbours Lx, Rx
//   med      = median of the nine n' = c(clamped neighbours), no-data neighbours replaced by the centre
//   out      = |ctr - med| > thr_abs + ((med * thr_rel_q8) >> 8) ? med : ctr        and a per-column count of the replacements
//
// Everything is integer and exact.
//
// Layout / mapping: that of convolve.hip.  Lines are handled in SAMPLE units (Ws = W * spp; a horizontal neighbour is spp
// samples away).  A block of 256 lanes owns a tile of 512 samples x 16 lines that lies inside ONE column group (a band of a
// BIL line; the whole line at groups 1): the tiles of a line are groups * ceil(gw * spp / 512).  The tile, one line above and
// below and 8 samples left and right go to LDS once, in 16-byte chunks: an aligned global_load_dwordx4 where the chunk lies
// inside the group and holds no listed column, eight 2-byte loads otherwise -- pixel index clamped to the group (the replicate
// border at the image edge and at a band border alike, channel kept), listed columns interpolated from their two good
// neighbours.  The arithmetic behind the barrier sees neither the table nor the borders.  Which chunks hold a listed column
// comes from one byte per chunk that a small kernel ahead of the tiles derives from the table (a few KB, read through L2).
// Then a lane owns ONE aligned 16-byte store, 8 consecutive samples of a line, as four packed u16 pairs; a wave takes a line,
// the four waves every fourth line of the tile.
//
// Median of nine on packed pairs: the three lines' values of a pair of sample columns are sorted (3 min/max exchanges), then
// median = med3(max of the three column minima, med3 of the column medians, min of the column maxima): 30 v_pk_min_u16 /
// v_pk_max_u16 per pair, 15 per sample.  At spp 1 the left and right neighbours of a pair straddle two dwords: one
// v_alignbyte_b32 each.  The threshold test runs per sample in 32 bits (T can reach 131 070).
//
// No data: as convolve.hip does, the fill keeps the packed minimum of what it loads and the barrier ORs "some sample is below
// valid_min" over the block; only such a tile pays for the compare-and-select that replaces no-data neighbours by the
// centre and the compare that lets a no-data centre pass.
//
// Counts: a lane's 8 columns x at most 4 lines fit eight 4-bit fields of one register; the four waves' registers meet in LDS
// and one lane per non-zero column issues one 64-bit atomicAdd per block.
//
// A line or a group that is not a multiple of 8 samples, or bases that are not 16-byte aligned, take the same kernel with
// ALIGNED = false: 2-byte loads into the same LDS image, the same arithmetic, 2-byte stores.
//
// One tile per block, no grid-stride loop.  LDS: 18 lines x 528 samples x 2 bytes + 1 KB of counts, about 20 KB per block.
#include "oip_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTileW = 512;                  // samples: 64 lanes x 8
constexpr int kTileH = 16;                   // lines
constexpr int kHP = 8;                       // halo samples either side in LDS (spp of them are read)
constexpr int kPitch = kTileW + 2 * kHP;
constexpr int kNch = kPitch / 8;
constexpr int kRows = kTileH + 2;

typedef unsigned short us2 __attribute__((ext_vector_type(2)));
typedef short ss2 __attribute__((ext_vector_type(2)));

struct DespikeArgs {
    const uint16_t *src;
    uint16_t *dst;
    const int32_t *tab;                      // (Lx, Rx) per column, or NULL
    const uint8_t *chunk_bad;                // with a table, ALIGNED: 1 where the 8 columns from 8 i on hold a listed one
    unsigned long long *count;               // per sample column, or NULL
    long Ws, L;                              // samples per line, lines of the raster
    long src_row0, out_row0, out_rows;
    int W;                                   // pixels per line
    int gw;                                  // pixels per group
    int tiles_g;                             // tiles across a group
    int tiles_x;                             // tiles across a line
    int thr_abs, thr_rel, vmin;
};

__device__ __forceinline__ us2 pk(unsigned v) { return __builtin_bit_cast(us2, v); }
__device__ __forceinline__ unsigned un(us2 v) { return __builtin_bit_cast(unsigned, v); }
__device__ __forceinline__ us2 pmin(us2 a, us2 b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ us2 pmax(us2 a, us2 b) { return __builtin_elementwise_max(a, b); }
__device__ __forceinline__ void sort2(us2 &a, us2 &b) { const us2 lo = pmin(a, b); b = pmax(a, b); a = lo; }
__device__ __forceinline__ us2 med3(us2 a, us2 b, us2 c) { return pmax(pmin(a, b), pmin(pmax(a, b), c)); }
// samples (2k + 1, 2k + 2) from the dwords holding (2k, 2k + 1) and (2k + 2, 2k + 3)
__device__ __forceinline__ unsigned straddle(unsigned lo, unsigned hi) { return __builtin_amdgcn_alignbyte(hi, lo, 2); }

// the median of three lines x three columns, two sample columns at a time
__device__ __forceinline__ us2 med9(us2 (&n)[3][3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) {            // column i: n[0][i] <= n[1][i] <= n[2][i]
        sort2(n[0][i], n[1][i]);
        sort2(n[1][i], n[2][i]);
        sort2(n[0][i], n[1][i]);
    }
    const us2 lo = pmax(pmax(n[0][0], n[0][1]), n[0][2]);
    const us2 hi = pmin(pmin(n[2][0], n[2][1]), n[2][2]);
    return med3(lo, med3(n[1][0], n[1][1], n[1][2]), hi);
}

// the 8 output samples of one lane on one line.  win: the lane's first LDS sample of the tile's LDS line above the output
// line.  hits: the 4-bit field k is 1 where sample k was replaced.
template <int SPP, bool MASK>
__device__ __forceinline__ uint4 despike_lane(const uint16_t *win, const DespikeArgs &a, unsigned *hits)
{
    unsigned d[3][12];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint4 q = *reinterpret_cast<const uint4 *>(win + j * kPitch + c * 8);
            d[j][c * 4 + 0] = q.x; d[j][c * 4 + 1] = q.y; d[j][c * 4 + 2] = q.z; d[j][c * 4 + 3] = q.w;
        }
    const unsigned vm = (unsigned)a.vmin | ((unsigned)a.vmin << 16);
    unsigned o[4], h = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int C = kHP / 2 + k;           // the dword of the pair
        const us2 ctr = pk(d[1][C]);
        us2 n[3][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            if (SPP == 1) {
                n[j][0] = pk(straddle(d[j][C - 1], d[j][C]));
                n[j][2] = pk(straddle(d[j][C], d[j][C + 1]));
            } else {
                n[j][0] = pk(d[j][C - SPP / 2]);
                n[j][2] = pk(d[j][C + SPP / 2]);
            }
            n[j][1] = pk(d[j][C]);
            if (MASK) {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const ss2 below = n[j][i] < pk(vm);                      // all ones where no data
                    const us2 m = __builtin_bit_cast(us2, below);
                    n[j][i] = (n[j][i] & ~m) | (ctr & m);
                }
            }
        }
        const unsigned med = un(med9(n)), cc = un(ctr);
        unsigned r[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int m = (int)((med >> (16 * e)) & 0xffffu), c = (int)((cc >> (16 * e)) & 0xffffu);
            const int T = a.thr_abs + (__mul24(m, a.thr_rel) >> 8);
            const int dd = c > m ? c - m : m - c;
            const bool rep = dd > T && !(MASK && c < a.vmin);                // a no-data centre passes through
            r[e] = (unsigned)(rep ? m : c);
            h |= (rep ? 1u : 0u) << (4 * (2 * k + e));
        }
        o[k] = r[0] | (r[1] << 16);
    }
    *hits = h;
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// ALIGNED requires: Ws % 8 == 0, gw * spp % 8 == 0, src and dst 16-byte aligned
template <int SPP, bool ALIGNED>
__global__ __launch_bounds__(kBlock) void despike_u16_kernel(const DespikeArgs a)
{
    constexpr int SH = SPP == 4 ? 2 : 0;
    __shared__ uint4 tile4[kRows * kNch];
    __shared__ unsigned hits4[kBlock];
    const long ty = (long)blockIdx.x / a.tiles_x;
    const int tx = (int)((long)blockIdx.x - ty * a.tiles_x);
    const int g = tx / a.tiles_g, tg = tx - g * a.tiles_g;
    const long gp0 = (long)g * a.gw, gp1 = gp0 + a.gw - 1;       // first and last pixel of the group
    const long gs0 = gp0 << SH, gs1 = (gp1 + 1) << SH;           // its samples [gs0, gs1)
    const long y0 = a.out_row0 + ty * kTileH;                    // first output line of the tile (global)
    const long left = a.out_row0 + a.out_rows - y0;
    const int rows = left < kTileH ? (int)left : kTileH;         // output lines of the tile, >= 1
    const long x0 = gs0 + (long)tg * kTileW;                     // first output sample of the tile
    const long wleft = gs1 - x0;
    const int cols = wleft < kTileW ? (int)wleft : kTileW;       // output samples of the tile, >= 1
    const int nch = (cols + 2 * kHP + 7) >> 3;                   // chunks of an LDS line that are read later
    const int nfill = (rows + 2) * kNch;

    // ---- the tile and its halo -> LDS: column repair and the group's replicate border happen here --------------------------
    unsigned lo = 0xffffffffu;
    for (int e = threadIdx.x; e < nfill; e += kBlock) {
        const int r = e / kNch, c = e - r * kNch;
        if (c >= nch) continue;
        long v = y0 - 1 + r;
        v = v < 0 ? 0 : (v > a.L - 1 ? a.L - 1 : v);             // inside [src_row0, src_row0 + src_rows): host-checked
        const uint16_t *line = a.src + (v - a.src_row0) * a.Ws;
        const long s = x0 - kHP + c * 8;
        uint4 q;
        if (ALIGNED && s >= gs0 && s + 8 <= gs1 && !(a.tab && a.chunk_bad[s >> 3])) {
            q = *reinterpret_cast<const uint4 *>(line + s);
        } else {
            unsigned t[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const long ss = s + k;
                long p = ss >> SH;                               // arithmetic shift: the floor for ss < 0 as well
                p = p < gp0 ? gp0 : (p > gp1 ? gp1 : p);
                if (SPP == 1 && a.tab) {
                    // (Lx, Rx) of a well-formed table lie inside the line with Lx <= p <= Rx; anything else copies a sample of the line
                    int lx = a.tab[2 * p], rx = a.tab[2 * p + 1];
                    lx = lx < 0 ? 0 : (lx > a.W - 1 ? a.W - 1 : lx);
                    rx = rx < 0 ? 0 : (rx > a.W - 1 ? a.W - 1 : rx);
                    const unsigned va = line[lx], vb = line[rx];
                    const long D = (long)rx - lx;
                    unsigned cv = va;
                    if (D > 0 && lx <= p && p <= rx) {
                        if ((int)va < a.vmin || (int)vb < a.vmin) cv = (int)va >= a.vmin ? va : vb;
                        else cv = (unsigned)(((unsigned long long)va * (unsigned long long)(rx - p) + (unsigned long long)vb * (unsigned long long)(p - lx) +
                                              (unsigned long long)(D / 2)) / (unsigned long long)D);
                    }
                    t[k] = cv;
                } else {
                    t[k] = line[(p << SH) + (ss & (SPP - 1))];
                }
            }
            q = make_uint4(t[0] | (t[1] << 16), t[2] | (t[3] << 16), t[4] | (t[5] << 16), t[6] | (t[7] << 16));
        }
        lo = un(pmin(pmin(pk(lo), pk(q.x)), pmin(pk(q.y), pmin(pk(q.z), pk(q.w)))));
        tile4[e] = q;
    }
    const int nodata = (int)(lo & 0xffffu) < a.vmin || (int)(lo >> 16) < a.vmin;
    const bool mask = __syncthreads_or(nodata) != 0;

    // ---- a wave per line, a lane per 16 bytes of it ------------------------------------------------------------------------
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned cnt = 0;                                            // eight 4-bit fields: this lane's replacements per column (<= 4 lines)
    if (lane * 8 < cols) {
        const uint16_t *tile = reinterpret_cast<const uint16_t *>(tile4);
        for (int r = wave; r < rows; r += kWaves) {
            const uint16_t *win = tile + r * kPitch + lane * 8;
            unsigned h;
            const uint4 o = mask ? despike_lane<SPP, true>(win, a, &h) : despike_lane<SPP, false>(win, a, &h);
            uint16_t *out = a.dst + (y0 - a.out_row0 + r) * a.Ws + x0 + lane * 8;
            if (ALIGNED) {
                *reinterpret_cast<uint4 *>(out) = o;             // cols % 8 == 0: the whole chunk is inside the group
            } else {
                const unsigned d[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if (lane * 8 + k < cols) out[k] = (uint16_t)(d[k >> 1] >> ((k & 1) * 16));
            }
            cnt += h;
        }
    }
    if (!a.count) return;                                        // (the same for every lane)

    // ---- counts: the four waves' fields of a column -> one atomic per non-zero column ---------------------------------------
    hits4[threadIdx.x] = cnt;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kTileW / kBlock; ++e) {
        const int col = threadIdx.x + e * kBlock;                // sample column of the tile
        if (col >= cols) continue;                               // (a replaced sample lies inside the tile: the fields beyond are 0)
        unsigned n = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) n += (hits4[w * 64 + (col >> 3)] >> (4 * (col & 7))) & 15u;
        if (n) atomicAdd(a.count + x0 + col, (unsigned long long)n);
    }
}

// one byte per 8 columns: does the chunk hold a column whose table entry is not (x, x)?
__global__ __launch_bounds__(kBlock) void despike_chunks_kernel(const int32_t *__restrict__ tab, int W, uint8_t *__restrict__ chunk_bad)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i * 8L >= W) return;
    int bad = 0;
    for (int k = 0; k < 8; ++k) {
        const int x = i * 8 + k;
        if (x < W) bad |= tab[2 * x] != x || tab[2 * x + 1] != x;
    }
    chunk_bad[i] = (uint8_t)bad;
}

}  // namespace

extern "C" int oip_despike_u16(oip_ctx *ctx, const uint16_t *d_src, long src_row0, long src_rows, uint16_t *d_dst, long out_row0, long out_rows,
                               int W, long L, int spp, int groups, const int32_t *d_coltab, int thr_abs, int thr_rel_q8, int valid_min,
                               uint64_t *d_count)
{
    OIP_CHECK_CTX(ctx);
    if (!d_src || !d_dst || ((uintptr_t)d_src & 1) || ((uintptr_t)d_dst & 1) || ((uintptr_t)d_coltab & 3) || ((uintptr_t)d_count & 7) ||
        (spp != 1 && spp != 4) || (groups != 1 && groups != 4) || (groups == 4 && (spp != 1 || W % 4 != 0)) || W < 1 || L < 1 || thr_abs < 0 ||
        thr_abs > 65535 || thr_rel_q8 < 0 || thr_rel_q8 > 256 || valid_min < 0 || valid_min > 65535 || src_row0 < 0 || src_rows < 0 || out_row0 < 0 ||
        out_rows < 0 || out_rows > L || out_row0 > L - out_rows)
        return oip_fail(ctx, OIP_E_INVALID, "oip_despike_u16: bad argument");
    if ((const uint16_t *)d_dst == d_src) return oip_fail(ctx, OIP_E_INVALID, "oip_despike_u16: the call is not in place (d_dst == d_src)");
    if (d_coltab && spp != 1) return oip_fail(ctx, OIP_E_UNSUPPORTED, "oip_despike_u16: a column table needs 1 sample per pixel");
    if (out_rows == 0) return OIP_OK;
    const long first = out_row0 - 1 < 0 ? 0 : out_row0 - 1;
    const long last = out_row0 + out_rows > L - 1 ? L - 1 : out_row0 + out_rows;
    if (first < src_row0 || last >= src_row0 + src_rows)
        return oip_fail(ctx, OIP_E_INVALID, "oip_despike_u16: source lines [%ld, %ld] needed, [%ld, %ld) resident", first, last, src_row0,
                        src_row0 + src_rows);
    DespikeArgs a;
    a.src = d_src;
    a.dst = d_dst;
    a.tab = d_coltab;
    a.chunk_bad = nullptr;
    a.count = reinterpret_cast<unsigned long long *>(d_count);
    a.Ws = (long)W * spp;
    a.L = L;
    a.src_row0 = src_row0;
    a.out_row0 = out_row0;
    a.out_rows = out_rows;
    a.W = W;
    a.gw = W / groups;
    const long gws = (long)a.gw * spp;
    a.tiles_g = (int)((gws + kTileW - 1) / kTileW);
    const long tiles_x = (long)a.tiles_g * groups, tiles_y = (out_rows + kTileH - 1) / kTileH;
    if (tiles_x * tiles_y >= (1L << 31)) return oip_fail(ctx, OIP_E_UNSUPPORTED, "oip_despike_u16: more than 2^31 tiles in one call");
    a.tiles_x = (int)tiles_x;
    a.thr_abs = thr_abs;
    a.thr_rel = thr_rel_q8;
    a.vmin = valid_min;
    const bool aligned = a.Ws % 8 == 0 && gws % 8 == 0 && ((uintptr_t)d_src & 15) == 0 && ((uintptr_t)d_dst & 15) == 0;
    const unsigned blocks = (unsigned)(tiles_x * tiles_y);
    void *ws = nullptr;
    const int chunks = (W + 7) / 8;
    if (d_coltab && aligned) {
        const int rc = oip_workspace(ctx, (size_t)chunks, &ws);
        if (rc != OIP_OK) return rc;
        a.chunk_bad = static_cast<const uint8_t *>(ws);
    }
    OipProfScope prof(ctx, "despike_u16_kernel");
    if (ws) hipLaunchKernelGGL(despike_chunks_kernel, dim3((chunks + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, d_coltab, W, static_cast<uint8_t *>(ws));
    if (spp == 1) {
        if (aligned) hipLaunchKernelGGL((despike_u16_kernel<1, true>), dim3(blocks), dim3(kBlock), 0, ctx->stream, a);
        else hipLaunchKernelGGL((despike_u16_kernel<1, false>), dim3(blocks), dim3(kBlock), 0, ctx->stream, a);
    } else {
        if (aligned) hipLaunchKernelGGL((despike_u16_kernel<4, true>), dim3(blocks), dim3(kBlock), 0, ctx->stream, a);
        else hipLaunchKernelGGL((despike_u16_kernel<4, false>), dim3(blocks), dim3(kBlock), 0, ctx->stream, a);
    }
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}
