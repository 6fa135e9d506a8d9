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
// Layout / mapping: the tile, grid and LDS layout of oip_tile.h with ry = rx = 1, a tile inside ONE column group (a band of a BIL
// line; the whole line at groups 1): the tiles of a line are groups * ceil(gw * spp / 512).  The edge policy of the fill is
// DespikeEdge: the 16-byte load where the chunk lies inside the group and holds no listed column, otherwise the pixel index
// clamped to the group (the replicate border at the image edge and at a band border alike) and listed columns interpolated
// from their two good neighbours.  The arithmetic behind the barrier sees neither the table nor the borders.  Which chunks
// hold a listed column comes from one byte per chunk that a small kernel ahead of the tiles derives from the table (a few KB,
// read through L2).  A lane's 8 samples are four packed u16 pairs.
//
// Median of nine on packed pairs: the three lines' values of a pair of sample columns are sorted (3 min/max exchanges), then
// median = med3(max of the three column minima, med3 of the column medians, min of the column maxima): 30 v_pk_min_u16 /
// v_pk_max_u16 per pair, 15 per sample.  At spp 1 the left and right neighbours of a pair straddle two dwords: one
// v_alignbyte_b32 each.  The threshold test runs per sample in 32 bits (T can reach 131 070).
//
// No data: only a tile that oip_tile_has_nodata() reports pays for the compare-and-select that replaces no-data neighbours by
// the centre and the compare that lets a no-data centre pass.
//
// Counts: a lane's 8 columns x at most 4 lines fit eight 4-bit fields of one register; the four waves' registers meet in LDS
// and one lane per non-zero column issues one 64-bit atomicAdd per block.  LDS: 18 lines x 528 samples x 2 bytes + 1 KB of counts.
#include "oip_tile.h"

namespace {

constexpr int kBlock = kOipTileBlock;
constexpr int kHP = oip_tile_hp(4, 1);       // halo samples either side in LDS (spp of them are read)
constexpr int kPitch = oip_tile_pitch(kHP);

typedef oip_us2 us2;
typedef short ss2 __attribute__((ext_vector_type(2)));

struct DespikeArgs : OipTileArgs {
    const int32_t *tab;                      // (Lx, Rx) per column, or NULL
    const uint8_t *chunk_bad;                // with a table, ALIGNED: 1 where the 8 columns from 8 i on hold a listed one
    unsigned long long *count;               // per sample column, or NULL
    int gw;                                  // pixels per group
    int tiles_g;                             // tiles across a group
    int thr_abs, thr_rel;
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

// the 8 output samples of one lane on one line.  win: as oip_tile_lines() hands it over (the LDS line above the output line).
// hits: the 4-bit field k is 1 where sample k was replaced.
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

// the edge policy of the fill (oip_tile.h): the border is the group's, and with a table a listed column is repaired on the way
template <int SPP>
struct DespikeEdge {
    const DespikeArgs &a;
    __device__ bool wide(long s) const { return !(a.tab && a.chunk_bad[s >> 3]); }
    __device__ unsigned sample(const uint16_t *line, long p, long at) const
    {
        if (SPP != 1 || !a.tab) return line[at];
        // (Lx, Rx) of a well-formed table lie inside the line with Lx <= p <= Rx; anything else copies a sample of the line
        int lx = a.tab[2 * p], rx = a.tab[2 * p + 1];
        lx = lx < 0 ? 0 : (lx > a.W - 1 ? a.W - 1 : lx);
        rx = rx < 0 ? 0 : (rx > a.W - 1 ? a.W - 1 : rx);
        const unsigned va = line[lx], vb = line[rx];
        const long D = (long)rx - lx;
        if (!(D > 0 && lx <= p && p <= rx)) return va;
        if ((int)va < a.vmin || (int)vb < a.vmin) return (int)va >= a.vmin ? va : vb;
        return (unsigned)(((unsigned long long)va * (unsigned long long)(rx - p) + (unsigned long long)vb * (unsigned long long)(p - lx) +
                           (unsigned long long)(D / 2)) / (unsigned long long)D);
    }
};

template <int SPP, bool ALIGNED>
__global__ __launch_bounds__(kBlock) void despike_u16_kernel(const DespikeArgs a)
{
    __shared__ uint4 tile4[(kOipTileH + 2) * oip_tile_nch(kHP)];
    __shared__ unsigned hits4[kBlock];
    const int tiles_g = a.tiles_g, gw = a.gw;
    asm volatile("" ::"s"(tiles_g), "s"(gw));                   // fetched with the other arguments, not behind the block-index division
    const OipTile t = oip_tile_of<true>(a, blockIdx.x, SPP, kHP, 1, tiles_g, gw);
    const bool mask = oip_tile_has_nodata(oip_tile_fill<SPP, kHP, ALIGNED>(tile4, a, t, 1, DespikeEdge<SPP>{a}), a.vmin);
    unsigned cnt = 0;                                            // eight 4-bit fields: this lane's replacements per column (<= 4 lines)
    oip_tile_lines<kHP, ALIGNED>(tile4, a, t, [&](const uint16_t *win, int) {
        unsigned h;
        const uint4 o = mask ? despike_lane<SPP, true>(win, a, &h) : despike_lane<SPP, false>(win, a, &h);
        cnt += h;
        return o;
    });
    if (!a.count) return;                                        // (the same for every lane)

    // ---- counts: the four waves' fields of a column -> one atomic per non-zero column ---------------------------------------
    hits4[threadIdx.x] = cnt;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kOipTileW / kBlock; ++e) {
        const int col = threadIdx.x + e * kBlock;         // sample column of the tile
        if (col >= t.cols) continue;                             // (a replaced sample lies inside the tile: the fields beyond are 0)
        unsigned n = 0;
#pragma unroll
        for (int w = 0; w < kOipTileWaves; ++w) n += (hits4[w * 64 + (col >> 3)] >> (4 * (col & 7))) & 15u;
        if (n) atomicAdd(a.count + t.x0 + col, (unsigned long long)n);
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
    const char *fn = "oip_despike_u16";
    if (((uintptr_t)d_coltab & 3) || ((uintptr_t)d_count & 7) || (groups != 1 && groups != 4) || thr_abs < 0 || thr_abs > 65535 || thr_rel_q8 < 0 ||
        thr_rel_q8 > 256)
        return oip_fail(ctx, OIP_E_INVALID, "%s: bad argument", fn);
    const OipTilePlan p = oip_tile_plan(d_src, src_row0, src_rows, d_dst, out_row0, out_rows, W, L, spp, valid_min, 1, groups, W / groups);
    if (const int rc = oip_tile_refusal(ctx, fn, p, OIP_TILE_IN_PLACE)) return rc;
    if (d_coltab && spp != 1) return oip_fail(ctx, OIP_E_UNSUPPORTED, "%s: a column table needs 1 sample per pixel", fn);
    if (const int rc = oip_tile_refusal(ctx, fn, p)) return rc;
    if (!p.blocks) return OIP_OK;
    DespikeArgs a;
    static_cast<OipTileArgs &>(a) = p.args;
    a.tab = d_coltab;
    a.chunk_bad = nullptr;
    a.count = reinterpret_cast<unsigned long long *>(d_count);
    a.gw = W / groups;
    a.tiles_g = p.tiles_g;
    a.thr_abs = thr_abs;
    a.thr_rel = thr_rel_q8;
    void *ws = nullptr;
    const int chunks = (W + 7) / 8;
    if (d_coltab && p.aligned) {
        const int rc = oip_workspace(ctx, (size_t)chunks, &ws);
        if (rc != OIP_OK) return rc;
        a.chunk_bad = static_cast<const uint8_t *>(ws);
    }
    OipProfScope prof(ctx, "despike_u16_kernel");
    if (ws)
        hipLaunchKernelGGL(despike_chunks_kernel, dim3((chunks + kBlock - 1) / kBlock), dim3(kBlock), 0, ctx->stream, d_coltab, W,
                           static_cast<uint8_t *>(ws));
    if (spp == 1) {
        if (p.aligned) hipLaunchKernelGGL((despike_u16_kernel<1, true>), dim3(p.blocks), dim3(kBlock), 0, ctx->stream, a);
        else hipLaunchKernelGGL((despike_u16_kernel<1, false>), dim3(p.blocks), dim3(kBlock), 0, ctx->stream, a);
    } else {
        if (p.aligned) hipLaunchKernelGGL((despike_u16_kernel<4, true>), dim3(p.blocks), dim3(kBlock), 0, ctx->stream, a);
        else hipLaunchKernelGGL((despike_u16_kernel<4, false>), dim3(p.blocks), dim3(kBlock), 0, ctx->stream, a);
    }
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}
