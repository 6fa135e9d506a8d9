// oip_tile.h -- the tile, grid and LDS layout that the neighbourhood filters on u16 rasters share (convolve.hip, despike.hip,
// denoise.hip), and its device code.  oip_tileplan.h holds the arithmetic.
//
// Lines are handled in SAMPLE units (Ws = W * spp; the channel of sample s is s % spp, its pixel s / spp; a horizontal
// neighbour is spp samples away).  A block of 256 lanes owns a tile of 512 samples x 16 lines; a tile starts at a multiple of
// 512 samples of its column group (the whole line, but for the bands of a BIL line), so the channel of a lane's sample k is
// k % spp.  One tile per block, no grid-stride loop: the grid is tiles_x * tiles_y in x (368 750 blocks at 30000 x 100000).
//
// Fill.  The tile plus its halo (ry lines above and below, rx * spp samples left and right rounded up to 8 = HP) goes to LDS
// once, in 16-byte chunks: an aligned global_load_dwordx4 where the chunk lies inside the line, eight clamped 2-byte loads
// where it crosses the border (pixel index clamped, channel kept) -- the replicate border costs nothing in the arithmetic
// behind the barrier.  Lines are clamped the same way and fetched from the resident window [src_row0, src_row0 + src_rows).
// Only the lines and chunks that the tile's output needs are touched (a last tile has fewer lines; the window holds no more).
// The border is that of the tile's column group; an edge policy says which chunks inside it may not take the 16-byte path
// and how a sample is read there: OipTileEdge is the plain line.  The LDS image is (16 + 2 ry) lines x PITCH = 512 + 2 HP
// samples x 2 bytes, at most 26 112 bytes.
//
// No data.  While a tile is filled each lane keeps the packed minimum of what it loads (v_pk_min_u16, one per dword); the
// barrier behind the fill ORs "some sample is below valid_min" over the block, and a tile without such a sample -- always so
// at valid_min 0 -- may run a loop without the no-data rules.  Both forms must give the same bytes.
//
// Compute.  A lane owns ONE aligned 16-byte store: 8 consecutive samples of a line; a wave takes a line, the four waves every
// fourth line of the tile.  For window line j the lane reads its 8 + 2 HP samples from LDS as ds_read_b128 (lanes read
// consecutive 16 bytes: conflict-free).
//
// A line or a group that is not a multiple of 8 samples, or bases that are not 16-byte aligned, take the same kernel with
// ALIGNED = false: 2-byte loads into the same LDS image, the same arithmetic, 2-byte stores.
#pragma once

#include "oip_internal.h"
#include "oip_tileplan.h"

// the plan's refusal, if it has one of a kind up to `upto`, as the entry point `fn` states it; OIP_OK otherwise.  (A filter's
// own checks that stand behind "not in place" go between a call with OIP_TILE_IN_PLACE and one without.)
inline int oip_tile_refusal(oip_ctx *ctx, const char *fn, const OipTilePlan &p, OipTileRefusal upto = OIP_TILE_TOO_MANY)
{
    if (p.refused > upto) return OIP_OK;
    switch (p.refused) {
        case OIP_TILE_OK: return OIP_OK;
        case OIP_TILE_BAD_ARGUMENT: return oip_fail(ctx, OIP_E_INVALID, "%s: bad argument", fn);
        case OIP_TILE_IN_PLACE: return oip_fail(ctx, OIP_E_INVALID, "%s: the call is not in place (d_dst == d_src)", fn);
        case OIP_TILE_WINDOW:
            return oip_fail(ctx, OIP_E_INVALID, "%s: source lines [%ld, %ld] needed, [%ld, %ld) resident", fn, p.window[0], p.window[1], p.window[2],
                            p.window[3]);
        default: return oip_fail(ctx, OIP_E_UNSUPPORTED, "%s: more than 2^31 tiles in one call", fn);
    }
}

typedef unsigned short oip_us2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned oip_pk_min_u16(unsigned a, unsigned b)
{
    return __builtin_bit_cast(unsigned, __builtin_elementwise_min(__builtin_bit_cast(oip_us2, a), __builtin_bit_cast(oip_us2, b)));
}

__device__ __forceinline__ void oip_unpack8(const uint4 q, int (&w)[8])
{
    w[0] = q.x & 0xffffu; w[1] = q.x >> 16; w[2] = q.y & 0xffffu; w[3] = q.y >> 16;
    w[4] = q.z & 0xffffu; w[5] = q.z >> 16; w[6] = q.w & 0xffffu; w[7] = q.w >> 16;
}

__device__ __forceinline__ uint4 oip_pack8(const unsigned (&o)[8])
{
    return make_uint4(o[0] | (o[1] << 16), o[2] | (o[3] << 16), o[4] | (o[5] << 16), o[6] | (o[7] << 16));
}

// The edge policy of the fill.  The border is that of the tile's column group (OipTile g0, g1).  A chunk inside the
// group for which wide() holds takes the 16-byte load; sample() reads the sample at index `at` of the line, which belongs
// to the clamped pixel p.  This one is the plain line.
struct OipTileEdge {
    __device__ bool wide(long) const { return true; }
    __device__ unsigned sample(const uint16_t *line, long, long at) const { return line[at]; }
};

// the tile `t` and its halo -> tile4.  Returns the packed minimum of what this lane loaded.  ALIGNED requires what
// OipTilePlan::aligned states.  A barrier has to follow: oip_tile_has_nodata(), or __syncthreads() where the minimum is not used.
template <int SPP, int HP, bool ALIGNED, class Edge>
__device__ __forceinline__ unsigned oip_tile_fill(uint4 *tile4, const OipTileArgs &a, const OipTile &t, int ry, const Edge edge)
{
    unsigned lo = 0xffffffffu;
    for (int e = threadIdx.x; e < t.nfill; e += kOipTileBlock) {
        const OipTileChunk ch = oip_tile_chunk(a, t, e, HP, ry);
        if (!ch.read) continue;
        const uint16_t *line = a.src + ch.row * a.Ws;
        uint4 q;
        if (oip_tile_chunk_wide(t, ALIGNED, ch.s) && edge.wide(ch.s)) {
            q = *reinterpret_cast<const uint4 *>(line + ch.s);
        } else {
            unsigned v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                long p;
                const long at = oip_tile_border_sample(t, ch.s, k, SPP, &p);
                v[k] = edge.sample(line, p, at);
            }
            q = oip_pack8(v);
        }
        lo = oip_pk_min_u16(oip_pk_min_u16(lo, q.x), oip_pk_min_u16(q.y, oip_pk_min_u16(q.z, q.w)));
        tile4[e] = q;
    }
    return lo;
}

// the barrier behind the fill: does the block's tile or halo hold a sample below vmin?
__device__ __forceinline__ bool oip_tile_has_nodata(unsigned lo, int vmin)
{
    const int nodata = (int)(lo & 0xffffu) < vmin || (int)(lo >> 16) < vmin;
    return __syncthreads_or(nodata) != 0;
}

// how many of the 8 samples of `lane` lie inside the tile (8 if ALIGNED: cols % 8 == 0), and the store of that many
template <bool ALIGNED>
__device__ __forceinline__ int oip_tile_nk(const OipTile &t, int lane)
{
    return ALIGNED ? 8 : (t.cols - lane * 8 < 8 ? t.cols - lane * 8 : 8);
}

template <bool ALIGNED>
__device__ __forceinline__ void oip_tile_store(uint16_t *out, const uint4 o, int nk)
{
    if (ALIGNED) {
        *reinterpret_cast<uint4 *>(out) = o;
    } else {
        const unsigned d[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (k < nk) out[k] = (uint16_t)(d[k >> 1] >> ((k & 1) * 16));
    }
}

// A wave per line, a lane per 16 bytes of it: f(win, nk) gives the lane's 8 samples, which are stored.  win: the lane's first
// LDS sample of LDS line r, r the output line less the tile's first (window line j is LDS line r + j).
template <int HP, bool ALIGNED, class F>
__device__ __forceinline__ void oip_tile_lines(const uint4 *tile4, const OipTileArgs &a, const OipTile &t, F f)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane * 8 >= t.cols) return;
    const uint16_t *tile = reinterpret_cast<const uint16_t *>(tile4);
    const int nk = oip_tile_nk<ALIGNED>(t, lane);
    for (int r = wave; r < t.rows; r += kOipTileWaves)
        oip_tile_store<ALIGNED>(a.dst + (t.y0 - a.out_row0 + r) * a.Ws + t.x0 + lane * 8, f(tile + r * oip_tile_pitch(HP) + lane * 8, nk), nk);
}
