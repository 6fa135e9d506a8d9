// oip_tileplan.h -- the tile arithmetic of the neighbourhood filters on u16 rasters (convolve.hip, despike.hip, denoise.hip): the
// tile constants, the checks and the plan of an entry point, which tile a block owns, which chunk of which source line goes
// where in its LDS image, and which sample stands in for one beyond a border.  oip_tile.h describes the layout and is the
// device side.  Nothing of HIP in here: the kernels run these lines, and tests/cpp/tileplan_test.cpp runs them on the CPU.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define OIP_TILE_FN __host__ __device__ __forceinline__
#else
#define OIP_TILE_FN inline
#endif

constexpr int kOipTileBlock = 256;           // lanes of a block
constexpr int kOipTileWaves = kOipTileBlock / 64;
constexpr int kOipTileW = 512;               // samples: 64 lanes x 8
constexpr int kOipTileH = 16;                // lines

// for `spp` samples per pixel and a horizontal radius of `rx` pixels: the halo samples either side of a tile in LDS, the
// samples and the 16-byte chunks of an LDS line, and the shift that turns a sample index into a pixel index
constexpr int oip_tile_hp(int spp, int rx) { return (rx * spp + 7) / 8 * 8; }
constexpr int oip_tile_pitch(int hp) { return kOipTileW + 2 * hp; }
constexpr int oip_tile_nch(int hp) { return oip_tile_pitch(hp) / 8; }
constexpr int oip_tile_sh(int spp) { return spp == 4 ? 2 : 0; }

// the head of every such kernel's arguments
struct OipTileArgs {
    const uint16_t *src;                     // line src_row0 of the raster: the resident window
    uint16_t *dst;                           // line out_row0
    long Ws, L;                              // samples per line, lines of the raster
    long src_row0, out_row0, out_rows;
    int W;                                   // pixels per line
    int vmin;
    int tiles_x;                             // tiles across a line
};

enum OipTileRefusal { OIP_TILE_OK = 0, OIP_TILE_BAD_ARGUMENT, OIP_TILE_IN_PLACE, OIP_TILE_WINDOW, OIP_TILE_TOO_MANY };

struct OipTilePlan {
    OipTileRefusal refused;
    long window[4];                          // OIP_TILE_WINDOW: source lines [0], [1] needed, [2] up to [3] (exclusive) resident
    OipTileArgs args;
    unsigned blocks;                         // 0: nothing to do (out_rows == 0)
    bool aligned;                            // lines, groups and bases are multiples of 16 bytes: the ALIGNED kernels apply
    int tiles_g;                             // tiles across a column group
};

// What an entry point checks and derives for output lines [out_row0, out_row0 + out_rows) of a W x L x spp raster of which
// lines [src_row0, src_row0 + src_rows) are resident at d_src, with `ry` lines of halo.  A line is `groups` column groups of
// `gw` pixels (1 and W, but for the bands of a BIL line); a tile lies inside one group.  The refusals in the order stated.
inline OipTilePlan oip_tile_plan(const uint16_t *d_src, long src_row0, long src_rows, uint16_t *d_dst, long out_row0, long out_rows, int W, long L,
                                 int spp, int valid_min, int ry, int groups, int gw)
{
    OipTilePlan p = {};
    p.refused = OIP_TILE_BAD_ARGUMENT;
    if (!d_src || !d_dst || ((uintptr_t)d_src & 1) || ((uintptr_t)d_dst & 1) || (spp != 1 && spp != 4) || W < 1 || L < 1 || ry < 0 || groups < 1 ||
        (groups > 1 && spp != 1) || gw < 1 || (long)gw * groups != W || valid_min < 0 || valid_min > 65535 || src_row0 < 0 || src_rows < 0 ||
        out_row0 < 0 || out_rows < 0 || out_rows > L || out_row0 > L - out_rows)
        return p;
    p.refused = OIP_TILE_IN_PLACE;
    if ((const uint16_t *)d_dst == d_src) return p;
    p.refused = OIP_TILE_OK;
    if (out_rows == 0) return p;
    const long first = out_row0 - ry < 0 ? 0 : out_row0 - ry;
    const long last = out_row0 + out_rows - 1 + ry > L - 1 ? L - 1 : out_row0 + out_rows - 1 + ry;
    if (first < src_row0 || last >= src_row0 + src_rows) {
        p.refused = OIP_TILE_WINDOW;
        p.window[0] = first, p.window[1] = last, p.window[2] = src_row0, p.window[3] = src_row0 + src_rows;
        return p;
    }
    const long Ws = (long)W * spp, gws = (long)gw * spp;
    p.tiles_g = (int)((gws + kOipTileW - 1) / kOipTileW);
    const long tiles_x = (long)p.tiles_g * groups, tiles_y = (out_rows + kOipTileH - 1) / kOipTileH;
    if (tiles_x * tiles_y >= (1L << 31)) {
        p.refused = OIP_TILE_TOO_MANY;
        return p;
    }
    p.args = {d_src, d_dst, Ws, L, src_row0, out_row0, out_rows, W, valid_min, (int)tiles_x};
    p.blocks = (unsigned)(tiles_x * tiles_y);
    p.aligned = Ws % 8 == 0 && gws % 8 == 0 && ((uintptr_t)d_src & 15) == 0 && ((uintptr_t)d_dst & 15) == 0;
    return p;
}

struct OipTile {
    long y0, x0;                             // first output line (of the raster) and first output sample (of the line)
    int rows, cols;                          // output lines and samples, both >= 1
    int nch;                                 // chunks of an LDS line that are read later
    int nfill;                               // chunks of the LDS image down to the last line that is
    long g0, g1;                             // the samples [g0, g1) of the tile's column group: the replicate border
};

// the tile of block `block`.  GROUPED: tiles_g tiles across a column group of gw pixels; otherwise the line is one group
template <bool GROUPED = false>
OIP_TILE_FN OipTile oip_tile_of(const OipTileArgs &a, long block, int spp, int hp, int ry, int tiles_g = 0, int gw = 0)
{
    const long ty = block / a.tiles_x;
    int tx = (int)(block - ty * a.tiles_x);
    OipTile t;
    t.g0 = 0, t.g1 = a.Ws;
    if (GROUPED) {
        const int g = tx / tiles_g;
        tx -= g * tiles_g;
        const long p0 = (long)g * gw;        // in pixels first: the compiler then sees that a group starts with a whole pixel
        t.g0 = p0 << oip_tile_sh(spp), t.g1 = (p0 + gw) << oip_tile_sh(spp);
    }
    t.y0 = a.out_row0 + ty * kOipTileH;
    const long left = a.out_row0 + a.out_rows - t.y0;
    t.rows = left < kOipTileH ? (int)left : kOipTileH;
    t.x0 = t.g0 + (long)tx * kOipTileW;
    const long wleft = t.g1 - t.x0;
    t.cols = wleft < kOipTileW ? (int)wleft : kOipTileW;
    t.nch = (t.cols + 2 * hp + 7) >> 3;
    t.nfill = (t.rows + 2 * ry) * oip_tile_nch(hp);
    return t;
}

struct OipTileChunk {
    bool read;                               // false: nothing reads the chunk, it is not filled
    long row;                                // the line of the resident window it comes from
    long s;                                  // its first sample of that line: may lie up to hp before the line or reach beyond it
};

// chunk `e` of the tile's LDS image (line e / NCH, chunk e % NCH of it).  The source line is the raster's clamped to
// [0, L - 1], which the plan found resident.
OIP_TILE_FN OipTileChunk oip_tile_chunk(const OipTileArgs &a, const OipTile &t, int e, int hp, int ry)
{
    const int r = e / oip_tile_nch(hp), c = e - r * oip_tile_nch(hp);
    if (c >= t.nch) return {false, 0, 0};
    long v = t.y0 - ry + r;
    v = v < 0 ? 0 : (v > a.L - 1 ? a.L - 1 : v);
    return {true, v - a.src_row0, t.x0 - hp + c * 8};
}

// does the chunk at sample `s` take the 16-byte copy (otherwise each of its samples is oip_tile_border_sample()'s)?  `aligned`:
// the plan's; the 8 samples have to lie inside the tile's group.
OIP_TILE_FN bool oip_tile_chunk_wide(const OipTile &t, bool aligned, long s) { return aligned && s >= t.g0 && s + 8 <= t.g1; }

// the replicate border: sample s + k of a line stands for its pixel clamped to the tile's group, channel kept.  The pixel
// into *p; returns that sample's index in the line.
OIP_TILE_FN long oip_tile_border_sample(const OipTile &t, long s, int k, int spp, long *p)
{
    const long ss = s + k, p0 = t.g0 >> oip_tile_sh(spp), p1 = (t.g1 >> oip_tile_sh(spp)) - 1;
    long q = ss >> oip_tile_sh(spp);         // arithmetic shift: the floor for ss < 0 as well
    q = q < p0 ? p0 : (q > p1 ? p1 : q);
    *p = q;
    return (q << oip_tile_sh(spp)) + (ss & (spp - 1));
}
