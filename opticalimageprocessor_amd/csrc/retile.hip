// retile.hip -- the device side of `oip cog` and of tiled TIFF input: the two layout kernels between a raster and its
// tile-major form (include/oip_c.h: oip_retile_u16, oip_untile_u16).  The reference has no counterpart (it writes strips and
// leaves tiling to gdal_translate); the siblings here are overview.hip and quicklook.hip, whose layout the kernels follow.
//
//   image: w x h pixels of spp u16 samples (1, or 4 pixel-interleaved); tiles T x T, T a multiple of 16; tx = ceil(w / T) by
//   ty = ceil(h / T) tiles, row-major.  Tile-major form: ty * tx consecutive blocks of T rows of T * spp samples;
//   sample (r, c, ch) of tile (j, i) = image sample (min(j T + r, h - 1), min(i T + c, w - 1), ch)
//
// so the part of an edge tile outside the image repeats the last column (per channel) and the last line -- with predictor 2
// that codes to runs of zeros -- and every byte of the tile-major buffer is defined.  The inverse writes the w x h x spp samples
// of the image and never looks at the padding.
//
// Layout / mapping.  Copy kernels, HBM-bound: 2 B in and 2 B out per sample, no LDS, no atomics.  A lane owns one 16-byte word
// of the RASTER line (8 samples at spp = 1, 2 pixels at spp = 4) and walks the rows of a tile row with it: the 64 lanes of a wave
// cover 1 KiB of consecutive raster bytes, which cross from one tile into the next every T * spp * 2 bytes (at least 32), so the
// raster side moves whole cache lines and the tile side whole tile rows (T >= 64 at spp 1: whole cache lines too).  A row of a
// tile is a multiple of 32 bytes, so the 16-byte words of the tile side are always aligned; four rows (four 16-byte loads) are
// in flight per lane.  grid.y cuts the selected tile rows into ranges of at most 64 rows of one tile row.  A workgroup whose
// words and rows all lie inside the image runs the body without clamps; the others -- the right end of the last tile column,
// the last tile row -- the clamped one (the choice is uniform over the workgroup).  All offsets are 64 bit: a strip has more
// than 2^31 samples.
//
// A raster the vector form cannot take (a pitch that is not a multiple of 8 samples, a base that is not on a 16-byte boundary:
// the deeper levels of the pyramid of an odd-width image) goes to the lane-per-sample kernels: 2-byte loads and stores, the
// same result.
#include "oip_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kRows = 4;                     // rows (16-byte loads) in flight per lane
constexpr int kRangeRows = 64;               // rows of one tile row that a workgroup walks (T is a multiple of 16, so of kRows)
constexpr long kMaxGridY = 65535;

// what every kernel here is handed besides its two buffers
struct RetileGeo {
    long pitch;                              // samples between raster lines
    long w, h;                               // pixels, lines
    long tx;                                 // tiles across
    long tile_row0;                          // first tile row of the call: the tile-major buffer starts there
    long y0;                                 // grid.y of this launch starts at range y0 (a call of more than 65535 ranges is several launches)
    int T, chunks;                           // tile size; ranges per tile row = ceil(T / kRangeRows)
};

// the range of a workgroup: tile row jr of the call (j of the image), rows [rs, re) of it
struct Range { long jr, j; int rs, re; };
__device__ __forceinline__ Range block_range(const RetileGeo &g)
{
    const long by = g.y0 + blockIdx.y;
    Range r;
    r.jr = by / g.chunks;
    r.j = g.tile_row0 + r.jr;
    r.rs = (int)(by - r.jr * g.chunks) * kRangeRows;
    r.re = r.rs + kRangeRows < g.T ? r.rs + kRangeRows : g.T;
    return r;
}

// the 16-byte word at sample s0 of a raster line of ns samples, samples past the line repeating its last pixel
template <int SPP> __device__ __forceinline__ uint4 load_clamped(const uint16_t *__restrict__ line, long s0, long ns, long w)
{
    if (s0 + 8 <= ns) return *reinterpret_cast<const uint4 *>(line + s0);
    unsigned v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const long s = s0 + k;
        long idx;
        if (SPP == 1) idx = s < ns ? s : ns - 1;
        else { const long p = s >> 2; idx = (p < w ? p : w - 1) * 4 + (s & 3); }
        v[k] = line[idx];
    }
    return make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
}

// the first `live` (1..8) samples of a word into a raster line
__device__ __forceinline__ void store_partial(uint16_t *o, uint4 q, int live)
{
    const unsigned p[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (k < live) o[k] = (uint16_t)(p[k >> 1] >> (16 * (k & 1)));
}

template <int SPP>
__global__ __launch_bounds__(kBlock) void retile_u16_kernel(const uint16_t *__restrict__ src, RetileGeo g, uint16_t *__restrict__ dst)
{
    const int wpt = g.T * SPP / 8;                             // words of a tile row
    const long nwords = g.tx * wpt;                            // words of the padded line
    const long ns = g.w * SPP;                                 // samples of a line that belong to the image
    const Range b = block_range(g);
    long wend = ((long)blockIdx.x + 1) * kBlock;
    if (wend > nwords) wend = nwords;
    const bool edge = b.j * g.T + b.re > g.h || wend * 8 > ns; // (uniform) a row or a word of this workgroup leaves the image
    const long wx = (long)blockIdx.x * kBlock + threadIdx.x;
    if (wx >= nwords) return;
    const long i = wx / wpt;
    const int q = (int)(wx - i * wpt);
    const long trow = (long)g.T * SPP;                         // samples of a tile row
    uint16_t *d = dst + ((b.jr * g.tx + i) * g.T + b.rs) * trow + q * 8;
    const long s0 = wx * 8;
    const long y0 = b.j * g.T + b.rs;
    if (!edge) {
        const uint16_t *s = src + y0 * g.pitch + s0;
        for (int r = b.rs; r < b.re; r += kRows) {
            uint4 v[kRows];
#pragma unroll
            for (int u = 0; u < kRows; ++u) v[u] = *reinterpret_cast<const uint4 *>(s + u * g.pitch);
#pragma unroll
            for (int u = 0; u < kRows; ++u) *reinterpret_cast<uint4 *>(d + u * trow) = v[u];
            s += kRows * g.pitch;
            d += kRows * trow;
        }
    } else {
        long y = y0;
        for (int r = b.rs; r < b.re; r += kRows) {
            uint4 v[kRows];
#pragma unroll
            for (int u = 0; u < kRows; ++u) {
                const long yy = y + u < g.h ? y + u : g.h - 1;
                v[u] = load_clamped<SPP>(src + yy * g.pitch, s0, ns, g.w);
            }
#pragma unroll
            for (int u = 0; u < kRows; ++u) *reinterpret_cast<uint4 *>(d + u * trow) = v[u];
            y += kRows;
            d += kRows * trow;
        }
    }
}

template <int SPP>
__global__ __launch_bounds__(kBlock) void untile_u16_kernel(const uint16_t *__restrict__ src, RetileGeo g, uint16_t *__restrict__ dst)
{
    const int wpt = g.T * SPP / 8;
    const long ns = g.w * SPP;
    const long nwords = (ns + 7) / 8;                          // words of the image line, the last one maybe partial
    const Range b = block_range(g);
    long wend = ((long)blockIdx.x + 1) * kBlock;
    if (wend > nwords) wend = nwords;
    const bool edge = b.j * g.T + b.re > g.h || wend * 8 > ns;
    const long wx = (long)blockIdx.x * kBlock + threadIdx.x;
    if (wx >= nwords) return;
    const long i = wx / wpt;
    const int q = (int)(wx - i * wpt);
    const long trow = (long)g.T * SPP;
    const uint16_t *s = src + ((b.jr * g.tx + i) * g.T + b.rs) * trow + q * 8;
    const long s0 = wx * 8;
    const long y0 = b.j * g.T + b.rs;
    uint16_t *d = dst + y0 * g.pitch + s0;
    if (!edge) {
        for (int r = b.rs; r < b.re; r += kRows) {
            uint4 v[kRows];
#pragma unroll
            for (int u = 0; u < kRows; ++u) v[u] = *reinterpret_cast<const uint4 *>(s + u * trow);
#pragma unroll
            for (int u = 0; u < kRows; ++u) *reinterpret_cast<uint4 *>(d + u * g.pitch) = v[u];
            s += kRows * trow;
            d += kRows * g.pitch;
        }
    } else {
        const int live = ns - s0 < 8 ? (int)(ns - s0) : 8;     // samples of the word inside the line
        long y = y0;
        for (int r = b.rs; r < b.re && y < g.h; r += kRows) {
            uint4 v[kRows];
#pragma unroll
            for (int u = 0; u < kRows; ++u) v[u] = *reinterpret_cast<const uint4 *>(s + u * trow);      // (inside the tile: T is a multiple of kRows)
#pragma unroll
            for (int u = 0; u < kRows; ++u) {
                if (y + u >= g.h) break;
                if (live == 8) *reinterpret_cast<uint4 *>(d + u * g.pitch) = v[u];
                else store_partial(d + u * g.pitch, v[u], live);
            }
            y += kRows;
            s += kRows * trow;
            d += kRows * g.pitch;
        }
    }
}

// any pitch / alignment: a lane owns one sample of the padded line (retile) or of the image line (untile)
__global__ __launch_bounds__(kBlock) void retile_u16_sample_kernel(const uint16_t *__restrict__ src, RetileGeo g, int spp, uint16_t *__restrict__ dst)
{
    const long trow = (long)g.T * spp;
    const long t = (long)blockIdx.x * kBlock + threadIdx.x;
    if (t >= g.tx * trow) return;
    const Range b = block_range(g);
    const long i = t / trow, q = t - i * trow;
    const long p = t / spp, c = t - p * spp;
    const long idx = (p < g.w ? p : g.w - 1) * spp + c;
    uint16_t *d = dst + ((b.jr * g.tx + i) * g.T + b.rs) * trow + q;
    long y = b.j * g.T + b.rs;
    for (int r = b.rs; r < b.re; ++r, ++y, d += trow) *d = src[(y < g.h ? y : g.h - 1) * g.pitch + idx];
}

__global__ __launch_bounds__(kBlock) void untile_u16_sample_kernel(const uint16_t *__restrict__ src, RetileGeo g, int spp, uint16_t *__restrict__ dst)
{
    const long trow = (long)g.T * spp;
    const long t = (long)blockIdx.x * kBlock + threadIdx.x;
    if (t >= g.w * spp) return;
    const Range b = block_range(g);
    const long i = t / trow, q = t - i * trow;
    const uint16_t *s = src + ((b.jr * g.tx + i) * g.T + b.rs) * trow + q;
    long y = b.j * g.T + b.rs;
    uint16_t *d = dst + y * g.pitch + t;
    for (int r = b.rs; r < b.re && y < g.h; ++r, ++y, s += trow, d += g.pitch) *d = *s;
}

// the checks both entry points share; fills g and says whether the raster takes the vector form
int retile_args(oip_ctx *ctx, const char *name, const void *d_img, long pitch, int w, long h, int spp, int T, long tile_row0, long tile_rows,
                const void *d_tiles, RetileGeo *g, bool *vec)
{
    if (w < 1 || h < 1 || h >= (1L << 31) || (spp != 1 && spp != 4) || (long)w * spp >= (1L << 31) || !d_img || !d_tiles || d_img == d_tiles ||
        ((uintptr_t)d_img & 1))
        return oip_fail(ctx, OIP_E_INVALID, "%s: bad argument", name);
    if (T < 16 || T > 1024 || T % 16 != 0) return oip_fail(ctx, OIP_E_INVALID, "%s: the tile size is a multiple of 16 in 16..1024", name);
    if (pitch < (long)w * spp) return oip_fail(ctx, OIP_E_INVALID, "%s: the pitch is shorter than the line", name);
    if ((uintptr_t)d_tiles & 15) return oip_fail(ctx, OIP_E_INVALID, "%s: the tile-major buffer is not 16-byte aligned", name);
    const long ty = (h + T - 1) / T;
    if (tile_row0 < 0 || tile_rows < 0 || tile_row0 > ty || tile_rows > ty - tile_row0)
        return oip_fail(ctx, OIP_E_INVALID, "%s: tile rows [%ld, %ld) outside the %ld of the image", name, tile_row0, tile_row0 + tile_rows, ty);
    g->pitch = pitch;
    g->w = w;
    g->h = h;
    g->tx = ((long)w + T - 1) / T;
    g->tile_row0 = tile_row0;
    g->y0 = 0;
    g->T = T;
    g->chunks = (T + kRangeRows - 1) / kRangeRows;
    *vec = pitch % 8 == 0 && ((uintptr_t)d_img & 15) == 0;
    return OIP_OK;
}

}  // namespace

extern "C" int oip_retile_u16(oip_ctx *ctx, const uint16_t *d_img, long src_pitch, int w, long h, int spp, int T, long tile_row0, long tile_rows,
                              uint16_t *d_tiles)
{
    OIP_CHECK_CTX(ctx);
    RetileGeo g;
    bool vec = false;
    if (int rc = retile_args(ctx, "oip_retile_u16", d_img, src_pitch, w, h, spp, T, tile_row0, tile_rows, d_tiles, &g, &vec)) return rc;
    if (tile_rows == 0) return OIP_OK;
    OipProfScope prof(ctx, vec ? "retile_u16_kernel" : "retile_u16_sample_kernel");
    const long lanes = vec ? g.tx * (T * spp / 8) : g.tx * (long)T * spp;
    const unsigned gx = (unsigned)((lanes + kBlock - 1) / kBlock);
    const long ranges = tile_rows * g.chunks;
    for (g.y0 = 0; g.y0 < ranges; g.y0 += kMaxGridY) {
        const dim3 grid(gx, (unsigned)(ranges - g.y0 < kMaxGridY ? ranges - g.y0 : kMaxGridY));
        if (!vec) hipLaunchKernelGGL(retile_u16_sample_kernel, grid, dim3(kBlock), 0, ctx->stream, d_img, g, spp, d_tiles);
        else if (spp == 1) hipLaunchKernelGGL(retile_u16_kernel<1>, grid, dim3(kBlock), 0, ctx->stream, d_img, g, d_tiles);
        else hipLaunchKernelGGL(retile_u16_kernel<4>, grid, dim3(kBlock), 0, ctx->stream, d_img, g, d_tiles);
    }
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}

extern "C" int oip_untile_u16(oip_ctx *ctx, const uint16_t *d_tiles, int w, long h, int spp, int T, long tile_row0, long tile_rows, uint16_t *d_img,
                              long dst_pitch)
{
    OIP_CHECK_CTX(ctx);
    RetileGeo g;
    bool vec = false;
    if (int rc = retile_args(ctx, "oip_untile_u16", d_img, dst_pitch, w, h, spp, T, tile_row0, tile_rows, d_tiles, &g, &vec)) return rc;
    if (tile_rows == 0) return OIP_OK;
    OipProfScope prof(ctx, vec ? "untile_u16_kernel" : "untile_u16_sample_kernel");
    const long ns = (long)w * spp;
    const long lanes = vec ? (ns + 7) / 8 : ns;
    const unsigned gx = (unsigned)((lanes + kBlock - 1) / kBlock);
    const long ranges = tile_rows * g.chunks;
    for (g.y0 = 0; g.y0 < ranges; g.y0 += kMaxGridY) {
        const dim3 grid(gx, (unsigned)(ranges - g.y0 < kMaxGridY ? ranges - g.y0 : kMaxGridY));
        if (!vec) hipLaunchKernelGGL(untile_u16_sample_kernel, grid, dim3(kBlock), 0, ctx->stream, d_tiles, g, spp, d_img);
        else if (spp == 1) hipLaunchKernelGGL(untile_u16_kernel<1>, grid, dim3(kBlock), 0, ctx->stream, d_tiles, g, d_img);
        else hipLaunchKernelGGL(untile_u16_kernel<4>, grid, dim3(kBlock), 0, ctx->stream, d_tiles, g, d_img);
    }
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}
