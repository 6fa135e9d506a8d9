// warp.hip -- bicubic resampling of a u16 raster by a displacement field given on a regular lattice of nodes: the device side
// of `oip regfix`.  The reference has no counterpart (its two geometric models are a constant shift per CCD pair and, per MSS
// band, a polynomial in the column alone).  include/oip_c.h states the arithmetic (oip_warp_grid_bicubic_u16);
// tests/_regfix_ref.py restates it.
//
//   field     d(y, x) = lerp_x(lerp_y(nodes)), Q10 integers, bilinear between the four surrounding nodes, edge value outside
//   position  s = 32 * coordinate + ((d + 16) >> 5)  in 1/32 px: a 1/32-px phase of its own for every output pixel
//   sample    cv::remap(INTER_CUBIC, BORDER_CONSTANT 0) as oip_bicubic.h states it, the source being the whole W x L raster
//
// The constant-shift and polynomial kernels (remap.hip, align.hip) share sixteen 2-D weights among the 8 pixels of a lane and
// slide a register window down the lines; a field allows neither, so a lane owns ONE output pixel and gathers its own 4 x 4
// window.  What the pixels of a tile do share is the lattice:
//   * a block owns kTileW columns x kTileH lines.  The column axis (node column, Q12 weight: two integer divisions) is
//     evaluated once per lane and serves the tile's lines; the line axis once per line into LDS;
//   * R = lerp_y of the node columns the tile spans is built once per line in LDS (at most kTileW + 2 columns, at step 1), so
//     a pixel's field is two lerps of LDS values per component, never a read of the lattice;
//   * the 32 x 4 table of 1-D bicubic weights sits in LDS as well (two 16-byte reads per pixel).
// The gather goes to global memory: neighbouring lanes' windows overlap almost entirely and the lines of a tile are re-read
// by the next line's pixels, so L1 / L2 serve nearly all of it and HBM sees each source sample about once.  Borders, fields
// that jump by many pixels between neighbours, odd widths, unaligned bases and spp 4 all take this one kernel; pixels whose
// window leaves the raster take the border summation order, the others the interior one, as OpenCV does.
#include "oip_bicubic.h"
#include "oip_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kTileW = kBlock;               // pixels: a lane per column
constexpr int kTileH = 8;                    // lines
constexpr int kNodeCols = kTileW + 2;        // node columns a tile can span (step 1)
constexpr long kMaxNodes = 1L << 27;

#define OIP_HD __host__ __device__ inline

// the node cell and the Q12 weight of one coordinate on one axis (n nodes at g0 + i * step)
struct WarpAxis {
    int c, w;
};
OIP_HD WarpAxis warp_axis(long coord, long g0, int step, int n)
{
    WarpAxis r = {0, 0};
    if (n == 1) return r;
    const long p = coord - g0, span = (long)(n - 1) * step;
    if (p <= 0) return r;                                        // left of the lattice: the edge value holds
    if (p >= span) { r.c = n - 2; r.w = 4096; return r; }
    unsigned t;
    if (p < (1L << 32)) {                                        // (nearly always: one 32-bit division)
        const unsigned q = (unsigned)p / (unsigned)step;
        r.c = (int)q;
        t = (unsigned)p - q * (unsigned)step;
    } else {
        const long q = p / step;
        r.c = (int)q;
        t = (unsigned)(p - q * step);
    }
    r.w = (int)((t * 4096u + (unsigned)step / 2u) / (unsigned)step);     // t < step <= 65536: below 2^29
    return r;
}

OIP_HD int warp_lerp(int a, int b, int w) { return a + (((b - a) * w + 2048) >> 12); }      // |b - a| <= 2^17, w <= 2^12

struct WarpArgs {
    const uint16_t *src;
    uint16_t *dst;
    const int32_t *nodes;                    // node lines j0 .. j0 + nrows - 1 of NX, then the same of NY
    const float *tab1d;
    long ny_off;                             // nrows * nx: from a node of NX to the same node of NY
    long L, src_row0, out_row0, out_rows, gx0, gy0;
    int W, nx, ny, j0, sx, sy, tiles_x, band_mask, src_vec, dst_vec;
};

// the SPP samples of one pixel as floats
template <int SPP> __device__ __forceinline__ void load_px(const uint16_t *__restrict__ p, int vec, float out[SPP])
{
    if constexpr (SPP == 4) {
        if (vec) {                                               // an 8-byte aligned base: so is every pixel
            const uint2 q = *reinterpret_cast<const uint2 *>(p);
            out[0] = (float)(q.x & 0xffffu);
            out[1] = (float)(q.x >> 16);
            out[2] = (float)(q.y & 0xffffu);
            out[3] = (float)(q.y >> 16);
            return;
        }
    }
#pragma unroll
    for (int c = 0; c < SPP; ++c) out[c] = (float)p[c];
}

template <int SPP> __device__ __forceinline__ void store_px(uint16_t *__restrict__ d, int vec, const unsigned o[SPP])
{
    if constexpr (SPP == 4) {
        if (vec) {
            *reinterpret_cast<uint2 *>(d) = make_uint2(o[0] | (o[1] << 16), o[2] | (o[3] << 16));
            return;
        }
    }
#pragma unroll
    for (int c = 0; c < SPP; ++c) d[c] = (uint16_t)o[c];
}

template <int SPP> __global__ __launch_bounds__(kBlock) void warp_grid_kernel(const WarpArgs a)
{
    __shared__ int s_r[2][kTileH][kNodeCols];
    __shared__ int s_cj[kTileH], s_wy[kTileH];
    __shared__ float4 s_tab[32];
    const int tid = threadIdx.x;
    const long ty = (long)blockIdx.x / a.tiles_x;
    const int tx = (int)((long)blockIdx.x - ty * a.tiles_x);
    const long y0 = a.out_row0 + ty * kTileH;                    // first output line of the tile (global)
    const long left = a.out_row0 + a.out_rows - y0;
    const int rows = left < kTileH ? (int)left : kTileH;         // >= 1
    const int x0 = tx * kTileW;
    const int cols = a.W - x0 < kTileW ? a.W - x0 : kTileW;      // >= 1

    if (tid < 32) s_tab[tid] = reinterpret_cast<const float4 *>(a.tab1d)[tid];
    if (tid < rows) {
        const WarpAxis q = warp_axis(y0 + tid, a.gy0, a.sy, a.ny);
        s_cj[tid] = q.c;
        s_wy[tid] = q.w;
    }
    // the node columns of the tile: ci_lo .. ci_hi + 1 (the cell index grows with the column)
    const int ci_lo = warp_axis(x0, a.gx0, a.sx, a.nx).c, ci_hi = warp_axis(x0 + cols - 1, a.gx0, a.sx, a.nx).c;
    const int ncol = a.nx == 1 ? 1 : ci_hi - ci_lo + 2;          // <= cols + 1; with one node, node ci + 1 is never read
    __syncthreads();
    for (int e = tid; e < rows * ncol; e += kBlock) {
        const int l = e / ncol, k = e - l * ncol;
        const int cj = s_cj[l], cj1 = cj + 1 < a.ny ? cj + 1 : cj, wy = s_wy[l];
        const int32_t *n0 = a.nodes + (long)(cj - a.j0) * a.nx + ci_lo + k;
        const int32_t *n1 = a.nodes + (long)(cj1 - a.j0) * a.nx + ci_lo + k;
        s_r[0][l][k] = warp_lerp(n0[0], n1[0], wy);
        s_r[1][l][k] = warp_lerp(n0[a.ny_off], n1[a.ny_off], wy);
    }
    __syncthreads();
    if (tid >= cols) return;

    const int x = x0 + tid;
    const WarpAxis ax = warp_axis(x, a.gx0, a.sx, a.nx);
    const int k = ax.c - ci_lo, k1 = k + 1 < ncol ? k + 1 : k;
    const long pitch = (long)a.W * SPP;
    for (int l = 0; l < rows; ++l) {
        const long y = y0 + l;
        const int ox = (warp_lerp(s_r[0][l][k], s_r[0][l][k1], ax.w) + 16) >> 5;        // 1/32 px
        const int oy = (warp_lerp(s_r[1][l][k], s_r[1][l][k1], ax.w) + 16) >> 5;
        const long X = (long)x + (ox >> 5) - 1, Y = y + (oy >> 5) - 1;                   // s >> 5 = coordinate + (o >> 5)
        const float4 tx4 = s_tab[ox & 31], ty4 = s_tab[oy & 31];                         // s & 31 = o & 31
        const float wx[4] = {tx4.x, tx4.y, tx4.z, tx4.w}, wy[4] = {ty4.x, ty4.y, ty4.z, ty4.w};

        float v[SPP][4][4];
        float sum[SPP];
        const bool inside = X >= 0 && X + 3 < a.W && Y >= 0 && Y + 3 < a.L;
        if (inside) {
            const uint16_t *p = a.src + (Y - a.src_row0) * pitch + X * SPP;
#pragma unroll
            for (int ky = 0; ky < 4; ++ky) {
#pragma unroll
                for (int kx = 0; kx < 4; ++kx) {
                    float s[SPP];
                    load_px<SPP>(p + ky * pitch + kx * SPP, a.src_vec, s);
#pragma unroll
                    for (int c = 0; c < SPP; ++c) v[c][ky][kx] = s[c];
                }
            }
#pragma unroll
            for (int c = 0; c < SPP; ++c) sum[c] = oip_bicubic_interior(v[c], wx, wy);
        } else {
            unsigned xmask = 0, ymask = 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                if (X + t >= 0 && X + t < a.W) xmask |= 1u << t;
                if (Y + t >= 0 && Y + t < a.L) ymask |= 1u << t;
            }
#pragma unroll
            for (int ky = 0; ky < 4; ++ky) {
#pragma unroll
                for (int kx = 0; kx < 4; ++kx) {
                    float s[SPP];
#pragma unroll
                    for (int c = 0; c < SPP; ++c) s[c] = 0.f;
                    if ((ymask & (1u << ky)) && (xmask & (1u << kx)))
                        load_px<SPP>(a.src + (Y + ky - a.src_row0) * pitch + (X + kx) * SPP, a.src_vec, s);
#pragma unroll
                    for (int c = 0; c < SPP; ++c) v[c][ky][kx] = s[c];
                }
            }
#pragma unroll
            for (int c = 0; c < SPP; ++c) sum[c] = oip_bicubic_border(v[c], wx, wy, xmask, ymask);
        }

        unsigned o[SPP];
#pragma unroll
        for (int c = 0; c < SPP; ++c) o[c] = oip_sat_u16(sum[c]);
        if (a.band_mask != (1 << SPP) - 1) {                     // bands outside the mask are copied through
            const uint16_t *q = a.src + (y - a.src_row0) * pitch + (long)x * SPP;
#pragma unroll
            for (int c = 0; c < SPP; ++c)
                if (!(a.band_mask & (1 << c))) o[c] = q[c];
        }
        uint16_t *d = a.dst + (y - a.out_row0) * pitch + (long)x * SPP;
        store_px<SPP>(d, a.dst_vec, o);
    }
}

// the node lines [*j0, *j1] that output lines [a, b) read; false for no line
bool warp_node_lines(long a, long b, int ny, long gy0, int sy, int *j0, int *j1)
{
    if (b <= a) return false;
    *j0 = warp_axis(a, gy0, sy, ny).c;
    const int c = warp_axis(b - 1, gy0, sy, ny).c;
    *j1 = c + 1 < ny ? c + 1 : c;
    return true;
}

}  // namespace

extern "C" int oip_warp_grid_src_range(long out_row0, long out_rows, long L, const int32_t *nodes_y, int nx, int ny, long gy0, int sy,
                                       int include_output, long *first, long *last)
{
    if (!nodes_y || !first || !last || out_row0 < 0 || out_rows < 0 || L < 1 || out_rows > L || out_row0 > L - out_rows || nx < 1 || ny < 1 ||
        (long)nx * ny > kMaxNodes || sy < 1 || sy > OIP_WARP_MAX_STEP)
        return OIP_E_INVALID;
    *first = *last = 0;
    int j0 = 0, j1 = 0;
    if (!warp_node_lines(out_row0, out_row0 + out_rows, ny, gy0, sy, &j0, &j1)) return OIP_OK;
    int lo = INT32_MAX, hi = INT32_MIN;
    for (long q = (long)j0 * nx; q < ((long)j1 + 1) * nx; ++q) {
        const int v = nodes_y[q];
        if (v < -OIP_WARP_MAX_Q10 || v > OIP_WARP_MAX_Q10) return OIP_E_INVALID;
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
    }
    // every field value of these lines lies between lo and hi (a lerp stays between its ends), and the first tap line
    // y + (((d + 16) >> 5) >> 5) - 1 grows with y and with d
    long f = out_row0 + (((lo + 16) >> 5) >> 5) - 1, l = out_row0 + out_rows - 1 + (((hi + 16) >> 5) >> 5) - 1 + 4;
    if (include_output) {
        f = f < out_row0 ? f : out_row0;
        l = l > out_row0 + out_rows ? l : out_row0 + out_rows;
    }
    f = f < 0 ? 0 : f;
    l = l > L ? L : l;
    if (f < l) { *first = f; *last = l; }
    return OIP_OK;
}

extern "C" int oip_warp_grid_bicubic_u16(oip_ctx *ctx, const uint16_t *d_src, long src_row0, long src_rows, uint16_t *d_dst, long out_row0,
                                         long out_rows, int W, long L, int spp, int band_mask, const int32_t *nodes_x, const int32_t *nodes_y,
                                         int nx, int ny, long gx0, long gy0, int sx, int sy)
{
    OIP_CHECK_CTX(ctx);
    if (!d_src || !d_dst || !nodes_x || !nodes_y || ((uintptr_t)d_src & 1) || ((uintptr_t)d_dst & 1) || (spp != 1 && spp != 4) || W < 1 ||
        L < 1 || band_mask < 1 || band_mask >= (1 << spp) || nx < 1 || ny < 1 || (long)nx * ny > kMaxNodes || sx < 1 || sy < 1 ||
        sx > OIP_WARP_MAX_STEP || sy > OIP_WARP_MAX_STEP || src_row0 < 0 || src_rows < 0 || src_rows > L || src_row0 > L - src_rows ||
        out_row0 < 0 || out_rows < 0 || out_rows > L || out_row0 > L - out_rows)
        return oip_fail(ctx, OIP_E_INVALID, "oip_warp_grid_bicubic_u16: bad argument");
    if ((const uint16_t *)d_dst == d_src) return oip_fail(ctx, OIP_E_INVALID, "oip_warp_grid_bicubic_u16: the call is not in place (d_dst == d_src)");
    for (long q = 0; q < (long)nx * ny; ++q)
        if (nodes_x[q] < -OIP_WARP_MAX_Q10 || nodes_x[q] > OIP_WARP_MAX_Q10 || nodes_y[q] < -OIP_WARP_MAX_Q10 || nodes_y[q] > OIP_WARP_MAX_Q10)
            return oip_fail(ctx, OIP_E_INVALID, "oip_warp_grid_bicubic_u16: node %ld is above 64 px (%d, %d in 1/1024 px)", q, nodes_x[q], nodes_y[q]);
    if (out_rows == 0) return OIP_OK;
    const bool copies = band_mask != (1 << spp) - 1;
    long first = 0, last = 0;
    if (oip_warp_grid_src_range(out_row0, out_rows, L, nodes_y, nx, ny, gy0, sy, copies, &first, &last) != OIP_OK)
        return oip_fail(ctx, OIP_E_INVALID, "oip_warp_grid_bicubic_u16: bad line window");
    if (first < last && (first < src_row0 || last > src_row0 + src_rows))
        return oip_fail(ctx, OIP_E_INVALID, "oip_warp_grid_bicubic_u16: source lines [%ld, %ld) needed, [%ld, %ld) resident", first, last, src_row0,
                        src_row0 + src_rows);
    const long tiles_x = ((long)W + kTileW - 1) / kTileW, tiles_y = (out_rows + kTileH - 1) / kTileH;
    if (tiles_x * tiles_y >= (1L << 31)) return oip_fail(ctx, OIP_E_UNSUPPORTED, "oip_warp_grid_bicubic_u16: more than 2^31 tiles in one call");

    // the node lines these output lines read go to the device during the call (pageable memory: the copy has left the
    // caller's arrays when the call returns)
    int j0 = 0, j1 = 0;
    warp_node_lines(out_row0, out_row0 + out_rows, ny, gy0, sy, &j0, &j1);
    const long nrows = j1 - j0 + 1, count = nrows * nx;
    void *work = nullptr;
    const int rc = oip_workspace(ctx, (size_t)count * 2 * sizeof(int32_t), &work);
    if (rc != OIP_OK) return rc;
    int32_t *d_nodes = static_cast<int32_t *>(work);
    OIP_HIP(ctx, hipMemcpyAsync(d_nodes, nodes_x + (long)j0 * nx, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    OIP_HIP(ctx, hipMemcpyAsync(d_nodes + count, nodes_y + (long)j0 * nx, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));

    WarpArgs a;
    a.src = d_src;
    a.dst = d_dst;
    a.nodes = d_nodes;
    a.tab1d = ctx->d_tab1d;
    a.ny_off = count;
    a.L = L;
    a.src_row0 = src_row0;
    a.out_row0 = out_row0;
    a.out_rows = out_rows;
    a.gx0 = gx0;
    a.gy0 = gy0;
    a.W = W;
    a.nx = nx;
    a.ny = ny;
    a.j0 = j0;
    a.sx = sx;
    a.sy = sy;
    a.tiles_x = (int)tiles_x;
    a.band_mask = band_mask;
    a.src_vec = ((uintptr_t)d_src & 7) == 0;
    a.dst_vec = ((uintptr_t)d_dst & 7) == 0;
    const unsigned blocks = (unsigned)(tiles_x * tiles_y);
    OipProfScope prof(ctx, "warp_grid_kernel");
    if (spp == 1) hipLaunchKernelGGL(warp_grid_kernel<1>, dim3(blocks), dim3(kBlock), 0, ctx->stream, a);
    else hipLaunchKernelGGL(warp_grid_kernel<4>, dim3(blocks), dim3(kBlock), 0, ctx->stream, a);
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}
