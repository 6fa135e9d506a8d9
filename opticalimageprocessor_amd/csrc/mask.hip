// mask.hip -- the no-data / saturation / cloud mask of a u16 raster on gfx950 (`oip mask`): one flag byte per C x C cell, then
// an opening and a buffer on the grid of cells.  The reference has no counterpart.  include/oip_c.h states every byte.
//
// Cells.  HBM-bound, read-only: 2 B per sample in, one byte per cell out.  The layout is noise.hip's: a lane owns one 16-byte
// vector (8 samples: 2 pixels at spp 4) of each of the C lines of a cell line, adjacent lanes read adjacent 16 bytes, and
// V = C * spp / 8 adjacent lanes share a cell (2, 4, 8 at spp 4; 1, 2 at spp 1 C 8, 16; at spp 1 C 4 a lane holds two cells).
// A pixel is classed once (no data / saturated / good) from the minimum and maximum of its channels; the three pixel counts of
// a cell travel in one packed word (10 bits each: a cell has at most 256 pixels) and the four channel sums over the good pixels
// fit 32 bits (256 * 65535 < 2^24).  The V partial results meet in a butterfly of wave shuffles (V divides 64: a cell never
// straddles a wave), the first lane of the cell evaluates the tests in 64-bit integers and stores the byte.  Every lane keeps
// its six counters in registers over all the cell lines it walks; they meet in LDS, and a workgroup adds each counter to HBM
// once.  grid.y walks the cell lines with a stride of gridDim.y, as in noise.hip.  The last vector of a line that is no multiple
// of 8 samples is read sample by sample: nothing outside the window is touched.
//
// Anything the vector form cannot take (a pitch that is not a multiple of 8 samples, a window that does not start on a 16-byte
// boundary) goes to the cell-per-lane kernel: 2-byte loads, the same bytes.
//
// Morphology.  Bit 16 of the grid is packed into 64-bit words, one bit per cell, 64 cells per word along a line (__ballot).
// Erosion and dilation by a square are separable: a vertical pass (AND / OR over the 2R+1 word lines that lie inside the grid)
// and a horizontal pass (AND / OR over the 2R+1 shifts of the 192 bits around a word; R <= 64 never reaches further).  Bits
// outside the grid count as set for an erosion and as clear for a dilation: the horizontal pass forces the tail bits of a
// line's last word accordingly when it loads them.  The largest grid (7500 x 25000 cells) is 2.9 M words; the plain loops over
// the shifts are a few G word operations, small beside the cells pass.  The last kernel unpacks the opening and the buffer
// into bits 4 and 8 and counts them with __popcll, one atomicAdd per counter and workgroup.
#include "oip_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kPerCu = 8;                    // workgroups per CU over the whole grid

struct MaskParams {
    unsigned vmin, sat;
    long long full;
    int band[4];                             // channel of blue, green, red, nir
    int q[4];                                // bright, white, hot, ndvi in q8; -1: disabled
};

// the three pixel counts of a cell in one word
constexpr unsigned kIncNd = 1u, kIncSat = 1u << 10, kIncGood = 1u << 20;

__device__ __forceinline__ unsigned pick4(const unsigned s[4], int i)
{
    return i == 0 ? s[0] : i == 1 ? s[1] : i == 2 ? s[2] : s[3];
}

// the flag byte of one cell from its packed pixel counts, its channel sums over the good pixels and its pixel count
__device__ __forceinline__ unsigned mask_cell_byte(unsigned acc, const unsigned s[4], unsigned n_cell, int spp, const MaskParams &p, bool *tested)
{
    const unsigned n_nd = acc & 1023u, n_sat = (acc >> 10) & 1023u;
    const long long m = (long long)(acc >> 20);
    unsigned f = (n_nd ? OIP_MASK_NODATA : 0u) | (n_sat ? OIP_MASK_SATURATED : 0u);
    *tested = spp == 4 && 2 * m >= (long long)n_cell && m >= 1;
    if (*tested) {
        const long long b = pick4(s, p.band[0]), g = pick4(s, p.band[1]), r = pick4(s, p.band[2]), n = pick4(s, p.band[3]);
        const long long V = b + g + r;
        const long long mx = b > g ? (b > r ? b : r) : (g > r ? g : r);
        const long long mn = b < g ? (b < r ? b : r) : (g < r ? g : r);
        bool ok = true;
        if (p.q[0] >= 0) ok = ok && 256 * V >= 3 * m * p.full * p.q[0];
        if (p.q[1] >= 0) ok = ok && 768 * (mx - mn) <= p.q[1] * V;
        if (p.q[2] >= 0) ok = ok && 256 * (2 * b - r) >= 2 * m * p.full * p.q[2];
        if (p.q[3] >= 0) ok = ok && 256 * (n - r) <= p.q[3] * (n + r);
        if (ok) f |= OIP_MASK_CANDIDATE;
    }
    return f;
}

// what a lane adds to its counters for one cell: {cells, NODATA, SATURATED, tested, CANDIDATE, saturated pixels}
__device__ __forceinline__ void mask_count(unsigned long long cnt[6], unsigned f, bool tested, unsigned acc)
{
    cnt[0] += 1ull;
    cnt[1] += (f & OIP_MASK_NODATA) ? 1ull : 0ull;
    cnt[2] += (f & OIP_MASK_SATURATED) ? 1ull : 0ull;
    cnt[3] += tested ? 1ull : 0ull;
    cnt[4] += (f & OIP_MASK_CANDIDATE) ? 1ull : 0ull;
    cnt[5] += (unsigned long long)((acc >> 10) & 1023u);
}

// the six counters of a workgroup into d_counts[0..4] and [7]; every lane of the workgroup arrives here
__device__ __forceinline__ void mask_flush(const unsigned long long cnt[6], unsigned long long *__restrict__ counts)
{
    __shared__ unsigned long long sh[6];
    if (threadIdx.x < 6) sh[threadIdx.x] = 0ull;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 6; ++k)
        if (cnt[k]) atomicAdd(&sh[k], cnt[k]);
    __syncthreads();
    if (counts && threadIdx.x < 6 && sh[threadIdx.x]) atomicAdd(counts + (threadIdx.x < 5 ? threadIdx.x : 7), sh[threadIdx.x]);
}

template <int SPP, int C>
__global__ __launch_bounds__(kBlock) void mask_cells_u16_kernel(const uint16_t *__restrict__ img, long pitch, int w, long rows, long nby,
                                                                MaskParams p, uint8_t *__restrict__ flags, long flag_pitch,
                                                                unsigned long long *__restrict__ counts)
{
    constexpr int K = (SPP == 1 && C == 4) ? 2 : 1;          // cells in a lane's vector
    constexpr int V = K == 2 ? 1 : C * SPP / 8;              // lanes (16-byte vectors) per cell
    constexpr int PPV = 8 / SPP;                             // pixels per vector
    constexpr int G = C < 8 ? C : 8;                         // lines loaded ahead of their use
    const long line = (long)w * SPP;                         // samples of a line
    const int nvec = (int)((line + 7) / 8), gw = (w + C - 1) / C;
    const int vx = blockIdx.x * kBlock + threadIdx.x;
    const bool active = vx < nvec;                           // (an inactive lane loads nothing and still takes part in the shuffles)
    const bool whole = (long)vx * 8 + 8 <= line;             // the vector lies inside the line
    const int px0 = vx * PPV;
    const int pv = active ? (w - px0 < PPV ? w - px0 : PPV) : 0;      // pixels of the vector that lie inside the line
    const int g = vx % V;
    unsigned long long cnt[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    for (long by = blockIdx.y; by < nby; by += gridDim.y) {
        const int nl = rows - by * C < C ? (int)(rows - by * C) : C;
        unsigned acc[K], s[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] = 0u;
        if (active) {
            const uint16_t *src = img + by * C * pitch + (long)vx * 8;
#pragma unroll
            for (int h = 0; h < C / G; ++h) {
                uint4 v[G];
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    v[j] = make_uint4(0u, 0u, 0u, 0u);       // a line or a sample outside the window: zeros, and lim keeps them uncounted
                    if (h * G + j < nl) {
                        const uint16_t *l = src + (long)(h * G + j) * pitch;
                        if (whole) {
                            v[j] = *reinterpret_cast<const uint4 *>(l);
                        } else {
                            unsigned t[8];
#pragma unroll
                            for (int i = 0; i < 8; ++i) t[i] = (long)vx * 8 + i < line ? (unsigned)l[i] : 0u;
                            v[j] = make_uint4(t[0] | t[1] << 16, t[2] | t[3] << 16, t[4] | t[5] << 16, t[6] | t[7] << 16);
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < G; ++j) {
                    const int lim = h * G + j < nl ? pv : 0;
                    const unsigned d[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
                    if (SPP == 4) {
#pragma unroll
                        for (int q = 0; q < 2; ++q) {
                            const unsigned c0 = d[2 * q] & 0xffffu, c1 = d[2 * q] >> 16, c2 = d[2 * q + 1] & 0xffffu, c3 = d[2 * q + 1] >> 16;
                            const unsigned lo = min(min(c0, c1), min(c2, c3)), hi = max(max(c0, c1), max(c2, c3));
                            const bool nd = lo < p.vmin, st = !nd && hi >= p.sat, good = !nd && !st;
                            const unsigned inc = nd ? kIncNd : st ? kIncSat : kIncGood;
                            acc[0] += q < lim ? inc : 0u;
                            s[0] += good ? c0 : 0u;          // (a pixel outside the window is zeros: it adds nothing)
                            s[1] += good ? c1 : 0u;
                            s[2] += good ? c2 : 0u;
                            s[3] += good ? c3 : 0u;
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < 8; ++i) {
                            const unsigned u = (i & 1) ? d[i >> 1] >> 16 : d[i >> 1] & 0xffffu;
                            const bool nd = u < p.vmin, st = !nd && u >= p.sat;
                            const unsigned inc = nd ? kIncNd : st ? kIncSat : kIncGood;
                            acc[K == 2 ? i >> 2 : 0] += i < lim ? inc : 0u;
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int m = 1; m < V; m <<= 1) {
            acc[0] += __shfl_xor(acc[0], m);
            if (SPP == 4) {
#pragma unroll
                for (int c = 0; c < 4; ++c) s[c] += __shfl_xor(s[c], m);
            }
        }
        if (active && g == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int bx = K == 2 ? vx * 2 + k : vx / V;
                if (bx < gw) {
                    const unsigned cw = w - bx * C < C ? (unsigned)(w - bx * C) : (unsigned)C;
                    bool tested;
                    const unsigned f = mask_cell_byte(acc[k], s, cw * (unsigned)nl, SPP, p, &tested);
                    flags[by * flag_pitch + bx] = (uint8_t)f;
                    mask_count(cnt, f, tested, acc[k]);
                }
            }
        }
    }
    mask_flush(cnt, counts);
}

// any pitch / alignment: a lane owns one cell
__global__ __launch_bounds__(kBlock) void mask_cells_u16_any_kernel(const uint16_t *__restrict__ img, long pitch, int w, long rows, long nby, int spp,
                                                                    int C, MaskParams p, uint8_t *__restrict__ flags, long flag_pitch,
                                                                    unsigned long long *__restrict__ counts)
{
    const int gw = (w + C - 1) / C;
    const int bx = blockIdx.x * kBlock + threadIdx.x;
    unsigned long long cnt[6] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    if (bx < gw) {
        const int cw = w - bx * C < C ? w - bx * C : C;
        for (long by = blockIdx.y; by < nby; by += gridDim.y) {
            const int nl = rows - by * C < C ? (int)(rows - by * C) : C;
            const uint16_t *src = img + by * C * pitch + (long)bx * C * spp;
            unsigned acc = 0u, s[4] = {0u, 0u, 0u, 0u};
            for (int j = 0; j < nl; ++j) {
                const uint16_t *l = src + (long)j * pitch;
                for (int x = 0; x < cw; ++x) {
                    unsigned c[4] = {0u, 0u, 0u, 0u}, lo = 0xffffffffu, hi = 0u;
                    for (int k = 0; k < spp; ++k) {
                        c[k] = l[x * spp + k];
                        lo = min(lo, c[k]);
                        hi = max(hi, c[k]);
                    }
                    const bool nd = lo < p.vmin, st = !nd && hi >= p.sat, good = !nd && !st;
                    acc += nd ? kIncNd : st ? kIncSat : kIncGood;
#pragma unroll
                    for (int k = 0; k < 4; ++k) s[k] += good ? c[k] : 0u;
                }
            }
            bool tested;
            const unsigned f = mask_cell_byte(acc, s, (unsigned)(cw * nl), spp, p, &tested);
            flags[by * flag_pitch + bx] = (uint8_t)f;
            mask_count(cnt, f, tested, acc);
        }
    }
    mask_flush(cnt, counts);
}

// ---- morphology on words of 64 cells --------------------------------------------------------------------------------------
// word (y, k) of the plane = bit 16 of cells (y, 64 k .. 64 k + 63); one wave per word, bits outside the grid clear
__global__ __launch_bounds__(kBlock) void mask_pack_kernel(const uint8_t *__restrict__ flags, long flag_pitch, int gw, long gh, int wpl,
                                                           unsigned long long *__restrict__ plane)
{
    const long words = gh * wpl;
    const int lane = threadIdx.x & 63;
    for (long i = (long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); i < words; i += (long)gridDim.x * (kBlock / 64)) {
        const long y = i / wpl;
        const long x = (i % wpl) * 64 + lane;
        const bool set = x < gw && (flags[y * flag_pitch + x] & OIP_MASK_CANDIDATE);
        const unsigned long long b = __ballot(set);
        if (lane == 0) plane[i] = b;
    }
}

// AND (erode) or OR over the word lines y - R .. y + R that lie inside the grid
template <bool ERODE>
__global__ __launch_bounds__(kBlock) void mask_morph_v_kernel(const unsigned long long *__restrict__ in, unsigned long long *__restrict__ out,
                                                              long gh, int wpl, int R)
{
    const long words = gh * wpl;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < words; i += (long)gridDim.x * kBlock) {
        const long y = i / wpl;
        const long k = i % wpl;
        const long y0 = y - R < 0 ? 0 : y - R, y1 = y + R > gh - 1 ? gh - 1 : y + R;
        unsigned long long a = ERODE ? ~0ull : 0ull;
        for (long j = y0; j <= y1; ++j) {
            const unsigned long long v = in[j * wpl + k];
            a = ERODE ? a & v : a | v;
        }
        out[i] = a;
    }
}

// AND (erode) or OR over the shifts -R .. R of a line; R <= 64: the words k - 1, k, k + 1 hold every bit that counts.  Bits
// outside the grid are set for an erosion and clear for a dilation, whatever the line's last word holds there.
template <bool ERODE>
__global__ __launch_bounds__(kBlock) void mask_morph_h_kernel(const unsigned long long *__restrict__ in, unsigned long long *__restrict__ out,
                                                              int gw, long gh, int wpl, int R)
{
    const long words = gh * wpl;
    const unsigned long long outside = ERODE ? ~0ull : 0ull;
    const int tail = gw - (wpl - 1) * 64;                                // cells of a line's last word: 1 .. 64
    const unsigned long long tmask = tail == 64 ? ~0ull : (1ull << tail) - 1ull;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < words; i += (long)gridDim.x * kBlock) {
        const int k = (int)(i % wpl);
        unsigned long long mid = in[i], lo = outside, hi = outside;
        if (k == wpl - 1) mid = ERODE ? mid | ~tmask : mid & tmask;
        if (k > 0) lo = in[i - 1];
        if (k + 1 < wpl) {
            hi = in[i + 1];
            if (k + 1 == wpl - 1) hi = ERODE ? hi | ~tmask : hi & tmask;
        }
        unsigned long long a = mid;
        for (int t = 1; t <= R; ++t) {
            // bit x of `up` is cell x + t, bit x of `dn` is cell x - t
            const unsigned long long up = t == 64 ? hi : (mid >> t) | (hi << (64 - t));
            const unsigned long long dn = t == 64 ? lo : (mid << t) | (lo >> (64 - t));
            a = ERODE ? a & up & dn : a | up | dn;
        }
        out[i] = a;
    }
}

// bits 4 and 8 of the flags from the opening and its dilation; one wave per word; counts[5] += CLOUD, counts[6] += BUFFER
__global__ __launch_bounds__(kBlock) void mask_unpack_kernel(uint8_t *__restrict__ flags, long flag_pitch, int gw, long gh, int wpl,
                                                             const unsigned long long *__restrict__ open, const unsigned long long *__restrict__ dil,
                                                             unsigned long long *__restrict__ counts)
{
    __shared__ unsigned long long sh[2];
    if (threadIdx.x < 2) sh[threadIdx.x] = 0ull;
    __syncthreads();
    const long words = gh * wpl;
    const int lane = threadIdx.x & 63;
    unsigned long long n_cloud = 0ull, n_buffer = 0ull;
    for (long i = (long)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); i < words; i += (long)gridDim.x * (kBlock / 64)) {
        const long y = i / wpl;
        const int k = (int)(i % wpl);
        const int cells = gw - k * 64 < 64 ? gw - k * 64 : 64;
        const unsigned long long m = cells == 64 ? ~0ull : (1ull << cells) - 1ull;
        const unsigned long long o = open[i] & m, b = dil[i] & m & ~o;
        if (lane < cells) {
            uint8_t *f = flags + y * flag_pitch + (long)k * 64 + lane;
            const unsigned keep = *f & ~(unsigned)(OIP_MASK_CLOUD | OIP_MASK_BUFFER);
            *f = (uint8_t)(keep | ((o >> lane) & 1ull ? OIP_MASK_CLOUD : 0u) | ((b >> lane) & 1ull ? OIP_MASK_BUFFER : 0u));
        }
        if (lane == 0) {
            n_cloud += (unsigned long long)__popcll(o);
            n_buffer += (unsigned long long)__popcll(b);
        }
    }
    if (n_cloud) atomicAdd(&sh[0], n_cloud);
    if (n_buffer) atomicAdd(&sh[1], n_buffer);
    __syncthreads();
    if (counts && threadIdx.x < 2 && sh[threadIdx.x]) atomicAdd(counts + 5 + threadIdx.x, sh[threadIdx.x]);
}

int grid_1d(const oip_ctx *ctx, long items)
{
    long g = (items + kBlock - 1) / kBlock;
    const long cap = (long)ctx->cu_count * kPerCu;
    if (g > cap) g = cap;
    return (int)(g < 1 ? 1 : g);
}

}  // namespace

extern "C" int oip_mask_cells_u16(oip_ctx *ctx, const uint16_t *d_src, long pitch, int w, long rows, int spp, int cell, int valid_min, int sat_level,
                                  int full_scale, const int *band, int bright_q8, int white_q8, int hot_q8, int ndvi_q8, uint8_t *d_flags,
                                  long flag_pitch, uint64_t *d_counts)
{
    OIP_CHECK_CTX(ctx);
    const int q[4] = {bright_q8, white_q8, hot_q8, ndvi_q8};
    bool ok = (cell == 4 || cell == 8 || cell == 16) && (spp == 1 || spp == 4) && w >= 0 && rows >= 0 && pitch >= (long)w * spp && d_src && d_flags &&
              !((uintptr_t)d_src & 1) && !((uintptr_t)d_counts & 7) && valid_min >= 0 && valid_min <= 65535 && sat_level >= 1 && sat_level <= 65535 &&
              full_scale >= 1 && full_scale <= 65535;
    for (int k = 0; k < 4; ++k) ok = ok && q[k] >= -1 && q[k] <= 256;
    if (ok && flag_pitch < (w + cell - 1) / cell) ok = false;
    MaskParams p;
    p.vmin = (unsigned)valid_min;
    p.sat = (unsigned)sat_level;
    p.full = full_scale;
    for (int k = 0; k < 4; ++k) {
        p.band[k] = k;
        p.q[k] = q[k];
    }
    if (ok && spp == 4) {
        unsigned seen = 0u;
        for (int k = 0; band && k < 4; ++k)
            if (band[k] >= 0 && band[k] <= 3) {
                seen |= 1u << band[k];
                p.band[k] = band[k];
            }
        ok = seen == 15u;
    }
    if (!ok) return oip_fail(ctx, OIP_E_INVALID, "oip_mask_cells_u16: bad argument");
    const int gw = (w + cell - 1) / cell;
    const long nby = (rows + cell - 1) / cell;
    if (gw == 0 || nby == 0) return OIP_OK;
    const bool vec = pitch % 8 == 0 && ((uintptr_t)d_src & 15) == 0;
    OipProfScope prof(ctx, vec ? "mask_cells_u16_kernel" : "mask_cells_u16_any_kernel");
    const long lanes = vec ? ((long)w * spp + 7) / 8 : (long)gw;
    const int gx = (int)((lanes + kBlock - 1) / kBlock);
    long gy = (long)ctx->cu_count * kPerCu / gx;
    if (gy < 1) gy = 1;
    if (gy > nby) gy = nby;
    if (gy > 65535) gy = 65535;
    const dim3 grid(gx, (unsigned)gy), wg(kBlock);
    unsigned long long *counts = reinterpret_cast<unsigned long long *>(d_counts);
#define OIP_MASK_LAUNCH(S, Ck) \
    hipLaunchKernelGGL((mask_cells_u16_kernel<S, Ck>), grid, wg, 0, ctx->stream, d_src, pitch, w, rows, nby, p, d_flags, flag_pitch, counts)
    if (vec) {
        if (spp == 4 && cell == 4) OIP_MASK_LAUNCH(4, 4);
        else if (spp == 4 && cell == 8) OIP_MASK_LAUNCH(4, 8);
        else if (spp == 4) OIP_MASK_LAUNCH(4, 16);
        else if (cell == 4) OIP_MASK_LAUNCH(1, 4);
        else if (cell == 8) OIP_MASK_LAUNCH(1, 8);
        else OIP_MASK_LAUNCH(1, 16);
    } else {
        hipLaunchKernelGGL(mask_cells_u16_any_kernel, grid, wg, 0, ctx->stream, d_src, pitch, w, rows, nby, spp, cell, p, d_flags, flag_pitch, counts);
    }
#undef OIP_MASK_LAUNCH
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}

extern "C" int oip_mask_morph_u8(oip_ctx *ctx, uint8_t *d_flags, long flag_pitch, int gw, long gh, int open_radius, int buffer_radius,
                                 uint64_t *d_counts)
{
    OIP_CHECK_CTX(ctx);
    if (!d_flags || gw < 0 || gh < 0 || flag_pitch < gw || open_radius < 0 || open_radius > 32 || buffer_radius < 0 || buffer_radius > 64 ||
        ((uintptr_t)d_counts & 7))
        return oip_fail(ctx, OIP_E_INVALID, "oip_mask_morph_u8: bad argument");
    if (gw == 0 || gh == 0) return OIP_OK;
    const int wpl = (gw + 63) / 64;
    const long words = gh * wpl;
    void *ws = nullptr;
    const int rc = oip_workspace(ctx, (size_t)words * 3 * sizeof(unsigned long long), &ws);
    if (rc != OIP_OK) return rc;
    unsigned long long *A = static_cast<unsigned long long *>(ws), *B = A + words, *Cp = B + words;
    const int gwave = grid_1d(ctx, words * 64), gword = grid_1d(ctx, words);
    const dim3 wg(kBlock);
    {
        OipProfScope prof(ctx, "mask_pack_kernel");
        hipLaunchKernelGGL(mask_pack_kernel, dim3(gwave), wg, 0, ctx->stream, d_flags, flag_pitch, gw, gh, wpl, A);
    }
    {
        OipProfScope prof(ctx, "mask_morph_kernels");
        // E = erosion of X (A -> B -> A), O = dilation of E (A -> B -> Cp), D = dilation of O (Cp -> B -> A)
        hipLaunchKernelGGL(mask_morph_v_kernel<true>, dim3(gword), wg, 0, ctx->stream, A, B, gh, wpl, open_radius);
        hipLaunchKernelGGL(mask_morph_h_kernel<true>, dim3(gword), wg, 0, ctx->stream, B, A, gw, gh, wpl, open_radius);
        hipLaunchKernelGGL(mask_morph_v_kernel<false>, dim3(gword), wg, 0, ctx->stream, A, B, gh, wpl, open_radius);
        hipLaunchKernelGGL(mask_morph_h_kernel<false>, dim3(gword), wg, 0, ctx->stream, B, Cp, gw, gh, wpl, open_radius);
        hipLaunchKernelGGL(mask_morph_v_kernel<false>, dim3(gword), wg, 0, ctx->stream, Cp, B, gh, wpl, buffer_radius);
        hipLaunchKernelGGL(mask_morph_h_kernel<false>, dim3(gword), wg, 0, ctx->stream, B, A, gw, gh, wpl, buffer_radius);
    }
    {
        OipProfScope prof(ctx, "mask_unpack_kernel");
        hipLaunchKernelGGL(mask_unpack_kernel, dim3(gwave), wg, 0, ctx->stream, d_flags, flag_pitch, gw, gh, wpl, Cp, A,
                           reinterpret_cast<unsigned long long *>(d_counts));
    }
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}
