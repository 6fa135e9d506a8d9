// align.hip -- inter-band (PAN<->MSS) bicubic alignment of the 4 MSS bands on gfx950.
//
// Replaces PreProcessor::DoInterBandAlignment, outer (preproc.h:351-425) and inner
// (preproc.h:428-468): per 20000-line section and per band the reference builds two float
// maps from the fitted polynomials, calls cv::remap(INTER_CUBIC, BORDER_CONSTANT), merges
// the four planes with cv::merge and memcpy's the section minus its leading overlap into
// the final 16UC4 image.  Here one kernel does all of it per output pixel:
//   mapX = (float)((cX1*xx + cX0 + xx)/4)                     xx = 4x   (fp64, left to right)
//   mapY = (float)((cY2*xx*xx + cY1*xx + cY0 + yy)/4)         yy = 4y, y section relative
// evaluated in fp64 in registers (never stored), OpenCV's 1/32-px bicubic on each planar
// band, and one 8-byte interleaved store (B0,B1,B2,B3) -- 4 x 2 B read + 8 B written per
// output pixel.  Lines of skipped tail sections are written as zeros (the reference leaves
// them uninitialised, SURVEY App.B-6).
#include "oip_bicubic.h"
#include "oip_geom.h"
#include "oip_internal.h"

#include <climits>
#include <cmath>

namespace {

constexpr int kBlock = 256;

struct AlignRow {
    int valid;      // 0: line of a skipped section -> zeros
    int yrel;       // section-relative line
    int base;       // section's first MSS line relative to d_planes' first line
    int lines;      // section's line count (cv::remap source height)
};

struct AlignCoef {
    double cx[4][2];
    double cy[4][3];
};

__global__ void align_rows_kernel(AlignRow *rows, OipAlignGeom g, long out_row0, long out_rows, long src_row0)
{
    long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= out_rows) return;
    AlignRow a;
    int sec;
    long yrel, off, lines;
    if (oip_align_row(g, out_row0 + r, &sec, &yrel, &off, &lines)) {
        a.valid = 1; a.yrel = (int)yrel; a.base = (int)(off - src_row0); a.lines = (int)lines;
    } else {
        a.valid = 0; a.yrel = 0; a.base = 0; a.lines = 0;
    }
    rows[r] = a;
}

// ---- general path: one lane = one (output column, band), any geometry, every border case ------------------
// For a fixed column the first tap line iy advances by exactly one per output line except where the f32
// rounding of mapY flips (rare) or a section seam restarts the section-relative line, so the window
// normally loads only the newest source line (4 taps per pixel instead of 16).
__device__ __forceinline__ void align_load_row(const uint16_t *__restrict__ pl, long lr, bool yok, int Wb, int cix,
                                               unsigned xmask, float out[4])
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int cj = cix + j;
        cj = cj < 0 ? 0 : (cj > Wb - 1 ? Wb - 1 : cj);
        out[j] = (yok && (xmask & (1u << j))) ? (float)pl[lr * Wb + cj] : 0.f;
    }
}

// the lane's band picks its coefficients from the kernel arguments (selects on scalar registers, no memory)
#define OIP_COEF(arr, b, k) ((b) == 0 ? (arr)[0][k] : ((b) == 1 ? (arr)[1][k] : ((b) == 2 ? (arr)[2][k] : (arr)[3][k])))
struct BandCoef {
    double cx0, cx1, cy0, cy1, cy2;
};
#define OIP_BAND_COEF(bc, co, b)                                                                      \
    BandCoef bc;                                                                                      \
    bc.cx0 = OIP_COEF((co).cx, b, 0); bc.cx1 = OIP_COEF((co).cx, b, 1);                               \
    bc.cy0 = OIP_COEF((co).cy, b, 0); bc.cy1 = OIP_COEF((co).cy, b, 1); bc.cy2 = OIP_COEF((co).cy, b, 2);

// output lines [r0, r1) of column x, band b
__device__ __forceinline__ void align_column(const uint16_t *__restrict__ planes, size_t plane_stride, long src_rows,
                                             uint16_t *__restrict__ dst, const AlignRow *__restrict__ rows, int Wb,
                                             const BandCoef bc, const float *__restrict__ tab1d, int x, int b, long r0, long r1)
{
    const int xx = x * 4;
    const double dxx = (double)xx;
    // column-only part of the maps (preproc.h:447-448), fp64, left to right
    const double cx0 = bc.cx0, cx1 = bc.cx1, cy0 = bc.cy0, cy1 = bc.cy1, cy2 = bc.cy2;
    const double mx = __dadd_rn(__dadd_rn(__dmul_rn(cx1, dxx), cx0), dxx) * 0.25;
    const int sx = oip_cvround((float)mx * 32.0f);
    const int cix = oip_sat_short(sx >> 5) - 1;
    const int fx = sx & 31;
    float wx[4];
    unsigned xmask = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        wx[j] = tab1d[fx * 4 + j];
        const int cj = cix + j;
        if (cj >= 0 && cj < Wb) xmask |= 1u << j;
    }
    const double coly = __dadd_rn(__dadd_rn(__dmul_rn(__dmul_rn(cy2, dxx), dxx), __dmul_rn(cy1, dxx)), cy0);
    const uint16_t *pl = planes + (size_t)b * plane_stride;
    const bool x_out = cix >= Wb || cix + 4 <= 0;
    const bool x_in = (unsigned)cix < (unsigned)(Wb - 3 > 0 ? Wb - 3 : 0);

    float win[4][4];               // [tap row][tap col]
    int cur_iy = INT_MIN, cur_base = INT_MIN;
    for (long r = r0; r < r1; ++r) {
        const AlignRow a = rows[r];
        unsigned res = 0;
        if (a.valid) {
            if (a.base != cur_base) { cur_base = a.base; cur_iy = INT_MIN; }       // new section: window stale
            const double yy = (double)((long)a.yrel * 4);
            const double my = __dadd_rn(coly, yy) * 0.25;
            const int sy = oip_cvround((float)my * 32.0f);
            const int iy = oip_sat_short(sy >> 5) - 1, fy = sy & 31;
            if (iy == cur_iy + 1 && cur_iy != INT_MIN) {
#pragma unroll
                for (int t = 0; t < 3; ++t) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) win[t][j] = win[t + 1][j];
                }
                const int rr = iy + 3;
                const long lr = (long)a.base + rr;
                align_load_row(pl, lr, rr >= 0 && rr < a.lines && lr >= 0 && lr < src_rows, Wb, cix, xmask, win[3]);
            } else if (iy != cur_iy) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int rr = iy + t;
                    const long lr = (long)a.base + rr;
                    align_load_row(pl, lr, rr >= 0 && rr < a.lines && lr >= 0 && lr < src_rows, Wb, cix, xmask, win[t]);
                }
            }
            cur_iy = iy;
            float sum;
            if (x_out || iy >= a.lines || iy + 4 <= 0) {
                sum = 0.f;
            } else {
                float wy[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) wy[j] = tab1d[fy * 4 + j];
                if (x_in && (unsigned)iy < (unsigned)(a.lines - 3 > 0 ? a.lines - 3 : 0)) {
                    sum = oip_bicubic_interior(win, wx, wy);
                } else {
                    unsigned ymask = 0;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int rr = iy + t;
                        const long lr = (long)a.base + rr;
                        if (rr >= 0 && rr < a.lines && lr >= 0 && lr < src_rows) ymask |= 1u << t;
                    }
                    sum = oip_bicubic_border(win, wx, wy, xmask, ymask);
                }
            }
            res = oip_sat_u16(sum);
        }
        dst[((size_t)r * Wb + x) * 4 + b] = (uint16_t)res;
    }
}

__global__ __launch_bounds__(kBlock) void align_mss_kernel(const uint16_t *__restrict__ planes, size_t plane_stride,
                                                           long src_rows, uint16_t *__restrict__ dst,
                                                           const AlignRow *__restrict__ rows, int Wb, long out_rows,
                                                           AlignCoef co, const float *__restrict__ tab1d,
                                                           int rows_per_block)
{
    // lane = 16 * band + pixel: the 2-byte taps of a 16-lane group are 32 contiguous bytes of one plane
    const int gid = blockIdx.x * kBlock + threadIdx.x;
    const int x = (gid >> 6) * 16 + (gid & 15), b = (gid >> 4) & 3;
    if (x >= Wb) return;
    const long r0 = (long)blockIdx.y * rows_per_block;
    long r1 = r0 + rows_per_block;
    if (r1 > out_rows) r1 = out_rows;
    OIP_BAND_COEF(bc, co, b)
    align_column(planes, plane_stride, src_rows, dst, rows, Wb, bc, tab1d, x, b, r0, r1);
}

// ---- fast path: one lane = 8 consecutive output pixels of ONE band ------------------------------------------
// Lane l of a wave: band l >> 4, pixel group l & 15 (8 pixels each): the 16 lanes of a band read 16 x 16
// contiguous bytes of its plane per source line (6 dwords per lane from a 4-byte aligned address, 11
// samples: the taps of its 8 pixels), and the wave covers 128 output pixels x 4 bands.  What makes 8
// pixels share their work:
//   * x: the group is REGULAR when its 8 map values land on consecutive source columns with one x phase
//     (checked per lane at start, in the reference's fp64 order) -- then the 16 weights wy*wx are shared;
//   * y: mapY = (colY(x) + 4 y) / 4.  Per line the exact (first tap line, phase) pair is evaluated for the
//     group's first and last pixel only: colY is checked to be monotonic across the 8 pixels (once per
//     lane), every later operation is monotonic, so equal end points mean equal values in between.
// Lines where a group's pixels disagree, lines whose window touches a border of the section buffer or of
// the image, and irregular groups are not computed here: the lane appends (group, band, line range) to a
// list and a second launch runs the general code on exactly those.  Arithmetic per pixel is
// oip_bicubic_interior's (w = wy*wx rounded once, row sums left to right, rows added in order).
// The four bands of a pixel sit in four different lanes; two permlane swaps (a 4x4 transpose over the
// 16-lane rows) and one bpermute per dword bring them together so that every lane stores 16 contiguous
// bytes = 2 interleaved 16UC4 pixels, the wave 1 KiB.
struct AlignFix {
    int group, band, ra, rb;
};

// Line load (six dwords per lane and source line, unclamped: ix0 + 11 < Wb below), tap window, weights and sums are
// oip_bicubic.h's oip_load_raw6 and OipTaps8<false>, shared with remap.hip's fast kernels; the map evaluation, the fix-up list
// and the transposing store are this kernel's own.
__global__ __launch_bounds__(kBlock, 3) void align_mss8_kernel(const uint16_t *__restrict__ planes, size_t plane_stride,
                                                               long src_rows, uint16_t *__restrict__ dst,
                                                               const AlignRow *__restrict__ rows, int Wb, long out_rows,
                                                               AlignCoef co, const float *__restrict__ tab1d,
                                                               int rows_per_block, AlignFix *__restrict__ fix,
                                                               int *__restrict__ fix_count, int fix_cap)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = lane >> 4;
    const int G = ((int)blockIdx.x * (kBlock / 64) + wave) * 16 + (lane & 15);
    const int x0 = G * 8;
    const long r0 = (long)blockIdx.y * rows_per_block;
    long r1 = r0 + rows_per_block;
    if (r1 > out_rows) r1 = out_rows;
    const bool live = x0 < Wb;                    // lanes past the line end still take part in the exchanges
    const uint16_t *pl = planes + (size_t)b * plane_stride;

    // x maps of the 8 pixels (preproc.h:447), fp64 left to right, and the column part of the y maps
    OIP_BAND_COEF(bc, co, b)
    const double cx0 = bc.cx0, cx1 = bc.cx1, cy0 = bc.cy0, cy1 = bc.cy1, cy2 = bc.cy2;
    int ix0 = 0, fx0 = 0;
    bool xreg = live && x0 + 7 < Wb;
    double c4_first = 0.0, c4_last = 0.0;
    {
        double prev = 0.0;
        int dir = 0;            // +1 non-decreasing so far, -1 non-increasing, 0 flat
        bool mono = true;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const double dxx = (double)((x0 + j) * 4);
            const double mx = __dadd_rn(__dadd_rn(__dmul_rn(cx1, dxx), cx0), dxx) * 0.25;
            const int sx = oip_cvround((float)mx * 32.0f);
            const int ix = oip_sat_short(sx >> 5) - 1, fx = sx & 31;
            if (j == 0) { ix0 = ix; fx0 = fx; }
            else xreg = xreg && ix == ix0 + j && fx == fx0;
            // (colY + yy) / 4 == colY / 4 + y exactly (scaling by 4 commutes with rounding)
            const double c4 = __dadd_rn(__dadd_rn(__dmul_rn(__dmul_rn(cy2, dxx), dxx), __dmul_rn(cy1, dxx)), cy0) * 0.25;
            if (j == 0) c4_first = c4;
            else {
                if (c4 > prev) { mono = mono && dir >= 0; dir = 1; }
                else if (c4 < prev) { mono = mono && dir <= 0; dir = -1; }
            }
            prev = c4;
            if (j == 7) c4_last = c4;
        }
        xreg = xreg && mono && ix0 >= 0 && ix0 + 11 < Wb;      // + 11: the sixth dword of an even first column stays in the line
    }
    const int c0 = xreg ? ix0 : 0;
    const uint32_t *lane_base = reinterpret_cast<const uint32_t *>(pl) + (c0 >> 1);
    const int half_pitch = Wb >> 1;
    float wx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wx[j] = tab1d[fx0 * 4 + j];

    OipTaps8<false> taps;
    uint32_t nraw[6] = {0u, 0u, 0u, 0u, 0u, 0u};
    long nline = -1;                 // global plane line whose raw dwords are in nraw (-1: none)
    int cur_iy = INT_MIN, cur_base = INT_MIN, cur_fy = -1;
    int bad_lo = INT_MAX, bad_hi = INT_MIN;
    if (live && !xreg) { bad_lo = (int)r0; bad_hi = (int)r1; }

    for (long rb = r0; rb < r1; rb += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long r = rb + k;
            if (r >= r1) break;
            const AlignRow a = rows[oip_uniform(r)];
            uint4 px = make_uint4(0u, 0u, 0u, 0u);            // the band's 8 pixels of this line, 16 bytes in pixel order
            if (a.valid) {                                    // uniform over the wave
                const double yrel = (double)a.yrel;
                const int sy0 = oip_cvround((float)__dadd_rn(c4_first, yrel) * 32.0f);
                const int sy7 = oip_cvround((float)__dadd_rn(c4_last, yrel) * 32.0f);
                const int iy = oip_sat_short(sy0 >> 5) - 1, fy = sy0 & 31;
                const long l0 = (long)a.base + iy;
                const bool ok = xreg && sy0 == sy7 && iy >= 0 && iy + 3 < a.lines && l0 >= 0 && l0 + 3 < src_rows;
                if (ok) {
                    const bool slide = a.base == cur_base && iy == cur_iy + 1;
                    if (slide) {
                        // rotate: this unrolled step's slot order is (k + t) & 3
                        if (nline == l0 + 3) taps.expand(nraw, c0, (k + 3) & 3);
                        else { uint32_t w[6]; oip_load_raw6(lane_base, l0 + 3, half_pitch, w); taps.expand(w, c0, (k + 3) & 3); }
                    } else {
#pragma unroll
                        for (int t = 0; t < 4; ++t) { uint32_t w[6]; oip_load_raw6(lane_base, l0 + t, half_pitch, w); taps.expand(w, c0, (k + t) & 3); }
                    }
                    cur_base = a.base; cur_iy = iy;
                    // next line's newest source line, in flight under this line's sums
                    nline = l0 + 4;
                    if (nline < src_rows) oip_load_raw6(lane_base, nline, half_pitch, nraw); else nline = -1;
                    if (fy != cur_fy) {
                        cur_fy = fy;
                        taps.weights(tab1d, fy, wx);
                    }
                    px = taps.sums(k);
                } else {
                    // the slot rotation of the unrolled loop assumes one slide per step: a skipped line breaks it
                    cur_iy = INT_MIN;
                    if (live) { bad_lo = bad_lo < (int)r ? bad_lo : (int)r; bad_hi = bad_hi > (int)r + 1 ? bad_hi : (int)r + 1; }
                }
            } else {
                cur_iy = INT_MIN;
            }
            // d[j] = this band's pixels 2j, 2j+1; transpose over the four 16-lane rows, then lane (row r, group g)
            // holds pixels 2r, 2r+1 of group g for all four bands
            uint32_t d0 = px.x, d1 = px.y, d2 = px.z, d3 = px.w;
            {
                auto s02 = __builtin_amdgcn_permlane32_swap(d0, d2, false, false);
                auto s13 = __builtin_amdgcn_permlane32_swap(d1, d3, false, false);
                auto t01 = __builtin_amdgcn_permlane16_swap(s02[0], s13[0], false, false);
                auto t23 = __builtin_amdgcn_permlane16_swap(s02[1], s13[1], false, false);
                d0 = t01[0]; d1 = t01[1]; d2 = t23[0]; d3 = t23[1];       // band 0..3 of this lane's pixel pair
            }
            // lane 4g + r takes over from lane (r, g) = 16 r + g: consecutive lanes then store consecutive 16 bytes
            const int src_lane = ((lane & 3) << 4) | (lane >> 2);
            d0 = __builtin_amdgcn_ds_bpermute(src_lane << 2, d0);
            d1 = __builtin_amdgcn_ds_bpermute(src_lane << 2, d1);
            d2 = __builtin_amdgcn_ds_bpermute(src_lane << 2, d2);
            d3 = __builtin_amdgcn_ds_bpermute(src_lane << 2, d3);
            // pixel pair p = (lane & 3) of group (lane >> 2): pixels xs, xs + 1
            const int gw = ((int)blockIdx.x * (kBlock / 64) + wave) * 16 + (lane >> 2);
            const int xs = gw * 8 + 2 * (lane & 3);
            if (xs + 1 < Wb) {
                uint4 o;
                o.x = (d0 & 0xffffu) | (d1 << 16);            // pixel xs: bands 0, 1
                o.y = (d2 & 0xffffu) | (d3 << 16);            //           bands 2, 3
                o.z = (d0 >> 16) | (d1 & 0xffff0000u);        // pixel xs + 1
                o.w = (d2 >> 16) | (d3 & 0xffff0000u);
                *reinterpret_cast<uint4 *>(dst + ((size_t)r * Wb + xs) * 4) = o;
            }
        }
    }
    if (bad_hi > bad_lo) {
        const int i = atomicAdd(fix_count, 1);
        if (i < fix_cap) fix[i] = AlignFix{G, b, bad_lo, bad_hi};
    }
}

// second launch: the listed (group, band, line range) entries through the general code; 64 lanes = 8 pixels x
// 8 line sub-ranges
__global__ __launch_bounds__(64) void align_fix_kernel(const uint16_t *__restrict__ planes, size_t plane_stride, long src_rows,
                                                       uint16_t *__restrict__ dst, const AlignRow *__restrict__ rows, int Wb,
                                                       AlignCoef co, const float *__restrict__ tab1d,
                                                       const AlignFix *__restrict__ fix, const int *__restrict__ fix_count, int fix_cap)
{
    int n = *fix_count;
    if (n > fix_cap) n = fix_cap;
    for (int e = blockIdx.x; e < n; e += gridDim.x) {
        const AlignFix f = fix[e];
        const int x = f.group * 8 + (threadIdx.x & 7);
        if (x >= Wb) continue;
        const int sub = threadIdx.x >> 3;
        const int per = (f.rb - f.ra + 7) / 8;
        const long a = f.ra + (long)sub * per;
        long bnd = a + per;
        if (bnd > f.rb) bnd = f.rb;
        const int fb = f.band;
        OIP_BAND_COEF(bc, co, fb)
        if (a < bnd) align_column(planes, plane_stride, src_rows, dst, rows, Wb, bc, tab1d, x, fb, a, bnd);
    }
}

// host mirror of the kernel's first-tap line for one band/column/line (range queries)
inline int host_iy(const double *cy3, int x, long yrel)
{
    double dxx = (double)(x * 4);
    double coly = ((cy3[2] * dxx) * dxx + cy3[1] * dxx) + cy3[0];
    double my = (coly + (double)(yrel * 4)) * 0.25;
    int sy = (int)rintf((float)my * 32.0f);
    int iy = sy >> 5;
    iy = iy < -32768 ? -32768 : (iy > 32767 ? 32767 : iy);
    return iy - 1;
}

}  // namespace

// MSS source lines needed by a window of output lines.  mapY is quadratic in the column, so
// its extremes over a line are at the ends or at the vertex; they are evaluated per band and
// widened by one line for the f32 rounding of the map.
extern "C" int oip_align_mss_src_range(long out_row0, long out_rows, long Lm, const double *cy, int Wb,
                                       int lines_per_section, int line_offset, int overlap, int keep_leading,
                                       int min_lines, long *first, long *last)
{
    if (!cy || Wb <= 0 || out_rows < 0 || out_row0 < 0) return OIP_E_INVALID;
    OipAlignGeom g = oip_align_geom(Wb, Lm, lines_per_section, line_offset, overlap, keep_leading, min_lines);
    if (out_row0 + out_rows > g.out_rows) return OIP_E_INVALID;
    long lo = -1, hi = -1;
    // candidate columns: ends and the vertex of each band's parabola
    int cand[4][3];
    for (int b = 0; b < 4; ++b) {
        const double *c = cy + b * 3;
        cand[b][0] = 0;
        cand[b][1] = Wb - 1;
        int xv = 0;
        if (c[2] != 0.0) {
            double v = -c[1] / (2.0 * c[2]) / 4.0;
            xv = v < 0 ? 0 : (v > Wb - 1 ? Wb - 1 : (int)v);
        }
        cand[b][2] = xv;
    }
    auto accum = [&](long orow) {
        int sec;
        long yrel, off, lines;
        if (!oip_align_row(g, orow, &sec, &yrel, &off, &lines)) return;
        for (int b = 0; b < 4; ++b)
            for (int k = 0; k < 3; ++k)
                for (int dxc = -1; dxc <= 1; ++dxc) {
                    int x = cand[b][k] + dxc;
                    if (x < 0 || x >= Wb) continue;
                    int iy = host_iy(cy + b * 3, x, yrel);
                    long r_lo = iy - 1, r_hi = iy + 4 + 1;          // widened by one line each side
                    if (r_lo < 0) r_lo = 0;
                    if (r_hi > lines) r_hi = lines;
                    if (r_lo >= r_hi) continue;
                    if (lo < 0 || off + r_lo < lo) lo = off + r_lo;
                    if (off + r_hi > hi) hi = off + r_hi;
                }
    };
    // tap lines are monotone in the output line inside one section: end points suffice
    long a = out_row0, bnd = out_row0 + out_rows;
    long r = a;
    while (r < bnd) {
        int sec;
        long yrel, off, lines;
        if (!oip_align_row(g, r, &sec, &yrel, &off, &lines)) break;   // zero tail from here on
        long sec_end = r + (lines - yrel);                             // first output line of the next section
        if (g.keep_leading && sec == 0 && r < g.overlap) sec_end = g.overlap + (lines - g.overlap);
        long e = sec_end < bnd ? sec_end : bnd;
        accum(r);
        accum(e - 1);
        r = e;
    }
    if (lo < 0) lo = hi = 0;
    if (first) *first = lo;
    if (last) *last = hi;
    return OIP_OK;
}

extern "C" int oip_align_mss_bicubic_u16x4(oip_ctx *ctx, const uint16_t *d_planes, size_t plane_stride, long src_row0,
                                           long src_rows, uint16_t *d_dst, long out_row0, long out_rows, int Wb,
                                           long Lm, const double *cx, const double *cy, int lines_per_section,
                                           int line_offset, int overlap, int keep_leading, int min_lines,
                                           long *rows_valid)
{
    OIP_CHECK_CTX(ctx);
    if (!d_planes || !d_dst || !cx || !cy || Wb <= 0 || Lm <= 0)
        return oip_fail(ctx, OIP_E_INVALID, "oip_align_mss_bicubic_u16x4: bad argument");
    // preproc.h:355-367
    if (overlap > OIP_IBPA_MAX_LINEOVERLAP)
        return oip_fail(ctx, OIP_E_INVALID, "Overlap value %d exceeds maximum allowed value(%d)", overlap, OIP_IBPA_MAX_LINEOVERLAP);
    if (lines_per_section > 32767) return oip_fail(ctx, OIP_E_INVALID, "Row number exceeds OpenCV allowed value");
    if (lines_per_section < overlap * 2 || overlap < 0 || lines_per_section <= overlap)
        return oip_fail(ctx, OIP_E_INVALID, "Lines per section too small or section overlapped lines too large");
    if (Lm - line_offset < min_lines || line_offset < 0)
        return oip_fail(ctx, OIP_E_INVALID, "Too few image lines left to process");
    if (Wb > 32767) return oip_fail(ctx, OIP_E_INVALID, "cv::remap cannot address more than 32767 columns");
    for (int i = 0; i < 8; ++i) if (!(cx[i] == cx[i])) return oip_fail(ctx, OIP_E_INVALID, "NaN polynomial coefficient");
    for (int i = 0; i < 12; ++i) if (!(cy[i] == cy[i])) return oip_fail(ctx, OIP_E_INVALID, "NaN polynomial coefficient");
    OipAlignGeom g = oip_align_geom(Wb, Lm, lines_per_section, line_offset, overlap, keep_leading, min_lines);
    if (rows_valid) *rows_valid = g.rows_valid;
    if (out_row0 < 0 || out_rows < 0 || out_row0 + out_rows > g.out_rows || src_row0 < 0 || src_rows < 0 ||
        src_row0 + src_rows > Lm)
        return oip_fail(ctx, OIP_E_INVALID, "oip_align_mss_bicubic_u16x4: row window outside the raster");
    if (plane_stride < (size_t)src_rows * Wb) return oip_fail(ctx, OIP_E_INVALID, "plane_stride too small");
    if (out_rows == 0) return OIP_OK;
    if (src_row0 != 0 || src_rows != Lm) {
        long first = 0, last = 0;
        int rc = oip_align_mss_src_range(out_row0, out_rows, Lm, cy, Wb, lines_per_section, line_offset, overlap,
                                         keep_leading, min_lines, &first, &last);
        if (rc) return oip_fail(ctx, rc, "oip_align_mss_bicubic_u16x4: bad row window");
        if (first < src_row0 || last > src_row0 + src_rows)
            return oip_fail(ctx, OIP_E_INVALID,
                            "oip_align_mss_bicubic_u16x4: source window [%ld,%ld) lacks halo lines, need [%ld,%ld)",
                            src_row0, src_row0 + src_rows, first, last);
    }
    // fast path: 8 pixels of one band per lane; needs even widths (dword-aligned sample pairs) and 16-byte aligned
    // output lines
    const bool fast = Wb % 2 == 0 && Wb >= 16 && (((uintptr_t)d_dst) & 15) == 0 &&
                      (((uintptr_t)d_planes) & 3) == 0 && (plane_stride % 2) == 0 && src_rows * (long)Wb >= 16;
    const int groups = (Wb + 7) / 8;
    int gx = (groups + 63) / 64;                                  // 4 waves x 16 groups per workgroup
    long want = (long)ctx->cu_count * 16 / gx;                    // 3..48 per CU: flat within 3 % (r04_grid_sweep.txt)
    if (want < 1) want = 1;
    long rpb = (out_rows + want - 1) / want;
    if (rpb < 32) rpb = 32;
    rpb = (rpb + 3) / 4 * 4;
    long gy = (out_rows + rpb - 1) / rpb;
    if (gy > 65535) { gy = 65535; rpb = ((out_rows + gy - 1) / gy + 3) / 4 * 4; gy = (out_rows + rpb - 1) / rpb; }
    const size_t rows_bytes = ((size_t)out_rows * sizeof(AlignRow) + 255) / 256 * 256;
    const long fix_cap = (long)groups * OIP_MSS_BANDS * gy;       // one entry per (group, band, line block) at most
    void *ws = nullptr;
    int rc = oip_workspace(ctx, rows_bytes + 256 + sizeof(AlignFix) * (size_t)fix_cap + 512, &ws);
    if (rc) return rc;
    AlignRow *rows = reinterpret_cast<AlignRow *>(ws);
    int *d_fix_count = reinterpret_cast<int *>((char *)ws + rows_bytes);
    AlignFix *d_fix = reinterpret_cast<AlignFix *>((char *)ws + rows_bytes + 256);
    {
        OipProfScope prof(ctx, "align_rows_kernel");
        int blocks = (int)((out_rows + 255) / 256);
        hipLaunchKernelGGL(align_rows_kernel, dim3(blocks), dim3(256), 0, ctx->stream, rows, g, out_row0, out_rows, src_row0);
    }
    AlignCoef co;
    memcpy(co.cx, cx, sizeof co.cx);
    memcpy(co.cy, cy, sizeof co.cy);
    if (fast) {
        ctx->prof_chain = nullptr;
        OIP_HIP(ctx, hipMemsetAsync(d_fix_count, 0, sizeof(int), ctx->stream));
        {
            OipProfScope prof(ctx, "align_mss_kernel");
            hipLaunchKernelGGL(align_mss8_kernel, dim3(gx, (unsigned)gy), dim3(kBlock), 0, ctx->stream, d_planes, plane_stride,
                               src_rows, d_dst, rows, Wb, out_rows, co, ctx->d_tab1d, (int)rpb, d_fix, d_fix_count, (int)fix_cap);
        }
        {
            OipProfScope prof(ctx, "align_fix_kernel");
            long nb = fix_cap < (long)ctx->cu_count * 64 ? fix_cap : (long)ctx->cu_count * 64;
            if (nb < 1) nb = 1;
            hipLaunchKernelGGL(align_fix_kernel, dim3((unsigned)nb), dim3(64), 0, ctx->stream, d_planes, plane_stride, src_rows,
                               d_dst, rows, Wb, co, ctx->d_tab1d, d_fix, d_fix_count, (int)fix_cap);
        }
    } else {
        OipProfScope prof(ctx, "align_mss_kernel");
        int gxg = (Wb + kBlock / 4 - 1) / (kBlock / 4);          // 16 pixels x 4 bands per wave
        long wantg = (long)ctx->cu_count * 16 / gxg;
        if (wantg < 1) wantg = 1;
        long rpbg = (out_rows + wantg - 1) / wantg;
        if (rpbg < 32) rpbg = 32;
        long gyg = (out_rows + rpbg - 1) / rpbg;
        if (gyg > 65535) { gyg = 65535; rpbg = (out_rows + gyg - 1) / gyg; gyg = (out_rows + rpbg - 1) / rpbg; }
        hipLaunchKernelGGL(align_mss_kernel, dim3(gxg, (unsigned)gyg), dim3(kBlock), 0, ctx->stream, d_planes, plane_stride,
                           src_rows, d_dst, rows, Wb, out_rows, co, ctx->d_tab1d, (int)rpbg);
    }
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}
