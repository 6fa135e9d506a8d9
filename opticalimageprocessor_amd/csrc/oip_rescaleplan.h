// oip_rescaleplan.h -- the host arithmetic of `oip rescale` (include/oip_c.h: oip_rescale_*): the Q14 tap tables of an axis, the
// size of a scaled axis, the source lines a window of output lines needs, the scale parser of the command line, and the plan
// that picks the output tile of rescale.hip so that its source region fits the LDS budget.  Nothing of HIP in here: host.cpp
// exports the C entries, rescale.hip runs the plan, and tests/cpp/rescale_test.cpp runs all of it on the CPU under sanitizers.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "oip_c.h"

#ifdef __HIP__                             // (a .hip translation unit; host.cpp and the CPU test take the plain form)
#define OIP_RESCALE_FN __host__ __device__ inline
#else
#define OIP_RESCALE_FN inline
#endif

constexpr int kOipRescaleMaxK = 24;          // taps of a row at the largest reduction, 1/4 with Lanczos-3
constexpr int kOipRescaleOne = 16384;        // Q14
constexpr int kOipRescaleBlock = 256;        // lanes of a workgroup
constexpr int kOipRescaleLds = 40960;        // bytes of LDS a workgroup may take: four workgroups on a CU of 160 KiB
constexpr int kOipRescaleTileH = 32;         // output lines of a tile at most
constexpr int kOipRescaleTileWs = 128;       // output samples across a tile at most (a multiple of 8)
constexpr int kOipRescaleLines = 4;          // output lines a lane of the horizontal pass carries per tap it reads

inline long oip_rescale_floor_div(long a, long b) { return a / b - ((a % b != 0) && ((a < 0) != (b < 0))); }

// the support a of a kernel kind, 0 for an unknown one
inline int oip_rescale_support(int kind) { return kind == OIP_RESCALE_LANCZOS ? 3 : kind == OIP_RESCALE_CUBIC ? 2 : kind == OIP_RESCALE_LINEAR ? 1 : 0; }

// h(x) of the three kinds
inline double oip_rescale_kernel(int kind, double x)
{
    const double ax = std::fabs(x);
    if (kind == OIP_RESCALE_LANCZOS) {
        if (ax >= 3.0) return 0.0;
        if (ax == 0.0) return 1.0;
        const double px = 3.14159265358979323846 * ax, p3 = px / 3.0;
        return (std::sin(px) / px) * (std::sin(p3) / p3);
    }
    if (kind == OIP_RESCALE_CUBIC) {
        const double A = -0.5;
        if (ax <= 1.0) return ((A + 2.0) * ax - (A + 3.0)) * ax * ax + 1.0;
        if (ax < 2.0) return ((A * ax - 5.0 * A) * ax + 8.0 * A) * ax - 4.0 * A;
        return 0.0;
    }
    return ax < 1.0 ? 1.0 - ax : 0.0;
}

// why an axis n_in -> n_out is refused, or NULL
inline const char *oip_rescale_axis_refusal(long n_in, long n_out)
{
    if (n_in < 1 || n_out < 1) return "an empty axis";
    if (n_in >= (1L << 31) || n_out >= (1L << 31)) return "an axis of 2^31 samples or more";
    if (n_in > 4 * n_out) return "a reduction below 1/4 (more than 24 taps a sample): reduce by 2 with `oip overviews` first";
    if (n_out > 16 * n_in) return "an enlargement beyond 16";
    return nullptr;
}

// K of include/oip_c.h: 2 ceil(a max(n_in, n_out) / n_out)
inline int oip_rescale_k(int kind, long n_in, long n_out)
{
    const long mx = n_in > n_out ? n_in : n_out, a = oip_rescale_support(kind);
    return (int)(2 * ((a * mx + n_out - 1) / n_out));
}

// first[o] for a row of K taps
inline long oip_rescale_first(long n_in, long n_out, int K, long o) { return oip_rescale_floor_div((2 * o + 1) * n_in - n_out, 2 * n_out) - K / 2 + 1; }

// the nearest source sample of output sample o: floor((2 o + 1) n_in / (2 n_out))
OIP_RESCALE_FN long oip_rescale_nearest(long n_in, long n_out, long o) { return (2 * o + 1) * n_in / (2 * n_out); }

inline int oip_rescale_fail(char *err, int errlen, int code, const char *what, const char *why)
{
    if (err && errlen > 0) snprintf(err, errlen, "%s: %s", what, why);
    return code;
}

// the table of an axis, steps 1..6 of include/oip_c.h
inline int oip_rescale_taps_impl(int kind, long n_in, long n_out, int *first, int16_t *taps, size_t cap, int *K, char *err, int errlen)
{
    const char *fn = "oip_rescale_taps";
    if (!oip_rescale_support(kind)) return oip_rescale_fail(err, errlen, OIP_E_INVALID, fn, "kernel 0 (lanczos), 1 (cubic) or 2 (linear) expected");
    if (const char *why = oip_rescale_axis_refusal(n_in, n_out)) return oip_rescale_fail(err, errlen, OIP_E_INVALID, fn, why);
    const int k = oip_rescale_k(kind, n_in, n_out);
    if (K) *K = k;
    if (!first && !taps) return OIP_OK;                          // the question for K alone
    if (!first || !taps || cap < (size_t)n_out * k) return oip_rescale_fail(err, errlen, OIP_E_INVALID, fn, "first and taps with room for n_out K values expected");
    const long mx = n_in > n_out ? n_in : n_out, den = 2 * n_out;
    for (long o = 0; o < n_out; ++o) {
        const long num = (2 * o + 1) * n_in - n_out;
        const long f = oip_rescale_floor_div(num, den) - k / 2 + 1;
        double w[kOipRescaleMaxK], sum = 0.0;
        for (int j = 0; j < k; ++j) {
            w[j] = oip_rescale_kernel(kind, (double)(den * (f + j) - num) / (double)(2 * mx));
            sum += w[j];
        }
        int t[kOipRescaleMaxK], total = 0, big = 0;
        for (int j = 0; j < k; ++j) {
            t[j] = (int)std::floor(w[j] / sum * 16384.0 + 0.5);
            total += t[j];
            if (t[j] > t[big]) big = j;
        }
        t[big] += kOipRescaleOne - total;
        int mag = 0;
        for (int j = 0; j < k; ++j) mag += t[j] < 0 ? -t[j] : t[j];
        if (mag > 32767) return oip_rescale_fail(err, errlen, OIP_E_RUNTIME, fn, "a row of taps whose magnitudes sum to more than 32767");
        first[o] = (int)f;
        for (int j = 0; j < k; ++j) taps[(size_t)o * k + j] = (int16_t)t[j];
    }
    return OIP_OK;
}

// n_out = floor(n_in p / q + 1/2)
inline int oip_rescale_size_impl(long n_in, long p, long q, long *n_out)
{
    if (n_in < 1 || p < 1 || q < 1 || !n_out) return OIP_E_INVALID;
    const unsigned __int128 v = ((unsigned __int128)2 * (unsigned long)n_in * (unsigned long)p + (unsigned long)q) / ((unsigned __int128)2 * (unsigned long)q);
    if (v >= ((unsigned __int128)1 << 31)) return OIP_E_INVALID;
    *n_out = (long)v;
    return OIP_OK;
}

// the source samples [*src0, *src0 + *srcs) that output samples [out0, out0 + outs) of an axis read: the clamped index range
inline int oip_rescale_src_range_impl(long n_in, long n_out, int K, long out0, long outs, long *src0, long *srcs)
{
    if (n_in < 1 || n_out < 1 || n_in >= (1L << 31) || n_out >= (1L << 31) || K < 2 || K > kOipRescaleMaxK || (K & 1) || out0 < 0 || outs < 0 ||
        outs > n_out || out0 > n_out - outs || !src0 || !srcs)
        return OIP_E_INVALID;
    if (outs == 0) {
        *src0 = 0, *srcs = 0;
        return OIP_OK;
    }
    long lo = oip_rescale_first(n_in, n_out, K, out0), hi = oip_rescale_first(n_in, n_out, K, out0 + outs - 1) + K - 1;
    lo = lo < 0 ? 0 : (lo > n_in - 1 ? n_in - 1 : lo);
    hi = hi < 0 ? 0 : (hi > n_in - 1 ? n_in - 1 : hi);
    *src0 = lo, *srcs = hi - lo + 1;
    return OIP_OK;
}

// A scale of the command line as a rational p / q in lowest terms: a decimal ("0.8" is 8/10, "2", "1.25") or a fraction
// ("2/3").  At most 9 digits a number; zero, signs, exponents and blanks are refused.  Never a double.
inline bool oip_rescale_parse_scale(const char *s, long *p, long *q)
{
    auto digits = [](const char *&c, long *v, int *n) {
        *v = 0, *n = 0;
        while (*c >= '0' && *c <= '9') {
            if (++*n > 9) return false;
            *v = *v * 10 + (*c++ - '0');
        }
        return true;
    };
    if (!s || !p || !q) return false;
    long a = 0, b = 1;
    int n = 0, m = 0;
    const char *c = s;
    if (!digits(c, &a, &n)) return false;
    if (*c == '/') {
        ++c;
        if (n == 0 || !digits(c, &b, &m) || m == 0) return false;
    } else if (*c == '.') {
        ++c;
        long f = 0;
        if (!digits(c, &f, &m) || n + m == 0 || n + m > 9) return false;
        for (int i = 0; i < m; ++i) a *= 10, b *= 10;
        a += f;
    } else if (n == 0) {
        return false;
    }
    if (*c || a < 1 || b < 1) return false;
    long x = a, y = b;
    while (y) { const long r = x % y; x = y; y = r; }
    *p = a / x, *q = b / x;
    return true;
}

// ---- the tile of rescale.hip -------------------------------------------------------------------------------------------------
// A workgroup owns th output lines x tw output pixels.  Its source region is sh lines x sw pixels: first[] moves by at most
// floor((T - 1) n_in / n_out) + 1 over T outputs, and the last row of taps reaches K - 1 further.  In LDS, in this order: the
// region (sh lines of `pitch` samples: sw pixels and up to 7 samples of alignment slack, a multiple of 8), the intermediate (th
// lines of pitch), the output tile (th lines of tw spp samples), the taps of the tile's columns (Kx x tw, transposed), their
// first[] (tw ints) and, with the no-data rule, a flag byte per intermediate sample.
struct OipRescaleTile {
    int th, tw;                              // output lines and pixels of a tile
    int sh, sw;                              // source lines and pixels of its region
    int pitch;                               // samples of an LDS line of the region and of the intermediate
    int lds;                                 // bytes
};

inline int oip_rescale_extent(int T, long n_in, long n_out, int K) { return (int)((long)(T - 1) * n_in / n_out) + 1 + K; }

inline int oip_rescale_tile_lds(const OipRescaleTile &t, int spp, int Kx, bool nodata)
{
    return 2 * (t.sh * t.pitch + t.th * t.pitch + t.th * t.tw * spp + Kx * t.tw) + 4 * t.tw + (nodata ? t.th * t.pitch : 0);
}

// the largest tile, from 32 lines x 128 samples down, whose LDS image fits kOipRescaleLds: the side with the larger source
// extent is halved first; 4 lines x 8 samples always fit (37 x 53 source pixels at 1/4 and 24 taps)
inline OipRescaleTile oip_rescale_tile(long W, long Wo, long L, long Lo, int spp, int Kx, int Ky, bool nodata)
{
    OipRescaleTile t = {};
    t.th = kOipRescaleTileH;
    t.tw = kOipRescaleTileWs / spp;
    const int min_tw = 8 / spp;
    for (;;) {
        t.sh = oip_rescale_extent(t.th, L, Lo, Ky);
        t.sw = oip_rescale_extent(t.tw, W, Wo, Kx);
        t.pitch = (t.sw * spp + 7 + 7) / 8 * 8;
        t.lds = oip_rescale_tile_lds(t, spp, Kx, nodata);
        if (t.lds <= kOipRescaleLds) return t;
        if (t.th > kOipRescaleLines && (t.sh >= t.sw || t.tw <= min_tw)) t.th /= 2;
        else if (t.tw > min_tw) t.tw /= 2;
        else return t;                       // (not reached for K <= 24 and ratios >= 1/4)
    }
}
