// oip_fft.h -- internal interface of the 2-D FFT engine (fft.hip) used by phasecorr.hip
#pragma once

#include <hip/hip_runtime.h>
#include <cstring>

#include <functional>
#include <vector>

#include "oip_fftplan.h"

struct oip_ctx;

// Arg-max of a correlation surface without a reduction pass: every workgroup of the last inverse pass
// folds its tile maximum into one of kPeakSlots 64-bit slots per surface with atomicMax.  A slot packs
// (order-preserving bits of the f32 value) << 32 | (0xFFFFFFFF - key), key = row-major index in the
// fftShift-ed image (< 2^32), so the largest value wins and, among equal values, the smallest key -- the
// first maximum in minMaxLoc's scan order.  0 = empty (NaN never enters).  peak_window_kernel (phasecorr.hip)
// reduces the slots and zeroes them for the next surface.  (kPeakSlots: oip_fftplan.h)
__host__ __device__ inline unsigned long long oip_peak_pack(float v, long key)
{
    if (v != v) return 0ull;                                   // NaN
    if (v == 0.f) v = 0.f;                                     // -0 == +0 for minMaxLoc
    unsigned u;
    memcpy(&u, &v, 4);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)key);
}
__host__ __device__ inline long oip_peak_key(unsigned long long packed, long none)
{
    return packed == 0ull ? none : (long)(0xFFFFFFFFu - (unsigned)(packed & 0xFFFFFFFFull));
}

// What a pass reads instead of / writes besides the complex array (fusions)
struct OipFftIo {
    int load_kind;      // 0: the complex array; 1: pack two real f32 images (zero padded)
    const float *re;    // f32 image, pitch == cols ...
    const float *im;    // ... may be null
    const uint16_t *re16;   // ... or a u16 raster window (pointer at its first pixel, own pitch)
    const uint16_t *im16;
    long pitch_re16, pitch_im16;
    // ... or an image that is only vertically up-sampled so far: V is rows x v_cols f32 (pitch ==
    // v_cols) and the loader applies the horizontal four cubic taps
    // value(y, x) = sum_j alpha[x][j] * V[y][clamp(xofs[x] - 1 + j)]
    const float *re_v;
    const float *im_v;
    int v_cols;
    const int *xofs;
    const float *alpha; // [cols][4]
    int x4;             // exact x4 geometry (host-verified): xofs[x] == (x - 2) >> 2, no table look-up needed
    int rows, cols;     // extent of the real images
    int store_kind;     // 0: the complex array; 1: peak partials only (nothing stored)
    unsigned long long *slots;  // store_kind 1: [2][kPeakSlots] arg-max slots (real part, imaginary part)
};

// OipFftPass and the host part of a plan (M, N, P, xf, yf, passes, n_y) come from the planner's header
struct OipFft2dPlan : OipFftHostPlan {
    const int *d_ypos;                // device: row position of frequency line ky in the scrambled spectrum, ky in [0, M)
};

int oip_fft2d_plan(oip_ctx *ctx, int M, int N, const OipFft2dPlan **out);
// forward: io (optional) applies to the FIRST pass' load; inverse: to the LAST pass' store
int oip_fft2d_exec(oip_ctx *ctx, const OipFft2dPlan *plan, float2 *data, int inverse, const OipFftIo *io, int rows_done = 0);
int oip_fft_table(oip_ctx *ctx, int T, const float2 **out);     // exp(-2 pi i t / T), t in [0, T)

// Inverse column passes over device-side lists of lane tiles (fft.hip): up to four arrays of one plan per launch, array a
// with count[a] entries tiles[a * stride + j], each a lane tile of the plan's column passes.  Every listed tile is
// transformed in place once per call -- the lists of a call must not name a tile twice.
struct OipColList {
    float2 *data[4];
    const int *count;               // device, [4]
    const int *tiles;               // device, [4][stride]
    int stride;
    int narr;
    unsigned long long *slots;      // peak pass: [4][2][kPeakSlots] arg-max slots, array a at slots + a * 2 * kPeakSlots
};
bool oip_fft_col_list_ok(const OipFft2dPlan *plan, int narr);
int oip_fft_col_list_pass(oip_ctx *ctx, const OipFft2dPlan *plan, int pass, const OipColList &list, bool peak, const char *name);

// position <-> frequency of one axis after the forward transform.  With factors
// (F1, F2, ..) position p = k1*(F2*F3..) + k2*(F3..) + .. holds frequency
// k = k1 + F1*(k2 + F2*(k3 ..)).
struct OipAxisDigits {
    int n;            // number of factors (<= 4)
    int f[4];
    int L;
};

__host__ __device__ inline int oip_pos_to_freq(const OipAxisDigits &a, int p)
{
    if (a.n == 1) return p;
    int d[4];
    int rem = p;
    int stride = a.L;
    for (int i = 0; i < a.n; ++i) {
        stride /= a.f[i];
        d[i] = rem / stride;
        rem -= d[i] * stride;
    }
    int k = 0;
    for (int i = a.n - 1; i >= 0; --i) k = k * a.f[i] + d[i];
    return k;
}

__host__ __device__ inline int oip_freq_to_pos(const OipAxisDigits &a, int k)
{
    if (a.n == 1) return k;
    int p = 0;
    int stride = a.L;
    int rem = k;
    for (int i = 0; i < a.n; ++i) {
        stride /= a.f[i];
        int d = rem % a.f[i];
        rem /= a.f[i];
        p += d * stride;
    }
    return p;
}
