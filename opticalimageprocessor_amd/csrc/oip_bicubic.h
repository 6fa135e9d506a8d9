// oip_bicubic.h -- OpenCV-exact 4x4 bicubic accumulation for the remap kernels.
//
// cv::remap(..., INTER_CUBIC, BORDER_CONSTANT, 0) on 16U data is
// remapBicubic<Cast<float,ushort>, float, 1> (OpenCV imgproc/imgwarp.cpp):
//   * the 2-D weight table entry is w[ky*4+kx] = wy[ky] * wx[kx]   (one f32 product)
//   * fully-inside window:   sum  = S00*w0 + S01*w1 + S02*w2 + S03*w3;      (row 0)
//                            sum += S10*w4 + ... ;  sum += row2;  sum += row3;
//     i.e. each row is summed left to right on its own, then added to the running sum
//   * window touching the border: sum = 0, then tap by tap  sum += S*w  for the taps that
//     exist (constant border value 0 contributes nothing and is skipped)
//   * result = saturate_cast<ushort>(cvRound(sum))
// All products and sums are separate f32 roundings (the x86-64 baseline build of OpenCV
// has no FMA), hence the explicit __fmul_rn/__fadd_rn: nothing here may contract.
#pragma once

#include <hip/hip_runtime.h>

__device__ __forceinline__ float oip_row_dot(float s0, float s1, float s2, float s3, float wy, const float *wx)
{
    float w0 = __fmul_rn(wy, wx[0]), w1 = __fmul_rn(wy, wx[1]), w2 = __fmul_rn(wy, wx[2]), w3 = __fmul_rn(wy, wx[3]);
    float r = __fadd_rn(__fmul_rn(s0, w0), __fmul_rn(s1, w1));
    r = __fadd_rn(r, __fmul_rn(s2, w2));
    r = __fadd_rn(r, __fmul_rn(s3, w3));
    return r;
}

// v[ky][kx]: source samples as f32 (zeros where invalid)
__device__ __forceinline__ float oip_bicubic_interior(const float v[4][4], const float *wx, const float *wy)
{
    float sum = oip_row_dot(v[0][0], v[0][1], v[0][2], v[0][3], wy[0], wx);
    sum = __fadd_rn(sum, oip_row_dot(v[1][0], v[1][1], v[1][2], v[1][3], wy[1], wx));
    sum = __fadd_rn(sum, oip_row_dot(v[2][0], v[2][1], v[2][2], v[2][3], wy[2], wx));
    sum = __fadd_rn(sum, oip_row_dot(v[3][0], v[3][1], v[3][2], v[3][3], wy[3], wx));
    return sum;
}

// xmask/ymask: bit i set when tap column/row i exists
__device__ __forceinline__ float oip_bicubic_border(const float v[4][4], const float *wx, const float *wy,
                                                    unsigned xmask, unsigned ymask)
{
    float sum = 0.f;
#pragma unroll
    for (int ky = 0; ky < 4; ++ky) {
        if (!(ymask & (1u << ky))) continue;
#pragma unroll
        for (int kx = 0; kx < 4; ++kx) {
            if (!(xmask & (1u << kx))) continue;
            sum = __fadd_rn(sum, __fmul_rn(v[ky][kx], __fmul_rn(wy[ky], wx[kx])));
        }
    }
    return sum;
}

// ---- 8 output pixels per lane, taps as packed pairs (align.hip's and remap.hip's fast kernels) ----------------------------
// These kernels are bound by the issue rate of vector instructions (profiles/experiments/r03_valu_rate.txt and
// r04_valu_rate2.txt give the cycles per instruction), so the 16-tap sums use gfx950's packed f32 instructions (v_pk_mul_f32 /
// v_pk_add_f32: two pixels per issue slot, 4.7 cycles against 2 x 3.1) on operands that ARE register pairs already -- a pair the
// compiler has to assemble costs a v_pk_mov_b32 (5.5 cycles) or two v_mov_b32, which is what its own vectoriser did to the
// scalar form.  A lane's 8 pixels are paired (j, j + 4): the pair's tap kx is then (s[j + kx], s[j + 4 + kx]) for every kx, so
// with the window line held as the seven pairs D[i] = (s[i], s[i + 4]) every operand of every tap is one of them.
typedef float oip_f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void oip_expand_pairs(const uint32_t w[6], bool odd, oip_f2 D[7])
{
    // samples start at the low half of w[0] for an even first column, at its high half for an odd one: bring the
    // odd case to the even layout with one funnel shift per dword, then one conversion per sample
    const unsigned sh = odd ? 16u : 0u;
    uint32_t e[6];
#pragma unroll
    for (int i = 0; i < 5; ++i) e[i] = __builtin_amdgcn_alignbit(w[i + 1], w[i], sh);
    e[5] = w[5] >> sh;
    float s[11];
#pragma unroll
    for (int q = 0; q < 11; ++q) s[q] = (q & 1) ? (float)(e[q >> 1] >> 16) : (float)(e[q >> 1] & 0xffffu);
#pragma unroll
    for (int i = 0; i < 7; ++i) { D[i].x = s[i]; D[i].y = s[i + 4]; }
}

// One tap row of the 8 pixels: sum[j] = (pixel j, pixel j + 4).  Per pair 4 packed multiplies and 3 packed adds, each half in
// oip_bicubic_interior's order: products rounded, row sum left to right, rows added in order (-ffp-contract=off keeps the
// compiler from fusing them).
__device__ __forceinline__ void oip_row_taps8(const oip_f2 D[7], const float *w4, bool first, oip_f2 sum[4])
{
    const oip_f2 w0 = {w4[0], w4[0]}, w1 = {w4[1], w4[1]}, w2 = {w4[2], w4[2]}, w3 = {w4[3], w4[3]};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        oip_f2 rr = D[j] * w0 + D[j + 1] * w1;
        rr = rr + D[j + 2] * w2;
        rr = rr + D[j + 3] * w3;
        sum[j] = first ? rr : sum[j] + rr;
    }
}

// saturate_cast<ushort> of the 8 sums and their 16 bytes in pixel order.  clamp(cvRound(v), 0, 65535) as three instructions per
// pixel pair less than rndne + cvt + med3 + pack: v + 1.5 * 2^23 rounds v to an integer exactly as rintf does (ties to even;
// |v| < 2^22: the sums of 16 products of 16-bit samples with weights of magnitude < 1.3 are far inside) and leaves it in the low
// bits of the float, 0x4B400000 + cvRound(v); clamping those bits between 0x4B400000 and 0x4B40FFFF as integers clamps the value,
// and the low halves of two results are one v_perm_b32.
__device__ __forceinline__ uint4 oip_sat_pack8(const oip_f2 sum[4])
{
    unsigned c[8];
    const oip_f2 magic = {12582912.0f, 12582912.0f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const oip_f2 t = sum[j] + magic;
        const int lo = (int)__float_as_uint(t.x), hi = (int)__float_as_uint(t.y);
        c[j] = (unsigned)(lo < 0x4B400000 ? 0x4B400000 : (lo > 0x4B40FFFF ? 0x4B40FFFF : lo));          // one v_med3_i32
        c[j + 4] = (unsigned)(hi < 0x4B400000 ? 0x4B400000 : (hi > 0x4B40FFFF ? 0x4B40FFFF : hi));
    }
    uint4 o;
    o.x = __builtin_amdgcn_perm(c[1], c[0], 0x05040100u);
    o.y = __builtin_amdgcn_perm(c[3], c[2], 0x05040100u);
    o.z = __builtin_amdgcn_perm(c[5], c[4], 0x05040100u);
    o.w = __builtin_amdgcn_perm(c[7], c[6], 0x05040100u);
    return o;
}

// ---- the same 8 pixels with fp16 accumulate (BASELINE config 5: "fp16 accumulate, tolerance stated") ------------------------
// Same geometry, phases, tap positions and border rules as the f32 form; only the 16-tap sum of the regular interior pixels
// changes: samples and the sixteen 2-D weights are rounded to fp16 and the sum is a chain of packed fp16 FMAs (v_pk_fma_f16: two
// output pixels per instruction, 16 instructions per pixel pair instead of 62 unfused f32 operations).  NOT the parity mode:
// fp16 carries 11 significant bits.  Samples enter as (sample - 2048) -- exact integers for 12-bit data -- and the running sum
// of 16 products rounds to 0.5..2 DN steps depending on its magnitude.  Measured against the f32 kernel on the 12-bit synthetic
// strips: tests/test_gpu_config5.py::test_remap_f16acc_tolerance prints max and mean |delta| (DESIGN.md section 4.2 records
// them: max 5, mean 0.25 DN); the bound asserted for arbitrary data is |delta| <= 6 + max|sample - 2048| / 64.  The mode is
// specified for data up to 15 bits (the biased sample must fit int16).  Irregular column groups and section-border lines still
// go through the f32 fix-up kernels.
typedef _Float16 oip_h2 __attribute__((ext_vector_type(2)));

// (a.y, b.x): the pair one sample further along the line
__device__ __forceinline__ oip_h2 oip_h2_shift(oip_h2 a, oip_h2 b)
{
    const uint32_t ua = __builtin_bit_cast(uint32_t, a), ub = __builtin_bit_cast(uint32_t, b);
    return __builtin_bit_cast(oip_h2, __builtin_amdgcn_alignbit(ub, ua, 16));
}

// one source line as packed fp16 pairs of (sample - kOipF16Bias): E[i] = (g[2i], g[2i+1]), O[i] = (g[2i+1], g[2i+2]),
// g[q] = sample c0 + q.  The bias is taken off in 16-bit integer arithmetic (exact), so 12-bit data enters fp16
// as integers in [-2048, 2047] -- all exactly representable -- and the partial sums stay small; the bicubic
// weights sum to one, so the bias is added back to the finished sum.
constexpr int kOipF16Bias = 2048;
__device__ __forceinline__ oip_h2 oip_h2_from_biased_pair(uint32_t w)
{
    oip_h2 r;
    r.x = (_Float16)(short)((w & 0xffffu) - kOipF16Bias);
    r.y = (_Float16)(short)((w >> 16) - kOipF16Bias);
    return r;
}
__device__ __forceinline__ void oip_expand_h(const uint32_t w[6], bool odd, oip_h2 E[6], oip_h2 O[5])
{
    // odd first column: one funnel shift per dword brings the line to the even layout (as oip_expand_pairs does) -- selecting
    // between the two layouts after the conversion cost ten v_cndmask per line
    const unsigned sh = odd ? 16u : 0u;
#pragma unroll
    for (int i = 0; i < 5; ++i) E[i] = oip_h2_from_biased_pair(__builtin_amdgcn_alignbit(w[i + 1], w[i], sh));
    E[5] = oip_h2_from_biased_pair(w[5] >> sh);       // only its first half (sample 10) is used, through O[4]
#pragma unroll
    for (int i = 0; i < 5; ++i) O[i] = oip_h2_shift(E[i], E[i + 1]);
}
// The 8 fp16 sums (acc[p] = pixels 2p, 2p+1) biased back, saturated and packed.  (float)acc + 2048 is exact in f32 for every
// fp16 value that can round to a different integer than its neighbour (|acc| >= 0.5 has an ulp >= 2^-11; below that the sum
// stays strictly inside (2047.5, 2048.5)), so adding 2048 + 1.5 * 2^23 in one step rounds exactly as rintf((float)acc + 2048)
// does and leaves the integer in the low bits (oip_sat_pack8's trick); the integer clamp maps +inf to 65535 and -inf to 0 as
// the fminf / fmaxf pair it replaces did.  A NaN sum -- not reachable: 16 products of int16 samples with weights whose
// magnitudes add up to 1.6 stay far below fp16's 65504 -- would saturate by its sign bit.
__device__ __forceinline__ uint4 oip_h2_sat_pack8(const oip_h2 acc[4])
{
    unsigned c[8];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int lo = (int)__float_as_uint((float)acc[p].x + (12582912.0f + (float)kOipF16Bias));
        const int hi = (int)__float_as_uint((float)acc[p].y + (12582912.0f + (float)kOipF16Bias));
        c[2 * p] = (unsigned)(lo < 0x4B400000 ? 0x4B400000 : (lo > 0x4B40FFFF ? 0x4B40FFFF : lo));
        c[2 * p + 1] = (unsigned)(hi < 0x4B400000 ? 0x4B400000 : (hi > 0x4B40FFFF ? 0x4B40FFFF : hi));
    }
    uint4 o;
    o.x = __builtin_amdgcn_perm(c[1], c[0], 0x05040100u);
    o.y = __builtin_amdgcn_perm(c[3], c[2], 0x05040100u);
    o.z = __builtin_amdgcn_perm(c[5], c[4], 0x05040100u);
    o.w = __builtin_amdgcn_perm(c[7], c[6], 0x05040100u);
    return o;
}

// ---- what the fast kernels share: line load, tap window, store ---------------------------------------------------------
// One source line of a lane = the 11 consecutive u16 its 8 pixels tap = 6 dwords from a 4-byte aligned address (12 samples with
// the one in front of an odd first column).  `lane_base` is the dword holding the lane's first tap column on line 0; widths are
// even, so a line is half_pitch dwords and the address is one 64-bit multiply-add with the six loads at immediate offsets.  A
// REGULAR group's window ends inside its own line (first column + 11 < width, checked by the callers), so no dword can leave
// the buffer and nothing is clamped: the clamped form made the compiler carry six separate 64-bit addresses through the merge
// of its two branches (84 v_lshl_add_u64 per line, a fifth of the vector instructions of kernels bound by their issue rate).
// The load is split from its use: the callers request the raw dwords of the NEXT output line's new source line before the
// current line's 16-tap sums, so twice the bytes are in flight per wave (the kernels are also bound by memory-level
// parallelism: 1 KiB per wave and line, 16-24 waves per CU, against ~35 KiB per CU that the latency-bandwidth product of HBM
// asks for).
__device__ __forceinline__ void oip_load_raw6(const uint32_t *__restrict__ lane_base, long row, int half_pitch, uint32_t w[6])
{
    const uint32_t *q = lane_base + row * half_pitch;
#pragma unroll
    for (int i = 0; i < 6; ++i) w[i] = q[i];
}

// The four tap lines of a lane's 8 pixels and their sixteen 2-D weights, in either accumulate mode.  Tap line t of step k of a
// loop unrolled by 4 lives in slot (k + t) & 3, so a window that slides by one line replaces one slot and the rotation is
// static.  expand(): raw dwords of a line (first tap column c0) into a slot; weights(): w[ky*4+kx] = wy[ky] * wx[kx], one f32
// product each (then rounded to fp16 for F16), rebuilt by the callers only when the y phase changes; sums(k): the 8 pixels of
// the line at step k, saturated and packed in pixel order.
template <bool F16> struct OipTaps8;

template <> struct OipTaps8<false> {
    oip_f2 win[4][7];
    float w2d[16];
    __device__ __forceinline__ void expand(const uint32_t raw[6], int c0, int slot) { oip_expand_pairs(raw, c0 & 1, win[slot]); }
    __device__ __forceinline__ void weights(const float *__restrict__ tab1d, int fy, const float wx[4])
    {
#pragma unroll
        for (int ky = 0; ky < 4; ++ky) {
            const float wy = tab1d[fy * 4 + ky];
#pragma unroll
            for (int kx = 0; kx < 4; ++kx) w2d[ky * 4 + kx] = __fmul_rn(wy, wx[kx]);
        }
    }
    __device__ __forceinline__ uint4 sums(int k) const
    {
        oip_f2 sum[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) oip_row_taps8(win[(k + t) & 3], w2d + t * 4, t == 0, sum);
        return oip_sat_pack8(sum);
    }
};

template <> struct OipTaps8<true> {
    oip_h2 E[4][6], O[4][5];
    oip_h2 w2d[16];
    __device__ __forceinline__ void expand(const uint32_t raw[6], int c0, int slot) { oip_expand_h(raw, c0 & 1, E[slot], O[slot]); }
    __device__ __forceinline__ void weights(const float *__restrict__ tab1d, int fy, const float wx[4])
    {
#pragma unroll
        for (int ky = 0; ky < 4; ++ky) {
            const float wy = tab1d[fy * 4 + ky];
#pragma unroll
            for (int kx = 0; kx < 4; ++kx) {
                const _Float16 h = (_Float16)__fmul_rn(wy, wx[kx]);
                w2d[ky * 4 + kx] = oip_h2{h, h};
            }
        }
    }
    __device__ __forceinline__ uint4 sums(int k) const
    {
        oip_h2 acc[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {             // output pixels 2p, 2p+1: one FMA chain over the 16 taps, row by row
            acc[p] = oip_h2{(_Float16)0.f, (_Float16)0.f};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const oip_h2 *Et = E[(k + t) & 3], *Ot = O[(k + t) & 3];
                acc[p] = __builtin_elementwise_fma(Et[p], w2d[t * 4 + 0], acc[p]);
                acc[p] = __builtin_elementwise_fma(Ot[p], w2d[t * 4 + 1], acc[p]);
                acc[p] = __builtin_elementwise_fma(Et[p + 1], w2d[t * 4 + 2], acc[p]);
                acc[p] = __builtin_elementwise_fma(Ot[p + 1], w2d[t * 4 + 3], acc[p]);
            }
        }
        return oip_h2_sat_pack8(acc);
    }
};

// The 8 pixels `o` of output columns x0 .. x0 + 7 to drow[0..7]; only columns >= col0 are stored.  vec: 16-byte stores to this
// raster are aligned.  The scalar tail takes the group that straddles col0 and destinations whose 16-byte stores would be
// misaligned.
__device__ __forceinline__ void oip_store8(uint16_t *drow, uint4 o, int x0, int col0, int vec)
{
    if (x0 >= col0 && vec) {
        *reinterpret_cast<uint4 *>(drow) = o;
    } else {
        const unsigned d[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (x0 + j >= col0) drow[j] = (uint16_t)(d[j >> 1] >> (16 * (j & 1)));
    }
}
