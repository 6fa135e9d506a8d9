// pansharpen.hip -- fusion of a PAN raster with the 4-band MSS product at a quarter of its resolution: the device side of
// `oip pansharpen`.  The reference has no counterpart.  include/oip_c.h states the arithmetic (oip_pansharpen_sfim_u16);
// tests/_pansharpen_ref.py restates it.
//
//   fused_b = up(MSS_b) * PAN / up(low(PAN))      (smoothing-filter intensity modulation)
//   up       x 4 by the OpenCV cubic at the phases 5/8, 7/8, 1/8, 3/8 as integer weights x 2048, separable: along the lines to
//            3 fractional bits (Hq), then across them; edges replicated.  The same operator for the four bands and for low(PAN)
//   gain     one IEEE f32 division per pixel, cut at max_gain, shared by the four bands; one f32 product and rint per sample
//
// A lane owns one MSS column cell, i.e. 4 output pixels of every line, and walks down kCells MSS lines (4 kCells output lines).
// It holds Hq of the 5 channels (4 bands + low PAN) x 4 column phases for the 4 MSS lines the cubic reaches: 80 registers that
// take one new MSS line per 4 output lines (5 neighbouring cells x 5 channels read; the neighbours' reads overlap, L1 / L2 serve
// them).  Per output line the lane reads its 4 PAN pixels (8 bytes) and stores 4 pixels x 4 bands (32 contiguous bytes, two
// 16-byte stores); a wave stores 2 KiB of one line.  The weights are compile-time constants of the unrolled phases.  Unaligned
// bases and pitches take the same kernel with 2-byte accesses (VEC = false).
#include "oip_internal.h"

namespace {

constexpr int kBlock = 256;                  // lanes = MSS column cells of a block: 1024 output pixels across
constexpr int kCells = 32;                   // MSS lines a block walks down: 128 output lines
constexpr int kUMax = 8 * 65535;

// 2048 x the cubic (a = -0.75) at t = 5/8, 7/8, 1/8, 3/8; the first tap of phases 0, 1 is cell - 2, of phases 2, 3 cell - 1
__device__ constexpr int kWt[4][4] = {{-135, 873, 1535, -225}, {-21, 235, 1981, -147}, {-147, 1981, 235, -21}, {-225, 1535, 873, -135}};

struct PanArgs {
    const uint16_t *pan, *mss, *low;
    uint16_t *dst;
    unsigned long long *stats;
    long pan_pitch, mss_pitch, low_pitch, dst_pitch;
    long h, y0, y1, j_first;                 // MSS lines; output lines [y0, y1); the MSS line of y0
    int w, tiles_x;
    float gmax;
};

// the raw samples of the 5 cells a lane's 4 pixels reach on one MSS line: 4 bands and low PAN
struct RawRow {
    unsigned m[5][4], l[5];
};

template <bool VEC> __device__ __forceinline__ void load_row(const PanArgs &a, long r, const int xi[5], RawRow &q)
{
    const uint16_t *m = a.mss + r * a.mss_pitch, *l = a.low + r * a.low_pitch;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const uint16_t *p = m + (long)xi[k] * 4;
        if constexpr (VEC) {
            const uint2 v = *reinterpret_cast<const uint2 *>(p);
            q.m[k][0] = v.x & 0xffffu; q.m[k][1] = v.x >> 16; q.m[k][2] = v.y & 0xffffu; q.m[k][3] = v.y >> 16;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) q.m[k][c] = p[c];
        }
        q.l[k] = l[xi[k]];
    }
}

// Hq of the 4 column phases from the samples of cells i - 2 .. i + 2: (sum + 128) >> 8, arithmetic shift
__device__ __forceinline__ void hfilter(const unsigned s[5], int hq[4])
{
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = r < 2 ? 0 : 1;
        int acc = 128;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc += __mul24(kWt[r][k], (int)s[o + k]);
        hq[r] = acc >> 8;
    }
}

__device__ __forceinline__ void row_to_hq(const RawRow &q, int hq[5][4])
{
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        unsigned s[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] = c < 4 ? q.m[k][c] : q.l[k];
        hfilter(s, hq[c]);
    }
}

template <bool VEC> __device__ __forceinline__ uint2 load_pan(const uint16_t *p)
{
    if constexpr (VEC) return *reinterpret_cast<const uint2 *>(p);
    return make_uint2(p[0] | ((unsigned)p[1] << 16), p[2] | ((unsigned)p[3] << 16));
}

// saturate_u16(rintf(v)) of 0 <= v < 2^23 in the low 16 bits of the result: v + 2^23 is rounded to an integer by the addition
// itself (to nearest, ties to even) and its bits are 0x4B000000 + that integer, whose low 16 bits survive the cut at
// 0x4B00FFFF.  (v <= 8 * 65535 * 8 here.)  Two instructions for the four of rint, conversion and the two bounds.
__device__ __forceinline__ unsigned sat_u16_bits(float v)
{
    const unsigned b = __float_as_uint(__fadd_rn(v, 8388608.f));
    return b < 0x4B00FFFFu ? b : 0x4B00FFFFu;
}
// the low halves of lo and hi as one word
__device__ __forceinline__ unsigned pack2(unsigned lo, unsigned hi) { return __builtin_amdgcn_perm(hi, lo, 0x05040100u); }

// one output line of phase RY from the window of 4 MSS lines: 4 pixels x 4 bands
template <bool VEC, int RY>
__device__ __forceinline__ void emit_line(const int (&win)[4][5][4], uint2 pan, float gmax, uint16_t *__restrict__ d, unsigned &nzero, unsigned &ncut)
{
    const unsigned pp[4] = {pan.x & 0xffffu, pan.x >> 16, pan.y & 0xffffu, pan.y >> 16};
    unsigned o[4][4];
#pragma unroll
    for (int px = 0; px < 4; ++px) {
        int u[5];
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            int acc = 1024;                                      // |Hq| < 2^23, |weight| < 2^11: the 24-bit product is exact
#pragma unroll
            for (int k = 0; k < 4; ++k) acc += __mul24(kWt[RY][k], win[k][c][px]);
            acc >>= 11;
            u[c] = acc < 0 ? 0 : (acc > kUMax ? kUMax : acc);
        }
        const float q = __fdiv_rn((float)pp[px], (float)u[4]);
        const bool zero = u[4] == 0, cut = !zero && q > gmax;
        const float g = zero ? 0.125f : (cut ? gmax : q);
        nzero += zero;
        ncut += cut;
#pragma unroll
        for (int c = 0; c < 4; ++c) o[px][c] = sat_u16_bits(__fmul_rn((float)u[c], g));
    }
    if constexpr (VEC) {
        uint4 *v = reinterpret_cast<uint4 *>(d);
        v[0] = make_uint4(pack2(o[0][0], o[0][1]), pack2(o[0][2], o[0][3]), pack2(o[1][0], o[1][1]), pack2(o[1][2], o[1][3]));
        v[1] = make_uint4(pack2(o[2][0], o[2][1]), pack2(o[2][2], o[2][3]), pack2(o[3][0], o[3][1]), pack2(o[3][2], o[3][3]));
    } else {
#pragma unroll
        for (int px = 0; px < 4; ++px)
#pragma unroll
            for (int c = 0; c < 4; ++c) d[px * 4 + c] = (uint16_t)o[px][c];
    }
}

template <bool VEC> __global__ __launch_bounds__(kBlock) void pansharpen_sfim_kernel(const PanArgs a)
{
    const long by = (long)blockIdx.x / a.tiles_x;
    const int bx = (int)((long)blockIdx.x - by * a.tiles_x);
    const int cell = bx * kBlock + (int)threadIdx.x;
    const bool active = cell < a.w;                              // the other lanes run along on the last cell and store nothing
    const int i = active ? cell : a.w - 1;
    int xi[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const int c = i - 2 + k;
        xi[k] = c < 0 ? 0 : (c > a.w - 1 ? a.w - 1 : c);
    }
    const long ja = a.j_first + by * kCells;                     // MSS lines [ja, jb) of this block
    const long jlast = (a.y1 - 1) >> 2;
    const long jb = ja + kCells < jlast + 1 ? ja + kCells : jlast + 1;
    auto line = [&](long j) { return j < 0 ? 0 : (j > a.h - 1 ? a.h - 1 : j); };

    int win[4][5][4];                                            // Hq of MSS lines j - 2 .. j + 1 (clamped): [line][channel][column phase]
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        RawRow q;
        load_row<VEC>(a, line(ja - 2 + k), xi, q);
        row_to_hq(q, win[k]);
    }
    unsigned nzero = 0, ncut = 0;
#pragma unroll 1
    for (long j = ja; j < jb; ++j) {
        // everything the 4 output lines of MSS line j read is requested first: the next MSS line and the 4 PAN lines (a line
        // outside [y0, y1) is not stored, and read from the nearest line inside)
        RawRow q;
        load_row<VEC>(a, line(j + 2), xi, q);
        uint2 pan[4];
        bool in[4];
        long off[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const long y = 4 * j + r;
            in[r] = y >= a.y0 && y < a.y1;
            off[r] = (y < a.y0 ? a.y0 : (y > a.y1 - 1 ? a.y1 - 1 : y)) - a.y0;
            pan[r] = load_pan<VEC>(a.pan + off[r] * a.pan_pitch + (long)i * 4);
        }
        uint16_t *d = a.dst + (long)i * 16;
        unsigned z = 0, c = 0;
        if (in[0] && active) emit_line<VEC, 0>(win, pan[0], a.gmax, d + off[0] * a.dst_pitch, z, c);
        if (in[1] && active) emit_line<VEC, 1>(win, pan[1], a.gmax, d + off[1] * a.dst_pitch, z, c);
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int ch = 0; ch < 5; ++ch)
#pragma unroll
                for (int p = 0; p < 4; ++p) win[k][ch][p] = win[k + 1][ch][p];
        row_to_hq(q, win[3]);
        if (in[2] && active) emit_line<VEC, 2>(win, pan[2], a.gmax, d + off[2] * a.dst_pitch, z, c);
        if (in[3] && active) emit_line<VEC, 3>(win, pan[3], a.gmax, d + off[3] * a.dst_pitch, z, c);
        nzero += z;
        ncut += c;
    }
    if (a.stats) {                                               // (a kernel argument: the same in every lane)
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            nzero += __shfl_down(nzero, s);
            ncut += __shfl_down(ncut, s);
        }
        if ((threadIdx.x & 63) == 0) {
            if (nzero) atomicAdd(a.stats, (unsigned long long)nzero);
            if (ncut) atomicAdd(a.stats + 1, (unsigned long long)ncut);
        }
    }
}

// [p, p + bytes) and [q, q + qbytes) share a byte
bool overlaps(const void *p, size_t bytes, const void *q, size_t qbytes)
{
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qbytes && b < a + bytes;
}

}  // namespace

extern "C" int oip_pansharpen_sfim_u16(oip_ctx *ctx, const uint16_t *d_pan, long pan_pitch, const uint16_t *d_mss, long mss_pitch, const uint16_t *d_low,
                                       long low_pitch, int w, long h, uint16_t *d_dst, long dst_pitch, long out_row0, long out_rows, int max_gain,
                                       uint64_t *d_stats)
{
    OIP_CHECK_CTX(ctx);
    if (!d_pan || !d_mss || !d_low || !d_dst || (((uintptr_t)d_pan | (uintptr_t)d_mss | (uintptr_t)d_low | (uintptr_t)d_dst) & 1) ||
        ((uintptr_t)d_stats & 7) || w < 1 || w > (1 << 26) || h < 1 || h > (1L << 40) || pan_pitch < 4L * w || mss_pitch < 4L * w || low_pitch < w ||
        dst_pitch < 16L * w || out_row0 < 0 || out_rows < 0 || out_rows > 4 * h || out_row0 > 4 * h - out_rows)
        return oip_fail(ctx, OIP_E_INVALID, "oip_pansharpen_sfim_u16: bad argument");
    if (max_gain < 1 || max_gain > OIP_PANSHARPEN_MAX_GAIN) return oip_fail(ctx, OIP_E_INVALID, "oip_pansharpen_sfim_u16: 1 <= max_gain <= 64 expected");
    if (out_rows == 0) return OIP_OK;
    const size_t dstBytes = ((size_t)(out_rows - 1) * dst_pitch + 16 * (size_t)w) * 2;
    if (overlaps(d_dst, dstBytes, d_pan, ((size_t)(out_rows - 1) * pan_pitch + 4 * (size_t)w) * 2) ||
        overlaps(d_dst, dstBytes, d_mss, ((size_t)(h - 1) * mss_pitch + 4 * (size_t)w) * 2) ||
        overlaps(d_dst, dstBytes, d_low, ((size_t)(h - 1) * low_pitch + (size_t)w) * 2) || (d_stats && overlaps(d_dst, dstBytes, d_stats, 16)))
        return oip_fail(ctx, OIP_E_INVALID, "oip_pansharpen_sfim_u16: the product overlaps an input");

    PanArgs a;
    a.pan = d_pan;
    a.mss = d_mss;
    a.low = d_low;
    a.dst = d_dst;
    a.stats = reinterpret_cast<unsigned long long *>(d_stats);
    a.pan_pitch = pan_pitch;
    a.mss_pitch = mss_pitch;
    a.low_pitch = low_pitch;
    a.dst_pitch = dst_pitch;
    a.h = h;
    a.y0 = out_row0;
    a.y1 = out_row0 + out_rows;
    a.j_first = out_row0 >> 2;
    a.w = w;
    a.tiles_x = (w + kBlock - 1) / kBlock;
    a.gmax = (float)max_gain * 0.125f;
    const long chunks = (((a.y1 - 1) >> 2) - a.j_first + kCells) / kCells;
    if (a.tiles_x * chunks >= (1L << 31)) return oip_fail(ctx, OIP_E_UNSUPPORTED, "oip_pansharpen_sfim_u16: more than 2^31 tiles in one call");
    const bool vec = ((uintptr_t)d_pan & 7) == 0 && pan_pitch % 4 == 0 && ((uintptr_t)d_mss & 7) == 0 && mss_pitch % 4 == 0 &&
                     ((uintptr_t)d_dst & 15) == 0 && dst_pitch % 8 == 0;
    const unsigned blocks = (unsigned)(a.tiles_x * chunks);
    OipProfScope prof(ctx, vec ? "pansharpen_sfim_kernel" : "pansharpen_sfim_kernel_general");
    if (vec) hipLaunchKernelGGL(pansharpen_sfim_kernel<true>, dim3(blocks), dim3(kBlock), 0, ctx->stream, a);
    else hipLaunchKernelGGL(pansharpen_sfim_kernel<false>, dim3(blocks), dim3(kBlock), 0, ctx->stream, a);
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}
