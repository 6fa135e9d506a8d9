// phasecorr.hip -- cv::phaseCorrelate and its two drivers on gfx950.
//
// Replaces the loop bodies of Stitcher::CalcSttParameters (stitcher.h:166-191) and
// PreProcessor::CalcInterBandCorrelation (preproc.h:251-329) including the OpenCV calls they
// make: Mat1w->Mat1f window conversion, cv::resize(INTER_CUBIC) x4 up-sampling of the MSS
// window (preproc.h:302-307) and cv::phaseCorrelate (stitcher.h:180, preproc.h:316).
//
// cv::phaseCorrelate (OpenCV imgproc/phasecorr.cpp), restated:
//   pad to getOptimalDFTSize with zeros (bottom/right) -> F1 = dft(a), F2 = dft(b)
//   P = F1 conj(F2)            (mulSpectrums, f32)
//   Pm = |P|                   (magSpectrums; the purely real bins store P*P instead)
//   C = P Pm / (Pm^2 + eps)    (divSpectrums: f32 formula in the row body, fp64 formula in the
//                               first/last column, C = P/(P*P+eps) in the purely real bins)
//   c = idft(C) unscaled -> fftShift -> first maximum -> 5x5 weighted centroid (fp64)
//   response = sum(5x5)/(M N);  shift = (N/2 - cx, M/2 - cy)
// Here two real images ride one complex FFT (fft.hip): for z = a + i b the spectra are
//   A(k) = (Z(k) + conj Z(-k))/2,   B(k) = (Z(k) - conj Z(-k))/(2i)
// and two correlation surfaces ride one inverse FFT as Y = C1 + i C2.  The FFT round-off
// differs from OpenCV's own DFT, so shifts agree to ~1e-4 px, not bitwise (parity unpinned:
// OpenCV is not in the reference tree).
#include "oip_corrgeom.h"
#include "oip_corrroute.h"
#include "oip_fft.h"
#include "oip_fft_dev.h"
#include "oip_internal.h"

#include <cfloat>
#include <cmath>

namespace {

using namespace oipcorr;      // the plan of a correlation call: switches, route, FFT plans, workspace (oip_corrroute.h)

constexpr int kBlock = 256;

// ---- window / resize -----------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void window_u16_to_f32_kernel(const uint16_t *__restrict__ img, size_t pitch,
                                                                   long row0, int col0, int rows, int cols,
                                                                   float *__restrict__ out)
{
    long i = (long)blockIdx.x * kBlock + threadIdx.x;
    const long n = (long)rows * cols;
    const long stride = (long)gridDim.x * kBlock;
    for (; i < n; i += stride) {
        long y = i / cols;
        int x = (int)(i - y * cols);
        out[i] = (float)img[(size_t)(row0 + y) * pitch + col0 + x];
    }
}

// cv::resize(f32, INTER_CUBIC) (OpenCV imgproc/resize.cpp).  The coefficient set-up is done on
// the host exactly as cv::hal::resize does it -- fx = (float)((dx+0.5)*scale - 0.5),
// sx = floor(fx), fx -= sx, interpolateCubic(fx) -- and cached per shape; the kernel is the
// HResizeCubic + VResizeCubic pair: 4 horizontal taps (edge replicated) into an f32 row value,
// then 4 vertical taps, every product and sum a separate f32 rounding.
template <typename SrcT>
__global__ __launch_bounds__(kBlock) void resize_cubic_kernel(const SrcT *__restrict__ src, long spitch, int sw, int sh,
                                                              float *__restrict__ dst, int dw, int dh,
                                                              const int *__restrict__ xofs, const float4 *__restrict__ alpha,
                                                              const int *__restrict__ yofs, const float4 *__restrict__ beta)
{
    const int dx = blockIdx.x * kBlock + threadIdx.x;
    const int dy = blockIdx.y;
    if (dx >= dw) return;
    const int sx = xofs[dx], sy = yofs[dy];
    const float4 a = alpha[dx], b = beta[dy];
    int cx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int c = sx - 1 + j;
        cx[j] = c < 0 ? 0 : (c > sw - 1 ? sw - 1 : c);
    }
    float r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        int yk = sy - 1 + k;
        yk = yk < 0 ? 0 : (yk > sh - 1 ? sh - 1 : yk);
        const SrcT *S = src + (size_t)yk * spitch;
        float v = __fmul_rn((float)S[cx[0]], a.x);
        v = __fadd_rn(v, __fmul_rn((float)S[cx[1]], a.y));
        v = __fadd_rn(v, __fmul_rn((float)S[cx[2]], a.z));
        v = __fadd_rn(v, __fmul_rn((float)S[cx[3]], a.w));
        r[k] = v;
    }
    float o = __fmul_rn(r[0], b.x);
    o = __fadd_rn(o, __fmul_rn(r[1], b.y));
    o = __fadd_rn(o, __fmul_rn(r[2], b.z));
    o = __fadd_rn(o, __fmul_rn(r[3], b.w));
    dst[(size_t)dy * dw + dx] = o;
}

// Vertical half of the cubic up-sampling only: V[dy][x] = sum_k beta[dy][k] * S[clamp(yofs[dy] - 1 + k)][x].
// The horizontal half is applied by the loader of the first FFT pass (OipFftIo::re_v / im_v), so the
// fully up-sampled image -- 16x the band window -- never exists in memory; V is 4x the window, written
// once and read once.  cv::resize interpolates horizontally first; doing the vertical taps first
// changes the f32 rounding of an output by an ulp or so, far inside what the FFT's own round-off
// already does to the correlation (the separate oip_resize_cubic_f32 entry keeps cv::resize's order
// bit for bit).
constexpr int kVRows = 4;       // output rows per thread of the vertical pass (they share most source rows)
constexpr int kVBatch = 8;      // images per launch (the four bands of two units)
template <typename SrcT> struct VBatch {
    const SrcT *src[kVBatch];
    float *dst[kVBatch];
    long spitch[kVBatch];       // source pitch per image (raster windows and compact unit windows mix in one batch)
};
template <typename SrcT>
__global__ __launch_bounds__(kBlock) void resize_cubic_v_kernel(VBatch<SrcT> vb, int sw, int sh, int dh,
                                                                const int *__restrict__ yofs, const float4 *__restrict__ beta)
{
    const int x = blockIdx.x * kBlock + threadIdx.x;
    if (x >= sw) return;
    const SrcT *__restrict__ src = vb.src[blockIdx.z];
    float *__restrict__ dst = vb.dst[blockIdx.z];
    const long spitch = vb.spitch[blockIdx.z];
#pragma unroll
    for (int j = 0; j < kVRows; ++j) {
        const int dy = blockIdx.y * kVRows + j;
        if (dy >= dh) break;
        const int sy = yofs[dy];
        const float4 b = beta[dy];
        int y0 = sy - 1, y1 = sy, y2 = sy + 1, y3 = sy + 2;
        y0 = y0 < 0 ? 0 : (y0 > sh - 1 ? sh - 1 : y0);
        y1 = y1 < 0 ? 0 : (y1 > sh - 1 ? sh - 1 : y1);
        y2 = y2 < 0 ? 0 : (y2 > sh - 1 ? sh - 1 : y2);
        y3 = y3 < 0 ? 0 : (y3 > sh - 1 ? sh - 1 : y3);
        float v = __fmul_rn((float)src[(size_t)y0 * spitch + x], b.x);
        v = __fadd_rn(v, __fmul_rn((float)src[(size_t)y1 * spitch + x], b.y));
        v = __fadd_rn(v, __fmul_rn((float)src[(size_t)y2 * spitch + x], b.z));
        v = __fadd_rn(v, __fmul_rn((float)src[(size_t)y3 * spitch + x], b.w));
        dst[(size_t)dy * sw + x] = v;
    }
}

// Exact x4 up-sampling (the reference geometry: MSS GSD = 4 x PAN GSD).  One lane owns one
// source pixel (q, p) and produces its 4x4 block of outputs from the 5x5 source neighbourhood:
// the four outputs of a row share their horizontal taps, the four rows share the horizontal
// sums.  Taps, clamping and the order of every f32 product/sum are those of the generic kernel
// (the host verified that each output's first tap lies in the lane's 5 columns / rows);
// 25 loads and 4 16-byte stores per 16 outputs instead of 16 loads and one 4-byte store each.
template <typename SrcT>
__global__ __launch_bounds__(kBlock) void resize_cubic_x4_kernel(const SrcT *__restrict__ src, long spitch, int sw, int sh,
                                                                 float *__restrict__ dst, int dw,
                                                                 const int *__restrict__ xofs, const float4 *__restrict__ alpha,
                                                                 const int *__restrict__ yofs, const float4 *__restrict__ beta)
{
    const int q = blockIdx.x * kBlock + threadIdx.x;
    const int p = blockIdx.y;
    if (q >= sw) return;
    float S[5][5];
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        int yr = p - 2 + r;
        yr = yr < 0 ? 0 : (yr > sh - 1 ? sh - 1 : yr);
        const SrcT *row = src + (size_t)yr * spitch;
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            int xc = q - 2 + c;
            xc = xc < 0 ? 0 : (xc > sw - 1 ? sw - 1 : xc);
            S[r][c] = (float)row[xc];
        }
    }
    float H[5][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int dx = 4 * q + i;
        const float4 a = alpha[dx];
        const bool hi = (xofs[dx] - 1) - (q - 2) != 0;         // first tap is column q-1 instead of q-2
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            const float s0 = hi ? S[r][1] : S[r][0], s1 = hi ? S[r][2] : S[r][1];
            const float s2 = hi ? S[r][3] : S[r][2], s3 = hi ? S[r][4] : S[r][3];
            float v = __fmul_rn(s0, a.x);
            v = __fadd_rn(v, __fmul_rn(s1, a.y));
            v = __fadd_rn(v, __fmul_rn(s2, a.z));
            v = __fadd_rn(v, __fmul_rn(s3, a.w));
            H[r][i] = v;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int dy = 4 * p + j;
        const float4 b = beta[dy];
        const bool hi = (yofs[dy] - 1) - (p - 2) != 0;
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float h0 = hi ? H[1][i] : H[0][i], h1 = hi ? H[2][i] : H[1][i];
            const float h2 = hi ? H[3][i] : H[2][i], h3 = hi ? H[4][i] : H[3][i];
            float v = __fmul_rn(h0, b.x);
            v = __fadd_rn(v, __fmul_rn(h1, b.y));
            v = __fadd_rn(v, __fmul_rn(h2, b.z));
            v = __fadd_rn(v, __fmul_rn(h3, b.w));
            o[i] = v;
        }
        *reinterpret_cast<float4 *>(dst + (size_t)dy * dw + 4 * q) = make_float4(o[0], o[1], o[2], o[3]);
    }
}

// ---- cross-power spectrum -----------------------------------------------------------------------
struct SpecRef {
    const float2 *z;    // packed spectrum (scrambled order)
    int part;           // 0: the image in the real slot, 1: the image in the imaginary slot
};
struct XpowerJob {
    SpecRef a[2], b[2]; // correlation c: A = a[c], B = b[c]
    int ncorr;          // 1 or 2 (second goes to the imaginary slot of the output)
};

__device__ __forceinline__ float2 spec_of(int part, float2 zk, float2 zm)
{
    if (part == 0) return make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
    return make_float2(0.5f * (zk.y + zm.y), 0.5f * (zm.x - zk.x));
}

// C for one bin, following mulSpectrums/magSpectrums/divSpectrums.  The formulas are odd in the
// imaginary part, so C(-k) == conj(C(k)) bit for bit: the CCS-implied half needs no own path.
__device__ __forceinline__ float2 cross_power_bin(float2 A, float2 B, bool real_bin, bool edge_col)
{
    const float eps = FLT_EPSILON;
    if (real_bin) {
        float p = __fmul_rn(A.x, B.x);
        float m = __fmul_rn(p, p);
        return make_float2(__fdiv_rn(p, __fadd_rn(m, eps)), 0.f);
    }
    float pr = __fadd_rn(__fmul_rn(A.x, B.x), __fmul_rn(A.y, B.y));
    float pi = __fsub_rn(__fmul_rn(A.y, B.x), __fmul_rn(A.x, B.y));
    float mag = (float)__dsqrt_rn(__dadd_rn(__dmul_rn((double)pr, (double)pr), __dmul_rn((double)pi, (double)pi)));
    if (edge_col) {
        double denom = __dadd_rn(__dmul_rn((double)mag, (double)mag), (double)eps);
        double re = __dmul_rn((double)pr, (double)mag);
        double im = __dmul_rn((double)pi, (double)mag);
        return make_float2((float)__ddiv_rn(re, denom), (float)__ddiv_rn(im, denom));
    }
    double denom = (double)__fadd_rn(__fmul_rn(mag, mag), eps);
    double re = (double)__fmul_rn(pr, mag);
    double im = (double)__fmul_rn(pi, mag);
    return make_float2((float)__ddiv_rn(re, denom), (float)__ddiv_rn(im, denom));
}

// The same bin for the fused row stage.  The spectra feeding it already differ from OpenCV's in
// their last bits (another FFT factorisation), so correctly rounded double-precision sqrt and
// divisions buy nothing there; what must survive is the structure: the magnitude formed in double
// (no overflow before the float rounding), mag * mag and p * mag rounded to float (where the
// reference overflows to inf and produces 0 or NaN), the + eps, and the special bins.  sqrt and the
// reciprocal use the hardware approximations (relative error about 1e-7, below the FFT round-off);
// inf and NaN propagate as in the division: x * (1 / inf) = 0, inf * 0 = NaN.
__device__ __forceinline__ float2 cross_power_bin_fast(float2 A, float2 B, bool real_bin, bool edge_col)
{
    if (real_bin || edge_col) return cross_power_bin(A, B, real_bin, edge_col);
    const float eps = FLT_EPSILON;
    float pr = __fadd_rn(__fmul_rn(A.x, B.x), __fmul_rn(A.y, B.y));
    float pi = __fsub_rn(__fmul_rn(A.y, B.x), __fmul_rn(A.x, B.y));
    float mag = (float)__builtin_amdgcn_sqrt(__dadd_rn(__dmul_rn((double)pr, (double)pr), __dmul_rn((double)pi, (double)pi)));
    float r = __builtin_amdgcn_rcpf(__fadd_rn(__fmul_rn(mag, mag), eps));
    return make_float2(__fmul_rn(__fmul_rn(pr, mag), r), __fmul_rn(__fmul_rn(pi, mag), r));
}

// One workgroup row handles the spectrum line of frequency ky AND its mirror -ky: every input
// line is read once, C(k) is computed once and written as Y(k) and Y(-k) = conj(C1) + i conj(C2).
// The x axis of the reference shapes is a single pass (natural order), so the mirrored
// column N-kx is a reversed, still coalesced, access.
__global__ __launch_bounds__(kBlock) void cross_power_kernel(float2 *__restrict__ out, XpowerJob job, int M, int N,
                                                             int P, OipAxisDigits yd, OipAxisDigits xd)
{
    const int px = blockIdx.x * kBlock + threadIdx.x;
    const int ky = blockIdx.y;                        // 0 .. M/2
    if (px >= N) return;
    const int kx = oip_pos_to_freq(xd, px);
    const int nkx = kx ? N - kx : 0, nky = ky ? M - ky : 0;
    const long r1 = (long)oip_freq_to_pos(yd, ky) * P, r2 = (long)oip_freq_to_pos(yd, nky) * P;
    const int px2 = oip_freq_to_pos(xd, nkx);
    const bool edge_col = (kx == 0) || (2 * kx == N);
    const bool real_bin = edge_col && (ky == 0 || 2 * ky == M);
    float2 y = make_float2(0.f, 0.f), ym = make_float2(0.f, 0.f);
    float2 zk[3], zm[3];
    const float2 *arr[3] = {nullptr, nullptr, nullptr};
    int narr = 0;
    // distinct input arrays of the job (at most 3)
    for (int c = 0; c < job.ncorr; ++c)
        for (int s = 0; s < 2; ++s) {
            const float2 *z = s ? job.b[c].z : job.a[c].z;
            bool seen = false;
            for (int i = 0; i < narr; ++i) seen = seen || arr[i] == z;
            if (!seen && narr < 3) arr[narr++] = z;
        }
    for (int i = 0; i < narr; ++i) { zk[i] = arr[i][r1 + px]; zm[i] = arr[i][r2 + px2]; }
    for (int c = 0; c < job.ncorr; ++c) {
        int ia = 0, ib = 0;
        for (int i = 0; i < narr; ++i) { if (arr[i] == job.a[c].z) ia = i; if (arr[i] == job.b[c].z) ib = i; }
        float2 A = spec_of(job.a[c].part, zk[ia], zm[ia]);
        float2 B = spec_of(job.b[c].part, zk[ib], zm[ib]);
        float2 C = cross_power_bin(A, B, real_bin, edge_col);
        if (c == 0) { y.x += C.x; y.y += C.y; ym.x += C.x; ym.y -= C.y; }        // Y = C1 + i C2
        else { y.x -= C.y; y.y += C.x; ym.x += C.y; ym.y += C.x; }               // i*conj(C2) = (C2.y, C2.x)
    }
    out[r1 + px] = y;
    if (r1 != r2) out[r2 + px2] = ym;
}

// ---- line-pair helpers of the row-stage kernels -------------------------------------------------------------------
//
// A row-stage workgroup moves the spectrum lines ky and -ky of an N-point array together: NT lanes, 16 bytes (two
// points) per lane and line -- half the vector-memory and LDS instructions of 8-byte accesses, whose operand traffic
// shares the SIMD-to-LDS path with the stages' ds_writes.  Piece q = tid + it * NT holds the points 2q and 2q + 1; the
// loop over `it` stays with the caller, and b0 is the index of the buffer's first 16-byte element in buf4.
// A kernel uses a helper only where it compiles to the instructions of the text it replaces (compare the assembly
// before adopting one elsewhere): these kernels sit at their register limits, and the same statements reached through
// another inlining order have come out with other register assignments, and with spills.

// piece q of the lines at element offsets e1 and e2 of z into registers (a prefetch: nothing here waits for the loads)
template <int N>
__device__ __forceinline__ void line_pair_fetch(float4 &la, float4 &lb, const float2 *z, long e1, long e2, int q)
{
    // lanes past the end of the line re-read its last pair (never committed): a select on
    // the loaded value would need the load to have completed -- a wait inside the prefetch
    q = q < N / 2 ? q : N / 2 - 1;
    la = *reinterpret_cast<const float4 *>(z + e1 + 2 * q);
    lb = *reinterpret_cast<const float4 *>(z + e2 + 2 * q);
}

// the fetched piece q into a two-line LDS buffer
template <int N>
__device__ __forceinline__ void line_pair_commit(float4 *buf4, int b0, float4 la, float4 lb, int q)
{
    if (q < N / 2) {
        // [point][line] interleave: (2q, line 0), (2q, line 1), (2q+1, line 0), (2q+1, line 1):
        // two 16-byte writes 32 bytes apart per lane (2-way bank conflict; four 8-byte writes
        // would be 4-way).  The repacking moves sit here, after the loads have landed.
        buf4[b0 + 2 * q] = make_float4(la.x, la.y, lb.x, lb.y);
        buf4[b0 + 2 * q + 1] = make_float4(la.z, la.w, lb.z, lb.w);
    }
}

// piece q of a two-line LDS buffer holding forward(conj(Y)) into registers as Y: ya = line ky, yb = line -ky
template <int N>
__device__ __forceinline__ void line_pair_read_conj(float4 &ya, float4 &yb, const float4 *buf4, int b0, int q)
{
    if (q < N / 2) {
        const float4 u = buf4[b0 + 2 * q], v = buf4[b0 + 2 * q + 1];
        ya = make_float4(u.x, -u.y, v.x, -v.y);
        yb = make_float4(u.z, -u.w, v.z, -v.w);
    }
}

// piece q of the result lines to element offsets e1 and e2 of out; line -ky only where it is another line (pair)
template <int N>
__device__ __forceinline__ void line_pair_store(float2 *out, long e1, long e2, bool pair, float4 ya, float4 yb, int q)
{
    if (q < N / 2) {
        *reinterpret_cast<float4 *>(out + e1 + 2 * q) = ya;
        if (pair) *reinterpret_cast<float4 *>(out + e2 + 2 * q) = yb;
    }
}

// What the fused row stage reads of a cross-power job: the packed spectra (one, or three), the outputs (one, or two),
// and for the three-spectra shape which slot of z[2] the last correlation takes (xpower_stage checks the rest of the
// shape on the host)
struct FusedJob {
    const float2 *z[3];
    float2 *out[2];
    int last_part;                      // 0: real slot, 1: imaginary slot
};

// Row stage of the whole correlation in one persistent kernel, for shapes whose row axis is a single
// factor (natural order along x).  The spectra arrive with only their column passes done.  A
// workgroup owns the lines ky and -ky of every spectrum of the job, each spectrum in its own
// two-line LDS buffer:
//   1. the prefetched lines (registers) go to LDS; the loads of the workgroup's NEXT line pair are
//      issued and stay in flight under everything below;
//   2. forward row transform of all spectra together (one barrier pair per stage);
//   3. cross-power in place: the thread of column kx is the only reader of bins (kx, ky) and
//      (-kx, -ky), so Y_o(kx, ky) / Y_o(-kx, -ky) overwrite them in buffer o;
//   4. inverse row transform of the outputs together; both lines of each output are stored.
// Against separate passes this saves a read + write of every spectrum (forward rows), a write +
// read of every Y (cross-power) and the re-read of spectra shared by two outputs; one workgroup
// per CU (3 x 48 KB of LDS at F = 3000) hides HBM latency by the register prefetch instead of
// occupancy.
// ALL chooses the stage scheduler: false = oipfft::StagesPipe (one buffer after the other, a barrier pair per stage and
// buffer, pipelined), true = oipfft::StagesAll (every stage dealt over all buffers at once; see kFusedRow).
template <bool ALL, int F, int NT, int NA, int... Rs>
__device__ __forceinline__ void row_stages(float2 *buf, const float2 *tw, int tid)
{
    if constexpr (ALL) oipfft::StagesAll<F, NT, NA, 1, Rs...>::run(buf, tw, tid);
    else oipfft::StagesPipe<F, NT, NA, 1, Rs...>::run(buf, tw, tid);
}
template <int F, int NT, int NARR, int NOUT, bool ALL, int... Rs>
__global__ __launch_bounds__(NT) void corr_rows_kernel(FusedJob fj, int M, int P, const int *__restrict__ ypos,
                                                       const float2 *__restrict__ twF)
{
    constexpr int TWN = oipfft::TwTable<F, Rs...>::value();
    constexpr int N = F;
    constexpr int NIT = (N + NT - 1) / NT;
    __shared__ __align__(16) float2 buf[NARR * 2 * F];   // [spectrum][point][line]: line 0 = ky, line 1 = -ky
    __shared__ float2 tw[TWN];
    const int half = M / 2;
    int ky = blockIdx.x;
    if (ky > half) return;
    for (int i = threadIdx.x; i < TWN; i += NT) tw[i] = twF[i];
    constexpr int NIT2 = (N / 2 + NT - 1) / NT;
    float4 la[NARR][NIT2], lb[NARR][NIT2];
    float4 *buf4 = reinterpret_cast<float4 *>(buf);
    // rows of the line pair whose loads are in la/lb (n1, n2) and of the pair in LDS (s1, s2)
    // (row positions come from a per-plan table: decoding them with the digit loop cost ~300 scalar
    // instructions and four dependent scalar loads per iteration, on every wave at the same time)
    long n1 = (long)ypos[ky] * P, n2 = (long)ypos[ky ? M - ky : 0] * P;
    auto fetch = [&](int tid) {
#pragma unroll
        for (int a = 0; a < NARR; ++a) {
#pragma unroll
            for (int it = 0; it < NIT2; ++it) line_pair_fetch<N>(la[a][it], lb[a][it], fj.z[a], n1, n2, tid + it * NT);
        }
    };
    auto commit = [&](int tid) {
#pragma unroll
        for (int a = 0; a < NARR; ++a) {
#pragma unroll
            for (int it = 0; it < NIT2; ++it) line_pair_commit<N>(buf4, a * F, la[a][it], lb[a][it], tid + it * NT);
        }
    };
    fetch(threadIdx.x);
    commit(threadIdx.x);
    long s1 = n1, s2 = n2;
    __syncthreads();
    for (; ky <= half; ky += gridDim.x) {
        // opaque per iteration: keeps the stage address arithmetic from being hoisted out of this
        // loop, where it would occupy registers for the whole kernel
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const bool pair = s1 != s2;
        // The lines of the NEXT pair are requested first and committed at the bottom of this same
        // iteration: the registers holding them then never cross the loop's back edge.  (Carried across
        // it, the register allocator gave the loop-header values other registers than the loads'
        // destinations and copied right after the loads -- waiting for them at the point of issue.)
        const int kn = ky + gridDim.x;
        const bool more = kn <= half;
        if (more) {
            n1 = (long)ypos[kn] * P;
            n2 = (long)ypos[M - kn] * P;
            fetch(tid);
        }
        __builtin_amdgcn_sched_barrier(0);
        row_stages<ALL, F, NT, NARR, Rs...>(buf, tw, tid);
#pragma unroll 1
        for (int it = 0; it < NIT; ++it) {
            const int kx = tid + it * NT;
            if (kx >= N) continue;
            const int nkx = kx ? N - kx : 0;
            const bool edge_col = (kx == 0) || (2 * kx == N);
            const bool real_bin = edge_col && (ky == 0 || 2 * ky == M);
            // The two job shapes are fixed (xpower_stage checks them on the host), so which spectrum and
            // slot feeds which correlation is known here -- no run-time selects:
            //   1 spectrum : Y0 = C(z0.re, z0.im)
            //   3 spectra  : A = z0.re against z0.im, z1.re | z1.im, z2.(re or im: fj.last_part)
            const float2 zk0 = buf[2 * kx], zm0 = buf[2 * nkx + 1];
            const float2 A = spec_of(0, zk0, zm0);
            float2 y0, y0m, y1 = make_float2(0.f, 0.f), y1m = make_float2(0.f, 0.f);
            {
                const float2 C = cross_power_bin_fast(A, spec_of(1, zk0, zm0), real_bin, edge_col);
                y0 = C;
                y0m = make_float2(C.x, -C.y);
            }
            if (NARR == 3) {
                const float2 zk1 = buf[2 * F + 2 * kx], zm1 = buf[2 * F + 2 * nkx + 1];
                const float2 zk2 = buf[4 * F + 2 * kx], zm2 = buf[4 * F + 2 * nkx + 1];
                float2 C = cross_power_bin_fast(A, spec_of(0, zk1, zm1), real_bin, edge_col);
                y0.x -= C.y; y0.y += C.x; y0m.x += C.y; y0m.y += C.x;                        // + i C, + i conj(C)
                C = cross_power_bin_fast(A, spec_of(1, zk1, zm1), real_bin, edge_col);
                y1 = C;
                y1m = make_float2(C.x, -C.y);
                const float2 B3 = fj.last_part ? spec_of(1, zk2, zm2) : spec_of(0, zk2, zm2);
                C = cross_power_bin_fast(A, B3, real_bin, edge_col);
                y1.x -= C.y; y1.y += C.x; y1m.x += C.y; y1m.y += C.x;
            }
            // inverse = conj(forward(conj(.)))
            buf[2 * kx] = make_float2(y0.x, -y0.y);
            buf[2 * nkx + 1] = pair ? make_float2(y0m.x, -y0m.y) : make_float2(0.f, 0.f);
            if (NOUT == 2) {
                buf[2 * F + 2 * kx] = make_float2(y1.x, -y1.y);
                buf[2 * F + 2 * nkx + 1] = pair ? make_float2(y1m.x, -y1m.y) : make_float2(0.f, 0.f);
            }
        }
        __syncthreads();
        asm volatile("" : "+v"(tid));
        row_stages<ALL, F, NT, NOUT, Rs...>(buf, tw, tid);
        // (Looks redundant: StagesPipe<..., NA = 1> already ends on a barrier.  Kept where it has always been -- the
        // pipelined scheduler with one output -- until dropping it has been measured on its own.)
        if (!ALL && NOUT == 1) __syncthreads();
        // Results leave LDS through registers so that the next pair can be committed before the stores
        // are issued.
        // (line_pair_read_conj and line_pair_store written out: through the helpers the three-spectra forms compile to
        // another register assignment in the cross-power loop)
        float4 ya[NOUT][NIT2], yb[NOUT][NIT2];      // line ky / line -ky, two points each
#pragma unroll
        for (int o = 0; o < NOUT; ++o) {
#pragma unroll
            for (int it = 0; it < NIT2; ++it) {
                const int q = tid + it * NT;
                if (q < N / 2) {
                    const float4 u = buf4[o * F + 2 * q], v = buf4[o * F + 2 * q + 1];
                    ya[o][it] = make_float4(u.x, -u.y, v.x, -v.y);
                    yb[o][it] = make_float4(u.z, -u.w, v.z, -v.w);
                }
            }
        }
        __syncthreads();
        if (more) commit(tid);
        __builtin_amdgcn_sched_barrier(0);
        const long o1 = s1, o2 = s2;
        s1 = n1; s2 = n2;
#pragma unroll
        for (int o = 0; o < NOUT; ++o) {
            float2 *out = fj.out[o];
#pragma unroll
            for (int it = 0; it < NIT2; ++it) {
                const int q = tid + it * NT;
                if (q < N / 2) {
                    *reinterpret_cast<float4 *>(out + o1 + 2 * q) = ya[o][it];
                    if (pair) *reinterpret_cast<float4 *>(out + o2 + 2 * q) = yb[o][it];
                }
            }
        }
        __syncthreads();
    }
}

// ---- row stage with the x4 cubic up-sampling of the bands applied to their spectra -------------------------------
//
// cv::resize(INTER_CUBIC) by exactly 4 is linear: along one axis, out = R s with R = C + E, where C is the circulant
// operator "zero-stuff by 4, convolve with the 16-tap kernel h" and E holds what edge replication changes -- it is
// non-zero in the columns of the source samples {0, 1, n-2, n-1} only (the taps that leave the image are clamped to
// sample 0 or n-1 instead of wrapping to n-2, n-1, 0, 1).  So the N = 4n point transform of an up-sampled line is
//     DFT_N(R s)[k] = H[k] DFT_n(s)[k mod n] + sum_j G_j[k] s[J_j],       H = DFT_N(h), G_j = DFT_N(E[:, J_j])
// -- a 750-point transform, one complex multiply and four multiply-adds per bin instead of a 3000-point transform of
// the up-sampled line.  The same holds along the columns (VEXP): the band windows are transformed at their own size
// (4000 x 750) and line ky of the up-sampled band's column transform is Hv[ky] B^[ky mod 4000] + sum_i Gv_i[ky] raw_i.
// Without VEXP (OIP_SPECTRAL_UP=1) the vertical taps are applied in the image domain (resize_cubic_v) and the columns of
// the resulting 16000 x 750 images are transformed.  The identity is exact; what changes against transforming the
// up-sampled image is the rounding (the f32 rounding of every up-sampled pixel is replaced by the rounding of H, G and
// the products), 4e-6 px on the shifts -- the size of the difference between any two float FFTs
// (tests/test_gpu_correlation.py compares the routes with each other and with the oracle, which up-samples first).
//
// One launch serves a pair of units: zp = PAN_A + i PAN_B (full width), four narrow arrays (bands 0|1 and 2|3 of unit
// A, then of unit B) and four outputs Y = C(PAN, band 2a) + i C(PAN, band 2a+1).  LDS holds the PAN line pair, one
// more full-width buffer and the eight narrow lines (144 KB): after the forward transforms the PAN spectra of the
// thread's bins move to registers, and the outputs are formed, inverse-transformed and stored two at a time in the two
// full-width buffers.  A thread owns the same bins of every line pair: kx <= N/2 and N - kx of line ky (and their
// mirrors in line -ky), which share H and G up to conjugation.
struct UpRowsJob {
    const float2 *zp;       // pitch P
    const float2 *zn;       // four narrow arrays, zn_stride elements apart, pitch Pn
    long zn_stride;
    int Pn;
    float2 *out[4];
    const float2 *xtab;     // [5][N]: H, G_0 .. G_3
    int nout;               // 4, or 2 for a single unit (arrays 2 and 3 are not read)
    // VEXP: the vertical up-sampling is applied to the spectra as well.  zn then holds the column transforms of the
    // band windows themselves (m = M / 4 rows): line ky of the up-sampled band is
    //     Hv[ky] zn[ky mod m] + sum_i Gv_i[ky] raw[i],      raw = band rows {0, 1, m-2, m-1}
    const float2 *vtab;     // [5][M]: Hv, Gv_0 .. Gv_3
    const uint2 *raw16;     // [4 rows][4 arrays x n / 2]: (bX | bY << 16) of two neighbouring points
    const int *ypos_s;      // row position of frequency line k in zn, k in [0, m)
    int m;
    // Column bounds for the peak search (col_sel_first_kernel): workgroup g leaves sum |Re| + |Im| of every line it
    // transformed, in column x < N of output o, at bound[(g * 4 + o) * P + x].  A thread owns its columns for the whole
    // launch and sums them in registers, in the order of its line pairs (no sum depends on an order between threads);
    // after its last line pair every workgroup of the grid writes its four rows in full -- zeros for the outputs a single
    // unit does not have -- so nothing has to clear the rows before the launch.
    float *bound;
    // WIN: only the 16-byte pieces q (columns 2 q, 2 q + 1) with q < win_hi or q >= win_lo are stored -- the circular,
    // tile-aligned range of columns around column 0 that the pruned peak search reads (rows_window).  The bounds above
    // are summed over every column all the same.
    int win_hi, win_lo;
};

// conj(a) b, acc + a b, acc + conj(a) b on packed-f32 instructions (two each; operand selection as in oipfft::cmul).
// The spectral operator is part of the transform: multiply-adds fuse (see oip_fft_dev.h).
__device__ __forceinline__ float2 cmulj(float2 a, float2 b)
{
    oipfft::oip_v2f t, r;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]" : "=v"(t) : "v"(oipfft::to_v(a)), "v"(oipfft::to_v(b)));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_hi:[1,0,0]" : "=v"(r) : "v"(oipfft::to_v(a)), "v"(oipfft::to_v(b)), "v"(t));
    return oipfft::to_f2(r);
}
__device__ __forceinline__ float2 cfma(float2 a, float2 b, float2 acc)
{
    oipfft::oip_v2f t, r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(t) : "v"(oipfft::to_v(a)), "v"(oipfft::to_v(b)), "v"(oipfft::to_v(acc)));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0]" : "=v"(r) : "v"(oipfft::to_v(a)), "v"(oipfft::to_v(b)), "v"(t));
    return oipfft::to_f2(r);
}
__device__ __forceinline__ float2 cfmaj(float2 a, float2 b, float2 acc)
{
    oipfft::oip_v2f t, r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(t) : "v"(oipfft::to_v(a)), "v"(oipfft::to_v(b)), "v"(oipfft::to_v(acc)));
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_hi:[1,0,0]" : "=v"(r) : "v"(oipfft::to_v(a)), "v"(oipfft::to_v(b)), "v"(t));
    return oipfft::to_f2(r);
}

// spec_of without its factor 1/2 (the row stage's horizontal tables carry it)
__device__ __forceinline__ float2 spec2_of(int part, float2 zk, float2 zm)
{
    if (part == 0) return make_float2(zk.x + zm.x, zk.y - zm.y);
    return make_float2(zk.y + zm.y, zm.x - zk.x);
}
// acc + s v for a real s (one packed multiply-add)
__device__ __forceinline__ float2 sfma(float s, float2 v, float2 acc)
{
    OIP_FFT_FMA
    return make_float2(acc.x + s * v.x, acc.y + s * v.y);
}

// the value of lane ^ 1 (DPP quad_perm [1, 0, 3, 2]: no LDS traffic); both lanes of the pair must be active
__device__ __forceinline__ float quad_swap1(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));
}

template <int NT, bool VEXP, bool WIN>
__global__ __launch_bounds__(NT) void corr_rows_up_kernel(UpRowsJob fj, int M, int P, const int *__restrict__ ypos,
                                                          const float2 *__restrict__ twF, const float2 *__restrict__ twS)
{
    constexpr int F = kUpRowsN, S = kUpRowsBandN;
    constexpr int TWF = oipfft::TwTable<F, 25, 15, 8>::value(), TWS = oipfft::TwTable<S, 25, 15, 2>::value();
    // A thread owns the bins kx = tid + NT r <= N/2 of line ky and their mirrors N - kx of the same line: H and G are
    // transforms of real sequences, so the mirror's table values are the conjugates -- half the table registers.
    constexpr int NB = (F / 2 + 1 + NT - 1) / NT;
    constexpr int WE = (F / 2) % NT / 64;           // the wave that owns bin N/2 (bin 0 is wave 0's)
    static_assert(WE != 0, "the two edge columns are evaluated by two waves");
    __shared__ __align__(16) float2 buf[2 * 2 * F + 4 * 2 * S];    // PAN / output 0 | output 1 | narrow arrays; [point][line]
    __shared__ float2 tw[TWF], tws[TWS];
    __shared__ float2 edge[4][2][4];                               // [array][line][j]: narrow line samples 0, 1, S-2, S-1
    __shared__ float2 edgeA[2][2];                                 // PAN spectra (unit A, unit B) at kx = 0 and N/2
    __shared__ float2 edgeT[2][5];                                 // H, G_0..3 at kx = 0 and N/2
    float2 *bufN = buf + 4 * F;
    float4 *buf4 = reinterpret_cast<float4 *>(buf), *buf4N = reinterpret_cast<float4 *>(bufN);
    const int half = M / 2;
    int ky = blockIdx.x;
    constexpr int NIT2 = (F / 2 + NT - 1) / NT;
    // Column bounds (UpRowsJob::bound): sum |Re| + |Im| of this thread's columns over the workgroup's line pairs, [output]
    // [piece]: 24 registers for the whole launch.  (They fit since the read-out below stores and sums a piece as it leaves
    // LDS: the 48 registers that held a whole round's results between the transform and the stores are gone.)
    float2 acc[4][NIT2];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
#pragma unroll
        for (int it = 0; it < NIT2; ++it) acc[o][it] = make_float2(0.f, 0.f);
    }
    // the workgroup's four rows, written once (plain 8-byte stores: the pitch of every plan is a multiple of 16 elements);
    // a workgroup without a line pair leaves zeros
    auto write_bounds = [&]() {
        float *brow = fj.bound + (long)blockIdx.x * 4 * P;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
#pragma unroll
            for (int it = 0; it < NIT2; ++it) {
                const int q = threadIdx.x + it * NT;
                if (q < F / 2) *reinterpret_cast<float2 *>(brow + o * P + 2 * q) = acc[o][it];
            }
        }
    };
    if (ky > half) { write_bounds(); return; }
    for (int i = threadIdx.x; i < TWF; i += NT) tw[i] = twF[i];
    for (int i = threadIdx.x; i < TWS; i += NT) tws[i] = twS[i];
    if (threadIdx.x < 10) edgeT[threadIdx.x / 5][threadIdx.x % 5] = fj.xtab[(threadIdx.x % 5) * F + (threadIdx.x / 5) * (F / 2)];
    // H and G of the thread's bins (30 registers): read once, before the first line pair, and held for the whole launch.
    // (They used to be re-read from L2 for each of the two cross-power rounds, when the results of a round waited in 48
    // registers for their stores; see the read-out in finish().)
    float2 H[NB], G[NB][4];
    auto load_tables = [&](int tid) {
#pragma unroll
        for (int r = 0; r < NB; ++r) {
            int kx = tid + NT * r;
            kx = kx <= F / 2 ? kx : 0;
            H[r] = fj.xtab[kx];
#pragma unroll
            for (int j = 0; j < 4; ++j) G[r][j] = fj.xtab[(1 + j) * F + kx];
        }
    };
    constexpr int NQ = 4 * (S / 2);                 // 16-byte pieces of one line of the four narrow arrays
    constexpr int NITN = (NQ + NT - 1) / NT;
    float4 la[NIT2], lb[NIT2], na[NITN], nb[NITN];
    long n1 = ypos[ky], n2 = ypos[ky ? M - ky : 0];     // rows (the pitches differ between zp and zn)
    // rows of the narrow arrays: the same lines, or (VEXP) the lines ky mod m and -ky mod m of the band transforms
    auto narrow_row = [&](int k, long full) { return VEXP ? (long)fj.ypos_s[k % fj.m] : full; };
    long m1 = narrow_row(ky, n1), m2 = narrow_row(ky ? M - ky : 0, n2);
    int kyc = ky;                                       // the frequency line whose loads are in the registers
    float2 vt[5];                                       // VEXP: Hv, Gv_0..3 of line kyc
    uint2 rawreg[NITN][4];                              // VEXP: the raw band rows at this thread's points (bX | bY << 16, two points)
    // VEXP: the narrow lines, their coefficients and the raw rows are requested at the commit itself -- their
    // registers (58 per thread) held across the second round's transforms spill, and a spilled load is waited for
    // where it is issued.  They are a quarter of the input bytes and mostly L2 / Infinity Cache hits (every line of
    // a band transform serves four frequency lines, the raw rows serve all).  (With the tables held for the launch the
    // lines and coefficients requested with the prefetch, or the raw rows held for the launch, spill again; either of
    // them without the held tables fits and does not do as well as the tables: DESIGN.md 4.3.)
    auto fetch_narrow = [&](int tid) {
        if (VEXP) {
#pragma unroll
            for (int r = 0; r < 5; ++r) vt[r] = fj.vtab[r * M + kyc];
#pragma unroll
            for (int it = 0; it < NITN; ++it) {
                int q = tid + it * NT;
                q = q < NQ ? q : NQ - 1;
#pragma unroll
                for (int r = 0; r < 4; ++r) rawreg[it][r] = fj.raw16[(long)r * NQ + q];
            }
        }
#pragma unroll
        for (int it = 0; it < NITN; ++it) {
            int q = tid + it * NT;
            q = q < NQ ? q : NQ - 1;
            const int a = q / (S / 2), i = q - a * (S / 2);
            const float2 *z = fj.zn + a * fj.zn_stride + 2 * i;
            na[it] = *reinterpret_cast<const float4 *>(z + m1 * fj.Pn);
            nb[it] = *reinterpret_cast<const float4 *>(z + m2 * fj.Pn);
        }
    };
    auto fetch = [&](int tid) {
        // (line_pair_fetch written out: with the helper the loads are scheduled differently in this kernel)
#pragma unroll
        for (int it = 0; it < NIT2; ++it) {
            int q = tid + it * NT;
            q = q < F / 2 ? q : F / 2 - 1;
            la[it] = *reinterpret_cast<const float4 *>(fj.zp + n1 * P + 2 * q);
            lb[it] = *reinterpret_cast<const float4 *>(fj.zp + n2 * P + 2 * q);
        }
        if (!VEXP) fetch_narrow(tid);
    };
    auto commit = [&](int tid) {
        if (VEXP) fetch_narrow(tid);
#pragma unroll
        for (int it = 0; it < NIT2; ++it) line_pair_commit<F>(buf4, 0, la[it], lb[it], tid + it * NT);
#pragma unroll
        for (int it = 0; it < NITN; ++it) {
            const int q = tid + it * NT;
            if (q < NQ) {
                const int a = q / (S / 2), i = q - a * (S / 2);
                if (VEXP) {
                    // line ky of the vertically up-sampled band pair from line ky mod m of its transform; Hv and Gv of
                    // line -ky are the conjugates.  The raw band rows of this thread's points are kernel-long
                    // constants (two u16 pairs per row and piece).
                    const float2 hv = vt[0];
                    float2 x0 = oipfft::cmul(hv, make_float2(na[it].x, na[it].y)), x1 = oipfft::cmul(hv, make_float2(na[it].z, na[it].w));
                    float2 y0 = cmulj(hv, make_float2(nb[it].x, nb[it].y)), y1 = cmulj(hv, make_float2(nb[it].z, nb[it].w));
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float2 gv = vt[1 + r];
                        const uint2 u = rawreg[it][r];
                        const float2 w0 = make_float2((float)(u.x & 0xffffu), (float)(u.x >> 16)), w1 = make_float2((float)(u.y & 0xffffu), (float)(u.y >> 16));
                        x0 = cfma(gv, w0, x0); x1 = cfma(gv, w1, x1);
                        y0 = cfmaj(gv, w0, y0); y1 = cfmaj(gv, w1, y1);
                    }
                    na[it] = make_float4(x0.x, x0.y, x1.x, x1.y);
                    nb[it] = make_float4(y0.x, y0.y, y1.x, y1.y);
                }
                buf4N[a * S + 2 * i] = make_float4(na[it].x, na[it].y, nb[it].x, nb[it].y);
                buf4N[a * S + 2 * i + 1] = make_float4(na[it].z, na[it].w, nb[it].z, nb[it].w);
                if (i == 0 || i == S / 2 - 1) {
                    const int j = i ? 2 : 0;
                    edge[a][0][j] = make_float2(na[it].x, na[it].y); edge[a][0][j + 1] = make_float2(na[it].z, na[it].w);
                    edge[a][1][j] = make_float2(nb[it].x, nb[it].y); edge[a][1][j + 1] = make_float2(nb[it].z, nb[it].w);
                }
            }
        }
    };
    fetch(threadIdx.x);
    commit(threadIdx.x);
    long s1 = n1, s2 = n2;
    __syncthreads();
    load_tables(threadIdx.x);
    for (; ky <= half; ky += gridDim.x) {
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const bool pair = s1 != s2;
        const int kn = ky + gridDim.x;
        const bool more = kn <= half;
        __builtin_amdgcn_sched_barrier(0);
        oipfft::StagesDual3<F, 1, S, 4, NT, 25, 15, 8, 2>::run(buf, tw, bufN, tws, tid);
        // PAN spectra of this thread's bins (unit A in the real slot, unit B in the imaginary one); those of the two
        // edge columns (kx = 0, N/2: divSpectrums' double-precision and real-only formulas) also go to edgeA
        float2 Aa[2 * NB], Ab[2 * NB];                  // [2 r]: bin kx, [2 r + 1]: bin N - kx
#pragma unroll
        for (int r = 0; r < NB; ++r) {
            const int kx = tid + NT * r, nkx = kx ? F - kx : 0;
            if (kx <= F / 2) {
                const float2 zk = buf[2 * kx], zm = buf[2 * nkx + 1];
                Aa[2 * r] = spec_of(0, zk, zm);
                Ab[2 * r] = spec_of(1, zk, zm);
                const float2 zk2 = buf[2 * nkx], zm2 = buf[2 * kx + 1];
                Aa[2 * r + 1] = spec_of(0, zk2, zm2);
                Ab[2 * r + 1] = spec_of(1, zk2, zm2);
                if (kx == 0 || 2 * kx == F) { edgeA[kx ? 1 : 0][0] = Aa[2 * r]; edgeA[kx ? 1 : 0][1] = Ab[2 * r]; }
            }
        }
        // outputs o0, o0 + 1 (narrow arrays of the same index) into the two full-width buffers
        auto xround = [&](int o0, const float2 (&A)[2 * NB]) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float2 *zn = bufN + (o0 + h) * 2 * S;
                float2 e0[4], e1[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) { e0[j] = edge[o0 + h][0][j]; e1[j] = edge[o0 + h][1][j]; }
                float2 *ob = buf + h * 2 * F;
#pragma unroll
                for (int r = 0; r < NB; ++r) {
                    const int kx = tid + NT * r, nkx = kx ? F - kx : 0;
                    if (kx > F / 2) continue;
                    const int c = kx % S, cm = c ? S - c : 0;      // the narrow bin of kx and of -kx
                    // sum_j G_j e_j = S + i T and sum_j conj(G_j) e_j = S - i T with S = sum Re(G_j) e_j, T = sum Im(G_j) e_j:
                    // bin kx and its mirror N - kx (conjugate table values) share the products, line by line
                    float2 S0 = make_float2(0.f, 0.f), T0 = S0, S1 = S0, T1 = S0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        S0 = sfma(G[r][j].x, e0[j], S0); T0 = sfma(G[r][j].y, e0[j], T0);
                        S1 = sfma(G[r][j].x, e1[j], S1); T1 = sfma(G[r][j].y, e1[j], T1);
                    }
                    {
                        // packed band spectrum at (ky, kx) and at (-ky, -kx): H and G of -kx are the conjugates
                        const float2 Z0 = oipfft::csub_rot(oipfft::cadd(oipfft::cmul(H[r], zn[2 * c]), S0), T0);          // + S0 + i T0
                        const float2 Z1 = oipfft::cadd_rot(oipfft::cadd(cmulj(H[r], zn[2 * cm + 1]), S1), T1);            // + S1 - i T1
                        const float2 C1 = cross_power_bin_fast(A[2 * r], spec2_of(0, Z0, Z1), false, false);
                        const float2 C2 = cross_power_bin_fast(A[2 * r], spec2_of(1, Z0, Z1), false, false);
                        // Y = C1 + i C2 at the bin, conj(C1) + i conj(C2) at its mirror; inverse = conj(forward(conj(.)))
                        ob[2 * kx] = make_float2(C1.x - C2.y, -(C1.y + C2.x));
                        ob[2 * nkx + 1] = pair ? make_float2(C1.x + C2.y, -(C2.x - C1.y)) : make_float2(0.f, 0.f);
                    }
                    if (kx != 0 && 2 * kx != F) {
                        // the same for bin (ky, N - kx) and its mirror (-ky, kx)
                        const float2 Z0 = oipfft::cadd_rot(oipfft::cadd(cmulj(H[r], zn[2 * cm]), S0), T0);                // + S0 - i T0
                        const float2 Z1 = oipfft::csub_rot(oipfft::cadd(oipfft::cmul(H[r], zn[2 * c + 1]), S1), T1);      // + S1 + i T1
                        const float2 C1 = cross_power_bin_fast(A[2 * r + 1], spec2_of(0, Z0, Z1), false, false);
                        const float2 C2 = cross_power_bin_fast(A[2 * r + 1], spec2_of(1, Z0, Z1), false, false);
                        ob[2 * nkx] = make_float2(C1.x - C2.y, -(C1.y + C2.x));
                        ob[2 * kx + 1] = pair ? make_float2(C1.x + C2.y, -(C2.x - C1.y)) : make_float2(0.f, 0.f);
                    }
                    // one bin pair at a time (keeps the LDS reads of all bins from being hoisted above the arithmetic)
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            // The two edge columns again with their own formulas.  The four evaluations of a round -- (h, C1 | C2) -- are
            // independent chains of double-precision divisions and a square root: each takes one of the first four lanes
            // of the wave that owns the column, side by side (in series in the owning lane they were more f64 work than
            // both main loops, with the rest of the workgroup waiting at finish()'s barrier).  That wave wrote edgeA and
            // the bins these lanes overwrite itself: the LDS accesses of one wave complete in order, so a wave-level
            // fence for the compiler is enough and no barrier is added.  The test is wave-uniform: the other six waves
            // branch over the block.
            const int wv = __builtin_amdgcn_readfirstlane(tid) >> 6;
            if (wv == 0 || wv == WE) {
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                const int ec = wv ? 1 : 0, kx = ec * (F / 2), lane = tid & 63;
                if (lane < 4) {
                    const int h = lane >> 1, part = lane & 1;
                    const bool real_bin = ky == 0 || 2 * ky == M;
                    const float2 Ae = edgeA[ec][o0 ? 1 : 0];
                    // (from LDS: a vector-memory load here would be younger than the prefetch and wait for it)
                    const float2 He = edgeT[ec][0];
                    const float2 *zn = bufN + (o0 + h) * 2 * S;
                    float2 Z0 = oipfft::cmul(He, zn[0]), Z1 = cmulj(He, zn[1]);       // kx = 0 and N/2 both map to narrow bin 0
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float2 Ge = edgeT[ec][1 + j];
                        Z0 = cfma(Ge, edge[o0 + h][0][j], Z0); Z1 = cfmaj(Ge, edge[o0 + h][1][j], Z1);
                    }
                    const float2 C = cross_power_bin(Ae, spec2_of(part, Z0, Z1), real_bin, true);
                    const float2 D = make_float2(quad_swap1(C.x), quad_swap1(C.y));    // the neighbour's: C2 for C1, C1 for C2
                    const float2 C1 = part ? D : C, C2 = part ? C : D;
                    float2 *ob = buf + h * 2 * F;
                    if (part == 0) ob[2 * kx] = make_float2(C1.x - C2.y, -(C1.y + C2.x));
                    else ob[2 * kx + 1] = pair ? make_float2(C1.x + C2.y, -(C2.x - C1.y)) : make_float2(0.f, 0.f);   // -kx == kx here
                }
            }
        };
        // Inverse row transform of the two buffers and the read-out: a piece leaves LDS, is stored if it lies in the window
        // (WIN: compared here, from the piece index -- wave-uniform but at the window's two ends; nothing is carried across
        // the iteration) and |Re| + |Im| of it is added to the thread's column bounds.  An unpaired line (ky = 0, M / 2)
        // counts once.  The order of the additions is the order of the line pairs: the sums are the same bits every run.
        auto finish = [&](int o0) {
            __syncthreads();
            asm volatile("" : "+v"(tid));
            oipfft::StagesAll<F, NT, 2, 1, 25, 15, 8>::run(buf, tw, tid);
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                float2 *out = fj.out[o0 + o];
#pragma unroll
                for (int it = 0; it < NIT2; ++it) {
                    const int q = tid + it * NT;
                    if (q < F / 2) {
                        float4 a, b;
                        line_pair_read_conj<F>(a, b, buf4, o * F, q);
                        if (!WIN || q < fj.win_hi || q >= fj.win_lo) line_pair_store<F>(out, s1 * P, s2 * P, pair, a, b, q);
                        float2 s = make_float2(fabsf(a.x) + fabsf(a.y), fabsf(a.z) + fabsf(a.w));
                        if (pair) { s.x += fabsf(b.x) + fabsf(b.y); s.y += fabsf(b.z) + fabsf(b.w); }
                        acc[o0 + o][it].x += s.x;
                        acc[o0 + o][it].y += s.y;
                    }
                }
            }
            __syncthreads();
        };
        xround(0, Aa);
        finish(0);
        __builtin_amdgcn_sched_barrier(0);
        if (fj.nout == 4) xround(2, Ab);
        __builtin_amdgcn_sched_barrier(0);
        // The lines of the NEXT pair are requested here -- after the last consumer of anything the compiler may have
        // spilled (a reload is a vector-memory load: younger than the prefetch, it would wait for it) -- and committed at
        // the bottom of this same iteration: three quarters of the iteration run without their registers.
        if (more) {
            // (scalar loads: as vector loads these look-ups put an s_waitcnt vmcnt(0) -- the stores of the first read-out
            // -- in front of the prefetch.  ABAB on one box: 1.1677 / 1.1696 -> 1.1509 / 1.1427 ms per launch)
            n1 = oip_sload_i32(ypos, kn);
            n2 = oip_sload_i32(ypos, M - kn);
            m1 = VEXP ? (long)oip_sload_i32(fj.ypos_s, kn % fj.m) : n1;
            m2 = VEXP ? (long)oip_sload_i32(fj.ypos_s, (M - kn) % fj.m) : n2;
            kyc = kn;
            fetch(tid);
        }
        __builtin_amdgcn_sched_barrier(0);
        if (fj.nout == 4) finish(2);
        if (more) commit(tid);
        s1 = n1; s2 = n2;
        __syncthreads();
    }
    write_bounds();
}

// ---- row stage with the VERTICAL x4 up-sampling applied to the band spectra (padded row lengths) ---------------------
//
// The reference's own strips are 12288 pixels wide: ten slices of 1228 columns, band windows of 307, and
// cv::phaseCorrelate pads the 1228-column images to 1250 (preproc.h:302-316).  1250 is not four times anything the
// band window has, so the horizontal taps stay in the image domain -- but 16000 = 4 x 4000 still holds on the vertical
// axis: cv::resize interpolates horizontally first (f32, reproduced exactly by hpack_bands_kernel on the 4000 band
// rows), and the vertical operator V = C + E acts on those rows, so along a column
//     DFT_M(V h)[ky] = Hv[ky] DFT_m(h)[ky mod m] + sum_i Gv_i[ky] h[J_i],       J = {0, 1, m-2, m-1}
// exactly (corr_rows_up_kernel, VEXP).  The horizontally up-sampled bands of a pair of units are transformed at
// their own height (four arrays bX + i bY side by side, m x 4N) and line ky of an up-sampled band's column transform
// is rebuilt on the way into LDS.  Against the image-domain route a pair of units costs 2 array-sized forward column
// transforms instead of 5, no vertical up-sampling kernel and one row-stage launch (5 spectra in, 4 out) instead of two
// (3 in, 2 out each).
//
// LDS: five two-line buffers [PAN_A + i PAN_B | array 0 .. 3]; output o = C(PAN_u, band 2a) + i C(PAN_u, band 2a+1)
// (arrays 0, 1: unit A = real slot of the PAN buffer; arrays 2, 3: unit B) overwrites array o's buffer in place -- the
// thread of column kx is the only reader of bins (kx, ky) and (-kx, -ky).
struct VRowsJob {
    const float2 *zp;       // pitch P
    const float2 *zn;       // m rows x four arrays, zn_stride elements apart, pitch Pn (column transforms done)
    long zn_stride;
    int Pn;
    float2 *out[4];
    int nout;               // 4, or 2 for a single unit (arrays 2 and 3 are neither read nor written)
    const float2 *vtab;     // [5][M]: Hv, Gv_0 .. Gv_3
    const float2 *raw;      // [4 rows][4 arrays][zn_stride]: (bX, bY) of the horizontally up-sampled band rows {0, 1, m-2, m-1}
    const int *ypos_s;      // row position of frequency line k in zn, k in [0, m)
    int m;
};

template <int F, int NT, int... Rs>
__global__ __launch_bounds__(NT, 2 * NT / 256) void corr_rows_v_kernel(VRowsJob fj, int a0, int part, int M, int P, const int *__restrict__ ypos,
                                                                      const float2 *__restrict__ twF)
{
    // One launch serves ONE unit: its PAN image (slot `part` of the packed PAN buffer) against band arrays a0, a0 + 1.
    // Three two-line buffers = 60 KB of LDS and <= 128 VGPRs, so two workgroups share a CU: one computes while the other
    // waits at a barrier or for its lines.  (All four arrays of a pair in one workgroup -- 105 KB, one workgroup per CU --
    // was measured first: 0.96 ms per pair against 2 x 0.33 ms for two launches of the image-domain kernel of this shape.)
    constexpr int TWN = oipfft::TwTable<F, Rs...>::value();
    constexpr int N = F, NARR = 3, NB = 2;
    constexpr int NIT = (N + NT - 1) / NT;
    static_assert(N % 2 == 0, "two points per lane");
    constexpr int NIT2 = (N / 2 + NT - 1) / NT;
    constexpr int NQ = NB * (N / 2);                // 16-byte pieces of one line of the two band arrays
    constexpr int NITN = (NQ + NT - 1) / NT;
    __shared__ __align__(16) float2 buf[NARR * 2 * F];   // [PAN | array a0 | array a0 + 1][point][line]: line 0 = ky, line 1 = -ky
    __shared__ float2 tw[TWN];
    float4 *buf4 = reinterpret_cast<float4 *>(buf);
    const int half = M / 2;
    int ky = blockIdx.x;
    if (ky > half) return;
    for (int i = threadIdx.x; i < TWN; i += NT) tw[i] = twF[i];
    float4 la[NIT2], lb[NIT2], na[NITN], nb[NITN];
    float2 vt[5];
    long n1 = ypos[ky], n2 = ypos[ky ? M - ky : 0];
    long m1 = fj.ypos_s[ky % fj.m], m2 = fj.ypos_s[(ky ? M - ky : 0) % fj.m];
    int kyc = ky;                                   // the frequency line whose loads are in the registers
    const float2 *zn = fj.zn + (long)a0 * fj.zn_stride;
    const float2 *raw = fj.raw + (long)a0 * fj.zn_stride;
    auto fetch = [&](int tid) {                     // the PAN line pair, the band lines and their coefficients: one iteration ahead
        // (line_pair_fetch written out: with the helper the loads are scheduled differently in this kernel)
#pragma unroll
        for (int it = 0; it < NIT2; ++it) {
            int q = tid + it * NT;
            q = q < N / 2 ? q : N / 2 - 1;
            la[it] = *reinterpret_cast<const float4 *>(fj.zp + n1 * P + 2 * q);
            lb[it] = *reinterpret_cast<const float4 *>(fj.zp + n2 * P + 2 * q);
        }
#pragma unroll
        for (int it = 0; it < NITN; ++it) {
            int q = tid + it * NT;
            q = q < NQ ? q : NQ - 1;
            const int a = q / (N / 2), i = q - a * (N / 2);
            const float2 *z = zn + a * fj.zn_stride + 2 * i;
            na[it] = *reinterpret_cast<const float4 *>(z + m1 * fj.Pn);
            nb[it] = *reinterpret_cast<const float4 *>(z + m2 * fj.Pn);
        }
#pragma unroll
        for (int r = 0; r < 5; ++r) vt[r] = fj.vtab[r * M + kyc];
    };
    auto commit = [&](int tid) {
#pragma unroll
        for (int it = 0; it < NIT2; ++it) line_pair_commit<N>(buf4, 0, la[it], lb[it], tid + it * NT);
        // line ky of the vertically up-sampled band pair: Hv[ky] zn[ky mod m] + sum_i Gv_i[ky] raw_i; Hv and Gv of line
        // -ky are the conjugates.  The raw rows (160 KB for a pair of units: L2 hits) are read here, not held.
        // (The same sum as in corr_rows_up_kernel's commit.  One function for both, fed the four raw rows as float2,
        // was tried: it gathers the raw loads ahead of the multiply-adds and this kernel then spills 16 VGPRs.)
#pragma unroll
        for (int it = 0; it < NITN; ++it) {
            const int q = tid + it * NT;
            if (q >= NQ) continue;
            const int a = q / (N / 2), i = q - a * (N / 2);
            const float2 hv = vt[0];
            float2 x0 = oipfft::cmul(hv, make_float2(na[it].x, na[it].y)), x1 = oipfft::cmul(hv, make_float2(na[it].z, na[it].w));
            float2 y0 = cmulj(hv, make_float2(nb[it].x, nb[it].y)), y1 = cmulj(hv, make_float2(nb[it].z, nb[it].w));
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float4 rw = *reinterpret_cast<const float4 *>(raw + ((long)r * 4 + a) * fj.zn_stride + 2 * i);
                const float2 gv = vt[1 + r];
                const float2 w0 = make_float2(rw.x, rw.y), w1 = make_float2(rw.z, rw.w);
                x0 = cfma(gv, w0, x0); x1 = cfma(gv, w1, x1);
                y0 = cfmaj(gv, w0, y0); y1 = cfmaj(gv, w1, y1);
            }
            buf4[(1 + a) * F + 2 * i] = make_float4(x0.x, x0.y, y0.x, y0.y);
            buf4[(1 + a) * F + 2 * i + 1] = make_float4(x1.x, x1.y, y1.x, y1.y);
        }
    };
    fetch(threadIdx.x);
    commit(threadIdx.x);
    long s1 = n1, s2 = n2;
    __syncthreads();
    for (; ky <= half; ky += gridDim.x) {
        int tid = threadIdx.x;
        asm volatile("" : "+v"(tid));               // per-iteration opaque copy: no stage addressing hoisted out of the loop
        const bool pair = s1 != s2;
        const int kn = ky + gridDim.x;
        const bool more = kn <= half;
        if (more) {
            // (plain loads here: this kernel requests its next lines at the TOP of the iteration, nothing of its own is in
            // flight yet, and the explicit scalar loads of corr_rows_up_kernel cost it 4.5 % -- 0.740 against 0.708 ms)
            n1 = ypos[kn];
            n2 = ypos[M - kn];
            m1 = fj.ypos_s[kn % fj.m];
            m2 = fj.ypos_s[(M - kn) % fj.m];
            kyc = kn;
            fetch(tid);
        }
        __builtin_amdgcn_sched_barrier(0);
        oipfft::StagesPipe<F, NT, NARR, 1, Rs...>::run(buf, tw, tid);
#pragma unroll 1
        for (int it = 0; it < NIT; ++it) {
            const int kx = tid + it * NT;
            if (kx >= N) continue;
            const int nkx = kx ? N - kx : 0;
            const bool edge_col = (kx == 0) || (2 * kx == N);
            const bool real_bin = edge_col && (ky == 0 || 2 * ky == M);
            const float2 A = spec_of(part, buf[2 * kx], buf[2 * nkx + 1]);
#pragma unroll
            for (int a = 0; a < NB; ++a) {
                float2 *b = buf + (1 + a) * 2 * F;
                const float2 zk = b[2 * kx], zm = b[2 * nkx + 1];
                const float2 C1 = cross_power_bin_fast(A, spec_of(0, zk, zm), real_bin, edge_col);
                const float2 C2 = cross_power_bin_fast(A, spec_of(1, zk, zm), real_bin, edge_col);
                // Y = C1 + i C2 at the bin, conj(C1) + i conj(C2) at its mirror; inverse = conj(forward(conj(.)))
                b[2 * kx] = make_float2(C1.x - C2.y, -(C1.y + C2.x));
                b[2 * nkx + 1] = pair ? make_float2(C1.x + C2.y, -(C2.x - C1.y)) : make_float2(0.f, 0.f);
            }
        }
        __syncthreads();
        asm volatile("" : "+v"(tid));
        oipfft::StagesPipe<F, NT, NB, 1, Rs...>::run(buf + 2 * F, tw, tid);
        float4 ya[NB][NIT2], yb[NB][NIT2];          // line ky / line -ky, two points each
#pragma unroll
        for (int o = 0; o < NB; ++o) {
#pragma unroll
            for (int it = 0; it < NIT2; ++it) line_pair_read_conj<N>(ya[o][it], yb[o][it], buf4, (1 + o) * F, tid + it * NT);
        }
        __syncthreads();
        if (more) commit(tid);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int o = 0; o < NB; ++o) {
            float2 *out = fj.out[a0 + o];
#pragma unroll
            for (int it = 0; it < NIT2; ++it) line_pair_store<N>(out, s1 * P, s2 * P, pair, ya[o][it], yb[o][it], tid + it * NT);
        }
        s1 = n1; s2 = n2;
        __syncthreads();
    }
}

// Horizontal half of cv::resize(INTER_CUBIC) x4 on the u16 band windows of a launch (HResizeCubic: four taps, edge
// replicated, every product and sum a separate f32 rounding -- the order of resize_cubic_kernel), packed two bands per
// complex value: array a = H(bX) + i H(bY) occupies columns [a stride, a stride + cols) of an m x (4 stride) array of
// pitch Pn, columns [cols, stride) zero (cv::phaseCorrelate's right padding); rows {0, 1, m-2, m-1} also go to
// raw[r][a][x] for the vertical operator's edge terms.
// (BandPackJob: the band windows of the four arrays of a launch, array a = bx[a] + i by[a]; also pack_bands_kernel's)
struct BandPackJob {
    const uint16_t *bx[4], *by[4];
    long pitch[4];
};
__global__ __launch_bounds__(128) void hpack_bands_kernel(BandPackJob job, int m, int n, int cols, int stride, int Pn, const int *__restrict__ xofs,
                                                          const float4 *__restrict__ alpha, float2 *__restrict__ z, float2 *__restrict__ raw)
{
    const int x = blockIdx.x * 128 + threadIdx.x;
    const int a = blockIdx.z;
    if (x >= stride) return;
    const bool in = x < cols;
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
    if (in) {
        const int sx = xofs[x];
        w = alpha[x];
        c0 = sx - 1; c1 = sx; c2 = sx + 1; c3 = sx + 2;
        c0 = c0 < 0 ? 0 : (c0 > n - 1 ? n - 1 : c0);
        c1 = c1 < 0 ? 0 : (c1 > n - 1 ? n - 1 : c1);
        c2 = c2 < 0 ? 0 : (c2 > n - 1 ? n - 1 : c2);
        c3 = c3 < 0 ? 0 : (c3 > n - 1 ? n - 1 : c3);
    }
    const uint16_t *bx = job.bx[a], *by = job.by[a];
    const long pitch = job.pitch[a];
    auto taps = [&](const uint16_t *S) {
        float v = __fmul_rn((float)S[c0], w.x);
        v = __fadd_rn(v, __fmul_rn((float)S[c1], w.y));
        v = __fadd_rn(v, __fmul_rn((float)S[c2], w.z));
        v = __fadd_rn(v, __fmul_rn((float)S[c3], w.w));
        return v;
    };
#pragma unroll 2
    for (int y = blockIdx.y; y < m; y += gridDim.y) {
        float2 v = make_float2(0.f, 0.f);
        if (in) v = make_float2(taps(bx + y * pitch), taps(by + y * pitch));
        z[(long)y * Pn + (long)a * stride + x] = v;
        const int r = y < 2 ? y : (y >= m - 2 ? y - (m - 4) : -1);
        if (r >= 0) raw[((long)r * 4 + a) * stride + x] = v;
    }
}

struct FusedRow {
    int F, fwd_threads;
    void (*fwd1)(FusedJob, int, int, const int *, const float2 *);        // one spectrum -> one output
    void (*fwd3)(FusedJob, int, int, const int *, const float2 *);        // three spectra -> two outputs
};
// power-of-two radices last: their stores are then contiguous in LDS (a leading radix-8 stage
// stores at a 128-byte stride, an 8-way bank conflict for ds_write_b64)
//
// 3000 points, three spectra: a three-stage factorisation (3000 = 25 * 15 * 8: composite butterflies in registers,
// oip_fft_dev.h) and every stage dealt over all buffers at once (StagesAll): a point crosses LDS three times per transform
// instead of five, a stage costs two barriers for all buffers instead of one per buffer.  Single-line items keep LDS
// accesses 8 bytes wide and conflict-free (the first stage stores at a 25-point stride: 100 dwords, odd multiple of 4).
// Measured per launch: 0.80 -> 0.76 ms at 3000 points.  The 1250-point geometry (25 * 25 * 2) was measured too and is
// slower this way (0.46 vs 0.33 ms: eight rounds of radix-2 items), so it keeps the five-stage kernel.
// xpower_stage's grid rule gives this entry one workgroup per CU, the grid it was tuned at: its LDS estimate is
// 8 * (3 * 2 * 3000 + 1500) = 156000 B, so per_cu = min(163840 / 156000, 2048 / 768) = min(1, 2) = 1.
const FusedRow kFusedRow[] = {
    {kUpRowsN, 768, corr_rows_kernel<3000, 768, 1, 1, false, 3, 5, 5, 5, 8>, corr_rows_kernel<3000, 768, 3, 2, /*all*/ true, 25, 15, 8>},
    {kVRowsN, 512, corr_rows_kernel<1250, 512, 1, 1, false, 5, 5, 5, 5, 2>, corr_rows_kernel<1250, 512, 3, 2, false, 5, 5, 5, 5, 2>},
    {kStitchRowsN, 256, corr_rows_kernel<200, 256, 1, 1, false, 5, 5, 8>, corr_rows_kernel<200, 256, 3, 2, false, 5, 5, 8>},
};

// ---- peak: first maximum of the fftShift-ed surface + 5x5 weighted centroid ----------------------

// weightedCentroid(C, peak, Size(5,5), &response) (phasecorr.cpp) in one launch: block `part` reduces the
// arg-max slots of its surface, evaluates the 25 window cells directly -- the last inverse column pass is
//     c(y, x) = sum_{n < F1} data[(y mod S) + S n][x] exp(+2 pi i n y / M)        (S = M / F1; nothing was stored by it)
// so a cell is a 128-term sum for the 16000-line geometry -- and runs weightedCentroid on them.  The cell values differ
// from the pass's own in the last bits (another summation order), like any two float transforms.
constexpr int kPeakWinThreads = 1024;
// up to four complex arrays per launch (the four outputs of a pair of units): block = array * nparts + part; array j uses
// the slot set slots + j * 2 * kPeakSlots
struct PeakWinJob {
    const float2 *data[4];
    double *result[4];
};
__global__ __launch_bounds__(kPeakWinThreads) void peak_window_kernel(PeakWinJob job, int M, int N, int P, int F1, int S,
                                                                     const float2 *__restrict__ twM, unsigned long long *__restrict__ slots,
                                                                     int nparts)
{
    constexpr int NW = kPeakWinThreads / 64;
    const int arr = blockIdx.x / nparts, part = blockIdx.x - arr * nparts;
    const float2 *__restrict__ data = job.data[arr];
    double *__restrict__ result = job.result[arr];
    slots += (long)arr * 2 * kPeakSlots;
    __shared__ unsigned long long sbest[NW];
    __shared__ float win[25];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long best = 0ull;
    for (int i = threadIdx.x; i < kPeakSlots; i += kPeakWinThreads) {
        const unsigned long long v = slots[part * kPeakSlots + i];
        best = v > best ? v : best;
        // last reader of this surface's slots: leave them empty for the next surface (the pass fills the imaginary
        // one's slots even when only the real surface is wanted)
        slots[part * kPeakSlots + i] = 0ull;
        if (nparts == 1) slots[kPeakSlots + i] = 0ull;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off, 64);
        best = o > best ? o : best;
    }
    if (lane == 0) sbest[wave] = best;
    __syncthreads();
    best = sbest[0];
    for (int w = 1; w < NW; ++w) best = sbest[w] > best ? sbest[w] : best;
    const long key = oip_peak_key(best, 0);           // an all-NaN surface has no entry: minMaxLoc leaves (0, 0)
    const int py = (int)(key / N), px = (int)(key - (long)py * N);
    // a wave per window cell (all loads of the window in flight together)
    for (int cell = wave; cell < 25; cell += NW) {
        const int ys = py - 2 + cell / 5, xs = px - 2 + cell % 5;
        float acc = 0.f;
        const bool inside = ys >= 0 && ys < M && xs >= 0 && xs < N;     // weightedCentroid clamps the window to the image
        if (inside) {
            int yo = ys - (M >> 1); if (yo < 0) yo += M;                 // fftShift
            int xo = xs - (N >> 1); if (xo < 0) xo += N;
            const int o1 = yo % S;
            for (int n = lane; n < F1; n += 64) {
                const float2 z = data[(long)(o1 + S * n) * P + xo];
                const float2 w = twM[(int)(((long)n * yo) % M)];         // exp(-2 pi i n yo / M); the sum wants its conjugate
                acc += part ? __fsub_rn(__fmul_rn(z.y, w.x), __fmul_rn(z.x, w.y)) : __fadd_rn(__fmul_rn(z.x, w.x), __fmul_rn(z.y, w.y));
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) win[cell] = inside ? acc : NAN;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double cxs = 0.0, cys = 0.0, si = 0.0;
    for (int dy = 0; dy < 5; ++dy)
        for (int dx = 0; dx < 5; ++dx) {
            const int y = py - 2 + dy, x = px - 2 + dx;
            if (y < 0 || y >= M || x < 0 || x >= N) continue;
            const double v = (double)win[dy * 5 + dx];
            cxs = __dadd_rn(cxs, __dmul_rn((double)x, v));
            cys = __dadd_rn(cys, __dmul_rn((double)y, v));
            si = __dadd_rn(si, v);
        }
    double response = si;
    si = __dadd_rn(si, DBL_EPSILON);
    const double cx = cxs / si, cy = cys / si;
    response = response / (double)((long)M * N);
    result[3 * part + 0] = (double)N / 2.0 - cx;
    result[3 * part + 1] = (double)M / 2.0 - cy;
    result[3 * part + 2] = response;
}

OipAxisDigits digits_of(const std::vector<int> &f, int L)
{
    OipAxisDigits d;
    d.n = (int)f.size();
    d.L = L;
    for (int i = 0; i < 4; ++i) d.f[i] = i < d.n ? f[i] : 1;
    return d;
}

// ---- peak search of the spectral route: which lane tiles can hold a surface's maximum -------------------------------
// After the inverse row transform an output array Y~(ky, x) holds two real surfaces, y = c1 + i c2, and the inverse
// column transform is y(n, x) = sum_ky Y~(ky, x) u(ky, n) with |u| = 1 (stage and inter-pass twiddles alike), so
//     |c1(n, x)|, |c2(n, x)|  <=  |y(n, x)|  <=  B(x) := sum_ky |Re Y~(ky, x)| + |Im Y~(ky, x)|       for every n.
// A column whose B(x) lies below a surface value already found cannot hold that surface's maximum.  The row stage sums
// B per workgroup (UpRowsJob::bound); col_sel_first_kernel adds the workgroups' rows in a fixed order, takes the maximum
// Bt over each lane tile of the column passes and has the tile with the largest Bt searched (its column passes run on
// it and on its two neighbours, wrapping in x: the 5 x 5 window around a peak reads two columns beyond it).  With the
// candidates m1, m2 of the two surfaces then in the arg-max slots, col_sel_second_kernel has every other tile searched
// unless Bt (1 + eps) < min(m1, m2) -- written so that a NaN anywhere means "search".  One round is enough: the true
// maximum is at least the candidate, so what stays unsearched is strictly below it and cannot even tie.  A unit with a
// real peak is searched in a handful of tiles (B is of the order M sqrt(N) where the peak is M N times the response);
// without one B exceeds every surface value and all tiles are searched, as before.
// eps = 2^-8: the f32 sum of n = 16000 non-negative terms is off by at most (n - 1) 2^-24 = 9.5e-4 of its value, and the
// f32 transform's own error is about 1e-5 of sum |x|; 2^-8 = 3.9e-3 covers both four times over and costs nothing, the
// bound sitting 3 to 20 times below a usable peak.
constexpr float kPruneMargin = 0x1p-8f;
constexpr int kSelThreads = 1024, kSelParts = kSelThreads / kSelCols;       // kSelCols, kSelMaxTiles: oip_corrroute.h
struct PruneWork {
    float *bound;       // [row-stage workgroups][4][P]: the row stage's partial column sums (every row is written by every launch)
    int groups;         // workgroups of the row stage
    float *bt;          // [4][T]
    int *flags;         // [4][T]: bit 0 column passes done, bit 1 searched
    int *count;         // [2 phases][2: column passes, peak pass][4]
    int *tiles;         // [2][2][4][T]; null: the plan has no list form (the exhaustive passes run)
    int *ticket;        // [4]: workgroups of col_sel_first_kernel that are done with an array; [4]: arrays col_sel_second_kernel is
                        // done with; zero between launches
    int T, vshift;      // lane tiles of the column passes and log2 of their width
    // The stored window of the row stage (rows_window): tiles 0 .. win_r and T - win_r .. T - 1 hold data, the others do
    // not; win_r < 0: every tile does.  A tile the search would list outside of it makes the pair a miss: *miss is set,
    // the array lists nothing, the pair adds nothing to the statistics, and the host runs the pair again with every
    // column stored.
    int win_r;
    int *miss;
};
__device__ __forceinline__ bool tile_stored(const PruneWork &pw, int t) { return pw.win_r < 0 || t <= pw.win_r || t >= pw.T - pw.win_r; }

// grid (ceil(N / kSelCols), arrays): a workgroup sums kSelCols columns -- thread (x, j) the rows j, j + kSelParts, ... of
// column x, thread (x, 0) the kSelParts partial sums, both in a fixed order -- and leaves the maxima of their tiles; the
// workgroup of an array that finishes last (a ticket) picks the tile and writes the first lists.
__global__ __launch_bounds__(kSelThreads) void col_sel_first_kernel(PruneWork pw, int P, int N, int full)
{
    __shared__ float sPart[kSelParts][kSelCols];
    __shared__ float sBt[kSelMaxTiles];
    __shared__ int sbest;
    const int a = blockIdx.y, T = pw.T, V = 1 << pw.vshift;
    const int xl = threadIdx.x & (kSelCols - 1), j = threadIdx.x / kSelCols, x0 = blockIdx.x * kSelCols;
    {
        const int x = x0 + xl < N ? x0 + xl : N - 1;
        const float *p = pw.bound + (long)a * P + x;
        float s = 0.f;
#pragma unroll 8
        for (int g = j; g < pw.groups; g += kSelParts) s += p[(long)g * 4 * P];
        sPart[j][xl] = s;
    }
    __syncthreads();
    if (threadIdx.x < kSelCols) {
        float s = sPart[0][xl];
        for (int k = 1; k < kSelParts; ++k) s += sPart[k][xl];
        sPart[0][xl] = s;
    }
    __syncthreads();
    if (threadIdx.x < kSelCols / V) {
        const int t = x0 / V + threadIdx.x;
        if (t < T) {
            float m = 0.f;
            bool bad = false;
            for (int x = t * V; x < (t + 1) * V && x < N; ++x) { const float b = sPart[0][x - x0]; bad = bad || b != b; m = fmaxf(m, b); }
            pw.bt[a * T + t] = bad ? NAN : m;
        }
        __threadfence();
    }
    __syncthreads();
    if (threadIdx.x == 0) sbest = atomicAdd(&pw.ticket[a], 1) == (int)gridDim.x - 1 ? 1 : 0;
    __syncthreads();
    if (!sbest) return;
    __syncthreads();
    __threadfence();                                    // the other workgroups' maxima, written before their tickets
    for (int t = threadIdx.x; t < T; t += kSelThreads) sBt[t] = __builtin_nontemporal_load(pw.bt + a * T + t);
    if (threadIdx.x == 0) pw.ticket[a] = 0;             // for the next launch
    __syncthreads();
    if (threadIdx.x < 64) {
        float bv = -1.f;        // Bt >= 0; a NaN never wins
        int bi = 0;
        for (int t = threadIdx.x; t < T; t += 64)
            if (sBt[t] > bv) { bv = sBt[t]; bi = t; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (threadIdx.x == 0) sbest = bi;
    }
    __syncthreads();
    const int tm = sbest, tp = tm ? tm - 1 : T - 1, tn = tm + 1 < T ? tm + 1 : 0;
    int *listA = pw.tiles + (long)(0 * 4 + a) * T, *listP = pw.tiles + (long)(1 * 4 + a) * T;
    // the tile and its neighbours (whose edge columns the 5 x 5 window reads) must hold data
    const bool missed = !full && !(tile_stored(pw, tm) && tile_stored(pw, tp) && tile_stored(pw, tn));
    for (int t = threadIdx.x; t < T; t += kSelThreads) {
        pw.flags[a * T + t] = full ? 3 : (missed ? 0 : (t == tm ? 3 : (t == tp || t == tn ? 1 : 0)));
        if (full) { listA[t] = t; listP[t] = t; }
    }
    if (threadIdx.x == 0) {
        int nA = T, nP = T;
        if (missed) {
            atomicExch(pw.miss, 1);
            nA = nP = 0;
        } else if (!full) {
            listP[0] = tm;
            nP = 1;
            nA = 0;
            listA[nA++] = tm;
            if (tp != tm) listA[nA++] = tp;
            if (tn != tm && tn != tp) listA[nA++] = tn;
        }
        pw.count[0 * 4 + a] = nA;
        pw.count[1 * 4 + a] = nP;
        pw.count[2 * 4 + a] = 0;
        pw.count[3 * 4 + a] = 0;
    }
}

__device__ __forceinline__ float peak_slot_value(unsigned long long packed)        // oip_peak_pack's value; empty: -inf
{
    if (!packed) return -INFINITY;
    unsigned u = (unsigned)(packed >> 32);
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    return __uint_as_float(u);
}

// stats[0] += tiles searched, stats[1] += tiles (per array): oip_peak_prune_stats
__global__ __launch_bounds__(kPeakSlots) void col_sel_second_kernel(PruneWork pw, const unsigned long long *__restrict__ slots,
                                                                   unsigned long long *__restrict__ stats)
{
    constexpr int NW = kPeakSlots / 64;
    __shared__ unsigned long long sb[2][NW];
    __shared__ int sflag[kSelMaxTiles];
    __shared__ int nA, nP, smiss;
    const int a = blockIdx.x, T = pw.T;
    const unsigned long long *s = slots + (long)a * 2 * kPeakSlots;
    unsigned long long b0 = s[threadIdx.x], b1 = s[kPeakSlots + threadIdx.x];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o0 = __shfl_xor(b0, off, 64), o1 = __shfl_xor(b1, off, 64);
        b0 = o0 > b0 ? o0 : b0;
        b1 = o1 > b1 ? o1 : b1;
    }
    if ((threadIdx.x & 63) == 0) { sb[0][threadIdx.x >> 6] = b0; sb[1][threadIdx.x >> 6] = b1; }
    if (threadIdx.x == 0) { nA = 0; nP = 0; }
    for (int t = threadIdx.x; t < T; t += kPeakSlots) sflag[t] = pw.flags[a * T + t];
    __syncthreads();
    b0 = sb[0][0]; b1 = sb[1][0];
    for (int w = 1; w < NW; ++w) { b0 = sb[0][w] > b0 ? sb[0][w] : b0; b1 = sb[1][w] > b1 ? sb[1][w] : b1; }
    const float mm = fminf(peak_slot_value(b0), peak_slot_value(b1));         // NaN never enters a slot
    // a pair that missed the stored window in the first round (any of its arrays) lists nothing more
    if (threadIdx.x == 0) smiss = pw.win_r >= 0 ? atomicAdd(pw.miss, 0) : 0;
    __syncthreads();
    const bool dead = smiss != 0;
    __syncthreads();
    for (int t = threadIdx.x; t < T && !dead; t += kPeakSlots) {
        if (sflag[t] & 2) continue;
        const float bt = pw.bt[a * T + t];
        const bool skip = bt * (1.f + kPruneMargin) < mm && mm < INFINITY;    // false for a NaN and for an infinite candidate
        if (!skip) {
            sflag[t] |= 4;
            const int tp = t ? t - 1 : T - 1, tn = t + 1 < T ? t + 1 : 0;
            if (!(tile_stored(pw, t) && tile_stored(pw, tp) && tile_stored(pw, tn))) smiss = 1;
        }
    }
    __syncthreads();
    const bool missed = smiss != 0;
    int *listA = pw.tiles + (long)(2 * 4 + a) * T, *listP = pw.tiles + (long)(3 * 4 + a) * T;
    for (int t = threadIdx.x; t < T && !missed; t += kPeakSlots) {
        if (!(sflag[t] & 4)) continue;
        listP[atomicAdd(&nP, 1)] = t;
        const int nb[3] = {t ? t - 1 : T - 1, t, t + 1 < T ? t + 1 : 0};
#pragma unroll
        for (int d = 0; d < 3; ++d)
            if (!(atomicOr(&sflag[nb[d]], 1) & 1)) listA[atomicAdd(&nA, 1)] = nb[d];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        pw.count[2 * 4 + a] = nA;
        pw.count[3 * 4 + a] = nP;
        if (missed && !dead) atomicExch(pw.miss, 1);
        // the pair's counters are added once, by the array that finishes last, and only if no array missed: the attempt
        // whose result is kept counts
        __threadfence();
        if (atomicAdd(&pw.ticket[4], 1) == (int)gridDim.x - 1) {
            __threadfence();
            atomicExch(&pw.ticket[4], 0);           // for the next launch
            if (pw.win_r < 0 || atomicAdd(pw.miss, 0) == 0) {
                unsigned long long searched = 0;
                for (int o = 0; o < (int)gridDim.x; ++o) searched += (unsigned long long)(atomicAdd(&pw.count[1 * 4 + o], 0) + atomicAdd(&pw.count[3 * 4 + o], 0));
                atomicAdd(&stats[0], searched);
                atomicAdd(&stats[1], (unsigned long long)T * gridDim.x);
            }
        }
    }
}

// The carved workspace of one correlation call (CorrPlan::reg)
struct PcWork {
    PruneWork prune;
    float2 *z[5];
    float2 *y[4];
    float *fa;          // base window, f32
    float *fb[8];       // second images, f32 (up-sampled bands; two units' worth)
    float *fsmall;      // MSS window before resize
    unsigned long long *slots;  // [4 arrays][2][kPeakSlots] arg-max slots, empty between surfaces
    float2 *band;       // the band array(s) of a spectral route, inside z[1] (CorrPlan::band_sub)
    void *raw;          // their raw edge rows: behind the band array (HV) or in fsmall (V) (CorrPlan::raw_sub)
};

int carve(oip_ctx *ctx, const CorrPlan &plan, PcWork *w)
{
    void *ws;
    int rc = oip_workspace(ctx, plan.total, &ws);
    if (rc) return rc;
    auto at = [&](CorrRegionId r, int i) { return i < plan.reg[r].count ? (char *)ws + plan.reg[r].part(i) : nullptr; };
    auto sub = [&](const CorrSubRegion &s) { return s.bytes ? at(s.in, s.part) + s.offset : nullptr; };
    memset(w, 0, sizeof *w);
    PruneWork &pw = w->prune;
    pw.win_r = -1;
    pw.groups = plan.groups;
    pw.T = plan.T;
    pw.vshift = plan.vshift;
    pw.bound = (float *)at(kRegBound, 0);
    if (int *l = (int *)at(kRegLists, 0)) {
        // (prune_list_bytes) but for the tickets (cleared below) every word of these is written by col_sel_first_kernel before anything reads it
        pw.bt = (float *)l;
        pw.flags = l + 4 * pw.T;
        pw.count = l + 8 * pw.T;
        pw.ticket = l + 8 * pw.T + 16;
        pw.tiles = l + 8 * pw.T + 16 + 8;
    }
    for (int i = 0; i < 5; ++i) w->z[i] = (float2 *)at(kRegZ, i);
    for (int i = 0; i < 4; ++i) w->y[i] = (float2 *)at(kRegY, i);
    w->fa = (float *)at(kRegFa, 0);
    for (int i = 0; i < 8; ++i) w->fb[i] = (float *)at(kRegFb, i);
    w->fsmall = (float *)at(kRegSmall, 0);
    w->slots = (unsigned long long *)at(kRegSlots, 0);
    w->band = (float2 *)sub(plan.band_sub);
    w->raw = sub(plan.raw_sub);
    // the slots must start empty (later surfaces are cleaned by peak_window_kernel)
    ctx->prof_chain = nullptr;
    OIP_HIP(ctx, hipMemsetAsync(w->slots, 0, sizeof(unsigned long long) * 4 * 2 * kPeakSlots, ctx->stream));
    if (pw.ticket) OIP_HIP(ctx, hipMemsetAsync(pw.ticket, 0, sizeof(int) * 8, ctx->stream));
    return OIP_OK;
}

int launch_window(oip_ctx *ctx, const uint16_t *img, size_t pitch, long row0, int col0, int rows, int cols, float *out)
{
    long n = (long)rows * cols;
    long blocks = (n + kBlock - 1) / kBlock;
    long cap = (long)ctx->cu_count * 32;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    OipProfScope prof(ctx, "window_u16_to_f32_kernel");
    hipLaunchKernelGGL(window_u16_to_f32_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, img, pitch, row0,
                       col0, rows, cols, out);
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}

int resize_tables(oip_ctx *ctx, int sw, int sh, int dw, int dh, OipResizeTab **out)
{
    for (auto &t : ctx->resize_tabs)
        if (t.sw == sw && t.sh == sh && t.dw == dw && t.dh == dh) { *out = &t; return OIP_OK; }
    std::vector<int> xofs, yofs;
    std::vector<float> alpha, beta;
    resize_axis(sw, dw, &xofs, &alpha);
    resize_axis(sh, dh, &yofs, &beta);
    OipResizeTab t;
    t.sw = sw; t.sh = sh; t.dw = dw; t.dh = dh;
    t.d_xspec = nullptr; t.xspec_state = 0;
    t.d_yspec = nullptr; t.yspec_state = 0;
    t.x4 = dw == 4 * sw && dh == 4 * sh && axis_in_x4_window(xofs) && axis_in_x4_window(yofs);
    t.x4h = axis_is_x4(xofs);
    t.x4v = axis_is_x4(yofs);
    OIP_HIP(ctx, hipMalloc((void **)&t.d_xofs, sizeof(int) * dw));
    OIP_HIP(ctx, hipMalloc((void **)&t.d_alpha, sizeof(float) * 4 * dw));
    OIP_HIP(ctx, hipMalloc((void **)&t.d_yofs, sizeof(int) * dh));
    OIP_HIP(ctx, hipMalloc((void **)&t.d_beta, sizeof(float) * 4 * dh));
    OIP_HIP(ctx, hipMemcpy(t.d_xofs, xofs.data(), sizeof(int) * dw, hipMemcpyHostToDevice));
    OIP_HIP(ctx, hipMemcpy(t.d_alpha, alpha.data(), sizeof(float) * 4 * dw, hipMemcpyHostToDevice));
    OIP_HIP(ctx, hipMemcpy(t.d_yofs, yofs.data(), sizeof(int) * dh, hipMemcpyHostToDevice));
    OIP_HIP(ctx, hipMemcpy(t.d_beta, beta.data(), sizeof(float) * 4 * dh, hipMemcpyHostToDevice));
    ctx->resize_tabs.push_back(t);
    *out = &ctx->resize_tabs.back();
    return OIP_OK;
}

template <typename SrcT>
int launch_resize(oip_ctx *ctx, const SrcT *src, long spitch, int sw, int sh, float *dst, int dw, int dh)
{
    OipResizeTab *t;
    int rc = resize_tables(ctx, sw, sh, dw, dh, &t);
    if (rc) return rc;
    if (t->x4 && ((uintptr_t)dst & 15) == 0) {
        OipProfScope prof(ctx, "resize_cubic_x4_kernel");
        hipLaunchKernelGGL(resize_cubic_x4_kernel<SrcT>, dim3((sw + kBlock - 1) / kBlock, sh), dim3(kBlock), 0, ctx->stream,
                           src, spitch, sw, sh, dst, dw, t->d_xofs, reinterpret_cast<const float4 *>(t->d_alpha), t->d_yofs,
                           reinterpret_cast<const float4 *>(t->d_beta));
        OIP_HIP(ctx, hipGetLastError());
        return OIP_OK;
    }
    OipProfScope prof(ctx, "resize_cubic_kernel");
    hipLaunchKernelGGL(resize_cubic_kernel<SrcT>, dim3((dw + kBlock - 1) / kBlock, dh), dim3(kBlock), 0, ctx->stream, src,
                       spitch, sw, sh, dst, dw, dh, t->d_xofs, reinterpret_cast<const float4 *>(t->d_alpha), t->d_yofs,
                       reinterpret_cast<const float4 *>(t->d_beta));
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}

// The same for the exact x4 geometry (host-verified: yofs[dy] == (dy - 2) >> 2, even widths and pitch): a
// thread owns two adjacent columns and kV4Blocks source rows; the four outputs of source row p use rows
// p-2 .. p+2, so a 5-row window slides down one row per 4 outputs -- 1.25 loads of a pixel pair per 4 x 2
// outputs instead of 32 -- and the outputs leave as 8-byte stores.  Same taps, same f32 order.
constexpr int kV4Blocks = 8;        // source rows (= 4 output rows each) per thread
constexpr int kV4Threads = 128;
template <typename SrcT>
__global__ __launch_bounds__(kV4Threads) void resize_cubic_v_x4_kernel(VBatch<SrcT> vb, int sw, int sh, int dh,
                                                                      const float4 *__restrict__ beta)
{
    const int c = blockIdx.x * kV4Threads + threadIdx.x;            // column pair
    if (2 * c >= sw) return;
    const SrcT *__restrict__ src = vb.src[blockIdx.z] + 2 * c;
    float *__restrict__ dst = vb.dst[blockIdx.z] + 2 * c;
    const long spitch = vb.spitch[blockIdx.z];
    const int p0 = blockIdx.y * kV4Blocks;
    auto load = [&](int r) {                                        // clamped source row as two floats
        r = r < 0 ? 0 : (r > sh - 1 ? sh - 1 : r);
        const SrcT *q = src + (size_t)r * spitch;
        return make_float2((float)q[0], (float)q[1]);
    };
    float2 w0 = load(p0 - 2), w1 = load(p0 - 1), w2 = load(p0), w3 = load(p0 + 1), w4;
#pragma unroll
    for (int k = 0; k < kV4Blocks; ++k) {
        const int p = p0 + k;
        if (4 * p >= dh) break;
        w4 = load(p + 2);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int dy = 4 * p + j;
            const float4 b = beta[dy];
            // rows (dy - 2 >> 2) - 1 ... + 2: p-2..p+1 for j = 0, 1 and p-1..p+2 for j = 2, 3
            const float2 t0 = j < 2 ? w0 : w1, t1 = j < 2 ? w1 : w2, t2 = j < 2 ? w2 : w3, t3 = j < 2 ? w3 : w4;
            float2 o;
            o.x = __fmul_rn(t0.x, b.x);
            o.x = __fadd_rn(o.x, __fmul_rn(t1.x, b.y));
            o.x = __fadd_rn(o.x, __fmul_rn(t2.x, b.z));
            o.x = __fadd_rn(o.x, __fmul_rn(t3.x, b.w));
            o.y = __fmul_rn(t0.y, b.x);
            o.y = __fadd_rn(o.y, __fmul_rn(t1.y, b.y));
            o.y = __fadd_rn(o.y, __fmul_rn(t2.y, b.z));
            o.y = __fadd_rn(o.y, __fmul_rn(t3.y, b.w));
            if (dy < dh) *reinterpret_cast<float2 *>(dst + (size_t)dy * sw) = o;
        }
        w0 = w1; w1 = w2; w2 = w3; w3 = w4;
    }
}

// vertical half only (see resize_cubic_v_kernel) of `count` equally shaped images in one launch by the tables of their
// geometry (which carry the horizontal taps for the FFT loader); generic: not the x4 kernel (CorrKnobs::v_generic)
template <typename SrcT>
int launch_resize_v(oip_ctx *ctx, const SrcT *const *src, float *const *dst, int count, const long *spitch, const OipResizeTab *tab, bool generic)
{
    const int sw = tab->sw, sh = tab->sh, dh = tab->dh;
    if (count < 1 || count > kVBatch) return oip_fail(ctx, OIP_E_RUNTIME, "launch_resize_v: bad batch");
    VBatch<SrcT> vb;
    for (int i = 0; i < kVBatch; ++i) { vb.src[i] = src[i < count ? i : 0]; vb.dst[i] = dst[i < count ? i : 0]; vb.spitch[i] = spitch[i < count ? i : 0]; }
    OipProfScope prof(ctx, "resize_cubic_v_kernel");
    bool aligned = !generic && (sw & 1) == 0 && dh == 4 * sh && tab->x4v;
    for (int i = 0; i < count; ++i)
        aligned = aligned && (spitch[i] & 1) == 0 && ((size_t)src[i] % (2 * sizeof(SrcT))) == 0 && ((size_t)dst[i] & 7) == 0;
    if (aligned) {
        hipLaunchKernelGGL(resize_cubic_v_x4_kernel<SrcT>, dim3((sw / 2 + kV4Threads - 1) / kV4Threads, (sh + kV4Blocks - 1) / kV4Blocks, count),
                           dim3(kV4Threads), 0, ctx->stream, vb, sw, sh, dh, reinterpret_cast<const float4 *>(tab->d_beta));
        OIP_HIP(ctx, hipGetLastError());
        return OIP_OK;
    }
    hipLaunchKernelGGL(resize_cubic_v_kernel<SrcT>, dim3((sw + kBlock - 1) / kBlock, (dh + kVRows - 1) / kVRows, count), dim3(kBlock), 0,
                       ctx->stream, vb, sw, sh, dh, tab->d_yofs, reinterpret_cast<const float4 *>(tab->d_beta));
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}

// H and G_j of the x4 cubic up-sampling n -> N = 4 n along one axis (0: horizontal, 1: vertical) as an operator on
// spectra (see corr_rows_up_kernel; oip_upsample_operator in host.cpp builds them), cached on the device per resize
// geometry.  *out stays null when the geometry has no such form.
int upsample_spectrum_tables(oip_ctx *ctx, OipResizeTab *t, int axis, const float2 **out)
{
    *out = nullptr;
    int &state = axis ? t->yspec_state : t->xspec_state;
    void *&d_spec = axis ? t->d_yspec : t->d_xspec;
    if (state == 1) { *out = (const float2 *)d_spec; return OIP_OK; }
    if (state < 0) return OIP_OK;
    state = -1;
    const int n = axis ? t->sh : t->sw, N = axis ? t->dh : t->dw;
    if (N != 4 * n || n < 8 || !(axis ? t->x4v : t->x4h)) return OIP_OK;
    std::vector<float2> tab((size_t)5 * N);
    if (oip_upsample_operator(n, reinterpret_cast<float *>(tab.data())) != OIP_OK) return OIP_OK;
    if (axis == 0)          // the horizontal tables carry the 1/2 of the unpacking of a packed band pair (spec2_of): exact
        for (auto &v : tab) { v.x *= 0.5f; v.y *= 0.5f; }
    OIP_HIP(ctx, hipMalloc(&d_spec, sizeof(float2) * tab.size()));
    OIP_HIP(ctx, hipMemcpy(d_spec, tab.data(), sizeof(float2) * tab.size(), hipMemcpyHostToDevice));
    state = 1;
    *out = (const float2 *)d_spec;
    return OIP_OK;
}

// one real image of a packed pair: an f32 image (pitch == cols) or a u16 raster window
struct RealSrc {
    const float *f32;
    const uint16_t *u16;
    long pitch16;
    const float *v;     // vertically up-sampled image; the horizontal taps are applied by the loader
};
inline RealSrc src_f32(const float *p) { return RealSrc{p, nullptr, 0, nullptr}; }
inline RealSrc src_u16(const uint16_t *p, long pitch) { return RealSrc{nullptr, p, pitch, nullptr}; }
inline RealSrc src_v(const float *p) { return RealSrc{nullptr, nullptr, 0, p}; }
inline RealSrc src_none() { return RealSrc{nullptr, nullptr, 0, nullptr}; }

// horizontal-tap tables of the V sources of a forward_packed call (all V sources of one call share them)
struct HTaps {
    int v_cols;
    const int *xofs;
    const float *alpha;
    int x4;
};

// forward transform of z = re + i im, the two f32 images read directly by the first pass;
// skip_rows: leave the row passes to the fused row-stage kernel
int forward_packed(oip_ctx *ctx, const OipFft2dPlan *pl, float2 *z, RealSrc re, RealSrc im, int rows, int cols, bool skip_rows,
                   const HTaps *vt = nullptr)
{
    OipFftIo io;
    memset(&io, 0, sizeof io);
    io.load_kind = 1;
    io.re = re.f32; io.re16 = re.u16; io.pitch_re16 = re.pitch16;
    io.im = im.f32; io.im16 = im.u16; io.pitch_im16 = im.pitch16;
    if (re.v || im.v) {
        if (!vt) return oip_fail(ctx, OIP_E_RUNTIME, "forward_packed: V source without horizontal taps");
        io.re_v = re.v; io.im_v = im.v;
        io.v_cols = vt->v_cols; io.xofs = vt->xofs; io.alpha = vt->alpha; io.x4 = vt->x4;
    }
    io.rows = rows; io.cols = cols;
    return oip_fft2d_exec(ctx, pl, z, 0, &io, skip_rows ? 1 : 0);
}

int launch_xpower(oip_ctx *ctx, float2 *out, const XpowerJob &job, const OipFft2dPlan *pl)
{
    OipProfScope prof(ctx, "cross_power_kernel");
    hipLaunchKernelGGL(cross_power_kernel, dim3((pl->N + kBlock - 1) / kBlock, pl->M / 2 + 1), dim3(kBlock), 0,
                       ctx->stream, out, job, pl->M, pl->N, pl->P, digits_of(pl->yf, pl->M), digits_of(pl->xf, pl->N));
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}

// What the drivers of one correlation call share: its plan (with the switches), the device forms of its FFT plans, its workspace,
// and for the inter-band routes the tables of the band -> PAN resize and the up-sampling operators the route applies
struct CorrCall {
    oip_ctx *ctx;
    const CorrPlan *plan;
    const OipFft2dPlan *pl, *band;      // plan->main, plan->band (null on the image route)
    OipResizeTab *tab;
    const float2 *xtab, *vtab;
    PcWork w;
};

int open_call(oip_ctx *ctx, const CorrPlan &plan, CorrCall *c)
{
    *c = CorrCall{ctx, &plan, nullptr, nullptr, nullptr, nullptr, nullptr, {}};
    int rc = oip_fft2d_plan(ctx, plan.M, plan.N, &c->pl);
    if (!rc && plan.route != kImage) rc = oip_fft2d_plan(ctx, plan.band.M, plan.band.N, &c->band);
    return rc ? rc : carve(ctx, plan, &c->w);
}

// plan and open a call on one pair of rows x cols images; too_tall: the caller's refusal of more than 65535 lines
int open_pair(oip_ctx *ctx, int rows, int cols, const CorrKnobs &knobs, const char *too_tall, CorrPlan *plan, CorrCall *c)
{
    char why[160];
    const int rc = plan_pair(rows, cols, knobs, too_tall, plan, why, sizeof why);
    return rc ? oip_fail(ctx, rc, "%s", why) : open_call(ctx, *plan, c);
}

// The fused row-stage kernel of this plan (forward rows + cross-power + inverse rows in one kernel), or null:
// forward row passes, cross_power_kernel and inverse row passes.
const FusedRow *row_stage(const CorrPlan &plan)
{
    for (const FusedRow &k : kFusedRow)
        if (plan.fused_rows && k.F == plan.N) return &k;
    return nullptr;
}

// Cross-power of ncorr (A, B) spectrum pairs into nout = ceil(ncorr / 2) arrays y[o] =
// C(2o) + i C(2o+1), through the fused row-stage kernel `rk` if there is one.  At most three distinct
// spectra per call.
int xpower_stage(oip_ctx *ctx, const OipFft2dPlan *pl, const FusedRow *rk, const SpecRef *a, const SpecRef *b, int ncorr,
                 float2 *const y[2])
{
    const int nout = (ncorr + 1) / 2;
    if (!rk) {
        for (int o = 0; o < nout; ++o) {
            XpowerJob job;
            memset(&job, 0, sizeof job);
            job.ncorr = ncorr - 2 * o > 1 ? 2 : 1;
            for (int c = 0; c < job.ncorr; ++c) { job.a[c] = a[2 * o + c]; job.b[c] = b[2 * o + c]; }
            int rc = launch_xpower(ctx, y[o], job, pl);
            if (rc) return rc;
        }
        return OIP_OK;
    }
    const float2 *twF;
    int rc = oip_fft_table(ctx, rk->F, &twF);
    if (rc) return rc;
    // the distinct spectra of the job, and per correlation which spectrum and slot hold A and B
    FusedJob fj;
    memset(&fj, 0, sizeof fj);
    int narr = 0, ia[4], ib[4], pa[4], pb[4];
    auto slot = [&](const float2 *z) {
        for (int i = 0; i < narr; ++i) if (fj.z[i] == z) return i;
        if (narr == 3) return -1;
        fj.z[narr] = z;
        return narr++;
    };
    for (int c = 0; c < ncorr; ++c) {
        ia[c] = slot(a[c].z); pa[c] = a[c].part;
        ib[c] = slot(b[c].z); pb[c] = b[c].part;
        if (ia[c] < 0 || ib[c] < 0) return oip_fail(ctx, OIP_E_RUNTIME, "xpower_stage: more than three spectra");
    }
    for (int o = 0; o < nout; ++o) fj.out[o] = y[o];
    // the kernel hard-wires which spectrum and slot feeds which correlation
    const bool one = narr == 1 && ncorr == 1 && ia[0] == 0 && pa[0] == 0 && ib[0] == 0 && pb[0] == 1;
    bool three = narr == 3 && ncorr == 4;
    const int want_ib[4] = {0, 1, 1, 2}, want_pb[3] = {1, 0, 1};
    for (int c = 0; c < 4 && three; ++c)
        three = ia[c] == 0 && pa[c] == 0 && ib[c] == want_ib[c] && (c == 3 || pb[c] == want_pb[c]);
    if (!one && !three) return oip_fail(ctx, OIP_E_RUNTIME, "xpower_stage: unsupported job shape");
    if (three) fj.last_part = pb[3];
    // persistent: as many workgroups as fit the CUs at once (LDS- or thread-limited)
    const size_t lds = sizeof(float2) * ((size_t)narr * 2 * rk->F + rk->F / 2);
    long per_cu = (long)(160 * 1024 / lds);
    if (per_cu > 2048 / rk->fwd_threads) per_cu = 2048 / rk->fwd_threads;
    if (per_cu < 1) per_cu = 1;
    long grid = (long)ctx->cu_count * per_cu;
    if (grid > pl->M / 2 + 1) grid = pl->M / 2 + 1;
    OipProfScope prof(ctx, "corr_rows_kernel");
    hipLaunchKernelGGL(one ? rk->fwd1 : rk->fwd3, dim3((unsigned)grid), dim3(rk->fwd_threads), 0, ctx->stream, fj, pl->M, pl->P,
                       pl->d_ypos, twF);
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}

// arg-max -> 5x5 window -> centroid of both parts (the real and imaginary surface) of `narr` arrays whose last inverse
// pass left per-tile maxima in slot sets 0 .. narr-1: one launch
int peak_windows(const CorrCall &c, float2 *const *y, double *const *d_results, int narr, int nparts)
{
    oip_ctx *ctx = c.ctx;
    const OipFft2dPlan *pl = c.pl;
    const float2 *twM;
    int rc;
    if ((rc = oip_fft_table(ctx, pl->M, &twM))) return rc;
    const int F1 = pl->yf[0];
    PeakWinJob job;
    for (int j = 0; j < 4; ++j) { job.data[j] = y[j < narr ? j : 0]; job.result[j] = d_results[j < narr ? j : 0]; }
    OipProfScope prof(ctx, "peak_window_kernel");
    hipLaunchKernelGGL(peak_window_kernel, dim3(narr * nparts), dim3(kPeakWinThreads), 0, ctx->stream, job, pl->M, pl->N, pl->P, F1, pl->M / F1, twM,
                       c.w.slots, nparts);
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}

// inverse transform of y whose last pass only leaves per-tile maxima, in slot set `slot_set`; peak_windows turns them
// into results
int inverse_to_slots(const CorrCall &c, float2 *y, bool rows_done, int slot_set)
{
    OipFftIo io;
    memset(&io, 0, sizeof io);
    io.store_kind = 1;
    io.slots = c.w.slots + (long)slot_set * 2 * kPeakSlots;
    return oip_fft2d_exec(c.ctx, c.pl, y, 1, &io, rows_done ? 1 : 0);
}

// one pair (a, b) -> result slot
int correlate_pair(const CorrCall &c, RealSrc a, RealSrc b, double *d_result)
{
    const PcWork &w = c.w;
    const FusedRow *rk = row_stage(*c.plan);
    int rc = forward_packed(c.ctx, c.pl, w.z[0], a, b, c.plan->rows, c.plan->cols, rk != nullptr);
    if (rc) return rc;
    const SpecRef sa[1] = {{w.z[0], 0}}, sb[1] = {{w.z[0], 1}};
    float2 *const y[2] = {w.y[0], nullptr};
    if ((rc = xpower_stage(c.ctx, c.pl, rk, sa, sb, 1, y))) return rc;
    if ((rc = inverse_to_slots(c, w.y[0], rk != nullptr, 0))) return rc;
    double *const res[1] = {d_result};
    return peak_windows(c, y, res, 1, 1);
}

// base image (real slot of zp) against (imag slot of zp, both slots of zq, slot `last_part` of zl)
int correlate_four(const CorrCall &c, const FusedRow *rk, float2 *zp, float2 *zq, float2 *zl, int last_part, double *d_results /* 4 x 3 */)
{
    const SpecRef sa[4] = {{zp, 0}, {zp, 0}, {zp, 0}, {zp, 0}};
    const SpecRef sb[4] = {{zp, 1}, {zq, 0}, {zq, 1}, {zl, last_part}};
    float2 *const y[2] = {c.w.y[0], c.w.y[1]};
    int rc;
    if ((rc = xpower_stage(c.ctx, c.pl, rk, sa, sb, 4, y))) return rc;
    if ((rc = inverse_to_slots(c, y[0], rk != nullptr, 0))) return rc;
    if ((rc = inverse_to_slots(c, y[1], rk != nullptr, 1))) return rc;
    double *const res[2] = {d_results, d_results + 6};
    return peak_windows(c, y, res, 2, 2);
}

// One inter-band unit: a PAN window (rows x cols u16) and the matching windows of the four bands
// (band_rows x band_cols u16), each with its own pitch -- a window of the resident raster or a compact
// copy received from another rank.
struct IbUnit {
    const uint16_t *pan;
    long pan_pitch;
    const uint16_t *band[OIP_MSS_BANDS];
    long band_pitch;
};
// The units a driver takes at once: two (which share transforms) or the last one alone; res[u]: the 4 x 3 results of unit
// u; miss: the group's flag of the row stage's window
struct UnitGroup {
    const IbUnit *unit[2];
    int n;
    double *res[2];
    int *miss;
    RealSrc pan(int u) const { return u < n ? src_u16(unit[u]->pan, unit[u]->pan_pitch) : src_none(); }
};

// vertical cubic passes of all bands of the group in one launch (u16 -> f32 V images, rows x band_cols, in fb)
int upsample_bands(const CorrCall &c, const UnitGroup &g, RealSrc *v /* 4 per unit */)
{
    const uint16_t *srcs[kVBatch];
    long pitches[kVBatch];
    for (int u = 0; u < g.n; ++u)
        for (int b = 0; b < OIP_MSS_BANDS; ++b) {
            srcs[4 * u + b] = g.unit[u]->band[b];
            pitches[4 * u + b] = g.unit[u]->band_pitch;
            v[4 * u + b] = src_v(c.w.fb[4 * u + b]);
        }
    return launch_resize_v<uint16_t>(c.ctx, srcs, c.w.fb, 4 * g.n, pitches, c.tab, c.plan->knobs.v_generic);
}

// The image route: base image against four up-sampled bands per unit, the horizontal taps in the FFT loader.  A unit is
// PAN + i b0 and b1 + i b2; the fourth bands of two units share one complex transform (b3 of unit A in the real slot, b3
// of unit B in the imaginary slot), so a pair costs 5 forward transforms instead of 6, a single unit 3; 2 inverse each.
int correlate_units_image(const CorrCall &c, const UnitGroup &g)
{
    const PcWork &w = c.w;
    const FusedRow *rk = row_stage(*c.plan);
    const HTaps vt{c.plan->band_cols, c.tab->d_xofs, c.tab->d_alpha, c.tab->x4h};
    auto forward = [&](float2 *z, RealSrc re, RealSrc im) { return forward_packed(c.ctx, c.pl, z, re, im, c.plan->rows, c.plan->cols, rk != nullptr, &vt); };
    RealSrc v[8];
    int rc;
    if ((rc = upsample_bands(c, g, v))) return rc;
    for (int u = 0; u < g.n; ++u)
        if ((rc = forward(w.z[2 * u], g.pan(u), v[4 * u])) || (rc = forward(w.z[2 * u + 1], v[4 * u + 1], v[4 * u + 2]))) return rc;
    float2 *zl = w.z[2 * g.n];
    if ((rc = forward(zl, v[3], g.n > 1 ? v[7] : src_none()))) return rc;
    for (int u = 0; u < g.n; ++u)
        if ((rc = correlate_four(c, rk, w.z[2 * u], w.z[2 * u + 1], zl, u, g.res[u]))) return rc;
    return OIP_OK;
}

// ---- the spectral routes: the up-sampling applied to the band spectra in the row stage ----------------------------------
// Their shared head: one full-size forward transform (PAN_A + i PAN_B; B may be absent) up to its row passes
int forward_pans(const CorrCall &c, const UnitGroup &g)
{
    return forward_packed(c.ctx, c.pl, c.w.z[0], g.pan(0), g.pan(1), c.plan->rows, c.plan->cols, true);
}
// the band windows of the four arrays of a launch: array a = bX + i bY of unit a / 2 (a single unit's twice)
BandPackJob band_pack_job(const UnitGroup &g)
{
    BandPackJob bj;
    for (int a = 0; a < 4; ++a) {
        const IbUnit *u = g.unit[(a < 2 * g.n ? a : 0) / 2];
        bj.bx[a] = u->band[2 * (a & 1)]; bj.by[a] = u->band[2 * (a & 1) + 1]; bj.pitch[a] = u->band_pitch;
    }
    return bj;
}
// the column passes of the packed band array (four arrays side by side), reported apart
int band_columns(const CorrCall &c)
{
    c.ctx->prof_tag = "_band";
    const int rc = oip_fft2d_exec(c.ctx, c.band, c.w.band, 0, nullptr, 1);
    c.ctx->prof_tag = nullptr;
    return rc;
}
// Their shared tail: the results of output o = 2 u + h are bands 2 h, 2 h + 1 of unit u.  exhaustive: the inverse column
// passes of every output into its own slot set (else the caller has searched them); then the peak windows.
int finish_outputs(const CorrCall &c, const UnitGroup &g, bool exhaustive)
{
    const int narr = 2 * g.n;
    double *res[4];
    for (int o = 0; o < narr; ++o) {
        res[o] = g.res[o / 2] + 6 * (o & 1);
        if (exhaustive)
            if (int rc = inverse_to_slots(c, c.w.y[o], true, o)) return rc;
    }
    return peak_windows(c, c.w.y, res, narr, 2);
}

// The band windows of a launch as one complex array: array a = bX + i bY occupies columns [n a, n a + n) of an
// m x (4 n) array of pitch Pn (the column passes then run over all four at once); rows {0, 1, m-2, m-1} of each array
// also go to raw16[r][a n / 2 + p / 2] as (bX | bY << 16) of the points p, p + 1 (n even).
template <bool PAIRS>        // PAIRS: two neighbouring columns per thread through 4-byte loads (host-checked alignment)
__global__ __launch_bounds__(128) void pack_bands_kernel(BandPackJob job, int m, int n, int Pn, float2 *__restrict__ z, unsigned *__restrict__ raw16)
{
    constexpr int W = PAIRS ? 2 : 1;
    const int p = W * (blockIdx.x * 128 + threadIdx.x);
    const int a = blockIdx.z;
    if (p >= n) return;
    const uint16_t *bx = job.bx[a] + p, *by = job.by[a] + p;
    const long pitch = job.pitch[a];
#pragma unroll 4
    for (int y = blockIdx.y; y < m; y += gridDim.y) {
        const int r = y < 2 ? y : (y >= m - 2 ? y - (m - 4) : -1);
        if (PAIRS) {
            const unsigned ux = *reinterpret_cast<const unsigned *>(bx + y * pitch), uy = *reinterpret_cast<const unsigned *>(by + y * pitch);
            *reinterpret_cast<float4 *>(z + (long)y * Pn + a * n + p) =
                make_float4((float)(ux & 0xffffu), (float)(uy & 0xffffu), (float)(ux >> 16), (float)(uy >> 16));
            if (r >= 0) *reinterpret_cast<uint2 *>(raw16 + ((long)r * 4 + a) * n + p) = make_uint2((ux & 0xffffu) | (uy << 16), (ux >> 16) | (uy & 0xffff0000u));
        } else {
            const unsigned ux = bx[y * pitch], uy = by[y * pitch];
            z[(long)y * Pn + a * n + p] = make_float2((float)ux, (float)uy);
            if (r >= 0) raw16[((long)r * 4 + a) * n + p] = ux | (uy << 16);
        }
    }
}

// The H and HV routes (3000-point rows, corr_rows_up_kernel): the band arrays are four quarter-width (`_quarter`) column
// transforms of the vertically up-sampled bands (H: V images, rows x band_cols, packed two by two), or the column
// transform of the band windows themselves, four arrays side by side (HV); one row-stage launch, four inverse column
// transforms.  Against the image route: 2 instead of 5 array-sized forward column transforms, 6 instead of 10 row
// transforms of 3000 points (in units of one).  win_r: the stored window of this run, -1 for every column.
int correlate_units_up(const CorrCall &c, const UnitGroup &g, int win_r)
{
    oip_ctx *ctx = c.ctx;
    const CorrPlan &plan = *c.plan;
    const OipFft2dPlan *pl = c.pl;
    const PcWork &w = c.w;
    const bool both = plan.route == kSpectralHV;
    const int narr = 2 * g.n, Pn = c.band->P;
    int rc;
    if ((rc = forward_pans(c, g))) return rc;
    if (both) {
        const BandPackJob bj = band_pack_job(g);
        {
            OipProfScope prof(ctx, "pack_bands_kernel");
            const int band_rows = plan.band_rows, band_cols = plan.band_cols;
            bool pairs = (band_cols & 1) == 0 && (Pn & 1) == 0;
            for (int a = 0; a < 4; ++a)
                pairs = pairs && (bj.pitch[a] & 1) == 0 && ((size_t)bj.bx[a] & 3) == 0 && ((size_t)bj.by[a] & 3) == 0;
            const int gy = band_rows < 128 ? band_rows : 128;
            if (pairs)
                hipLaunchKernelGGL(pack_bands_kernel<true>, dim3((band_cols / 2 + 127) / 128, gy, 4), dim3(128), 0, ctx->stream, bj, band_rows, band_cols, Pn,
                                   w.band, (unsigned *)w.raw);
            else
                hipLaunchKernelGGL(pack_bands_kernel<false>, dim3((band_cols + 127) / 128, gy, 4), dim3(128), 0, ctx->stream, bj, band_rows, band_cols, Pn,
                                   w.band, (unsigned *)w.raw);
            OIP_HIP(ctx, hipGetLastError());
        }
        if ((rc = band_columns(c))) return rc;
    } else {
        RealSrc v[8];
        if ((rc = upsample_bands(c, g, v))) return rc;
        ctx->prof_tag = "_quarter";
        for (int a = 0; a < narr && !rc; ++a)
            rc = forward_packed(ctx, c.band, w.band + a * (long)plan.M * Pn, src_f32(v[2 * a].v), src_f32(v[2 * a + 1].v), plan.rows, plan.band_cols, true);
        ctx->prof_tag = nullptr;
        if (rc) return rc;
    }
    const float2 *twF, *twS;
    if ((rc = oip_fft_table(ctx, kUpRowsN, &twF)) || (rc = oip_fft_table(ctx, kUpRowsBandN, &twS))) return rc;
    UpRowsJob fj;
    memset(&fj, 0, sizeof fj);
    fj.zp = w.z[0];
    fj.zn = w.band;
    fj.zn_stride = both ? plan.band_cols : (long)plan.M * Pn;
    fj.Pn = Pn;
    for (int o = 0; o < 4; ++o) fj.out[o] = w.y[o];
    fj.xtab = c.xtab;
    fj.nout = narr;
    fj.vtab = c.vtab;
    fj.raw16 = reinterpret_cast<const uint2 *>(w.raw);
    fj.ypos_s = both ? c.band->d_ypos : nullptr;
    fj.m = plan.band_rows;
    fj.bound = w.prune.bound;
    // (not cleared: every workgroup of the launch below writes its four rows in full, with 8-byte stores)
    // The stored window (rows_window): tiles 0 .. win_r and T - win_r .. T - 1 of the column passes' lane tiles, as pieces
    // of two columns.  The peak search below tells a pair that needs a tile outside of it (PruneWork::miss).
    PruneWork pw = w.prune;
    const int full = c.plan->knobs.peak_prune ? 0 : 1;           // every tile is listed: every column is stored
    pw.win_r = win_r;
    pw.miss = g.miss;
    if (win_r >= 0) {
        fj.win_hi = ((win_r + 1) << pw.vshift) / 2;
        fj.win_lo = ((pw.T - win_r) << pw.vshift) / 2;
    }
    if (c.plan->knobs.window_poison)      // debug: what the window leaves unwritten reads as NaN, not as the last pair's data
        for (int o = 0; o < narr; ++o) OIP_HIP(ctx, hipMemsetAsync(w.y[o], 0xff, sizeof(float2) * (size_t)pl->M * pl->P, ctx->stream));
    {
        OipProfScope prof(ctx, "corr_rows_up_kernel");
        // (no windowed instance without VEXP: it has not been built since that kernel stopped spilling -- DESIGN.md 4.3)
        auto k = both ? (win_r >= 0 ? corr_rows_up_kernel<512, true, true> : corr_rows_up_kernel<512, true, false>)
                      : corr_rows_up_kernel<512, false, false>;
        // measured in bench.py, VEXP: 1.275 ms with 512 threads (244 VGPRs, no scratch), 1.36 with 768 (168, 28 spilled)
        hipLaunchKernelGGL(k, dim3((unsigned)w.prune.groups), dim3(512), 0, ctx->stream, fj, pl->M, pl->P, pl->d_ypos, twF, twS);
        OIP_HIP(ctx, hipGetLastError());
    }
    // a plan without list forms of its column passes: the exhaustive passes, each output into its own slot set
    if (!pw.tiles) return finish_outputs(c, g, true);
    // The inverse column passes of all outputs over the tiles that can hold a maximum (see PruneWork): select, column
    // passes, peak pass -- twice.  OIP_PEAK_PRUNE=0 lists every tile the first time: the exhaustive
    // search through the same kernels.  A tile that is not searched keeps its untransformed data in y[o]; nothing else
    // reads it (peak_window_kernel reads the two columns either side of a searched tile at most, and those are done).
    if (!ctx->d_prune_stats) {
        OIP_HIP(ctx, hipMalloc((void **)&ctx->d_prune_stats, 2 * sizeof(unsigned long long)));
        OIP_HIP(ctx, hipMemsetAsync(ctx->d_prune_stats, 0, 2 * sizeof(unsigned long long), ctx->stream));
    }
    {
        OipProfScope prof(ctx, "col_sel_first_kernel");
        hipLaunchKernelGGL(col_sel_first_kernel, dim3((pl->N + kSelCols - 1) / kSelCols, narr), dim3(kSelThreads), 0, ctx->stream, pw, pl->P, pl->N, full);
        OIP_HIP(ctx, hipGetLastError());
    }
    OipColList cl;
    memset(&cl, 0, sizeof cl);
    for (int o = 0; o < 4; ++o) cl.data[o] = w.y[o < narr ? o : 0];
    cl.stride = pw.T;
    cl.narr = narr;
    cl.slots = w.slots;
    for (int phase = 0; phase < 2; ++phase) {
        if (phase == 1) {
            OipProfScope prof(ctx, "col_sel_second_kernel");
            hipLaunchKernelGGL(col_sel_second_kernel, dim3(narr), dim3(kPeakSlots), 0, ctx->stream, pw, w.slots, ctx->d_prune_stats);
            OIP_HIP(ctx, hipGetLastError());
            if (full) break;            // every tile was listed the first time
        }
        for (int kind = 0; kind < 2; ++kind) {
            cl.count = pw.count + (phase * 2 + kind) * 4;
            cl.tiles = pw.tiles + (long)(phase * 2 + kind) * 4 * pw.T;
            if (kind == 1) {
                if ((rc = oip_fft_col_list_pass(ctx, pl, 0, cl, true, "col_sel_peak"))) return rc;
                continue;
            }
            for (int i = pl->n_y - 1; i >= 1; --i) {
                char name[32];
                snprintf(name, sizeof name, "col_sel_F%d", pl->passes[i].F);
                if ((rc = oip_fft_col_list_pass(ctx, pl, i, cl, false, name))) return rc;
            }
        }
    }
    return finish_outputs(c, g, false);
}

// The V route, a padded geometry -- the reference's 12288-wide strips: 1228-column slices, 1250-point rows -- with the
// vertical up-sampling on the spectra (corr_rows_v_kernel): the horizontally up-sampled bands transformed at their own
// height (four arrays side by side in z[1], their four raw edge rows in the small scratch), one row-stage launch per
// unit, four inverse column transforms.
int correlate_units_vup(const CorrCall &c, const UnitGroup &g)
{
    oip_ctx *ctx = c.ctx;
    const CorrPlan &plan = *c.plan;
    const OipFft2dPlan *pl = c.pl;
    const PcWork &w = c.w;
    const int N = plan.N, Pn = c.band->P;
    int rc;
    if ((rc = forward_pans(c, g))) return rc;
    float2 *raw = reinterpret_cast<float2 *>(w.raw);
    const BandPackJob hj = band_pack_job(g);
    {
        OipProfScope prof(ctx, "hpack_bands_kernel");
        const int gy = plan.band_rows < 256 ? plan.band_rows : 256;
        hipLaunchKernelGGL(hpack_bands_kernel, dim3((N + 127) / 128, gy, 4), dim3(128), 0, ctx->stream, hj, plan.band_rows, plan.band_cols, plan.cols, N, Pn,
                           c.tab->d_xofs, reinterpret_cast<const float4 *>(c.tab->d_alpha), w.band, raw);
        OIP_HIP(ctx, hipGetLastError());
    }
    if ((rc = band_columns(c))) return rc;
    const float2 *twF;
    if ((rc = oip_fft_table(ctx, kVRowsN, &twF))) return rc;
    VRowsJob fj;
    memset(&fj, 0, sizeof fj);
    fj.zp = w.z[0];
    fj.zn = w.band;
    fj.zn_stride = N;
    fj.Pn = Pn;
    for (int o = 0; o < 4; ++o) fj.out[o] = w.y[o];
    fj.nout = 2 * g.n;
    fj.vtab = c.vtab;
    fj.raw = raw;
    fj.ypos_s = c.band->d_ypos;
    fj.m = plan.band_rows;
    {
        OipProfScope prof(ctx, "corr_rows_v_kernel");
        long grid = 2L * ctx->cu_count;     // two workgroups per CU (60 KB of LDS, <= 128 VGPRs each)
        if (grid > pl->M / 2 + 1) grid = pl->M / 2 + 1;
        for (int u = 0; u < g.n; ++u)
            hipLaunchKernelGGL((corr_rows_v_kernel<1250, 512, 5, 5, 5, 5, 2>), dim3((unsigned)grid), dim3(512), 0, ctx->stream, fj, 2 * u, u, pl->M, pl->P,
                               pl->d_ypos, twF);
        OIP_HIP(ctx, hipGetLastError());
    }
    return finish_outputs(c, g, true);
}

// nflags ints that follow the results in d_small (the miss flags of the row stage's window) ride the same copy
int fetch_results(oip_ctx *ctx, int count, double *host_out, int nflags = 0, int *flags_out = nullptr)
{
    ctx->prof_chain = nullptr;
    OIP_HIP(ctx, hipMemcpyAsync(ctx->h_small, ctx->d_small, sizeof(double) * count + sizeof(int) * nflags, hipMemcpyDeviceToHost, ctx->stream));
    OIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(host_out, ctx->h_small, sizeof(double) * count);
    if (nflags) memcpy(flags_out, (const char *)ctx->h_small + sizeof(double) * count, sizeof(int) * nflags);
    return OIP_OK;
}

}  // namespace

extern "C" int oip_window_u16_to_f32(oip_ctx *ctx, const uint16_t *d_img, size_t pitch, long row0, int col0, int rows,
                                     int cols, float *d_out)
{
    OIP_CHECK_CTX(ctx);
    if (!d_img || !d_out || rows <= 0 || cols <= 0 || row0 < 0 || col0 < 0 || (size_t)(col0 + cols) > pitch)
        return oip_fail(ctx, OIP_E_INVALID, "oip_window_u16_to_f32: bad argument");
    return launch_window(ctx, d_img, pitch, row0, col0, rows, cols, d_out);
}

extern "C" int oip_resize_cubic_f32(oip_ctx *ctx, const float *d_src, int sw, int sh, float *d_dst, int dw, int dh)
{
    OIP_CHECK_CTX(ctx);
    if (!d_src || !d_dst || sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || dh > 65535)
        return oip_fail(ctx, OIP_E_INVALID, "oip_resize_cubic_f32: bad argument");
    return launch_resize<float>(ctx, d_src, sw, sw, sh, d_dst, dw, dh);
}

extern "C" int oip_phase_correlate_f32(oip_ctx *ctx, const float *d_a, const float *d_b, int rows, int cols, double *dx,
                                       double *dy, double *response)
{
    OIP_CHECK_CTX(ctx);
    if (!d_a || !d_b || rows <= 0 || cols <= 0) return oip_fail(ctx, OIP_E_INVALID, "oip_phase_correlate_f32: bad argument");
    const CorrKnobs knobs = CorrKnobs::from_env();
    CorrPlan plan;
    CorrCall c;
    int rc = open_pair(ctx, rows, cols, knobs, "oip_phase_correlate_f32: more than 65535 rows", &plan, &c);
    if (rc) return rc;
    double *d_res = (double *)ctx->d_small;
    if ((rc = correlate_pair(c, src_f32(d_a), src_f32(d_b), d_res))) return rc;
    double r[3];
    if ((rc = fetch_results(ctx, 3, r))) return rc;
    if (dx) *dx = r[0];
    if (dy) *dy = r[1];
    if (response) *response = r[2];
    return OIP_OK;
}

// CCD-pair correlations of n window pairs (the loop body of stitcher.h:166-191 after the colRange): window i is
// rows x cols u16 at a[i] / b[i] with its own pitch; results go to d_res[3 * i]
static int stt_pairs(oip_ctx *ctx, const CorrKnobs &knobs, const uint16_t *const *a, const size_t *pitch_a, const uint16_t *const *b,
                     const size_t *pitch_b, int n, int rows, int cols, double *host_out)
{
    CorrPlan plan;
    CorrCall c;
    int rc = open_pair(ctx, rows, cols, knobs, "correlation window taller than 65535 lines", &plan, &c);
    if (rc) return rc;
    if ((rc = oip_small(ctx, sizeof(double) * 3 * (size_t)(n > 0 ? n : 1)))) return rc;
    double *d_res = (double *)ctx->d_small;
    for (int i = 0; i < n; ++i)
        if ((rc = correlate_pair(c, src_u16(a[i], (long)pitch_a[i]), src_u16(b[i], (long)pitch_b[i]), d_res + 3 * i)))
            return rc;
    if (n > 0 && (rc = fetch_results(ctx, 3 * n, host_out))) return rc;
    return OIP_OK;
}

extern "C" int oip_stt_correlate_windows(oip_ctx *ctx, const uint16_t *const *d_a, const size_t *pitch_a,
                                         const uint16_t *const *d_b, const size_t *pitch_b, int n, int rows, int cols,
                                         double *out)
{
    OIP_CHECK_CTX(ctx);
    if (n < 0 || (n > 0 && (!d_a || !d_b || !pitch_a || !pitch_b || !out)) || rows <= 0 || cols <= 0)
        return oip_fail(ctx, OIP_E_INVALID, "oip_stt_correlate_windows: bad argument");
    for (int i = 0; i < n; ++i)
        if (!d_a[i] || !d_b[i] || pitch_a[i] < (size_t)cols || pitch_b[i] < (size_t)cols)
            return oip_fail(ctx, OIP_E_INVALID, "oip_stt_correlate_windows: window %d has a null pointer or a pitch below %d", i, cols);
    return stt_pairs(ctx, CorrKnobs::from_env(), d_a, pitch_a, d_b, pitch_b, n, rows, cols, out);
}

extern "C" int oip_stt_correlate(oip_ctx *ctx, const uint16_t *d_pan1, const uint16_t *d_pan2, int W, long L, long row0,
                                 long nrows, int sections, int lines_per_section, int overlap_cols, int edge_cols,
                                 double *out)
{
    OIP_CHECK_CTX(ctx);
    if (!d_pan1 || !d_pan2 || !out) return oip_fail(ctx, OIP_E_INVALID, "oip_stt_correlate: bad argument");
    OIPGPU::CcdGeom g;
    const std::string refused = OIPGPU::MakeCcdGeom(W, L, sections, lines_per_section, overlap_cols, edge_cols, &g);
    if (!refused.empty()) return oip_fail(ctx, OIP_E_INVALID, "%s", refused.c_str());
    std::vector<int> which;
    std::vector<const uint16_t *> a, b;
    for (int s = 0; s < sections; ++s) {
        const long off = g.section_start(s);
        if (off < row0 || off + g.rows > row0 + nrows) continue;     // another rank's section
        which.push_back(s);
        // the u16->f32 conversion happens in the first FFT pass' loader
        a.push_back(d_pan1 + (size_t)(off - row0) * W + g.col1);
        b.push_back(d_pan2 + (size_t)(off - row0) * W + g.col2);
    }
    std::vector<size_t> pitch(which.size(), (size_t)W);
    std::vector<double> r(3 * which.size() + 3);
    int rc = stt_pairs(ctx, CorrKnobs::from_env(), a.data(), pitch.data(), b.data(), pitch.data(), (int)which.size(), g.rows, g.cols, r.data());
    if (rc) return rc;
    for (int s = 0; s < sections; ++s)
        for (int k = 0; k < 3; ++k) out[3 * s + k] = NAN;
    for (size_t i = 0; i < which.size(); ++i)
        for (int k = 0; k < 3; ++k) out[3 * which[i] + k] = r[3 * i + k];
    return OIP_OK;
}

// The loop body of preproc.h:262-329 for n units: per unit and band (dx, dy, response) -> host_out[12 * u + 3 * b].
// Units go two at a time by the route of the plan (oip_corrroute.h: plan_interband).
static int interband_units(oip_ctx *ctx, const CorrKnobs &knobs, const IbUnit *units, int n, int rows, int cols, int band_rows, int band_cols,
                           double *host_out)
{
    // planned once per geometry and switches (0.1 ms of host arithmetic, most of it the x4 test of the resize offsets)
    const CorrPlan *cached = nullptr;
    for (const CorrPlan &p : ctx->corr_plans)
        if (p.rows == rows && p.cols == cols && p.band_rows == band_rows && p.band_cols == band_cols && p.knobs == knobs) cached = &p;
    int rc;
    if (!cached) {
        CorrPlan p;
        char why[160];
        if ((rc = plan_interband(rows, cols, band_rows, band_cols, ctx->cu_count, knobs, &p, why, sizeof why))) return oip_fail(ctx, rc, "%s", why);
        ctx->corr_plans.push_back(p);
        cached = &ctx->corr_plans.back();
    }
    const CorrPlan &plan = *cached;
    CorrCall c;
    if ((rc = open_call(ctx, plan, &c))) return rc;
    const bool haxis = plan.route == kSpectralH || plan.route == kSpectralHV, vaxis = plan.route == kSpectralHV || plan.route == kSpectralV;
    if ((rc = resize_tables(ctx, band_cols, band_rows, cols, rows, &c.tab))) return rc;
    if (haxis && (rc = upsample_spectrum_tables(ctx, c.tab, 0, &c.xtab))) return rc;
    if (vaxis && (rc = upsample_spectrum_tables(ctx, c.tab, 1, &c.vtab))) return rc;
    if ((haxis && !c.xtab) || (vaxis && !c.vtab)) return oip_fail(ctx, OIP_E_RUNTIME, "inter-band correlation: no up-sampling operator for the planned route");
    ctx->rows_window[0] = plan.lists ? 1 << plan.vshift : 0;
    ctx->rows_window[1] = plan.lists ? plan.T : 0;
    ctx->rows_window[2] = plan.win_r;
    // One miss flag of the row stage's window per group of units follows the results in d_small.
    const int ngroups = (n + 1) / 2;
    if ((rc = oip_small(ctx, sizeof(double) * 12 * (size_t)(n > 0 ? n : 1) + sizeof(int) * (size_t)(ngroups + 1)))) return rc;
    double *d_res = (double *)ctx->d_small;
    int *d_miss = reinterpret_cast<int *>(d_res + 12 * (size_t)n);
    if (plan.win_r >= 0) OIP_HIP(ctx, hipMemsetAsync(d_miss, 0, sizeof(int) * ngroups, ctx->stream));
    // group k: units 2 k, 2 k + 1 (or the last one alone); win_r: the row stage's window, -1 for every column
    auto run_group = [&](int k, int win_r) -> int {
        UnitGroup g{{&units[2 * k], &units[2 * k + (2 * k + 1 < n ? 1 : 0)]}, 2 * k + 1 < n ? 2 : 1, {d_res + 24 * k, d_res + 24 * k + 12}, d_miss + k};
        switch (plan.route) {
        case kSpectralH:
        case kSpectralHV: return correlate_units_up(c, g, win_r);
        case kSpectralV: return correlate_units_vup(c, g);
        default: return correlate_units_image(c, g);
        }
    };
    for (int k = 0; k < ngroups; ++k)
        if ((rc = run_group(k, plan.win_r))) return rc;
    if (n > 0 && plan.win_r >= 0) {
        // Groups whose peak search needed a tile outside the stored window (their flags came with the results) run again
        // from the top with every column stored -- with the same partner, on which a unit's last digits depend -- and the
        // results are fetched again.  Nothing waits but this call's own fetch.
        std::vector<int> miss((size_t)ngroups);
        if ((rc = fetch_results(ctx, 12 * n, host_out, ngroups, miss.data()))) return rc;
        int again = 0;
        for (int k = 0; k < ngroups; ++k)
            if (miss[k]) {
                ++again;
                if ((rc = run_group(k, -1))) return rc;
            }
        ctx->rows_window_pairs += ngroups;
        ctx->rows_window_rerun += again;
        if (!again) return OIP_OK;
    }
    if (n > 0 && (rc = fetch_results(ctx, 12 * n, host_out))) return rc;
    return OIP_OK;
}

extern "C" int oip_peak_prune_stats(oip_ctx *ctx, long long *tiles_searched, long long *tiles_total)
{
    OIP_CHECK_CTX(ctx);
    unsigned long long *h = nullptr;
    if (ctx->d_prune_stats) {
        int rc = oip_small(ctx, 2 * sizeof(unsigned long long));
        if (rc) return rc;
        h = (unsigned long long *)ctx->h_small;
        OIP_HIP(ctx, hipMemcpyAsync(h, ctx->d_prune_stats, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        OIP_HIP(ctx, hipMemsetAsync(ctx->d_prune_stats, 0, 2 * sizeof(unsigned long long), ctx->stream));
        OIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (tiles_searched) *tiles_searched = h ? (long long)h[0] : 0;
    if (tiles_total) *tiles_total = h ? (long long)h[1] : 0;
    return OIP_OK;
}

extern "C" int oip_rows_window_stats(oip_ctx *ctx, long long *pairs, long long *pairs_rerun)
{
    OIP_CHECK_CTX(ctx);
    if (pairs) *pairs = ctx->rows_window_pairs;
    if (pairs_rerun) *pairs_rerun = ctx->rows_window_rerun;
    ctx->rows_window_pairs = ctx->rows_window_rerun = 0;
    return OIP_OK;
}

extern "C" int oip_rows_window_geometry(oip_ctx *ctx, int *tile_cols, int *tiles, int *radius)
{
    OIP_CHECK_CTX(ctx);
    if (tile_cols) *tile_cols = ctx->rows_window[0];
    if (tiles) *tiles = ctx->rows_window[1];
    if (radius) *radius = ctx->rows_window[2];
    return OIP_OK;
}

extern "C" int oip_interband_correlate_units(oip_ctx *ctx, const uint16_t *const *d_pan, const size_t *pan_pitch,
                                             const uint16_t *const *d_bands, const size_t *band_pitch, int n, int rows,
                                             int cols, double *out)
{
    OIP_CHECK_CTX(ctx);
    if (n < 0 || (n > 0 && (!d_pan || !pan_pitch || !d_bands || !band_pitch || !out)) || rows <= 0 || cols <= 0)
        return oip_fail(ctx, OIP_E_INVALID, "oip_interband_correlate_units: bad argument");
    // preproc.h:274-276: the band window is the PAN window integer-divided by 4
    const int band_rows = rows / OIP_MSS_BANDS, band_cols = cols / OIP_MSS_BANDS;
    if (band_rows <= 0 || band_cols <= 0) return oip_fail(ctx, OIP_E_INVALID, "oip_interband_correlate_units: window too small");
    std::vector<IbUnit> units((size_t)n);
    for (int i = 0; i < n; ++i) {
        units[i].pan = d_pan[i];
        units[i].pan_pitch = (long)pan_pitch[i];
        units[i].band_pitch = (long)band_pitch[i];
        bool ok = d_pan[i] && pan_pitch[i] >= (size_t)cols && band_pitch[i] >= (size_t)band_cols;
        for (int b = 0; b < OIP_MSS_BANDS; ++b) { units[i].band[b] = d_bands[4 * i + b]; ok = ok && d_bands[4 * i + b]; }
        if (!ok) return oip_fail(ctx, OIP_E_INVALID, "oip_interband_correlate_units: unit %d has a null pointer or a short pitch", i);
    }
    return interband_units(ctx, CorrKnobs::from_env(), units.data(), n, rows, cols, band_rows, band_cols, out);
}

extern "C" int oip_interband_correlate(oip_ctx *ctx, const uint16_t *d_pan, long Lp, long prow0, long pn,
                                       const uint16_t *d_planes, size_t plane_stride, long mrow0, long mn, int W,
                                       int slices, int sections, int corr_lines, double *out)
{
    OIP_CHECK_CTX(ctx);
    if (!d_pan || !d_planes || !out) return oip_fail(ctx, OIP_E_INVALID, "oip_interband_correlate: bad argument");
    OIPGPU::InterBandGeom g;
    const std::string refused = OIPGPU::MakeInterBandGeom(W, Lp, slices, sections, corr_lines, &g);
    if (!refused.empty()) return oip_fail(ctx, OIP_E_INVALID, "%s", refused.c_str());
    std::vector<int> which;
    std::vector<IbUnit> units;
    for (int sec = 0; sec < sections; ++sec) {
        const long p0 = g.pan_start(sec), m0 = g.mss_start(sec);
        if (p0 < prow0 || p0 + g.base_rows > prow0 + pn) continue;
        if (m0 < mrow0 || m0 + g.band_rows > mrow0 + mn) continue;
        for (int i = 0; i < slices; ++i) {
            which.push_back(sec * slices + i);
            IbUnit u;
            u.pan = d_pan + (size_t)(p0 - prow0) * W + (size_t)i * g.base_cols;
            u.pan_pitch = W;
            for (int b = 0; b < OIP_MSS_BANDS; ++b)
                u.band[b] = d_planes + (size_t)b * plane_stride + (size_t)(m0 - mrow0) * g.Wb + (size_t)i * g.band_cols;
            u.band_pitch = g.Wb;
            units.push_back(u);
        }
    }
    std::vector<double> r(12 * units.size() + 12);
    int rc = interband_units(ctx, CorrKnobs::from_env(), units.data(), (int)units.size(), g.base_rows, g.base_cols, g.band_rows, g.band_cols, r.data());
    if (rc) return rc;
    OIPGPU::ShiftTableInit(g, out);
    for (size_t j = 0; j < which.size(); ++j) OIPGPU::ShiftTablePut(g, out, which[j], &r[12 * j]);
    return OIP_OK;
}
