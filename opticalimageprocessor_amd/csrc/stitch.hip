// stitch.hip -- the strip stitch on gfx950: the plain one, and the balanced and feathered ones of `oip stitch --balance /
// --feather / --balance-lines` (their moments pass is seam.hip).
//
// The plain stitch replaces the line loop of IMO::StitchBigRaw (imageop.h:340-351): output line i is
// left[i][0 : W-fold] followed by right[i][fold : W]  (fold = --fold-cols / 2, main.cpp:189).  The balanced ones have no
// counterpart in the reference, which cuts hard at the seam.  After prestitch the last 2*fold columns of image 1 and the first
// 2*fold columns of image 2 see the same ground; lines are handled in SAMPLE units as StitchTiff does (Ws = W*spp, fs =
// fold*spp; the channel of sample index j is j % spp):
//
//   oip_stitch_rows_u16            the cut
//   oip_stitch_balanced_u16        image 2 balanced (b' = (G b + O) in Q16), a linear blend of half-width h pixels around the
//                                  seam, and "no data" (a sample below valid_min) handled inside it
//   oip_stitch_balanced_lines_u16  the same with a (G, O) per line and channel from tables in HBM (entry r * spp + c)
//
// One walk, two forms.  A 2 B in / 2 B out copy whose only difficulty is alignment: the right half starts fs samples into its
// source line and Ws - fs samples into the output line, so source and destination are in general only 2-byte aligned relative
// to each other.  In the vector form (stitch_chunks_kernel) a lane owns one aligned 16-byte store of the output (8 samples;
// flat over the output raster, so a wave writes one aligned KiB whatever the line pitch), finds its line and column by one
// integer division, reads the five dwords covering its source span and funnel-shifts them by 16 bits when the source is
// odd-sample aligned; 4 chunks in flight per lane.  Three kinds of chunk:
//   left of the blend zone    copy of image 1, whatever the policy
//   right of it               image 2 through the policy: a copy, or one 64-bit multiply-add, a shift and a clamp per sample
//   touching it (or the seam) per sample, through the policy: both images' samples and the blend's division
//                             (2h*spp/8 + 2 chunks of a line at most)
// Anything the vector form cannot take (an output line that is not a multiple of 8 samples, misaligned bases, an odd sample
// count) goes to the per-sample form (stitch_samples_kernel).  What differs between the three stitches is a policy struct
// passed by value: where the (G, O) pairs come from and what they do to a sample.
//   PlainCopy      no pairs; the blend zone is empty (z0 == z1 == half)
//   ConstPairs     the pairs of the strip, read once at kernel start: with the output line a multiple of 8 samples a chunk
//                  starts at channel 0, so the lane's four pairs are loop constants
//   LinePairs<SPP> the pairs of line r, read per chunk and per lane next to the image samples -- one dword from either table at
//                  SPP 1, one 16-byte load from either at SPP 4 (tables off a 16-byte boundary: the per-sample form) -- which
//                  the thousands of chunks of a line share through L2.  A chunk or sample left of the blend zone reads no entry.
// The arithmetic is stated once (balance_px, seam_sample), so equal pairs on every line give ConstPairs's bytes, and G = 65536,
// O = 0, h = 0 give PlainCopy's.
#include "oip_internal.h"

namespace {

constexpr int kBlock = 256;

// 8 consecutive u16 starting at element index `e` of `p` (e may be odd), as 4 dwords.  The dwords covering the span are
// clamped to the last one that holds a valid element; lanes never dereference outside the raster.
__device__ __forceinline__ uint4 load8_u16(const uint16_t *__restrict__ p, long e, long n_elems)
{
    const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
    const long d0 = e >> 1, dmax = (n_elems - 1) >> 1;
    uint32_t w[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const long di = d0 + i;
        w[i] = q[di > dmax ? dmax : di];
    }
    uint4 o;
    if (e & 1) {
        o.x = __builtin_amdgcn_alignbit(w[1], w[0], 16);
        o.y = __builtin_amdgcn_alignbit(w[2], w[1], 16);
        o.z = __builtin_amdgcn_alignbit(w[3], w[2], 16);
        o.w = __builtin_amdgcn_alignbit(w[4], w[3], 16);
    } else {
        o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3];
    }
    return o;
}

__device__ __forceinline__ uint4 pack8(const unsigned (&t)[8])
{
    return make_uint4(t[0] | (t[1] << 16), t[2] | (t[3] << 16), t[4] | (t[5] << 16), t[6] | (t[7] << 16));
}

// b' = clamp((G b + O + 32768) >> 16, 0, 65535), 64-bit, arithmetic shift.  t >> 16 lies in 0..65535 exactly when the high
// dword of t is zero; a negative high dword clamps to 0, a positive one to 65535.  orr = O + 32768 as 64 bits.
__device__ __forceinline__ unsigned balance_px(unsigned b, int G, long long orr)
{
    const long long t = (long long)G * (long long)(int)b + orr;
    const int hi = (int)(t >> 32);
    const unsigned lo = (unsigned)t;
    return hi == 0 ? lo >> 16 : (hi < 0 ? 0u : 65535u);
}

struct SeamGeom {
    long Ws;           // samples per input line
    int half;          // Ws - fs: samples an output line takes from either image
    int off_b;         // Ws - 2 fs: output sample x pairs with sample x - off_b of image 2
    int z0, z1;        // the blend zone in output samples: [half - h*spp, half + h*spp)
    int spp_shift;     // log2(spp)
    unsigned h2, h4;   // 2h, 4h
    unsigned vmin;     // samples below it are "no data" inside the blend zone
};

// output sample x of line r, any x; G / orr: those of channel x % spp
__device__ __forceinline__ unsigned seam_sample(const uint16_t *__restrict__ left, const uint16_t *__restrict__ right, const SeamGeom &g,
                                                long r, int x, int G, long long orr)
{
    if (x < g.z0) return left[r * g.Ws + x];
    const unsigned b = right[r * g.Ws + (x - g.off_b)];
    const unsigned bb = balance_px(b, G, orr);
    if (x >= g.z1) return bb;
    const unsigned a = left[r * g.Ws + x];
    if (a < g.vmin) return bb;
    if (b < g.vmin) return a;
    const unsigned wr = 2u * (unsigned)((x - g.z0) >> g.spp_shift) + 1u, wl = g.h4 - wr;
    return (wl * a + wr * bb + g.h2) / g.h4;          // 4h * 65535 + 2h < 2^32: h <= 16384, host-checked
}

// gain and offset + 32768 of channel k % spp in slot k: slot i % 4 of a chunk is the channel of its sample i
struct SeamPairs {
    int G[4];
    long long orr[4];
};
struct NoPairs {};

// the pairs of line r from per-line tables; at SPP 4 the table bases are 16-byte aligned
template <int SPP>
__device__ __forceinline__ void seam_line_pairs(const int *__restrict__ gain, const int *__restrict__ offset, long r, int (&G)[4], long long (&orr)[4])
{
    if (SPP == 4) {
        const int4 g4 = reinterpret_cast<const int4 *>(gain)[r], o4 = reinterpret_cast<const int4 *>(offset)[r];
        G[0] = g4.x; G[1] = g4.y; G[2] = g4.z; G[3] = g4.w;
        orr[0] = (long long)o4.x + 32768; orr[1] = (long long)o4.y + 32768; orr[2] = (long long)o4.z + 32768; orr[3] = (long long)o4.w + 32768;
    } else {
        const int g1 = gain[r];
        const long long o1 = (long long)offset[r] + 32768;
#pragma unroll
        for (int k = 0; k < 4; ++k) { G[k] = g1; orr[k] = o1; }
    }
}

// ---- policies ------------------------------------------------------------------------------------------------------
// z0 / z1: the blend zone [z0, z1) in output samples; start(): what a lane keeps for the whole kernel; pairs(k, r): what a
// chunk of line r that is not left of the zone works with; right8 / sample: 8 samples of image 2 right of the zone / sample
// x of a chunk that touches it (vector form); sample_at: output sample x of line r on its own (per-sample form).
struct PlainCopy {
    __device__ int z0(const SeamGeom &g) const { return g.half; }    // an empty zone at the seam
    __device__ int z1(const SeamGeom &g) const { return g.half; }
    __device__ NoPairs start() const { return {}; }
    __device__ NoPairs pairs(NoPairs, long) const { return {}; }
    __device__ uint4 right8(NoPairs, uint4 q) const { return q; }
    __device__ unsigned sample(NoPairs, const uint16_t *__restrict__ left, const uint16_t *__restrict__ right, const SeamGeom &g, long r, int x,
                               int) const
    {
        return x < g.half ? left[r * g.Ws + x] : right[r * g.Ws + (x - g.off_b)];
    }
    __device__ unsigned sample_at(const uint16_t *__restrict__ left, const uint16_t *__restrict__ right, const SeamGeom &g, long r, int x) const
    {
        return sample({}, left, right, g, r, x, 0);
    }
};

struct Balanced {                                  // what both balanced policies do with the pairs of a chunk
    const int *gain, *offset;
    __device__ int z0(const SeamGeom &g) const { return g.z0; }
    __device__ int z1(const SeamGeom &g) const { return g.z1; }
    __device__ uint4 right8(const SeamPairs &c, uint4 q) const
    {
        const unsigned t[8] = {balance_px(q.x & 0xffffu, c.G[0], c.orr[0]), balance_px(q.x >> 16, c.G[1], c.orr[1]),
                               balance_px(q.y & 0xffffu, c.G[2], c.orr[2]), balance_px(q.y >> 16, c.G[3], c.orr[3]),
                               balance_px(q.z & 0xffffu, c.G[0], c.orr[0]), balance_px(q.z >> 16, c.G[1], c.orr[1]),
                               balance_px(q.w & 0xffffu, c.G[2], c.orr[2]), balance_px(q.w >> 16, c.G[3], c.orr[3])};
        return pack8(t);
    }
    __device__ unsigned sample(const SeamPairs &c, const uint16_t *__restrict__ left, const uint16_t *__restrict__ right, const SeamGeom &g,
                               long r, int x, int slot) const
    {
        return seam_sample(left, right, g, r, x, c.G[slot], c.orr[slot]);
    }
};

struct ConstPairs : Balanced {
    int spp;
    __device__ SeamPairs start() const
    {
        SeamPairs k;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            k.G[i] = gain[i & (spp - 1)];
            k.orr[i] = (long long)offset[i & (spp - 1)] + 32768;
        }
        return k;
    }
    __device__ const SeamPairs &pairs(const SeamPairs &k, long) const { return k; }
    __device__ unsigned sample_at(const uint16_t *__restrict__ left, const uint16_t *__restrict__ right, const SeamGeom &g, long r, int x) const
    {
        const int c = x & (spp - 1);
        return seam_sample(left, right, g, r, x, gain[c], (long long)offset[c] + 32768);
    }
};

template <int SPP>
struct LinePairs : Balanced {
    __device__ NoPairs start() const { return {}; }
    __device__ SeamPairs pairs(NoPairs, long r) const
    {
        SeamPairs c;
        seam_line_pairs<SPP>(gain, offset, r, c.G, c.orr);
        return c;
    }
    __device__ unsigned sample_at(const uint16_t *__restrict__ left, const uint16_t *__restrict__ right, const SeamGeom &g, long r, int x) const
    {
        if (x < g.z0) return left[r * g.Ws + x];                      // a copy: no table entry is read
        const long e = r * SPP + (x & (SPP - 1));
        return seam_sample(left, right, g, r, x, gain[e], (long long)offset[e] + 32768);
    }
};

// ---- the walk ------------------------------------------------------------------------------------------------------
// requires: out base 16-byte aligned, (2*half) % 8 == 0, left/right bases 4-byte aligned, Ws * L even
template <class P>
__global__ __launch_bounds__(kBlock) void stitch_chunks_kernel(const uint16_t *__restrict__ left, const uint16_t *__restrict__ right,
                                                               uint16_t *__restrict__ out, SeamGeom g, long L, P p)
{
    const auto k = p.start();
    const int cpr = (2 * g.half) / 8;             // chunks per output line
    const long nchunks = (long)cpr * L;
    const long n_elems = g.Ws * L;
    constexpr int U = 4;
    const long stride = (long)gridDim.x * kBlock;
    for (long f0 = (long)blockIdx.x * kBlock + threadIdx.x; f0 < nchunks; f0 += stride * U) {
        uint4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long f = f0 + u * stride;
            if (f >= nchunks) break;
            const long r = f / cpr;
            const int x0 = (int)(f - r * cpr) * 8;
            if (x0 + 8 <= p.z0(g)) {
                v[u] = load8_u16(left, r * g.Ws + x0, n_elems);
                continue;
            }
            const auto c = p.pairs(k, r);
            if (x0 >= p.z1(g)) {
                v[u] = p.right8(c, load8_u16(right, r * g.Ws + (x0 - g.off_b), n_elems));
            } else {
                unsigned t[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) t[i] = p.sample(c, left, right, g, r, x0 + i, i & 3);
                v[u] = pack8(t);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long f = f0 + u * stride;
            if (f >= nchunks) break;
            reinterpret_cast<uint4 *>(out)[f] = v[u];
        }
    }
}

template <class P>
__global__ __launch_bounds__(kBlock) void stitch_samples_kernel(const uint16_t *__restrict__ left, const uint16_t *__restrict__ right,
                                                                uint16_t *__restrict__ out, SeamGeom g, long L, P p)
{
    const long ow = 2L * g.half;
    const long n = ow * L;
    const long stride = (long)gridDim.x * kBlock;
    for (long i = (long)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const long r = i / ow;
        out[i] = (uint16_t)p.sample_at(left, right, g, r, (int)(i - r * ow));
    }
}

// In-place sample permutation of an interleaved 4-channel image: sample i of every pixel becomes sample order[i].  A lane
// owns two pixels (one 16-byte load and store of its own: in place is safe); `sel` holds the four selectors, 4 bits each.
__global__ __launch_bounds__(kBlock) void permute_u16x4_kernel(uint16_t *__restrict__ img, long npairs, long npix, unsigned sel)
{
    const long stride = (long)gridDim.x * kBlock;
    for (long f = (long)blockIdx.x * kBlock + threadIdx.x; f < npairs; f += stride) {
        if (2 * f + 1 < npix) {
            uint4 v = reinterpret_cast<uint4 *>(img)[f], o;
            const unsigned a[4] = {v.x & 0xffffu, v.x >> 16, v.y & 0xffffu, v.y >> 16};
            const unsigned b[4] = {v.z & 0xffffu, v.z >> 16, v.w & 0xffffu, v.w >> 16};
            o.x = a[sel & 3] | (a[(sel >> 4) & 3] << 16);
            o.y = a[(sel >> 8) & 3] | (a[(sel >> 12) & 3] << 16);
            o.z = b[sel & 3] | (b[(sel >> 4) & 3] << 16);
            o.w = b[(sel >> 8) & 3] | (b[(sel >> 12) & 3] << 16);
            reinterpret_cast<uint4 *>(img)[f] = o;
        } else {                                                        // the odd last pixel
            uint2 v = reinterpret_cast<uint2 *>(img)[2 * f], o;
            const unsigned a[4] = {v.x & 0xffffu, v.x >> 16, v.y & 0xffffu, v.y >> 16};
            o.x = a[sel & 3] | (a[(sel >> 4) & 3] << 16);
            o.y = a[(sel >> 8) & 3] | (a[(sel >> 12) & 3] << 16);
            reinterpret_cast<uint2 *>(img)[2 * f] = o;
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------
SeamGeom seam_geom(int Ws, int fs, int spp, int feather, int valid_min)
{
    SeamGeom g;
    g.Ws = Ws;
    g.half = Ws - fs;
    g.off_b = Ws - 2 * fs;
    g.z0 = g.half - feather * spp;
    g.z1 = g.half + feather * spp;
    g.spp_shift = spp == 4 ? 2 : 0;
    g.h2 = 2u * (unsigned)feather;
    g.h4 = 4u * (unsigned)feather;
    g.vmin = valid_min < 0 ? 0u : (unsigned)valid_min;
    return g;
}

// what the vector form requires of a call
bool stitch_fast(const SeamGeom &g, long L, const uint16_t *d_left, const uint16_t *d_right, const uint16_t *d_out)
{
    return ((2 * g.half) % 8 == 0) && (((uintptr_t)d_out & 15) == 0) && (((uintptr_t)d_left & 3) == 0) && (((uintptr_t)d_right & 3) == 0) &&
           (g.Ws * L >= 16 && (g.Ws * L) % 2 == 0);
}

// the vector form on a grid of at most `fast_per_cu` blocks per CU, or the per-sample form on at most `slow_per_cu`; either
// walks the rest with a grid stride
template <class P>
int stitch_launch(oip_ctx *ctx, bool fast, int fast_per_cu, int slow_per_cu, const uint16_t *d_left, const uint16_t *d_right, uint16_t *d_out,
                  const SeamGeom &g, long L, const P &p)
{
    const long per_block = fast ? (long)kBlock * 4 : kBlock;
    const long items = fast ? (long)(2 * g.half / 8) * L : 2L * g.half * L;
    const long cap = (long)ctx->cu_count * (fast ? fast_per_cu : slow_per_cu);
    long blocks = (items + per_block - 1) / per_block;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    if (fast)
        hipLaunchKernelGGL(stitch_chunks_kernel<P>, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, d_left, d_right, d_out, g, L, p);
    else
        hipLaunchKernelGGL(stitch_samples_kernel<P>, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, d_left, d_right, d_out, g, L, p);
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}

// the two balanced entries' refusals; OIP_OK when the call may go on
int balanced_check(oip_ctx *ctx, const char *fn, const uint16_t *d_left, const uint16_t *d_right, const uint16_t *d_out, int Ws, long L, int fs,
                   int spp, const int32_t *d_gain, const int32_t *d_offset, int feather, int valid_min)
{
    if (!d_left || !d_right || !d_out || !d_gain || !d_offset || ((uintptr_t)d_gain & 3) || ((uintptr_t)d_offset & 3) || ((uintptr_t)d_left & 1) ||
        ((uintptr_t)d_right & 1) || ((uintptr_t)d_out & 1) || (spp != 1 && spp != 4) || Ws <= 0 || Ws % spp != 0 || fs < 0 || fs % spp != 0 ||
        fs >= Ws || L < 0 || feather < 0 || (long)feather * spp > fs || valid_min > 65535)
        return oip_fail(ctx, OIP_E_INVALID, "%s: bad argument", fn);
    if (feather > 16384) return oip_fail(ctx, OIP_E_UNSUPPORTED, "%s: feather above 16384 pixels (the blend's 32-bit numerator)", fn);
    return OIP_OK;
}

}  // namespace

extern "C" int oip_permute_u16x4(oip_ctx *ctx, uint16_t *d_img, size_t npixels, const int *order)
{
    OIP_CHECK_CTX(ctx);
    if (!order || (!d_img && npixels)) return oip_fail(ctx, OIP_E_INVALID, "oip_permute_u16x4: bad argument");
    unsigned sel = 0;
    for (int i = 0; i < 4; ++i) {
        if (order[i] < 0 || order[i] > 3) return oip_fail(ctx, OIP_E_INVALID, "oip_permute_u16x4: sample index outside 0..3");
        sel |= (unsigned)order[i] << (4 * i);
    }
    if (((uintptr_t)d_img & 15) != 0) return oip_fail(ctx, OIP_E_INVALID, "oip_permute_u16x4: image not 16-byte aligned");
    if (npixels == 0 || sel == 0x3210u) return OIP_OK;
    OipProfScope prof(ctx, "permute_u16x4_kernel");
    const long npairs = (long)((npixels + 1) / 2);
    long blocks = (npairs + kBlock - 1) / kBlock;
    const long cap = (long)ctx->cu_count * 64;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(permute_u16x4_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, d_img, npairs, (long)npixels, sel);
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}

extern "C" int oip_stitch_rows_u16(oip_ctx *ctx, const uint16_t *d_left, const uint16_t *d_right, uint16_t *d_out,
                                   int W, long L, int fold)
{
    OIP_CHECK_CTX(ctx);
    if (!d_left || !d_right || !d_out || W <= 0 || L < 0 || fold < 0 || fold >= W)
        return oip_fail(ctx, OIP_E_INVALID, "oip_stitch_rows_u16: bad argument");
    if (L == 0) return OIP_OK;
    OipProfScope prof(ctx, "stitch_rows_kernel");
    const SeamGeom g = seam_geom(W, fold, 1, 0, 0);
    return stitch_launch(ctx, stitch_fast(g, L, d_left, d_right, d_out), 128, 32, d_left, d_right, d_out, g, L, PlainCopy{});
}

extern "C" int oip_stitch_balanced_u16(oip_ctx *ctx, const uint16_t *d_left, const uint16_t *d_right, uint16_t *d_out, int Ws, long L, int fs,
                                       int spp, const int32_t *d_gain_q16, const int32_t *d_offset_q16, int feather, int valid_min)
{
    OIP_CHECK_CTX(ctx);
    const int rc = balanced_check(ctx, "oip_stitch_balanced_u16", d_left, d_right, d_out, Ws, L, fs, spp, d_gain_q16, d_offset_q16, feather, valid_min);
    if (rc != OIP_OK || L == 0) return rc;
    OipProfScope prof(ctx, "stitch_balanced_kernel");
    const SeamGeom g = seam_geom(Ws, fs, spp, feather, valid_min);
    return stitch_launch(ctx, stitch_fast(g, L, d_left, d_right, d_out), 8, 8, d_left, d_right, d_out, g, L,
                         ConstPairs{{d_gain_q16, d_offset_q16}, spp});
}

extern "C" int oip_stitch_balanced_lines_u16(oip_ctx *ctx, const uint16_t *d_left, const uint16_t *d_right, uint16_t *d_out, int Ws, long L, int fs,
                                             int spp, const int32_t *d_line_gain_q16, const int32_t *d_line_offset_q16, int feather, int valid_min)
{
    OIP_CHECK_CTX(ctx);
    const int rc = balanced_check(ctx, "oip_stitch_balanced_lines_u16", d_left, d_right, d_out, Ws, L, fs, spp, d_line_gain_q16, d_line_offset_q16,
                                  feather, valid_min);
    if (rc != OIP_OK || L == 0) return rc;
    OipProfScope prof(ctx, "stitch_balanced_lines_kernel");
    const SeamGeom g = seam_geom(Ws, fs, spp, feather, valid_min);
    const bool tables16 = spp == 1 || ((((uintptr_t)d_line_gain_q16 | (uintptr_t)d_line_offset_q16) & 15) == 0);
    const bool fast = stitch_fast(g, L, d_left, d_right, d_out) && tables16;
    if (spp == 1) return stitch_launch(ctx, fast, 8, 8, d_left, d_right, d_out, g, L, LinePairs<1>{{d_line_gain_q16, d_line_offset_q16}});
    return stitch_launch(ctx, fast, 8, 8, d_left, d_right, d_out, g, L, LinePairs<4>{{d_line_gain_q16, d_line_offset_q16}});
}
