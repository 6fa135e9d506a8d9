// mtf.hip -- the two device passes of `oip mtf` on gfx950: slanted-edge tiles of a u16 raster (ISO 12233), from which the host
// derives the MTF at Nyquist across and along the lines.  The reference has no counterpart.
//
// A tile is 32 profiles of 32 samples taken along the axis (x: pieces of lines, y: pieces of columns), staggered by half a tile
// along the profile.  Pass 1 (oip_mtf_tiles_u16) gives every tile and channel a 16-byte record {status, s, Sc, Num}; pass 2
// (oip_mtf_esf_u16) bins the samples of the listed tiles into the 4x oversampled edge-spread function.  include/oip_c.h states
// every quantity in exact integers; tests/_mtf_ref.py restates them.
//
// Layout / mapping of pass 1.  Read-once, 16 B written per 1024 samples read.  A profile is two 16-sample segments, and the
// staggered neighbour of a tile shares one of them, so the unit of work is the segment: first and last sample, total variation,
// first moment of the differences, minimum and maximum.  Two segments combine into the profile's D, TV and S1 by integer
// identities (profile_of), so every sample is loaded once and reduced once.  Half a wave (32 lanes) owns a run of kRun tiles
// along the profile axis; lane r owns profile r and walks the run segment by segment, keeping the previous segment's six
// numbers.  The sums over the 32 profiles are wave shuffles inside the half; nothing goes through LDS.  Axis x at spp 1 with a
// 16-byte aligned window reads four segments (128 bytes of the lane's line) at a time with 16-byte loads; every other case (axis y, where the 32 lanes of a load
// read 32 adjacent columns, spp 4, odd pitches and starts) reads samples one by one through the same code.  The one integer
// division per profile is a 32-bit one; the line through the centroids divides by the constant 64 Den.
//
// Pass 2 runs one wave per listed tile: lane (r, h) owns half h of profile r, recomputes the record exactly as pass 1 does, then
// adds its 16 samples into the wave's 64 sums and counts in LDS; lane b stores bin b.
#include "oip_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kRun = 16;                     // tiles per half-wave along the profile axis: 17 segments loaded for 16 tiles
constexpr int kDen = 87296;                  // 32 * sum r^2 - (sum r)^2, r = 0..31

struct MtfParams {
    int contrast_min, tv_slack;
    unsigned vmin, vmax;
};

// what a 16-sample segment of a profile contributes
struct MtfSeg {
    int first, last, tv, s1;                 // s1 = sum (2 i + 1) (v[i + 1] - v[i]), i = 0..14
    unsigned mn, mx;
};

__device__ __forceinline__ MtfSeg mtf_seg(const unsigned v[16])
{
    MtfSeg s;
    s.first = (int)v[0];
    s.last = (int)v[15];
    s.tv = 0;
    s.s1 = 0;
    s.mn = s.mx = v[0];
#pragma unroll
    for (int i = 0; i < 15; ++i) {
        const int d = (int)v[i + 1] - (int)v[i];
        s.tv += d < 0 ? -d : d;
        s.s1 += (2 * i + 1) * d;
        s.mn = v[i + 1] < s.mn ? v[i + 1] : s.mn;
        s.mx = v[i + 1] > s.mx ? v[i + 1] : s.mx;
    }
    return s;
}

// a segment from two 16-byte loads, or from 16 samples `step` apart
__device__ __forceinline__ MtfSeg mtf_seg_of(const uint4 &a, const uint4 &b)
{
    const unsigned q[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    unsigned v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = (i & 1) ? q[i >> 1] >> 16 : q[i >> 1] & 0xffffu;
    return mtf_seg(v);
}
__device__ __forceinline__ MtfSeg mtf_load_seg(const uint16_t *__restrict__ p, long step)
{
    unsigned v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = p[i * step];
    return mtf_seg(v);
}

// D, TV and S1 (before the polarity) of the profile made of segments a (samples 0..15) and b (16..31): the difference across the
// joint has weight 2 * 15 + 1 = 31, and the weights of b's differences are 32 above their local ones
struct MtfProfile {
    int D, TV, S1;
    bool nodata;
};

__device__ __forceinline__ MtfProfile profile_of(const MtfSeg &a, const MtfSeg &b, const MtfParams &P)
{
    MtfProfile f;
    const int j = b.first - a.last;
    f.D = b.last - a.first;
    f.TV = a.tv + b.tv + (j < 0 ? -j : j);
    f.S1 = a.s1 + 31 * j + b.s1 + 32 * (b.last - b.first);
    f.nodata = a.mn < P.vmin || b.mn < P.vmin || a.mx > P.vmax || b.mx > P.vmax;
    return f;
}

// sums and minima over the 32 lanes of a half-wave (the masks stay below 32: a lane only ever reads its own half)
__device__ __forceinline__ int half_sum(int v)
{
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ int half_min(int v)
{
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) {
        const int o = __shfl_xor(v, m);
        v = o < v ? o : v;
    }
    return v;
}

struct MtfTile {
    int status, s, Sc, Num, sumD;
    int f;                                   // this lane's f_r; meaningful when the status is 0
};

// the record of a tile from its 32 profiles, one per lane of the half-wave (r = lane & 31).  A lane's code is the first test its
// own profile fails; the smallest code over the lanes is the first test any profile fails.
__device__ __forceinline__ MtfTile mtf_finish(int r, const MtfProfile &f, const MtfParams &P)
{
    MtfTile t;
    t.sumD = half_sum(f.D);
    t.s = (t.sumD > 0) - (t.sumD < 0);
    const int S0 = t.s * f.D, S1 = t.s * f.S1;
    int code = 8;
    unsigned c = 0u;
    if (f.nodata) code = 1;
    else if (S0 < P.contrast_min) code = 3;
    else if (4 * f.TV > 5 * S0 + 4 * P.tv_slack || S1 < 0) code = 4;
    else {
        // S1 <= 61 TV and 4 TV <= 5 * 65535 + 4 * 65535: 64 S1 < 2^30; S0 >= contrast_min >= 1
        c = (unsigned)(64 * S1) / (unsigned)S0;
        if (c < 1280u || c > 2688u) code = 5;
    }
    const int first = half_min(code);
    const int cc = first == 8 ? (int)c : 0;
    t.Sc = half_sum(cc);
    t.Num = 32 * half_sum(r * cc) - 496 * t.Sc;
    const int an = t.Num < 0 ? -t.Num : t.Num;
    const bool slant_ok = 4 * kDen <= an && an <= 32 * kDen;
    // with every c_r >= 1280 and |Num| <= 32 Den the numerator is positive: the division is the floor
    t.f = (int)((2ll * kDen * t.Sc + 32ll * t.Num * (2 * r - 31)) / (64ll * kDen));
    const int dev = cc - t.f;
    const unsigned long long bent = __ballot(first == 8 && slant_ok && (dev > 64 || dev < -64));
    const bool curved = (unsigned)(bent >> (threadIdx.x & 32)) != 0u;
    t.status = first == 1 ? 1 : t.sumD == 0 ? 2 : first < 8 ? first : !slant_ok ? 6 : curved ? 7 : 0;
    if (t.status != 0) t.s = t.Sc = t.Num = 0;
    return t;
}

// pass 1.  `along` tiles lie along the profile axis (x: tx, y: ty) and `across` the other way; ps / is are the distances in
// samples between profiles and between the samples of a profile.
template <bool VEC>
__global__ __launch_bounds__(kBlock) void mtf_tiles_u16_kernel(const uint16_t *__restrict__ img, long ps, long is, int spp, int axis, long along,
                                                               long across, MtfParams P, int32_t *__restrict__ rec, long rec_pitch,
                                                               size_t rec_plane_stride)
{
    const int r = threadIdx.x & 31;
    const long hw = (long)blockIdx.x * (kBlock / 32) + (threadIdx.x >> 5);
    const long nrun = (along + kRun - 1) / kRun;
    long run, a;
    int c;
    if (axis == 0) {                         // the halves of a wave take neighbouring runs of one line block
        run = hw % nrun;
        a = hw / nrun % across;
        c = (int)(hw / (nrun * across));
    } else {                                 // ... neighbouring column blocks of one run
        a = hw % across;
        run = hw / across % nrun;
        c = (int)(hw / (nrun * across));
    }
    if (c >= spp) return;
    const long t0 = run * kRun;
    const uint16_t *p = img + c + (a * 32 + r) * ps + t0 * 16 * is;
    // tile t0 + k from its two segments; it exists, so sample 16 (t0 + k) + 31 lies inside the window
    auto emit = [&](int k, const MtfSeg &first, const MtfSeg &second) {
        const MtfTile t = mtf_finish(r, profile_of(first, second, P), P);
        if (r < 4) {
            const long ty = axis == 0 ? a : t0 + k, tx = axis == 0 ? t0 + k : a;
            const int word = r == 0 ? t.status : r == 1 ? t.s : r == 2 ? t.Sc : t.Num;
            rec[((size_t)c * rec_plane_stride + (size_t)(ty * rec_pitch + tx)) * 4 + r] = word;
        }
    };
    MtfSeg prev;
    if (VEC) {
        // the run's kRun + 1 segments in groups of four: a lane asks for 128 bytes of its line at a time (the run starts on a
        // multiple of 512 bytes of the line), so that a cache line is fetched once and not once per segment; segment s of the
        // run exists while t0 + s <= along
        for (int g = 0; g <= kRun / 4; ++g) {
            const int ns = g < kRun / 4 ? 4 : 1;
            uint4 q[8];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < ns && t0 + 4 * g + j <= along) {
                    const uint4 *v = reinterpret_cast<const uint4 *>(p + (4 * g + j) * 16);
                    q[2 * j] = v[0];
                    q[2 * j + 1] = v[1];
                }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j >= ns || t0 + 4 * g + j > along) break;
                const MtfSeg cur = mtf_seg_of(q[2 * j], q[2 * j + 1]);
                if (4 * g + j > 0) emit(4 * g + j - 1, prev, cur);
                prev = cur;
            }
        }
    } else {
        prev = mtf_load_seg(p, is);
        for (int k = 0; k < kRun && t0 + k < along; ++k) {
            const MtfSeg cur = mtf_load_seg(p + (long)(k + 1) * 16 * is, is);
            emit(k, prev, cur);
            prev = cur;
        }
    }
}

// pass 2: one wave per listed tile; lane (r, h) owns samples 16 h .. 16 h + 15 of profile r
__global__ __launch_bounds__(64) void mtf_esf_u16_kernel(const uint16_t *__restrict__ img, long ps, long is, int axis, MtfParams P,
                                                         const int32_t *__restrict__ list, uint32_t *__restrict__ esf, int32_t *__restrict__ s0)
{
    __shared__ unsigned acc[128];
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int32_t *e = list + (size_t)blockIdx.x * 3;
    const long a = axis == 0 ? e[1] : e[2], t = axis == 0 ? e[2] : e[1];
    const uint16_t *p = img + e[0] + (a * 32 + r) * ps + (t * 16 + h * 16) * is;
    unsigned v[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = p[i * is];
    const MtfSeg mine = mtf_seg(v);
    MtfSeg other;
    other.first = __shfl_xor(mine.first, 32);
    other.last = __shfl_xor(mine.last, 32);
    other.tv = __shfl_xor(mine.tv, 32);
    other.s1 = __shfl_xor(mine.s1, 32);
    other.mn = __shfl_xor(mine.mn, 32);
    other.mx = __shfl_xor(mine.mx, 32);
    const MtfTile tile = mtf_finish(r, h ? profile_of(other, mine, P) : profile_of(mine, other, P), P);
    acc[lane] = 0u;
    acc[lane + 64] = 0u;
    __syncthreads();
    if (tile.status == 0) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int b = (128 * (16 * h + i) - tile.f + 1024) >> 5;
            if (b >= 0 && b < 64) {
                atomicAdd(&acc[b], v[i]);
                atomicAdd(&acc[64 + b], 1u);
            }
        }
    }
    __syncthreads();
    uint32_t *out = esf + (size_t)blockIdx.x * 128;
    out[lane] = acc[lane];
    out[lane + 64] = acc[lane + 64];
    if (s0 && lane == 0) s0[blockIdx.x] = tile.s * tile.sumD;          // sum S0_r; 0 unless the status is 0
}

// the arguments both passes share; on success the tile counts
int mtf_check(oip_ctx *ctx, const char *who, const void *d_src, long pitch, int w, long rows, int spp, int axis, int contrast_min, int tv_slack,
              int valid_min, int valid_max, long *nty, long *ntx)
{
    if ((axis != 0 && axis != 1) || (spp != 1 && spp != 4) || contrast_min < 1 || tv_slack < 0 || tv_slack > 65535 || valid_min < 0 ||
        valid_max > 65535 || valid_min > valid_max || w < 0 || rows < 0 || pitch < (long)w * spp || !d_src || ((uintptr_t)d_src & 1))
        return oip_fail(ctx, OIP_E_INVALID, "%s: bad argument", who);
    if (w < 32 || rows < 32) {
        *nty = *ntx = 0;
    } else if (axis == 0) {
        *nty = rows / 32;
        *ntx = (w - 32) / 16 + 1;
    } else {
        *nty = (rows - 32) / 16 + 1;
        *ntx = w / 32;
    }
    return OIP_OK;
}

}  // namespace

extern "C" int oip_mtf_tiles_u16(oip_ctx *ctx, const uint16_t *d_src, long pitch, int w, long rows, int spp, int axis, int contrast_min, int tv_slack,
                                 int valid_min, int valid_max, int32_t *d_rec, long rec_pitch, size_t rec_plane_stride)
{
    OIP_CHECK_CTX(ctx);
    long nty, ntx;
    const int rc = mtf_check(ctx, "oip_mtf_tiles_u16", d_src, pitch, w, rows, spp, axis, contrast_min, tv_slack, valid_min, valid_max, &nty, &ntx);
    if (rc) return rc;
    if (!d_rec || ((uintptr_t)d_rec & 3) || rec_pitch < ntx) return oip_fail(ctx, OIP_E_INVALID, "oip_mtf_tiles_u16: bad argument");
    if (nty == 0 || ntx == 0) return OIP_OK;
    if (spp == 4 && rec_plane_stride < (size_t)((nty - 1) * rec_pitch + ntx))
        return oip_fail(ctx, OIP_E_INVALID, "oip_mtf_tiles_u16: the record planes overlap");
    const long along = axis == 0 ? ntx : nty, across = axis == 0 ? nty : ntx;
    const long halves = (along + kRun - 1) / kRun * across * spp;
    const long blocks = (halves + kBlock / 32 - 1) / (kBlock / 32);
    if (blocks > 0x7fffffffl) return oip_fail(ctx, OIP_E_INVALID, "oip_mtf_tiles_u16: the window holds too many tiles for one call");
    const MtfParams P = {contrast_min, tv_slack, (unsigned)valid_min, (unsigned)valid_max};
    const long ps = axis == 0 ? pitch : spp, is = axis == 0 ? spp : pitch;
    const bool vec = axis == 0 && spp == 1 && pitch % 8 == 0 && ((uintptr_t)d_src & 15) == 0;
    OipProfScope prof(ctx, vec ? "mtf_tiles_u16_kernel" : "mtf_tiles_u16_any_kernel");
    if (vec)
        hipLaunchKernelGGL(mtf_tiles_u16_kernel<true>, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, d_src, ps, is, spp, axis, along, across, P,
                           d_rec, rec_pitch, rec_plane_stride);
    else
        hipLaunchKernelGGL(mtf_tiles_u16_kernel<false>, dim3((unsigned)blocks), dim3(kBlock), 0, ctx->stream, d_src, ps, is, spp, axis, along, across, P,
                           d_rec, rec_pitch, rec_plane_stride);
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}

extern "C" int oip_mtf_esf_u16(oip_ctx *ctx, const uint16_t *d_src, long pitch, int w, long rows, int spp, int axis, int contrast_min, int tv_slack,
                               int valid_min, int valid_max, const int32_t *d_list, long n, uint32_t *d_esf, int32_t *d_s0)
{
    OIP_CHECK_CTX(ctx);
    long nty, ntx;
    const int rc = mtf_check(ctx, "oip_mtf_esf_u16", d_src, pitch, w, rows, spp, axis, contrast_min, tv_slack, valid_min, valid_max, &nty, &ntx);
    if (rc) return rc;
    if (n < 0 || n > 0x7fffffffl || (n > 0 && (!d_list || !d_esf || ((uintptr_t)d_list & 3) || ((uintptr_t)d_esf & 3))) || ((uintptr_t)d_s0 & 3))
        return oip_fail(ctx, OIP_E_INVALID, "oip_mtf_esf_u16: bad argument");
    if (n == 0) return OIP_OK;
    // the list is checked on the host before anything is launched: an entry outside the window would read outside it
    std::vector<int32_t> list((size_t)n * 3);
    OIP_HIP(ctx, hipMemcpyAsync(list.data(), d_list, list.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    OIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (long k = 0; k < n; ++k) {
        const int32_t *e = &list[(size_t)k * 3];
        if (e[0] < 0 || e[0] >= spp || e[1] < 0 || e[1] >= nty || e[2] < 0 || e[2] >= ntx)
            return oip_fail(ctx, OIP_E_INVALID, "oip_mtf_esf_u16: entry %ld (channel %d, ty %d, tx %d) lies outside the %ld x %ld tiles of the window", k,
                            e[0], e[1], e[2], nty, ntx);
    }
    const MtfParams P = {contrast_min, tv_slack, (unsigned)valid_min, (unsigned)valid_max};
    const long ps = axis == 0 ? pitch : spp, is = axis == 0 ? spp : pitch;
    OipProfScope prof(ctx, "mtf_esf_u16_kernel");
    hipLaunchKernelGGL(mtf_esf_u16_kernel, dim3((unsigned)n), dim3(64), 0, ctx->stream, d_src, ps, is, axis, P, d_list, d_esf, d_s0);
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}
