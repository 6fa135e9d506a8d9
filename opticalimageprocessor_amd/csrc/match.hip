// match.hip -- the device side of `oip regcheck`: dense template matching of two u16 rasters on a grid of tiles by zero-mean
// normalised cross-correlation in the spatial domain.  The reference has no counterpart; the point of the kernel is that it
// shares nothing with phasecorr.hip, whose results it is there to judge.  Definition: include/oip_c.h (oip_match_tiles_u16),
// restated in tests/_regcheck_ref.py.
//
//   per tile:    sa = sum a, saa = sum a^2 over the T x T template of A; bad_a, bad_b: samples outside [valid_min, valid_max]
//   per offset:  sb = sum b, sbb = sum b^2, sab = sum a b over B's window at (ty + dy, tx + dx), (dy, dx) in [-S, S]^2
//   score = (n sab - sa sb) / sqrt((n saa - sa^2) (n sbb - sb^2)) in fp64 from the exact integers; the peak and the sums at
//   the peak and its four neighbours make the tile's record of 20 uint64.
//
// Mapping.  One workgroup of 256 lanes per tile.  The template (T^2 samples) and B's search window ((T + 2S)^2) are staged in
// LDS -- 18 KB at T = 64, S = 4; 82 KB at T = 128, S = 16 -- from either stride (1, or 4: one band of a chunky raster) with
// 64-bit addresses, and sa, saa and the two counts are taken from the values on their way in.  The (2S + 1)^2 offsets times P
// row partitions are the work items (P = 256 / offsets, at most T: 3 at S = 4, 1 at S = 16 where an item loop of 5 passes
// runs); an item owns one offset and the template rows p, p + P, ...  Consecutive lanes own consecutive dx, so a wave reads
// consecutive u16 of the window and the same 16 bytes of the template (one broadcast read per 8 samples).
//
// Exactness.  a, b < 2^16 and b = 256 bh + bl with bh, bl < 2^8: each of a bl, a bh, b bl, b bh is < 2^24, and a template row
// has at most 128 samples, so a row's five 32-bit partial sums stay below 128 * 2^24 = 2^31 (sum b below 2^23).  They are
// folded into 64-bit sums after every row: sab = sum(a bl) + 256 sum(a bh), likewise sbb.  Full-range data cannot overflow.
// The partitions' 64-bit sums meet in LDS; integer sums, so the order does not matter and the record does not depend on P.
//
// Cost per tile at T = 64, S = 4: 4096 + 5184 two-byte loads (18.6 KB), 81 * 4096 = 332 k sample-offsets of about 9 VALU
// and 1.1 LDS instructions each.  Measured (profiles/regcheck_kernel.json): the dense grid of a 30000 x 100000
// PAN pair, 7.3e5 tiles, in 65 ms -- 15 % of the time it takes to read and upload the two strips.
#include "oip_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kRec = OIP_MATCH_RECORD_WORDS;

struct MatchArgs {
    const uint16_t *a, *b;
    long pitch_a, pitch_b;
    int stride_a, stride_b;
    int T, S, P;
    int x0, step_x, nx;
    long y0, step_y;
    unsigned vmin, vmax;
    uint64_t *records, *sums;
};

__device__ __forceinline__ uint64_t wave_sum(uint64_t v)      // lane 0 of the wave holds the sum
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

// rows x cols samples at p (lines `pitch` samples apart, samples `stride` apart) into LDS; the lane's share of their sum, sum
// of squares and out-of-range count
__device__ __forceinline__ void stage(const uint16_t *p, long pitch, int stride, int cols, int count, unsigned vmin, unsigned vmax,
                                      uint16_t *dst, uint64_t &s, uint64_t &ss, uint64_t &bad)
{
    for (int e = threadIdx.x; e < count; e += kBlock) {
        const int r = e / cols, c = e - r * cols;
        const unsigned v = p[(long)r * pitch + (long)c * stride];
        dst[e] = (uint16_t)v;
        s += v;
        ss += (uint64_t)(v * v);                               // < 2^32
        bad += (v < vmin || v > vmax) ? 1u : 0u;
    }
}

__global__ __launch_bounds__(kBlock) void match_tiles_kernel(MatchArgs g)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int T = g.T, S = g.S, P = g.P;
    const int K = 2 * S + 1, nOff = K * K, Wn = T + 2 * S;
    const int items = nOff * P;
    uint16_t *sA = reinterpret_cast<uint16_t *>(smem);
    uint16_t *sB = sA + T * T;
    uint64_t *part = reinterpret_cast<uint64_t *>(smem + ((size_t)(T * T + Wn * Wn) * 2 + 15) / 16 * 16);     // [P][nOff][3]
    uint64_t *wsum = part + (size_t)items * 3;                                                                 // [kWaves][4]
    double *wbest = reinterpret_cast<double *>(wsum + kWaves * 4);                                               // [kWaves]
    int *wbest_o = reinterpret_cast<int *>(wbest + kWaves);                                                        // [kWaves]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const long tile = blockIdx.x;
    const long tj = tile / g.nx;
    const int ti = (int)(tile - tj * g.nx);
    const long ty = g.y0 + tj * g.step_y;
    const long tx = g.x0 + (long)ti * g.step_x;

    // ---- stage the template and the search window; the tile's own sums on the way
    uint64_t s = 0, ss = 0, bad_a = 0, unused0 = 0, unused1 = 0, bad_b = 0;
    stage(g.a + ty * g.pitch_a + tx * g.stride_a, g.pitch_a, g.stride_a, T, T * T, g.vmin, g.vmax, sA, s, ss, bad_a);
    stage(g.b + (ty - S) * g.pitch_b + (tx - S) * g.stride_b, g.pitch_b, g.stride_b, Wn, Wn * Wn, g.vmin, g.vmax, sB, unused0, unused1, bad_b);
    s = wave_sum(s);
    ss = wave_sum(ss);
    bad_a = wave_sum(bad_a);
    bad_b = wave_sum(bad_b);
    if (lane == 0) {
        wsum[wave * 4 + 0] = s;
        wsum[wave * 4 + 1] = ss;
        wsum[wave * 4 + 2] = bad_a;
        wsum[wave * 4 + 3] = bad_b;
    }
    __syncthreads();

    // ---- the sums of every offset: an item is (row partition p, offset o)
    for (int item = tid; item < items; item += kBlock) {
        const int p = item / nOff, o = item - p * nOff;
        const int oy = o / K, ox = o - oy * K;
        uint64_t sb = 0, sbb = 0, sab = 0;
        for (int r = p; r < T; r += P) {
            const uint16_t *ar = sA + r * T;
            const uint16_t *br = sB + (r + oy) * Wn + ox;
            unsigned s1 = 0, ql = 0, qh = 0, cl = 0, ch = 0;   // a row's partial sums: each < 2^31 (see the head of the file)
            for (int c = 0; c < T; c += 8) {
                const uint4 av = *reinterpret_cast<const uint4 *>(ar + c);      // 16-byte aligned: T is a multiple of 8
                const unsigned aw[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const unsigned a = (k & 1) ? aw[k >> 1] >> 16 : aw[k >> 1] & 0xffffu;
                    const unsigned b = br[c + k];
                    const unsigned bl = b & 0xffu, bh = b >> 8;
                    s1 += b;
                    ql += b * bl;
                    qh += b * bh;
                    cl += a * bl;
                    ch += a * bh;
                }
            }
            sb += s1;
            sbb += (uint64_t)ql + ((uint64_t)qh << 8);
            sab += (uint64_t)cl + ((uint64_t)ch << 8);
        }
        uint64_t *q = part + (size_t)item * 3;
        q[0] = sb;
        q[1] = sbb;
        q[2] = sab;
    }
    __syncthreads();

    const uint64_t sa = wsum[0] + wsum[4] + wsum[8] + wsum[12], saa = wsum[1] + wsum[5] + wsum[9] + wsum[13];
    const long n = (long)T * T;
    const long va = n * (long)saa - (long)sa * (long)sa;

    // ---- partitions -> one (sb, sbb, sab) per offset (kept in partition 0's slot, which only this lane touches), its score,
    // the lane's best: ascending o, so the first of equal scores stays
    double best = -3.0;
    int best_o = 0x7fffffff;
    for (int o = tid; o < nOff; o += kBlock) {
        uint64_t v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            uint64_t t = 0;
            for (int p = 0; p < P; ++p) t += part[((size_t)p * nOff + o) * 3 + k];
            v[k] = t;
            part[(size_t)o * 3 + k] = t;
        }
        if (g.sums) {
            uint64_t *q = g.sums + ((size_t)tile * nOff + o) * 3;
            q[0] = v[0];
            q[1] = v[1];
            q[2] = v[2];
        }
        const long vb = n * (long)v[1] - (long)v[0] * (long)v[0];
        if (va > 0 && vb > 0) {
            const long num = n * (long)v[2] - (long)sa * (long)v[0];
            const double sc = (double)num / sqrt((double)va * (double)vb);
            if (sc > best) {
                best = sc;
                best_o = o;
            }
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const double os = __shfl_down(best, d, 64);
        const int oo = __shfl_down(best_o, d, 64);
        if (os > best || (os == best && oo < best_o)) {
            best = os;
            best_o = oo;
        }
    }
    if (lane == 0) {
        wbest[wave] = best;
        wbest_o[wave] = best_o;
    }
    __syncthreads();                                            // (also: every offset's total is in part[o])

    // ---- the record
    if (tid == 0) {
        for (int k = 1; k < kWaves; ++k)
            if (wbest[k] > best || (wbest[k] == best && wbest_o[k] < best_o)) {
                best = wbest[k];
                best_o = wbest_o[k];
            }
        const int pk = best > -2.5 ? best_o : S * K + S;        // no offset has a score: the offset (0, 0)
        const int pj = pk / K, pi = pk - pj * K;
        uint64_t *rec = g.records + (size_t)tile * kRec;
        rec[0] = sa;
        rec[1] = saa;
        rec[2] = wsum[2] + wsum[6] + wsum[10] + wsum[14];
        rec[3] = wsum[3] + wsum[7] + wsum[11] + wsum[15];
        rec[4] = (uint64_t)pk;
        const int nj[5] = {pj, pj, pj, pj - 1, pj + 1}, ni[5] = {pi, pi - 1, pi + 1, pi, pi};
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const bool in = nj[k] >= 0 && nj[k] < K && ni[k] >= 0 && ni[k] < K;
            const uint64_t *q = part + (size_t)(in ? nj[k] * K + ni[k] : 0) * 3;
            rec[5 + 3 * k] = in ? q[0] : 0;
            rec[6 + 3 * k] = in ? q[1] : 0;
            rec[7 + 3 * k] = in ? q[2] : 0;
        }
    }
}

}  // namespace

extern "C" int oip_match_tiles_u16(oip_ctx *ctx, const uint16_t *d_a, long pitch_a, int stride_a, const uint16_t *d_b, long pitch_b,
                                   int stride_b, int w, long rows, int T, int S, int x0, long y0, int step_x, long step_y, int nx, long ny,
                                   int valid_min, int valid_max, uint64_t *d_records, uint64_t *d_sums)
{
    OIP_CHECK_CTX(ctx);
    if (T < OIP_MATCH_MIN_T || T > OIP_MATCH_MAX_T || T % 8 != 0 || S < 1 || S > OIP_MATCH_MAX_S)
        return oip_fail(ctx, OIP_E_INVALID, "oip_match_tiles_u16: T a multiple of 8 in 8..128 and 1 <= S <= 16 expected");
    if ((stride_a != 1 && stride_a != 4) || (stride_b != 1 && stride_b != 4))
        return oip_fail(ctx, OIP_E_INVALID, "oip_match_tiles_u16: a sample stride of 1 or 4 expected");
    if (w < 1 || rows < 1 || nx < 1 || ny < 1 || step_x < 1 || step_y < 1 || valid_min < 0 || valid_max > 65535 || valid_min > valid_max ||
        !d_a || !d_b || !d_records || ((uintptr_t)d_a & 1) || ((uintptr_t)d_b & 1) || ((uintptr_t)d_records & 7) || ((uintptr_t)d_sums & 7) ||
        (long)nx * ny >= (1L << 31) || rows >= (1L << 40) || step_y >= (1L << 31))
        return oip_fail(ctx, OIP_E_INVALID, "oip_match_tiles_u16: bad argument");
    if (pitch_a < (long)(w - 1) * stride_a + 1 || pitch_b < (long)(w - 1) * stride_b + 1)
        return oip_fail(ctx, OIP_E_INVALID, "oip_match_tiles_u16: a pitch is shorter than its line");
    // every search window inside w x rows: the template of the last tile ends at x0 + (nx - 1) step_x + T, its window S further
    if (x0 < S || y0 < S || (long)x0 + (long)(nx - 1) * step_x + T + S > (long)w || y0 + (ny - 1) * step_y + T + S > rows)
        return oip_fail(ctx, OIP_E_INVALID, "oip_match_tiles_u16: a search window leaves the %d x %ld image", w, rows);
    const int K = 2 * S + 1, nOff = K * K, Wn = T + 2 * S;
    const int P = nOff >= kBlock ? 1 : (kBlock / nOff < T ? kBlock / nOff : T);
    const size_t lds = ((size_t)(T * T + Wn * Wn) * 2 + 15) / 16 * 16 + ((size_t)nOff * P * 3 + kWaves * 4) * sizeof(uint64_t) +
                       kWaves * (sizeof(double) + sizeof(int));
    if (lds > 64 * 1024)
        OIP_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(match_tiles_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    OipProfScope prof(ctx, "match_tiles_kernel");
    MatchArgs g;
    g.a = d_a; g.b = d_b; g.pitch_a = pitch_a; g.pitch_b = pitch_b; g.stride_a = stride_a; g.stride_b = stride_b;
    g.T = T; g.S = S; g.P = P; g.x0 = x0; g.step_x = step_x; g.nx = nx; g.y0 = y0; g.step_y = step_y;
    g.vmin = (unsigned)valid_min; g.vmax = (unsigned)valid_max; g.records = d_records; g.sums = d_sums;
    hipLaunchKernelGGL(match_tiles_kernel, dim3((unsigned)((long)nx * ny)), dim3(kBlock), lds, ctx->stream, g);
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}
