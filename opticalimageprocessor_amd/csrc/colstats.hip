// colstats.hip -- per-column count, sum and sum of squares of a u16 raster on gfx950: the one pass over a strip from which
// `oip rrc-calib` derives the "k , b" files that IMO::LoadRRCParamFile reads (imageop.h:140-192).  The reference has no
// counterpart (it only consumes such files); the sibling here is rrc.hip, which applies them.
//
//   n[x] += #valid,  S1[x] += sum v,  S2[x] += sum v*v        over the valid samples v of column x, exact integers
//
// Layout / mapping.  HBM-bound, read-only: 2 B per pixel in, 24 B per column and row block out.  As in rrc.hip a lane owns 8
// consecutive columns (one 16-byte load per line, four lines in flight) and walks a block of lines; grid.y cuts the lines
// into blocks.  A row block has at most 65536 lines, so n and S1 of a block fit 32-bit registers; S2 needs 64 bits.
// S2 form: `S2 += (uint64_t)(v * v)` on the exact 32-bit product, which hipcc lowers to v_mul_u32_u24 + v_lshl_add_u64 (two
// full-rate instructions per sample).  The other candidate, one 32 x 32 + 64 multiply-add per sample (v_mad_u64_u32), timed
// the same within the run-to-run spread on the MI355X (30000 x 100000: 1.071 ms against 1.086 ms; 12288 x 100000: 0.480
// against 0.471; spread 2 %): the kernel waits for HBM either way, so the form without a multi-pass instruction stays.
// Squares of several lines gathered in 32 bits are not an option: one square of a 16-bit sample already fills them.
//
// Cross-block reduction: 64-bit integer vector atomics (global_atomic_add_x2, no return) into d_acc, which makes the totals
// additive over calls as well.  An atomic wave-instruction is only fast when its 64 lanes hit consecutive addresses
// (MI355X: a wave whose lanes are 64 B apart is an order of magnitude slower), and a lane's 8 columns are 64 B apart from
// its neighbour's.  So a block transposes each plane through LDS first -- written [column-in-lane][lane] (conflict-free
// 8-byte stores), read with lane = column (rows padded by 4 entries: the 32 lanes of a read group then hit 32 different
// 8-byte banks) -- and every atomic instruction adds 512 contiguous bytes.  The row blocks are sized so that the grid is
// about one resident set of workgroups (8 per CU): the atomics of a block are then ~2 % of the bytes it reads.
//
// Anything the vector form cannot take (a pitch that is not a multiple of 8 pixels, a window that does not start on a
// 16-byte boundary) goes to the column-per-lane kernel: 2-byte loads, 128 contiguous bytes per wave and line.
#include "oip_internal.h"

namespace {

constexpr int kBlock = 256;
constexpr int kRowsInFlight = 4;
constexpr int kMaxBlockRows = 65536;         // 65536 * 65535 < 2^32: S1 of a row block in 32 bits
constexpr int kLdsRow = kBlock + 4;          // padded row of the transpose (see header)

// one sample into the running sums of its column; vspan = valid_max - valid_min
template <bool MASK>
__device__ __forceinline__ void colstats_px(unsigned v, unsigned vmin, unsigned vspan, unsigned &n, unsigned &s1, unsigned long long &s2)
{
    if (MASK) {
        const bool ok = v - vmin <= vspan;
        v = ok ? v : 0u;
        n += ok ? 1u : 0u;
    }
    s1 += v;
    s2 += (unsigned long long)(v * v);       // v < 2^16: the 32-bit product is exact
}

template <bool MASK>
__global__ __launch_bounds__(kBlock) void colstats_u16_kernel(const uint16_t *__restrict__ img, long pitch, int w, long rows,
                                                              unsigned vmin, unsigned vspan, unsigned long long *__restrict__ acc,
                                                              long rows_per_block)
{
    __shared__ unsigned long long sh[8 * kLdsRow];
    const int x0 = (blockIdx.x * kBlock + threadIdx.x) * 8;
    const long r0 = (long)blockIdx.y * rows_per_block;
    long r1 = r0 + rows_per_block;
    if (r1 > rows) r1 = rows;
    unsigned n[8], s1[8];
    unsigned long long s2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { n[i] = 0; s1[i] = 0; s2[i] = 0; }
    // (a partial last group still loads 16 bytes: the pitch is a multiple of 8 pixels -- host-checked -- so they lie inside
    // the line; its surplus columns are summed and never added)
    if (x0 < w) {
        auto line = [&](uint4 q) {
            const unsigned p[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                colstats_px<MASK>(p[i] & 0xffffu, vmin, vspan, n[2 * i], s1[2 * i], s2[2 * i]);
                colstats_px<MASK>(p[i] >> 16, vmin, vspan, n[2 * i + 1], s1[2 * i + 1], s2[2 * i + 1]);
            }
        };
        const uint16_t *s = img + r0 * pitch + x0;
        long r = r0;
        for (; r + kRowsInFlight <= r1; r += kRowsInFlight) {
            uint4 v[kRowsInFlight];
#pragma unroll
            for (int u = 0; u < kRowsInFlight; ++u) v[u] = *reinterpret_cast<const uint4 *>(s + u * pitch);
#pragma unroll
            for (int u = 0; u < kRowsInFlight; ++u) line(v[u]);
            s += kRowsInFlight * pitch;
        }
        for (; r < r1; ++r) {
            line(*reinterpret_cast<const uint4 *>(s));
            s += pitch;
        }
    }
    // block totals -> d_acc, one plane at a time through the LDS transpose (every lane takes part in the barriers)
    const int xb = blockIdx.x * kBlock * 8;
    auto flush = [&](int plane, auto value) {
#pragma unroll
        for (int i = 0; i < 8; ++i) sh[i * kLdsRow + threadIdx.x] = value(i);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = j * kBlock + threadIdx.x;                  // column of the block; its owner is lane c / 8, slot c % 8
            if (xb + c < w) atomicAdd(acc + (size_t)plane * w + xb + c, sh[(c & 7) * kLdsRow + (c >> 3)]);
        }
        __syncthreads();
    };
    if (MASK) {
        flush(0, [&](int i) { return (unsigned long long)n[i]; });
    } else {
        const unsigned long long all = (unsigned long long)(r1 - r0);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = j * kBlock + threadIdx.x;
            if (xb + c < w) atomicAdd(acc + xb + c, all);
        }
    }
    flush(1, [&](int i) { return (unsigned long long)s1[i]; });
    flush(2, [&](int i) { return s2[i]; });
}

// any pitch / alignment: a lane owns one column of the row block
template <bool MASK>
__global__ __launch_bounds__(kBlock) void colstats_u16_column_kernel(const uint16_t *__restrict__ img, long pitch, int w, long rows,
                                                                     unsigned vmin, unsigned vspan, unsigned long long *__restrict__ acc,
                                                                     long rows_per_block)
{
    const int x = blockIdx.x * kBlock + threadIdx.x;
    if (x >= w) return;
    const long r0 = (long)blockIdx.y * rows_per_block;
    long r1 = r0 + rows_per_block;
    if (r1 > rows) r1 = rows;
    unsigned n = 0, s1 = 0;
    unsigned long long s2 = 0;
    const uint16_t *s = img + r0 * pitch + x;
    long r = r0;
    for (; r + kRowsInFlight <= r1; r += kRowsInFlight) {
        unsigned v[kRowsInFlight];
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u) v[u] = s[u * pitch];
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u) colstats_px<MASK>(v[u], vmin, vspan, n, s1, s2);
        s += kRowsInFlight * pitch;
    }
    for (; r < r1; ++r) {
        colstats_px<MASK>(*s, vmin, vspan, n, s1, s2);
        s += pitch;
    }
    atomicAdd(acc + x, MASK ? (unsigned long long)n : (unsigned long long)(r1 - r0));
    atomicAdd(acc + (size_t)w + x, (unsigned long long)s1);
    atomicAdd(acc + 2 * (size_t)w + x, s2);
}

// grid.y: about `per_cu` workgroups per CU over the whole grid, a block of lines between 64 and kMaxBlockRows long.  (Not
// rrc.hip's row_blocks(): that one has no upper bound on a block's lines -- the 32-bit S1 needs one -- and aims at 16 short
// blocks per CU, where every block here ends in atomics and one resident set of longer blocks amortises them.)
inline void colstats_row_blocks(const oip_ctx *ctx, int gx, long rows, int per_cu, long *rows_per_block, int *gy)
{
    long want = (long)ctx->cu_count * per_cu / (gx > 0 ? gx : 1);
    if (want < 1) want = 1;
    long rpb = (rows + want - 1) / want;
    if (rpb < 64) rpb = 64;
    rpb = (rpb + kRowsInFlight - 1) / kRowsInFlight * kRowsInFlight;
    if (rpb > kMaxBlockRows) rpb = kMaxBlockRows;
    *rows_per_block = rpb;
    *gy = (int)((rows + rpb - 1) / rpb);     // rows < 2^31: at most 32768 blocks of kMaxBlockRows lines
}

}  // namespace

extern "C" int oip_colstats_u16(oip_ctx *ctx, const uint16_t *d_img, long pitch, int w, long rows, int valid_min, int valid_max,
                                uint64_t *d_acc)
{
    OIP_CHECK_CTX(ctx);
    if (w <= 0 || rows < 0 || rows >= (1L << 31) || pitch < w || !d_img || !d_acc || ((uintptr_t)d_acc & 7) || ((uintptr_t)d_img & 1) ||
        valid_min < 0 || valid_max > 65535 || valid_min > valid_max)
        return oip_fail(ctx, OIP_E_INVALID, "oip_colstats_u16: bad argument");
    if (rows == 0) return OIP_OK;
    const bool mask = !(valid_min == 0 && valid_max == 65535);
    const unsigned vmin = (unsigned)valid_min, vspan = (unsigned)(valid_max - valid_min);
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(d_acc);
    const bool vec = pitch % 8 == 0 && ((uintptr_t)d_img & 15) == 0;
    OipProfScope prof(ctx, vec ? "colstats_u16_kernel" : "colstats_u16_column_kernel");
    long rpb;
    int gy;
    if (vec) {
        const int gx = ((w + 7) / 8 + kBlock - 1) / kBlock;
        colstats_row_blocks(ctx, gx, rows, 8, &rpb, &gy);
        if (mask)
            hipLaunchKernelGGL(colstats_u16_kernel<true>, dim3(gx, gy), dim3(kBlock), 0, ctx->stream, d_img, pitch, w, rows, vmin, vspan, acc, rpb);
        else
            hipLaunchKernelGGL(colstats_u16_kernel<false>, dim3(gx, gy), dim3(kBlock), 0, ctx->stream, d_img, pitch, w, rows, vmin, vspan, acc, rpb);
    } else {
        const int gx = (w + kBlock - 1) / kBlock;
        colstats_row_blocks(ctx, gx, rows, 16, &rpb, &gy);
        if (mask)
            hipLaunchKernelGGL(colstats_u16_column_kernel<true>, dim3(gx, gy), dim3(kBlock), 0, ctx->stream, d_img, pitch, w, rows, vmin, vspan, acc, rpb);
        else
            hipLaunchKernelGGL(colstats_u16_column_kernel<false>, dim3(gx, gy), dim3(kBlock), 0, ctx->stream, d_img, pitch, w, rows, vmin, vspan, acc, rpb);
    }
    OIP_HIP(ctx, hipGetLastError());
    return OIP_OK;
}
