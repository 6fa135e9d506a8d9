// tiffdeflate.hip -- the Deflate strips and tiles of a TIFF file (compression 8 / 32946) inflated on the GPU.
//
// The sibling of the LZW decoder in tifflzw.hip, behind the same reader (oip_host.hpp::read_tiff_to_device), with another shape:
// a lane of its own per strip does not carry over, because a decoder's Huffman tables plus its 32 KiB of history do not fit 64
// times into a CU.  Here a stream is a WAVE, in a single-wave workgroup:
//   - the history is a 32 KiB ring in LDS; matches read the ring, never the image in HBM;
//   - the Huffman tables (10-bit literal/length and 8-bit distance primaries, canonical counts for the longer codes) are in LDS
//     and rebuilt per dynamic block, the primaries by the 64 lanes;
//   - 2 KiB of input are staged in LDS at a time, loaded coalesced;
//   - every lane holds the same bit buffer and decodes the same symbol (table reads are broadcasts); lane 0 stores a literal, the
//     lanes copy a match together, and the ring goes to the image in 16-byte words whenever 16 KiB of it are new -- with the
//     Adler-32 of the bytes as they leave.
// About 38 KiB of LDS a workgroup: four resident waves per CU.  The decoder itself is csrc/oip_inflate.h, the code the host's
// threads run and the sanitizers have seen; this file gives it its lanes.  Predictor 2 is undone by a second kernel, a wave per
// image row (rows are independent; mod-2^16 sums in any order give the same bytes).
//
// The other direction, the Deflate strips and tiles of a product (oip_tiff_deflate_strips_u16, below the decoder): the encoder of
// csrc/oip_deflate.h with the same shape -- a stream is a wave in a single-wave workgroup.  The 32 KiB input ring, the 4096-entry
// hash table, the block's token record (two bits per position, a word per match), the histograms, the codes and the 512-byte
// bit buffer are LDS, about 66 KiB a workgroup: two resident waves per CU.  The lanes stage the input (the predictor-2
// differences of the image's rows, made while they are staged: the image is only read), hash and compare the 64 positions of a
// round, count the literals, rank the symbols by frequency, and place a block's codes by a prefix sum of their bit counts; one
// lane walks a round's 64 candidates and builds the code lengths.  Nothing of a stream is kept in HBM but its output: the streams
// land in fixed slots of the stored bound's size and oip_tiffpack.h packs them, as for LZW.
#include "oip_internal.h"
#include "oip_deflate.h"
#include "oip_inflate.h"
#include "oip_tiffdecode.h"
#include "oip_tiffpack.h"

#include <cstdint>
#include <memory>
#include <vector>

namespace {

constexpr long kStreamsPerLaunch = 1L << 20;

struct WaveLane {
    __device__ unsigned lane() const { return threadIdx.x; }
    __device__ unsigned nlanes() const { return 64; }
    __device__ void sync() const { __syncthreads(); }
    __device__ unsigned sum(unsigned v) const
    {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        return v;
    }
    __device__ unsigned uni(unsigned v) const { return (unsigned)__builtin_amdgcn_readfirstlane((int)v); }
};

struct DeflateJob {
    const uint8_t *file;
    const unsigned long long *off, *len;         // [nstrips]: stream offsets inside `file`, byte counts
    long rows;
    int width, spp;
    long rps, nstrips, strip0;
    uint16_t *img;
    unsigned *got;                               // [nstrips] bytes a stream decoded to
    int *status;                                 // [nstrips] oipinflate::Status
};

__global__ __launch_bounds__(64) void deflate_decode_kernel(DeflateJob j)
{
    __shared__ oipinflate::Shared sh;
    const long k = j.strip0 + blockIdx.x;
    if (k >= j.nstrips) return;
    const size_t rowBytes = (size_t)j.width * j.spp * 2;
    const long r0 = k * j.rps;
    long nr = j.rows - r0;
    if (nr > j.rps) nr = j.rps;
    uint8_t *out = reinterpret_cast<uint8_t *>(j.img) + (size_t)r0 * rowBytes;
    const unsigned cap = (unsigned)((size_t)nr * rowBytes);
    WaveLane lanes;
    // (the stream's place and size are the same in every lane of the workgroup: scalar registers)
    const unsigned long long off = ((unsigned long long)lanes.uni((unsigned)(j.off[k] >> 32)) << 32) | lanes.uni((unsigned)j.off[k]);
    oipinflate::Decoder<WaveLane> d(lanes, sh, j.file + off, lanes.uni((unsigned)j.len[k]), out, cap);
    unsigned got = 0;
    const int st = d.run(&got);
    if (threadIdx.x == 0) { j.got[k] = got; j.status[k] = st; }
}

// four 16-bit adds in one register: the low 15 bits of every field carry on their own, the top bits by xor (as tifflzw.hip)
__device__ __forceinline__ unsigned long long padd16(unsigned long long a, unsigned long long b)
{
    const unsigned long long m = 0x7fff7fff7fff7fffull;
    return ((a & m) + (b & m)) ^ ((a ^ b) & ~m);
}

// Predictor 2 undone: a wave per row, 64 pixels a round, an inclusive scan across the lanes plus the carry of the rounds before.
// FIELDS = 4: a pixel is four samples in one 64-bit word; 1: one sample.  Rows of a stream that failed are left as they are.
template <int FIELDS>
__global__ __launch_bounds__(64) void deflate_unpredict_kernel(uint16_t *img, long rows, int width, long rps, const unsigned *got, const int *status)
{
    const long r = blockIdx.x;
    if (r >= rows) return;
    const long k = r / rps;
    const long nr = rows - k * rps < rps ? rows - k * rps : rps;
    if (status[k] != 0 || (size_t)got[k] != (size_t)nr * width * FIELDS * 2) return;
    uint16_t *row = img + (size_t)r * width * FIELDS;
    const int lane = threadIdx.x;
    unsigned long long carry = 0;
    for (int x0 = 0; x0 < width; x0 += 64) {
        const int x = x0 + lane;
        unsigned long long v = 0;
        if (x < width) v = FIELDS == 4 ? reinterpret_cast<const unsigned long long *>(row)[x] : (unsigned long long)row[x];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long t = __shfl_up(v, d, 64);
            if (lane >= d) v = padd16(v, t);
        }
        v = padd16(v, carry);
        if (x < width) {
            if (FIELDS == 4) reinterpret_cast<unsigned long long *>(row)[x] = v;
            else row[x] = (uint16_t)v;
        }
        carry = __shfl(v, 63, 64);                                             // (lanes past the row's end added zeros)
    }
}

// any other number of samples: lane c of the row's wave walks channel c
__global__ __launch_bounds__(64) void deflate_unpredict_any_kernel(uint16_t *img, long rows, int width, int spp, long rps, const unsigned *got, const int *status)
{
    const long r = blockIdx.x;
    if (r >= rows || (int)threadIdx.x >= spp) return;
    const long k = r / rps;
    const long nr = rows - k * rps < rps ? rows - k * rps : rps;
    if (status[k] != 0 || (size_t)got[k] != (size_t)nr * width * spp * 2) return;
    uint16_t *row = img + (size_t)r * width * spp + threadIdx.x;
    unsigned prev = row[0];
    for (long x = 1; x < width; ++x) { prev = (prev + row[x * spp]) & 0xffffu; row[x * spp] = (uint16_t)prev; }
}

// ---- encode --------------------------------------------------------------------------------------------------------------------
constexpr long kEncodeStreamsPerLaunch = 32768;

struct WaveLaneEnc : WaveLane {
    __device__ unsigned scan(unsigned v) const                                 // exclusive prefix sum over the 64 lanes
    {
        unsigned s = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned t = __shfl_up(s, d, 64);
            if ((int)threadIdx.x >= d) s += t;
        }
        return s - v;
    }
    __device__ void amax(unsigned *p, unsigned v) const { atomicMax(p, v); }
    __device__ void inc(unsigned *p) const { atomicAdd(p, 1u); }
    __device__ void aor(unsigned *p, unsigned v) const { atomicOr(p, v); }
};

// byte i of a strip's stream: the little-endian bytes of (sample - the same channel of the previous pixel) mod 2^16, rows restarting
struct PredictorSource {
    const uint16_t *img;                         // the strip's first sample
    unsigned rowSamples, spp;
    __device__ unsigned at(unsigned i) const
    {
        const unsigned s = i >> 1;
        unsigned v = img[s];
        if (s % rowSamples >= spp) v -= img[s - spp];
        return (v >> (8 * (i & 1u))) & 255u;
    }
};

struct DeflateEncJob {
    const uint16_t *img;
    long rows;
    int width, spp;
    long rps, nstrips, strip0;
    uint8_t *slots;
    size_t slot_bytes;                           // >= stored_bound of a full strip
    unsigned *len;                               // [nstrips]; 0: the encoder refused (cannot happen with slots of the stored bound)
};

__global__ __launch_bounds__(64) void deflate_encode_kernel(DeflateEncJob j)
{
    extern __shared__ __align__(16) unsigned char lds[];
    oipdeflate::Shared &sh = *reinterpret_cast<oipdeflate::Shared *>(lds);
    const long k = j.strip0 + blockIdx.x;
    if (k >= j.nstrips) return;
    const size_t rowSamples = (size_t)j.width * j.spp;
    const long r0 = k * j.rps;
    long nr = j.rows - r0;
    if (nr > j.rps) nr = j.rps;
    WaveLaneEnc lanes;
    const PredictorSource src{j.img + (size_t)r0 * rowSamples, (unsigned)rowSamples, (unsigned)j.spp};
    const unsigned n = (unsigned)((size_t)nr * rowSamples * 2);
    oipdeflate::Encoder<WaveLaneEnc, PredictorSource> e(lanes, sh, src, n, j.slots + (size_t)blockIdx.x * j.slot_bytes, (unsigned)oipdeflate::stored_bound(n));
    unsigned size = 0;
    const int st = e.run(&size);
    if (threadIdx.x == 0) j.len[k] = st == oipdeflate::kOk ? size : 0u;
}

// device scratch of one call: the output slots of a launch, the stream lengths and offsets
void deflate_scratch_layout(long nstrips, size_t slot_bytes, size_t *len, size_t *off, size_t *total)
{
    const long per = nstrips < kEncodeStreamsPerLaunch ? nstrips : kEncodeStreamsPerLaunch;
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    *len = up((size_t)per * slot_bytes);
    *off = *len + up((size_t)nstrips * sizeof(unsigned));
    *total = *off + up((size_t)nstrips * sizeof(unsigned long long));
}
size_t deflate_slot_bytes(size_t strip) { return (oipdeflate::stored_bound(strip) + 3) / 4 * 4; }
}  // namespace

// (oip_tiff_decode's refusals and two of its own: the row kernels take a row per workgroup, so fewer than 2^31 rows, and address the
// image as u16 whatever the number of samples, so a 2-byte aligned image; the LZW decoder needs neither)
extern "C" int oip_tiff_deflate_decode_u16(oip_ctx *ctx, const uint8_t *d_file, size_t file_bytes, const uint64_t *strip_off,
                                           const uint64_t *strip_len, long nstrips, long rows, int width, int spp, long rows_per_strip,
                                           int predictor, uint16_t *d_img)
{
    OIP_CHECK_CTX(ctx);
    if (rows >= ((long)1 << 31)) return oip_fail(ctx, OIP_E_INVALID, "oip_tiff_deflate_decode_u16: 2^31 rows or more");
    if (((uintptr_t)d_img) & 1) return oip_fail(ctx, OIP_E_INVALID, "oip_tiff_deflate_decode_u16: image not 2-byte aligned");
    return oip_tiff_decode(ctx, "oip_tiff_deflate_decode_u16", "Deflate", oipinflate::status_text, oipinflate::kMaxStream, 0, d_file, file_bytes, strip_off,
                           strip_len, nstrips, rows, width, spp, rows_per_strip, predictor, d_img, [&](const OipTiffStreams &t) {
        for (long s0 = 0; s0 < nstrips; s0 += kStreamsPerLaunch) {
            const long ns = nstrips - s0 < kStreamsPerLaunch ? nstrips - s0 : kStreamsPerLaunch;
            DeflateJob j{d_file, t.off, t.len, rows, width, spp, rows_per_strip, nstrips, s0, d_img, t.got, t.status};
            OipProfScope prof(ctx, "deflate_decode_kernel");
            hipLaunchKernelGGL(deflate_decode_kernel, dim3((unsigned)ns), dim3(64), 0, ctx->stream, j);
        }
        if (predictor == 2 && width > 1) {
            OipProfScope prof(ctx, "deflate_unpredict_kernel");
            if (spp == 4) hipLaunchKernelGGL(deflate_unpredict_kernel<4>, dim3((unsigned)rows), dim3(64), 0, ctx->stream, d_img, rows, width, rows_per_strip, t.got, t.status);
            else if (spp == 1) hipLaunchKernelGGL(deflate_unpredict_kernel<1>, dim3((unsigned)rows), dim3(64), 0, ctx->stream, d_img, rows, width, rows_per_strip, t.got, t.status);
            else hipLaunchKernelGGL(deflate_unpredict_any_kernel, dim3((unsigned)rows), dim3(64), 0, ctx->stream, d_img, rows, width, spp, rows_per_strip, t.got, t.status);
        }
    });
}

extern "C" size_t oip_deflate_stream_host(const uint8_t *src, size_t n, uint8_t *dst, size_t cap)
{
    if ((!src && n) || !dst) return 0;
    std::unique_ptr<oipdeflate::Shared> work(new oipdeflate::Shared);
    return oipdeflate::deflate_host(src, n, dst, cap, work.get());
}

extern "C" size_t oip_tiff_deflate_worst_bytes(long rows, int width, int spp, long rows_per_strip)
{
    if (rows <= 0 || width <= 0 || spp <= 0 || rows_per_strip <= 0) return 0;
    const size_t strip = (size_t)rows_per_strip * width * spp * 2;
    const size_t nstrips = ((size_t)rows + rows_per_strip - 1) / rows_per_strip;
    return nstrips * (oipdeflate::stored_bound(strip) + 2);                    // (+ 2: to the next even offset, and the payload's even end)
}

extern "C" size_t oip_tiff_deflate_scratch_bytes(long rows, int width, int spp, long rows_per_strip)
{
    if (rows <= 0 || width <= 0 || spp <= 0 || rows_per_strip <= 0) return 0;
    const long nstrips = (rows + rows_per_strip - 1) / rows_per_strip;
    size_t a, b, total;
    deflate_scratch_layout(nstrips, deflate_slot_bytes((size_t)rows_per_strip * width * spp * 2), &a, &b, &total);
    return total;
}

extern "C" int oip_tiff_deflate_strips_u16(oip_ctx *ctx, const uint16_t *d_img, long rows, int width, int spp, long rows_per_strip,
                                           uint8_t *d_payload, size_t payload_cap, uint64_t *strip_off, uint64_t *strip_len,
                                           size_t *payload_bytes, void *d_scratch, size_t scratch_bytes)
{
    OIP_CHECK_CTX(ctx);
    if (!d_img || !d_payload || !strip_off || !strip_len || !payload_bytes || rows <= 0 || width <= 0 || (spp != 1 && spp != 4) ||
        rows_per_strip <= 0)
        return oip_fail(ctx, OIP_E_INVALID, "oip_tiff_deflate_strips_u16: bad argument");
    if ((((uintptr_t)d_img) & 1)) return oip_fail(ctx, OIP_E_INVALID, "oip_tiff_deflate_strips_u16: image not 2-byte aligned");
    if ((((uintptr_t)d_payload) & 1)) return oip_fail(ctx, OIP_E_INVALID, "oip_tiff_deflate_strips_u16: payload not 2-byte aligned");
    const long nstrips = (rows + rows_per_strip - 1) / rows_per_strip;
    const size_t strip = (size_t)rows_per_strip * width * spp * 2;
    if (strip > (1u << 30)) return oip_fail(ctx, OIP_E_INVALID, "oip_tiff_deflate_strips_u16: strip larger than 1 GiB");
    if (payload_cap < oip_tiff_deflate_worst_bytes(rows, width, spp, rows_per_strip))
        return oip_fail(ctx, OIP_E_INVALID, "oip_tiff_deflate_strips_u16: payload buffer too small");
    const size_t slot_bytes = deflate_slot_bytes(strip);
    const long per = nstrips < kEncodeStreamsPerLaunch ? nstrips : kEncodeStreamsPerLaunch;
    size_t o_len, o_off, need;
    deflate_scratch_layout(nstrips, slot_bytes, &o_len, &o_off, &need);
    void *own = nullptr;                         // scratch of this call's own when the caller brought none
    auto release = [&] { if (own) (void)hipFree(own); };
#define OIP_DEFLATE_HIP(call)                                                                                 \
    do {                                                                                                      \
        hipError_t e__ = (call);                                                                              \
        if (e__ != hipSuccess) {                                                                              \
            release();                                                                                        \
            return oip_fail(ctx, OIP_E_DEVICE, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
        }                                                                                                     \
    } while (0)
    if (d_scratch) {
        if (scratch_bytes < need || (((uintptr_t)d_scratch) & 7)) return oip_fail(ctx, OIP_E_INVALID, "oip_tiff_deflate_strips_u16: scratch too small or misaligned");
    } else {
        OIP_DEFLATE_HIP(hipMalloc(&own, need));
        d_scratch = own;
    }
    const size_t lds = sizeof(oipdeflate::Shared);
    static_assert(sizeof(oipdeflate::Shared) <= 80 * 1024, "two workgroups of the encoder per CU");
    OIP_DEFLATE_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(deflate_encode_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    uint8_t *d_slots = reinterpret_cast<uint8_t *>(d_scratch);
    unsigned *d_len = reinterpret_cast<unsigned *>((char *)d_scratch + o_len);
    unsigned long long *d_off = reinterpret_cast<unsigned long long *>((char *)d_scratch + o_off);
    std::vector<unsigned> len((size_t)nstrips);
    std::vector<unsigned long long> off((size_t)nstrips);
    size_t pos = 0;
    for (long s0 = 0; s0 < nstrips; s0 += per) {
        const long ns = nstrips - s0 < per ? nstrips - s0 : per;
        DeflateEncJob j{d_img, rows, width, spp, rows_per_strip, nstrips, s0, d_slots, slot_bytes, d_len};
        {
            OipProfScope prof(ctx, "deflate_encode_kernel");
            hipLaunchKernelGGL(deflate_encode_kernel, dim3((unsigned)ns), dim3(64), lds, ctx->stream, j);
        }
        OIP_DEFLATE_HIP(hipGetLastError());
        OIP_DEFLATE_HIP(hipMemcpyAsync(len.data() + s0, d_len + s0, (size_t)ns * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
        OIP_DEFLATE_HIP(hipStreamSynchronize(ctx->stream));
        for (long k = s0; k < s0 + ns; ++k) {
            if (len[(size_t)k] == 0 || len[(size_t)k] > slot_bytes) { release(); return oip_fail(ctx, OIP_E_RUNTIME, "oip_tiff_deflate_strips_u16: strip %ld was not encoded", k); }
            if (pos & 1) ++pos;                                                  // strips start on even offsets (oip_tiff.hpp)
            off[(size_t)k] = pos;
            pos += len[(size_t)k];
        }
        const size_t end = (pos + 1) & ~(size_t)1;
        if (end > payload_cap) { release(); return oip_fail(ctx, OIP_E_INVALID, "oip_tiff_deflate_strips_u16: payload buffer too small"); }
        OIP_DEFLATE_HIP(hipMemcpyAsync(d_off + s0, off.data() + s0, (size_t)ns * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
        {
            OipProfScope prof(ctx, "deflate_pack_kernel");
            hipLaunchKernelGGL(tiff_pack_kernel, dim3((unsigned)ns), dim3(256), 0, ctx->stream, d_slots, slot_bytes, d_len, d_off, s0, nstrips, d_payload);
        }
        OIP_DEFLATE_HIP(hipGetLastError());
        OIP_DEFLATE_HIP(hipStreamSynchronize(ctx->stream));                      // the slots and off[] are reused by the next launch
    }
#undef OIP_DEFLATE_HIP
    release();
    for (long k = 0; k < nstrips; ++k) { strip_off[k] = off[(size_t)k]; strip_len[k] = len[(size_t)k]; }
    *payload_bytes = pos;
    return OIP_OK;
}
