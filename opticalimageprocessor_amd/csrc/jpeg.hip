// jpeg.hip -- the scan of a baseline JPEG file (the browse image of `oip quicklook --format jpeg`) encoded on the GPU.
//
// The sibling of the LZW and Deflate encoders (tifflzw.hip, tiffdeflate.hip) with the same shape: independent streams, here the
// restart intervals of the scan -- one per row of 8 x 8 blocks, so an interval reads its own 8 image lines and nothing else -- each
// coded by one WAVE in a single-wave workgroup running the coder of csrc/oip_jpeg.h, the code the host instantiation runs and the
// sanitizers have seen; this file gives it its lanes.  A lane takes one block a round (for RGB the lanes go Y, Cb, Cr, Y, ...):
// staging (with the colour conversion), DCT and quantisation in registers, the coefficients in zigzag order in LDS, a wave prefix
// sum of the lanes' bit counts, the codes or-ed into a bit buffer in LDS, a count over the 0xFF flags of every 64 bytes for the
// stuffing, byte stores.  About 29 KiB of LDS a workgroup: five resident waves per CU.
//
// The payload is packed without slots: the kernel runs twice, first storing nothing and returning every interval's length, then --
// the offsets being the running sum of the lengths -- storing every interval at its place, each store bounded by the length the
// first pass measured.  What an interval can take at most (416 bytes a block, oip_jpeg_worst_bytes) is therefore only a capacity
// the caller proves, never memory the coder touches; the price is the arithmetic done twice.
#include "oip_internal.h"
#include "oip_jpeg.h"

#include <cstdint>
#include <memory>
#include <vector>

namespace {

struct WaveLanes {
    __device__ unsigned lane() const { return threadIdx.x; }
    __device__ void sync() const { __syncthreads(); }
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
    __device__ unsigned sum(unsigned v) const
    {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        return v;
    }
    __device__ unsigned rank(bool f, unsigned *total) const
    {
        const unsigned long long m = __ballot(f);
        *total = (unsigned)__popcll(m);
        return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    }
    __device__ void aor(uint32_t *p, uint32_t v) const { atomicOr(p, v); }
    __device__ unsigned long long tick() const { return (unsigned long long)clock64(); }
};

struct JpegJob {
    const uint8_t *img;
    long pitch;
    int w;
    long h;
    int nch;
    const oipjpeg::Tables *tab;
    long intervals;
    uint8_t *payload;                            // null: measure only
    const unsigned long long *off;               // [intervals] (with a payload)
    unsigned *len;                               // [intervals]: written by the measuring pass, the bound of the storing one
    unsigned long long *cycles;                  // [5]: the storing pass's cycles per phase of the coder, summed over the waves
};

__global__ __launch_bounds__(64) void jpeg_scan_kernel(JpegJob j)
{
    __shared__ oipjpeg::Shared<64> sh;
    const long k = blockIdx.x;
    if (k >= j.intervals) return;
    static_assert(sizeof(oipjpeg::Tables) % 4 == 0, "the tables are copied by words");
    for (unsigned i = threadIdx.x; i < sizeof(oipjpeg::Tables) / 4; i += 64)
        reinterpret_cast<uint32_t *>(&sh.tab)[i] = reinterpret_cast<const uint32_t *>(j.tab)[i];
    __syncthreads();
    WaveLanes lanes;
    oipjpeg::Encoder<WaveLanes, 64> e(lanes, sh);
    if (!j.payload) {
        const size_t n = e.run(j.img, j.pitch, j.w, j.h, j.nch, k, nullptr, 0);
        if (threadIdx.x == 0) j.len[k] = (unsigned)n;
    } else {
        e.run(j.img, j.pitch, j.w, j.h, j.nch, k, j.payload + j.off[k], j.len[k]);
        if (threadIdx.x == 0)
            for (int i = 0; i < e.kPhases; ++i) atomicAdd(&j.cycles[i], e.cycles[i]);
    }
}

struct JpegPlan {
    bool ok;
    long intervals;
    size_t worst_bytes, scratch_bytes, o_len, o_off, o_cycles;
};

JpegPlan plan_jpeg(int w, long h, int nch)
{
    JpegPlan p{};
    if (w < 1 || w > 65535 || h < 1 || h > 65535 || (nch != 1 && nch != 3)) return p;
    p.ok = true;
    p.intervals = (h + 7) / 8;
    p.worst_bytes = (size_t)p.intervals * (size_t)((w + 7) / 8) * nch * oipjpeg::kBlockBytes;
    p.o_len = (sizeof(oipjpeg::Tables) + 7) & ~(size_t)7;
    p.o_off = p.o_len + (((size_t)p.intervals * sizeof(unsigned) + 7) & ~(size_t)7);
    p.o_cycles = p.o_off + (size_t)p.intervals * sizeof(unsigned long long);
    p.scratch_bytes = p.o_cycles + 5 * sizeof(unsigned long long);
    return p;
}

}  // namespace

extern "C" size_t oip_jpeg_worst_bytes(int w, long h, int nch) { return plan_jpeg(w, h, nch).worst_bytes; }

extern "C" size_t oip_jpeg_scratch_bytes(int w, long h, int nch) { return plan_jpeg(w, h, nch).scratch_bytes; }

extern "C" int oip_jpeg_scan_u8(oip_ctx *ctx, const uint8_t *d_img, long pitch_bytes, int w, long h, int nch, int quality, uint8_t *d_payload,
                                size_t payload_cap, uint64_t *interval_off, uint64_t *interval_len, size_t *payload_bytes, void *d_scratch,
                                size_t scratch_bytes)
{
    OIP_CHECK_CTX(ctx);
    const char *fn = "oip_jpeg_scan_u8";
    if (!d_img || !d_payload || !interval_off || !interval_len || !payload_bytes) return oip_fail(ctx, OIP_E_INVALID, "%s: bad argument", fn);
    const JpegPlan p = plan_jpeg(w, h, nch);
    if (!p.ok) return oip_fail(ctx, OIP_E_INVALID, "%s: width and height 1..65535 and 1 or 3 channels expected", fn);
    if (quality < 1 || quality > 100) return oip_fail(ctx, OIP_E_INVALID, "%s: quality 1..100 expected", fn);
    if (pitch_bytes < (long)w * nch) return oip_fail(ctx, OIP_E_INVALID, "%s: pitch below the line's bytes", fn);
    if (payload_cap < p.worst_bytes) return oip_fail(ctx, OIP_E_INVALID, "%s: payload buffer too small", fn);
    OipDeviceBlock own;                          // scratch of this call's own when the caller brought none
    if (d_scratch) {
        if (scratch_bytes < p.scratch_bytes || (((uintptr_t)d_scratch) & 7)) return oip_fail(ctx, OIP_E_INVALID, "%s: scratch too small or misaligned", fn);
    } else {
        OIP_HIP(ctx, own.alloc(p.scratch_bytes));
        d_scratch = own.p;
    }
    std::unique_ptr<oipjpeg::Tables> tab(new oipjpeg::Tables);
    oipjpeg::make_tables(quality, tab.get());
    unsigned *d_len = reinterpret_cast<unsigned *>((char *)d_scratch + p.o_len);
    unsigned long long *d_off = reinterpret_cast<unsigned long long *>((char *)d_scratch + p.o_off);
    unsigned long long *d_cycles = reinterpret_cast<unsigned long long *>((char *)d_scratch + p.o_cycles);
    OIP_HIP(ctx, hipMemcpyAsync(d_scratch, tab.get(), sizeof(oipjpeg::Tables), hipMemcpyHostToDevice, ctx->stream));
    OIP_HIP(ctx, hipMemsetAsync(d_cycles, 0, 5 * sizeof(unsigned long long), ctx->stream));
    JpegJob j{d_img, pitch_bytes, w, h, nch, reinterpret_cast<const oipjpeg::Tables *>(d_scratch), p.intervals, nullptr, d_off, d_len, d_cycles};
    {
        OipProfScope prof(ctx, "jpeg_measure_kernel");
        hipLaunchKernelGGL(jpeg_scan_kernel, dim3((unsigned)p.intervals), dim3(64), 0, ctx->stream, j);
    }
    OIP_HIP(ctx, hipGetLastError());
    std::vector<unsigned> len((size_t)p.intervals);
    std::vector<unsigned long long> off((size_t)p.intervals);
    OIP_HIP(ctx, hipMemcpyAsync(len.data(), d_len, len.size() * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    OIP_HIP(ctx, hipStreamSynchronize(ctx->stream));
    size_t pos = 0;
    const size_t slot = p.worst_bytes / (size_t)p.intervals;
    for (long k = 0; k < p.intervals; ++k) {     // (cannot fire: an interval is at least a byte and at most its 416 bytes a block)
        if (len[(size_t)k] == 0 || len[(size_t)k] > slot) return oip_fail(ctx, OIP_E_RUNTIME, "%s: interval %ld was not encoded", fn, k);
        off[(size_t)k] = pos;
        pos += len[(size_t)k];
    }
    OIP_HIP(ctx, hipMemcpyAsync(d_off, off.data(), off.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
    j.payload = d_payload;
    {
        OipProfScope prof(ctx, "jpeg_store_kernel");
        hipLaunchKernelGGL(jpeg_scan_kernel, dim3((unsigned)p.intervals), dim3(64), 0, ctx->stream, j);
    }
    OIP_HIP(ctx, hipGetLastError());
    OIP_HIP(ctx, hipStreamSynchronize(ctx->stream));                              // off[] and the call's own scratch end with the call
    for (long k = 0; k < p.intervals; ++k) { interval_off[k] = off[(size_t)k]; interval_len[k] = len[(size_t)k]; }
    *payload_bytes = pos;
    return OIP_OK;
}

extern "C" size_t oip_jpeg_interval_host(const uint8_t *img, long pitch_bytes, int w, long h, int nch, int quality, long interval, uint8_t *dst, size_t cap)
{
    const JpegPlan p = plan_jpeg(w, h, nch);
    if (!img || !dst || !p.ok || quality < 1 || quality > 100 || pitch_bytes < (long)w * nch || interval < 0 || interval >= p.intervals) return 0;
    std::unique_ptr<oipjpeg::Shared<1>> work(new oipjpeg::Shared<1>);
    return oipjpeg::interval_host(img, pitch_bytes, w, h, nch, quality, interval, dst, cap, work.get());
}

extern "C" int oip_write_jpeg_u8(const char *path, const uint8_t *payload, const uint64_t *interval_off, const uint64_t *interval_len, int w, long h,
                                 int nch, int quality, char *err, int errlen)
{
    auto fail = [&](int code, const char *fmt, auto... a) {
        if (err && errlen > 0) snprintf(err, errlen, fmt, a...);
        return code;
    };
    if (!path || !payload || !interval_off || !interval_len || !plan_jpeg(w, h, nch).ok || quality < 1 || quality > 100)
        return fail(OIP_E_INVALID, "%s", "oip_write_jpeg_u8: bad argument (width and height 1..65535, 1 or 3 channels, quality 1..100 expected)");
    if (!oipjpeg::write_file(path, payload, interval_off, interval_len, w, (int)h, nch, quality))
        return fail(OIP_E_IO, "oip_write_jpeg_u8: cannot write '%s': %s", path, strerror(errno));
    return OIP_OK;
}
