// oip_host.hpp -- C++ host layer above the C ABI (include/oip_c.h), mirroring the reference's
// class interface for the hot path: ImageOperations (IMO), Stitcher, PreProcessor -- same
// method names, argument meaning and error behaviour (exception types -> exit codes of
// main.cpp:320-343), with the raster loops running on the MI355X.  Used by the `oip` CLI.
//
// Differences kept deliberately small:
//   * the line width is a constructor/run-time argument (reference: PIXELS_PER_LINE 12288);
//   * TIFF input and output go through a dependency-free TIFF/BigTIFF codec (oip_tiff.hpp) instead of
//     GDAL / cv::imread / cv::imwrite;
//   * timing lines are logged like the reference's (seconds, MBps) through a plain logger.
#pragma once

#include <sys/stat.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <ctime>
#include <chrono>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <filesystem>
#include <functional>
#include <future>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "oip_c.h"
#include "oip_corrgeom.h"
#include "oip_tiff.hpp"
#include "oip_tifftiled.hpp"

namespace OIPGPU {

struct errno_error : public std::runtime_error {      // libimsux errno_error stand-in (same role)
    explicit errno_error(const std::string &s) : std::runtime_error(s + ": " + std::strerror(errno)) {}
    errno_error(const std::string &complete, int) : std::runtime_error(complete) {}   // the C ABI's message already names the errno
};
struct usage_error : public std::invalid_argument {   // main.cpp:20-23
    explicit usage_error(const std::string &s) : std::invalid_argument(s) {}
};

// ---- logging (libimsux logger stand-in: timestamped lines to stdout and $LOGFILE / oip.log) ----
inline FILE *&log_file() { static FILE *f = nullptr; return f; }
inline void log_line(bool stamped, const char *fmt, ...)
{
    char msg[2048];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    char ts[64] = "";
    if (stamped) {
        time_t t = time(nullptr);
        struct tm tmv;
        localtime_r(&t, &tmv);
        strftime(ts, sizeof ts, "%Y-%m-%d %H:%M:%S ", &tmv);
    }
    printf("%s%s\n", ts, msg);
    if (log_file()) { fprintf(log_file(), "%s%s\n", ts, msg); fflush(log_file()); }
}
#define OLOG(...) ::OIPGPU::log_line(true, __VA_ARGS__)
#define RLOG(...) ::OIPGPU::log_line(false, __VA_ARGS__)

struct stop_watch {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double tick()
    {
        auto t1 = std::chrono::steady_clock::now();
        double s = std::chrono::duration<double>(t1 - t0).count();
        t0 = t1;
        return s > 0 ? s : 1e-9;
    }
};

// Which compression a TIFF product gets.  "reference" (default) = what the reference's libraries do for that product:
// cv::imwrite -> LZW + horizontal predictor (ALIGNED.TIFF, stitched MSS without -g), GDAL with COMPRESS=LZW
// PREDICTOR=2 (stitched MSS with -g, imageop.h:471-472), GDAL with default options -> none (stitched PAN,
// imageop.h:316-328).  --tiff-compress none|lzw|deflate (or $OIP_TIFF_COMPRESS) forces one for every product; deflate (259 = 8,
// predictor 2, csrc/oip_deflate.h) is what no reference product has and archive COGs do.
inline int &tiff_policy() { static int p = -1; return p; }       // -1 reference, else TIFF_NONE / TIFF_LZW / TIFF_DEFLATE
inline int tiff_compression(int reference_choice)
{
    if (tiff_policy() < 0) {
        const char *e = getenv("OIP_TIFF_COMPRESS");
        if (e && std::string(e) == "none") return TIFF_NONE;
        if (e && std::string(e) == "lzw") return TIFF_LZW;
        if (e && std::string(e) == "deflate") return TIFF_DEFLATE;
        return reference_choice;
    }
    return tiff_policy();
}

inline std::string to_lower(std::string s)
{
    for (auto &c : s) c = (char)tolower((unsigned char)c);
    return s;
}

// ---- small threading helpers of the pipelined actions ----------------------------------------------------
template <typename T> class BlockingQueue {
public:
    void push(T v)
    {
        { std::lock_guard<std::mutex> lk(mMu); mQ.push_back(std::move(v)); }
        mCv.notify_one();
    }
    T pop()
    {
        std::unique_lock<std::mutex> lk(mMu);
        mCv.wait(lk, [&] { return !mQ.empty(); });
        T v = std::move(mQ.front());
        mQ.pop_front();
        return v;
    }
private:
    std::mutex mMu;
    std::condition_variable mCv;
    std::deque<T> mQ;
};

// a thread that runs jobs in the order they are posted (a product writer: HBM -> file beside the compute thread); the
// first exception stops it and is re-thrown by finish()
class JobThread {
public:
    JobThread() : mThread([this] { loop(); }) {}
    ~JobThread() { try { finish(); } catch (...) {} }
    void post(std::function<void()> job) { mQ.push(std::move(job)); }
    void finish()
    {
        if (mThread.joinable()) { mQ.push(nullptr); mThread.join(); }
        if (mError) { auto e = mError; mError = nullptr; std::rethrow_exception(e); }
    }
private:
    void loop()
    {
        for (;;) {
            std::function<void()> job = mQ.pop();
            if (!job) return;
            if (mError) continue;                 // drain after a failure
            try { job(); } catch (...) { mError = std::current_exception(); }
        }
    }
    BlockingQueue<std::function<void()>> mQ;
    std::exception_ptr mError;
    std::thread mThread;
};

inline double seconds_since(const std::chrono::steady_clock::time_point &t0)
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
inline std::chrono::steady_clock::time_point &process_start()
{
    static std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    return t;
}

// ---- device context + error mapping ----------------------------------------------------------
class Device {
public:
    static Device &get()
    {
        static Device d;
        return d;
    }
    oip_ctx *ctx()
    {
        if (!mCtx) {
            const auto t0 = std::chrono::steady_clock::now();
            if (oip_create(0, &mCtx) != OIP_OK)
                throw std::runtime_error("no usable MI355X (gfx950) device: this build has no CPU fallback");
            mCreateSeconds = seconds_since(t0);
        }
        return mCtx;
    }
    double create_seconds() const { return mCreateSeconds; }
    void check(int rc)
    {
        if (rc == OIP_OK) return;
        std::string m = oip_last_error(mCtx);
        switch (rc) {
            case OIP_E_INVALID: throw std::invalid_argument(m);
            case OIP_E_IO: throw errno_error(m, 0);
            default: throw std::runtime_error(m);
        }
    }
    ~Device() { if (mCtx) oip_destroy(mCtx); }
private:
    oip_ctx *mCtx = nullptr;
    double mCreateSeconds = 0.0;
};

template <typename T> struct DevBuf {              // RAII device buffer
    T *p = nullptr;
    size_t n = 0;
    DevBuf() = default;
    explicit DevBuf(size_t count) { alloc(count); }
    void alloc(size_t count)
    {
        release();
        void *v = nullptr;
        Device::get().check(oip_malloc(Device::get().ctx(), &v, count * sizeof(T)));
        p = (T *)v;
        n = count;
    }
    void release() { if (p) oip_free(Device::get().ctx(), p); p = nullptr; n = 0; }
    // pageable host memory moves through the pinned staging ring (include/oip_c.h, raster I/O staging); small
    // tables take the plain copy
    void upload(const T *h, size_t count)
    {
        if (count * sizeof(T) >= ((size_t)8 << 20)) Device::get().check(oip_upload_staged(Device::get().ctx(), p, h, count * sizeof(T), nullptr));
        else Device::get().check(oip_memcpy_h2d(Device::get().ctx(), p, h, count * sizeof(T)));
    }
    void assign(const std::vector<T> &h) { alloc(h.size()); upload(h.data(), h.size()); }       // a host table, e.g. IMO::LoadLut's
    void download(T *h, size_t count) const
    {
        if (count * sizeof(T) >= ((size_t)8 << 20)) { Device::get().check(oip_download_staged(Device::get().ctx(), h, p, count * sizeof(T))); return; }
        Device::get().check(oip_memcpy_d2h(Device::get().ctx(), h, p, count * sizeof(T)));
        Device::get().check(oip_sync(Device::get().ctx()));
    }
    // ReadFileContent / LoadRawImage with the buffer in HBM (imageop.h:52-82, :110-127): the whole file, which
    // must hold exactly `count` elements
    void load_file(const std::string &filePath, size_t count)
    {
        OLOG("Reading raw image from file `%s' ...", filePath.c_str());
        stop_watch sw;
        size_t got = 0;
        Device::get().check(oip_read_file_to_device(Device::get().ctx(), filePath.c_str(), 0, count * sizeof(T), p, &got, nullptr));
        if (got != count * sizeof(T))
            throw std::runtime_error("file size(" + std::to_string(count * sizeof(T)) + ") doesn't match with read byte count(" +
                                     std::to_string(got) + ")");
        double es = sw.tick();
        OLOG("%zu bytes read in %.3f seconds (%.1f MBps).", got, es, got / es / 1024.0 / 1024.0);
    }
    // WriteBufferToFile with the buffer in HBM (imageop.h:84-97)
    void save_file(const std::string &filePath, size_t count) const
    {
        Device::get().check(oip_write_device_to_file(Device::get().ctx(), p, count * sizeof(T), filePath.c_str(), 0));
    }
    void swap(DevBuf &o) { std::swap(p, o.p); std::swap(n, o.n); }
    ~DevBuf() { release(); }
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
};

constexpr int BYTES_PER_PIXEL = 2;
constexpr int MSS_BANDS = OIP_MSS_BANDS;

// The device codec of a TIFF compression: its numbers (csrc/oip_tiffstreams.h), its entry points (include/oip_c.h: LZW's and
// Deflate's take the same arguments) and its knob.  nullptr: the compression has none.
struct TiffDeviceCodec {
    const OipTiffCodec &codec;
    int knob;                                    // the value of its environment variable, 1 where unset; 0 sends its streams to the host's threads
                                                 // (same file bytes, same image: test and A/B knob), the other values: tiff_streams_on_device
    decltype(&oip_tiff_lzw_worst_bytes) worst_bytes, scratch_bytes;
    decltype(&oip_tiff_lzw_strips_u16) strips;
    decltype(&oip_tiff_lzw_decode_u16) decode;
};
inline const TiffDeviceCodec *tiff_device_codec(int compression)
{
    // (both variables are read at the first call, whichever compression it asks for, and hold for the life of the process)
    auto knob = [](const char *name) { const char *e = getenv(name); return e ? atoi(e) : 1; };
    static const TiffDeviceCodec lzw{kOipTiffLzw, knob("OIP_TIFF_GPU_LZW"), oip_tiff_lzw_worst_bytes, oip_tiff_lzw_scratch_bytes, oip_tiff_lzw_strips_u16, oip_tiff_lzw_decode_u16};
    static const TiffDeviceCodec deflate{kOipTiffDeflate, knob("OIP_TIFF_GPU_DEFLATE"), oip_tiff_deflate_worst_bytes, oip_tiff_deflate_scratch_bytes,
                                         oip_tiff_deflate_strips_u16, oip_tiff_deflate_decode_u16};
    return compression == TIFF_LZW ? &lzw : compression == TIFF_DEFLATE ? &deflate : nullptr;
}

// whether the streams (strips or tiles) of a compressed file being read or written go through the device codec: the route rule of
// csrc/oip_tiffstreams.h with the codec's knob
inline bool tiff_on_device(int compression, OipTiffDirection dir, size_t nstreams, uint64_t streamBytes)
{
    const TiffDeviceCodec *dc = tiff_device_codec(compression);
    return dc && tiff_streams_on_device(dc->codec, dir, nstreams, streamBytes, dc->knob);
}

// the bytes of tile-major samples a batch of tile rows may hold on its way to or from a tiled TIFF (OIP_COG_BATCH_MB: test hook, several
// batches on a small image)
inline size_t cog_batch_bytes(size_t dflt)
{
    if (const char *e = getenv("OIP_COG_BATCH_MB")) {
        const long mb = atol(e);
        if (mb > 0) return (size_t)mb << 20;
    }
    return dflt;
}

// rows x rowSamples u16 in HBM -> the writer, 256 MiB of lines at a time, the next block coming down (staging download lane)
// while the strips of the current one are encoded (a few threads) and the previous one's are written (TiffWriterU16's own
// thread): download || encode || write
inline void tiff_rows_from_device(TiffWriterU16 &tw, const uint16_t *d_img, long rows, size_t rowSamples, long mark)
{
    oip_ctx *ctx = Device::get().ctx();
    size_t chunkBytes = (size_t)256 << 20;
    if (const char *e = getenv("OIP_TIFF_CHUNK_MB")) {                 // test hook: several blocks on a small image
        const long mb = atol(e);
        if (mb > 0) chunkBytes = (size_t)mb << 20;
    }
    const long chunk = std::max<long>(1, (long)(chunkBytes / (rowSamples * 2)));
    const size_t cap = (size_t)std::min(chunk, rows) * rowSamples;
    std::unique_ptr<uint16_t[]> buf[2] = {std::unique_ptr<uint16_t[]>(new uint16_t[cap]), std::unique_ptr<uint16_t[]>(rows > chunk ? new uint16_t[cap] : nullptr)};
    auto fetch = [&](long r0, uint16_t *dst) {
        const long nr = std::min(chunk, rows - r0);
        return oip_download_staged_after(ctx, dst, d_img + (size_t)r0 * rowSamples, (size_t)nr * rowSamples * 2, mark);
    };
    Device::get().check(fetch(0, buf[0].get()));
    int cur = 0;
    for (long r0 = 0; r0 < rows; r0 += chunk) {
        const long nr = std::min(chunk, rows - r0);
        std::future<int> next;
        if (r0 + chunk < rows) next = std::async(std::launch::async, fetch, r0 + chunk, buf[cur ^ 1].get());
        try {
            tw.write_rows(buf[cur].get(), nr);
        } catch (...) {
            if (next.valid()) next.wait();
            throw;
        }
        if (next.valid()) Device::get().check(next.get());
        cur ^= 1;
    }
}

// An LZW or Deflate product whose pixels are in HBM, in file sample order: the strips are encoded where the image is
// (csrc/tifflzw.hip: a lane per strip; csrc/tiffdeflate.hip: a wave per strip) and leave the device packed, as one block that goes
// into the file behind the header.  The encoder runs on the compute stream: everything the image waits for is ahead of it there.
// TiffStripPrep: what a caller that knows the product's geometry before its pixels exist prepares meanwhile (the pipelined
// default action, on its product writer's thread while the strip is still being read): the device buffers, and the file with
// the worst-case size reserved and mapped -- writing a NEW file is bound by the allocation of its pages; the
// file is cut back to the encoded size afterwards.
struct TiffStripPrep {
    DevBuf<uint8_t> payload, scratch;
    oip_file_sink *sink = nullptr;
    uint64_t payloadAt = 0;
    void prepare(TiffWriterU16 &tw, const std::string &path, int width, long height, int spp, int compression, bool withSink)
    {
        const long rps = tw.rows_per_strip();
        const TiffDeviceCodec &dc = *tiff_device_codec(compression);
        payload.alloc(dc.worst_bytes(height, width, spp, rps));
        scratch.alloc(dc.scratch_bytes(height, width, spp, rps));
        if (withSink) {
            payloadAt = tw.begin_external_strips();
            Device::get().check(oip_file_sink_open(Device::get().ctx(), path.c_str(), (size_t)payloadAt + payload.n, &sink));
        }
    }
    ~TiffStripPrep() { if (sink) oip_file_sink_close(nullptr, sink); }
};

inline void tiff_strips_from_device(TiffWriterU16 &tw, const std::string &path, const uint16_t *d_img, int width, long height, int spp,
                                    int compression, TiffStripPrep *prep = nullptr)
{
    oip_ctx *ctx = Device::get().ctx();
    const TiffDeviceCodec &dc = *tiff_device_codec(compression);
    stop_watch sw;
    const long rps = tw.rows_per_strip();
    const size_t nstrips = (size_t)((height + rps - 1) / rps);
    TiffStripPrep own;
    std::future<int> reserving;
    size_t reserved = 0;
    if (!prep) {
        // nothing was prepared: the product file is reserved and mapped by a helper thread WHILE the strips are being encoded
        // -- at the size sensor data encodes to (raw + 3 %: LZW does not compress it, and Deflate's worst case is below that); a
        // payload that turns out larger goes the plain way.  (Writing a new file is bound by the allocation of its pages)
        prep = &own;
        const size_t worst = dc.worst_bytes(height, width, spp, rps);
        prep->payload.alloc(worst);
        const size_t raw = (size_t)height * width * spp * 2;
        if (raw >= ((size_t)64 << 20)) {
            reserved = std::min(worst, raw + raw / 32 + ((size_t)64 << 10));
            own.payloadAt = tw.begin_external_strips();
            TiffStripPrep *op = &own;
            reserving = std::async(std::launch::async, [=] { return oip_file_sink_open(ctx, path.c_str(), (size_t)op->payloadAt + reserved, &op->sink); });
        }
    } else if (prep->sink) {
        reserved = prep->payload.n;
    }
    std::vector<uint64_t> off(nstrips), len(nstrips);
    size_t bytes = 0;
    const double tAlloc = sw.tick();
    const int rcEncode = dc.strips(ctx, d_img, height, width, spp, rps, prep->payload.p, prep->payload.n, off.data(), len.data(), &bytes, prep->scratch.p,
                                prep->scratch.n);
    if (reserving.valid() && reserving.get() != OIP_OK && prep->sink) { oip_file_sink_close(nullptr, prep->sink); prep->sink = nullptr; }
    Device::get().check(rcEncode);
    const double tEncode = sw.tick();
    const size_t even = (bytes + 1) & ~(size_t)1;
    if (prep->sink && even <= reserved) {
        Device::get().check(oip_file_sink_write(ctx, prep->sink, (size_t)prep->payloadAt, prep->payload.p, even, 0));
        oip_file_sink *k = prep->sink;
        prep->sink = nullptr;
        Device::get().check(oip_file_sink_close(ctx, k));
        if (::truncate(path.c_str(), (off_t)(prep->payloadAt + even)) != 0) throw errno_error("truncate() of the TIFF product failed");
    } else {
        uint64_t at = prep->payloadAt;
        if (prep->sink) {                                              // reserved too little: drop the reservation, write the plain way
            oip_file_sink *k = prep->sink;
            prep->sink = nullptr;
            Device::get().check(oip_file_sink_close(ctx, k));
            if (::truncate(path.c_str(), (off_t)at) != 0) throw errno_error("truncate() of the TIFF product failed");
        } else if (!reserved) {
            at = tw.begin_external_strips();
        }
        Device::get().check(oip_write_device_to_file_at(ctx, prep->payload.p, even, path.c_str(), (size_t)at, 0));
    }
    tw.end_external_strips(off.data(), len.data(), nstrips, bytes);
    const double tWrite = sw.tick();
    RLOG("TIMING %s strips=%zu alloc=%.4f encode=%.4f write=%.4f bytes=%zu prepared=%d", dc.codec.timing, nstrips,
         tAlloc, tEncode, tWrite, bytes, prep != &own);
}

// The pixels of the directory `tw` is writing (width x height x spp u16 in HBM, in file sample order) leave the device:
// uncompressed as one external payload, LZW and Deflate strips from the device encoder where tiff_on_device() says so, else
// through the host's.
inline void tiff_image_from_device(TiffWriterU16 &tw, const std::string &path, const uint16_t *d_img, int width, long height, int spp,
                                   int compression, long mark)
{
    const size_t rowSamples = (size_t)width * spp;
    if (compression == TIFF_NONE) {
        const uint64_t at = tw.begin_external_payload();
        Device::get().check(oip_write_device_to_file_at(Device::get().ctx(), d_img, (size_t)height * rowSamples * 2, path.c_str(), (size_t)at, mark));
        tw.end_external_payload();
    } else if (tiff_on_device(compression, OIP_TIFF_WRITE, (size_t)((height + tw.rows_per_strip() - 1) / tw.rows_per_strip()), (uint64_t)tw.rows_per_strip() * rowSamples * 2)) {
        tiff_strips_from_device(tw, path, d_img, width, height, spp, compression);
    } else {
        tiff_rows_from_device(tw, d_img, height, rowSamples, mark);
    }
}

// A TIFF product whose pixels are in HBM (rows x width x spp u16, interleaved).  Uncompressed: the pixel payload goes from
// the device into the file behind the header (TiffWriterU16::begin_external_payload + oip_write_device_to_file_at) -- no
// strip-sized heap copy, as the reference's cv::imwrite / GDAL paths make (imageop.h:316-328, preproc.h:167-185).  LZW: the
// lines come down 256 MiB at a time and their strips are encoded on a few threads.  opencv_order (4 samples): the image takes
// cv::imwrite's on-disk sample order (c2,c1,c0,c3) ON THE DEVICE first -- d_img is modified; `order` (4 samples, GDAL band
// maps): out sample i = in sample order[i], likewise.  mark: 0, or the compute-stream mark the image is complete at.
inline void write_tiff_from_device(const std::string &path, uint16_t *d_img, int width, long height, int spp, int compression,
                                   bool opencv_order, const int *order = nullptr, long mark = 0, bool permute_done = false)
{
    oip_ctx *ctx = Device::get().ctx();
    if (spp == MSS_BANDS && !permute_done && (opencv_order || order)) {
        const int cvOrder[4] = {2, 1, 0, 3};
        Device::get().check(oip_permute_u16x4(ctx, d_img, (size_t)width * height, order ? order : cvOrder));
        mark = 0;                                                      // (the permutation is younger than the mark)
    }
    TiffWriterU16 tw(path, width, height, spp, false, compression);
    tiff_image_from_device(tw, path, d_img, width, height, spp, compression, mark);
    tw.close();
}

// The tiles of the directory `tw` is writing (w x h x spp u16 in HBM, in file sample order) leave the device, in batches of tile
// rows of at most 256 MiB of tile-major samples and at least one tile row (OIP_COG_BATCH_MB: test hook, several batches on a small
// image): oip_retile_u16 into the batch buffer; uncompressed, the batch itself goes into the file; LZW and Deflate, every tile is
// one "strip" of the device encoder (a T-wide image of tile_rows tx T lines in strips of T lines) and the packed payload goes.
// Where tiff_on_device() says host (OIP_TIFF_GPU_LZW=0; Deflate on the directory's tile count: the same for every batch size):
// the tile-major form comes down and the host coders write it (TiffTiledWriterU16::write_tiles; same bytes).
inline void tiled_image_from_device(TiffTiledWriterU16 &tw, const std::string &path, const uint16_t *d_img, int w, long h, int spp, int T,
                                    int compression)
{
    oip_ctx *ctx = Device::get().ctx();
    auto ck = [](int rc) { Device::get().check(rc); };
    stop_watch sw;
    const long tx = tw.tiles_x(), ty = tw.tiles_y();
    const size_t tileSamples = (size_t)T * T * spp, rowSamples = (size_t)tx * tileSamples, n = (size_t)tx * ty;
    const long batchRows = std::max<long>(1, std::min<long>(ty, (long)(cog_batch_bytes((size_t)256 << 20) / (rowSamples * 2))));
    DevBuf<uint16_t> batch((size_t)batchRows * rowSamples);
    if (compression != TIFF_NONE && !tiff_on_device(compression, OIP_TIFF_WRITE, n, (uint64_t)tileSamples * 2)) {
        std::vector<uint16_t> host(n * tileSamples);
        for (long j0 = 0; j0 < ty; j0 += batchRows) {
            const long nr = std::min(batchRows, ty - j0);
            ck(oip_retile_u16(ctx, d_img, (long)w * spp, w, h, spp, T, j0, nr, batch.p));
            batch.download(host.data() + (size_t)j0 * rowSamples, (size_t)nr * rowSamples);
        }
        tw.write_tiles(host.data());
        return;
    }
    const TiffDeviceCodec *dc = tiff_device_codec(compression);      // (nullptr: uncompressed)
    DevBuf<uint8_t> payload, scratch;
    if (dc) {
        payload.alloc(dc->worst_bytes(batchRows * tx * T, T, spp, T));
        scratch.alloc(dc->scratch_bytes(batchRows * tx * T, T, spp, T));
    }
    std::vector<uint64_t> off(n), len(n);
    const uint64_t at = tw.begin_tiles();
    uint64_t pos = 0;
    double tEncode = 0.0, tWrite = 0.0;
    sw.tick();
    for (long j0 = 0; j0 < ty; j0 += batchRows) {
        const long nr = std::min(batchRows, ty - j0);
        const size_t k0 = (size_t)j0 * tx, nt = (size_t)nr * tx;
        if (pos & 1) ++pos;                                            // a batch starts on an even offset, as every tile does
        ck(oip_retile_u16(ctx, d_img, (long)w * spp, w, h, spp, T, j0, nr, batch.p));
        if (!dc) {
            for (size_t k = 0; k < nt; ++k) { off[k0 + k] = pos + k * tileSamples * 2; len[k0 + k] = tileSamples * 2; }
            ck(oip_write_device_to_file_at(ctx, batch.p, nt * tileSamples * 2, path.c_str(), (size_t)(at + pos), 0));
            pos += nt * tileSamples * 2;
            tWrite += sw.tick();
        } else {
            size_t bytes = 0;
            ck(dc->strips(ctx, batch.p, (long)nt * T, T, spp, T, payload.p, payload.n, off.data() + k0, len.data() + k0, &bytes, scratch.p, scratch.n));
            tEncode += sw.tick();
            for (size_t k = 0; k < nt; ++k) off[k0 + k] += pos;
            ck(oip_write_device_to_file_at(ctx, payload.p, bytes, path.c_str(), (size_t)(at + pos), 0));
            pos += bytes;
            tWrite += sw.tick();
        }
    }
    tw.end_tiles(off.data(), len.data(), n, pos);
    if (dc)
        RLOG("TIMING %s tiles=%zu tile=%d encode=%.4f write=%.4f bytes=%zu", dc->codec.timing, n, T, tEncode, tWrite, (size_t)pos);
}

// ---- overviews: <product>.ovr, the reduced-resolution pyramid of a product or strip (not in the reference) ----------------
// `oip overviews` and `oip stitch --overviews` come through here.  levels: 0 = oip_overview_levels.
struct OverviewOptions {
    int levels = 0;
    int validMin = 1;                       // 0 is the border value of prestitch and the aligner (BORDER_CONSTANT)
};

// The pyramid of a w0 x h0 x spp image whose LEVEL 1 is resident (oip_halve_u16 of the image, or of a strip block by block):
// a TIFF of `levels` chained directories, level 1 first (TiffWriterU16 with overview_levels), every level leaving the device
// the way a product of its geometry does.  Levels 2 .. n are resident calls that alternate between level1's buffer and a second
// one a quarter of its size: a level is in the file before the level after the next one replaces it.
inline void write_overviews_from_device(const std::string &path, DevBuf<uint16_t> &level1, int w0, long h0, int spp, int levels, int validMin)
{
    oip_ctx *ctx = Device::get().ctx();
    const int comp = tiff_compression(spp == 1 ? TIFF_NONE : TIFF_LZW);
    OLOG("Write %d overview levels to file '%s' ...", levels, path.c_str());
    TiffWriterU16 tw(path, w0, h0, spp, false, comp, levels);
    DevBuf<uint16_t> second;
    uint16_t *cur = level1.p;
    for (int k = 1; k <= levels; ++k) {
        const int w = tw.width();
        const long h = tw.height();
        RLOG("    level %d: %d x %ld x %d", k, w, h, spp);
        tiff_image_from_device(tw, path, cur, w, h, spp, comp, 0);
        if (k == levels) break;
        const int nw = (w + 1) / 2;
        const long nh = (h + 1) / 2;
        if (k == 1) second.alloc((size_t)nw * nh * spp);
        uint16_t *next = cur == level1.p ? second.p : level1.p;
        Device::get().check(oip_halve_u16(ctx, cur, (long)w * spp, w, h, spp, validMin, next, (long)nw * spp));
        tw.next_directory();
        cur = next;
    }
    tw.close();
}

// the same of an image that is itself resident (a stitched product, a TIFF read to the device)
inline void write_overviews_of_device_image(const std::string &path, const uint16_t *d_img, int w, long h, int spp, const OverviewOptions &o)
{
    const int levels = o.levels > 0 ? o.levels : oip_overview_levels(w, h);
    const int w1 = (w + 1) / 2;
    const long h1 = (h + 1) / 2;
    DevBuf<uint16_t> level1((size_t)w1 * h1 * spp);
    Device::get().check(oip_halve_u16(Device::get().ctx(), d_img, (long)w * spp, w, h, spp, o.validMin, level1.p, (long)w1 * spp));
    write_overviews_from_device(path, level1, w, h, spp, levels, o.validMin);
}


// cv::imread of a 16-bit TIFF (imageop.h:380-388) with the image ending up in HBM.  LZW files -- what the reference's own
// products are -- go from the file into device memory as they are and their strips are decoded there (csrc/tifflzw.hip: a
// strip per lane; a tiled file with square tiles of a multiple of 16: a tile per lane into a tile-major buffer, then
// oip_untile_u16); anything else, and OIP_TIFF_GPU_LZW=0, decodes on the host's threads (read_tiff_u16) and uploads.  Same
// checks and error texts either way: the header is validated by the host reader in both.  Deflate files take the same two
// routes, their streams inflated by csrc/tiffdeflate.hip (a stream per wave), under the same conditions and the two of the route
// rule (csrc/oip_tiffstreams.h: at least 256 streams, none decoding to more than 2 MiB; what was measured is told there).
// Streams [k0, k0 + n) of the file -- strips or tiles -- go from the file into device memory as they are and are decoded into d_out, an
// image of `rows` x `width` pixels in strips of `rps` rows; `tail` ends the message of a stream the decoder refuses.
inline void tiff_streams_to_device(const std::string &path, const TiffLayout &lay, size_t k0, size_t n, long rows, int width, long rps, uint16_t *d_out,
                                   const std::string &tail = "")
{
    oip_ctx *ctx = Device::get().ctx();
    uint64_t lo = ~(uint64_t)0, hi = 0;
    for (size_t k = k0; k < k0 + n; ++k) { lo = std::min(lo, lay.offs[k]); hi = std::max(hi, lay.offs[k] + lay.lens[k]); }
    if (lay.tiled() && hi <= lo) throw std::runtime_error("read TIFF [" + path + "]: empty tiles");
    DevBuf<uint8_t> file((size_t)(hi - lo));
    size_t got = 0;
    Device::get().check(oip_read_file_to_device(ctx, path.c_str(), (size_t)lo, (size_t)(hi - lo), file.p, &got, nullptr));
    if (got != (size_t)(hi - lo)) throw std::runtime_error("read TIFF [" + path + "]: truncated file");
    Device::get().check(oip_stage_sync(ctx));
    std::vector<uint64_t> off(lay.offs.begin() + k0, lay.offs.begin() + k0 + n);
    for (auto &o : off) o -= lo;
    const int rc = tiff_device_codec((int)lay.compression)->decode(ctx, file.p, file.n, off.data(), lay.lens.data() + k0, (long)n, rows, width, (int)lay.spp, rps, (int)lay.predictor, d_out);
    if (rc != OIP_OK) throw std::runtime_error("read TIFF [" + path + "]: " + std::string(oip_last_error(ctx)) + tail);
}

inline void read_tiff_to_device(const std::string &path, int *width, long *height, int *spp, DevBuf<uint16_t> &img)
{
    const TiffLayout lay = read_tiff_layout(path);
    *width = (int)lay.width; *height = (long)lay.height; *spp = (int)lay.spp;
    const size_t samples = (size_t)lay.width * lay.height * lay.spp;
    // (tiled: square tiles the layout kernel takes -- a multiple of 16 up to 1024 --, each one a "strip" of the decoder)
    const uint64_t T = lay.tile_width;
    const uint64_t streamBytes = (lay.tiled() ? T * T : lay.rows_per_strip * lay.width) * lay.spp * 2;
    bool device = tiff_on_device((int)lay.compression, OIP_TIFF_READ, lay.offs.size(), streamBytes) && (lay.spp == 1 || lay.spp == 4) &&
                  (lay.tiled() ? T == lay.tile_length && T % 16 == 0 && T <= 1024 : lay.rows_per_strip * lay.width * lay.spp * 2 < ((uint64_t)1 << 32));
    uint64_t lo = ~(uint64_t)0, hi = 0;
    for (size_t k = 0; k < lay.offs.size(); ++k) { lo = std::min(lo, lay.offs[k]); hi = std::max(hi, lay.offs[k] + lay.lens[k]); }
    if (device && hi - lo > 3 * samples + ((uint64_t)64 << 20)) device = false;       // strips scattered over a far larger file
    if (!device) {
        std::vector<uint16_t> host;
        read_tiff_u16(path, width, height, spp, &host);
        img.alloc(host.size());
        img.upload(host.data(), host.size());
        return;
    }
    img.alloc(samples);
    if (!lay.tiled()) {
        tiff_streams_to_device(path, lay, 0, lay.offs.size(), (long)lay.height, (int)lay.width, (long)lay.rows_per_strip, img.p);
        return;
    }
    // batches of tile rows of at most 1 GiB of tile-major samples: decoded into the tile-major buffer (width T, T rows a "strip"), and
    // oip_untile_u16 puts them into the image
    oip_ctx *ctx = Device::get().ctx();
    const long tx = (long)((lay.width + T - 1) / T), ty = (long)((lay.height + T - 1) / T);
    const size_t rowSamples = (size_t)tx * T * T * lay.spp;
    const long batchRows = std::max<long>(1, std::min<long>(ty, (long)(cog_batch_bytes((size_t)1 << 30) / (rowSamples * 2))));
    DevBuf<uint16_t> tiles((size_t)batchRows * rowSamples);
    for (long j0 = 0; j0 < ty; j0 += batchRows) {
        const long nr = std::min(batchRows, ty - j0);
        const size_t k0 = (size_t)j0 * tx, nt = (size_t)nr * tx;
        tiff_streams_to_device(path, lay, k0, nt, (long)(nt * T), (int)T, (long)T, tiles.p, " (tiles from " + std::to_string(k0) + " on)");
        Device::get().check(oip_untile_u16(ctx, tiles.p, (int)lay.width, (long)lay.height, (int)lay.spp, (int)T, j0, nr, img.p, (long)(lay.width * lay.spp)));
    }
    Device::get().check(oip_sync(ctx));                            // (the last untile reads `tiles`)
}

// ---- ImageOperations (imageop.h:33-568, hot-path subset) -----------------------------------------
struct RRCParam { double k; double b; };     // imageop.h:26-29

// ---- oip stitch --balance / --feather: seam balancing and feathering (not in the reference) ------------------
// The two CCDs are calibrated apart, so the hard cut of StitchBigRaw shows any level difference as a step.  The overlap that
// the cut discards gives image 2's gain and offset relative to image 1 (oip_seam_moments_u16 + oip_seam_fit) and room to
// blend (oip_stitch_balanced_u16).  Inactive by default: the stitch is then oip_stitch_rows_u16's, as before.  With blockLines the
// fit is made per block of lines and interpolated to a (G, O) per line (oip_seam_moments_blocks_u16, oip_seam_fit_blocks,
// oip_seam_line_tables, oip_stitch_balanced_lines_u16).  `oip stitch` and both stitches of `oip task` come through here.
struct SeamOptions {
    int balance = -1;                       // -1: none, else OIP_SEAM_MOMENTS / OIP_SEAM_GAIN / OIP_SEAM_OFFSET
    int feather = 0;                        // half-width of the blend zone in pixels (the halved --feather)
    int validMin = 1, validMax = 65535;     // 0 is the border value of prestitch and the aligner (BORDER_CONSTANT)
    long minCount = 0;
    long blockLines = 0;                    // > 0 (with a balance mode): a fit per block of this many lines, interpolated per line
    bool active() const { return balance >= 0 || feather > 0; }
};

// the stitch of two resident images through the seam path; Ws, fs in samples (include/oip_c.h)
inline void StitchSeam(const uint16_t *dl, const uint16_t *dr, uint16_t *dout, int Ws, long L, int fs, int spp, const SeamOptions &o)
{
    oip_ctx *ctx = Device::get().ctx();
    auto ck = [](int rc) { Device::get().check(rc); };
    auto fit_ck = [](int rc, const char *err) {
        if (rc == OIP_E_INVALID) throw std::invalid_argument(err);
        if (rc != OIP_OK) throw std::runtime_error(err);
    };
    const bool blocks = o.balance >= 0 && o.blockLines > 0;
    const long B = blocks ? o.blockLines : 1, nb = blocks ? std::max<long>(1, L / B) : 1;
    const size_t plane = (size_t)6 * spp;
    std::vector<int32_t> G(spp, 65536), O(spp, 0);
    std::vector<uint64_t> planes;                                      // (nb, 6, spp) with --balance-lines
    char err[1024] = "";
    if (o.balance >= 0) {
        DevBuf<uint64_t> acc(plane * nb);
        ck(oip_memset(ctx, acc.p, 0, plane * nb * sizeof(uint64_t)));
        if (blocks) ck(oip_seam_moments_blocks_u16(ctx, dl, dr, Ws, L, fs, spp, o.validMin, o.validMax, B, acc.p));
        else ck(oip_seam_moments_u16(ctx, dl, dr, Ws, L, fs, spp, o.validMin, o.validMax, acc.p));
        planes.resize(plane * nb);
        acc.download(planes.data(), planes.size());
        std::vector<uint64_t> totals(plane, 0);
        for (long k = 0; k < nb; ++k)
            for (size_t i = 0; i < plane; ++i) totals[i] += planes[(size_t)k * plane + i];
        std::vector<double> rep(plane);
        std::vector<int> ident(spp);
        fit_ck(oip_seam_fit(totals.data(), spp, o.balance, (uint64_t)o.minCount, G.data(), O.data(), rep.data(), ident.data(), err, sizeof err), err);
        for (int c = 0; c < spp; ++c)
            OLOG("seam channel %d: n %llu, mean %.3f / %.3f, sigma %.3f / %.3f, r %.6f, gain_q16 %d, offset_q16 %d%s", c + 1,
                 (unsigned long long)totals[c], rep[6 * c + 1], rep[6 * c + 2], rep[6 * c + 3], rep[6 * c + 4], rep[6 * c + 5], G[c], O[c],
                 ident[c] ? " (identity substituted)" : "");
    }
    if (blocks) {
        // a (G, O) per block, the strip's where a block has none of its own, then per line: tables of L * spp pairs in HBM
        const size_t nodes = (size_t)nb * spp, entries = (size_t)L * spp;
        std::vector<int32_t> bg(nodes), bo(nodes), g0(spp), o0(spp), tab(2 * entries + 1);
        std::vector<int> sub(nodes), ident0(spp);
        fit_ck(oip_seam_fit_blocks(planes.data(), nb, spp, o.balance, (uint64_t)o.minCount, bg.data(), bo.data(), sub.data(), g0.data(), o0.data(),
                                   ident0.data(), nullptr, err, sizeof err), err);
        for (int c = 0; c < spp; ++c) {
            long s = 0;
            int32_t gmin = bg[c], gmax = bg[c], omin = bo[c], omax = bo[c];
            for (long k = 0; k < nb; ++k) {
                const size_t e = (size_t)k * spp + c;
                s += sub[e];
                gmin = std::min(gmin, bg[e]); gmax = std::max(gmax, bg[e]);
                omin = std::min(omin, bo[e]); omax = std::max(omax, bo[e]);
            }
            OLOG("seam blocks channel %d: %ld blocks of %ld lines, %ld substituted, gain_q16 %d..%d, offset_q16 %d..%d", c + 1, nb, B, s, gmin, gmax,
                 omin, omax);
        }
        if (oip_seam_line_tables(bg.data(), bo.data(), nb, spp, L, B, tab.data(), tab.data() + entries) != OIP_OK)
            throw std::invalid_argument("oip_seam_line_tables: bad argument");
        DevBuf<int32_t> dtab(2 * entries + 4);                         // (both tables 16-byte aligned: entries * 4 bytes is, at spp 4)
        dtab.upload(tab.data(), 2 * entries);
        ck(oip_stitch_balanced_lines_u16(ctx, dl, dr, dout, Ws, L, fs, spp, dtab.p, dtab.p + entries, o.feather, o.validMin));
        ck(oip_sync(ctx));                  // `dtab` leaves scope
        return;
    }
    DevBuf<int32_t> go((size_t)2 * spp);
    std::vector<int32_t> h(G);
    h.insert(h.end(), O.begin(), O.end());
    go.upload(h.data(), h.size());
    ck(oip_stitch_balanced_u16(ctx, dl, dr, dout, Ws, L, fs, spp, go.p, go.p + spp, o.feather, o.validMin));
    ck(oip_sync(ctx));                      // `go` leaves scope
}

class ImageOperations {
public:
    static size_t FileSize(const std::string &filePath)            // imageop.h:43-47
    {
        struct stat st;
        memset(&st, 0, sizeof st);
        if (stat(filePath.c_str(), &st)) throw errno_error("stat() call for file failed");
        return (size_t)st.st_size;
    }

    // imageop.h:52-82: size = bytes read; offset; total = 0 for all available
    static char *ReadFileContent(const std::string &filePath, size_t &size, size_t offset = 0, size_t total = 0,
                                 char *buff = nullptr)
    {
        FILE *f = fopen(filePath.c_str(), "rb");
        if (!f) throw std::invalid_argument("cannot open file [" + filePath + "]: " + std::to_string(errno));
        size_t want = total;
        if (total == 0) {
            if (fseek(f, 0, SEEK_END)) { fclose(f); throw std::invalid_argument("ReadFileContent(): seek2end failed"); }
            want = (size_t)ftello(f) - offset;
        }
        if (fseeko(f, (off_t)offset, SEEK_SET)) { fclose(f); throw std::invalid_argument("ReadFileContent(): rewind failed"); }
        if (!buff) buff = new char[want ? want : 1];
        const size_t unit = 8u * 1024 * 1024;
        size_t rb = 0;
        for (char *p = buff;;) {
            size_t rn = fread(p, 1, std::min(unit, want - rb), f);
            p += rn;
            rb += rn;
            if (rn == 0 || rb == want) { size = rb; break; }
        }
        fclose(f);
        return buff;
    }

    static size_t WriteBufferToFile(const char *buff, size_t size, const std::string &saveFilePath)   // imageop.h:84-97
    {
        FILE *f = fopen(saveFilePath.c_str(), "wb");
        if (!f) throw std::runtime_error("open file [" + saveFilePath + "] failed: " + std::to_string(errno));
        const size_t unit = std::min((size_t)8 * 1024 * 1024, size);
        size_t written = 0;
        for (const char *p = buff; written < size;) {
            size_t wb = fwrite(p, 1, std::min(unit, size - written), f);
            if (wb == 0) { fclose(f); throw std::runtime_error("write file failed: " + std::to_string(errno)); }
            written += wb;
            p += wb;
        }
        fclose(f);
        return written;
    }

    // imageop.h:99-108: cwd / stem(template) + stemExtension + (replaceExtension | ext(template))
    static std::string BuildOutputFilePath(const std::string &templatePath, const std::string &stemExtension,
                                           const char *replaceExtension = nullptr)
    {
        auto cd = std::filesystem::current_path();
        std::filesystem::path tmpl = templatePath;
        auto out = cd / tmpl.stem();
        out += stemExtension;
        out += replaceExtension ? std::string(replaceExtension) : tmpl.extension().string();
        return out.string();
    }

    static void *LoadRawImage(const std::string &filePath, size_t offset = 0, size_t bytes = 0, size_t expectedSize = 0)
    {                                                                // imageop.h:110-127
        OLOG("Reading raw image from file `%s' ...", filePath.c_str());
        size_t size = 0;
        stop_watch sw;
        void *content = ReadFileContent(filePath, size, offset, bytes);
        if (expectedSize > 0 && size != expectedSize) {
            delete[] (char *)content;
            throw std::runtime_error("file size(" + std::to_string(expectedSize) + ") doesn't match with read byte count(" +
                                     std::to_string(size) + ")");
        }
        double es = sw.tick();
        OLOG("%zu bytes read in %.3f seconds (%.1f MBps).", size, es, size / es / 1024.0 / 1024.0);
        return content;
    }

    // imageop.h:129-138 -- on the GPU, through pinned double-buffered line blocks
    static void InplaceRRC(uint16_t *buff, int w, int h, const RRCParam *rrcParam)
    {
        Device::get().check(oip_rrc_u16_host(Device::get().ctx(), buff, w, h, reinterpret_cast<const double *>(rrcParam)));
    }

    // LoadRRCParamFile (imageop.h:140-192): the n (k, b) pairs of a parameter file, as the 2n doubles the kernels take
    static std::vector<double> LoadLut(const std::string &paramFilePath, int n)
    {
        OLOG("Loading RRC paramter from file `%s' ...", paramFilePath.c_str());
        std::vector<double> kb((size_t)n * 2);
        char err[1024];
        int rc = oip_load_rrc_param_file(paramFilePath.c_str(), n, kb.data(), err, sizeof err);
        if (rc == OIP_E_IO) throw errno_error(err);
        if (rc != OIP_OK) throw std::runtime_error(err);
        OLOG("LoadRRCParamFile(): loaded.");
        return kb;
    }
    // the four band files of an MSS strip W samples wide, one after the other (preproc.h:202-222)
    static std::vector<double> LoadMssLuts(const std::string files[MSS_BANDS], int W)
    {
        const int bw = W / MSS_BANDS;
        std::vector<double> all((size_t)W * 2);
        for (int b = 0; b < MSS_BANDS; ++b) {
            const std::vector<double> kb = LoadLut(files[b], bw);
            std::copy(kb.begin(), kb.end(), all.begin() + (size_t)b * bw * 2);
        }
        return all;
    }

    // imageop.h:194-228.  The raster goes file -> HBM -> file through the staging ring (no whole-file heap buffer);
    // keepBuffer hands back a heap copy like the reference does.
    static uint16_t *DoRRC4RAW(const std::string &raw, int pixelPerLine, const std::string &rrc,
                               const std::string saveRaw = "", bool keepBuffer = false)
    {
        size_t size = FileSize(raw);
        const size_t npx = size / BYTES_PER_PIXEL;
        DevBuf<uint16_t> image(npx ? npx : 1);
        image.load_file(raw, npx);
        long lines = (long)(size / ((size_t)pixelPerLine * BYTES_PER_PIXEL));
        const std::vector<double> rrcParam = LoadLut(rrc, pixelPerLine);
        DevBuf<double> kb;
        kb.assign(rrcParam);
        OLOG("Do inplace RRC ...");
        stop_watch sw;
        Device::get().check(oip_rrc_u16(Device::get().ctx(), image.p, image.p, pixelPerLine, lines, kb.p));
        Device::get().check(oip_sync(Device::get().ctx()));
        double es = sw.tick();
        OLOG("Done for %zu bytes in %.3f seconds (%.1f MBps).", size, es, size / es / (1024.0 * 1024.0));
        if (!saveRaw.empty()) {
            OLOG("Write RRC result as file \"%s\" ...", saveRaw.c_str());
            sw.tick();
            image.save_file(saveRaw, npx);
            es = sw.tick();
            OLOG("%zu bytes written in %.3f seconds (%.1f MBps).", size, es, size / es / (1024.0 * 1024.0));
        }
        if (!keepBuffer) return nullptr;
        std::unique_ptr<uint16_t[]> out(new uint16_t[npx ? npx : 1]);
        image.download(out.get(), npx);
        return out.release();
    }

    // imageop.h:277-363, RAW output only (the GTiff writer is "next")
    static std::string StitchBigRaw(const std::string &leftImagePath, const std::string &rightImagePath,
                                    const std::string &stitchedFilePath, int pixelPerLine, int foldColPixels,
                                    const SeamOptions *seam = nullptr, const OverviewOptions *overviews = nullptr)
    {
        size_t szl = FileSize(leftImagePath), szr = FileSize(rightImagePath);
        if (szl != szr)
            throw std::invalid_argument("RAW image sizes not match: left = " + std::to_string(szl) + " bytes, right = " +
                                        std::to_string(szr) + " bytes");
        const size_t bytesPerLine = (size_t)pixelPerLine * BYTES_PER_PIXEL;
        const long imageLines = (long)(szl / bytesPerLine);
        const int outputFullLinePixels = (pixelPerLine - foldColPixels) * 2;
        bool outputIsTiff = true;                                      // imageop.h:297-306
        std::string outputFilePath = stitchedFilePath;
        if (stitchedFilePath.empty()) {
            outputFilePath = (std::filesystem::current_path() /
                              ("stitched_" + std::to_string(outputFullLinePixels) + "n" + std::to_string(BYTES_PER_PIXEL * 8) + "b.TIFF")).string();
        } else {
            outputIsTiff = to_lower(std::filesystem::path(stitchedFilePath).extension().string()) == ".tiff";
        }
        const size_t npx = (size_t)pixelPerLine * imageLines, nout = (size_t)outputFullLinePixels * imageLines;
        DevBuf<uint16_t> dl(npx), dr(npx), dout(nout);
        dl.load_file(leftImagePath, npx);
        dr.load_file(rightImagePath, npx);
        OLOG("Begin stitching two images ...");
        stop_watch sw;
        if (seam && seam->active()) StitchSeam(dl.p, dr.p, dout.p, pixelPerLine, imageLines, foldColPixels, 1, *seam);
        else Device::get().check(oip_stitch_rows_u16(Device::get().ctx(), dl.p, dr.p, dout.p, pixelPerLine, imageLines, foldColPixels));
        if (outputIsTiff) {                                            // 1-band GTiff (imageop.h:316-328), straight from the device
            write_tiff_from_device(outputFilePath, dout.p, outputFullLinePixels, imageLines, 1, tiff_compression(TIFF_NONE), false);
        } else {
            dout.save_file(outputFilePath, nout);
        }
        double es = sw.tick();
        OLOG("%zu bytes written in %.3f seconds (%.1f MBps).", nout * 2, es, nout * 2 / es / (1024.0 * 1024.0));
        if (overviews) write_overviews_of_device_image(outputFilePath + OIP_OVERVIEW_SUFFIX, dout.p, outputFullLinePixels, imageLines, 1, *overviews);
        return outputFilePath;
    }

    // imageop.h:365-457 (+ StitchTiffGDAL :460-567): two 16UC4 images -> column-range concat.  cv::imread
    // hands the reference BGRA-ordered Mats, i.e. the original channel order c0..c3; the same is rebuilt
    // here from the on-disk RGBA order.  Without -g the result is re-encoded like cv::imwrite; with -g
    // GDAL writes band b from channel bandMap[b]-1 (imageop.h:529).
    static std::string StitchTiff(const std::string &leftImagePath, const std::string &rightImagePath,
                                  const std::string &stitchedFilePath, int foldColPixels, bool useGDAL = false,
                                  const int *bandMap = nullptr, const SeamOptions *seam = nullptr, const OverviewOptions *overviews = nullptr)
    {
        std::string outputFilePath = stitchedFilePath;
        if (stitchedFilePath.empty()) outputFilePath = (std::filesystem::current_path() / "stitched.TIFF").string();
        else if (to_lower(std::filesystem::path(stitchedFilePath).extension().string()) != ".tiff")
            throw std::invalid_argument("Output file should be a tiff image");
        int wl, wr, sl, sr;
        long hl, hr;
        DevBuf<uint16_t> dl, dr;
        OLOG("Reading tiff image from file `%s' ...", leftImagePath.c_str());
        read_tiff_to_device(leftImagePath, &wl, &hl, &sl, dl);
        OLOG("Reading tiff image from file `%s' ...", rightImagePath.c_str());
        read_tiff_to_device(rightImagePath, &wr, &hr, &sr, dr);
        if (hl != hr || wl != wr) throw std::runtime_error("images have different sizes");
        if (sl != MSS_BANDS || sr != MSS_BANDS) throw std::runtime_error("StitchTiff(): 4-channel 16-bit images expected");
        if (foldColPixels < 0 || foldColPixels >= wl) throw std::invalid_argument("fold columns exceed the image width");
        // the stitch itself: 4 interleaved samples per pixel are just 4x wider u16 lines
        const int W4 = wl * 4, fold4 = foldColPixels * 4;
        const size_t nin = (size_t)W4 * hl, nout = (size_t)2 * (W4 - fold4) * hl;
        (void)nin;
        DevBuf<uint16_t> dout(nout);
        // (balancing acts on the samples in file order, before any --GDAL / --band-map permutation below)
        if (seam && seam->active()) StitchSeam(dl.p, dr.p, dout.p, W4, hl, fold4, MSS_BANDS, *seam);
        else Device::get().check(oip_stitch_rows_u16(Device::get().ctx(), dl.p, dr.p, dout.p, W4, hl, fold4));
        const int ow = 2 * (wl - foldColPixels);
        OLOG("Write stitched image to file '%s' ...", outputFilePath.c_str());
        // file order is RGBA = (c2, c1, c0, c3) of the reference's Mat.  The stitched image stays on the device: its samples are
        // put in file order there and the product goes out like every other TIFF of the CLI (LZW strips encoded on the device)
        const size_t bytes = nout * 2;
        if (!useGDAL && bytes / 2 < 4000000000ull) {
            write_tiff_from_device(outputFilePath, dout.p, ow, hl, MSS_BANDS, tiff_compression(TIFF_LZW), false);   // same on-disk order in and out
        } else {
            const int mat2file[4] = {2, 1, 0, 3};              // Mat channel c lives at file sample mat2file[c]
            int order[4];
            for (int b = 0; b < 4; ++b) order[b] = mat2file[bandMap ? bandMap[b] - 1 : b];
            write_tiff_from_device(outputFilePath, dout.p, ow, hl, MSS_BANDS, tiff_compression(TIFF_LZW), false, order);
        }
        // (dout is in the product's on-disk sample order by now; the average is per channel)
        if (overviews) write_overviews_of_device_image(outputFilePath + OIP_OVERVIEW_SUFFIX, dout.p, ow, hl, MSS_BANDS, *overviews);
        return outputFilePath;
    }
};
typedef ImageOperations IMO;

// ---- Stitcher (stitcher.h:18-223) ------------------------------------------------------------------
class Stitcher {
public:
    // stitcher.h:21-46; foldCols is the already-halved value (main.cpp:189)
    static std::string Stitch(const std::string &leftImagePath, const std::string &rightImagePath,
                              const std::string &outputPath = "", int foldCols = 0, int pixelsPerLine = OIP_PIXELS_PER_LINE,
                              bool useGDAL = false, const int *bandMap = nullptr, const SeamOptions *seam = nullptr,
                              const OverviewOptions *overviews = nullptr)
    {
        std::string leftExt = to_lower(std::filesystem::path(leftImagePath).extension().string());
        std::string rightExt = to_lower(std::filesystem::path(rightImagePath).extension().string());
        if (leftExt != rightExt) throw std::invalid_argument("Stitch(): two images should be same type");
        if (leftExt != ".tiff" && leftExt != ".raw") throw std::invalid_argument("Stitch(): only RAW and TIFF image supported");
        if (leftExt == ".raw") return IMO::StitchBigRaw(leftImagePath, rightImagePath, outputPath, pixelsPerLine, foldCols, seam, overviews);
        return IMO::StitchTiff(leftImagePath, rightImagePath, outputPath, foldCols, useGDAL, bandMap, seam, overviews);
    }

    Stitcher(const std::string &pan1, const std::string &pan2, const std::string &rrc1, const std::string &rrc2,
             int sections = OIP_STT_DEF_SECTIONS, int linePerSection = OIP_STT_DEF_SECLINES,
             int overlapCols = OIP_STT_DEF_OVERLAPPX, int pixelsPerLine = OIP_PIXELS_PER_LINE)
        : mFilePAN1(pan1), mFilePAN2(pan2), mParamFileRRC1(rrc1), mParamFileRRC2(rrc2), mSections(sections),
          mLinePerSection(linePerSection), mOverlapCols(overlapCols), mW(pixelsPerLine)
    {                                                                  // stitcher.h:49-81
        size_t s1 = IMO::FileSize(pan1);
        if ((size_t)sections * linePerSection * BYTES_PER_PIXEL > s1)
            throw std::invalid_argument("PAN1 size too small for SECTION & LINE_PER_SECTION argument");
        size_t s2 = IMO::FileSize(pan2);
        if ((size_t)sections * linePerSection * BYTES_PER_PIXEL > s2)
            throw std::invalid_argument("PAN2 size too small for SECTION & LINE_PER_SECTION argument");
        if (s1 != s2) throw std::invalid_argument("PAN1 size doesn't match PAN2 size");
        mSizePAN = s1;
        mLinesPAN = (int)(s1 / ((size_t)mW * BYTES_PER_PIXEL));
        OLOG("PAN: %d lines total.", mLinesPAN);
        if (mLinesPAN < sections * linePerSection)
            throw std::invalid_argument("PAN line count less than sections times line-per-section, use smaller -s and/or -l value(s)");
        mRrcFilePAN1 = mFilePAN1;
        mRrcFilePAN2 = mFilePAN2;
    }

    // The reference reads both PAN files three times (CalcSttParameters, DoRRC, PreStitch) and writes two of them
    // back in between; here each raw strip is read ONCE into HBM and every step works on the resident copy -- the
    // .RRC.RAW / .RRC.PRESTT.RAW products are still written, from the device.
    void LoadRawOnce()
    {
        const size_t npx = (size_t)mW * mLinesPAN;
        if (!mD1.p) { mD1.alloc(npx); mD1.load_file(mFilePAN1, npx); }
        if (!mD2.p) { mD2.alloc(npx); mD2.load_file(mFilePAN2, npx); }
    }

    // stitcher.h:148-201 (runs on the files mRrcFilePAN1/2 point at: the raw ones, App.B-1)
    void CalcSttParameters(double threshold = OIP_STT_DEF_PHCTHRHLD, double maxDeltaY = 0.0, int edgeCols = 0)
    {
        LoadRawOnce();
        std::vector<double> r(3 * (size_t)mSections);
        Device::get().check(oip_stt_correlate(Device::get().ctx(), mD1.p, mD2.p, mW, mLinesPAN, 0, mLinesPAN, mSections,
                                              mLinePerSection, mOverlapCols, edgeCols, r.data()));
        const CcdGeom g(mW, mLinesPAN, mSections, mLinePerSection, mOverlapCols, edgeCols);    // (the call above has checked it)
        OLOG("Calculating stitching delta values ...");
        RLOG("| offset |  delta x |  delta y | response | r |");
        RLOG("-----------------------------------------------");
        for (int i = 0; i < mSections; ++i) {
            double dx = r[3 * i], dy = r[3 * i + 1], resp = r[3 * i + 2];
            bool isValid = resp >= threshold && (maxDeltaY <= 0.0 || std::abs(dy) <= maxDeltaY);
            RLOG("|%7ld |%10.4f|%10.4f|%10.4f|%s|", g.section_start(i), dx, dy, resp, isValid ? " Y " : " N ");
        }
        int valid = 0;                                                  // stitcher.h:181-198
        if (oip_stt_mean(r.data(), mSections, threshold, maxDeltaY, &mDeltaX, &mDeltaY, &mResponse, &valid) != OIP_OK)
            throw std::runtime_error("No valid delta value found for stitching parameter calculating");
        OLOG("Total %d valid delta value pairs found, everage value:", valid);
        OLOG("    dx: %.5f, dy: %.5f, r: %.5f", mDeltaX, mDeltaY, mResponse);
    }

    // The three strip-sized products of `prestitch` (.RRC.RAW x 2, .RRC.PRESTT.RAW: 6 GB each at the 30000 x 100000 geometry) go
    // out on writer threads behind marks of the compute stream, each on a download lane of its own: a NEW file takes 6-7 GB/s
    // from one writer whatever else the process does, so three files at once are what shortens the command.
    // Finish() -- called by PreStitch, by the destructor and by the CLI -- waits for them and logs the reference's lines.
    void DoRRC()                                                        // stitcher.h:141-146
    {
        LoadRawOnce();
        mRrcFilePAN1 = IMO::BuildOutputFilePath(mFilePAN1, ".RRC");
        mRrcFilePAN2 = IMO::BuildOutputFilePath(mFilePAN2, ".RRC");
        const size_t npx = (size_t)mW * mLinesPAN;
        DevBuf<double> kb((size_t)mW * 2);
        oip_ctx *ctx = Device::get().ctx();
        for (int c = 0; c < 2; ++c) {                                   // IMO::DoRRC4RAW on the resident strip
            const std::vector<double> prm = IMO::LoadLut(c ? mParamFileRRC2 : mParamFileRRC1, mW);
            kb.upload(prm.data(), prm.size());
            DevBuf<uint16_t> &d = c ? mD2 : mD1;
            OLOG("Do inplace RRC ...");
            stop_watch sw;
            Device::get().check(oip_rrc_u16(ctx, d.p, d.p, mW, (long)mLinesPAN, kb.p));
            Device::get().check(oip_sync(ctx));
            double es = sw.tick();
            OLOG("Done for %zu bytes in %.3f seconds (%.1f MBps).", mSizePAN, es, mSizePAN / es / (1024.0 * 1024.0));
            const std::string save = c ? mRrcFilePAN2 : mRrcFilePAN1;
            OLOG("Write RRC result as file \"%s\" ...", save.c_str());
            long mark = 0;
            Device::get().check(oip_compute_mark(ctx, &mark));
            const uint16_t *src = d.p;
            const size_t bytes = mSizePAN;
            (void)npx;
            mWriter[c].post([=] {
                stop_watch w;
                { FILE *f = fopen(save.c_str(), "wb"); if (!f) throw std::runtime_error("open file [" + save + "] failed: " + std::to_string(errno)); fclose(f); }
                Device::get().check(oip_write_device_to_file_at(ctx, src, bytes, save.c_str(), 0, mark));
                const double s = w.tick();
                OLOG("%zu bytes written in %.3f seconds (%.1f MBps).", bytes, s, bytes / s / (1024.0 * 1024.0));
            });
        }
    }

    // fp16acc: the fp16-accumulate resampling variant (BASELINE config 5; not the parity mode)
    int PreStitch(bool fp16acc = false)                                 // stitcher.h:83-139
    {
        LoadRawOnce();                                                  // mD2 holds what mRrcFilePAN2 names (raw with --no-rrc)
        mPreSttFilePAN2 = IMO::BuildOutputFilePath(mRrcFilePAN2, ".PRESTT");
        const size_t npx = (size_t)mW * mLinesPAN;
        oip_ctx *ctx = Device::get().ctx();
        stop_watch sw;
        mPre.alloc(npx);
        auto fn = fp16acc ? oip_remap_shift_bicubic_u16_f16acc : oip_remap_shift_bicubic_u16;
        Device::get().check(fn(ctx, mD2.p, 0, mLinesPAN, mPre.p, 0, mLinesPAN, mW, mLinesPAN, mDeltaX, mDeltaY,
                               OIP_REMAP_SECTION_ROWS, OIP_REMAP_ROW_GUARD));
        long mark = 0;
        Device::get().check(oip_compute_mark(ctx, &mark));
        const std::string save = mPreSttFilePAN2;
        const uint16_t *src = mPre.p;
        const size_t bytes = mSizePAN;
        mWriter[2].post([=] {
            { FILE *f = fopen(save.c_str(), "wb"); if (!f) throw std::runtime_error("open file [" + save + "] failed: " + std::to_string(errno)); fclose(f); }
            Device::get().check(oip_write_device_to_file_at(ctx, src, bytes, save.c_str(), 0, mark));
        });
        Finish();
        double es = sw.tick();
        OLOG("Pre-stitched PAN2 written to file '%s'.", mPreSttFilePAN2.c_str());
        OLOG("%zu bytes processed & written in %.3f seconds (%.1f MBps).", mSizePAN, es, mSizePAN / es / (1024.0 * 1024.0));
        const int ucut = mDeltaY >= 0.0 ? 0 : (int)(-mDeltaY) + 1, bcut = mDeltaY >= 0.0 ? (int)mDeltaY + 1 : 0;
        return mLinesPAN - (ucut + bcut);        // SectionaryRemap's returned row_offset
    }

    // every product posted so far is on disk when this returns (the first failure of a writer is re-thrown)
    void Finish()
    {
        for (auto &w : mWriter) w.finish();
    }

    double deltaX() const { return mDeltaX; }
    double deltaY() const { return mDeltaY; }
    double response() const { return mResponse; }

private:
    std::string mFilePAN1, mFilePAN2, mParamFileRRC1, mParamFileRRC2, mRrcFilePAN1, mRrcFilePAN2, mPreSttFilePAN2;
    double mDeltaX = 0, mDeltaY = 0, mResponse = 0;
    size_t mSizePAN = 0;
    int mSections, mLinePerSection, mOverlapCols, mLinesPAN = 0, mW;
    DevBuf<uint16_t> mD1, mD2, mPre;            // the two strips, resident from the first step that needs them; the resampled CCD 2
    JobThread mWriter[3];                       // (declared after the buffers: joined before they are released)
};

// ---- PreProcessor (preproc.h:30-599) ---------------------------------------------------------------
// the fitted polynomials as preproc.h:339-344 logs them
inline void LogShiftCoeffs(const double cx[MSS_BANDS][2], const double cy[MSS_BANDS][3])
{
    for (int b = 0; b < MSS_BANDS; ++b) {
        OLOG("BAND %d\tdeltaX coeff: [1] %.15f, [0] %.9f", b, cx[b][1], cx[b][0]);
        OLOG("\tdeltaY coeff: [2] %.15f, [1] %.15f, [0] %.9f", cy[b][2], cy[b][1], cy[b][0]);
    }
}

class PreProcessor {
public:
    // CheckFilesAttributes' size rules (preproc.h:565-571)
    static void CheckStripSizes(size_t sizePAN, size_t sizeMSS, size_t lineBytes)
    {
        if (sizePAN != MSS_BANDS * sizeMSS)
            throw std::runtime_error("PAN file size does not match MSS file size: PAN file should be " + std::to_string(MSS_BANDS) +
                                     "x as large as MSS file");
        if (sizePAN % lineBytes != 0)
            throw std::runtime_error("PAN file size invalid: should be multiplies of " + std::to_string(lineBytes));
    }

    PreProcessor(const std::string &panFile, const std::string &mssFile, const std::string &rrcFile4PAN,
                 const std::string rrcFile4MSSBand[MSS_BANDS], int pixelsPerLine = OIP_PIXELS_PER_LINE)
        : mPanFile(panFile), mMssFile(mssFile), mRrcPanFile(rrcFile4PAN), mW(pixelsPerLine)
    {
        for (int i = 0; i < MSS_BANDS; ++i) mRrcMssBndFile[i] = rrcFile4MSSBand[i];
        CheckFilesAttributes();
    }

    void LoadPAN()                                                      // preproc.h:51-54
    {
        OLOG("Loading PAN raw image ...");
        mPAN.alloc(mSizePAN / 2);
        mPAN.load_file(mPanFile, mSizePAN / 2);
    }

    // Fused task: the PAN strip is already on the device (RRC'd / pre-stitched by the
    // previous step of the same process) -- no file round trip.  Not owned.
    void UseDevicePAN(const uint16_t *d_pan) { mPanView = d_pan; }

    // --fit reference (default): NumCpp Poly1d::fit as the reference calls it; --fit lstsq: QR on a scaled abscissa
    void SetFitMode(int mode) { mFitMode = mode; }

    void LoadMSS()                                                      // preproc.h:56-80 (split deferred to DoRRC4MSS)
    {
        OLOG("Loading MSS raw image ...");
        mMssBil.alloc(mSizeMSS / 2);
        mMssBil.load_file(mMssFile, mSizeMSS / 2);
        mPlaneStride = (size_t)(mW / MSS_BANDS) * mLinesMSS;
        mPlanes.alloc(mPlaneStride * MSS_BANDS);
        Device::get().check(oip_sync(Device::get().ctx()));
        mSplitDone = false;
    }

    void DoRRC4PAN()                                                    // preproc.h:188-200
    {
        if (!mPAN.p) throw std::logic_error("PAN raw image data not loaded, call `LoadPAN()' first");
        const std::vector<double> prm = IMO::LoadLut(mRrcPanFile, mW);
        DevBuf<double> kb;
        kb.assign(prm);
        OLOG("Begin inplace RRC for PAN data ... ");
        stop_watch sw;
        Device::get().check(oip_rrc_u16(Device::get().ctx(), mPAN.p, mPAN.p, mW, (long)mLinesPAN, kb.p));
        Device::get().check(oip_sync(Device::get().ctx()));
        double es = sw.tick();
        OLOG("RRC for PAN done in %.4f seconds (%.1f MBps).", es, mSizePAN / es / 1024.0 / 1024.0);
    }

    // preproc.h:202-222; doRRC=false is --no-rrc4mss (split only)
    void DoRRC4MSS(bool doRRC = true)
    {
        if (!mMssBil.p) throw std::logic_error("MSS raw image data not loaded, call `LoadMSS()' first");
        DevBuf<double> kb;
        if (doRRC) kb.assign(IMO::LoadMssLuts(mRrcMssBndFile, mW));
        OLOG("Splitting %d bands of MSS image%s ...", MSS_BANDS, doRRC ? " with inplace RRC" : "");
        stop_watch sw;
        Device::get().check(oip_mss_split_rrc_u16(Device::get().ctx(), mMssBil.p, mPlanes.p, mPlaneStride, mW, (long)mLinesMSS,
                                                  doRRC ? kb.p : nullptr));
        Device::get().check(oip_sync(Device::get().ctx()));
        double es = sw.tick();
        OLOG("RRC done for MSS bands in %.4f seconds (%.1f MBps).", es, mSizeMSS / es / 1024.0 / 1024.0);
        mMssBil.release();
        mSplitDone = true;
    }

    void CalcInterBandCorrelation(int slices = OIP_IBCV_DEF_SLICES, int sections = OIP_IBCV_DEF_SECTIONS,
                                  double threshold = OIP_IBCV_DEF_THRESHOLD, bool autoUnloadPAN = true)
    {                                                                   // preproc.h:224-347
        if (!mSplitDone) DoRRC4MSS(false);
        OLOG("Calculating inter-band correlation with %d slices in %d section(s) ...", slices, sections);
        const int n = slices * sections;
        std::vector<double> t((size_t)MSS_BANDS * n * 4);
        stop_watch sw;
        const uint16_t *pan = mPanView ? mPanView : mPAN.p;
        if (!pan) throw std::logic_error("PAN raw image data not loaded, call `LoadPAN()' first");
        Device::get().check(oip_interband_correlate(Device::get().ctx(), pan, (long)mLinesPAN, 0, (long)mLinesPAN, mPlanes.p,
                                                    mPlaneStride, 0, (long)mLinesMSS, mW, slices, sections,
                                                    OIP_CORRELATION_LINES, t.data()));
        OLOG("Inter-band correlation finished in %.3f seconds, result:", sw.tick());
        FitShiftTable(t, slices, sections, threshold);
        if (autoUnloadPAN) mPAN.release();
    }

    // preproc.h:351-425 (+ inner :428-468); writes <stem>.ALIGNED.TIFF
    // keepOnDevice (fused task): the aligned 16UC4 image stays on the device (swapped into *keepOnDevice,
    // *keptRows lines) and no file is written
    void DoInterBandAlignment(int linePerSection, int lineOffset = 0, int sectionOverlap = OIP_IBPA_DEFAULT_LINEOVERLAP,
                              bool keepLeadingLines = false, bool autoUnloadRawMSS = true, DevBuf<uint16_t> *keepOnDevice = nullptr,
                              long *keptRows = nullptr)
    {
        OLOG("Doing inter-band alignment ...");
        const int Wb = mW / MSS_BANDS;
        const long rows = (long)mLinesMSS - lineOffset - (keepLeadingLines ? 0 : sectionOverlap);
        if (rows <= 0) throw std::invalid_argument("Too few image lines left to process");
        DevBuf<uint16_t> out((size_t)rows * Wb * MSS_BANDS);
        long processed = 0;
        stop_watch sw;
        Device::get().check(oip_align_mss_bicubic_u16x4(Device::get().ctx(), mPlanes.p, mPlaneStride, 0, (long)mLinesMSS, out.p, 0,
                                                        rows, Wb, (long)mLinesMSS, &mDeltaXcoeffs[0][0], &mDeltaYcoeffs[0][0],
                                                        linePerSection, lineOffset, sectionOverlap, keepLeadingLines ? 1 : 0,
                                                        OIP_IBPA_MIN_PROCESSLINES, &processed));
        Device::get().check(oip_sync(Device::get().ctx()));
        OLOG("Alignment done in %.3f seconds (%ld lines valid of %ld).", sw.tick(), processed, rows);
        if (keepOnDevice) {
            keepOnDevice->swap(out);
            if (keptRows) *keptRows = rows;
        } else {
            // preproc.h:167-185 WriteAlignedMSS_TIFF: 4-channel 16-bit TIFF, samples in OpenCV's on-disk order
            auto save = IMO::BuildOutputFilePath(mMssFile, ".ALIGNED", ".TIFF");
            OLOG("Outputing aligned TIFF image (%d x %ld x 4) to [%s] ...", Wb, rows, save.c_str());
            write_tiff_from_device(save, out.p, Wb, rows, MSS_BANDS, tiff_compression(TIFF_LZW), true);
            OLOG("Output done.");
        }
        if (autoUnloadRawMSS) mPlanes.release();
        OLOG("DoInterBandAlignment(): done.");
    }

    void WriteRRCedPAN()                                                // preproc.h:93-105
    {
        auto save = IMO::BuildOutputFilePath(mPanFile, ".RRC");
        mPAN.save_file(save, mSizePAN / 2);
        OLOG("Written to file [%s].", save.c_str());
    }

    // ---- the default action (main.cpp:288-317) as ONE pipeline ------------------------------------------------------
    // The reference runs LoadPAN, LoadMSS, DoRRC4PAN, DoRRC4MSS, CalcInterBandCorrelation and DoInterBandAlignment one after
    // the other, each over the whole strip (preproc.h:51-80, :188-222, :224-347, :351-425), and so do the step methods above.
    // Here three host threads share the context:
    //   reader   the two RAW files go file -> pinned ring -> HBM (oip_read_file_to_device, parallel pread) in the order the
    //            arithmetic needs them: per correlation section its MSS lines, then its PAN lines in blocks; the MSS lines
    //            between the sections; the PAN lines between the sections last.  Every block carries a ticket.
    //   compute  (this thread) waits for a block's ticket on the device, corrects it (RRC in place / BIL split + RRC), runs a
    //            section's phase correlations as soon as its lines are resident (the pairs of units of the one-call form are
    //            kept, so the shifts are the serial run's bits), then filter + fit, the alignment kernel and the sample
    //            permutation of the product -- while the reader is still bringing the PAN lines between the sections.
    //   writers  <pan>.RRC.RAW goes out block by block behind the RRC kernel of each block (--write-rrcpan), the aligned image
    //            goes HBM -> pinned -> <mss>.ALIGNED.TIFF (uncompressed: straight into the file's pixel payload; LZW: strips
    //            encoded on a few threads as their lines come down).
    // Products are byte-identical to the step-by-step flow's (tests/test_gpu_cli.py runs both; OIP_PIPELINE=0 selects the steps).
    struct DefaultActionOptions {
        bool doRRC4PAN = false, writeRrcPan = false, doRRC4MSS = true, keepLeading = false;
        int slices = OIP_IBCV_DEF_SLICES, sections = OIP_IBCV_DEF_SECTIONS;
        double threshold = OIP_IBCV_DEF_THRESHOLD;
        int linesSection = OIP_IBPA_DEFAULT_BATCHLINES, lineOffset = 0, overlapLines = OIP_IBPA_DEFAULT_LINEOVERLAP;
    };

    // The locals stand in the order their lifetimes need: what a thread's jobs use is declared before the object that owns the
    // thread, and the reader -- declared last -- is stopped first, whatever is thrown.
    void RunPipelined(const DefaultActionOptions &o)
    {
        oip_ctx *ctx = Device::get().ctx();
        auto ck = [](int rc) { Device::get().check(rc); };
        PipelineTimes t;
        const int W = mW, Wb = W / MSS_BANDS;
        const long Lp = (long)mLinesPAN, Lm = (long)mLinesMSS;
        // the argument checks of CalcInterBandCorrelation (preproc.h:228-237) and DoInterBandAlignment, before a byte is read
        std::string refused = InterBandArgCheck(Lp, o.slices, o.sections, OIP_CORRELATION_LINES);
        if (!refused.empty()) throw std::invalid_argument(refused);
        const long outRows = Lm - o.lineOffset - (o.keepLeading ? 0 : o.overlapLines);
        if (outRows <= 0) throw std::invalid_argument("Too few image lines left to process");
        InterBandGeom g;
        refused = MakeInterBandGeom(W, Lp, o.slices, o.sections, OIP_CORRELATION_LINES, &g);
        if (!refused.empty()) throw std::invalid_argument(refused);
        if (g.mss_start(g.sections - 1) + g.band_rows > Lm) throw std::invalid_argument("oip_interband_correlate: section outside the strip");
        mPAN.alloc((size_t)W * Lp);
        mMssBil.alloc((size_t)W * Lm);
        mPlaneStride = (size_t)Wb * Lm;
        mPlanes.alloc(mPlaneStride * MSS_BANDS);
        DevBuf<uint16_t> out((size_t)outRows * Wb * MSS_BANDS);
        DevBuf<double> kbPan, kbMss;
        t.setup = seconds_since(t.t0);
        const std::vector<ArrivalItem> order = ArrivalOrder(g, Lm, std::max<long>(1, (long)(((size_t)256 << 20) / ((size_t)W * BYTES_PER_PIXEL))));
        const std::string rrcPanPath = IMO::BuildOutputFilePath(mPanFile, ".RRC");
        AlignedProduct product(IMO::BuildOutputFilePath(mMssFile, ".ALIGNED", ".TIFF"), Wb, outRows);
        JobThread panWriter;
        StripReader reader(*this, order, t);
        product.prepare();
        PrepareWhileReading(o, g, kbPan, kbMss, rrcPanPath, &t);

        std::vector<double> table((size_t)MSS_BANDS * g.n_units * 4);
        ShiftTableInit(g, table.data());
        int unitsDone = 0;
        for (const ArrivalItem &it : order) {
            if (it.kind == ArrivalItem::kMss || it.kind == ArrivalItem::kPan) reader.wait_next();
            if (it.kind == ArrivalItem::kMss)
                ck(oip_mss_split_rrc_u16(ctx, mMssBil.p + (size_t)it.a * W, mPlanes.p + (size_t)it.a * Wb, mPlaneStride, W, it.b - it.a, kbMss.p));
            else if (it.kind == ArrivalItem::kPan) CorrectPanBlock(o, it, kbPan.p, panWriter, rrcPanPath);
            else if (it.kind == ArrivalItem::kUnits) CorrelateUnitsThrough(g, (int)it.a, &unitsDone, table.data(), &t);
            else FitAlignAndPost(o, table, out.p, outRows, product, &t);       // every section and every MSS line is in
        }
        reader.finish();
        ck(oip_sync(ctx));
        t.computeDone = seconds_since(t.t0);
        OLOG("%zu bytes read in %.3f seconds (%.1f MBps).", mSizePAN + mSizeMSS, t.readDone, (mSizePAN + mSizeMSS) / t.readDone / 1024.0 / 1024.0);
        if (o.doRRC4PAN) OLOG("RRC for PAN done in %.4f seconds (%.1f MBps).", t.computeDone, mSizePAN / t.computeDone / 1024.0 / 1024.0);
        OLOG("RRC done for MSS bands in %.4f seconds (%.1f MBps).", t.computeDone, mSizeMSS / t.computeDone / 1024.0 / 1024.0);
        panWriter.finish();
        if (o.writeRrcPan) OLOG("Written to file [%s].", rrcPanPath.c_str());
        // the strips are done with: their 9 GB go back while the product is still on its way to the file (releasing them is a
        // good part of what a process of this size pays at exit)
        mMssBil.release();
        mPlanes.release();
        mPAN.release();
        product.finish();
        t.all = seconds_since(t.t0);
        OLOG("DoInterBandAlignment(): done.");
        t.log(mSizePAN + mSizeMSS, product.bytes() + (o.writeRrcPan ? mSizePAN : 0));
    }

    const double *deltaXcoeffs() const { return &mDeltaXcoeffs[0][0]; }
    const double *deltaYcoeffs() const { return &mDeltaYcoeffs[0][0]; }

private:
    // ---- the parts of RunPipelined ----
    // seconds since the action started, and the one line harnesses read (bench.py's `cli` object)
    struct PipelineTimes {
        const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        double setup = 0, prepared = 0, readDone = 0, corrDone = 0, alignDone = 0, computeDone = 0, all = 0;
        std::string corrCalls;                             // start+duration of every correlation call, ms
        void log(size_t bytesRead, size_t bytesWritten) const
        {
            double lane[4] = {0, 0, 0, 0};                   // the reader's own time: in pread (all pool threads), waiting for a ring slot's DMA
            oip_stage_stats(Device::get().ctx(), lane, 0);
            RLOG("TIMING default_action pipelined=1 setup=%.4f prepared=%.4f read_done=%.4f correlation_done=%.4f aligned=%.4f compute_done=%.4f products_written=%.4f "
                 "device_create=%.4f since_process_start=%.4f reader_in_pread=%.4f reader_waiting_for_slot=%.4f bytes_read=%zu bytes_written=%zu "
                 "correlation_calls_ms=%s",
                 setup, prepared, readDone, corrDone, alignDone, computeDone, all, Device::get().create_seconds(), seconds_since(process_start()), lane[0], lane[1],
                 bytesRead, bytesWritten, corrCalls.c_str());
        }
    };

    // The reader: the two RAW files go file -> pinned ring -> HBM in the order of arrival, a ticket per read item.  Its thread
    // is a JobThread's, joined by that member's destructor: nothing can stand between the thread's start and its guard.
    class StripReader {
    public:
        StripReader(PreProcessor &pp, const std::vector<ArrivalItem> &order, PipelineTimes &times)
        {
            OLOG("Loading PAN raw image ...");
            OLOG("Loading MSS raw image ...");
            OLOG("Reading raw image from file `%s' ...", pp.mPanFile.c_str());
            OLOG("Reading raw image from file `%s' ...", pp.mMssFile.c_str());
            mThread.post([this, &pp, &order, &times] {
                const size_t lineBytes = (size_t)pp.mW * BYTES_PER_PIXEL;
                try {
                    for (const ArrivalItem &it : order) {
                        if (it.kind != ArrivalItem::kMss && it.kind != ArrivalItem::kPan) continue;
                        if (mCancel.load()) break;
                        const bool pan = it.kind == ArrivalItem::kPan;
                        const size_t off = (size_t)it.a * lineBytes, n = (size_t)(it.b - it.a) * lineBytes;
                        size_t got = 0;
                        long t = 0;
                        Device::get().check(oip_read_file_to_device(Device::get().ctx(), (pan ? pp.mPanFile : pp.mMssFile).c_str(), off, n,
                                                                    (char *)(pan ? pp.mPAN.p : pp.mMssBil.p) + off, &got, &t));
                        if (got != n)
                            throw std::runtime_error("file size(" + std::to_string(pan ? pp.mSizePAN : pp.mSizeMSS) + ") doesn't match with read byte count(" +
                                                     std::to_string(off + got) + ")");
                        mTickets.push(t);
                    }
                    times.readDone = seconds_since(times.t0);
                } catch (...) {
                    mTickets.push(-1);
                    throw;
                }
            });
        }
        ~StripReader() { mCancel = true; }
        // the next read item: the compute stream waits for it on the device; a failure of the reader is raised here
        void wait_next()
        {
            const long t = mTickets.pop();
            if (t < 0) finish();
            Device::get().check(oip_stage_wait(Device::get().ctx(), t));
        }
        void finish() { mThread.finish(); }
    private:
        BlockingQueue<long> mTickets;                      // one per read item, in order; -1: the reader failed
        std::atomic<bool> mCancel{false};
        JobThread mThread;
    };

    // <mss>.ALIGNED.TIFF of the pipeline.  The file exists from the start -- its blocks are reserved on the writer thread while
    // the strip is still being read -- and a run that fails takes it away again.  The writer thread is declared (and started,
    // idle) before the file is created: nothing in the constructor can throw once the file is there, so the destructor, which
    // lets the writer finish its jobs before what they use goes, always gets to take a failed run's file away.
    struct AlignedProduct {
        const std::string path;
        const int comp, Wb;
        const long rows;
        bool done = false;
        oip_file_sink *sink = nullptr;                     // the product's prepared file (uncompressed products)
        uint64_t payloadAt = 0;
        JobThread writer;
        TiffWriterU16 tiff;
        std::unique_ptr<TiffStripPrep> stripPrep;

        size_t bytes() const { return (size_t)rows * Wb * MSS_BANDS * 2; }
        // the strips of a compressed product are encoded on the device
        bool on_device() const
        {
            const long rps = tiff.rows_per_strip();
            return tiff_on_device(comp, OIP_TIFF_WRITE, (size_t)((rows + rps - 1) / rps), (uint64_t)rps * Wb * MSS_BANDS * 2);
        }
        AlignedProduct(const std::string &path_, int Wb_, long rows_)
            : path(path_), comp(tiff_compression(TIFF_LZW)), Wb(Wb_), rows(rows_), tiff(path, Wb, rows, MSS_BANDS, false, comp)
        {
        }
        ~AlignedProduct()
        {
            try { writer.finish(); } catch (...) {}
            if (sink) oip_file_sink_close(nullptr, sink);
            if (!done) ::remove(path.c_str());
        }
        // what the writer thread does while the strip is being read.  Called once the reader has started: the jobs pin memory and
        // reserve the file's blocks, and the first section's lines should not start behind that
        void prepare()
        {
            oip_ctx *ctx = Device::get().ctx();
            // (an empty transfer: the writer's download lane pins its two slots now, not when the product is waiting for them)
            writer.post([=] { Device::get().check(oip_download_staged_after(ctx, nullptr, nullptr, 0, 0)); });
            if (comp != TIFF_NONE && on_device()) {
                // likewise for the LZW or Deflate product: device buffers of the strip encoder, the file reserved at its worst-case size
                stripPrep.reset(new TiffStripPrep());
                writer.post([this] { stripPrep->prepare(tiff, path, Wb, rows, MSS_BANDS, comp, true); });
            }
            if (comp == TIFF_NONE) {
                // the writer thread has nothing to do until the fit is in: it prepares the product file -- header out, blocks
                // reserved, pages mapped and populated (oip_file_sink_open) -- so that the pixels, when they exist, are copied
                // into pages that exist (the allocation is what bounds a buffered write of a new file)
                writer.post([this, ctx] {
                    payloadAt = tiff.begin_external_payload();
                    Device::get().check(oip_file_sink_open(ctx, path.c_str(), (size_t)payloadAt + bytes(), &sink));
                });
            }
        }
        // the image (rows x Wb x 4 u16 in file sample order, complete at `mark` of the compute stream) goes to the file
        void post_write(const uint16_t *img, long mark, long processed, PipelineTimes *times)
        {
            oip_ctx *ctx = Device::get().ctx();
            writer.post([this, ctx, img, mark, processed, times] {
                Device::get().check(oip_compute_mark_sync(ctx, mark));
                times->alignDone = seconds_since(times->t0);
                OLOG("Alignment done in %.3f seconds (%ld lines valid of %ld).", times->alignDone, processed, rows);
                OLOG("Outputing aligned TIFF image (%d x %ld x 4) to [%s] ...", Wb, rows, path.c_str());
                if (comp == TIFF_NONE) {
                    Device::get().check(oip_file_sink_write(ctx, sink, (size_t)payloadAt, img, bytes(), mark));
                    oip_file_sink *k = sink;
                    sink = nullptr;
                    Device::get().check(oip_file_sink_close(ctx, k));
                    tiff.end_external_payload();
                } else if (on_device()) {
                    tiff_strips_from_device(tiff, path, img, Wb, rows, MSS_BANDS, comp, stripPrep.get());
                } else {
                    tiff_rows_from_device(tiff, img, rows, (size_t)Wb * MSS_BANDS, mark);     // download || encode || write
                }
                tiff.close();
                OLOG("Output done.");
            });
        }
        // the product is on disk when this returns (a failure of the writer is re-thrown)
        void finish() { writer.finish(); done = true; }
    };

    // while the first section is on its way: the LUTs, and everything the first correlation call would otherwise set up behind
    // the data -- FFT plans and twiddles, the up-sampling operator's tables, the workspace (a call with no units does just that)
    void PrepareWhileReading(const DefaultActionOptions &o, const InterBandGeom &g, DevBuf<double> &kbPan, DevBuf<double> &kbMss,
                             const std::string &rrcPanPath, PipelineTimes *t)
    {
        if (o.doRRC4PAN) kbPan.assign(IMO::LoadLut(mRrcPanFile, mW));
        if (o.doRRC4MSS) kbMss.assign(IMO::LoadMssLuts(mRrcMssBndFile, mW));
        Device::get().check(oip_interband_correlate_units(Device::get().ctx(), nullptr, nullptr, nullptr, nullptr, 0, g.base_rows, g.base_cols, nullptr));
        t->prepared = seconds_since(t->t0);
        if (o.writeRrcPan) {                               // sized up front: blocks land at their offsets in any order
            FILE *f = fopen(rrcPanPath.c_str(), "wb");
            if (!f) throw std::runtime_error("open file [" + rrcPanPath + "] failed: " + std::to_string(errno));
            fclose(f);
        }
        if (o.doRRC4PAN) OLOG("Begin inplace RRC for PAN data ... ");
        OLOG("Splitting %d bands of MSS image%s ...", MSS_BANDS, o.doRRC4MSS ? " with inplace RRC" : "");
        OLOG("Calculating inter-band correlation with %d slices in %d section(s) ...", o.slices, o.sections);
    }

    // a PAN block is resident: RRC in place; --write-rrcpan: out to its place in the file behind a mark of the RRC kernel
    void CorrectPanBlock(const DefaultActionOptions &o, const ArrivalItem &it, const double *kbPan, JobThread &panWriter, const std::string &rrcPanPath)
    {
        oip_ctx *ctx = Device::get().ctx();
        uint16_t *blk = mPAN.p + (size_t)it.a * mW;
        if (o.doRRC4PAN) Device::get().check(oip_rrc_u16(ctx, blk, blk, mW, it.b - it.a, kbPan));
        if (!o.writeRrcPan) return;
        long mark = 0;
        Device::get().check(oip_compute_mark(ctx, &mark));
        const size_t lineBytes = (size_t)mW * BYTES_PER_PIXEL, off = (size_t)it.a * lineBytes, nb = (size_t)(it.b - it.a) * lineBytes;
        panWriter.post([=] { Device::get().check(oip_write_device_to_file_at(ctx, blk, nb, rrcPanPath.c_str(), off, mark)); });
    }

    // section `sec` is resident: the units that may run now (InterBandGeom::units_through) in one call, their shifts into the table
    void CorrelateUnitsThrough(const InterBandGeom &g, int sec, int *unitsDone, double *table, PipelineTimes *t)
    {
        const int first = *unitsDone, cnt = g.units_through(sec) - first;
        if (cnt <= 0) return;
        std::vector<const uint16_t *> dPan(cnt), dBands((size_t)cnt * MSS_BANDS);
        std::vector<size_t> panPitch(cnt, (size_t)g.W), bandPitch(cnt, (size_t)g.Wb);
        for (int j = 0; j < cnt; ++j) {
            const int u = first + j, us = u / g.slices, i = u % g.slices;
            dPan[j] = mPAN.p + (size_t)g.pan_start(us) * g.W + (size_t)i * g.base_cols;
            for (int b = 0; b < MSS_BANDS; ++b)
                dBands[(size_t)j * MSS_BANDS + b] = mPlanes.p + (size_t)b * mPlaneStride + (size_t)g.mss_start(us) * g.Wb + (size_t)i * g.band_cols;
        }
        std::vector<double> r((size_t)12 * cnt);
        const double tc0 = seconds_since(t->t0);
        Device::get().check(oip_interband_correlate_units(Device::get().ctx(), dPan.data(), panPitch.data(), dBands.data(), bandPitch.data(), cnt, g.base_rows,
                                                          g.base_cols, r.data()));
        t->corrCalls += (t->corrCalls.empty() ? "" : ",") + std::to_string((int)(tc0 * 1e3)) + "+" + std::to_string((int)((seconds_since(t->t0) - tc0) * 1e3));
        for (int j = 0; j < cnt; ++j) ShiftTablePut(g, table, first + j, &r[(size_t)12 * j]);
        *unitsDone = first + cnt;
        if (sec == g.sections - 1) t->corrDone = seconds_since(t->t0);
    }

    // filter, fit, the alignment kernel, and the image on its way to the product
    void FitAlignAndPost(const DefaultActionOptions &o, const std::vector<double> &table, uint16_t *out, long outRows, AlignedProduct &product, PipelineTimes *t)
    {
        oip_ctx *ctx = Device::get().ctx();
        const int Wb = mW / MSS_BANDS;
        OLOG("Inter-band correlation finished in %.3f seconds, result:", t->corrDone);
        FitShiftTable(table, o.slices, o.sections, o.threshold);
        OLOG("Doing inter-band alignment ...");
        long processed = 0, mark = 0;
        Device::get().check(oip_align_mss_bicubic_u16x4(ctx, mPlanes.p, mPlaneStride, 0, (long)mLinesMSS, out, 0, outRows, Wb, (long)mLinesMSS, &mDeltaXcoeffs[0][0],
                                                        &mDeltaYcoeffs[0][0], o.linesSection, o.lineOffset, o.overlapLines, o.keepLeading ? 1 : 0,
                                                        OIP_IBPA_MIN_PROCESSLINES, &processed));
        // preproc.h:167-185 WriteAlignedMSS_TIFF: cv::imwrite stores the Mat's channels (c0,c1,c2,c3) as samples (c2,c1,c0,c3);
        // the image takes that order on the device, so its lines go from HBM into the file as they are
        const int fileOrder[4] = {2, 1, 0, 3};
        Device::get().check(oip_permute_u16x4(ctx, out, (size_t)outRows * Wb, fileOrder));
        Device::get().check(oip_compute_mark(ctx, &mark));
        product.post_write(out, mark, processed, t);
    }

    // the shift table [band][unit][dx, dy, rs, cx] of all units: dumped (preproc.h:470-490), filtered and fitted (:331-346)
    void FitShiftTable(const std::vector<double> &table, int slices, int sections, double threshold)
    {
        const int n = slices * sections, sliceCols = mW / slices;
        RLOG("|#SLC|Start|Center| End |   B1.x   |   B2.x   |   B3.x   |   B4.x   |   B1.y   |   B2.y   |   B3.y   |   B4.y   "
             "|   B1.r   |   B2.r   |   B3.r   |   B4.r   |");
        for (int u = 0; u < n; ++u) {
            auto v = [&](int b, int k) { return table[((size_t)b * n + u) * 4 + k]; };
            const int i = u % slices;
            RLOG("|%4d|%5d|%6d|%5d|%10.4f|%10.4f|%10.4f|%10.4f|%10.4f|%10.4f|%10.4f|%10.4f|%10.4f|%10.4f|%10.4f|%10.4f|", i, i * sliceCols, (int)v(0, 3),
                 (i + 1) * sliceCols, v(0, 0), v(1, 0), v(2, 0), v(3, 0), v(0, 1), v(1, 1), v(2, 1), v(3, 1), v(0, 2), v(1, 2), v(2, 2), v(3, 2));
        }
        OLOG("Filter invalid correlation values & try polynomial fitting ...");
        char err[512];
        int rc = oip_filter_and_fit_mode(table.data(), n, threshold, OIP_IBCV_MIN_COUNT, mFitMode, &mDeltaXcoeffs[0][0], &mDeltaYcoeffs[0][0], err, sizeof err);
        if (rc != OIP_OK) { OLOG("%s.", err); throw std::runtime_error(err); }
        LogShiftCoeffs(mDeltaXcoeffs, mDeltaYcoeffs);
        OLOG("CalcInterBandCorrelation(): done.");
    }

    void CheckFilesAttributes()                                         // preproc.h:552-572
    {
        OLOG("Checking PAN raw file attributes ...");
        mSizePAN = IMO::FileSize(mPanFile);
        const size_t lineBytes = (size_t)mW * BYTES_PER_PIXEL;
        mLinesPAN = mSizePAN / lineBytes;
        OLOG("Checking MSS raw file attributes ...");
        mSizeMSS = IMO::FileSize(mMssFile);
        mLinesMSS = mSizeMSS / lineBytes;
        CheckStripSizes(mSizePAN, mSizeMSS, lineBytes);
        OLOG("CheckFilesAttributes(): OK.");
    }

    const std::string mPanFile, mMssFile, mRrcPanFile;
    std::string mRrcMssBndFile[MSS_BANDS];
    int mW;
    size_t mSizePAN = 0, mSizeMSS = 0, mLinesPAN = 0, mLinesMSS = 0, mPlaneStride = 0;
    DevBuf<uint16_t> mPAN, mMssBil, mPlanes;
    const uint16_t *mPanView = nullptr;
    bool mSplitDone = false;
    int mFitMode = OIP_FIT_REFERENCE;
    double mDeltaXcoeffs[MSS_BANDS][2] = {};
    double mDeltaYcoeffs[MSS_BANDS][3] = {};
};

// ---- fused task ---------------------------------------------------------------
// DOC/sample-task.sh runs five commands -- prestitch, stitch (PAN), the default action for each CCD,
// stitch (MSS) -- that hand 6 strip-sized files to one another through the file system.  Here the same
// steps run in one process with every intermediate resident in HBM: four RAW inputs are read once, two
// TIFFs are written.  Each step is the very code path of the stand-alone command (same C-ABI calls, same
// parameters), so the two products are identical to the five-command flow's; tests/test_gpu_cli.py
// compares them.
struct TaskOptions {
    int width = OIP_PIXELS_PER_LINE;
    // prestitch
    int sections = OIP_STT_DEF_SECTIONS, sectionLines = OIP_STT_DEF_SECLINES, overlapCols = OIP_STT_DEF_OVERLAPPX, edgeCols = 0;
    double sttThreshold = OIP_STT_DEF_PHCTHRHLD, sttMaxDeltaY = 0.0;
    // stitching (as given on the command line: halved like main.cpp:189)
    int foldColsPAN = 0, foldColsMSS = 0;
    bool useGDAL = false;
    const int *bandMap = nullptr;
    // default action
    int slices = OIP_IBCV_DEF_SLICES, ibcSections = OIP_IBCV_DEF_SECTIONS, linesSection = OIP_IBPA_DEFAULT_BATCHLINES, lineOffset = 0,
        overlapLines = OIP_IBPA_DEFAULT_LINEOVERLAP;
    double ibcThreshold = OIP_IBCV_DEF_THRESHOLD;
    bool keepLeading = false;
    int fitMode = OIP_FIT_REFERENCE;
    bool fp16acc = false;
    bool panOnly = false;       // stitched PAN product only: fused RRC / resampling straight into the stitched raster
    SeamOptions seamPAN, seamMSS;   // the two stitches' seam options (inactive: the hard cut of oip_stitch_rows_u16); not with panOnly
};

inline void RunFusedTask(const std::string &pan1, const std::string &pan2, const std::string &rrc1, const std::string &rrc2,
                         const std::string &mss1, const std::string &mss2, const std::string rrcMss1[MSS_BANDS],
                         const std::string rrcMss2[MSS_BANDS], const std::string &outPAN, const std::string &outMSS,
                         const TaskOptions &o)
{
    oip_ctx *ctx = Device::get().ctx();
    auto ck = [](int rc) { Device::get().check(rc); };
    stop_watch total;
    const int W = o.width;
    // ---- step 1: prestitch.  Sizes and checks as Stitcher's constructor (stitcher.h:49-81)
    const size_t s1 = IMO::FileSize(pan1), s2 = IMO::FileSize(pan2);
    if ((size_t)o.sections * o.sectionLines * BYTES_PER_PIXEL > s1) throw std::invalid_argument("PAN1 size too small for SECTION & LINE_PER_SECTION argument");
    if (s1 != s2) throw std::invalid_argument("PAN1 size doesn't match PAN2 size");
    const long L = (long)(s1 / ((size_t)W * BYTES_PER_PIXEL));
    if (L < (long)o.sections * o.sectionLines)
        throw std::invalid_argument("PAN line count less than sections times line-per-section, use smaller -s and/or -l value(s)");
    const size_t npx = (size_t)W * L;
    DevBuf<uint16_t> p1(npx), p2(npx), p2s;
    p1.load_file(pan1, npx);
    p2.load_file(pan2, npx);
    // CalcSttParameters on the raw strips (App. B-1), same filter and mean as stitcher.h:181-198
    std::vector<double> r(3 * (size_t)o.sections);
    ck(oip_stt_correlate(ctx, p1.p, p2.p, W, L, 0, L, o.sections, o.sectionLines, o.overlapCols, o.edgeCols, r.data()));
    double dx = 0, dy = 0, resp = 0;
    int valid = 0;
    if (oip_stt_mean(r.data(), o.sections, o.sttThreshold, o.sttMaxDeltaY, &dx, &dy, &resp, &valid) != OIP_OK)
        throw std::runtime_error("No valid delta value found for stitching parameter calculating");
    OLOG("Total %d valid delta value pairs found, everage value:", valid);
    OLOG("    dx: %.5f, dy: %.5f, r: %.5f", dx, dy, resp);
    if (o.panOnly) {
        // stitched PAN alone: no corrected strip is needed afterwards, so the left half of every stitched line is the RRC of
        // the raw CCD-1 line (oip_rrc_u16_window) and the right half the resampled CCD-2 line, corrected on load
        // (oip_remap_shift_rrc_bicubic_u16_window): neither .RRC.RAW nor .RRC.PRESTT.RAW is materialised.  Same bits as the flow below.
        const int fold = o.foldColsPAN / 2;
        if (fold < 0 || fold >= W) throw std::invalid_argument("fold columns exceed the image width");
        const long ow = 2L * (W - fold);
        const size_t nout = (size_t)ow * L;
        DevBuf<uint16_t> st(nout);
        DevBuf<double> kb((size_t)W * 2);
        std::vector<double> prm = IMO::LoadLut(rrc1, W);
        kb.upload(prm.data(), prm.size());
        ck(oip_rrc_u16_window(ctx, p1.p, W, st.p, ow, W - fold, L, kb.p));
        ck(oip_sync(ctx));
        p1.release();
        prm = IMO::LoadLut(rrc2, W);
        kb.upload(prm.data(), prm.size());
        // the raw CCD-2 samples are corrected on load by the resampling kernel itself (either accumulate mode): one pass over the strip
        ck(oip_remap_shift_rrc_bicubic_u16_window(ctx, p2.p, 0, L, kb.p, st.p, ow, fold, W - fold, 0, L, W, L, dx, dy, OIP_REMAP_SECTION_ROWS,
                                                  OIP_REMAP_ROW_GUARD, o.fp16acc ? 1 : 0));
        OLOG("Write stitched image to file '%s' ...", outPAN.c_str());
        write_tiff_from_device(outPAN, st.p, (int)ow, L, 1, tiff_compression(TIFF_NONE), false);
        OLOG("Fused task (PAN only) done in %.3f seconds.", total.tick());
        return;
    }
    JobThread panWriter;                       // (declared before the buffers its job shares)
    // DoRRC (both strips, in place) + PreStitch of PAN2
    {
        DevBuf<double> kb((size_t)W * 2);
        for (int c = 0; c < 2; ++c) {
            const std::vector<double> prm = IMO::LoadLut(c ? rrc2 : rrc1, W);
            kb.upload(prm.data(), prm.size());
            ck(oip_rrc_u16(ctx, c ? p2.p : p1.p, c ? p2.p : p1.p, W, L, kb.p));
            ck(oip_sync(ctx));
        }
    }
    p2s.alloc(npx);
    ck((o.fp16acc ? oip_remap_shift_bicubic_u16_f16acc : oip_remap_shift_bicubic_u16)(ctx, p2.p, 0, L, p2s.p, 0, L, W, L, dx, dy,
                                                                                     OIP_REMAP_SECTION_ROWS, OIP_REMAP_ROW_GUARD));
    p2.release();
    // ---- step 2: stitched PAN product
    {
        const int fold = o.foldColsPAN / 2;
        if (fold < 0 || fold >= W) throw std::invalid_argument("fold columns exceed the image width");
        const size_t nout = (size_t)2 * (W - fold) * L;
        auto st = std::make_shared<DevBuf<uint16_t>>(nout);
        if (o.seamPAN.active()) StitchSeam(p1.p, p2s.p, st->p, W, L, fold, 1, o.seamPAN);
        else ck(oip_stitch_rows_u16(ctx, p1.p, p2s.p, st->p, W, L, fold));
        long mark = 0;
        ck(oip_compute_mark(ctx, &mark));
        OLOG("Write stitched image to file '%s' ...", outPAN.c_str());
        // the largest product of the task (4 (W - fold) L bytes) goes out on a writer thread, behind the mark of the stitch
        // kernel, while the two default actions below run: a new file takes ~6 GB/s whatever else the process does
        const int comp = tiff_compression(TIFF_NONE);
        panWriter.post([=] { write_tiff_from_device(outPAN, st->p, 2 * (W - fold), L, 1, comp, false, nullptr, mark); });
    }
    // ---- step 3: inter-band alignment per CCD, PAN taken from the device
    DevBuf<uint16_t> aligned[2];
    long arows[2] = {0, 0};
    for (int c = 0; c < 2; ++c) {
        PreProcessor pp(c ? pan2 : pan1, c ? mss2 : mss1, "", c ? rrcMss2 : rrcMss1, W);
        pp.UseDevicePAN(c ? p2s.p : p1.p);
        pp.SetFitMode(o.fitMode);
        pp.LoadMSS();
        pp.DoRRC4MSS(true);
        pp.CalcInterBandCorrelation(o.slices, o.ibcSections, o.ibcThreshold, false);
        pp.DoInterBandAlignment(o.linesSection, o.lineOffset, o.overlapLines, o.keepLeading, true, &aligned[c], &arows[c]);
        (c ? p2s : p1).release();
    }
    // ---- step 4: stitched MSS product (imageop.h:365-457 / :460-567 on the aligned 16UC4 images)
    {
        if (arows[0] != arows[1]) throw std::runtime_error("images have different sizes");
        const int Wb = W / MSS_BANDS, fold = o.foldColsMSS / 2;
        if (fold < 0 || fold >= Wb) throw std::invalid_argument("fold columns exceed the image width");
        const int W4 = Wb * MSS_BANDS, fold4 = fold * MSS_BANDS;
        const size_t nout = (size_t)2 * (W4 - fold4) * arows[0];
        DevBuf<uint16_t> st(nout);
        // (the fit is per channel: the order the aligned images hold their samples in, the Mat's here and the file's in `oip stitch`,
        // does not change what a channel gets)
        if (o.seamMSS.active()) StitchSeam(aligned[0].p, aligned[1].p, st.p, W4, arows[0], fold4, MSS_BANDS, o.seamMSS);
        else ck(oip_stitch_rows_u16(ctx, aligned[0].p, aligned[1].p, st.p, W4, arows[0], fold4));
        OLOG("Write stitched image to file '%s' ...", outMSS.c_str());
        const int ow = 2 * (Wb - fold);
        if (!o.useGDAL && nout < 4000000000ull) {
            write_tiff_from_device(outMSS, st.p, ow, arows[0], MSS_BANDS, tiff_compression(TIFF_LZW), true);     // as cv::imwrite of the stitched Mat
        } else {
            int order[4];
            for (int b = 0; b < 4; ++b) order[b] = o.bandMap ? o.bandMap[b] - 1 : b;  // band b <- Mat channel map[b]-1
            write_tiff_from_device(outMSS, st.p, ow, arows[0], MSS_BANDS, tiff_compression(TIFF_LZW), false, order);
        }
    }
    panWriter.finish();
    OLOG("Fused task done in %.3f seconds.", total.tick());
}

}  // namespace OIPGPU
