// oip_rastertools.hpp -- the raster tools that are not in the reference (rrc-calib, quicklook, mtfc, despike, denoise, noise, mask, wallis, mtf,
// overviews, cog, rescale, regcheck, regfix, pansharpen) above the host layer of oip_host.hpp.  Stated once for all of them: the file checks made before a
// device is touched (container, RAW size rule, line range, GuardOutput), the loaders of a resident image, the driver that streams
// a RAW strip through the device in line blocks (geometry: oip_stripplan.hpp), the filter driver above it, the closing
// throughput line and the text-report writer.  Then the tools, each as Options / Check / Run.  The ranges of option values are
// refused by the tool's run_* in oip_main.cpp (exit 104-109); a *Check holds what needs the container, a file or a combination
// with the image (exit 2 or 254), and the few option checks of the older tools that run_* does not make (quicklook's --factor
// and --bands, a --width nothing else tests).  No condition is stated in both.
#pragma once

#include "oip_host.hpp"
#include "oip_maskreport.hpp"
#include "oip_mtfreport.hpp"
#include "oip_noisereport.hpp"
#include "oip_regreport.hpp"
#include "oip_rescaleplan.h"
#include "oip_wallisreport.hpp"
#include "oip_stripplan.hpp"
#include "oip_warpfield.hpp"

namespace OIPGPU {

// ---- what the tools refuse without a device ---------------------------------------------------------------------
// the container of an image by its extension: ".raw" or ".tiff"
inline std::string RasterContainer(const std::string &file, const char *tool)
{
    const std::string ext = to_lower(std::filesystem::path(file).extension().string());
    if (ext != ".tiff" && ext != ".raw") throw std::invalid_argument(std::string(tool) + ": only RAW and TIFF image supported");
    return ext;
}

// the lines of a RAW file of lineBytes per line; CheckFilesAttributes' size rule (preproc.h:552-572)
inline long RawLineCount(const std::string &file, const char *what, size_t lineBytes)
{
    const size_t size = IMO::FileSize(file);
    if (size == 0 || size % lineBytes != 0)
        throw std::invalid_argument(std::string(what) + " file size invalid: should be multiplies of " + std::to_string(lineBytes));
    return (long)(size / lineBytes);
}

// the lines [first, first + count) of the `total` lines of `what` that --line-offset / --lines (0: to the end) select
inline void LineRange(const std::string &what, long total, long lineOffset, long lines, long *first, long *count)
{
    if (lineOffset >= total) throw std::invalid_argument(what + " has " + std::to_string(total) + " lines: --line-offset is beyond them");
    *first = lineOffset;
    *count = lines > 0 ? std::min(lines, total - lineOffset) : total - lineOffset;
}

// ... of a RAW file of `width` samples per line; returns the file's lines
inline long RawLineRange(const std::string &file, const char *what, int width, long lineOffset, long lines, long *first, long *count)
{
    const long total = RawLineCount(file, what, (size_t)width * BYTES_PER_PIXEL);
    LineRange(std::string(what) + " file", total, lineOffset, lines, first, count);
    return total;
}

// the output rule of every tool that reads an image and writes one file for it (all but rrc-calib, whose coefficient files
// have RrcCalibCheck's): `path` is none of the input files, and an existing file only with --force
inline void GuardOutput(const std::string &path, const std::vector<std::string> &inputs, const char *tool, bool force)
{
    struct stat st;
    if (stat(path.c_str(), &st) != 0) return;
    for (const std::string &in : inputs)
        if (std::filesystem::equivalent(path, in))
            throw std::invalid_argument("output file [" + path + "] is " + (inputs.size() == 1 ? "the input image" : "an input image"));
    if (!force) throw std::runtime_error("output file [" + path + "] exists: " + tool + " does not replace a file without --force");
}

// the product of a filter (mtfc, despike, denoise, regfix): <stem><suffix><ext> unless named, in the container `ext` of the input
inline std::string FilterOutputPath(const std::string &file, const std::string &out, const char *suffix, const std::string &ext, const char *tool, bool force)
{
    const std::string path = out.empty() ? IMO::BuildOutputFilePath(file, suffix) : out;
    if (to_lower(std::filesystem::path(path).extension().string()) != ext)
        throw std::invalid_argument(std::string(tool) + ": the output has the container of the input (" + ext + ")");
    GuardOutput(path, {file}, tool, force);
    return path;
}

// OIP_<TOOL>_BLOCK_LINES of mtfc, despike, denoise, noise, mask, wallis, mtf, overviews and regfix (test hooks: several blocks on a small image), rounded
// down to the multiple q of lines the tool needs and never below q; 0 without one
inline long BlockLinesHook(const char *name, long q = 1)
{
    const char *e = getenv(name);
    const long v = e ? atol(e) : 0;
    return v > 0 ? std::max(q, v / q * q) : 0;
}

// the closing line of a tool
inline void LogThroughput(size_t bytes, double seconds) { OLOG("%zu bytes in %.3f seconds (%.1f MBps).", bytes, seconds, bytes / seconds / 1024.0 / 1024.0); }

// a text report: write(FILE *) returns whether every line went out; a failed open, write or close is an error
template <class Write> inline void WriteTextFile(const std::string &path, Write write)
{
    FILE *f = fopen(path.c_str(), "w");
    if (!f) throw std::runtime_error("open file [" + path + "] failed: " + std::to_string(errno));
    const bool ok = write(f);
    if (fclose(f) != 0 || !ok) throw std::runtime_error("write file [" + path + "] failed");
}

// ---- resident images --------------------------------------------------------------------------------------------
struct ResidentImage {
    DevBuf<uint16_t> buf;
    int w = 0, spp = 1;
    long h = 0;
    size_t bytes() const { return (size_t)w * h * spp * BYTES_PER_PIXEL; }
};

// a TIFF product of 1 or 4 samples per pixel, read to the device
inline void LoadTiffProduct(const std::string &file, const char *tool, ResidentImage *m)
{
    OLOG("Reading image from file `%s' ...", file.c_str());
    read_tiff_to_device(file, &m->w, &m->h, &m->spp, m->buf);
    if (m->spp != 1 && m->spp != MSS_BANDS) throw std::invalid_argument(std::string(tool) + ": a TIFF of 1 or 4 samples per pixel expected");
}

// ... or a whole single-band RAW strip of rawWidth samples per line, which `what` names in the size rule
inline void LoadResident(const std::string &file, bool isTiff, int rawWidth, const char *what, const char *tool, ResidentImage *m)
{
    if (isTiff) return LoadTiffProduct(file, tool, m);
    m->w = rawWidth;
    m->spp = 1;
    m->h = RawLineCount(file, what, (size_t)rawWidth * BYTES_PER_PIXEL);
    m->buf.alloc((size_t)m->w * m->h);
    m->buf.load_file(file, (size_t)m->w * m->h);
}

// ---- the strip-streaming driver ---------------------------------------------------------------------------------
// A RAW strip is never resident.  The line blocks of `plan` go file -> pinned ring -> one of two device blocks; work(src,
// srcFirst, srcLines, dst, dstFirst, dstLines) of a block runs behind its upload (ticket) while the host reads the next
// block from the file into the pinned ring.  With an output (outPath != NULL) the block's dstLines lines go from one of two
// further device blocks to their byte offset in the product on a writer thread behind a compute mark: read || kernel ||
// write.  Without one, dst is NULL and nothing is written.
template <class Work> inline void StreamStrip(const std::string &file, const StripPlan &plan, const std::string *outPath, Work work)
{
    oip_ctx *ctx = Device::get().ctx();
    auto ck = [](int rc) { Device::get().check(rc); };
    DevBuf<uint16_t> in[2], res[2];
    for (int i = 0; i < (plan.secondSlot() ? 2 : 1); ++i) {
        in[i].alloc((size_t)plan.inLines() * plan.lineBytes / BYTES_PER_PIXEL);
        if (outPath) res[i].alloc((size_t)plan.outLines() * plan.lineBytes / BYTES_PER_PIXEL);
    }
    if (outPath) { FILE *f = fopen(outPath->c_str(), "wb"); if (!f) throw std::runtime_error("open file [" + *outPath + "] failed: " + std::to_string(errno)); fclose(f); }
    OLOG("Reading raw image from file `%s' ...", file.c_str());
    std::future<void> written[2];
    std::unique_ptr<JobThread> writer(outPath ? new JobThread : nullptr);      // (declared after the buffers: joined before they are released)
    for (long i = 0; i < plan.blocks(); ++i) {
        const StripBlock b = plan.block(i);
        uint16_t *d = in[b.slot].p, *q = res[b.slot].p;
        // uploads do not wait for the compute stream: the kernel that read this buffer two blocks ago goes first (the call orders
        // the upload behind the previous block's kernel as well -- a kernel is ~1 % of a block's transfer time)
        if (i >= 2) ck(oip_stage_order_after_compute(ctx));
        size_t got = 0;
        long ticket = 0;
        ck(oip_read_file_to_device(ctx, file.c_str(), b.srcOffset, b.srcBytes, d, &got, &ticket));
        if (got != b.srcBytes)
            throw std::runtime_error("file size(" + std::to_string(b.srcOffset + b.srcBytes) + ") doesn't match with read byte count(" +
                                     std::to_string(b.srcOffset + got) + ")");
        ck(oip_stage_wait(ctx, ticket));
        if (written[b.slot].valid()) {                                  // the output block of two blocks ago is in the file
            try { written[b.slot].get(); } catch (const std::future_error &) { writer->finish(); throw; }      // (a failed writer drops its jobs)
        }
        work(d, b.srcFirst, b.srcLines, q, b.dstFirst, b.dstLines);
        if (!outPath) continue;
        long mark = 0;
        ck(oip_compute_mark(ctx, &mark));
        auto done = std::make_shared<std::promise<void>>();
        written[b.slot] = done->get_future();
        writer->post([=] {                                              // (outPath is the caller's: it outlives the writer, joined in here)
            const int rc = oip_write_device_to_file_at(ctx, q, b.dstBytes, outPath->c_str(), b.dstOffset, mark);
            done->set_value();                                          // the buffer is free either way; finish() reports a failure
            Device::get().check(rc);
        });
    }
    if (writer) writer->finish();
}

// read only: work(src, firstLineInRange, lines)
template <class Work> inline void ReadStrip(const std::string &file, const StripPlan &plan, Work work)
{
    StreamStrip(file, plan, nullptr, [&](const uint16_t *src, long s0, long lines, uint16_t *, long, long) { work(src, s0 - plan.first, lines); });
}

// The filters (mtfc, despike, denoise, regfix) write an image of the size and container of their input through one
// work(src, srcFirst, srcLines, dst, dstFirst, dstLines, w, L, spp), the argument order of their kernels.  A TIFF product is
// resident: one call over the whole image, which leaves through the product writer of `oip stitch` (`word` is the tool's for
// what it writes).  A RAW strip of rawWidth samples per line streams through StreamStrip with `halo` lines either side of a
// block, one call per block with spp == 1; `hook` is the tool's OIP_*_BLOCK_LINES.  Returns the bytes of the image.
template <class Work>
inline size_t FilterImage(const std::string &file, const std::string &outPath, bool isTiff, int rawWidth, long halo, const char *hook, const char *tool,
                          const char *word, Work work)
{
    if (isTiff) {
        ResidentImage m;
        LoadTiffProduct(file, tool, &m);
        DevBuf<uint16_t> res((size_t)m.w * m.h * m.spp);
        work(m.buf.p, 0, m.h, res.p, 0, m.h, m.w, m.h, m.spp);
        OLOG("Write %s image to file '%s' ...", word, outPath.c_str());
        write_tiff_from_device(outPath, res.p, m.w, m.h, m.spp, tiff_compression(m.spp == 1 ? TIFF_NONE : TIFF_LZW), false);
        return m.bytes();
    }
    const size_t lineBytes = (size_t)rawWidth * BYTES_PER_PIXEL;
    const long L = RawLineCount(file, "image", lineBytes);
    StreamStrip(file, StripPlan{0, L, L, halo, StripBlockLines(lineBytes, 1, BlockLinesHook(hook)), lineBytes}, &outPath,
                [&](const uint16_t *d, long s0, long sn, uint16_t *q, long r, long m) { work(d, s0, sn, q, r, m, rawWidth, L, 1); });
    return (size_t)L * lineBytes;
}

// ---- oip rrc-calib: the coefficient files every other action consumes --------------------------------
// One read-only pass over a strip accumulates every column's count, sum and sum of squares (oip_colstats_u16); moment
// matching on those totals (oip_rrc_fit_columns) gives each column the (k, b) that brings its statistics to the sensor-wide
// ones, written in the format IMO::LoadRRCParamFile reads (imageop.h:140-192).  Not in the reference, which only consumes
// such files.
struct RrcCalibOptions {
    int width = OIP_PIXELS_PER_LINE;
    int mode = OIP_RRCFIT_MOMENTS;
    int validMin = 0, validMax = 65535;
    long minCount = 0;
    long lineOffset = 0, lines = 0;         // lines == 0: to the end of the file
    bool force = false;
    std::string badPan, badMss;             // --bad-pan / --bad-mss: the columns the fit refuses, as `oip despike --bad-columns` reads them
};

// The statistics kernel runs per line block of the strip (ReadStrip).  `groups` equal column groups.  Returns the fitted W
// (k, b) pairs, and in `deadCols` (may be NULL) the columns the fit refused; nothing is written here.
inline std::vector<double> RrcCalibImage(const std::string &file, const char *what, int groups, const RrcCalibOptions &o, std::vector<int> *deadCols = nullptr)
{
    const int W = o.width, gw = W / groups;
    long first = 0, nLines = 0;
    const long L = RawLineRange(file, what, W, o.lineOffset, o.lines, &first, &nLines);
    oip_ctx *ctx = Device::get().ctx();
    auto ck = [](int rc) { Device::get().check(rc); };
    const size_t lineBytes = (size_t)W * BYTES_PER_PIXEL;
    DevBuf<uint64_t> acc((size_t)3 * W);
    ck(oip_memset(ctx, acc.p, 0, (size_t)3 * W * sizeof(uint64_t)));
    stop_watch sw;
    ReadStrip(file, StripPlan{first, nLines, L, 0, StripBlockLines(lineBytes), lineBytes},
              [&](const uint16_t *d, long, long m) { ck(oip_colstats_u16(ctx, d, W, W, m, o.validMin, o.validMax, acc.p)); });
    std::vector<uint64_t> totals((size_t)3 * W);
    acc.download(totals.data(), totals.size());
    LogThroughput((size_t)nLines * lineBytes, sw.tick());

    std::vector<double> kb((size_t)2 * W), ref((size_t)2 * groups);
    std::vector<int> dead(groups);
    char err[1024] = "";
    const int rc = oip_rrc_fit_columns(totals.data(), W, groups, o.mode, (uint64_t)o.minCount, kb.data(), dead.data(), ref.data(), err, sizeof err);
    if (rc == OIP_E_INVALID) throw std::invalid_argument(err);
    if (rc != OIP_OK) throw std::runtime_error(err);
    for (int g = 0; g < groups; ++g) {
        double kmin = INFINITY, kmax = -INFINITY, bmin = INFINITY, bmax = -INFINITY;
        for (int i = 0; i < gw; ++i) {
            const double k = kb[2 * ((size_t)g * gw + i)], b = kb[2 * ((size_t)g * gw + i) + 1];
            kmin = std::min(kmin, k); kmax = std::max(kmax, k); bmin = std::min(bmin, b); bmax = std::max(bmax, b);
        }
        OLOG("%s%s: %ld lines, %d usable / %d dead columns, mu_ref %.6f, sigma_ref %.6f, k in [%.9f, %.9f], b in [%.6f, %.6f]", what,
             groups > 1 ? (" band " + std::to_string(g + 1)).c_str() : "", nLines, gw - dead[g], dead[g], ref[2 * g], ref[2 * g + 1], kmin, kmax, bmin,
             bmax);
    }
    if (deadCols) {
        deadCols->resize(W);
        int n = 0;
        if (oip_rrc_dead_columns(totals.data(), W, o.mode, (uint64_t)o.minCount, deadCols->data(), &n) != OIP_OK) throw std::invalid_argument("oip_rrc_dead_columns: bad argument");
        deadCols->resize(n);
    }
    return kb;
}

// what is refused without a device, all of it stated here alone: --width (a multiple of 4 for MSS), the file sizes, the line
// range, outputs named twice, outputs that exist
inline void RrcCalibCheck(const std::string &pan, const std::string &mss, const std::string &outPan, const std::string *outMss, const RrcCalibOptions &o)
{
    long a = 0, b = 0;
    if (o.width <= 0 || (!mss.empty() && o.width % MSS_BANDS != 0)) throw std::invalid_argument("--width: a positive line width (a multiple of 4 for MSS) expected");
    if (!pan.empty()) RawLineRange(pan, "PAN", o.width, o.lineOffset, o.lines, &a, &b);
    if (!mss.empty()) RawLineRange(mss, "MSS", o.width, o.lineOffset, o.lines, &a, &b);
    std::vector<std::string> outs;
    if (!pan.empty()) outs.push_back(outPan);
    for (int i = 0; i < MSS_BANDS && !mss.empty(); ++i) outs.push_back(outMss[i]);
    if (!o.badPan.empty()) outs.push_back(o.badPan);
    if (!o.badMss.empty()) outs.push_back(o.badMss);
    for (size_t i = 0; i < outs.size(); ++i)
        for (size_t j = i + 1; j < outs.size(); ++j)
            if (outs[i] == outs[j] || (std::filesystem::exists(outs[i]) && std::filesystem::exists(outs[j]) && std::filesystem::equivalent(outs[i], outs[j])))
                throw std::invalid_argument("output file [" + outs[i] + "] is named for two outputs");
    struct stat st;
    for (const auto &f : outs)
        if (!o.force && stat(f.c_str(), &st) == 0)
            throw std::runtime_error("output file [" + f + "] exists: calibration does not replace a coefficient file without --force");
}

inline void RunRrcCalib(const std::string &pan, const std::string &mss, const std::string &outPan, const std::string *outMss, const RrcCalibOptions &o)
{
    RrcCalibCheck(pan, mss, outPan, outMss, o);
    // every image and group is fitted before the first file is written: a band without a usable column leaves no partial set
    std::vector<double> kbPan, kbMss;
    std::vector<int> deadPan, deadMss;
    if (!pan.empty()) kbPan = RrcCalibImage(pan, "PAN", 1, o, o.badPan.empty() ? nullptr : &deadPan);
    if (!mss.empty()) kbMss = RrcCalibImage(mss, "MSS", MSS_BANDS, o, o.badMss.empty() ? nullptr : &deadMss);
    auto write = [](const std::string &path, const double *kb, int n) {
        char err[1024] = "";
        if (oip_write_rrc_param_file(path.c_str(), kb, n, err, sizeof err) != OIP_OK) throw errno_error(err, 0);
        OLOG("RRC parameters written to file [%s].", path.c_str());
    };
    if (!pan.empty()) write(outPan, kbPan.data(), o.width);
    const int bw = o.width / MSS_BANDS;
    for (int b = 0; b < MSS_BANDS && !mss.empty(); ++b) write(outMss[b], &kbMss[2 * (size_t)b * bw], bw);
    // the columns the fit refused, behind the coefficient files: the list `oip despike --bad-columns` reads
    auto writeList = [&](const std::string &path, const std::vector<int> &cols, const std::string &image) {
        char err[1024] = "";
        const std::string comment = "columns of " + image + " (" + std::to_string(o.width) + " samples per line) without usable statistics: oip rrc-calib --mode " +
                                    (o.mode == OIP_RRCFIT_MOMENTS ? "moments" : "gain");
        if (oip_write_column_list(path.c_str(), cols.data(), (int)cols.size(), comment.c_str(), err, sizeof err) != OIP_OK) throw errno_error(err, 0);
        OLOG("%zu bad columns written to file [%s].", cols.size(), path.c_str());
    };
    if (!o.badPan.empty()) writeList(o.badPan, deadPan, pan);
    if (!o.badMss.empty()) writeList(o.badMss, deadMss, mss);
}

// ---- oip quicklook: an 8-bit browse image of a strip or product ---------------------------------------------
// The products are too large to look at (a stitched PAN strip is ~4.8 GB of 12-bit values in 16-bit samples): one read-only
// pass box-decimates the image by F x F (oip_decimate_box_u16), and everything behind it works on planes F^2 times smaller --
// per band a histogram (oip_histogram_u16), percentile limits and an 8-bit table on the host (oip_stretch_limits,
// oip_stretch_lut_u8), one look-up kernel (oip_apply_lut_u8) and an uncompressed 8-bit TIFF -- or, with --format jpeg, a JFIF
// file whose scan is encoded where the 8-bit image lies (oip_jpeg_scan_u8): only the payload and the interval table come back
// to the host.  Not in the reference.
struct QuicklookOptions {
    int width = OIP_PIXELS_PER_LINE;        // RAW input: samples per line
    bool bil = false;                       // RAW input: the MSS line layout, 4 bands of width / 4 next to each other
    int factor = OIP_QUICKLOOK_DEF_FACTOR;
    double clipLow = OIP_QUICKLOOK_DEF_CLIPLOW, clipHigh = OIP_QUICKLOOK_DEF_CLIPHIGH;
    int validMin = 1, validMax = 65535;     // 0 is the border value of prestitch and the aligner (BORDER_CONSTANT)
    std::vector<int> bands;                 // 1-based; empty: 1 for one band, 1,2,3 for four
    long lineOffset = 0, lines = 0;         // lines == 0: to the end of the image
    bool force = false;
    bool jpeg = false;                      // --format jpeg: <stem>.QL.JPG instead of <stem>.QL.TIFF
    int quality = OIP_JPEG_DEF_QUALITY;
};

// what is refused without a device and stated here alone: --factor and --bands, --width with --bil, the output; returns the
// output path and whether the input is a TIFF
inline std::string QuicklookCheck(const std::string &file, const std::string &out, const QuicklookOptions &o, bool *isTiff)
{
    *isTiff = RasterContainer(file, "quicklook") == ".tiff";
    const int F = o.factor;
    if (F != 2 && F != 4 && F != 8 && F != 16 && F != 32 && F != 64) throw usage_error("--factor: one of 2, 4, 8, 16, 32, 64 expected");
    if (o.bands.size() > 3 || o.bands.size() == 2) throw usage_error("--bands: one band (grey) or three (RGB) expected");
    if (!*isTiff) {
        const int nb = o.bil ? MSS_BANDS : 1;
        for (int b : o.bands)
            if (b < 1 || b > nb) throw usage_error("--bands: band index out of range (1.." + std::to_string(nb) + ")");
        if (o.width <= 0 || (o.bil && o.width % MSS_BANDS != 0)) throw std::invalid_argument("--width: a positive line width (a multiple of 4 with --bil) expected");
    } else {
        for (int b : o.bands)
            if (b < 1 || b > MSS_BANDS) throw usage_error("--bands: band index out of range (1.." + std::to_string(MSS_BANDS) + ")");
    }
    // (not FilterOutputPath: a quick look is a .TIFF -- a .JPG with --format jpeg -- whatever the input is, and may be named like
    // anything: the name's extension is not inspected)
    const std::string path = out.empty() ? IMO::BuildOutputFilePath(file, OIP_QUICKLOOK_SUFFIX, o.jpeg ? ".JPG" : ".TIFF") : out;
    GuardOutput(path, {file}, "quicklook", o.force);
    return path;
}

inline void RunQuicklook(const std::string &file, const std::string &out, const QuicklookOptions &o)
{
    bool isTiff = false;
    const std::string outPath = QuicklookCheck(file, out, o, &isTiff);
    const int F = o.factor;
    long first = 0, nLines = 0, fileLines = 0;
    int bw = 0, nb = 0;                     // band width in pixels, bands of the image
    if (!isTiff) {
        fileLines = RawLineRange(file, "image", o.width, o.lineOffset, o.lines, &first, &nLines);
        nb = o.bil ? MSS_BANDS : 1;
        bw = o.width / nb;
    }
    oip_ctx *ctx = Device::get().ctx();
    auto ck = [](int rc) { Device::get().check(rc); };
    stop_watch total;
    size_t inBytes = 0;
    DevBuf<uint16_t> planes;
    int ow = 0;
    long oh = 0;
    size_t plane = 0;
    auto alloc_planes = [&]() {
        ow = (bw + F - 1) / F;
        oh = (nLines + F - 1) / F;
        if (o.jpeg && (ow > OIP_JPEG_MAX_DIM || oh > OIP_JPEG_MAX_DIM))
            throw std::invalid_argument("quicklook: a JPEG holds at most " + std::to_string(OIP_JPEG_MAX_DIM) + " x " + std::to_string(OIP_JPEG_MAX_DIM) +
                                        " pixels and the browse image has " + std::to_string(ow) + " x " + std::to_string(oh) + ": use a larger --factor");
        plane = (size_t)ow * oh;
        planes.alloc(plane * nb);
    };
    if (isTiff) {
        ResidentImage m;
        LoadTiffProduct(file, "quicklook", &m);
        LineRange("image", m.h, o.lineOffset, o.lines, &first, &nLines);
        nb = m.spp;
        bw = m.w;
        for (int b : o.bands)
            if (b > nb) throw usage_error("--bands: band index out of range (1.." + std::to_string(nb) + ")");
        alloc_planes();
        ck(oip_decimate_box_u16(ctx, m.buf.p + (size_t)first * m.w * m.spp, (long)m.w * m.spp, m.w, nLines, m.spp, F, planes.p, ow, plane));
        ck(oip_sync(ctx));                  // the image is released at the end of this block
        inBytes = (size_t)nLines * m.w * m.spp * BYTES_PER_PIXEL;
    } else {
        // the decimation runs per line block of the strip (ReadStrip), a block being a multiple of F lines
        const size_t lineBytes = (size_t)o.width * BYTES_PER_PIXEL;
        alloc_planes();
        ReadStrip(file, StripPlan{first, nLines, fileLines, 0, StripBlockLines(lineBytes, F), lineBytes}, [&](const uint16_t *d, long r, long m) {
            for (int b = 0; b < nb; ++b)    // a BIL band is a window of the line
                ck(oip_decimate_box_u16(ctx, d + (size_t)b * bw, o.width, bw, m, 1, F, planes.p + (size_t)b * plane + (size_t)(r / F) * ow, ow, 0));
        });
        ck(oip_sync(ctx));
        inBytes = (size_t)nLines * lineBytes;
    }
    std::vector<int> bands = o.bands;
    if (bands.empty()) bands = nb == 1 ? std::vector<int>{1} : std::vector<int>{1, 2, 3};
    const int nch = (int)bands.size();

    // per band: histogram of the decimated plane -> limits -> table
    DevBuf<uint64_t> hist(65536);
    DevBuf<uint8_t> luts((size_t)nch * 65536);
    std::vector<uint64_t> h(65536);
    std::vector<uint8_t> lut((size_t)nch * 65536);
    const uint16_t *chan[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < nch; ++i) {
        chan[i] = planes.p + (size_t)(bands[i] - 1) * plane;
        ck(oip_memset(ctx, hist.p, 0, 65536 * sizeof(uint64_t)));
        ck(oip_histogram_u16(ctx, chan[i], ow, ow, oh, hist.p));
        hist.download(h.data(), h.size());
        int lo = 0, hi = 0;
        uint64_t nValid = 0;
        if (oip_stretch_limits(h.data(), o.validMin, o.validMax, o.clipLow, o.clipHigh, &lo, &hi, &nValid) != OIP_OK ||
            oip_stretch_lut_u8(lo, hi, &lut[(size_t)i * 65536]) != OIP_OK)
            throw std::invalid_argument("quicklook: invalid stretch arguments");
        OLOG("band %d: %ld lines, %llu valid samples, stretch %d..%d", bands[i], nLines, (unsigned long long)nValid, lo, hi);
    }
    luts.upload(lut.data(), lut.size());
    DevBuf<uint8_t> img8(plane * nch);
    ck(oip_apply_lut_u8(ctx, chan, ow, ow, oh, nch, luts.p, img8.p));
    if (o.jpeg) {
        // the scan is encoded where img8 lies; the payload (the capacity is the coder's bound, the bytes written are the file's)
        // and the interval table come back
        DevBuf<uint8_t> payload(oip_jpeg_worst_bytes(ow, oh, nch));
        std::vector<uint64_t> off((size_t)(oh + 7) / 8), len(off.size());
        size_t bytes = 0;
        ck(oip_jpeg_scan_u8(ctx, img8.p, (long)ow * nch, ow, oh, nch, o.quality, payload.p, payload.n, off.data(), len.data(), &bytes, nullptr, 0));
        std::vector<uint8_t> host(bytes);
        payload.download(host.data(), host.size());
        OLOG("Write quick look (%d x %ld, %s; JPEG, quality %d) to file '%s' ...", ow, oh, nch == 1 ? "grey" : "RGB", o.quality, outPath.c_str());
        char err[1024] = "";
        if (oip_write_jpeg_u8(outPath.c_str(), host.data(), off.data(), len.data(), ow, oh, nch, o.quality, err, sizeof err) != OIP_OK) throw errno_error(err, 0);
    } else {
        std::vector<uint8_t> host(plane * nch);
        img8.download(host.data(), host.size());
        OLOG("Write quick look (%d x %ld, %s) to file '%s' ...", ow, oh, nch == 1 ? "grey" : "RGB", outPath.c_str());
        write_tiff_u8(outPath, host.data(), ow, oh, nch);
    }
    LogThroughput(inBytes, total.tick());
}

// ---- oip mtfc: MTF compensation of a strip or product ---------------------------------------------------------------
// A small fixed-point restoration filter (oip_convolve_u16) behind the radiometric correction: the taps come from a kernel
// file or from the MTF at Nyquist of the two axes (oip_mtfc_load_kernel / oip_mtfc_design3, then oip_mtfc_quantise).  The
// output has the container of the input.  Not in the reference.
struct MtfcOptions {
    int width = OIP_PIXELS_PER_LINE;        // RAW input: samples per line
    std::string kernelFile;                 // --kernel, or
    double mtfX = 0.0, mtfY = 0.0;          // --mtf-x / --mtf-y: the MTF at Nyquist across and along the lines
    double maxGain = OIP_MTFC_DEF_MAXGAIN;
    int validMin = 1;                       // 0 is the border value of prestitch and the aligner (BORDER_CONSTANT)
    bool force = false;
};

struct MtfcTaps {
    int ky = 0, kx = 0;
    int32_t t[OIP_CONVOLVE_MAX_K * OIP_CONVOLVE_MAX_K];
};

// what is refused without a device and stated here alone: the container, --width and the size of a RAW file, the taps, the
// output; returns the output path
inline std::string MtfcCheck(const std::string &file, const std::string &out, const MtfcOptions &o, bool *isTiff, MtfcTaps *taps)
{
    const std::string ext = RasterContainer(file, "mtfc");
    *isTiff = ext == ".tiff";
    if (!*isTiff) {
        if (o.width <= 0) throw std::invalid_argument("--width: a positive line width expected");
        RawLineCount(file, "image", (size_t)o.width * BYTES_PER_PIXEL);
    }
    double c[OIP_CONVOLVE_MAX_K * OIP_CONVOLVE_MAX_K];
    char err[1024] = "";
    if (!o.kernelFile.empty()) {
        const int rc = oip_mtfc_load_kernel(o.kernelFile.c_str(), c, &taps->ky, &taps->kx, err, sizeof err);
        if (rc == OIP_E_IO) throw errno_error(err, 0);
        if (rc != OIP_OK) throw std::invalid_argument(err);
    } else {
        taps->ky = taps->kx = 3;
        if (oip_mtfc_design3(o.mtfX, o.mtfY, o.maxGain, c) != OIP_OK) throw std::invalid_argument("--mtf-x/--mtf-y/--max-gain: 0 < M <= 1 and G >= 1 expected");
    }
    if (oip_mtfc_quantise(c, taps->ky, taps->kx, taps->t, err, sizeof err) != OIP_OK) throw std::invalid_argument(err);
    return FilterOutputPath(file, out, OIP_MTFC_SUFFIX, ext, "mtfc", o.force);
}

inline void RunMtfc(const std::string &file, const std::string &out, const MtfcOptions &o)
{
    bool isTiff = false;
    MtfcTaps taps;
    const std::string outPath = MtfcCheck(file, out, o, &isTiff, &taps);
    const int ky = taps.ky, kx = taps.kx;
    long absSum = 0;
    OLOG("MTFC taps (Q12, %d x %d):", ky, kx);
    for (int j = 0; j < ky; ++j) {
        std::string row;
        for (int i = 0; i < kx; ++i) {
            row += (i ? " " : "") + std::to_string(taps.t[j * kx + i]);
            absSum += std::abs((long)taps.t[j * kx + i]);
        }
        RLOG("    %s", row.c_str());
    }
    OLOG("sum |t| = %ld (gain at most %.3f), valid-min %d", absSum, absSum / 4096.0, o.validMin);
    oip_ctx *ctx = Device::get().ctx();
    auto ck = [](int rc) { Device::get().check(rc); };
    stop_watch total;
    // a block of a strip needs ky / 2 halo lines either side
    const size_t bytes = FilterImage(file, outPath, isTiff, o.width, ky / 2, "OIP_MTFC_BLOCK_LINES", "mtfc", "filtered",
                                     [&](const uint16_t *src, long s0, long sn, uint16_t *dst, long r, long m, int w, long L, int spp) {
                                         ck(oip_convolve_u16(ctx, src, s0, sn, dst, r, m, w, L, spp, taps.t, ky, kx, o.validMin));
                                     });
    LogThroughput(bytes, total.tick());
}

// ---- oip despike: repair of a raw strip ahead of RRC ------------------------------------------------------------------
// Listed bad columns are interpolated and isolated impulse pixels replaced by a conditional 3 x 3 median (oip_despike_u16)
// before RRC multiplies them and a resampling spreads them.  The list comes from `oip rrc-calib --bad-pan / --bad-mss` or
// from a --report of an earlier run.  The output has the container of the input.  Not in the reference.
struct DespikeOptions {
    int width = OIP_PIXELS_PER_LINE;        // RAW input: samples per line
    bool bil = false;                       // RAW input: the MSS line layout, 4 bands of width / 4 next to each other
    bool hasThreshold = false;              // without --threshold: column repair only (thr_abs 65535)
    int thrAbs = 65535, thrRelQ8 = 0;
    int validMin = 1;                       // 0 is what the de-framer writes for missing frames
    std::string badColumns, report;
    bool force = false;
};

struct DespikeTable {
    std::vector<int32_t> tab;               // empty: no list
    int listed = 0, longestRun = 0;
};

// what is refused without a device and stated here alone: the container and what it excludes, --width with --bil, the size of a
// RAW file, the list and its table, the output and the report; returns the output path
inline std::string DespikeCheck(const std::string &file, const std::string &out, const DespikeOptions &o, bool *isTiff, DespikeTable *table)
{
    const std::string ext = RasterContainer(file, "despike");
    *isTiff = ext == ".tiff";
    if (*isTiff) {
        if (!o.badColumns.empty() || o.bil)
            throw std::invalid_argument("despike: --bad-columns and --bil apply to a RAW strip: the columns of a TIFF product are no longer detector columns");
    } else {
        if (o.width <= 0 || (o.bil && o.width % MSS_BANDS != 0)) throw std::invalid_argument("--width: a positive line width (a multiple of 4 with --bil) expected");
        RawLineCount(file, "image", (size_t)o.width * BYTES_PER_PIXEL);
    }
    if (!o.badColumns.empty()) {
        const int W = o.width;
        std::vector<int> cols(W);
        char err[1024] = "";
        int n = 0;
        int rc = oip_load_column_list(o.badColumns.c_str(), W, cols.data(), W, &n, err, sizeof err);
        if (rc == OIP_E_IO) throw errno_error(err, 0);
        if (rc != OIP_OK) throw std::invalid_argument(err);
        table->tab.resize((size_t)2 * W);
        rc = oip_despike_column_table(cols.data(), n, W, o.bil ? MSS_BANDS : 1, table->tab.data(), &table->longestRun, err, sizeof err);
        if (rc != OIP_OK) throw std::invalid_argument(err);
        table->listed = n;
    }
    const std::string path = FilterOutputPath(file, out, OIP_DESPIKE_SUFFIX, ext, "despike", o.force);
    if (!o.report.empty()) {
        struct stat st;
        const bool exists = stat(o.report.c_str(), &st) == 0;
        const bool same = std::filesystem::absolute(o.report).lexically_normal() == std::filesystem::absolute(path).lexically_normal();
        if (same || (exists && (std::filesystem::equivalent(o.report, file) || (stat(path.c_str(), &st) == 0 && std::filesystem::equivalent(o.report, path)))))
            throw std::invalid_argument("report file [" + o.report + "] is the input image or the output");
        if (exists && !o.force) throw std::runtime_error("report file [" + o.report + "] exists: despike does not replace a file without --force");
    }
    return path;
}

inline void RunDespike(const std::string &file, const std::string &out, const DespikeOptions &o)
{
    bool isTiff = false;
    DespikeTable table;
    const std::string outPath = DespikeCheck(file, out, o, &isTiff, &table);
    if (o.hasThreshold) OLOG("despike: threshold %d + %d / 256 of the median, valid-min %d", o.thrAbs, o.thrRelQ8, o.validMin);
    else OLOG("despike: column repair only (no --threshold), valid-min %d", o.validMin);
    if (!o.badColumns.empty()) OLOG("%d bad columns listed in [%s], longest run %d", table.listed, o.badColumns.c_str(), table.longestRun);
    oip_ctx *ctx = Device::get().ctx();
    auto ck = [](int rc) { Device::get().check(rc); };
    stop_watch total;
    DevBuf<uint64_t> cnt;                                               // replacements per sample column; only a threshold replaces
    std::vector<uint64_t> counts;
    DevBuf<int32_t> tab;                                                // the column table and --bil: a RAW strip's alone (DespikeCheck)
    if (!table.tab.empty()) tab.assign(table.tab);
    // a block of a strip needs one halo line either side
    const size_t bytes = FilterImage(file, outPath, isTiff, o.width, 1, "OIP_DESPIKE_BLOCK_LINES", "despike", "repaired",
                                     [&](const uint16_t *src, long s0, long sn, uint16_t *dst, long r, long m, int w, long L, int spp) {
                                         if (o.hasThreshold && !cnt.p) {                        // the first block knows the columns
                                             counts.resize((size_t)w * spp);
                                             cnt.alloc(counts.size());
                                             ck(oip_memset(ctx, cnt.p, 0, counts.size() * sizeof(uint64_t)));
                                         }
                                         ck(oip_despike_u16(ctx, src, s0, sn, dst, r, m, w, L, spp, o.bil ? MSS_BANDS : 1, tab.p, o.thrAbs, o.thrRelQ8,
                                                            o.validMin, cnt.p));
                                     });
    if (o.hasThreshold) {
        cnt.download(counts.data(), counts.size());                     // (synchronises: the last kernel has run)
        uint64_t sum = 0;
        std::vector<size_t> hit;
        for (size_t x = 0; x < counts.size(); ++x)
            if (counts[x]) { sum += counts[x]; hit.push_back(x); }
        OLOG("%llu samples replaced in %zu of %zu columns", (unsigned long long)sum, hit.size(), counts.size());
        if (!o.report.empty()) {
            WriteTextFile(o.report, [&](FILE *f) {
                fprintf(f, "# column count: samples replaced by oip despike --threshold %d in %s\n", o.thrAbs, file.c_str());
                for (size_t x : hit) fprintf(f, "%zu %llu\n", x, (unsigned long long)counts[x]);
                return true;
            });
            OLOG("Replacement counts written to file [%s].", o.report.c_str());
        }
        std::stable_sort(hit.begin(), hit.end(), [&](size_t a, size_t b) { return counts[a] > counts[b]; });
        for (size_t i = 0; i < hit.size() && i < 10; ++i) RLOG("    column %zu: %llu", hit[i], (unsigned long long)counts[hit[i]]);
    } else if (!o.report.empty()) {
        WriteTextFile(o.report, [&](FILE *f) { return fprintf(f, "# column count: no --threshold, no sample replaced in %s\n", file.c_str()) > 0; });
    }
    LogThroughput(bytes, total.tick());
}

// `oip despike --noise REPORT [--k-sigma K]`: the two threshold parameters from the report of `oip noise`, each the maximum
// over the report's bands of oip_noise_despike_threshold.  No device is touched.
inline void DespikeNoiseThreshold(const std::string &report, double kSigma, DespikeOptions *o)
{
    std::vector<NoiseModel> models;
    std::string err;
    if (!ParseNoiseReport(report, &models, &err)) throw std::runtime_error(err);
    if (!NoiseDespikeThreshold(models, kSigma, &o->thrAbs, &o->thrRelQ8, &err)) throw std::runtime_error("noise report [" + report + "], " + err);
    o->hasThreshold = true;
    OLOG("despike: %g sigma of the noise model of [%s] (%zu band%s): threshold %d, relative %d / 256", kSigma, report.c_str(), models.size(),
         models.size() == 1 ? "" : "s", o->thrAbs, o->thrRelQ8);
}

// ---- oip denoise: the sigma filter that the noise model drives ---------------------------------------------------------------
// The acting side of `oip noise` for the noise itself (oip_sigma_filter_u16): an edge-preserving mean over the neighbours that lie
// within K sigma of a pilot estimate, sigma taken at the pilot's signal level from the report's model of the band (or one --sigma
// for every level).  It runs behind RRC / prestitch and ahead of mtfc.  The output has the container of the input.  Not in the
// reference.
struct DenoiseOptions {
    int width = OIP_PIXELS_PER_LINE;        // RAW input: samples per line
    std::string noiseReport;                // --noise, or
    double sigma = 0.0;                     // --sigma: one sigma at every level of every band
    double kSigma = 2.0;
    int radius = 2;
    int minMembers = 5;                     // 2 * radius + 1 unless given
    int validMin = 1;                       // 0 is the border value of prestitch and the aligner (BORDER_CONSTANT)
    bool force = false;
};

// thr[spp][256] of a run: from the report's models (one per sample of a pixel), or --sigma at every level; no device is touched
inline std::vector<uint16_t> DenoiseThresholds(const DenoiseOptions &o, const std::vector<NoiseModel> &models, int spp)
{
    std::vector<uint16_t> thr;
    if (o.noiseReport.empty()) {
        const double t = std::ceil(o.kSigma * o.sigma);
        thr.assign((size_t)spp * 256, (uint16_t)(t < 65535.0 ? t : 65535.0));
        return thr;
    }
    std::string err;
    if (!NoiseDenoiseTables(models, spp, o.kSigma, &thr, &err)) throw std::runtime_error("noise report [" + o.noiseReport + "] " + err);
    return thr;
}

// what is refused without a device and stated here alone: the container, --width and the size of a RAW file, the report and, for
// a RAW strip (one band), its tables, the output; returns the output path
inline std::string DenoiseCheck(const std::string &file, const std::string &out, const DenoiseOptions &o, bool *isTiff, std::vector<NoiseModel> *models)
{
    const std::string ext = RasterContainer(file, "denoise");
    *isTiff = ext == ".tiff";
    if (!*isTiff) {
        if (o.width <= 0) throw std::invalid_argument("--width: a positive line width expected");
        RawLineCount(file, "image", (size_t)o.width * BYTES_PER_PIXEL);
    }
    if (!o.noiseReport.empty()) {
        std::string err;
        if (!ParseNoiseReport(o.noiseReport, models, &err)) throw std::runtime_error(err);
    }
    if (!*isTiff) DenoiseThresholds(o, *models, 1);                      // (a TIFF's samples per pixel are known once it is read)
    return FilterOutputPath(file, out, OIP_DENOISE_SUFFIX, ext, "denoise", o.force);
}

inline void RunDenoise(const std::string &file, const std::string &out, const DenoiseOptions &o)
{
    bool isTiff = false;
    std::vector<NoiseModel> models;
    const std::string outPath = DenoiseCheck(file, out, o, &isTiff, &models);
    const int side = 2 * o.radius + 1;
    OLOG("denoise: sigma filter %d x %d, %g sigma of %s, min-members %d, valid-min %d", side, side, o.kSigma,
         o.noiseReport.empty() ? ("--sigma " + std::to_string(o.sigma)).c_str() : ("the noise model of [" + o.noiseReport + "]").c_str(), o.minMembers,
         o.validMin);
    oip_ctx *ctx = Device::get().ctx();
    auto ck = [](int rc) { Device::get().check(rc); };
    stop_watch total;
    std::vector<uint16_t> table;                                        // the first block knows the samples per pixel
    DevBuf<uint16_t> thr;
    DevBuf<uint64_t> stats(4);
    ck(oip_memset(ctx, stats.p, 0, 4 * sizeof(uint64_t)));
    // a block of a strip needs `radius` halo lines either side
    const size_t bytes = FilterImage(file, outPath, isTiff, o.width, o.radius, "OIP_DENOISE_BLOCK_LINES", "denoise", "denoised",
                                     [&](const uint16_t *src, long s0, long sn, uint16_t *dst, long r, long m, int w, long L, int spp) {
                                         if (!thr.p) {
                                             table = DenoiseThresholds(o, models, spp);          // refuses a report of another band count
                                             for (int c = 0; c < spp; ++c)
                                                 OLOG("denoise: band %d thresholds at levels 0, 64, 128, 255: %d %d %d %d", c + 1, table[c * 256],
                                                      table[c * 256 + 64], table[c * 256 + 128], table[c * 256 + 255]);
                                             thr.assign(table);
                                         }
                                         ck(oip_sigma_filter_u16(ctx, src, s0, sn, dst, r, m, w, L, spp, o.radius, thr.p, o.minMembers, o.validMin, stats.p));
                                     });
    uint64_t s[4];
    stats.download(s, 4);                                               // (synchronises: the last kernel has run)
    const uint64_t filtered = s[0] - s[1];
    OLOG("denoise: %llu samples with data, %llu filtered (mean members %.2f of %d), %.3f %% left alone, %.3f %% changed", (unsigned long long)s[0],
         (unsigned long long)filtered, filtered ? (double)s[2] / (double)filtered : 0.0, side * side, s[0] ? 100.0 * (double)s[1] / (double)s[0] : 0.0,
         s[0] ? 100.0 * (double)s[3] / (double)s[0] : 0.0);
    RLOG("    counters: valid %llu alone %llu members %llu changed %llu", (unsigned long long)s[0], (unsigned long long)s[1], (unsigned long long)s[2],
         (unsigned long long)s[3]);
    LogThroughput(bytes, total.tick());
}

// ---- oip noise: the noise-level function of a strip or product ----------------------------------------------------------
// The measuring side of despike's threshold.  One read-only pass gives every B x B block a key (oip_noise_blocks_u16: signal
// level and standard deviation, or a sentinel for a block with no data or with structure); per band the histogram of the keys
// (oip_histogram_u16), the sigma of every level (oip_noise_levels) and the fit sigma^2 = a + b mu (oip_noise_fit) follow, and
// go to <stem>.NOISE.CSV (oip_noisereport.hpp).  A RAW strip streams through in blocks of lines that are multiples of B; a TIFF
// product is resident.  Not in the reference.
struct NoiseOptions {
    int width = OIP_PIXELS_PER_LINE;        // RAW input: samples per line
    bool bil = false;                       // RAW input: the MSS line layout, 4 bands of width / 4 next to each other
    int block = 8, bits = 12;               // level_shift = bits - 8
    int validMin = 1, validMax = 65535;
    long minBlocks = 100;
    long lineOffset = 0, lines = 0;         // lines == 0: to the end of the image
    bool force = false;
    std::string params;                     // the first line of the report
};

// what is refused without a device and depends on the image (the option ranges are run_noise's): the container, --bil on a
// TIFF, --width with --bil, the size and line range of a RAW file, an image without a block, the output; returns the output path
// and whether the input is a TIFF
inline std::string NoiseCheck(const std::string &file, const std::string &out, const NoiseOptions &o, bool *isTiff)
{
    *isTiff = RasterContainer(file, "noise") == ".tiff";
    if (*isTiff) {
        if (o.bil) throw std::invalid_argument("noise: --bil applies to a RAW strip: a TIFF product holds its bands per pixel");
    } else {
        if (o.width <= 0 || (o.bil && o.width % MSS_BANDS != 0)) throw std::invalid_argument("--width: a positive line width (a multiple of 4 with --bil) expected");
        long first = 0, n = 0;
        RawLineRange(file, "image", o.width, o.lineOffset, o.lines, &first, &n);
        if (n < o.block || o.width / (o.bil ? MSS_BANDS : 1) < o.block) throw std::invalid_argument("noise: the image holds no block of " + std::to_string(o.block) + " x " + std::to_string(o.block));
    }
    const std::string path = out.empty() ? IMO::BuildOutputFilePath(file, OIP_NOISE_SUFFIX, ".CSV") : out;
    GuardOutput(path, {file}, "noise", o.force);
    return path;
}

inline void RunNoise(const std::string &file, const std::string &out, const NoiseOptions &o)
{
    bool isTiff = false;
    const std::string outPath = NoiseCheck(file, out, o, &isTiff);
    const int B = o.block, shift = o.bits - 8;
    oip_ctx *ctx = Device::get().ctx();
    auto ck = [](int rc) { Device::get().check(rc); };
    stop_watch total;
    size_t inBytes = 0;
    DevBuf<uint16_t> keys;                  // one plane of nbx x nby keys per band
    int nb = 0, nbx = 0;
    long nby = 0, first = 0, nLines = 0;
    size_t plane = 0;
    auto alloc_keys = [&](int bandWidth) {
        nbx = bandWidth / B;
        nby = nLines / B;
        if (nbx < 1 || nby < 1) throw std::invalid_argument("noise: the image holds no block of " + std::to_string(B) + " x " + std::to_string(B));
        plane = (size_t)nbx * nby;
        keys.alloc(plane * nb);
    };
    if (isTiff) {
        ResidentImage m;
        LoadTiffProduct(file, "noise", &m);
        LineRange("image", m.h, o.lineOffset, o.lines, &first, &nLines);
        nb = m.spp;
        alloc_keys(m.w);
        ck(oip_noise_blocks_u16(ctx, m.buf.p + (size_t)first * m.w * m.spp, (long)m.w * m.spp, m.w, nLines, m.spp, B, shift, o.validMin, o.validMax, keys.p,
                                nbx, plane));
        ck(oip_sync(ctx));                  // the image is released at the end of this block
        inBytes = (size_t)nLines * m.w * m.spp * BYTES_PER_PIXEL;
    } else {
        // the kernel runs per line block of the strip (ReadStrip), a block being a multiple of B lines; a BIL band is a window
        // of the line, so that no block straddles two bands
        const long fileLines = RawLineRange(file, "image", o.width, o.lineOffset, o.lines, &first, &nLines);
        const size_t lineBytes = (size_t)o.width * BYTES_PER_PIXEL;
        nb = o.bil ? MSS_BANDS : 1;
        const int bw = o.width / nb;
        alloc_keys(bw);
        ReadStrip(file, StripPlan{first, nLines, fileLines, 0, StripBlockLines(lineBytes, B, BlockLinesHook("OIP_NOISE_BLOCK_LINES", B)), lineBytes},
                  [&](const uint16_t *d, long r, long m) {
                      for (int b = 0; b < nb; ++b)
                          ck(oip_noise_blocks_u16(ctx, d + (size_t)b * bw, o.width, bw, m, 1, B, shift, o.validMin, o.validMax,
                                                  keys.p + (size_t)b * plane + (size_t)(r / B) * nbx, nbx, 0));
                  });
        ck(oip_sync(ctx));
        inBytes = (size_t)nLines * lineBytes;
    }

    // per band: histogram of the key plane -> sigma per level -> fit; every band is fitted before the report is written
    DevBuf<uint64_t> hist(65536);
    std::vector<uint64_t> h(65536);
    std::vector<NoiseBand> bands(nb);
    for (int b = 0; b < nb; ++b) {
        NoiseBand &n = bands[b];
        ck(oip_memset(ctx, hist.p, 0, 65536 * sizeof(uint64_t)));
        ck(oip_histogram_u16(ctx, keys.p + (size_t)b * plane, nbx, nbx, nby, hist.p));
        hist.download(h.data(), h.size());
        n.nodata = h[OIP_NOISE_KEY_NODATA];
        n.structured = h[OIP_NOISE_KEY_STRUCTURED];
        char err[512] = "";
        if (oip_noise_levels(h.data(), (uint64_t)o.minBlocks, n.sigma, n.blocks, &n.levels) != OIP_OK) throw std::invalid_argument("oip_noise_levels: bad argument");
        const int rc = oip_noise_fit(n.sigma, n.blocks, shift, &n.a, &n.b, &n.muRef, err, sizeof err);
        if (rc != OIP_OK)
            throw std::runtime_error("band " + std::to_string(b + 1) + ": " + err + " (" + std::to_string(n.realBlocks()) + " blocks, " + std::to_string(n.nodata) +
                                     " without data, " + std::to_string(n.structured) + " structured; --min-blocks " + std::to_string(o.minBlocks) + ")");
    }
    WriteTextFile(outPath, [&](FILE *f) { return WriteNoiseReport(f, o.params, bands, shift); });
    for (int b = 0; b < nb; ++b) OLOG("noise: %s", NoiseBandLine(b + 1, bands[b]).c_str());
    const double es = total.tick();
    OLOG("Report written to '%s'; %zu bytes in %.3f seconds (%.1f MBps).", outPath.c_str(), inBytes, es, inBytes / es / 1024.0 / 1024.0);
}

// ---- oip mask: no-data, saturation and cloud mask of a strip or product ------------------------------------------------------
// Which parts of a product are usable.  One read-only pass gives every C x C cell a flag byte (oip_mask_cells_u16: no data,
// saturated, and with 4 samples per pixel the cloud candidate of four spectral tests); an opening and a buffer on the grid of
// cells (oip_mask_morph_u8) turn the candidates into CLOUD and BUFFER.  The grid goes to <stem>.MASK.TIFF (8-bit, one sample),
// the eight counters and four shares to <stem>.MASK.CSV (oip_maskreport.hpp).  A RAW strip streams through in blocks of lines
// that are multiples of C; a TIFF product is resident.  With one sample per pixel there is no cloud stage.  Not in the reference.
struct MaskOptions {
    int width = OIP_PIXELS_PER_LINE;        // RAW input: samples per line
    int cell = 8, bits = 12;                // full_scale = 2^bits - 1
    int saturation = 0;                     // 0: full_scale
    int validMin = 1;
    int band[4] = {2, 1, 0, 3};             // 0-based channel of blue, green, red, nir: the product's R, G, B, alpha order
    int q8[4] = {77, 38, 20, 51};           // bright, white, hot, ndvi
    bool noCloud = false;
    int open = 1, buffer = 2;
    bool force = false;
    std::string report;                     // --report: the CSV; empty: <stem>.MASK.CSV
};

struct MaskPaths {
    std::string tiff, csv;
};

// what is refused without a device and depends on the image (the option ranges are run_mask's): the container, the size of a
// RAW file, the samples of a TIFF, the two outputs; returns the output paths, whether the input is a TIFF and (TIFF) its samples
inline MaskPaths MaskCheck(const std::string &file, const std::string &out, const MaskOptions &o, bool *isTiff, int *spp)
{
    *isTiff = RasterContainer(file, "mask") == ".tiff";
    *spp = 1;
    if (*isTiff) {
        int w = 0;
        long h = 0;
        read_tiff_geometry(file, &w, &h, spp);
        if (*spp != 1 && *spp != MSS_BANDS) throw std::invalid_argument("mask: a TIFF of 1 or 4 samples per pixel expected");
    } else {
        RawLineCount(file, "image", (size_t)o.width * BYTES_PER_PIXEL);
    }
    MaskPaths p;
    p.tiff = out.empty() ? IMO::BuildOutputFilePath(file, OIP_MASK_SUFFIX, ".TIFF") : out;
    p.csv = o.report.empty() ? IMO::BuildOutputFilePath(file, OIP_MASK_SUFFIX, ".CSV") : o.report;
    if (p.tiff == p.csv) throw std::invalid_argument("output file [" + p.tiff + "] is named for the mask and for the report");
    GuardOutput(p.tiff, {file}, "mask", o.force);
    GuardOutput(p.csv, {file}, "mask", o.force);
    return p;
}

inline void RunMask(const std::string &file, const std::string &out, const MaskOptions &o)
{
    bool isTiff = false;
    int spp = 1;
    const MaskPaths paths = MaskCheck(file, out, o, &isTiff, &spp);
    const int C = o.cell, full = (1 << o.bits) - 1, sat = o.saturation > 0 ? o.saturation : full;
    const bool cloud = spp == MSS_BANDS && !o.noCloud;
    if (spp != MSS_BANDS && !o.noCloud) OLOG("mask: one sample per pixel: the cloud tests need four and are skipped.");
    oip_ctx *ctx = Device::get().ctx();
    auto ck = [](int rc) { Device::get().check(rc); };
    stop_watch total;
    size_t inBytes = 0;
    DevBuf<uint8_t> flags;
    DevBuf<uint64_t> counts(8);
    ck(oip_memset(ctx, counts.p, 0, 8 * sizeof(uint64_t)));
    int gw = 0, width = 0;
    long gh = 0, height = 0;
    auto alloc_flags = [&](int w, long h) {
        width = w;
        height = h;
        if (oip_mask_grid(w, h, C, &gw, &gh) != OIP_OK || gw < 1 || gh < 1) throw std::invalid_argument("mask: the image is empty");
        flags.alloc((size_t)gw * gh);
    };
    if (isTiff) {
        ResidentImage m;
        LoadTiffProduct(file, "mask", &m);
        alloc_flags(m.w, m.h);
        ck(oip_mask_cells_u16(ctx, m.buf.p, (long)m.w * m.spp, m.w, m.h, m.spp, C, o.validMin, sat, full, o.band, o.q8[0], o.q8[1], o.q8[2], o.q8[3], flags.p,
                              gw, counts.p));
        ck(oip_sync(ctx));                  // the image is released at the end of this block
        inBytes = m.bytes();
    } else {
        // the kernel runs per line block of the strip (ReadStrip), a block being a multiple of C lines
        const size_t lineBytes = (size_t)o.width * BYTES_PER_PIXEL;
        const long L = RawLineCount(file, "image", lineBytes);
        alloc_flags(o.width, L);
        ReadStrip(file, StripPlan{0, L, L, 0, StripBlockLines(lineBytes, C, BlockLinesHook("OIP_MASK_BLOCK_LINES", C)), lineBytes},
                  [&](const uint16_t *d, long r, long m) {
                      ck(oip_mask_cells_u16(ctx, d, o.width, o.width, m, 1, C, o.validMin, sat, full, o.band, o.q8[0], o.q8[1], o.q8[2], o.q8[3],
                                            flags.p + (size_t)(r / C) * gw, gw, counts.p));
                  });
        ck(oip_sync(ctx));
        inBytes = (size_t)L * lineBytes;
    }
    if (cloud) ck(oip_mask_morph_u8(ctx, flags.p, gw, gw, gh, o.open, o.buffer, counts.p));
    std::vector<uint8_t> host((size_t)gw * gh);
    uint64_t n[8];
    flags.download(host.data(), host.size());
    counts.download(n, 8);
    ck(oip_sync(ctx));
    if (spp == MSS_BANDS && o.noCloud) {    // --no-cloud on four samples: the candidates are dropped, nothing was opened
        for (uint8_t &b : host) b &= (uint8_t)(OIP_MASK_NODATA | OIP_MASK_SATURATED);
        n[3] = n[4] = 0;
    }
    OLOG("Write mask (%d x %ld cells of %d x %d) to file '%s' ...", gw, gh, C, C, paths.tiff.c_str());
    write_tiff_u8(paths.tiff, host.data(), gw, gh, 1);
    // (without a cloud stage the report says so: the four tests disabled, no opening, no buffer)
    const int off[4] = {-1, -1, -1, -1};
    const std::string params = MaskParamsLine(file, C, width, height, o.bits, sat, o.validMin, o.band, cloud ? o.q8 : off, cloud ? o.open : 0, cloud ? o.buffer : 0);
    WriteTextFile(paths.csv, [&](FILE *f) { return WriteMaskReport(f, params, n); });
    OLOG("mask: %s", MaskSummaryLine(n).c_str());
    OLOG("Report written to '%s'.", paths.csv.c_str());
    LogThroughput(inBytes, total.tick());
}

// ---- oip wallis: local brightness and contrast equalisation of a strip or product ------------------------------------------------
// The Wallis filter.  A read-only pass gives every B x B block its n, S1, S2 (oip_block_moments_u16); the host turns them into a
// gain and an offset per block and channel (oip_wallis_fit), which pull the block's mean and standard deviation toward the
// image's own (or a given) pair; the second pass transforms every sample with the gain and offset interpolated between the
// blocks' centres (oip_wallis_apply_u16).  The product has the size and container of the input (<stem>.WAL.<ext>), the figures
// go to <stem>.WAL.CSV (oip_wallisreport.hpp).  A TIFF product is resident; a RAW strip is read twice, the node tables stay on
// the device in between.  With --line-offset / --lines the selected lines are the raster.  The defaults (contrast 0.8,
// brightness 0.6, gains 0.25 .. 4, blocks of 128) are conventions: nothing was measured on real imagery.  Not in the reference.
struct WallisOptions {
    int width = OIP_PIXELS_PER_LINE;        // RAW input: samples per line
    int block = 128;
    double contrast = 0.8, brightness = 0.6, gMin = 0.25, gMax = 4.0;
    long minCount = 0;
    int validMin = 1, validMax = 65535, maxValue = 65535;
    std::vector<double> mean, std;          // --mean / --std: none, one for every channel, or one per channel
    long lineOffset = 0, lines = 0;         // lines == 0: to the end of the image
    bool force = false;
    std::string report;                     // --report: the CSV; empty: <stem>.WAL.CSV
};

struct WallisPaths {
    std::string image, csv;
};

// what is refused without a device and depends on the image (the option ranges are run_wallis's): the container, the size of a
// RAW file, the samples of a TIFF, the line range, targets that are not one or one per channel, the two outputs; returns the
// output paths, whether the input is a TIFF and its samples per pixel
inline WallisPaths WallisCheck(const std::string &file, const std::string &out, const WallisOptions &o, bool *isTiff, int *spp)
{
    const std::string ext = RasterContainer(file, "wallis");
    *isTiff = ext == ".tiff";
    *spp = 1;
    long first = 0, n = 0;
    if (*isTiff) {
        int w = 0;
        long h = 0;
        read_tiff_geometry(file, &w, &h, spp);
        if (*spp != 1 && *spp != MSS_BANDS) throw std::invalid_argument("wallis: a TIFF of 1 or 4 samples per pixel expected");
        LineRange("image", h, o.lineOffset, o.lines, &first, &n);
    } else {
        RawLineRange(file, "image", o.width, o.lineOffset, o.lines, &first, &n);
    }
    for (const std::vector<double> *t : {&o.mean, &o.std})
        if (t->size() > 1 && (int)t->size() != *spp)
            throw std::invalid_argument("wallis: --mean / --std take one value, or one per sample of a pixel (" + std::to_string(*spp) + ")");
    WallisPaths p;
    p.csv = o.report.empty() ? IMO::BuildOutputFilePath(file, OIP_WALLIS_SUFFIX, ".CSV") : o.report;
    p.image = out.empty() ? IMO::BuildOutputFilePath(file, OIP_WALLIS_SUFFIX) : out;
    if (p.image == p.csv) throw std::invalid_argument("output file [" + p.image + "] is named for the image and for the report");
    GuardOutput(p.csv, {file}, "wallis", o.force);
    FilterOutputPath(file, p.image, OIP_WALLIS_SUFFIX, ext, "wallis", o.force);
    return p;
}

inline void RunWallis(const std::string &file, const std::string &out, const WallisOptions &o)
{
    bool isTiff = false;
    int spp = 1;
    const WallisPaths paths = WallisCheck(file, out, o, &isTiff, &spp);
    const int B = o.block;
    OLOG("wallis: blocks of %d, contrast %g, brightness %g, gain %g .. %g, valid %d .. %d, max value %d", B, o.contrast, o.brightness, o.gMin, o.gMax,
         o.validMin, o.validMax, o.maxValue);
    oip_ctx *ctx = Device::get().ctx();
    auto ck = [](int rc) { Device::get().check(rc); };
    stop_watch total;
    int W = 0, gw = 0;
    long L = 0, gh = 0, first = 0;
    DevBuf<uint64_t> acc, stats(3);
    DevBuf<int32_t> gain, offset;
    std::vector<double> report;
    ck(oip_memset(ctx, stats.p, 0, 3 * sizeof(uint64_t)));
    auto alloc_acc = [&](int w, long lines) {
        W = w;
        L = lines;
        if (oip_wallis_grid(W, L, B, &gw, &gh) != OIP_OK || gw < 1 || gh < 1) throw std::invalid_argument("wallis: the image is empty");
        acc.alloc((size_t)3 * spp * gw * gh);
    };
    // moments on the host -> node tables on the device
    auto fit = [&]() {
        const size_t nodes = (size_t)gw * gh * spp;
        std::vector<uint64_t> moments((size_t)3 * nodes);
        ck(oip_sync(ctx));
        acc.download(moments.data(), moments.size());
        std::vector<double> tm(spp, std::nan("")), ts(spp, std::nan(""));
        for (int c = 0; c < spp; ++c) {
            if (!o.mean.empty()) tm[c] = o.mean[o.mean.size() == 1 ? 0 : c];
            if (!o.std.empty()) ts[c] = o.std[o.std.size() == 1 ? 0 : c];
        }
        std::vector<int32_t> G(nodes), O(nodes);
        std::vector<int> sub(nodes);
        report.assign((size_t)9 * spp, 0.0);
        char err[512] = "";
        const int rc = oip_wallis_fit(moments.data(), gw, (size_t)gw * gh, gw, gh, spp, o.contrast, o.brightness, o.gMin, o.gMax, (uint64_t)o.minCount,
                                      tm.data(), ts.data(), G.data(), O.data(), sub.data(), report.data(), err, sizeof err);
        if (rc == OIP_E_INVALID) throw std::invalid_argument(err);
        if (rc != OIP_OK) throw std::runtime_error(err);
        for (int c = 0; c < spp; ++c) OLOG("wallis: %s", WallisSummaryLine(c, report.data() + 9 * c).c_str());
        gain.assign(G);
        offset.assign(O);
    };
    size_t bytes = 0;
    if (isTiff) {
        ResidentImage m;
        LoadTiffProduct(file, "wallis", &m);
        long n = 0;
        LineRange("image", m.h, o.lineOffset, o.lines, &first, &n);
        alloc_acc(m.w, n);
        uint16_t *img = m.buf.p + (size_t)first * m.w * spp;
        ck(oip_block_moments_u16(ctx, img, (long)W * spp, W, L, spp, B, o.validMin, o.validMax, acc.p, gw, (size_t)gw * gh));
        fit();
        ck(oip_wallis_apply_u16(ctx, img, img, 0, L, W, L, spp, B, gain.p, offset.p, gw, gh, o.validMin, o.validMax, o.maxValue, stats.p));
        OLOG("Write equalised image to file '%s' ...", paths.image.c_str());
        write_tiff_from_device(paths.image, img, W, L, spp, tiff_compression(spp == 1 ? TIFF_NONE : TIFF_LZW), false);
        bytes = (size_t)W * L * spp * BYTES_PER_PIXEL;
    } else {
        const size_t lineBytes = (size_t)o.width * BYTES_PER_PIXEL;
        long n = 0;
        const long fileLines = RawLineRange(file, "image", o.width, o.lineOffset, o.lines, &first, &n);
        alloc_acc(o.width, n);
        // pass 1: the moments per line block of the strip, a block being a multiple of B lines
        ReadStrip(file, StripPlan{first, L, fileLines, 0, StripBlockLines(lineBytes, B, BlockLinesHook("OIP_WALLIS_BLOCK_LINES", B)), lineBytes},
                  [&](const uint16_t *d, long r, long m) {
                      ck(oip_block_moments_u16(ctx, d, W, W, m, 1, B, o.validMin, o.validMax, acc.p + (size_t)(r / B) * gw, gw, (size_t)gw * gh));
                  });
        fit();
        // pass 2: the transform is pointwise, a block needs no halo and may be cut anywhere
        StreamStrip(file, StripPlan{first, L, fileLines, 0, StripBlockLines(lineBytes, 1, BlockLinesHook("OIP_WALLIS_BLOCK_LINES")), lineBytes}, &paths.image,
                    [&](const uint16_t *d, long, long, uint16_t *q, long r, long m) {
                        ck(oip_wallis_apply_u16(ctx, d, q, r - first, m, W, L, 1, B, gain.p, offset.p, gw, gh, o.validMin, o.validMax, o.maxValue, stats.p));
                    });
        bytes = (size_t)L * lineBytes;
    }
    uint64_t n[3];
    ck(oip_sync(ctx));
    stats.download(n, 3);
    const std::string params = WallisParamsLine(file, W, first, L, spp, B, o.contrast, o.brightness, o.gMin, o.gMax, o.minCount, o.validMin, o.validMax, o.maxValue);
    WriteTextFile(paths.csv, [&](FILE *f) { return WriteWallisReport(f, params, spp, report.data(), n); });
    OLOG("wallis: %llu samples transformed, %llu clamped at %d, %llu clamped at %d", (unsigned long long)n[0], (unsigned long long)n[1], o.validMin,
         (unsigned long long)n[2], o.maxValue);
    OLOG("Report written to '%s'.", paths.csv.c_str());
    LogThroughput(bytes, total.tick());
}

// ---- oip mtf: the MTF at Nyquist from the edges of a strip or product -------------------------------------------------------
// The measuring side of mtfc's --mtf-x / --mtf-y.  Per line block, axis and band: every 32 x 32 tile gets a record
// (oip_mtf_tiles_u16), the status-0 tiles are listed in (channel, ty, tx) order and binned into edge-spread functions
// (oip_mtf_esf_u16), and oip_mtf_tile turns each into a value.  Rows, status counts and order statistics go to <stem>.MTF.CSV
// (oip_mtfreport.hpp).  Tiles are anchored at the first line of the range; a RAW strip streams through in blocks that are
// multiples of 32 lines with 32 halo lines, of which the y tiles that start in a block read up to 16 below it, so the report
// does not depend on the block size; a TIFF product is resident.  Not in the reference.
struct MtfOptions {
    int width = OIP_PIXELS_PER_LINE;        // RAW input: samples per line
    int axes = 3;                           // bit 0: x (across the lines), bit 1: y (along the lines)
    int contrastMin = 200, tvSlack = 256;
    std::string noiseReport;                // --noise: tv_slack per band from the sigma_ref of a report of `oip noise`
    int validMin = 1, validMax = 65535;
    long lineOffset = 0, lines = 0;         // lines == 0: to the end of the image
    bool force = false;
    std::string params;                     // the first line of the report
};

// what is refused without a device and depends on the image (the option ranges are run_mtf's): the container, the size and line
// range of a RAW file, an image without a tile, the noise report, the output; returns the output path and whether the input is
// a TIFF, and in *slack the slack of every band of a --noise report (empty without one)
inline std::string MtfCheck(const std::string &file, const std::string &out, const MtfOptions &o, bool *isTiff, std::vector<int> *slack)
{
    *isTiff = RasterContainer(file, "mtf") == ".tiff";
    if (!*isTiff) {
        if (o.width <= 0) throw std::invalid_argument("--width: a positive line width expected");
        long first = 0, n = 0;
        RawLineRange(file, "image", o.width, o.lineOffset, o.lines, &first, &n);
        if (n < 32 || o.width < 32) throw std::invalid_argument("mtf: the image holds no tile of 32 x 32");
    }
    slack->clear();
    if (!o.noiseReport.empty()) {
        std::vector<NoiseModel> models;
        std::string err;
        if (!ParseNoiseReport(o.noiseReport, &models, &err)) throw std::runtime_error(err);
        for (const NoiseModel &m : models) slack->push_back(oip_mtf_tv_slack(std::sqrt(m.a + m.b * m.muRef)));
    }
    const std::string path = out.empty() ? IMO::BuildOutputFilePath(file, OIP_MTF_SUFFIX, ".CSV") : out;
    GuardOutput(path, {file}, "mtf", o.force);
    return path;
}

inline void RunMtf(const std::string &file, const std::string &out, const MtfOptions &o)
{
    bool isTiff = false;
    std::vector<int> noiseSlack;
    const std::string outPath = MtfCheck(file, out, o, &isTiff, &noiseSlack);
    oip_ctx *ctx = Device::get().ctx();
    auto ck = [](int rc) { Device::get().check(rc); };
    stop_watch total;
    std::vector<MtfRow> rows;
    std::vector<std::vector<MtfGroup>> groups;                          // [band][axis]
    DevBuf<int32_t> rec, list, s0;
    DevBuf<uint32_t> esf;
    std::vector<int32_t> hrec, hlist, hs0;
    std::vector<uint32_t> hesf;
    auto slack_of = [&](int band) {                                     // band: 0-based
        if (noiseSlack.empty()) return o.tvSlack;
        if ((size_t)band >= noiseSlack.size())
            throw std::runtime_error("noise report [" + o.noiseReport + "] holds " + std::to_string(noiseSlack.size()) + " band(s), the image more");
        return noiseSlack[band];
    };
    // the tiles that START in lines [a, a + m) of the n-line range, of which `src` holds line a first and at least 16 lines
    // past a + m where the range has them
    auto block = [&](const uint16_t *src, long pitch, int w, int spp, long a, long m, long n) {
        if ((int)groups.size() < spp) groups.resize(spp, std::vector<MtfGroup>(2));
        for (int axis = 0; axis < 2; ++axis) {
            if (!(o.axes >> axis & 1)) continue;
            const long step = axis == 0 ? 32 : 16;
            const long ty0 = a / step, tyEnd = std::min((a + m + step - 1) / step, n >= 32 ? (n - 32) / step + 1 : 0);
            const long nty = tyEnd - ty0, ntx = axis == 0 ? (w - 32) / 16 + 1 : w / 32;
            if (nty < 1 || ntx < 1) continue;
            const long rowsIn = step * (nty - 1) + 32;
            const size_t plane = (size_t)nty * ntx;
            if (rec.n < plane * spp * 4) rec.alloc(plane * spp * 4);
            hrec.resize(plane * spp * 4);
            int slackDone = -1;                                         // the slack the records on the host were made with
            for (int c = 0; c < spp; ++c) {
                const int slack = slack_of(c);
                if (slack != slackDone) {                               // (only bands of a --noise report differ)
                    ck(oip_mtf_tiles_u16(ctx, src, pitch, w, rowsIn, spp, axis, o.contrastMin, slack, o.validMin, o.validMax, rec.p, ntx, plane));
                    rec.download(hrec.data(), plane * spp * 4);
                    slackDone = slack;
                }
                const int32_t *crec = &hrec[(size_t)c * plane * 4];
                hlist.clear();
                MtfGroup &g = groups[c][axis];
                for (long ty = 0; ty < nty; ++ty)
                    for (long tx = 0; tx < ntx; ++tx) {
                        const int32_t *r = &crec[((size_t)ty * ntx + tx) * 4];
                        ++g.tiles;
                        ++g.status[r[0] & 7];
                        if (r[0] == OIP_MTF_OK) { hlist.push_back(c); hlist.push_back((int32_t)ty); hlist.push_back((int32_t)tx); }
                    }
                const size_t k = hlist.size() / 3;
                if (k == 0) continue;
                if (list.n < k * 3) { list.alloc(k * 3); esf.alloc(k * 128); s0.alloc(k); }
                list.upload(hlist.data(), k * 3);
                ck(oip_mtf_esf_u16(ctx, src, pitch, w, rowsIn, spp, axis, o.contrastMin, slack, o.validMin, o.validMax, list.p, (long)k, esf.p, s0.p));
                hesf.resize(k * 128);
                hs0.resize(k);
                esf.download(hesf.data(), k * 128);
                s0.download(hs0.data(), k);
                for (size_t i = 0; i < k; ++i) {
                    const int32_t *r = &crec[((size_t)hlist[3 * i + 1] * ntx + hlist[3 * i + 2]) * 4];
                    MtfRow row;
                    const int rc = oip_mtf_tile(r[1], &hesf[i * 128], &hesf[i * 128 + 64], &row.mtf);
                    if (rc == OIP_MTF_NO_VALUE) { ++g.emptybin; continue; }
                    if (rc != OIP_OK) throw std::runtime_error("oip_mtf_tile: bad argument");
                    row.band = c + 1; row.axis = axis; row.ty = ty0 + hlist[3 * i + 1]; row.tx = hlist[3 * i + 2];
                    row.polarity = r[1]; row.slopeQ = r[3]; row.sumS0 = hs0[i];
                    rows.push_back(row);
                    g.values.push_back(row.mtf);
                }
            }
        }
    };
    size_t inBytes = 0;
    long first = 0, nLines = 0;
    if (isTiff) {
        ResidentImage m;
        LoadTiffProduct(file, "mtf", &m);
        LineRange("image", m.h, o.lineOffset, o.lines, &first, &nLines);
        if (nLines < 32 || m.w < 32) throw std::invalid_argument("mtf: the image holds no tile of 32 x 32");
        const long bl = BlockLinesHook("OIP_MTF_BLOCK_LINES", 32);
        for (long a = 0; a < nLines; a += bl > 0 ? bl : nLines)
            block(m.buf.p + (size_t)(first + a) * m.w * m.spp, (long)m.w * m.spp, m.w, m.spp, a, std::min(bl > 0 ? bl : nLines, nLines - a), nLines);
        inBytes = (size_t)nLines * m.w * m.spp * BYTES_PER_PIXEL;
    } else {
        const long fileLines = RawLineRange(file, "image", o.width, o.lineOffset, o.lines, &first, &nLines);
        const size_t lineBytes = (size_t)o.width * BYTES_PER_PIXEL;
        StreamStrip(file, StripPlan{first, nLines, fileLines, 32, StripBlockLines(lineBytes, 32, BlockLinesHook("OIP_MTF_BLOCK_LINES", 32)), lineBytes}, nullptr,
                    [&](const uint16_t *d, long s0Line, long, uint16_t *, long r, long m) {
                        block(d + (size_t)(r - s0Line) * o.width, o.width, o.width, 1, r - first, m, nLines);
                    });
        inBytes = (size_t)nLines * lineBytes;
    }
    ck(oip_sync(ctx));
    for (int a = 0; a < 2; ++a) {
        if (!(o.axes >> a & 1)) continue;
        size_t values = 0;
        for (const auto &g : groups) values += g[a].values.size();
        if (values == 0) {
            MtfGroup all;
            for (const auto &g : groups) all.add(g[a]);
            throw std::runtime_error("mtf: no tile with a value on axis " + std::string(MtfAxisName(a)) + " (" + MtfGroupLine("all", a, all) + ")");
        }
    }
    WriteTextFile(outPath, [&](FILE *f) { return WriteMtfReport(f, o.params, rows, groups, o.axes); });
    for (size_t b = 0; b < groups.size(); ++b)
        for (int a = 0; a < 2; ++a)
            if (o.axes >> a & 1) OLOG("mtf: %s", MtfGroupLine("band " + std::to_string(b + 1), a, groups[b][a]).c_str());
    const double es = total.tick();
    OLOG("Report written to '%s'; %zu bytes in %.3f seconds (%.1f MBps).", outPath.c_str(), inBytes, es, inBytes / es / 1024.0 / 1024.0);
}

// ---- oip overviews: the reduced-resolution pyramid of a strip or product ------------------------------------------------
// Every band at 16 bits, each level the 2 x 2 average of the one before that skips no data (oip_halve_u16), written where
// GDAL, QGIS and libtiff programs look for it: <IMAGE>.ovr beside the image, a TIFF of chained reduced-resolution
// directories (write_overviews_from_device).  A RAW strip is halved block by block into a resident level 1, a quarter of the
// strip; a TIFF product is resident.  `oip stitch --overviews` writes the same of its product while that is still in HBM.
// Not in the reference.
struct OverviewsOptions {
    int width = OIP_PIXELS_PER_LINE;        // RAW input: samples per line
    OverviewOptions pyramid;                // --levels (0: oip_overview_levels), --valid-min
    bool force = false;
};

// what is refused without a device and depends on the image (--levels and --valid-min are run_overviews'): the container,
// --width and the size of a RAW file, the output; returns the output path
inline std::string OverviewsCheck(const std::string &file, const std::string &out, const OverviewsOptions &o, bool *isTiff)
{
    *isTiff = RasterContainer(file, "overviews") == ".tiff";
    if (!*isTiff) {
        if (o.width <= 0) throw std::invalid_argument("--width: a positive line width expected");
        RawLineCount(file, "image", (size_t)o.width * BYTES_PER_PIXEL);
    }
    // (not FilterOutputPath: the overview file is a TIFF named after the whole file name of the image, beside it)
    const std::string path = out.empty() ? file + OIP_OVERVIEW_SUFFIX : out;
    GuardOutput(path, {file}, "overviews", o.force);
    return path;
}

inline void RunOverviews(const std::string &file, const std::string &out, const OverviewsOptions &o)
{
    bool isTiff = false;
    const std::string outPath = OverviewsCheck(file, out, o, &isTiff);
    oip_ctx *ctx = Device::get().ctx();
    auto ck = [](int rc) { Device::get().check(rc); };
    stop_watch total;
    size_t bytes = 0;
    if (isTiff) {
        ResidentImage m;
        LoadTiffProduct(file, "overviews", &m);
        write_overviews_of_device_image(outPath, m.buf.p, m.w, m.h, m.spp, o.pyramid);
        bytes = m.bytes();
    } else {
        // level 1 is built per line block of the strip (ReadStrip), a block being an even number of lines
        const int W = o.width;
        const size_t lineBytes = (size_t)W * BYTES_PER_PIXEL;
        const long L = RawLineCount(file, "image", lineBytes);
        const int w1 = (W + 1) / 2;
        DevBuf<uint16_t> level1((size_t)w1 * ((L + 1) / 2));
        ReadStrip(file, StripPlan{0, L, L, 0, StripBlockLines(lineBytes, 2, BlockLinesHook("OIP_OVERVIEWS_BLOCK_LINES", 2)), lineBytes}, [&](const uint16_t *d, long r, long m) {
            ck(oip_halve_u16(ctx, d, W, W, m, 1, o.pyramid.validMin, level1.p + (size_t)(r / 2) * w1, w1));
        });
        write_overviews_from_device(outPath, level1, W, L, 1, o.pyramid.levels > 0 ? o.pyramid.levels : oip_overview_levels(W, L), o.pyramid.validMin);
        bytes = (size_t)L * lineBytes;
    }
    LogThroughput(bytes, total.tick());
}

// ---- oip cog: a product or strip as a tiled TIFF with internal overviews -------------------------------------------------
// The image in T x T tiles and its pyramid -- the levels `oip overviews` writes to <IMAGE>.ovr, sample for sample -- in ONE
// file whose directories all lie ahead of the pixels (TiffTiledWriterU16, oip_tifftiled.hpp): a reader gets a window at any
// resolution by decoding the tiles it covers.  The image is resident (a TIFF product, strips or tiles, or a whole single-band
// RAW strip); every directory leaves through tiled_image_from_device, the levels alternating between two buffers as
// write_overviews_from_device does.  Not in the reference.
struct CogOptions {
    int width = OIP_PIXELS_PER_LINE;        // RAW input: samples per line
    int tile = 0;                           // --tile: a multiple of 16 in 16..1024; 0: OIP_COG_DEF_TILE, at 4 samples OIP_COG_DEF_TILE_4
    int levels = -1;                        // --levels: 0 none, 1..16; -1: oip_overview_levels
    int validMin = 1;                       // --valid-min, as in `oip overviews`
    bool force = false;
};

// what is refused without a device and depends on the image (--tile, --levels and --valid-min are run_cog's): the container,
// --width and the size of a RAW file, the output; returns the output path
inline std::string CogCheck(const std::string &file, const std::string &out, const CogOptions &o, bool *isTiff)
{
    *isTiff = RasterContainer(file, "cog") == ".tiff";
    if (!*isTiff) {
        if (o.width <= 0) throw std::invalid_argument("--width: a positive line width expected");
        RawLineCount(file, "image", (size_t)o.width * BYTES_PER_PIXEL);
    }
    const std::string path = out.empty() ? IMO::BuildOutputFilePath(file, OIP_COG_SUFFIX, ".TIFF") : out;
    GuardOutput(path, {file}, "cog", o.force);
    return path;
}

inline void RunCog(const std::string &file, const std::string &out, const CogOptions &o)
{
    bool isTiff = false;
    const std::string outPath = CogCheck(file, out, o, &isTiff);
    oip_ctx *ctx = Device::get().ctx();
    auto ck = [](int rc) { Device::get().check(rc); };
    stop_watch total;
    ResidentImage m;
    LoadResident(file, isTiff, o.width, "image", "cog", &m);
    const int spp = m.spp, T = o.tile > 0 ? o.tile : (spp == MSS_BANDS ? OIP_COG_DEF_TILE_4 : OIP_COG_DEF_TILE);
    const int levels = o.levels >= 0 ? o.levels : oip_overview_levels(m.w, m.h);
    const int comp = tiff_compression(spp == 1 ? TIFF_NONE : TIFF_LZW);
    OLOG("Write image in %d x %d tiles and %d overview levels to file '%s' ...", T, T, levels, outPath.c_str());
    TiffTiledWriterU16 tw(outPath, m.w, m.h, spp, T, comp, levels);
    DevBuf<uint16_t> lv[2];
    const uint16_t *cur = m.buf.p;
    for (int k = 0; k <= levels; ++k) {
        const int w = tw.width();
        const long h = tw.height();
        RLOG("    level %d: %d x %ld x %d, %ld x %ld tiles", k, w, h, spp, tw.tiles_x(), tw.tiles_y());
        tiled_image_from_device(tw, outPath, cur, w, h, spp, T, comp);
        if (k == levels) break;
        const int nw = (w + 1) / 2;
        const long nh = (h + 1) / 2;
        DevBuf<uint16_t> &next = lv[k & 1];
        if (!next.p) next.alloc((size_t)nw * nh * spp);                 // (level 1 and level 2: every later level fits the one two before it)
        ck(oip_halve_u16(ctx, cur, (long)w * spp, w, h, spp, o.validMin, next.p, (long)nw * spp));
        tw.next_directory();
        cur = next.p;
    }
    tw.close();
    LogThroughput(m.bytes(), total.tick());
}

// ---- oip rescale: a strip or product on another pixel grid ------------------------------------------------------------------
// Antialiased resampling by a separable polyphase filter (include/oip_c.h: oip_rescale_taps, oip_rescale_u16): a scale along the
// lines corrects a line rate that does not match the ground speed, a scale on both axes delivers at a stated sample distance,
// and x 4 brings the aligned MSS product to the PAN grid without fusing it.  A scale is a rational p / q (a decimal is read as
// one), an axis that is not named keeps its size, --to-width / --to-lines name a size outright.  The image is resident, in and
// out (2 (W L + Wo Lo) spp bytes of device memory); the tables are built on the host; one kernel call; the output leaves
// through the product writer (TIFF) or as it lies (RAW).  Lanczos-3 and Q14 taps are conventions: nothing was measured on real
// imagery.  Not in the reference.
struct RescaleOptions {
    int width = OIP_PIXELS_PER_LINE;        // RAW input: samples per line
    long px = 1, qx = 1, py = 1, qy = 1;    // the scales across and along as rationals
    long toWidth = 0, toLines = 0;          // --to-width / --to-lines: the size outright; 0: by the scale
    int kind = OIP_RESCALE_LANCZOS;
    int validMin = 1;                       // 0: no no-data rule
    bool force = false;
};

struct RescaleGeometry {
    std::string path;
    bool inTiff = false, outTiff = false;
    int W = 0, Wo = 0, spp = 1;
    long L = 0, Lo = 0;
};

// what is refused without a device and depends on the image (the option syntax is run_rescale's): the container, the size of a
// RAW file, the samples of a TIFF, an empty axis or a ratio outside 1/4 .. 16 on either axis, the container of the output (a RAW
// file holds one sample per pixel), the output itself
inline RescaleGeometry RescaleCheck(const std::string &file, const std::string &out, const RescaleOptions &o)
{
    RescaleGeometry g;
    const std::string ext = RasterContainer(file, "rescale");
    g.inTiff = ext == ".tiff";
    if (g.inTiff) {
        read_tiff_geometry(file, &g.W, &g.L, &g.spp);
        if (g.spp != 1 && g.spp != MSS_BANDS) throw std::invalid_argument("rescale: a TIFF of 1 or 4 samples per pixel expected");
    } else {
        g.W = o.width;
        g.L = RawLineCount(file, "image", (size_t)o.width * BYTES_PER_PIXEL);
    }
    long wo = o.toWidth, lo = o.toLines;
    if (wo == 0 && oip_rescale_size_impl(g.W, o.px, o.qx, &wo) != OIP_OK) throw std::invalid_argument("rescale: the scale across the line gives no valid width");
    if (lo == 0 && oip_rescale_size_impl(g.L, o.py, o.qy, &lo) != OIP_OK) throw std::invalid_argument("rescale: the scale along the strip gives no valid line count");
    if (const char *why = oip_rescale_axis_refusal(g.W, wo))
        throw std::invalid_argument("rescale: " + std::to_string(g.W) + " -> " + std::to_string(wo) + " pixels a line: " + why + " (ratios of 1/4 .. 16 are supported)");
    if (const char *why = oip_rescale_axis_refusal(g.L, lo))
        throw std::invalid_argument("rescale: " + std::to_string(g.L) + " -> " + std::to_string(lo) + " lines: " + why + " (ratios of 1/4 .. 16 are supported)");
    if (wo * g.spp >= (1L << 31)) throw std::invalid_argument("rescale: an output line of 2^31 samples or more");
    g.Wo = (int)wo;
    g.Lo = lo;
    g.path = out.empty() ? IMO::BuildOutputFilePath(file, OIP_RESCALE_SUFFIX) : out;
    const std::string oext = to_lower(std::filesystem::path(g.path).extension().string());
    if (oext != ".tiff" && oext != ".raw") throw std::invalid_argument("rescale: the output is a RAW or a TIFF file");
    g.outTiff = oext == ".tiff";
    if (!g.outTiff && g.spp != 1) throw std::invalid_argument("rescale: a RAW file holds one sample per pixel, the image has " + std::to_string(g.spp));
    GuardOutput(g.path, {file}, "rescale", o.force);
    return g;
}

inline void RunRescale(const std::string &file, const std::string &out, const RescaleOptions &o)
{
    const RescaleGeometry g = RescaleCheck(file, out, o);
    static const char *const names[] = {"lanczos", "cubic", "linear"};
    // the tables of both axes, on the host
    std::vector<int> first[2];
    std::vector<int16_t> taps[2];
    int K[2] = {0, 0};
    for (int axis = 0; axis < 2; ++axis) {
        const long n_in = axis ? g.L : g.W, n_out = axis ? g.Lo : g.Wo;
        char err[256] = "";
        int rc = oip_rescale_taps(o.kind, n_in, n_out, nullptr, nullptr, 0, &K[axis], err, sizeof err);
        if (rc == OIP_OK) {
            first[axis].resize(n_out);
            taps[axis].resize((size_t)n_out * K[axis]);
            rc = oip_rescale_taps(o.kind, n_in, n_out, first[axis].data(), taps[axis].data(), taps[axis].size(), &K[axis], err, sizeof err);
        }
        if (rc == OIP_E_INVALID) throw std::invalid_argument(err);
        if (rc != OIP_OK) throw std::runtime_error(err);
    }
    OLOG("rescale: %d x %ld -> %d x %ld pixels of %d samples, kernel %s, %d x %d taps, valid-min %d", g.W, g.L, g.Wo, g.Lo, g.spp, names[o.kind], K[0], K[1],
         o.validMin);
    oip_ctx *ctx = Device::get().ctx();
    auto ck = [](int rc) { Device::get().check(rc); };
    stop_watch total;
    ResidentImage m;
    LoadResident(file, g.inTiff, o.width, "image", "rescale", &m);
    if (m.w != g.W || m.h != g.L || m.spp != g.spp) throw std::runtime_error("rescale: the image changed while it was read");
    DevBuf<int> fx, fy;
    DevBuf<int16_t> tx, ty;
    fx.assign(first[0]), tx.assign(taps[0]), fy.assign(first[1]), ty.assign(taps[1]);
    const size_t samples = (size_t)g.Wo * g.Lo * g.spp;
    DevBuf<uint16_t> res(samples);
    ck(oip_rescale_u16(ctx, m.buf.p, 0, g.L, g.W, g.L, g.spp, res.p, 0, g.Lo, g.Wo, g.Lo, fx.p, tx.p, K[0], fy.p, ty.p, K[1], o.validMin));
    if (g.outTiff) {
        OLOG("Write rescaled image of %d x %ld pixels to file '%s' ...", g.Wo, g.Lo, g.path.c_str());
        write_tiff_from_device(g.path, res.p, g.Wo, g.Lo, g.spp, tiff_compression(g.spp == 1 ? TIFF_NONE : TIFF_LZW), false);
    } else {
        OLOG("Write rescaled strip of %d x %ld samples (--width %d) to file '%s' ...", g.Wo, g.Lo, g.Wo, g.path.c_str());
        ck(oip_sync(ctx));
        res.save_file(g.path, samples);
    }
    LogThroughput(m.bytes() + samples * BYTES_PER_PIXEL, total.tick());
}

// ---- oip regcheck: how well two rasters are registered ------------------------------------------------------------------
// Dense template matching (oip_match_tiles_u16: ZNCC from exact integer sums, no code shared with the phase correlation it
// judges) of image 2 against image 1 on a grid of tiles; shift, score and flags per tile and the summary come from the
// records on the host (oip_regreport.hpp) and go to <stem of image1>.REG.CSV.  Both images are resident.  Three uses: band
// against band inside one aligned MSS product (one image, --band1 / --band2), PAN against an MSS band (--scale 4 box-decimates
// image 1 first), the CCD overlap (--shift-x W - fold).  Not in the reference.
struct RegcheckOptions {
    std::string image2;                     // empty: image 1
    int band1 = 1, band2 = 1;               // 1-based
    int scale = 1;                          // 1: none; 2 .. 64: box decimation of image 1 (oip_decimate_box_u16)
    long shiftX = 0, shiftY = 0;            // image 2's origin in (decimated) image-1 coordinates
    int tile = 64, search = 4, step = 0;    // step 0: the tile size
    int validMin = 1, validMax = 65535;
    double minScore = 0.5;
    int width = OIP_PIXELS_PER_LINE, width2 = 0;      // RAW inputs: samples per line (width2 0: width)
    bool bil = false;                       // refused: BIL RAW is left out on purpose
    bool force = false;
    std::string mask;                       // --mask: the mask of image 1 (`oip mask`); empty: none
    int maskCell = 8, maskBits = OIP_MASK_CLOUD | OIP_MASK_BUFFER;
    std::string params;                     // the first line of the report
};

// the mask of `regcheck --mask` on the host
struct RegcheckMask {
    std::vector<uint8_t> flags;
    int gw = 0;
    long gh = 0;
};

// what is refused without a device and depends on the images (the option ranges are run_regcheck's): the containers, --bil, a
// band index beyond the container's bands, the sizes of RAW files, a mask that is not what `oip mask` writes, the output;
// returns the output path, and the mask if one is named
inline std::string RegcheckCheck(const std::string &file, const std::string &out, const RegcheckOptions &o, bool *isTiff1, bool *isTiff2,
                                 RegcheckMask *mask)
{
    const std::string file2 = o.image2.empty() ? file : o.image2;
    *isTiff1 = RasterContainer(file, "regcheck") == ".tiff";
    *isTiff2 = RasterContainer(file2, "regcheck") == ".tiff";
    if (o.bil) throw std::invalid_argument("regcheck: a BIL RAW strip is not supported: split the bands first (the default action writes them)");
    const int bands[2] = {o.band1, o.band2};
    const bool tiff[2] = {*isTiff1, *isTiff2};
    for (int k = 0; k < 2; ++k) {
        const int nb = tiff[k] ? MSS_BANDS : 1;
        if (bands[k] < 1 || bands[k] > nb) throw usage_error(std::string(k ? "--band2" : "--band1") + ": band index out of range (1.." + std::to_string(nb) + ")");
    }
    if (!*isTiff1) RawLineCount(file, "image1", (size_t)o.width * BYTES_PER_PIXEL);
    if (!*isTiff2) RawLineCount(file2, "image2", (size_t)(o.width2 > 0 ? o.width2 : o.width) * BYTES_PER_PIXEL);
    std::vector<std::string> inputs = {file, file2};
    if (!o.mask.empty()) {
        read_tiff_u8(o.mask, &mask->gw, &mask->gh, &mask->flags);
        inputs.push_back(o.mask);
    }
    const std::string path = out.empty() ? IMO::BuildOutputFilePath(file, OIP_REGCHECK_SUFFIX, ".CSV") : out;
    GuardOutput(path, inputs, "regcheck", o.force);
    return path;
}

inline void RunRegcheck(const std::string &file, const std::string &out, const RegcheckOptions &o)
{
    bool isTiff[2] = {false, false};
    RegcheckMask mask;
    const std::string outPath = RegcheckCheck(file, out, o, &isTiff[0], &isTiff[1], &mask);
    const std::string file2 = o.image2.empty() ? file : o.image2;
    oip_ctx *ctx = Device::get().ctx();
    auto ck = [](int rc) { Device::get().check(rc); };
    stop_watch total;
    ResidentImage img[2];
    auto bandWithin = [](const char *key, int band, const ResidentImage &m) {
        if (band > m.spp) throw usage_error(std::string(key) + ": band index out of range (1.." + std::to_string(m.spp) + ")");
    };
    LoadResident(file, isTiff[0], o.width, "image1", "regcheck", &img[0]);
    bandWithin("--band1", o.band1, img[0]);
    RegMask rm;
    if (!o.mask.empty()) {                  // the mask is image 1's: its grid is that of image 1's pixels
        int gw = 0;
        long gh = 0;
        if (oip_mask_grid(img[0].w, img[0].h, o.maskCell, &gw, &gh) != OIP_OK || gw != mask.gw || gh != mask.gh)
            throw std::invalid_argument("regcheck: the mask [" + o.mask + "] is " + std::to_string(mask.gw) + " x " + std::to_string(mask.gh) + " cells, image 1 (" +
                                        std::to_string(img[0].w) + " x " + std::to_string(img[0].h) + " pixels) has " + std::to_string(gw) + " x " +
                                        std::to_string(gh) + " cells of " + std::to_string(o.maskCell));
        rm.flags = mask.flags.data(); rm.gw = mask.gw; rm.gh = mask.gh; rm.cell = o.maskCell; rm.bits = o.maskBits;
    }
    const bool shared = o.image2.empty() || std::filesystem::equivalent(file, file2);          // one file: read once
    if (!shared) LoadResident(file2, isTiff[1], o.width2 > 0 ? o.width2 : o.width, "image2", "regcheck", &img[1]);
    const ResidentImage &m2 = shared ? img[0] : img[1];
    bandWithin("--band2", o.band2, m2);

    // plane A: band1 of image 1, or of its F x F box decimation (one plane per band)
    const uint16_t *A = img[0].buf.p + (o.band1 - 1);
    long pitchA = (long)img[0].w * img[0].spp, w1 = img[0].w, h1 = img[0].h;
    int strideA = img[0].spp;
    DevBuf<uint16_t> planes;
    if (o.scale > 1) {
        const int F = o.scale, ow = (img[0].w + F - 1) / F;
        const long oh = (img[0].h + F - 1) / F;
        const size_t plane = (size_t)ow * oh;
        planes.alloc(plane * img[0].spp);
        ck(oip_decimate_box_u16(ctx, img[0].buf.p, pitchA, img[0].w, img[0].h, img[0].spp, F, planes.p, ow, plane));
        A = planes.p + (size_t)(o.band1 - 1) * plane;
        pitchA = ow; strideA = 1; w1 = ow; h1 = oh;
    }
    const uint16_t *B = m2.buf.p + (o.band2 - 1);
    const long pitchB = (long)m2.w * m2.spp;
    const int strideB = m2.spp;

    RegOverlap ov;
    RegGrid g;
    g.T = o.tile; g.S = o.search; g.step = o.step > 0 ? o.step : o.tile; g.scale = o.scale;
    if (!RegIntersect(w1, h1, m2.w, m2.h, o.shiftX, o.shiftY, &ov) || ov.w >= (1L << 31) ||
        oip_match_grid((int)ov.w, ov.h, g.T, g.S, g.step, &g.x0, &g.y0, &g.nx, &g.ny) != OIP_OK)
        throw std::invalid_argument("regcheck: the images overlap on " + std::to_string(ov.w) + " x " + std::to_string(ov.h) +
                                    " pixels, which holds no tile of " + std::to_string(g.T + 2 * g.S) + " x " + std::to_string(g.T + 2 * g.S));
    g.originX = ov.ax; g.originY = ov.ay;
    const size_t n = (size_t)g.nx * g.ny;
    OLOG("Matching %d x %ld tiles of %d x %d, search +-%d, on %ld x %ld pixels ...", g.nx, g.ny, g.T, g.T, g.S, ov.w, ov.h);
    DevBuf<uint64_t> records(n * OIP_MATCH_RECORD_WORDS);
    stop_watch sw;
    ck(oip_match_tiles_u16(ctx, A + ov.ay * pitchA + ov.ax * strideA, pitchA, strideA, B + ov.by * pitchB + ov.bx * strideB, pitchB, strideB, (int)ov.w, ov.h,
                           g.T, g.S, g.x0, g.y0, g.step, g.step, g.nx, g.ny, o.validMin, o.validMax, records.p, nullptr));
    std::vector<uint64_t> rec(n * OIP_MATCH_RECORD_WORDS);
    records.download(rec.data(), rec.size());
    ck(oip_sync(ctx));
    OLOG("Matched in %.3f seconds.", sw.tick());
    RegSummary sum;
    WriteTextFile(outPath, [&](FILE *f) { return WriteRegReport(f, o.params, rec.data(), g, o.minScore, &sum, o.mask.empty() ? nullptr : &rm); });
    OLOG("regcheck: %s", RegSummaryLine(sum).c_str());
    OLOG("Report written to '%s' in %.3f seconds.", outPath.c_str(), total.tick());
}

// ---- oip regfix: resample a raster by the shift field regcheck measured -----------------------------------------------------
// `oip regcheck` reports, per tile of a regular lattice, where image 1's content is found in image 2.  This tool turns that
// report into a displacement field (oip_warpfield.hpp: the tiles without a flag, the others filled from their neighbours,
// optional smoothing) and resamples image 2 by it (oip_warp_grid_bicubic_u16: the product's OpenCV-exact bicubic with a phase
// of its own per pixel), so that image 2 lands on image 1.  The three uses are regcheck's: a band of an aligned MSS product,
// an MSS band against PAN, CCD 2 on the overlap.  The output has the container of the input.  Not in the reference.
struct RegfixOptions {
    std::string report;
    std::vector<int> bands;                 // 1-based; empty: the report's band2
    bool allBands = false;
    int smooth = 0;
    int width = OIP_PIXELS_PER_LINE;        // RAW input: samples per line
    bool bil = false;                       // refused, as regcheck refuses it
    bool force = false;
};

// what is refused without a device and depends on the image (--smooth and --width are run_regfix's): the container, --bil, the
// samples of a TIFF, the size of a RAW file, the report against the image's size, the bands, the output; returns the output path
inline std::string RegfixCheck(const std::string &file, const std::string &out, const RegfixOptions &o, bool *isTiff, WarpField *field, int *bandMask)
{
    const std::string ext = RasterContainer(file, "regfix");
    *isTiff = ext == ".tiff";
    if (o.bil) throw std::invalid_argument("regfix: a BIL RAW strip is not supported: split the bands first (the default action writes them)");
    int w = 0, spp = 1;
    long h = 0;
    if (*isTiff) {
        read_tiff_geometry(file, &w, &h, &spp);
        if (spp != 1 && spp != MSS_BANDS) throw std::invalid_argument("regfix: a TIFF of 1 or 4 samples per pixel expected");
    } else {
        w = o.width;
        h = RawLineCount(file, "image", (size_t)o.width * BYTES_PER_PIXEL);
    }
    *field = ParseRegReport(ReadRegReport(o.report), w, h);
    SmoothField(field->X.data(), field->nx, field->ny, o.smooth);
    SmoothField(field->Y.data(), field->nx, field->ny, o.smooth);
    std::vector<int> bands = o.bands;
    if (o.allBands) { bands.clear(); for (int b = 1; b <= spp; ++b) bands.push_back(b); }
    else if (bands.empty()) bands.push_back(field->band2);
    *bandMask = 0;
    for (int b : bands) {
        if (b < 1 || b > spp) throw usage_error("--bands: band index out of range (1.." + std::to_string(spp) + ")");
        *bandMask |= 1 << (b - 1);
    }
    return FilterOutputPath(file, out, OIP_REGFIX_SUFFIX, ext, "regfix", o.force);
}

inline void RunRegfix(const std::string &file, const std::string &out, const RegfixOptions &o)
{
    bool isTiff = false;
    WarpField f;
    int mask = 0;
    const std::string outPath = RegfixCheck(file, out, o, &isTiff, &f, &mask);
    int minX = INT_MAX, maxX = INT_MIN, minY = INT_MAX, maxY = INT_MIN;
    for (size_t q = 0; q < f.X.size(); ++q) {
        minX = std::min(minX, f.X[q]); maxX = std::max(maxX, f.X[q]);
        minY = std::min(minY, f.Y[q]); maxY = std::max(maxY, f.Y[q]);
    }
    OLOG("regfix: %d x %d nodes at (%ld, %ld), step %d x %d, %ld of %ld tiles used, smooth %d", f.nx, f.ny, f.gx0, f.gy0, f.sx, f.sy, f.used,
         (long)f.nx * f.ny, o.smooth);
    OLOG("regfix: dx in [%.4f, %.4f], dy in [%.4f, %.4f] px, band mask %d", minX / 1024.0, maxX / 1024.0, minY / 1024.0, maxY / 1024.0, mask);
    oip_ctx *ctx = Device::get().ctx();
    auto ck = [](int rc) { Device::get().check(rc); };
    stop_watch total;
    // the halo of a strip's block holds the largest vertical shift and the bicubic window; a RAW strip's band mask is 1 (RegfixCheck)
    const size_t bytes = FilterImage(file, outPath, isTiff, o.width, (f.maxAbsY() + 1023) / 1024 + 3, "OIP_REGFIX_BLOCK_LINES", "regfix", "resampled",
                                     [&](const uint16_t *src, long s0, long sn, uint16_t *dst, long r, long m, int w, long L, int spp) {
                                         ck(oip_warp_grid_bicubic_u16(ctx, src, s0, sn, dst, r, m, w, L, spp, mask, f.X.data(), f.Y.data(), f.nx, f.ny,
                                                                      f.gx0, f.gy0, f.sx, f.sy));
                                     });
    LogThroughput(bytes, total.tick());
}

// ---- oip pansharpen: fuse the PAN strip and the aligned MSS product -------------------------------------------------------------
// The two products of one scene -- the stitched PAN strip and the stitched, band-aligned MSS product at a quarter of its
// resolution -- become one 4-band product at PAN resolution by smoothing-filter intensity modulation: each band is up-sampled by
// 4 and multiplied by PAN / up(low(PAN)), low(PAN) being the 4 x 4 box mean (oip_decimate_box_u16) -- the detail PAN holds beyond
// the MSS resolution, as a ratio (include/oip_c.h: oip_pansharpen_sfim_u16 states it to the bit).  All rasters are resident, as
// in `oip stitch` of TIFFs: about 1.33 bytes of device memory per output byte.  Not in the reference.
struct PansharpenOptions {
    std::string pan, mss;
    long lineOffset = 0;                    // the first PAN line used
    int maxGain = OIP_PANSHARPEN_DEF_GAIN;
    int width = OIP_PIXELS_PER_LINE;        // RAW PAN: samples per line
    bool force = false;
    bool overviews = false;                 // also <output>.ovr, as `stitch --overviews`
    OverviewOptions pyramid;
};

struct PansharpenGeometry {
    bool panTiff = false;
    int W = 0, w = 0;
    long Hp = 0, h = 0, outW = 0, outH = 0, mssLines = 0;
};

// what is refused without a device and depends on the images (--max-gain, --line-offset and --width are run_pansharpen's): the
// containers, the sample counts, the size of a RAW file, the geometry, the output and its overview file; returns the output path
inline std::string PansharpenCheck(const std::string &out, const PansharpenOptions &o, PansharpenGeometry *g)
{
    g->panTiff = RasterContainer(o.pan, "pansharpen") == ".tiff";
    if (RasterContainer(o.mss, "pansharpen") != ".tiff") throw std::invalid_argument("pansharpen: the MSS product is a TIFF of 4 samples per pixel");
    int spp = 1;
    if (g->panTiff) {
        read_tiff_geometry(o.pan, &g->W, &g->Hp, &spp);
        if (spp != 1) throw std::invalid_argument("pansharpen: a PAN TIFF of 1 sample per pixel expected, not " + std::to_string(spp));
    } else {
        g->W = o.width;
        g->Hp = RawLineCount(o.pan, "PAN", (size_t)o.width * BYTES_PER_PIXEL);
    }
    read_tiff_geometry(o.mss, &g->w, &g->h, &spp);
    if (spp != MSS_BANDS) throw std::invalid_argument("pansharpen: an MSS TIFF of 4 samples per pixel expected, not " + std::to_string(spp));
    if (g->W != 4L * g->w)
        throw std::invalid_argument("pansharpen: the PAN line (" + std::to_string(g->W) + ") is not 4 times the MSS line (" + std::to_string(g->w) + ")");
    if (oip_pansharpen_geometry(g->W, g->Hp, g->w, g->h, o.lineOffset, &g->outW, &g->outH, &g->mssLines) != OIP_OK)
        throw std::invalid_argument("pansharpen: the PAN raster has " + std::to_string(g->Hp) + " lines: fewer than 4 from --line-offset " +
                                    std::to_string(o.lineOffset) + " on");
    const std::string path = out.empty() ? IMO::BuildOutputFilePath(o.mss, OIP_PANSHARPEN_SUFFIX, ".TIFF") : out;
    if (to_lower(std::filesystem::path(path).extension().string()) != ".tiff") throw std::invalid_argument("pansharpen: the output is a TIFF");
    GuardOutput(path, {o.pan, o.mss}, "pansharpen", o.force);
    if (o.overviews) GuardOutput(path + OIP_OVERVIEW_SUFFIX, {o.pan, o.mss}, "pansharpen", o.force);
    return path;
}

inline void RunPansharpen(const std::string &out, const PansharpenOptions &o)
{
    PansharpenGeometry g;
    const std::string outPath = PansharpenCheck(out, o, &g);
    OLOG("pansharpen: PAN %d x %ld from line %ld, MSS %d x %ld -> %ld x %ld x %d, max gain %d", g.W, g.Hp, o.lineOffset, g.w, g.h, g.outW, g.outH,
         MSS_BANDS, o.maxGain);
    if (g.mssLines < g.h) OLOG("pansharpen: the PAN raster ends first: the last %ld MSS lines are left unused", g.h - g.mssLines);
    oip_ctx *ctx = Device::get().ctx();
    auto ck = [](int rc) { Device::get().check(rc); };
    stop_watch total;
    ResidentImage pan, mss;
    LoadResident(o.pan, g.panTiff, g.W, "PAN", "pansharpen", &pan);
    if (pan.w != g.W || pan.h != g.Hp || pan.spp != 1) throw std::runtime_error("pansharpen: the PAN file changed while it was read");
    LoadTiffProduct(o.mss, "pansharpen", &mss);
    if (mss.w != g.w || mss.h != g.h || mss.spp != MSS_BANDS) throw std::runtime_error("pansharpen: the MSS file changed while it was read");

    const uint16_t *p0 = pan.buf.p + (size_t)o.lineOffset * g.W;
    DevBuf<uint16_t> low((size_t)g.w * g.mssLines), res((size_t)g.outW * g.outH * MSS_BANDS);
    DevBuf<uint64_t> stats(2);
    const uint64_t none[2] = {0, 0};
    uint64_t count[2] = {0, 0};
    stats.upload(none, 2);
    stop_watch sw;
    ck(oip_decimate_box_u16(ctx, p0, g.W, g.W, g.outH, 1, 4, low.p, g.w, 0));
    ck(oip_pansharpen_sfim_u16(ctx, p0, g.W, mss.buf.p, (long)g.w * MSS_BANDS, low.p, g.w, g.w, g.mssLines, res.p, g.outW * MSS_BANDS, 0, g.outH, o.maxGain,
                               stats.p));
    stats.download(count, 2);
    const double px = (double)g.outW * g.outH;
    OLOG("pansharpen: fused in %.3f seconds; low-resolution PAN zero on %.4f %% of the pixels (gain 1), gain cut at %d on %.4f %%", sw.tick(),
         100.0 * count[0] / px, o.maxGain, 100.0 * count[1] / px);
    pan.buf.release();
    mss.buf.release();
    low.release();
    OLOG("Write fused image to file '%s' ...", outPath.c_str());
    write_tiff_from_device(outPath, res.p, (int)g.outW, g.outH, MSS_BANDS, tiff_compression(TIFF_LZW), false);
    if (o.overviews) write_overviews_of_device_image(outPath + OIP_OVERVIEW_SUFFIX, res.p, (int)g.outW, g.outH, MSS_BANDS, o.pyramid);
    LogThroughput((size_t)g.outW * g.outH * MSS_BANDS * BYTES_PER_PIXEL, total.tick());
}

}  // namespace OIPGPU
