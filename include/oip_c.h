/*
 * oip_c.h -- C ABI of liboipgpu.so, the MI355X (gfx950) implementation of the
 * arloan/OpticalImageProcessor hot path: per-column relative radiometric correction,
 * cross-CCD / inter-band phase correlation, bicubic resampling and strip stitching.
 *
 * The reference has no FFI: the path sits behind header-only C++ classes with static
 * methods (IMO, Stitcher, PreProcessor).  Each entry point below names the reference
 * seam it replaces (file:line under OpticalImageProcessor/).  INTEGRATION.md shows the
 * few lines a maintainer adds to the reference to call them.
 *
 * Conventions
 *   - plain pointers and sizes only; `d_*` arguments are device (HBM) pointers, everything
 *     else is host memory.  Rasters are headerless row-major uint16 (little endian), pitch ==
 *     width, exactly the reference's RAW layout (oipshared.h:27-32).
 *   - every call returns an oip_status; oip_last_error(ctx) gives the message.  The status
 *     classes mirror the exception types the reference throws so a C++ shell can re-throw
 *     them and keep the exit codes of main.cpp:320-343.
 *   - kernels are enqueued on the context's stream and are asynchronous unless the
 *     function returns host values (then it synchronises the stream itself).
 *   - one oip_ctx per device; a context is not thread-safe, distinct contexts are independent.
 *   - there is NO CPU fallback: without a gfx950 device oip_create fails.
 */
#ifndef OIP_C_H
#define OIP_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct oip_ctx oip_ctx;

typedef enum oip_status {
    OIP_OK = 0,
    OIP_E_INVALID = 1,   /* std::invalid_argument in the reference                       */
    OIP_E_RUNTIME = 2,   /* std::runtime_error                                           */
    OIP_E_IO = 3,        /* errno_error (open/read/write/stat)                           */
    OIP_E_DEVICE = 4,    /* HIP failure / no gfx950 device                               */
    OIP_E_NOMEM = 5,
    OIP_E_UNSUPPORTED = 6
} oip_status;

/* reference constants (oipshared.h:27-54, imageop.h:19-20); width is a run-time argument
 * everywhere below, these are only the defaults */
#define OIP_PIXELS_PER_LINE      12288
#define OIP_MSS_BANDS            4
#define OIP_CORRELATION_LINES    16000
#define OIP_IBCV_DEF_THRESHOLD   0.4
#define OIP_IBCV_MIN_COUNT       5
#define OIP_IBCV_DEF_SECTIONS    5
#define OIP_IBCV_DEF_SLICES      10
#define OIP_IBCV_MIN_SLICES      8
#define OIP_IBPA_DEFAULT_BATCHLINES  20000
#define OIP_IBPA_DEFAULT_LINEOVERLAP 520
#define OIP_IBPA_MAX_LINEOVERLAP     3000
#define OIP_IBPA_MIN_PROCESSLINES    1500
#define OIP_STT_DEF_SECTIONS     10
#define OIP_STT_DEF_SECLINES     16000
#define OIP_STT_DEF_OVERLAPPX    200
#define OIP_STT_DEF_PHCTHRHLD    0.4
#define OIP_REMAP_ROW_GUARD      32767
#define OIP_REMAP_SECTION_ROWS   30000

/* ---- context, stream, memory ------------------------------------------------------ */
int         oip_version(void);                       /* 0x0101 == "1.1" (main.cpp:94)  */
int         oip_create(int device, oip_ctx **out);
void        oip_destroy(oip_ctx *ctx);
const char *oip_last_error(const oip_ctx *ctx);
int         oip_set_stream(oip_ctx *ctx, void *hip_stream);  /* borrow a hipStream_t (NULL: own) */
void       *oip_get_stream(oip_ctx *ctx);
int         oip_sync(oip_ctx *ctx);
int         oip_malloc(oip_ctx *ctx, void **d_ptr, size_t bytes);
int         oip_free(oip_ctx *ctx, void *d_ptr);
int         oip_memset(oip_ctx *ctx, void *d_ptr, int value, size_t bytes);
int         oip_memcpy_h2d(oip_ctx *ctx, void *d_dst, const void *src, size_t bytes);
int         oip_memcpy_d2h(oip_ctx *ctx, void *dst, const void *d_src, size_t bytes);
int         oip_host_alloc(oip_ctx *ctx, void **ptr, size_t bytes);   /* pinned staging */
int         oip_host_free(oip_ctx *ctx, void *ptr);

/* ---- RRC --------------------------------------------------------------------------- */
/* IMO::LoadRRCParamFile(path, expectedLines)  imageop.h:140-192.  kb_out receives
 * expected_lines (k,b) pairs == RRCParam[expected_lines].  No context needed. */
int oip_load_rrc_param_file(const char *path, int expected_lines, double *kb_out,
                            char *err, int errlen);

/* IMO::InplaceRRC(buff, w, h, rrcParam)  imageop.h:129-138; callers imageop.h:207,
 * preproc.h:195, :215.  dst[y*w+x] = (uint16_t)(k[x]*src[y*w+x] + b[x]) in fp64 with two
 * roundings and x86-64 truncate/wrap conversion; bit-exact.  d_dst may equal d_src
 * (in place, as the reference).  d_kb: w (k,b) pairs in HBM. */
int oip_rrc_u16(oip_ctx *ctx, const uint16_t *d_src, uint16_t *d_dst, int w, long h,
                const double *d_kb);

/* The same seam on a WINDOW: columns [0, w) of h lines of a raster of pitch src_pitch, written to a raster of pitch
 * dst_pitch (pitches in pixels; d_kb: the w (k,b) pairs of the window's columns).  With dst = the stitched raster
 * (pitch 2 (W - fold), w = W - fold) this is the left half of IMO::StitchBigRaw's output line (imageop.h:340-351)
 * taken straight from the raw CCD-1 strip: prestitch -> stitch without materialising <pan1>.RRC.RAW. */
int oip_rrc_u16_window(oip_ctx *ctx, const uint16_t *d_src, long src_pitch, uint16_t *d_dst, long dst_pitch,
                       int w, long h, const double *d_kb);

/* Host-buffer form of the same seam: `buff` is the reference's heap buffer, corrected in
 * place through pinned, double-buffered line blocks (H2D || kernel || D2H). */
int oip_rrc_u16_host(oip_ctx *ctx, uint16_t *buff, int w, long h, const double *kb);

/* ---- RRC calibration: producing the files the loader above reads -------------------- */
/* Per-column count, sum and sum of squares of a u16 raster window, ADDED into d_acc: the one pass over a strip from
 * which the coefficients that IMO::LoadRRCParamFile (imageop.h:140-192) reads are derived.
 * d_img: first pixel of the window; rows lines of w columns, `pitch` pixels apart (every line `pitch` pixels long in
 * memory, as a window of a raster is).  Only samples v with valid_min <= v <= valid_max count (0 and 65535: every sample).
 * d_acc: 3*w uint64 in HBM, planes [n | S1 | S2] of w entries each:
 *   n[x] += #valid,  S1[x] += sum v,  S2[x] += sum v*v.
 * The caller zeroes d_acc (oip_memset) before the first call; several calls over consecutive line blocks of a strip give
 * the strip's totals.  rows < 2^31 per call.  Asynchronous on the context's stream.  Sums are exact integers: the result
 * does not depend on the launch geometry or on the order of the calls.  A BIL MSS raster (preproc.h:62-75) needs no call
 * of its own: column x of its W-wide line is column x % (W/4) of band x / (W/4). */
int oip_colstats_u16(oip_ctx *ctx, const uint16_t *d_img, long pitch, int w, long rows,
                     int valid_min, int valid_max, uint64_t *d_acc);

/* Moment matching on those totals, host: one (k, b) per column such that IMO::InplaceRRC (imageop.h:129-138) with the
 * file written below -- read back by IMO::LoadRRCParamFile, imageop.h:140-192 -- brings every column's statistics to
 * its group's.  acc: the 3*w totals of oip_colstats_u16 (host copy).  The w columns form `groups` equal groups (1: PAN,
 * 4: the bands of a BIL MSS line; w % groups == 0), each fitted against its own reference.  In this order:
 *   usable(x): n >= max(min_count, 2) and D = n*S2 - S1*S1 > 0 (exact, 128-bit);  gain mode: n >= max(min_count, 1), S1 > 0
 *   mu_x = (double)S1 / (double)n,  sigma_x = sqrt((double)D) / (double)n
 *   mu_ref, sigma_ref: plain fp64 sums over the group's usable columns in ascending order, divided by their count
 *   OIP_RRCFIT_MOMENTS: k = sigma_ref / sigma_x, b = mu_ref - k * mu_x (two roundings);  OIP_RRCFIT_GAIN: k = mu_ref / mu_x, b = 0
 * kb_out: w (k,b) pairs; a column that is not usable gets (1, 0).  dead_out[g] (may be NULL): such columns of group g.
 * ref_out (may be NULL): groups x (mu_ref, sigma_ref); sigma_ref is 0 in gain mode.
 * OIP_E_RUNTIME if a group has no usable column (the message names it).  No context needed. */
#define OIP_RRCFIT_MOMENTS 0
#define OIP_RRCFIT_GAIN    1
int oip_rrc_fit_columns(const uint64_t *acc, int w, int groups, int mode, uint64_t min_count,
                        double *kb_out, int *dead_out, double *ref_out, char *err, int errlen);

/* The columns that oip_rrc_fit_columns treats as not usable (the same predicate, stated once), ascending: cols has room for
 * w entries, *n receives their number.  The list `oip despike --bad-columns` consumes.  OIP_E_INVALID for a bad argument. */
int oip_rrc_dead_columns(const uint64_t *acc, int w, int mode, uint64_t min_count, int *cols, int *n);

/* Writes RRCParam[n] in the format IMO::LoadRRCParamFile reads (imageop.h:148-188): "1\n", "<n>\n", "0\n", then n rows
 * "k , b" in %.17g (the doubles load back bit for bit), every row ended by one '\n' and nothing after the last (the
 * reader fails on a trailing blank line); a row is far shorter than the reader's 1024-byte buffer.  An existing file is
 * replaced: refusing to do so is the caller's policy (`oip rrc-calib` without --force). */
int oip_write_rrc_param_file(const char *path, const double *kb, int n, char *err, int errlen);

/* ---- quick look: an 8-bit browse image of a strip or product (`oip quicklook`; not in the reference) ------------- */
#define OIP_QUICKLOOK_SUFFIX       ".QL"   /* <stem>.QL.TIFF, built like the reference's other product names (imageop.h:99-108) */
#define OIP_QUICKLOOK_DEF_FACTOR   16
#define OIP_QUICKLOOK_DEF_CLIPLOW  2.0
#define OIP_QUICKLOOK_DEF_CLIPHIGH 98.0

/* F x F box decimation of a u16 raster window, the one pass over the full-size image.  d_src: first sample of the window;
 * rows lines of w pixels of spp samples (1, or 4 pixel-interleaved), lines `pitch` SAMPLES apart, the window inside the
 * lines of its raster (start + w * spp <= pitch).  factor F in {2, 4, 8, 16, 32, 64}.  Output: one plane per channel
 * (spp = 4 de-interleaves), ceil(w / F) x ceil(rows / F) samples, lines dst_pitch samples apart, plane c at
 * d_dst + c * dst_plane_stride (samples; ignored at spp = 1).  For each output sample, with S the exact integer sum of
 * the source samples of its channel that lie inside the image within its F x F block and n their count:
 *   q = (S + n / 2) / n          (integer division; n / 2 floored; edge blocks use their own n)
 * A strip larger than the device is cut into calls by the caller: as long as every call starts on a line that is a
 * multiple of F (and writes from output line first / F on) the result is that of one call.  Asynchronous on the context's
 * stream.  A pitch that is not a multiple of 8 samples, or a window that does not start on a 16-byte boundary, takes a
 * slower kernel with the same result. */
int oip_decimate_box_u16(oip_ctx *ctx, const uint16_t *d_src, long pitch, int w, long rows, int spp, int factor,
                         uint16_t *d_dst, long dst_pitch, size_t dst_plane_stride);

/* Histogram of a u16 raster window (rows lines of w samples, `pitch` samples apart), ADDED into d_hist: 65536 uint64 in
 * HBM, zeroed by the caller (oip_memset) before the first call.  Exact counts, additive over calls.  Asynchronous. */
int oip_histogram_u16(oip_ctx *ctx, const uint16_t *d_img, long pitch, int w, long rows, uint64_t *d_hist);

/* out[(r * w + x) * nch + c] = luts[c * 65536 + planes[c][r * pitch + x]]: nch (1 or 3) u16 planes through one 65536-entry
 * table each into an interleaved 8-bit image.  d_planes: nch device pointers -- the array itself is host memory and is read
 * during the call; d_luts (nch * 65536 bytes) and d_out (rows * w * nch bytes) are in HBM.  Asynchronous. */
int oip_apply_lut_u8(oip_ctx *ctx, const uint16_t *const *d_planes, long pitch, int w, long rows, int nch,
                     const uint8_t *d_luts, uint8_t *d_out);

/* Percentile limits of a histogram, host.  hist: 65536 counts.  N = number of samples with valid_min <= v <= valid_max;
 * for p in (p_lo, p_hi):  r = min(N - 1, (uint64_t)floor((double)N * p / 100.0))  and the limit is the value at sorted
 * index r among the valid samples, i.e. the smallest v whose cumulative count (from valid_min) exceeds r.
 * N == 0: *lo = *hi = 0.  *n_valid (may be NULL) = N.  OIP_E_INVALID unless 0 <= p_lo <= p_hi <= 100 and
 * 0 <= valid_min <= valid_max <= 65535.  No context needed. */
int oip_stretch_limits(const uint64_t *hist, int valid_min, int valid_max, double p_lo, double p_hi,
                       int *lo, int *hi, uint64_t *n_valid);

/* The linear stretch lo..hi -> 0..255 as a table, host: with span = hi - lo > 0
 *   lut[v] = ((clamp(v, lo, hi) - lo) * 510 + span) / (2 * span)      (integers: round half up of 255 (v - lo) / span)
 * and with span == 0: lut[v] = v < lo ? 0 : 255.  lut: 65536 bytes.  OIP_E_INVALID unless 0 <= lo <= hi <= 65535. */
int oip_stretch_lut_u8(int lo, int hi, uint8_t *lut);

/* An 8-bit baseline TIFF (classic, little-endian, uncompressed strips, chunky): spp 1 (BlackIsZero) or 3 (RGB), data =
 * height x width x spp bytes.  An existing file is replaced.  OIP_E_INVALID for geometry it cannot hold (4 GiB),
 * OIP_E_IO when the file cannot be written. */
int oip_write_tiff_u8(const char *path, const uint8_t *data, int width, long height, int spp, char *err, int errlen);

/* ---- raster I/O staging (imageop.h:43-127, stitcher.h:103-120) ---------------------------------------
 * IMO::ReadFileContent + LoadRawImage / WriteBufferToFile move a raster through one pageable heap buffer,
 * serially with the arithmetic (8 MiB fread / fwrite units on the calling thread, imageop.h:69-79, :88-95).
 * These entry points move it in 32 MiB blocks through a ring of pinned buffers on a staging stream of the
 * context's own -- a slot is filled from the file by parallel pread on the host copy pool -- so disk, host
 * copies, PCIe and the kernels of the compute stream overlap.  Staging calls may run on other host threads
 * while the first drives kernels through the same context: they use streams and pinned slots of their own,
 * set the context's device for the calling thread, and never touch the compute stream's state.  Calls of one
 * lane serialise on a lock (ring lane: read_file / upload_staged / rrc_u16_host; download lane:
 * download_staged[_after] / write_file[_at] / file_sink_write: three of them, a call takes a free one), ring and download
 * lanes run concurrently (full duplex): a reader thread,
 * the compute thread and a writer thread form the pipeline of the `oip` CLI's default action.
 * Ordering: downloads and file writes start after the compute-stream work enqueued before the call, or after
 * a MARK of the compute stream (oip_compute_mark) when one is given; UPLOADS DO NOT wait for the compute
 * stream -- before re-uploading into a buffer that queued kernels still read, call
 * oip_stage_order_after_compute(ctx) (or upload elsewhere).
 *   ticket != NULL : the call returns once the last block's DMA is ENQUEUED and *ticket identifies it;
 *                    oip_stage_wait(ctx, t) makes the compute stream wait (on the device) for everything up
 *                    to t.  ticket == NULL: the compute stream is ordered behind the transfer by the call itself.
 *   downloads start after the compute-stream work enqueued before the call and return when the host side
 *   (file or buffer) is complete. */
/* ReadFileContent(filePath, size, offset, total, buff) with `buff` in HBM; bytes == 0: to the end of the file */
int oip_read_file_to_device(oip_ctx *ctx, const char *path, size_t offset, size_t bytes, void *d_dst,
                            size_t *bytes_read, long *ticket);
/* WriteBufferToFile(buff, size, saveFilePath) with `buff` in HBM (append != 0: "ab", as the section writes of
 * stitcher.h:114-120 accumulate one output file) */
int oip_write_device_to_file(oip_ctx *ctx, const void *d_src, size_t bytes, const char *path, int append);
/* the same into an EXISTING or new file at byte `file_offset` without truncating it (the file grows as needed): a product
 * written block by block as its lines become final -- <pan>.RRC.RAW while the strip is still being read, the pixel payload
 * of an uncompressed TIFF (oip_tiff.hpp) behind its header.  mark: 0, or a mark of the compute stream to wait for. */
int oip_write_device_to_file_at(oip_ctx *ctx, const void *d_src, size_t bytes, const char *path, size_t file_offset, long mark);
/* A product file PREPARED ahead of its pixels: created, its blocks reserved (a full file system fails at open, cleanly) and
 * mapped -- by a thread that has time for it, e.g. while the strip is still being read -- so that the later write is
 * HBM -> pinned slot -> parallel memory copies into pages that exist (on page-cache-backed files several
 * times the rate of allocating them during the write, which is what bounds WriteBufferToFile's loop, imageop.h:84-97).
 * The file is not truncated: a header written before stays.  bytes: the final size of the file.  A sink whose reservation or
 * mapping failed (or OIP_FILE_WRITE=pwrite) writes through pwrite.  mark as oip_write_device_to_file_at. */
typedef struct oip_file_sink oip_file_sink;
int oip_file_sink_open(oip_ctx *ctx, const char *path, size_t bytes, oip_file_sink **out);
int oip_file_sink_write(oip_ctx *ctx, oip_file_sink *sink, size_t file_offset, const void *d_src, size_t bytes, long mark);
int oip_file_sink_close(oip_ctx *ctx, oip_file_sink *sink);
/* A MARK names the compute-stream work enqueued so far (an event from a ring of 64; taken by the compute thread, e.g. right
 * after the RRC kernel of a line block).  A download-lane transfer given the mark starts once that work is done, not after
 * what the compute thread enqueued later (a 12-ms correlation batch, say).  A mark that has left the ring means "everything
 * enqueued so far". */
int oip_compute_mark(oip_ctx *ctx, long *mark);
int oip_compute_mark_sync(oip_ctx *ctx, long mark);   /* the calling host thread waits for the mark */
/* the same between a pageable host buffer and HBM (copies to/from the pinned ring run on a thread pool) */
int oip_upload_staged(oip_ctx *ctx, void *d_dst, const void *host, size_t bytes, long *ticket);
/* the same for a 2-D block (a column block of a raster): `rows` rows of `width` bytes; host rows src_pitch bytes apart,
 * device rows dst_pitch bytes apart; width at most 32 MiB */
int oip_upload_staged_2d(oip_ctx *ctx, void *d_dst, size_t dst_pitch, const void *host, size_t src_pitch, size_t width,
                         size_t rows, long *ticket);
int oip_download_staged(oip_ctx *ctx, void *host, const void *d_src, size_t bytes);
int oip_download_staged_after(oip_ctx *ctx, void *host, const void *d_src, size_t bytes, long mark);
int oip_stage_wait(oip_ctx *ctx, long ticket);
int oip_stage_sync(oip_ctx *ctx);
int oip_stage_order_after_compute(oip_ctx *ctx);      /* the ring lane's later transfers wait for the compute stream's work enqueued so far */
int oip_stage_threads(void);                          /* threads of the host copy pool (OIP_HOST_COPY_THREADS) */
/* where the host side of the upload lane spent its time since the last reset: out[0] seconds in pageable -> pinned copies,
 * out[1] seconds waiting for a ring slot whose DMA had not finished (the link is the limit then), out[2] bytes, out[3] calls */
int oip_stage_stats(oip_ctx *ctx, double *out, int reset);

/* PreProcessor::LoadMSS split (preproc.h:62-75) fused with DoRRC4MSS (preproc.h:202-222):
 * one pass over the BIL MSS raster (each line = 4 bands x w/4 px) writing 4 planar,
 * RRC-corrected bands (band b at d_planes + b*plane_stride).  d_kb4: 4 x (w/4) (k,b)
 * pairs, band-major; NULL = split only (--no-rrc4mss). */
int oip_mss_split_rrc_u16(oip_ctx *ctx, const uint16_t *d_bil, uint16_t *d_planes,
                          size_t plane_stride, int w, long lines, const double *d_kb4);

/* ---- correlation ------------------------------------------------------------------- */
/* cv::phaseCorrelate(src1, src2, noArray(), &response)  call sites stitcher.h:180,
 * preproc.h:316.  d_a/d_b: continuous rows x cols f32.  Synchronises; host outputs. */
int oip_phase_correlate_f32(oip_ctx *ctx, const float *d_a, const float *d_b, int rows,
                            int cols, double *dx, double *dy, double *response);

/* Mat1w.colRange -> Mat1f conversion (stitcher.h:175-176, preproc.h:258-293) */
int oip_window_u16_to_f32(oip_ctx *ctx, const uint16_t *d_img, size_t pitch, long row0,
                          int col0, int rows, int cols, float *d_out);

/* cv::resize(f32, dsize, 0, 0, INTER_CUBIC)  call site preproc.h:302-307 */
int oip_resize_cubic_f32(oip_ctx *ctx, const float *d_src, int sw, int sh, float *d_dst,
                         int dw, int dh);

/* Loop body of Stitcher::CalcSttParameters (stitcher.h:166-191) for all sections:
 * out[s*3 + {0,1,2}] = dx, dy, response of section s (host).  d_pan1/d_pan2 hold global
 * lines [row0, row0+nrows) of the W-wide rasters of L lines; sections not fully inside
 * that range are skipped and reported as NaN (multi-GPU: each rank computes the sections
 * it owns, results are all-gathered). */
int oip_stt_correlate(oip_ctx *ctx, const uint16_t *d_pan1, const uint16_t *d_pan2, int W,
                      long L, long row0, long nrows, int sections, int lines_per_section,
                      int overlap_cols, int edge_cols, double *out);

/* The same loop body for n explicit window pairs (multi-GPU: a section whose lines live on several ranks
 * is gathered into compact windows on the rank that computes it): window i of CCD 1 / CCD 2 is rows x cols
 * u16 at d_a[i] / d_b[i] with row pitch pitch_a[i] / pitch_b[i] (elements) -- the Mat1w.colRange views of
 * stitcher.h:175-176.  out[3*i + {0,1,2}] = dx, dy, response.  The pointer arrays are host arrays of
 * device pointers. */
int oip_stt_correlate_windows(oip_ctx *ctx, const uint16_t *const *d_a, const size_t *pitch_a,
                              const uint16_t *const *d_b, const size_t *pitch_b, int n, int rows, int cols,
                              double *out);

/* Loop body of PreProcessor::CalcInterBandCorrelation (preproc.h:251-329):
 * out[((b*sections + sec)*slices + i)*4 + {0..3}] = dx, dy, rs, cx.  PAN lines
 * [prow0, prow0+pn) and MSS band lines [mrow0, mrow0+mn) are resident; sections not fully
 * inside are reported as NaN.
 * cv::resize(INTER_CUBIC) of the band window (preproc.h:302-307) followed by the transform of the up-sampled
 * image is computed, for slices of 3000 columns whose window is exactly 4 x the band window, as the transform of
 * the band window itself expanded by the up-sampling operator's own transform (an exact identity, see DESIGN.md
 * 4.3); results agree with "up-sample, then transform" to ~4e-6 px.  Environment: OIP_SPECTRAL_UP=0 keeps the
 * up-sampling in the image domain (1: horizontal axis only on the spectra).  Every correlation entry reads its switches
 * once, at its top; oip_corr_route_describe states the route they give a geometry. */
int oip_interband_correlate(oip_ctx *ctx, const uint16_t *d_pan, long Lp, long prow0, long pn,
                            const uint16_t *d_planes, size_t plane_stride, long mrow0, long mn,
                            int W, int slices, int sections, int corr_lines, double *out);

/* The (section, slice) body of the same loop (preproc.h:262-329) for n explicit units: unit u is a PAN
 * window of rows x cols u16 at d_pan[u] (pitch pan_pitch[u]) and the four band windows of (rows/4) x
 * (cols/4) u16 at d_bands[4*u + b] (pitch band_pitch[u]).  out[12*u + 3*b + {0,1,2}] = dx, dy, rs of band
 * b.  Lets a multi-GPU host hand any unit to any rank (a unit needs 96 MB + 4 x 6 MB of windows at the
 * 30000-wide geometry).  Units are processed two at a time (2u, 2u+1 share transforms), so the last
 * digits of a unit's result (~1e-6 px) depend on its partner: a host that wants the bits of the
 * single-GPU run keeps the pairs of oip_interband_correlate's order (section-major, slices in order). */
int oip_interband_correlate_units(oip_ctx *ctx, const uint16_t *const *d_pan, const size_t *pan_pitch,
                                  const uint16_t *const *d_bands, const size_t *band_pitch, int n, int rows,
                                  int cols, double *out);

/* The spectral route's peak search transforms only the lane tiles (16 or 32 columns) of a correlation surface whose
 * column bound admits a maximum; OIP_PEAK_PRUNE=0 in the environment, read per call, searches all of
 * them through the same kernels.  This returns how many tiles were searched and how many there were, summed over the
 * output arrays of every correlation since the previous call, and starts the count again (either pointer may be
 * null).  Waits for the context's stream. */
int oip_peak_prune_stats(oip_ctx *ctx, long long *tiles_searched, long long *tiles_total);

/* The row stage of that route stores only the columns the pruned search reads: the lane tiles 0 .. R and T - R .. T - 1
 * of the T tiles of the column passes, a circular window around column 0, where the surfaces of inter-band shifts of a
 * few pixels peak.  R = OIP_ROWS_WINDOW in the environment, read per call (default 8; 0 stores every
 * column, and so do OIP_PEAK_PRUNE=0 and plans without tile lists).  A pair of units whose search lists a tile outside
 * the window is detected on the device and run again inside the same call with every column stored: results have
 * the same bits either way.  OIP_ROWS_WINDOW_POISON=1 (debug) fills the output arrays with NaN before the row stage.
 * oip_rows_window_stats returns how many pairs (or single units) went through the windowed row stage and how many of
 * them were run again, since the previous call, and starts the count again; oip_rows_window_geometry returns the tile
 * width in columns, T and R (-1: every column stored) of the latest correlation call.  Any pointer may be null. */
int oip_rows_window_stats(oip_ctx *ctx, long long *pairs, long long *pairs_rerun);
int oip_rows_window_geometry(oip_ctx *ctx, int *tile_cols, int *tiles, int *radius);

/* The x4 cubic up-sampling of cv::resize (preproc.h:302-307) along one axis as an operator on spectra -- what
 * oip_interband_correlate applies to the transforms of the band windows instead of transforming the up-sampled
 * image.  Host only.  out: 5 x (4 n) complex floats, rows H, G_0 .. G_3:
 *   DFT_4n(up-sampled s)[k] = H[k] DFT_n(s)[k mod n] + sum_j G_j[k] s[J_j],   J = {0, 1, n-2, n-1}.
 * OIP_E_UNSUPPORTED for n < 8. */
int oip_upsample_operator(int n, float *out);

/* The plan of the 2-D FFT engine for an M x N transform (rows x columns, each 2^a 3^b 5^c), as its planner makes it for
 * every correlation of that size.  Host only: no context, no device.  buf receives one line per pass, in forward order
 * (column passes, then row passes):
 *   axis=<y|x> F=<factor> mode=<0|1> kind=<ct|generic> vshift=<log2 V> Vp=<LDS pitch> radix=<r,r,..> lds=<bytes>
 * kind ct: a kernel specialised for (F, mode); generic: the run-time kernel, V = 1 << vshift transforms per tile.  lds:
 * the dynamic LDS of a generic launch; the tile and twiddle arrays (an upper bound) of a specialised kernel.
 * Where the planner or the launcher refuses the size, the code of the refusal is returned (OIP_E_INVALID, OIP_E_UNSUPPORTED,
 * OIP_E_RUNTIME) and buf holds its text; OIP_E_INVALID with an empty buf: null buf or len too short for the lines. */
int oip_fft_plan_describe(int M, int N, char *buf, int len);

/* The plan of an inter-band correlation call on units of rows x cols PAN lines (band windows rows / 4 x cols / 4, as
 * oip_interband_correlate_units derives them) on a device of cu_count CUs, with the switches of the environment as a call
 * would read them (OIP_SPECTRAL_UP, OIP_SPECTRAL_V, OIP_FUSED_ROWS, OIP_PEAK_PRUNE, OIP_ROWS_WINDOW; csrc/oip_corrroute.h:
 * CorrKnobs).  Host only: no context, no device.  buf receives one JSON object: "route" ("image", "H", "HV", "V": DESIGN.md
 * 4.3), the window, band and DFT sizes, "row_kernel" and "pack_kernel" (the profile names of the route's row stage and of
 * what brings the bands into its arrays), the peak search's "groups", "tiles", "tile_cols" and "lists", "window" (the row
 * stage's stored radius, -1: every column), and the workspace: "total" bytes, "regions" (name, offset, bytes of a part,
 * count of parts, in address order) and the arrays "inside" a part of one.  Where the planner refuses the geometry its code
 * is returned and buf holds {"refused": text, "code": code}; OIP_E_INVALID with an empty buf: bad argument or len too short. */
int oip_corr_route_describe(int rows, int cols, int cu_count, char *buf, int len);

/* The validity filter and means of Stitcher::CalcSttParameters (stitcher.h:181-198), host: table[3*s +
 * {0,1,2}] = dx, dy, response of section s, in section order.  OIP_E_RUNTIME when no section is valid
 * ("No valid delta value found for stitching parameter calculating"). */
int oip_stt_mean(const double *table, int sections, double threshold, double max_delta_y, double *dx,
                 double *dy, double *response, int *valid);

/* FilterInterBandShiftValues + DoCorrelationPolynomialFitting (preproc.h:492-550), host.
 * shifts: [4][n][4] (dx,dy,rs,cx).  cx_out[4][2], cy_out[4][3] ascending coefficients.
 * oip_filter_and_fit fits like the reference (OIP_FIT_REFERENCE). */
#define OIP_FIT_REFERENCE 0  /* NumCpp Poly1d::fit as called at preproc.h:535-536: inv(A^T A) A^T y, raw abscissa */
#define OIP_FIT_LSTSQ     1  /* the same least-squares problem by Householder QR on a scaled abscissa       */
int oip_filter_and_fit(const double *shifts, int n, double threshold, int min_count,
                       double *cx_out, double *cy_out, char *err, int errlen);
int oip_filter_and_fit_mode(const double *shifts, int n, double threshold, int min_count, int fit_mode,
                            double *cx_out, double *cy_out, char *err, int errlen);
/* nc::polynomial::Poly1d<double>::fit(x, y, deg), ascending coefficients: the reference's operation
 * order (oip_polyfit_reference) and the well-conditioned solver (oip_polyfit) */
int oip_polyfit_reference(const double *x, const double *y, int n, int deg, double *coeffs);
int oip_polyfit(const double *x, const double *y, int n, int deg, double *coeffs);

/* ---- resampling -------------------------------------------------------------------- */
/* Stitcher::PreStitch (stitcher.h:83-139) + IMO::SectionaryRemap (imageop.h:230-275) +
 * cv::remap(INTER_CUBIC, BORDER_CONSTANT) (imageop.h:258): out(x,y) = bicubic(src, x+dx,
 * y+dy) with OpenCV's 1/32-px quantisation, per-section borders and cuts.  The float maps
 * are never materialised.  d_src holds global lines [src_row0, src_row0+src_rows) and
 * d_dst receives output lines [out_row0, out_row0+out_rows) of the W x L raster (whole
 * strip: 0, L, 0, L).  OIP_E_INVALID if L <= row_guard (imageop.h:242-244). */
int oip_remap_shift_bicubic_u16(oip_ctx *ctx, const uint16_t *d_src, long src_row0,
                                long src_rows, uint16_t *d_dst, long out_row0, long out_rows,
                                int W, long L, double dx, double dy, int section_rows,
                                int row_guard);
/* The same call with the 16-tap sums of the regular interior pixels accumulated in packed fp16 (BASELINE
 * config 5: "fp16 accumulate (tolerance stated)").  NOT the parity mode: |result - fp32 result| <= 6 DN on
 * 12-bit data (measured: max 5, mean 0.25 DN, 20-25 % of the pixels differ), <= 6 + max|sample - 2048|/64
 * DN in general; samples enter as (sample - 2048), so the mode is specified for data up to 15 bits.
 * Geometry, 1/32-px phases, section borders and the irregular columns are identical (and computed in
 * f32); widths that are not a multiple of 8 fall back to the fp32 kernel altogether. */
int oip_remap_shift_bicubic_u16_f16acc(oip_ctx *ctx, const uint16_t *d_src, long src_row0,
                                       long src_rows, uint16_t *d_dst, long out_row0, long out_rows,
                                       int W, long L, double dx, double dy, int section_rows,
                                       int row_guard);
/* The same resampling written into a WINDOW of another raster: column x >= dst_col0 of output line r goes to
 * d_dst[r * dst_pitch + dst_col_off + (x - dst_col0)], columns below dst_col0 are not stored (d_dst: first output line
 * of the destination raster, dst_pitch in pixels).  With dst_pitch = 2 (W - fold), dst_col0 = fold, dst_col_off = W - fold
 * the resampled CCD-2 line lands in the right half of IMO::StitchBigRaw's output line (imageop.h:340-351): prestitch ->
 * stitch without materialising .RRC.PRESTT.RAW (the fused single-pass pipeline of DOC/sample-task.sh; `oip task`).
 * f16acc != 0 selects the fp16-accumulate variant.  Pixels are those of the two plain calls, bit for bit. */
int oip_remap_shift_bicubic_u16_window(oip_ctx *ctx, const uint16_t *d_src, long src_row0, long src_rows,
                                       uint16_t *d_dst, long dst_pitch, int dst_col0, long dst_col_off,
                                       long out_row0, long out_rows, int W, long L, double dx, double dy,
                                       int section_rows, int row_guard, int f16acc);
/* The same with the source being the RAW CCD-2 strip: every sample is corrected on load (IMO::InplaceRRC's pixel, exact;
 * d_kb: the W (k,b) pairs in HBM), so Stitcher::DoRRC of CCD 2, PreStitch and the right half of StitchBigRaw are ONE pass
 * over the strip and <pan2>.RRC.RAW is not materialised either.  Bits are those of oip_rrc_u16 followed by
 * oip_remap_shift_bicubic_u16_window with the same f16acc (f16acc != 0 needs W % 8 == 0 and a 16-byte aligned source:
 * OIP_E_UNSUPPORTED otherwise). */
int oip_remap_shift_rrc_bicubic_u16_window(oip_ctx *ctx, const uint16_t *d_src_raw, long src_row0, long src_rows,
                                           const double *d_kb, uint16_t *d_dst, long dst_pitch, int dst_col0,
                                           long dst_col_off, long out_row0, long out_rows, int W, long L, double dx,
                                           double dy, int section_rows, int row_guard, int f16acc);
/* source lines [first, last) that output lines [out_row0, out_row0+out_rows) read: the halo
 * a row-block shard has to hold (host arithmetic only) */
int oip_remap_shift_src_range(long out_row0, long out_rows, long L, double dy,
                              int section_rows, long *first, long *last);

/* PreProcessor::DoInterBandAlignment outer (preproc.h:351-425) + inner (:428-468) incl.
 * cv::remap and cv::merge: 4 planar bands -> interleaved 16UC4, polynomial maps evaluated
 * in fp64 in the kernel.  cx[4][2], cy[4][3] host.  d_planes holds MSS lines [src_row0,
 * src_row0+src_rows); d_dst receives output lines [out_row0, out_row0+out_rows) of the
 * (Lm - line_offset - (keep?0:overlap)) x Wb x 4 result; skipped tail lines are zero.
 * rows_valid (may be NULL): the reference's processedLines. */
int oip_align_mss_bicubic_u16x4(oip_ctx *ctx, const uint16_t *d_planes, size_t plane_stride,
                                long src_row0, long src_rows, uint16_t *d_dst, long out_row0,
                                long out_rows, int Wb, long Lm, const double *cx,
                                const double *cy, int lines_per_section, int line_offset,
                                int overlap, int keep_leading, int min_lines, long *rows_valid);
int oip_align_mss_src_range(long out_row0, long out_rows, long Lm, const double *cy, int Wb,
                            int lines_per_section, int line_offset, int overlap,
                            int keep_leading, int min_lines, long *first, long *last);

/* IMO::StitchBigRaw line loop (imageop.h:340-351), RAW output: out line = left[0:W-fold] ||
 * right[fold:W]; `fold` is the already-halved value (main.cpp:189). */
int oip_stitch_rows_u16(oip_ctx *ctx, const uint16_t *d_left, const uint16_t *d_right,
                        uint16_t *d_out, int W, long L, int fold);

/* In-place sample permutation of an interleaved 4-channel u16 image: sample i of every pixel becomes the former sample
 * order[i].  cv::imwrite stores a 4-channel Mat (c0,c1,c2,c3) as samples (c2,c1,c0,c3) (preproc.h:167-185 WriteAlignedMSS_TIFF;
 * imageop.h:390-402), GDAL writes band b from channel bandMap[b]-1 (imageop.h:529): with the image already in file order on the
 * device, its lines go from HBM into the TIFF's pixel payload without a host pass.  d_img 16-byte aligned. */
int oip_permute_u16x4(oip_ctx *ctx, uint16_t *d_img, size_t npixels, const int *order);

/* ---- seam balancing and feathering of the stitch (`oip stitch --balance / --feather`; not in the reference) --------
 * IMO::StitchBigRaw cuts hard at the seam, and the two CCDs are calibrated apart (oip_rrc_fit_columns matches a strip to
 * itself), so a level difference between them is a step through every product.  After prestitch the last 2*fold columns
 * of image 1 and the first 2*fold columns of image 2 see the same ground: that overlap gives image 2's gain and offset
 * relative to image 1, and room to blend the two.
 * Lines are in SAMPLE units, as for the 4-sample TIFF stitch: spp samples per pixel (1 or 4, pixel-interleaved),
 * Ws = W * spp samples per input line, fs = fold * spp (fold: the halved --fold-cols); the channel of sample j is j % spp.
 * An overlap pair of line r is  a = left[r * Ws + Ws - 2 fs + j],  b = right[r * Ws + j],  j in [0, 2 fs). */

/* Per channel c the totals over the pairs of L lines whose TWO samples lie in [valid_min, valid_max], ADDED into d_acc:
 * (6, spp) uint64 in HBM, planes  n | Sa = sum a | Sb = sum b | Saa = sum a*a | Sbb = sum b*b | Sab = sum a*b,  entry
 * [k * spp + c].  The caller zeroes d_acc (oip_memset) before the first call; calls over consecutive line blocks add up to
 * the strip's totals.  Sums are exact integers: they do not depend on the launch geometry or the order of the calls, as
 * long as one channel sees at most 2^32 pairs in all (2 * fold * L <= 2^32: then Sab <= 2^32 * 65535^2 < 2^64; a single
 * call beyond that is OIP_E_INVALID).  2 fs <= Ws, L < 2^31.  The windows may start on any 2-byte boundary.  Asynchronous. */
int oip_seam_moments_u16(oip_ctx *ctx, const uint16_t *d_left, const uint16_t *d_right, int Ws, long L, int fs, int spp,
                         int valid_min, int valid_max, uint64_t *d_acc);

/* Gain and offset of image 2 relative to image 1 from those totals, host.  acc: the 6 * spp totals (host copy).  Per
 * channel, in this order, every step one correctly rounded fp64 operation (integers below 2^53 convert exactly, the
 * 128-bit ones to the nearest double):
 *   Da = n * Saa - Sa * Sa,  Db = n * Sbb - Sb * Sb,  Dab = n * Sab - Sa * Sb              exact 128-bit integers
 *   mean_a = (double)Sa / (double)n,  mean_b = (double)Sb / (double)n
 *   ra = sqrt((double)Da),  rb = sqrt((double)Db),  sigma_a = ra / (double)n,  sigma_b = rb / (double)n
 *   r = (double)Dab / (ra * rb)                                   (0 when Da or Db is 0; everything is 0 when n is 0)
 *   OIP_SEAM_MOMENTS: g = sqrt((double)Da / (double)Db);  OIP_SEAM_GAIN: g = (double)Sa / (double)Sb;  OIP_SEAM_OFFSET: g = 1
 *   G = rint(g * 65536)
 *   O = rint((mean_a - (G / 65536) * mean_b) * 65536)             from the QUANTISED gain, so that the means still meet
 *                                                                 after quantisation; OIP_SEAM_GAIN: O = 0
 * A channel gets the identity (G = 65536, O = 0) and identity[c] = 1 -- not an error, like a dead column of the RRC fit --
 * when n < max(min_count, 2), when Da or Db is 0 in moments mode, or when Sb is 0 in gain mode.
 * gain_q16 / offset_q16 / identity: spp entries each.  report (may be NULL): spp x (n, mean_a, mean_b, sigma_a, sigma_b, r);
 * r is the number that tells whether fold matches the real overlap.
 * OIP_E_INVALID, with the channel and the value in err, for a G outside [16384, 262144] (a quarter to four: the images
 * do not show the same ground, usually a wrong --fold-cols) or an O that does not fit 32 bits.  No context needed. */
#define OIP_SEAM_MOMENTS 0
#define OIP_SEAM_GAIN    1
#define OIP_SEAM_OFFSET  2
int oip_seam_fit(const uint64_t *acc, int spp, int mode, uint64_t min_count, int32_t *gain_q16, int32_t *offset_q16,
                 double *report, int *identity, char *err, int errlen);

/* oip_stitch_rows_u16 with image 2 balanced, a blend zone around the seam and "no data" inside it: the one pass over the
 * full-size product.  d_out: L lines of 2 (Ws - fs) samples.  d_gain_q16 / d_offset_q16: spp int32 each in HBM (G_c, O_c).
 * In integers, for output pixel column p of line r, channel c, with s = W - fold (the seam) and h = feather (half-width of
 * the blend zone in pixels, 0 <= h <= fold; above 16384: OIP_E_UNSUPPORTED):
 *   a  = left[r][p],  b = right[r][p - (W - 2 fold)]
 *   b' = clamp((G_c * b + O_c + 32768) >> 16, 0, 65535)           64-bit, arithmetic shift
 *   p <  s - h: a          p >= s + h: b'
 *   otherwise, with t = p - (s - h), wr = 2 t + 1, wl = 4 h - wr:   (wl * a + wr * b' + 2 h) / (4 h), floored;
 *              b' instead if a < valid_min, else a instead if b < valid_min
 * With G = 65536, O = 0, h = 0 the output is oip_stitch_rows_u16's, byte for byte.  An output line that is not a multiple
 * of 8 samples, or bases that are not 16-byte (out) / 4-byte (in) aligned, take a slower kernel with the same result.
 * Asynchronous on the context's stream. */
int oip_stitch_balanced_u16(oip_ctx *ctx, const uint16_t *d_left, const uint16_t *d_right, uint16_t *d_out, int Ws, long L,
                            int fs, int spp, const int32_t *d_gain_q16, const int32_t *d_offset_q16, int feather,
                            int valid_min);

/* -- gains that follow the strip (`oip stitch --balance-lines B`).  Over 100 000 lines illumination, stray light and the two
 * detectors' temperatures drift apart: one (G, O) meets the means of the whole overlap and leaves a step at the ends.  The
 * strip is cut into nb = max(1, L / B) blocks of B = block_lines >= 1 lines (integer division): block k < nb - 1 covers lines
 * [k B, (k + 1) B), the last one [(nb - 1) B, L) -- a short tail is merged into it, so it holds B .. 2B - 1 lines, or all L
 * lines when L < B.  Each block is fitted, the fits are nodes at the blocks' nominal centres, and every line gets the
 * linear interpolation of its two nodes.  All of it in exact integers or correctly rounded fp64, like the block above. */

/* oip_seam_moments_u16 per block, in ONE launch: d_acc is (nb, 6, spp) uint64, entry [(k * 6 + m) * spp + c], and the six
 * totals of block k are ADDED into plane k (the caller zeroes the array).  Same arguments, checks and limit (2 * fold * L <=
 * 2^32 per call) plus block_lines >= 1; the planes summed over k equal what oip_seam_moments_u16 adds for the same lines,
 * exactly, and no total depends on the launch geometry.  Asynchronous. */
int oip_seam_moments_blocks_u16(oip_ctx *ctx, const uint16_t *d_left, const uint16_t *d_right, int Ws, long L, int fs, int spp,
                                int valid_min, int valid_max, long block_lines, uint64_t *d_acc);

/* The fits of those totals, host.  acc: nb * 6 * spp totals (host copy).
 *   1. (G0_c, O0_c, identity0_c) = oip_seam_fit of the planes' sum.  Its errors (a gain outside [16384, 262144], an offset
 *      that does not fit 32 bits) are this function's, with the same text and OIP_E_INVALID.
 *   2. oip_seam_fit's arithmetic on the totals of each block k, channel c.  Where that would give the identity (fewer than
 *      max(min_count, 2) pairs, Da or Db 0 in moments mode, Sb 0 in gain mode), a gain outside [16384, 262144] or an offset
 *      that does not fit 32 bits, the block channel takes (G0_c, O0_c) and substituted[k * spp + c] = 1: never an error --
 *      the zero-filled line blocks of the de-framer, water and cloud are such blocks.
 * gain_q16 / offset_q16 / substituted: nb * spp entries, [k * spp + c].  gain0_q16 / offset0_q16 / identity0: spp entries.
 * report (may be NULL): nb * spp * 6 doubles, block k's spp x 6 at report + k * spp * 6 as oip_seam_fit lays out its own
 * (the block's own statistics, substituted or not).  No context needed. */
int oip_seam_fit_blocks(const uint64_t *acc, long nb, int spp, int mode, uint64_t min_count, int32_t *gain_q16,
                        int32_t *offset_q16, int *substituted, int32_t *gain0_q16, int32_t *offset0_q16, int *identity0,
                        double *report, char *err, int errlen);

/* The nodes as per-line tables, host: line_gain_q16 / line_offset_q16 are L * spp int32, entry [r * spp + c].  Node k sits at
 * line y_k = k B + floor(B / 2).  For line r and either quantity V:
 *   u = r - floor(B / 2),  k = clamp(floor(u / B), 0, max(nb - 2, 0)),  t = clamp(u - k B, 0, B),  k' = min(k + 1, nb - 1)
 *   V(r) = floor((V_k * (B - t) + V_k' * t + floor(B / 2)) / B)       64-bit, the floor toward minus infinity
 * Constant before the first node and after the last, constant for nb = 1, and never outside the interval of its two
 * nodes.  nb must be max(1, L / B); L = 0 writes nothing.  OIP_E_INVALID otherwise.  No context needed. */
int oip_seam_line_tables(const int32_t *gain_q16, const int32_t *offset_q16, long nb, int spp, long L, long block_lines,
                         int32_t *line_gain_q16, int32_t *line_offset_q16);

/* oip_stitch_balanced_u16 with one change: d_line_gain_q16 / d_line_offset_q16 are the per-line tables, L * spp int32 each
 * in HBM, and line r, channel c uses G[r * spp + c], O[r * spp + c].  b', the blend, the no-data rule, the h <= 16384 limit
 * and the slower kernel for lines that are not a multiple of 8 samples or misaligned bases (here also: 4-sample tables that
 * are not 16-byte aligned) are as stated there.  Output samples left of the blend zone are copies and read no table entry.
 * Tables that repeat one (G, O) on every line give oip_stitch_balanced_u16's bytes; the identity with h = 0 gives
 * oip_stitch_rows_u16's.  Asynchronous on the context's stream. */
int oip_stitch_balanced_lines_u16(oip_ctx *ctx, const uint16_t *d_left, const uint16_t *d_right, uint16_t *d_out, int Ws, long L,
                                  int fs, int spp, const int32_t *d_line_gain_q16, const int32_t *d_line_offset_q16,
                                  int feather, int valid_min);

/* ---- MTF compensation: a fixed-point restoration filter (`oip mtfc`; not in the reference) -------------------------
 * CCD 2 goes through a bicubic resampling in prestitch and every MSS band through one in the aligner; CCD 1 goes through
 * none, so the halves of a stitched product differ in sharpness.  MTFC is the small convolution that level-1 chains apply
 * behind the radiometric correction.  Specified in exact integers: any evaluation order gives the same bytes. */
#define OIP_MTFC_SUFFIX        ".MTFC"  /* <stem>.MTFC.<ext>, built like the reference's other product names (imageop.h:99-108) */
#define OIP_MTFC_DEF_MAXGAIN   2.0
#define OIP_CONVOLVE_MAX_K     9

/* The raster is W pixels x L lines of spp samples (1, or 4 pixel-interleaved); lines are W * spp samples apart and the
 * channel of sample j is j % spp.  d_src holds global lines [src_row0, src_row0 + src_rows) and d_dst receives output lines
 * [out_row0, out_row0 + out_rows), the first at d_dst (oip_remap_shift_bicubic_u16's convention: a strip cut into calls
 * gives the bytes of one call).  taps: HOST array of ky * kx Q12 integers, row-major; ky, kx odd in 1..9; ry = ky / 2,
 * rx = kx / 2.  For output line y, pixel x, channel c, all in integers:
 *   s(v, u) = src[clamp(v, 0, L-1)][clamp(u, 0, W-1)][c]                replicate at the image border
 *   ctr = s(y, x)
 *   ctr < valid_min:  out = ctr                                         no data passes through
 *   otherwise:        n(j, i) = s(y + j - ry, x + i - rx),  n'(j, i) = n(j, i) < valid_min ? ctr : n(j, i)
 *                     acc = sum_{j,i} taps[j * kx + i] * n'(j, i)       correlation form, as cv::filter2D
 *                     out = clamp((acc + 2048) >> 12, valid_min, 65535) arithmetic shift (floor)
 * Clamping at valid_min keeps data from becoming no data; replacing no-data neighbours by the centre keeps the black
 * borders of prestitch and the aligner from ringing into the image.
 * OIP_E_INVALID: sum |taps| > 32767 -- the bound that makes acc + 2048 fit int32: 32767 * 65535 + 2048 = 2 147 387 393
 * < 2^31 --, valid_min outside 0..65535, spp other than 1 or 4, W < 1, L < 1, ky or kx even or above 9, output lines
 * outside [0, L), a needed source line clamp(out_row0 - ry, 0, L-1) .. clamp(out_row0 + out_rows - 1 + ry, 0, L-1) that is
 * not resident, d_dst == d_src (the call is not in place).  out_rows == 0 is a no-op.  A line that is not a multiple of 8
 * samples, or bases that are not 16-byte aligned, take a slower kernel with the same result.  Asynchronous on the
 * context's stream (the taps are copied during the call). */
int oip_convolve_u16(oip_ctx *ctx, const uint16_t *d_src, long src_row0, long src_rows, uint16_t *d_dst, long out_row0,
                     long out_rows, int W, long L, int spp, const int32_t *taps, int ky, int kx, int valid_min);

/* The taps, host, no context needed.  fp64, every step one correctly rounded operation in the stated order.
 * oip_mtfc_quantise: c (ky * kx coefficients, row-major) -> Q12 taps:
 *   1. t = rint(c * 4096) per tap, ties to even
 *   2. OIP_E_INVALID unless |sum c - 1| <= 1e-6, the plain ascending row-major sum
 *   3. 4096 - sum t is added to the centre tap: the DC gain is exactly 1 and flat areas are unchanged
 *   4. OIP_E_INVALID if sum |t| > 32767 (err names the sum)
 * oip_mtfc_design3: the separable 3 x 3 filter that brings the MTF at Nyquist of either axis to 1, limited by max_gain.
 *   Per axis  g = min(1 / m, max_gain),  a = (g - 1) / 4,  f = [-a, 1 + 2 * a, -a]  (response at Nyquist 1 + 4 a = g);
 *   c9[j * 3 + i] = fy[j] * fx[i].  OIP_E_INVALID unless 0 < m <= 1 and max_gain >= 1.
 * oip_mtfc_load_kernel: a text file, first line `ky kx`, then ky rows of kx numbers, white-space separated, read with
 *   strtod.  c: room for 81 doubles.  OIP_E_IO when the file cannot be read, OIP_E_INVALID for a malformed file, an even
 *   size or a size above 9. */
int oip_mtfc_quantise(const double *c, int ky, int kx, int32_t *taps, char *err, int errlen);
int oip_mtfc_design3(double mtf_x, double mtf_y, double max_gain, double *c9);
int oip_mtfc_load_kernel(const char *path, double *c, int *ky, int *kx, char *err, int errlen);

/* ---- despike: repair of a raw strip ahead of RRC (`oip despike`; not in the reference) ------------------------------
 * oip_rrc_fit_columns finds dead detectors and gives them (1, 0); a hot or flickering pixel goes through RRC multiplied by its
 * k; the first resampling then spreads each such sample over a 4 x 4 bicubic footprint.  This is the step before all that:
 * listed bad columns are interpolated from their good neighbours and isolated impulse pixels are replaced by a conditional
 * 3 x 3 median.  Specified in exact integers: any evaluation order gives the same bytes.  The zero-filled line blocks that
 * the de-framer writes for missing frames (aux_separator.h:280-310) are no data: they pass through and stay out of their
 * neighbours' medians. */
#define OIP_DESPIKE_SUFFIX     ".DSPK"  /* <stem>.DSPK.<ext>, built like the reference's other product names (imageop.h:99-108) */

/* Raster and window conventions are oip_convolve_u16's: W pixels x L lines of spp samples (1, or 4 pixel-interleaved); d_src
 * holds global lines [src_row0, src_row0 + src_rows), d_dst receives [out_row0, out_row0 + out_rows), the first at d_dst; a
 * strip cut into calls gives the bytes of one call.  groups: 1, or 4 for a BIL MSS line (preproc.h:62-75; needs spp 1 and
 * W % 4 == 0): four bands of gw = W / groups columns next to each other that never mix.  d_coltab: NULL, or 2 * W int32 in HBM,
 * (Lx, Rx) per column as oip_despike_column_table builds them (spp 1 only, else OIP_E_UNSUPPORTED; the table is trusted: an
 * entry that is not Lx <= x <= Rx inside the line copies a sample of the line).  d_count: NULL, or W * spp uint64 in HBM that
 * are ADDED into; the caller zeroes them (oip_memset).  For output line y, pixel x, channel ch, all in integers:
 *   1. column repair, with a = src[v][Lx], b = src[v][Rx], D = Rx - Lx:
 *        D == 0 (every good column has Lx = Rx = x):   c(v, x) = a
 *        a < valid_min or b < valid_min:               c = a >= valid_min ? a : b
 *        otherwise:                                    c = (a * (Rx - x) + b * (x - Lx) + D / 2) / D     D / 2 and the division floored
 *      without a table c = src.
 *   2. s(v, u) = c(clamp(v, 0, L-1), clamp(u, g0, g0 + gw - 1)),  g0 = (x / gw) * gw: replicate at the image border and at
 *      band borders; with spp 4 the pixel index is clamped and the channel kept.
 *   3. ctr = s(y, x).  ctr < valid_min: out = ctr, no count.  Otherwise
 *        n'(j, i) = s(y + j - 1, x + i - 1), replaced by ctr where it is < valid_min
 *        med = the 5th smallest of the nine n' (the centre is one of them)
 *        T = thr_abs + ((med * thr_rel_q8) >> 8)
 *        |ctr - med| > T:  out = med and d_count[x * spp + ch] += 1;  otherwise out = ctr
 *      med >= valid_min always: data never becomes no data.
 * thr_abs = thr_rel_q8 = 0 is the plain 3 x 3 median with a replicate border; thr_abs = 65535 switches the despike off (the
 * output is the column-repaired input).  The counts are exact and do not depend on the launch geometry or on how the strip
 * is cut.  OIP_E_INVALID: thr_abs outside 0..65535, thr_rel_q8 outside 0..256, valid_min outside 0..65535, spp or groups other
 * than stated, W < 1, L < 1, output lines outside [0, L), a needed source line clamp(out_row0 - 1, 0, L-1) ..
 * clamp(out_row0 + out_rows, 0, L-1) that is not resident, d_dst == d_src (the call is not in place).  out_rows == 0 is a
 * no-op.  A line or a group that is not a multiple of 8 samples, or bases that are not 16-byte aligned, take a slower kernel
 * with the same result.  Asynchronous on the context's stream. */
int oip_despike_u16(oip_ctx *ctx, const uint16_t *d_src, long src_row0, long src_rows, uint16_t *d_dst, long out_row0,
                    long out_rows, int W, long L, int spp, int groups, const int32_t *d_coltab, int thr_abs,
                    int thr_rel_q8, int valid_min, uint64_t *d_count);

/* The column list and the table, host, no context needed.
 * oip_load_column_list: a text file; `#` starts a comment that runs to the end of the line; otherwise white-space separated
 *   decimal integers, each a 0-based column of the w-sample line (BIL MSS: band b column i is b * w / 4 + i), in any order,
 *   duplicates tolerated.  cols (room for cap) receives them sorted and unique, *n their number; an empty list is valid.
 *   OIP_E_IO when the file cannot be read; OIP_E_INVALID for a token that is not a number, a value outside [0, w), more than
 *   cap columns.
 * oip_write_column_list: `# comment` (one line), then one index per line.  An existing file is replaced: refusing to do so is
 *   the caller's policy.
 * oip_despike_column_table: tab (2 * w int32) receives (Lx, Rx) per column: (x, x) for a good one, for a listed one the nearest
 *   good column on either side INSIDE ITS GROUP (groups 1 or 4, w % groups == 0); a missing side is set to the other (a copy).
 *   OIP_E_INVALID for a column outside [0, w) or a group without a good column (err names the group).  longest_run (may be
 *   NULL): the longest run of adjacent listed columns inside a group. */
int oip_load_column_list(const char *path, int w, int *cols, int cap, int *n, char *err, int errlen);
int oip_write_column_list(const char *path, const int *cols, int n, const char *comment, char *err, int errlen);
int oip_despike_column_table(const int *bad, int nbad, int w, int groups, int32_t *tab, int *longest_run, char *err, int errlen);

/* ---- noise: the noise-level function of a strip or product (`oip noise`; not in the reference) ----------------------
 * sigma as a function of the signal level (read noise plus shot noise), measured on the image itself by the local-means /
 * local-standard-deviations method (Gao 1993): many small blocks, and per signal level the mode of their standard deviations.
 * A block that holds an edge or a ramp would put the scene's variance into that mode; an exact integer F test on the block's
 * four quadrants keeps such blocks out.  What `oip despike --noise` derives its two threshold parameters from. */
#define OIP_NOISE_SUFFIX        ".NOISE"   /* <stem>.NOISE.CSV */
#define OIP_NOISE_KEY_NODATA     0x00FF
#define OIP_NOISE_KEY_STRUCTURED 0x01FF

/* One u16 key per B x B block and channel of a u16 raster window, the one pass over the full-size image.  Raster conventions
 * are oip_decimate_box_u16's: rows lines of w pixels of spp samples (1, or 4 pixel-interleaved), lines `pitch` SAMPLES apart,
 * the window inside the lines of its raster.  block B is 8 or 16.  Blocks are anchored at the window's first sample; only whole
 * blocks exist, floor(w / B) per line of blocks and floor(rows / B) lines of blocks: trailing columns and lines are ignored.
 * Plane c of the keys is at d_keys + c * key_plane_stride (keys), its lines key_pitch keys apart.  For a block and channel,
 * with v its n = B * B samples and Sq[0..3] the sums of its four (B/2 x B/2) quadrants, all in unsigned 64-bit integers:
 *   S1 = sum v,  S2 = sum v * v,  D = n * S2 - S1 * S1           (n (n - 1) times the sample variance)
 *   E = 4 * (Sq[0]^2 + Sq[1]^2 + Sq[2]^2 + Sq[3]^2) - S1 * S1    (n times the between-quadrant sum of squares: D - E >= 0)
 *   any v < valid_min or v > valid_max:   key = 0x00FF           (no data)
 *   E * (n - 4) > 12 * (D - E):           key = 0x01FF           (structured: the F ratio of the between-quadrant mean square
 *                                                                 E / 3 to the within-quadrant one (D - E) / (n - 4) exceeds
 *                                                                 4; equality passes, and so does a constant block)
 *   otherwise  level = min(255, (S1 / n) >> level_shift)
 *              q     = min(254, isqrt(floor(16 * D / (n * (n - 1)))))      isqrt exact: the sample standard deviation in
 *              key   = level << 8 | q                                      quarter DN
 * The largest product is E * (n - 4) < 2^56 at B = 16.  The sentinels have q = 255, which no real key has.  The keys are 16-bit:
 * oip_histogram_u16 over a key plane gives the 256 x 256 (level x q) counts of the band, additive over line blocks, with
 * hist[0x00FF] and hist[0x01FF] the no-data and structured counts.  A strip cut into calls at lines that are multiples of B
 * (writing from key line first / B on) gives the keys of one call.  Asynchronous on the context's stream.  OIP_E_INVALID: block
 * not 8 or 16, spp not 1 or 4, level_shift outside 0..8, a valid range that is empty or outside 0..65535, pitch < w * spp,
 * key_pitch < floor(w / B).  rows < B or w < B is a no-op.  A pitch that is not a multiple of 8 samples, or a window that does
 * not start on a 16-byte boundary, takes a slower kernel with the same keys. */
int oip_noise_blocks_u16(oip_ctx *ctx, const uint16_t *d_src, long pitch, int w, long rows, int spp, int block, int level_shift,
                         int valid_min, int valid_max, uint16_t *d_keys, long key_pitch, size_t key_plane_stride);

/* The sigma of every signal level from the key histogram of a band, host, fp64 in this order.  hist: the 65536 counts of
 * oip_histogram_u16 over a key plane, hist[l * 256 + q].  Per level l:
 *   N = sum over q = 0..254 of hist[l][q]      (real blocks only: the sentinels' q = 255 never counts);  blocks[l] = N
 *   usable: N >= max(min_blocks, 1), and a mode k* exists: the smallest q in 0..253 with the largest non-zero count
 *   r = k* / 8 + 1 (integers), window [max(0, k* - r), min(253, k* + r)], c_w = the count inside it
 *   and 10 * c_w >= 3 * N: the distribution is peaked around its mode, which a level reached only by textured blocks is not
 *   sigma[l] = 0.25 * (sum over the window, q ascending, of ((double)q + 0.5) * (double)c_q) / (double)c_w
 * sigma[l] = -1 for a level that is not usable.  *n_usable (may be NULL): the usable levels.  No context needed. */
int oip_noise_levels(const uint64_t *hist, uint64_t min_blocks, double *sigma, uint64_t *blocks, int *n_usable);

/* sigma^2 = a + b * mu fitted to the usable levels (sigma[l] >= 0) of oip_noise_levels, host, fp64.  Per usable level
 * mu = ((double)l + 0.5) * 2^level_shift, v = sigma * sigma, weight w = (double)blocks[l]; plain sums in ascending l:
 *   sw = sum w, mx = (sum w mu) / sw, mv = (sum w v) / sw, sxx = sum w (mu - mx)^2, sxy = sum w (mu - mx) (v - mv)
 *   b = sxy / sxx, a = mv - b * mx
 *   fewer than two usable levels, or sxx == 0, or b < 0:   b = 0, a = mv
 *   else a < 0:                                            a = 0, b = (sum w mu v) / (sum w mu mu)
 * *mu_ref: the mu of the first usable level, ascending, at which twice the cumulative block count reaches the total (integers).
 * OIP_E_RUNTIME (err says so) without a usable level; OIP_E_INVALID for level_shift outside 0..8. */
int oip_noise_fit(const double *sigma, const uint64_t *blocks, int level_shift, double *a, double *b, double *mu_ref, char *err, int errlen);

/* The two threshold parameters of oip_despike_u16 from a noise model: the tangent to the concave k * sqrt(a + b * mu) at mu_ref,
 * which lies above the curve everywhere.  fp64:
 *   st = sqrt(a + b * mu_ref),  R = k * b / (2 * st),  N0 = k * st - R * mu_ref
 *   thr_rel_q8 = ceil(256 * R),  thr_abs = ceil(N0) + 1          (the + 1 covers the floor in despike's >> 8)
 * so that thr_abs + ((m * thr_rel_q8) >> 8) >= k * sqrt(a + b * m) for every m in 0..65535.  OIP_E_INVALID unless a, b, mu_ref
 * are finite and >= 0 and k is finite and > 0; OIP_E_RUNTIME (err says why) if st == 0, thr_rel_q8 > 256 or thr_abs > 65535. */
int oip_noise_despike_threshold(double a, double b, double mu_ref, double k, int *thr_abs, int *thr_rel_q8, char *err, int errlen);

/* ---- denoise: a sigma filter driven by the noise model (`oip denoise`; not in the reference) ------------------------
 * The acting partner of `oip noise` for the noise itself: Lee's sigma filter with a pilot estimate, an edge-preserving
 * smoother whose strength at every signal level comes from the measured sigma^2 = a + b * level.  It runs behind the
 * radiometric correction and ahead of `oip mtfc`, which amplifies what noise is left.  Specified in exact integers: any
 * evaluation order gives the same bytes. */
#define OIP_DENOISE_SUFFIX     ".DNS"   /* <stem>.DNS.<ext>, built like the reference's other product names (imageop.h:99-108) */

/* Raster and window conventions are oip_convolve_u16's: W pixels x L lines of spp samples (1, or 4 pixel-interleaved); d_src
 * holds global lines [src_row0, src_row0 + src_rows), d_dst receives [out_row0, out_row0 + out_rows), the first at d_dst; a
 * strip cut into calls gives the bytes of one call.  The border is replicated: s(v, u) = src[clamp(v, 0, L-1)][clamp(u, 0,
 * W-1)][ch], the channel kept.  radius r is 1, 2 or 3.  d_thr: spp * 256 uint16 in HBM, thr[ch][level]: the half width of the
 * range around a value of level (value >> 8).  For output line y, pixel x, channel ch, c = s(y, x), all in integers:
 *   c < valid_min:   out = c                                             no data passes through
 *   T0 = thr[ch][c >> 8],    lo0 = max(c - T0, valid_min),   hi0 = min(c + T0, 65535)
 *   stage 1, the pilot: over the 3 x 3 neighbours n = s(y + j, x + i), |j|, |i| <= 1:
 *                    S1 = sum and m1 = count of the n with lo0 <= n <= hi0           (m1 >= 1: the centre)
 *                    c1 = (2 * S1 + m1) / (2 * m1)                       integer division: the mean, half up
 *   T1 = thr[ch][c1 >> 8],   lo = max(c1 - T1, valid_min),   hi = min(c1 + T1, 65535)
 *   stage 2: over the (2r+1) x (2r+1) neighbours: S = sum and m = count of the n with lo <= n <= hi
 *   m < min_members: out = c;   otherwise out = (2 * S + m) / (2 * m)
 * A neighbour below valid_min is never a member (lo >= valid_min).  2 * S + m <= 2 * 49 * 65535 + 49 < 2^24.  It follows that
 * |c1 - c| <= T0, that |out - c1| <= T1 wherever m >= min_members, and that a sample further than T0 from all its neighbours
 * has c1 = c and m = 1: with min_members > 1 an impulse stays as it is (impulses are oip_despike_u16's business).
 * d_stats: NULL, or 4 uint64 in HBM that are ADDED into, over the output samples; the caller zeroes them (oip_memset):
 *   [0] samples with c >= valid_min   [1] of those, the samples left alone because m < min_members
 *   [2] sum of m over the filtered samples   [3] samples with out != c
 * The counters are exact and do not depend on the launch geometry or on how the strip is cut.
 * OIP_E_INVALID: radius outside 1..3, min_members outside 1..(2r+1)^2, valid_min outside 0..65535, spp other than 1 or 4, W < 1,
 * L < 1, output lines outside [0, L), a needed source line clamp(out_row0 - r, 0, L-1) .. clamp(out_row0 + out_rows - 1 + r,
 * 0, L-1) that is not resident, d_dst == d_src (the call is not in place).  out_rows == 0 is a no-op.  A line that is not a
 * multiple of 8 samples, or bases that are not 16-byte aligned, take a slower kernel with the same result.  Asynchronous on
 * the context's stream. */
int oip_sigma_filter_u16(oip_ctx *ctx, const uint16_t *d_src, long src_row0, long src_rows, uint16_t *d_dst, long out_row0,
                         long out_rows, int W, long L, int spp, int radius, const uint16_t *d_thr, int min_members, int valid_min,
                         uint64_t *d_stats);

/* The threshold table of one band from its noise model, host, no context needed.  fp64, per level l = 0..255, one correctly
 * rounded operation at a time in this order:
 *   thr256[l] = min(65535, ceil(k * sqrt(a + b * (256 * l + 128))))      k sigma at the middle of the level
 * OIP_E_INVALID unless a, b are finite and >= 0 and k is finite and > 0; OIP_E_RUNTIME (err says so) for a = b = 0, a model
 * without noise. */
int oip_denoise_thresholds(double a, double b, double k, uint16_t *thr256, char *err, int errlen);

/* ---- mask: no-data, saturation and cloud mask of a strip or product (`oip mask`; not in the reference) ---------------
 * Which parts of a raster are usable: one flag byte per C x C cell, then an opening and a buffer on the grid of cells.  It sits
 * behind `oip align` / `oip stitch` and ahead of `oip regcheck --mask`, `oip regfix` and `oip pansharpen`.  Specified in exact
 * integers: any launch geometry and any cutting of a strip gives the same bytes and the same counters. */
#define OIP_MASK_SUFFIX     ".MASK"   /* <stem>.MASK.TIFF, <stem>.MASK.CSV */
#define OIP_MASK_NODATA     1         /* the cell holds a pixel with a channel below valid_min */
#define OIP_MASK_SATURATED  2         /* the cell holds a saturated pixel */
#define OIP_MASK_CLOUD      4         /* the cell lies in the opening of the candidates (oip_mask_morph_u8) */
#define OIP_MASK_BUFFER     8         /* the cell lies within buffer_radius of CLOUD and is not CLOUD */
#define OIP_MASK_CANDIDATE 16         /* the cell passed every enabled spectral test */

/* One flag byte per cell of a u16 raster window, the one pass over the full-size image.  Raster conventions are
 * oip_noise_blocks_u16's: rows lines of w pixels of spp samples (1, or 4 pixel-interleaved), lines `pitch` SAMPLES apart, the
 * window inside the lines of its raster.  cell C is 4, 8 or 16.  Cell (j, i) covers pixels [iC, min(w, iC + C)) x [jC,
 * min(rows, jC + C)): the grid is gw = ceil(w / C) by gh = ceil(rows / C), and the cells at the right and bottom edge may hold
 * fewer than C * C pixels, n_cell.  The byte of cell (j, i) goes to d_flags[j * flag_pitch + i].
 * Per pixel:   nodata: any channel < valid_min;   sat: not nodata and any channel >= sat_level;   good: neither.
 * Per cell, in unsigned 64-bit integers (every sum is below 256 * 65535 < 2^24 and fits 32 bits):
 *   m = good pixels, n_nd = nodata pixels, n_sat = saturated pixels
 *   spp 4, band[4] = the channel of (blue, green, red, nir):  b, g, r, n = the sums of those channels over the good pixels,
 *   V = b + g + r,  mx = max(b, g, r),  mn = min(b, g, r)
 * Bits:   1 NODATA: n_nd > 0        2 SATURATED: n_sat > 0
 *        16 CANDIDATE: spp 4 only; the cell is tested (2 * m >= n_cell and m >= 1) and every enabled test holds, in signed
 *           64-bit integers (the largest product, 3 * m * full * q8, is below 2^35), `full` = full_scale:
 *             bright           256 * V >= 3 * m * full * bright_q8
 *             white            768 * (mx - mn) <= white_q8 * V
 *             haze (HOT)       256 * (2 * b - r) >= 2 * m * full * hot_q8           (blue - red / 2)
 *             not vegetation   256 * (n - r) <= ndvi_q8 * (n + r)
 *           A test whose q8 parameter is -1 is disabled; otherwise the parameter is in 0..256.
 * With spp 1 no cell is tested and bit 16 is never set (band is ignored and may be NULL).  Bits 4 and 8 are written as 0.
 * d_counts: NULL, or 8 uint64 in HBM that are ADDED into; the caller zeroes them (oip_memset).  This call adds
 *   [0] cells   [1] NODATA cells   [2] SATURATED cells   [3] tested cells   [4] CANDIDATE cells   [7] saturated pixels
 * ([5] and [6] belong to oip_mask_morph_u8).  The counters are exact and do not depend on the launch geometry or on how a strip
 * is cut.  A strip cut into calls at lines that are multiples of C (each call writing from cell line first / C on) gives the
 * bytes and the counters of one call.  Lines and offsets are 64-bit.  Asynchronous on the context's stream.  OIP_E_INVALID:
 * cell not 4, 8 or 16, spp not 1 or 4, w < 0, rows < 0, pitch < w * spp, flag_pitch < gw, valid_min outside 0..65535, sat_level
 * or full_scale outside 1..65535, a q8 parameter outside -1..256, with spp 4 a band that is not a permutation of 0..3.  w == 0
 * or rows == 0 is a no-op.  A pitch that is not a multiple of 8 samples, or a window that does not start on a 16-byte
 * boundary, takes a slower kernel with the same bytes. */
int oip_mask_cells_u16(oip_ctx *ctx, const uint16_t *d_src, long pitch, int w, long rows, int spp, int cell, int valid_min, int sat_level,
                       int full_scale, const int *band, int bright_q8, int white_q8, int hot_q8, int ndvi_q8, uint8_t *d_flags,
                       long flag_pitch, uint64_t *d_counts);

/* Opening and buffer on the whole gw x gh grid of flag bytes, in place.  X = the cells with bit 16.
 *   E (erosion): a cell is in E iff every cell of the (2a+1) x (2a+1) square around it that lies inside the grid is in X;
 *                what lies outside the grid does not constrain
 *   O = the cells within Chebyshev distance a of a cell of E (the opening);   D = the cells within Chebyshev distance d of O
 *   bit 4 CLOUD = O,   bit 8 BUFFER = D \ O
 * a = open_radius in 0..32, d = buffer_radius in 0..64; a radius may exceed the grid.  Bits 1, 2 and 16 are kept, bits 4 and 8
 * are overwritten: a second call changes nothing.  It follows that O is a subset of X, that a = 0 gives O = X and that the
 * opening is idempotent.  d_counts (NULL, or the 8 uint64 of oip_mask_cells_u16): [5] += CLOUD cells, [6] += BUFFER cells.
 * Scratch (3 bits per cell) comes from the context's grow-only workspace.  OIP_E_INVALID: a radius out of range, gw < 0,
 * gh < 0, flag_pitch < gw.  An empty grid is a no-op.  Asynchronous on the context's stream. */
int oip_mask_morph_u8(oip_ctx *ctx, uint8_t *d_flags, long flag_pitch, int gw, long gh, int open_radius, int buffer_radius,
                      uint64_t *d_counts);

/* gw = ceil(w / cell), gh = ceil(h / cell).  Host, no context needed.  OIP_E_INVALID: cell not 4, 8 or 16, w < 0, h < 0. */
int oip_mask_grid(int w, long h, int cell, int *gw, long *gh);

/* 1 if any cell of the gw x gh grid (host bytes, lines flag_pitch apart) that intersects the pixel rectangle [x, x + tw) x
 * [y, y + th) has a bit of `bits` set, else 0: the part of the rectangle outside the grid holds no cell, and neither does an
 * empty rectangle.  Host, no context needed.  What `oip regcheck --mask` asks per tile. */
int oip_mask_tile_flag(const uint8_t *flags, long flag_pitch, int gw, long gh, int cell, long x, long y, long tw, long th, int bits);

/* ---- wallis: local brightness and contrast equalisation of a strip or product (`oip wallis`; not in the reference) ------
 * The Wallis filter ("dodging"): every sample gets a gain and an offset that pull the mean and the standard deviation of its
 * neighbourhood toward a target, interpolated bilinearly between the nodes of a coarse grid of B x B blocks.  It removes the
 * low-frequency unevenness (illumination, haze, residual vignetting) that no other step touches.  Two passes on the device
 * (block moments; the point transform) around one host step (moments -> node gains and offsets).  Everything on the device
 * is exact integers: any launch geometry and any cutting of a strip gives the same bytes and the same counters. */
#define OIP_WALLIS_SUFFIX ".WAL"      /* <stem>.WAL.<ext>, <stem>.WAL.CSV */

/* n, S1, S2 of every block of a u16 raster window, the read-only pass.  Raster conventions are oip_mask_cells_u16's: rows
 * lines of w pixels of spp samples (1, or 4 pixel-interleaved), lines `pitch` SAMPLES apart, the window inside the lines of
 * its raster; lines and offsets are 64-bit.  block B is 32, 64, 128 or 256.  Block (j, i) covers pixels [iB, min(w, iB + B)) x
 * [jB, min(rows, jB + B)): the grid is gw = ceil(w / B) by gh = ceil(rows / B), and the blocks at the right and bottom edge hold
 * fewer pixels.  Per block and channel c, over the samples v with valid_min <= v <= valid_max, in unsigned 64-bit integers:
 *   n = count,   S1 = sum v,   S2 = sum v * v          (S2 <= 65536 * 65535^2 < 2^48)
 * They are STORED, not added:  d_acc[(m * spp + c) * acc_plane_stride + j * acc_pitch + i],  m = 0, 1, 2 for n, S1, S2.
 * A block without a valid sample stores three zeros.  A strip cut into calls at lines that are multiples of B (each call
 * writing from block line first / B on: the caller offsets d_acc) gives the entries of one call.  No entry depends on the launch
 * geometry.  Asynchronous on the context's stream.  OIP_E_INVALID: block not one of the four, spp not 1 or 4, w < 0, rows < 0,
 * pitch < w * spp, acc_pitch < gw, planes that overlap (acc_plane_stride < (gh - 1) * acc_pitch + gw), valid_min > valid_max
 * or either outside 0..65535.  w == 0 or rows == 0 is a no-op.  A pitch that is not a multiple of 8 samples, or a window that
 * does not start on a 16-byte boundary, takes a slower kernel with the same entries. */
int oip_block_moments_u16(oip_ctx *ctx, const uint16_t *d_src, long pitch, int w, long rows, int spp, int block, int valid_min, int valid_max,
                          uint64_t *d_acc, long acc_pitch, size_t acc_plane_stride);

/* gw = ceil(w / block), gh = ceil(h / block).  Host, no context needed.  OIP_E_INVALID: block not 32, 64, 128 or 256, w < 0,
 * h < 0. */
int oip_wallis_grid(int w, long h, int block, int *gw, long *gh);

/* Node gains and offsets from the block moments.  Host, no context needed.  acc: a host copy of the 3 * spp planes in the
 * layout above.  contrast c in (0, 1], brightness b in [0, 1], 0 < g_min <= 1 <= g_max <= 16.  target_mean / target_std: NULL,
 * or spp values; NaN (or NULL) = take the image's own; a given mean lies in 0..65535, a given std is at most 65535.
 * Every step is one correctly rounded fp64 operation in the stated order; integers below 2^53 convert exactly, the 128-bit
 * integers D convert to the nearest double (as in oip_seam_fit).
 *   1. Per channel the totals N, A, Q = the sums of its planes n, S1, S2 (N < 2^63).
 *        D0 = N * Q - A * A (exact, 128-bit)    m0 = (double)A / (double)N    s0 = sqrt((double)D0) / (double)N
 *        m_t = the given mean or m0,  s_t = the given std or s0.
 *      OIP_E_RUNTIME, naming the channel: N < max(min_count, 2), or s_t is not > 0 (a constant channel without --std).
 *   2. fit(n, S1, S2):   D = n * S2 - S1 * S1 (128-bit)     m = (double)S1 / (double)n     s = sqrt((double)D) / (double)n
 *        den = c * s + (1 - c) * s_t      g = (c * s_t) / den      g = min(max(g, g_min), g_max)
 *        o = (b * m_t + (1 - b) * m) - g * m
 *        G = rint(g * 65536) (Q16)        O = rint(o * 256) (Q8)         |O| <= 256 * 17 * 65535 < 2^29
 *   3. Node (j, i, c) = fit of its block.  Where n < max(min_count, 2) or D == 0 the node takes the fit of the channel's
 *      totals (G0_c, O0_c) and substituted[...] = 1: never an error -- the black borders of prestitch and the aligner, water
 *      and cloud produce such blocks.  With D0 == 0 (a constant channel with a given std) (G0, O0) is the identity (65536, 0).
 * Q16 keeps a gain of 16 below 2^20 and resolves 1.5e-5, less than half a DN over the full scale; Q8 keeps the offset's
 * rounding error at 1/512 DN while 256 * O stays below 2^37.
 * Out: node_gain_q16 / node_offset_q8 / substituted: gh * gw * spp values each, entry [(j * gw + i) * spp + c].  report (may be
 * NULL): 9 doubles per channel: N, m0, s0, m_t, s_t, nodes, substituted nodes, min G, max G.  With c = b = 1 this is plain
 * normalisation of every block to (m_t, s_t); smaller c and b leave part of the local statistics in place.
 * OIP_E_INVALID: a NULL table, spp not 1 or 4, gw < 1, gh < 1, acc_pitch < gw, planes that overlap (acc_plane_stride <
 * (gh - 1) * acc_pitch + gw, at either spp: there are 3 * spp planes), a parameter outside its range, a channel whose A or Q does not
 * fit 64 bits (u16 samples with N < 2^48 never get there).  err (may be NULL) receives the text. */
int oip_wallis_fit(const uint64_t *acc, long acc_pitch, size_t acc_plane_stride, int gw, long gh, int spp, double contrast, double brightness,
                   double g_min, double g_max, uint64_t min_count, const double *target_mean, const double *target_std, int32_t *node_gain_q16,
                   int32_t *node_offset_q8, int *substituted, double *report, char *err, int errlen);

/* The point transform, the read-write pass.  The raster is W pixels x L lines of spp samples, lines W * spp samples apart;
 * d_src holds the global lines [row0, row0 + rows) and d_dst receives the same lines.  The transform is pointwise: any cut of a
 * strip gives the bytes of one call, and d_dst == d_src is allowed (no other overlap is).  d_gain_q16 / d_offset_q8: the
 * gh * gw * spp node values of oip_wallis_fit on the device, gains in 0..2^20 and |offset| < 2^29 (values outside are not
 * checked and give unspecified samples, never an access outside the rasters).  Node (j, i) sits at line jB + B/2, column
 * iB + B/2.  For either table V (G or O) and channel c, in signed 64-bit integers, floors toward minus infinity (B is a power
 * of two: every division is an arithmetic shift), as in oip_seam_line_tables:
 *   along the strip:  u = y - B/2,  k = clamp(floor(u / B), 0, max(gh - 2, 0)),  t = clamp(u - k B, 0, B),  k' = min(k + 1, gh - 1)
 *                     Vy(i) = floor((V[k][i] * (B - t) + V[k'][i] * t + B/2) / B)
 *   across the line:  the same formula on Vy with x and gw  ->  G(y, x, c), O(y, x, c)
 *   v = src[y][x][c]
 *   v < valid_min or v > valid_max:   out = v                                  (no data and saturation pass through)
 *   otherwise:                        out = clamp((G * v + 256 * O + 32768) >> 16, valid_min, clamp_max)
 * The tables are constant before the first node and after the last, in both axes; a value never leaves the interval of its
 * nodes.  G * v < 2^36, 256 * |O| < 2^37.  Nodes that all hold (65536, 0) give the input's bytes (with clamp_max >= valid_max);
 * nodes that all hold one (G, O) give the plain per-sample transform.
 * d_stats: NULL, or 3 uint64 in HBM that are ADDED into: [0] transformed samples, [1] samples clamped at valid_min, [2] samples
 * clamped at clamp_max.  The counters are exact and independent of the launch geometry and of the cut.
 * OIP_E_INVALID: block, spp or the valid range as for oip_block_moments_u16, clamp_max outside valid_min..65535, W < 1, L < 1,
 * gw != ceil(W / B) or gh != ceil(L / B), lines outside [0, L).  rows == 0 is a no-op.  A line that is not a multiple of 8
 * samples, or bases that are not on 16-byte boundaries, take a slower kernel with the same result.  Asynchronous. */
int oip_wallis_apply_u16(oip_ctx *ctx, const uint16_t *d_src, uint16_t *d_dst, long row0, long rows, int W, long L, int spp, int block,
                         const int32_t *d_gain_q16, const int32_t *d_offset_q8, int gw, long gh, int valid_min, int valid_max, int clamp_max,
                         uint64_t *d_stats);

/* ---- mtf: the MTF at Nyquist from the straight edges of a strip or product (`oip mtf`; not in the reference) --------
 * The slanted-edge method (ISO 12233) on every 32 x 32 tile that holds one straight, high-contrast, slightly slanted edge.
 * What `oip mtfc --mtf REPORT` takes its two numbers from.  The device part is exact integers: any launch geometry and any
 * cut of the strip give the same bytes.  The host part is fp64, one correctly rounded operation at a time in the stated order.
 *
 * A tile is 32 profiles of 32 samples p[r][i].  axis 0 (x, the MTF across the lines): a profile is a piece of a line and i
 * runs over columns; tile (ty, tx) starts at line 32 ty, column 16 tx, tx = 0 .. floor((w - 32) / 16).  axis 1 (y, along the
 * lines): a profile is a piece of a column and i runs over lines; tile (ty, tx) starts at line 16 ty, column 32 tx.  Tiles are
 * staggered by half a tile along the profile; the centring window lets an edge pass in at most one of two overlapping tiles.
 * Only whole tiles exist.  Channel c of pixel i is src[i * spp + c].  Den = 32 * sum r^2 - (sum r)^2 = 87296 (r = 0..31).
 *
 * The record of a tile and channel is four int32 {status, s, Sc, Num}.  With
 *   D_r = p[r][31] - p[r][0],  d[r][i] = p[r][i + 1] - p[r][i] (i = 0..30),  s = sign(sum_r D_r),  e = s * d,  S0_r = s * D_r,
 *   TV_r = sum_i |d[r][i]|,  S1_r = sum_i (2 i + 1) * e[r][i],
 *   c_r = (64 * S1_r) / S0_r          (integers, both non-negative: the centroid of the derivative in Q7 samples, sample i at i)
 *   Sc = sum_r c_r,  Num = 32 * sum_r r * c_r - 496 * Sc,
 *   f_r = floor((2 * Den * Sc + 32 * Num * (2 r - 31)) / (64 * Den))  in int64  (the least-squares line through the centroids, Q7)
 * the tests run in this order, each over all 32 profiles; the first that fails gives the status and the other words are 0:
 *   1 NODATA       a sample lies outside [valid_min, valid_max]
 *   2 FLAT         sum_r D_r == 0
 *   3 LOWCONTRAST  some S0_r < contrast_min
 *   4 TEXTURED     some 4 * TV_r > 5 * S0_r + 4 * tv_slack, or some S1_r < 0
 *   5 OFFCENTRE    some c_r < 1280 or c_r > 2688        (the edge 10 to 21 samples in: 8 samples covered on either side)
 *   6 SLANT        not 4 * Den <= |Num| <= 32 * Den     (the edge crosses 1 to 8 samples over the 32 profiles)
 *   7 CURVED       some |c_r - f_r| > 64                (half a sample off the line)
 *   0 OK           the record holds s, Sc, Num */
#define OIP_MTF_SUFFIX      ".MTF"   /* <stem>.MTF.CSV */
#define OIP_MTF_NO_VALUE    16       /* oip_mtf_tile: the tile gives no value (EMPTYBIN) */
enum { OIP_MTF_OK = 0, OIP_MTF_NODATA, OIP_MTF_FLAT, OIP_MTF_LOWCONTRAST, OIP_MTF_TEXTURED, OIP_MTF_OFFCENTRE, OIP_MTF_SLANT, OIP_MTF_CURVED };

/* Pass 1: the records of every whole tile of the resident window (rows lines of w pixels of spp samples, lines `pitch` SAMPLES
 * apart, the window inside the lines of its raster).  The record of channel c, tile (ty, tx) is at
 * d_rec + 4 * (c * rec_plane_stride + ty * rec_pitch + tx): pitch and plane stride count records.  A strip cut into calls at
 * multiples of 32 lines (axis 1: the next call starts 16 lines before the end of the previous one's last tile) gives the
 * records of one call.  OIP_E_INVALID: axis not 0 or 1, spp not 1 or 4, contrast_min < 1, tv_slack outside 0..65535, a valid
 * range that is empty or outside 0..65535, pitch < w * spp, rec_pitch below the tiles per tile line, overlapping planes.  A
 * window smaller than one tile is a no-op.  Axis 0 at spp 1 with a pitch that is a multiple of 8 samples and a window on a
 * 16-byte boundary reads 16 bytes at a time; everything else takes sample loads, with the same records.  Asynchronous on the
 * context's stream. */
int oip_mtf_tiles_u16(oip_ctx *ctx, const uint16_t *d_src, long pitch, int w, long rows, int spp, int axis, int contrast_min, int tv_slack,
                      int valid_min, int valid_max, int32_t *d_rec, long rec_pitch, size_t rec_plane_stride);

/* Pass 2: the edge-spread function (the mean profile across the edge, oversampled by 4) of n listed tiles of the same window
 * under the same parameters.  d_list: n entries {channel, ty, tx} of int32 in HBM.  Per entry the record is recomputed from the
 * samples; with status 0, for every r and i:
 *   u = 128 * i - f_r,  b = (u + 1024) >> 5 (arithmetic: a floor);  0 <= b < 64:  sum[b] += p[r][i], cnt[b] += 1
 * d_esf receives 128 uint32 per entry, the 64 sums and then the 64 counts; all zero for a tile whose status is not 0.  d_s0:
 * NULL, or n int32 that receive sum_r S0_r (0 unless the status is 0): 32 times the contrast the report states.  The list is
 * read back and checked before anything is launched (the call synchronises the stream): OIP_E_INVALID for an entry outside
 * the window's channels and tiles, and for what oip_mtf_tiles_u16 refuses.  n == 0 is a no-op. */
int oip_mtf_esf_u16(oip_ctx *ctx, const uint16_t *d_src, long pitch, int w, long rows, int spp, int axis, int contrast_min, int tv_slack,
                    int valid_min, int valid_max, const int32_t *d_list, long n, uint32_t *d_esf, int32_t *d_s0);

/* The MTF at Nyquist of one tile from its polarity s (+1 or -1) and its 64 sums and 64 counts, host, fp64 in this order:
 *   any cnt[b] == 0:  OIP_MTF_NO_VALUE
 *   E_b = (double)s * (double)sum[b] / (double)cnt[b]                       (the product first)
 *   L_j = E_(j+1) - E_j,  w_j = 0.54 - 0.46 * cos(2.0 * pi * (double)j / 62.0),  t_j = w_j * L_j      j = 0..62
 *   k = (j - 31) mod 8 in 0..7,  C8[k] = cos(pi k / 4),  S8[k] = sin(pi k / 4) from a table of the literals 0, +-1 and
 *   +-0.70710678118654752      (Nyquist of the original sampling is 1/8 cycle per bin)
 *   A0 = sum t_j,  Re = sum t_j * C8[k],  Im = sum t_j * S8[k], each from 0.0 in ascending j
 *   not A0 > 0:  OIP_MTF_NO_VALUE
 *   *mtf = hypot(Re, Im) / A0 / (q * q),  q = sin(pi / 8.0) / (pi / 8.0)     (the two-point difference and the quarter-sample bin)
 * OIP_E_INVALID for s other than +-1 or a NULL pointer. */
int oip_mtf_tile(int s, const uint32_t *sum, const uint32_t *cnt, double *mtf);

/* median = v[(n - 1) / 2], p75 = v[3 (n - 1) / 4], p90 = v[9 (n - 1) / 10] of the n values sorted ascending (integer indices;
 * the input is not modified).  OIP_E_INVALID for n < 1 or a value that is not finite. */
int oip_mtf_summary(const double *values, long n, double *median, double *p75, double *p90);

/* The tv_slack that lets noise of sigma_ref DN through the TEXTURED test: ceil(48 * sigma_ref), at most 65535.  The 31 noise
 * differences of a profile have mean |.| 1.13 sigma each and sum to 35 sigma; the rest is margin.  -1 for a sigma_ref that is
 * negative or not a number. */
int oip_mtf_tv_slack(double sigma_ref);

/* The strips of an LZW TIFF product, encoded on the device (cv::imwrite's TIFF encoder behind preproc.h:167-185 and GDAL's
 * COMPRESS=LZW PREDICTOR=2 behind imageop.h:460-567 do this on the host, strip by strip).  d_img: rows x width x spp u16,
 * interleaved, in file sample order (oip_permute_u16x4 first where cv::imwrite / a band map reorder); spp 1 or 4; strip k
 * holds rows [k rows_per_strip, (k + 1) rows_per_strip).  Every strip is the horizontal-predictor differences of its rows
 * through TIFF 6.0's LZW as libtiff writes it (MSB-first 9..12-bit codes, ClearCode first, early change, EndOfInformation).
 * The encoded strips are packed into d_payload at even offsets in strip order; strip_off / strip_len (host arrays, one
 * entry per strip) say where, *payload_bytes is the end of the last one.  payload_cap >= oip_tiff_lzw_worst_bytes().
 * d_scratch: NULL (the call allocates and frees its own) or >= oip_tiff_lzw_scratch_bytes() of device memory, 8-byte aligned,
 * that a caller who knows the product's geometry early prepares off the critical path.  Refusals are OIP_E_INVALID with nothing
 * launched, the ones oip_tiff_deflate_strips_u16 has: a null pointer, rows, width or rows_per_strip below 1, spp other than 1 or
 * 4, a strip above 1 GiB, an image of 4 samples that is not 8-byte aligned, payload_cap below oip_tiff_lzw_worst_bytes(), a
 * scratch buffer below oip_tiff_lzw_scratch_bytes() or not 8-byte aligned.  Synchronises the context's stream. */
size_t oip_tiff_lzw_worst_bytes(long rows, int width, int spp, long rows_per_strip);
size_t oip_tiff_lzw_scratch_bytes(long rows, int width, int spp, long rows_per_strip);
int oip_tiff_lzw_strips_u16(oip_ctx *ctx, const uint16_t *d_img, long rows, int width, int spp, long rows_per_strip,
                            uint8_t *d_payload, size_t payload_cap, uint64_t *strip_off, uint64_t *strip_len,
                            size_t *payload_bytes, void *d_scratch, size_t scratch_bytes);

/* ... and read: the LZW strips of a TIFF file (cv::imread of the stitch inputs, imageop.h:380-388) decoded on the device.
 * d_file: the file's bytes from some base offset on, already in HBM (oip_read_file_to_device); strip_off / strip_len (host):
 * every strip's offset inside d_file and its size; chunky u16 samples, predictor 1 or 2.  d_img receives rows x width x spp
 * samples in file order.  A stream that ends without EndOfInformation is tolerated (as libtiff does); a corrupt stream or a
 * strip that does not decode to exactly its rows is OIP_E_RUNTIME with the strip named.  Synchronises the stream. */
int oip_tiff_lzw_decode_u16(oip_ctx *ctx, const uint8_t *d_file, size_t file_bytes, const uint64_t *strip_off,
                            const uint64_t *strip_len, long nstrips, long rows, int width, int spp, long rows_per_strip,
                            int predictor, uint16_t *d_img);

/* The same for a Deflate TIFF (compression 8, or its older number 32946): every strip -- or tile, passed as a T-wide image in
 * strips of T rows -- is one zlib stream (RFC 1950 around RFC 1951), inflated by one wave of the device (csrc/tiffdeflate.hip)
 * with the decoder the host reader runs (csrc/oip_inflate.h; no libz).  Arguments, argument checks and the order of the samples
 * are those of oip_tiff_lzw_decode_u16; spp up to 16, predictor 1 or 2.  What a stream must be, on the host and on the device
 * alike (the yardstick is zlib's inflate):
 *   header    CM = 8, CINFO <= 7, FCHECK valid, FDICT clear.
 *   blocks    stored, fixed and dynamic; BTYPE 3 is corrupt.  Corrupt as well: a stored block whose LEN is not ~NLEN; HLIT > 286
 *             or HDIST > 30; a code-length code, literal/length set or distance set that is over-subscribed; one that is
 *             incomplete -- except, as in zlib, a literal/length or distance set of a single code of length 1, and a distance
 *             set with no code at all; a repeat code 16 with no length before it; a repeat that runs past HLIT + HDIST; no code
 *             for end-of-block; literal/length symbols 286 and 287; distance symbols 30 and 31; bits that are no code of an
 *             incomplete set; a distance that reaches before the start of the stream's own output (there is no dictionary).
 *   size      exactly the bytes of its strip or tile; more or fewer is an error.
 *   trailer   where all four Adler-32 bytes are present they must match; a stream that ends after its final block with fewer
 *             than four bytes left is accepted (libtiff stops reading when the output is full, and such files exist).  A stream
 *             that ends inside a block is an error.  Bytes after the trailer are ignored.
 * A stream that breaks a rule ends its own decode: OIP_E_RUNTIME with the first such strip and the cause named; the other
 * strips are decoded and nothing outside d_img's rows x width x spp samples is written.  Input reads are bounded by the
 * stream's length, window indices are masked and every store is bounded by the strip's size, whatever the stream holds.
 * Synchronises the stream. */
int oip_tiff_deflate_decode_u16(oip_ctx *ctx, const uint8_t *d_file, size_t file_bytes, const uint64_t *strip_off,
                                const uint64_t *strip_len, long nstrips, long rows, int width, int spp, long rows_per_strip,
                                int predictor, uint16_t *d_img);

/* ... and written: the strips of a Deflate TIFF product (compression 8, predictor 2) encoded on the device, the mirror of
 * oip_tiff_lzw_strips_u16 with its arguments, its refusals (OIP_E_INVALID with nothing launched: a null pointer, rows, width or
 * rows_per_strip below 1, spp other than 1 or 4, a strip above 1 GiB, payload_cap below oip_tiff_deflate_worst_bytes(), a scratch
 * buffer below oip_tiff_deflate_scratch_bytes() or not 8-byte aligned) and its packing: streams at even offsets of d_payload in
 * strip order, strip_off / strip_len (host) say where, *payload_bytes ends the last one.  A tile batch is a T-wide image in strips
 * of T rows.  d_img (2-byte aligned) is read, never written: the predictor-2 differences (sample minus the same channel of the
 * previous pixel mod 2^16, restarting at every row, little-endian bytes) are made as the input is staged.  Every strip is one zlib
 * stream from one wave of the device (csrc/tiffdeflate.hip) running the encoder the host writers run (csrc/oip_deflate.h; no libz):
 *   validity  zlib's inflate and oip_tiff_deflate_decode_u16 accept it and get exactly the strip's bytes.  Header 0x78 0x01 (CM 8,
 *             CINFO 7, FDICT clear, FCHECK valid), the Adler-32 of the bytes as trailer, BFINAL on the last block, no dictionary;
 *             lengths 3..258; distances 1..30656, never before the stream's start.
 *   blocks    dynamic Huffman blocks (BTYPE 2) of at most 16384 input bytes or 2048 matches, their literal/length, distance and
 *             code-length codes built from the block's own histogram and limited to 15 / 15 / 7 bits; every set sent is complete
 *             (a set with fewer than two used symbols gets symbols 0 / 1 added, as zlib does).  A block goes out fixed (BTYPE 1)
 *             or stored (BTYPE 0, neighbours merged up to 65535 bytes) where that is smaller, stored on ties.
 *   size      never more than n + 5 ceil(n / 65535) + 6 bytes for a strip of n bytes (11 for none): a stream that would pass
 *             that is written again as stored blocks only.  oip_tiff_deflate_worst_bytes() is that bound for every strip plus
 *             the padding to even offsets.
 *   matching  one hashed candidate (4 bytes, 4096 slots, the last position of an earlier 64-position round) and distance 1 per
 *             position, greedy; see csrc/oip_deflate.h.  A floor, not zlib's ratio on compressible scenes.
 *   function  the bytes of a stream depend on the strip's bytes alone: not on the launch, the batch, the strip's index, any
 *             alignment, or on whether the host or the device ran the coder (oip_deflate_stream_host gives the same bytes).
 * LDS indices are masked or bounded and every store of a stream is bounded by its slot, whatever the image holds.  The scratch
 * (output slots of one launch, lengths, offsets) does not hold tokens: those stay in LDS.  Synchronises the context's stream. */
size_t oip_tiff_deflate_worst_bytes(long rows, int width, int spp, long rows_per_strip);
size_t oip_tiff_deflate_scratch_bytes(long rows, int width, int spp, long rows_per_strip);
int oip_tiff_deflate_strips_u16(oip_ctx *ctx, const uint16_t *d_img, long rows, int width, int spp, long rows_per_strip,
                                uint8_t *d_payload, size_t payload_cap, uint64_t *strip_off, uint64_t *strip_len,
                                size_t *payload_bytes, void *d_scratch, size_t scratch_bytes);

/* The same encoder in its host instantiation, for one stream and without a context: src[0, n) as a zlib stream into dst[0, cap).
 * Returns the stream's size, or 0 when cap is too small (never when cap >= n + 5 ceil(n / 65535) + 6, or 11 for n = 0), when n is
 * 0xFFFF0000 or more, or when a pointer is null.  No alignment is asked of either buffer; nothing past either is touched. */
size_t oip_deflate_stream_host(const uint8_t *src, size_t n, uint8_t *dst, size_t cap);

/* ---- JPEG: the browse image of `oip quicklook --format jpeg` as a JFIF file, its scan encoded on the device (not in the
 * reference).  Baseline sequential DCT (ITU-T T.81 SOF0) in a JFIF 1.01 wrapper: 8 bits a sample; 1 component (grey) or 3 (Y, Cb,
 * Cr, 4:4:4: one 8 x 8 block per component per MCU); the four typical Huffman tables of T.81 Annex K.3; a DRI segment with a
 * restart interval of exactly one MCU row, ceil(w / 8) MCUs, RST0..RST7 cycling between the intervals and none before EOI.  An
 * interval reads its own 8 image lines and nothing else, so the intervals are independent streams: one wave of the device each
 * (csrc/jpeg.hip) running the coder the host instantiation runs (csrc/oip_jpeg.h; no libjpeg).  The arithmetic, all of it exact
 * integers (>> is an arithmetic shift, / truncates; tests/_jpeg_ref.py restates it):
 *   colour    (3 channels, from interleaved R, G, B bytes; the results lie in 0..255 without a clamp)
 *               Y  = ( 19595 R + 38470 G +  7471 B +   32768) >> 16
 *               Cb = (-11058 R - 21710 G + 32768 B + 8421375) >> 16
 *               Cr = ( 32768 R - 27439 G -  5329 B + 8421375) >> 16
 *   padding   the image is extended to multiples of 8 by repeating its last column, then its last line.
 *   DCT       T[k][n] = rint(8192 c_k cos((2n + 1) k pi / 16)), c_0 = sqrt(1/8), c_k = 1/2 otherwise:
 *               k = 0:  2896  2896  2896  2896  2896  2896  2896  2896      k = 4:  2896 -2896 -2896  2896  2896 -2896 -2896  2896
 *               k = 1:  4017  3406  2276   799  -799 -2276 -3406 -4017      k = 5:  2276 -4017   799  3406 -3406  -799  4017 -2276
 *               k = 2:  3784  1567 -1567 -3784 -3784 -1567  1567  3784      k = 6:  1567 -3784  3784 -1567 -1567  3784 -3784  1567
 *               k = 3:  3406  -799 -4017 -2276  2276  4017   799 -3406      k = 7:   799 -2276  3406 -4017  4017 -3406  2276  -799
 *             rows of a block, samples s[0..7]:   t[k] = (sum_n T[k][n] (s[n] - 128) + 512) >> 10
 *             then its columns, t[0..7] of a column:   F[k] = (sum_m T[k][m] t[m] + 32768) >> 16
 *             (int32 holds it: |row sum| <= 128 * 8 * 4017, |column sum| <= 8 * 4017^2; |DC| <= 1024, |AC| <= 1020)
 *   tables    the IJG rule on the base tables of Annex K.1 (Y, grey) and K.2 (Cb, Cr):
 *               scale = Q < 50 ? 5000 / Q : 200 - 2 Q,   q = clamp((base * scale + 50) / 100, 1, 255)
 *   quantise  sign(F) ((2 |F| + q) / (2 q))
 *   entropy   T.81 F.1.2: the DC difference against the previous block of the same component, 0 at the start of each interval;
 *             AC run/size symbols with ZRL and EOB, no EOB when coefficient 63 is not zero; bits MSB first, a 0xFF byte followed
 *             by 0x00, each interval padded with 1-bits to a byte.
 *   file      SOI; APP0 "JFIF", version 1.01, no units, density 1 : 1, no thumbnail; one DQT per table in use (8-bit entries,
 *             table 0 and for 3 channels table 1); SOF0 (components 1..nch, sampling 1 x 1, tables 0, 1, 1); one DHT per table in
 *             use (DC 0, AC 0 and for 3 channels DC 1, AC 1); DRI; SOS (Ss 0, Se 63, Ah Al 0); the intervals with RST(k mod 8)
 *             behind interval k but the last; EOI.
 *   function  the bytes of an interval depend on its own 8 lines, nch and the quality alone: not on the launch, the interval's
 *             index, the pitch, any alignment, or on whether the host or the device ran the coder.
 *
 * oip_jpeg_scan_u8 encodes the scan of d_img (device; h lines of w pixels of nch interleaved bytes, lines pitch_bytes apart; read,
 * never written; no alignment asked) into d_payload (device): interval k, without its RSTn, at interval_off[k] with
 * interval_len[k] bytes (host arrays of ceil(h / 8) entries), packed behind one another in order; *payload_bytes ends the last.
 * All offsets are 64-bit.  A coefficient costs at most 26 bits, doubled by stuffing 416 bytes a block:
 * oip_jpeg_worst_bytes() = ceil(h / 8) * ceil(w / 8) * nch * 416 is the capacity the caller proves (0 for arguments the scan
 * refuses).  The coder runs twice -- measuring, then storing every interval at the running sum of the lengths, each store bounded by
 * the measured length -- so no more than *payload_bytes of the payload is ever written.  d_scratch (8-byte aligned, at least
 * oip_jpeg_scratch_bytes(): the tables, lengths and offsets, and in its last 40 bytes five uint64 counters, the cycles the waves of
 * the storing pass spent staging, transforming, counting bits, placing codes and stuffing -- a profile's input
 * (profiles/jpeg_bench.py), no part of the contract) may be NULL: the call then allocates its own.  OIP_E_INVALID with
 * nothing launched for a null pointer, w or h outside 1..65535, nch other than 1 or 3, quality outside 1..100, pitch_bytes <
 * w * nch, payload_cap below the bound, a scratch buffer too small or misaligned.  Synchronises the context's stream. */
size_t oip_jpeg_worst_bytes(int w, long h, int nch);
size_t oip_jpeg_scratch_bytes(int w, long h, int nch);
int oip_jpeg_scan_u8(oip_ctx *ctx, const uint8_t *d_img, long pitch_bytes, int w, long h, int nch, int quality,
                     uint8_t *d_payload, size_t payload_cap, uint64_t *interval_off, uint64_t *interval_len,
                     size_t *payload_bytes, void *d_scratch, size_t scratch_bytes);

/* The same coder in its host instantiation, for one interval and without a context: interval `interval` (0 .. ceil(h / 8) - 1) of
 * the host image img into dst[0, cap).  Returns its size, or 0 when cap is too small (never when cap >= ceil(w / 8) * nch * 416) or
 * an argument is one the scan refuses.  Nothing past either buffer is touched. */
size_t oip_jpeg_interval_host(const uint8_t *img, long pitch_bytes, int w, long h, int nch, int quality, long interval,
                              uint8_t *dst, size_t cap);

/* The JFIF file of a scan, host: the headers above, the intervals of `payload` (host) with their RSTn, EOI.  An existing file is
 * replaced.  OIP_E_INVALID for a null pointer or geometry and quality the scan refuses, OIP_E_IO (errno in the message) where the
 * file cannot be written.  No context needed. */
#define OIP_JPEG_DEF_QUALITY 90   /* of `oip quicklook --format jpeg`: a convention, nothing measured */
#define OIP_JPEG_MAX_DIM     65535
int oip_write_jpeg_u8(const char *path, const uint8_t *payload, const uint64_t *interval_off, const uint64_t *interval_len,
                      int w, long h, int nch, int quality, char *err, int errlen);

/* ---- overviews: reduced-resolution levels of a strip or product (`oip overviews`; not in the reference) ---- */
#define OIP_OVERVIEW_SUFFIX ".ovr"   /* appended to the whole file name, GDAL's external-overview convention */

/* One level of the pyramid.  Level 0 is the image: w0 x h0 pixels of spp samples (1, or 4 pixel-interleaved); level k >= 1
 * has w_k = ceil(w_{k-1} / 2), h_k = ceil(h_{k-1} / 2) and the same spp.  For its sample (y, x, c): of the up-to-four samples
 * (2y + j, 2x + i, c), j, i in {0, 1}, of level k - 1 that lie inside level k - 1, keep those with v >= valid_min; with n their
 * number and S their sum the output is
 *   n == 0 ? 0 : (S + n / 2) / n      (integer division; n / 2 floored)
 * Exact integers: any evaluation order gives the same bytes.  With valid_min = 0 a full block is (S + 2) >> 2.  Every output
 * is 0 or >= valid_min, so data never becomes no data, and no data appears only where all inputs were no data.  A level is
 * defined from the level before it, as gdaladdo -r average does it, not from the image: a direct 2^k box differs by 1 DN on
 * about a quarter of the samples.
 * d_src: rows lines of w pixels of spp samples, src_pitch SAMPLES apart (a window inside a wider raster is allowed).  Output:
 * ceil(rows / 2) lines of ceil(w / 2) pixels, dst_pitch samples apart.  A strip cut into calls at even lines (each call
 * writing from output line first / 2 on) gives the bytes of one call.  Asynchronous on the context's stream.  OIP_E_INVALID for
 * spp other than 1 or 4, w < 1, rows < 0 or >= 2^31, valid_min outside 0..65535, a pitch shorter than its line, d_dst ==
 * d_src; rows == 0 is a no-op.  A source pitch that is not a multiple of 8 samples, or a source that does not start on a
 * 16-byte boundary, takes a slower kernel (a lane per output sample) with the same result. */
int oip_halve_u16(oip_ctx *ctx, const uint16_t *d_src, long src_pitch, int w, long rows, int spp, int valid_min,
                  uint16_t *d_dst, long dst_pitch);
/* host: the default level count of a w x h image, the smallest n >= 1 with ceil(w / 2^n) <= 256 and ceil(h / 2^n) <= 256,
 * at most 16.  No context needed. */
int oip_overview_levels(int w, long h);

/* ---- cog: tiled TIFF with internal overviews, and tiled TIFF input (`oip cog`; not in the reference) ---- */
#define OIP_COG_SUFFIX ".COG"   /* <stem>.COG.TIFF, built like the reference's other product names (imageop.h:99-108) */
#define OIP_COG_DEF_TILE   256   /* --tile at 1 sample per pixel */
#define OIP_COG_DEF_TILE_4 128   /* ... at 4: a 256 x 256 x 4 tile is 512 KiB for one lane of the LZW encoder, 3.3 x the time of 128 */

/* The tile-major form of an image, and back.
 * Grid.  An image is w x h pixels of spp samples (1, or 4 pixel-interleaved), u16.  Tiles are T x T pixels, T a multiple of 16 in
 * 16..1024.  The grid has tx = ceil(w / T) by ty = ceil(h / T) tiles, numbered row-major: tile (j, i) is number k = j tx + i.
 * Tile-major form.  ty tx consecutive blocks of T rows of T spp samples (T T spp samples a tile, no gaps).  Sample (r, c, ch) of
 * tile (j, i) is image sample
 *   (min(j T + r, h - 1), min(i T + c, w - 1), ch)
 * so the part of an edge tile outside the image replicates the last column, per channel, and the last line; nothing is
 * zero-filled (with TIFF's predictor 2 the replicated columns code to runs of zeros, and a reader that ignores the padding sees
 * nothing of it).  Every byte of the tile-major buffer is defined: oip_retile_u16 writes every sample of every tile it is asked for.
 * Inverse.  oip_untile_u16 writes exactly the w x h x spp samples of the image (the rows of the selected tile rows) and ignores
 * the padding, whatever it holds; the slack of a pitched destination is not touched.
 * Batches.  tile_row0 / tile_rows select tile rows [tile_row0, tile_row0 + tile_rows) of the grid; d_tiles then holds only that
 * range: tile (j, i) lies at d_tiles + ((j - tile_row0) tx + i) T T spp.  d_img is always the image's first line.  Any cut of
 * the grid into calls gives the bytes of one call.
 * d_img: lines `pitch` SAMPLES apart (a window inside a wider raster is allowed).  d_tiles: 16-byte aligned.  A raster whose
 * pitch is not a multiple of 8 samples, or that does not start on a 16-byte boundary, takes a slower kernel (a lane per sample)
 * with the same result.  Asynchronous on the context's stream.  OIP_E_INVALID for spp other than 1 or 4, w < 1, h < 1 or >= 2^31,
 * w spp >= 2^31, T not a multiple of 16 in 16..1024, a pitch shorter than the line, tile rows outside the grid, a NULL or
 * misaligned pointer, d_img == d_tiles; tile_rows == 0 is a no-op.
 * The file `oip cog` writes (TiffTiledWriterU16, csrc/oip_tifftiled.hpp), little-endian, classic or BigTIFF (BigTIFF when the
 * worst-case sum of all payloads would pass 4 GiB, or with OIP_TIFF_FORCE_BIG): (1) the header; (2) directory 0, the image, then
 * directories 1 .. n, levels 1 .. n of the pyramid above with NewSubfileType (254) = 1, chained by their next-directory offsets,
 * each followed by its own out-of-line values (BitsPerSample and SampleFormat where they do not fit the entry, TileOffsets,
 * TileByteCounts); (3) from an even offset, the tiles of the image in tile order, then those of level 1, 2, .. n, every tile on
 * an even offset.  A tile is the T T spp samples of the tile-major form, uncompressed or one LZW stream with predictor 2 along
 * each of its rows.  Tags: those of a strip product of the same geometry and spp, with 322, 323, 324, 325 in place of 273, 278, 279. */
int oip_retile_u16(oip_ctx *ctx, const uint16_t *d_img, long src_pitch_samples, int w, long h, int spp, int T, long tile_row0,
                   long tile_rows, uint16_t *d_tiles);
int oip_untile_u16(oip_ctx *ctx, const uint16_t *d_tiles, int w, long h, int spp, int T, long tile_row0, long tile_rows,
                   uint16_t *d_img, long dst_pitch_samples);

/* ---- rescale: antialiased resampling of a strip or product to another pixel grid (`oip rescale`; not in the reference) ----
 * A separable polyphase filter: one table of Q14 taps per axis, built on the host, lines first, then across the line.  Exact
 * integers on the device: any tile, any launch geometry and any cut of the output into windows give the same bytes.
 * Lanczos-3 and Q14 taps are conventions; nothing was measured on real imagery. */
#define OIP_RESCALE_SUFFIX ".RSC"      /* <stem>.RSC.<ext> */
#define OIP_RESCALE_LANCZOS 0          /* Lanczos-3, a = 3 (the default) */
#define OIP_RESCALE_CUBIC   1          /* Keys' cubic with -0.5, a = 2 */
#define OIP_RESCALE_LINEAR  2          /* the triangle, a = 1 */

/* The tap table of an axis that goes from n_in to n_out samples.  Host, no context needed.
 *   h(x): lanczos  x = 0: 1,  |x| < 3: (sin(pi x) / (pi x)) (sin(pi x / 3) / (pi x / 3)),  else 0
 *         cubic    |x| <= 1: 1.5 |x|^3 - 2.5 |x|^2 + 1,  |x| < 2: -0.5 |x|^3 + 2.5 |x|^2 - 4 |x| + 2,  else 0
 *         linear   max(0, 1 - |x|)
 * On reduction the kernel is stretched by n_in / n_out, which is the antialiasing.  For output index o, in this order:
 *   1. num = (2 o + 1) n_in - n_out,  den = 2 n_out              (pixel centres: the centre of o lies at num / den)
 *   2. K = 2 ceil(a max(n_in, n_out) / n_out), in integers        (the same for every o; 2 .. 24)
 *   3. first[o] = floor(num / den) - K / 2 + 1
 *   4. w_k = h((2 n_out (first[o] + k) - num) / (2 max(n_in, n_out))),  k = 0 .. K - 1: one fp64 division of two integers
 *   5. t_k = floor(w_k / S * 16384 + 0.5),  S = w_0 + w_1 + ... in that order
 *   6. 16384 - sum t_k is added to the largest t_k, among equal ones to the first
 * taps[o * K + k] = t_k, int16 in Q14; every row sums to exactly 16384; equal sizes give rows 0 0 16384 0 0 0 (lanczos).
 * first[] may point before the axis or reach beyond it: indices are clamped where they are used.  *K receives K; with first
 * and taps both NULL that is all the call does.  cap: the int16 values taps has room for.
 * OIP_E_INVALID: an unknown kind, an empty axis, an axis of 2^31 or more, n_in > 4 n_out (K would pass 24: halve with
 * `oip overviews` first), n_out > 16 n_in, one table NULL, cap < n_out K.  OIP_E_RUNTIME: a row with sum |t_k| > 32767 (the three
 * kinds stay below 25 300).  err (may be NULL) receives the text. */
int oip_rescale_taps(int kind, long n_in, long n_out, int *first, int16_t *taps, size_t cap, int *K, char *err, int errlen);

/* n_out = floor(n_in p / q + 1/2) for a scale p / q, in exact integers.  Host.  OIP_E_INVALID: n_in, p or q below 1, a result of
 * 2^31 or more.  A result of 0 is returned as such (and refused as an empty axis later). */
int oip_rescale_size(long n_in, long p, long q, long *n_out);

/* The source samples [*src0, *src0 + *srcs) that the outputs [out0, out0 + outs) of an axis n_in -> n_out with rows of K taps
 * read: clamp(first[out0]) .. clamp(first[out0 + outs - 1] + K - 1), clamped to 0 .. n_in - 1.  What oip_rescale_u16 wants
 * resident of its lines.  outs == 0 gives an empty range.  Host.  OIP_E_INVALID: an axis below 1 or of 2^31 or more, K not
 * even in 2 .. 24, outputs outside [0, n_out). */
int oip_rescale_src_range(long n_in, long n_out, int K, long out0, long outs, long *src0, long *srcs);

/* The resampler.  The source is W pixels x L lines of spp samples (1, or 4 pixel-interleaved), lines W spp samples apart; d_src
 * holds its lines [src_row0, src_row0 + src_rows).  The output is Wo x Lo; d_dst receives its lines [out_row0, out_row0 +
 * out_rows), lines Wo spp samples apart.  d_first_x / d_taps_x (Wo rows of Kx) and d_first_y / d_taps_y (Lo rows of Ky): the
 * tables of oip_rescale_taps for W -> Wo and L -> Lo, on the device.  With s' = s - 32768, clampL / clampW to the image (the
 * replicate border), per channel (a horizontal neighbour is spp samples away), >> an arithmetic shift:
 *   v(y, xs)  = clamp((sum_k ty[y][k] s'(clampL(fy[y] + k), xs) + 8192) >> 14, -32768, 32767)
 *   out(y, x) = clamp(((sum_k tx[x][k] v(y, clampW(fx[x] + k)) + 8192) >> 14) + 32768, 0, 65535)
 * The intermediate is clamped to 16 bits, so every operand fits 16 bits; |sum| <= sum |t| * 32768 < 2^31 for any int16 rows with
 * sum |t| <= 65535.  A constant image maps to itself; equal sizes give the input's bytes.
 * No data.  valid_min == 0 switches the rule off.  Otherwise an output sample whose footprint -- the clamped index ranges
 * clampL(fy[y] .. fy[y] + Ky - 1) x clampW(fx[x] .. fx[x] + Kx - 1) of its channel, whatever the taps are -- holds a source
 * sample below valid_min takes the nearest source sample instead:
 *   src[floor((2 y + 1) L / (2 Lo))][floor((2 x + 1) W / (2 Wo))]
 * so no data stays no data and nothing rings across the edge of a fill.  A raster without such samples gives the bytes of
 * valid_min == 0.
 * Windows.  The call needs the source lines oip_rescale_src_range(L, Lo, Ky, out_row0, out_rows) states; any cut of the output
 * lines into calls gives the bytes of one call.  Lines and offsets are 64-bit.  One launch per call; asynchronous on the
 * context's stream.  Lines that are not multiples of 8 samples, or bases that are not on 16-byte boundaries, take 2-byte
 * loads (source) or stores (output) in the same kernel, with the same result.
 * OIP_E_INVALID: a NULL or odd pointer, d_dst == d_src, spp not 1 or 4, a size below 1, L or Lo or a line of 2^31 or more, K not
 * even in 2 .. 24, W > 4 Wo, Wo > 16 W (and the same for lines), valid_min outside 0..65535, windows outside their rasters, a
 * source window that does not hold the lines needed ("source lines [a, b] needed, [c, d) resident").  out_rows == 0 is a
 * no-op.  Tables that oip_rescale_taps did not build are not checked: they give unspecified samples, never an access outside
 * the rasters. */
int oip_rescale_u16(oip_ctx *ctx, const uint16_t *d_src, long src_row0, long src_rows, int W, long L, int spp, uint16_t *d_dst, long out_row0,
                    long out_rows, int Wo, long Lo, const int *d_first_x, const int16_t *d_taps_x, int Kx, const int *d_first_y,
                    const int16_t *d_taps_y, int Ky, int valid_min);

/* ---- regcheck: tile-matching registration check of two rasters (`oip regcheck`; not in the reference) ---- */
/* Dense template matching by zero-mean normalised cross-correlation in the spatial domain, built from exact integer sums: a
 * measure of registration that shares no code with the phase correlation it judges.
 * Planes.  A is the reference image, B the sensed one; both u16, w x rows samples, given as a base pointer, a pitch in
 * SAMPLES and a sample stride of 1 or 4 (4: one band of a pixel-interleaved 4-sample raster, base + band):
 *   A(y, x) = d_a[y * pitch_a + x * stride_a].
 * Tiles.  Tile (j, i), 0 <= j < ny, 0 <= i < nx, has its T x T template at (ty, tx) = (y0 + j * step_y, x0 + i * step_x) in A;
 * T a multiple of 8, 8 <= T <= 128.  For every offset (dy, dx) in [-S, S]^2, 1 <= S <= 16, B's window at (ty + dy, tx + dx).
 * Sums over the n = T^2 samples, exact in 64 bits (sum a b < 2^46 at T = 128):
 *   sa = sum a, saa = sum a^2                    once per tile
 *   sb = sum b, sbb = sum b^2, sab = sum a b     per offset
 *   bad_a, bad_b: the samples outside [valid_min, valid_max] in the template and in B's whole (T + 2S)^2 search window
 *   num = n sab - sa sb,  va = n saa - sa^2,  vb = n sbb - sb^2        (all fit int64)
 *   score = (double)num / sqrt((double)va * (double)vb);  no score (-2) where va <= 0 or vb <= 0
 * Peak: the largest score; among equal ones the first offset in row-major order (dy, then dx); the offset (0, 0) where no
 * offset has a score.  (dx, dy) is where A's template is found in B, relative to its own position.
 * Record of tile j * nx + i, OIP_MATCH_RECORD_WORDS uint64:
 *   0 sa   1 saa   2 bad_a   3 bad_b   4 peak index (dy + S) * (2S + 1) + (dx + S)
 *   5..19 (sb, sbb, sab) at the peak, then at its left (dx - 1), right (dx + 1), upper (dy - 1) and lower (dy + 1) neighbour;
 *         three zeros for a neighbour outside the range
 * d_sums, if not NULL, receives (sb, sbb, sab) of every offset of every tile: nx * ny * (2S + 1)^2 * 3 uint64, tile-major,
 * offsets in row-major order.  Everything else -- scores, sub-pixel offsets, flags -- is computed on the host from the
 * record's integers (oip_match_peak).  Asynchronous on the context's stream.
 * OIP_E_INVALID: T or S out of range, a stride other than 1 or 4, w, rows, nx, ny, step_x or step_y < 1, a pitch shorter than
 * (w - 1) * stride + 1, valid_min > valid_max or outside 0..65535, a NULL or odd plane or record pointer, nx * ny >= 2^31,
 * or any search window that leaves w x rows: x0 < S, y0 < S, x0 + (nx - 1) step_x + T + S > w or the same in y. */
#define OIP_MATCH_RECORD_WORDS 20
#define OIP_MATCH_MIN_T 8
#define OIP_MATCH_MAX_T 128
#define OIP_MATCH_MAX_S 16
#define OIP_MATCH_NO_SCORE (-2.0)
#define OIP_MATCH_NODATA 1      /* bad_a + bad_b > 0 */
#define OIP_MATCH_FLAT   2      /* no offset has a score */
#define OIP_MATCH_EDGE   4      /* |dy| = S or |dx| = S at the peak */
#define OIP_MATCH_WEAK   8      /* score < min_score */
#define OIP_MATCH_MASKED 16     /* `oip regcheck --mask`: the template's footprint touches a masked cell (oip_mask_tile_flag); OR-ed in on the host */
#define OIP_REGCHECK_SUFFIX ".REG"
int oip_match_tiles_u16(oip_ctx *ctx, const uint16_t *d_a, long pitch_a, int stride_a, const uint16_t *d_b, long pitch_b,
                        int stride_b, int w, long rows, int T, int S, int x0, long y0, int step_x, long step_y, int nx, long ny,
                        int valid_min, int valid_max, uint64_t *d_records, uint64_t *d_sums);
/* host: the grid of step `step` whose search windows lie inside w x rows: x0 = y0 = S, nx = (w - 2S - T) / step + 1 and ny
 * likewise.  OIP_E_INVALID (and nx = ny = 0) for T, S out of range, step < 1, or an image that holds no tile.  No context. */
int oip_match_grid(int w, long rows, int T, int S, int step, int *x0, long *y0, int *nx, long *ny);
/* host: shift, score and flags of one record.  The score is the peak's; per axis the shift is the peak's integer offset plus
 *   f = (l - r) / (2 (l - 2 c + r))     l, c, r: the scores of the left (upper) neighbour, the peak, the right (lower) one
 * clamped to +-0.5 -- the vertex of the parabola through the three -- only where the peak is off the range's border on that
 * axis, all three have a score and the denominator is negative; f = 0 otherwise.  flags: the OIP_MATCH_ bits above.
 * OIP_E_INVALID for T, S out of range or a peak index >= (2S + 1)^2.  No context. */
int oip_match_peak(const uint64_t *record, int T, int S, double min_score, double *dx, double *dy, double *score, int *flags);
/* host: over the n_ok of n tiles whose flags are 0, out[8] = n_ok, mean dx, mean dy, their standard deviations (population),
 * the RMS of the radial error r = sqrt(dx^2 + dy^2), its nearest-rank 90th percentile (CE90: the ceil(0.9 n_ok)-th smallest)
 * and its maximum; all zero where n_ok = 0.  No context. */
int oip_match_summary(const double *dx, const double *dy, const int *flags, long n, double *out);

/* ---- regfix: resampling of a raster by the shift field regcheck measured (`oip regfix`; not in the reference) ----
 * The reference's geometric models are a constant shift per CCD pair and, per MSS band, a polynomial in the column alone; this
 * is the resampler that takes a field.  Everything is integer except the 16-tap sum.
 * Field.  A lattice of nx x ny nodes, nx, ny >= 1, nx * ny <= 2^27, at pixel (gx0 + i * sx, gy0 + j * sy) of the raster to be
 * resampled; steps 1 <= sx, sy <= OIP_WARP_MAX_STEP; gx0, gy0 any value.  Node (j, i) carries NX[j * nx + i] and NY[j * nx + i],
 * int32 in Q10 (1/1024 px), |value| <= OIP_WARP_MAX_Q10 (64 px).
 * Per axis (x shown; y the same with gy0, sy, ny):
 *   p = x - gx0;  ci = clamp(floor(p / sx), 0, nx - 2);  t = clamp(p - ci * sx, 0, sx);  wx = (t * 4096 + sx / 2) / sx   (Q12)
 *   with one node on the axis ci = 0, wx = 0 and node ci + 1 is never read.  Outside the lattice the edge value holds.
 * Per output sample, y first, then x, with lerp(a, b, w) = a + (((b - a) * w + 2048) >> 12) (arithmetic shift; every product
 * fits int32), for N = NX and N = NY alike:
 *   R[i] = lerp(N[cj][i], N[cj + 1][i], wy);   d = lerp(R[ci], R[ci + 1], wx);   s = 32 * coordinate + ((d + 16) >> 5)   (1/32 px)
 * Sampling is cv::remap(INTER_CUBIC, BORDER_CONSTANT 0) as csrc/oip_bicubic.h states it: first tap X = (s_x >> 5) - 1, phase
 * s_x & 31, the same in y, w = wy * wx as one f32 product, the interior and the border summation order,
 * saturate_cast<ushort>(cvRound(sum)), nothing contracted.  There is no `short` saturation of coordinates and there are no
 * sections: the source is the whole W x L raster.  The convention is regcheck's: out(y, x) = src(y + dy, x + dx).
 * Raster and window conventions are oip_convolve_u16's; spp 1 or 4 (pixel-interleaved); band_mask: bit c set for the channels
 * that are resampled, 1 <= band_mask < 2^spp; the other channels are copied through.  nodes_x / nodes_y are host arrays, copied
 * during the call.  OIP_E_INVALID: a value outside the stated ranges, a NULL or odd pointer, d_dst == d_src, output lines
 * outside [0, L), a source line that oip_warp_grid_src_range names and that is not resident.  out_rows == 0 is a no-op.
 * Asynchronous on the context's stream; lines and pitches in 64 bits. */
#define OIP_WARP_MAX_STEP 65536
#define OIP_WARP_MAX_Q10 65536
#define OIP_REGFIX_SUFFIX ".REGFIX"
#define OIP_REGFIX_MAX_SMOOTH 16
int oip_warp_grid_bicubic_u16(oip_ctx *ctx, const uint16_t *d_src, long src_row0, long src_rows, uint16_t *d_dst, long out_row0,
                              long out_rows, int W, long L, int spp, int band_mask, const int32_t *nodes_x, const int32_t *nodes_y,
                              int nx, int ny, long gx0, long gy0, int sx, int sy);
/* host: source lines [first, last), inside [0, L), that contain every source line output lines [out_row0, out_row0 + out_rows)
 * read (0, 0 if none): from the extremes of NY over the node lines those output lines lie between, so a few lines more than a
 * pixel-by-pixel count.  include_output != 0: the output lines themselves as well (a band_mask that copies channels through
 * reads them).  OIP_E_INVALID for arguments out of range or a node above 64 px in those node lines.  No context needed. */
int oip_warp_grid_src_range(long out_row0, long out_rows, long L, const int32_t *nodes_y, int nx, int ny, long gy0, int sy,
                            int include_output, long *first, long *last);

/* host, no context needed: the field of `oip regfix` from a regcheck report (csrc/oip_warpfield.hpp; tests/_regfix_ref.py
 * restates all three).
 * oip_regfix_load_report: the `# oip regcheck ...` line gives scale, shift-x, shift-y and band2 as key=value tokens; the tile
 *   lines x,y,dx,dy,score,flags must form a row-major regular lattice with x and y divisible by scale.  Node (j, i) lies at
 *   (x / scale - shift-x, y / scale - shift-y) in image-2 pixels and carries rint(d * 1024) (fp64, ties to even) where
 *   flags == 0; the other nodes are filled by oip_regfix_fill.  geom[8] = nx, ny, gx0, gy0, sx, sy, band2, tiles used.  nx * ny
 *   may not exceed cap (nodes_x / nodes_y: room for cap values each); a step on an axis with one node is 1.  w, h > 0: the image
 *   the field is for -- a node outside [0, w) x [0, h) is an error; 0: not checked.  OIP_E_IO when the file cannot be read,
 *   OIP_E_INVALID (err says why) for a missing header token, a ragged or irregular lattice, a number that is not finite, a value
 *   above 64 px, a node outside the image, no usable tile.
 * oip_regfix_fill: set[q] != 0 marks the nodes that carry a value.  In passes, every unset node with k >= 1 set 4-neighbours as
 *   of the pass's start gets floor((2 * sum + k) / (2 k)) per component and becomes set; until none is left.  OIP_E_INVALID if no
 *   node is set.
 * oip_regfix_smooth: `passes` (0 .. OIP_REGFIX_MAX_SMOOTH) times [1 2 1] along the node lines, then across them, with replicated
 *   edges: (a + 2 b + c + 2) >> 2, arithmetic shift. */
int oip_regfix_load_report(const char *path, long w, long h, int32_t *nodes_x, int32_t *nodes_y, long cap, long *geom, char *err, int errlen);
int oip_regfix_fill(int32_t *nodes_x, int32_t *nodes_y, const uint8_t *set, int nx, int ny);
int oip_regfix_smooth(int32_t *nodes_x, int32_t *nodes_y, int nx, int ny, int passes);

/* ---- pansharpen: fusion of the PAN strip with the aligned MSS product (`oip pansharpen`; not in the reference) ----
 * Smoothing-filter intensity modulation, fused_b = up(MSS_b) * PAN / up(low(PAN)), stated to the bit; tests/_pansharpen_ref.py
 * restates it.  P: PAN, W x Hp u16.  M: the MSS product, w x h pixels of 4 pixel-interleaved u16 samples.  off >= 0: the first
 * PAN line used.  W = 4 w; hh = min(h, (Hp - off) / 4) >= 1 MSS lines are used; the product is 4 w x 4 hh x 4 u16,
 * pixel-interleaved.  MSS pixel (j, i) covers PAN pixels (off + 4 j .. off + 4 j + 3, 4 i .. 4 i + 3), regcheck --scale 4's
 * convention.
 * 1. Lm (w x hh) = (S + 8) >> 4 of the 4 x 4 PAN block: oip_decimate_box_u16 with factor 4 on full blocks.
 * 2. Up-sampling by 4, the same for each band of M and for Lm.  Output coordinate x: cell i = x >> 2, phase r = x & 3; first tap
 *    c0 = i - 2 for r in {0, 1}, i - 1 for r in {2, 3}; taps clamp(c0 + k, 0, n - 1), k = 0 .. 3.  Weights: the OpenCV cubic
 *    (a = -0.75) at t = 5/8, 7/8, 1/8, 3/8 times 2048, exact integers, each row summing to 2048:
 *      r=0: -135  873 1535 -225      r=1: -21  235 1981 -147      r=2: -147 1981  235  -21      r=3: -225 1535  873 -135
 *    along the lines  Hq = (sum wx[k] s[k] + 128) >> 8   (arithmetic shift; 3 fractional bits), then across them, same indexing,
 *    U = clamp((sum wy[k] Hq[k] + 1024) >> 11, 0, 8 * 65535).  Everything fits int32 (|Hq| <= 616439, 616439 * 2768 + 1024 <
 *    2^31) and both operands of every product fit 24 signed bits.
 * 3. Modulation in IEEE single precision, every operation rounded on its own, nothing contracted.  UL = U(Lm), U_b = U(M_b), both
 *    exact in f32.  g = UL == 0 ? 0.125f : min(__fdiv_rn((float)P, (float)UL), gmax), gmax = (float)max_gain * 0.125f;
 *    out_b = saturate_u16(rintf(__fmul_rn((float)U_b, g))), ties to even.  One division per pixel, shared by the four bands.
 * 4. Counters: pixels with UL == 0; pixels whose quotient was above gmax.
 * oip_pansharpen_sfim_u16: d_mss and d_low are the WHOLE low-resolution rasters (w x h; h is the hh above), d_pan and d_dst point
 * at output line out_row0 of their rasters -- a caller can stream PAN and product in line blocks; any out_row0 / out_rows with
 * 0 <= out_row0, out_row0 + out_rows <= 4 h, multiples of 4 or not; out_rows == 0 is a no-op.  Pitches in SAMPLES; lines and
 * offsets in 64 bits.  d_stats: NULL, or two uint64 on the device that the two counters of the call's pixels are ADDED to.
 * Asynchronous on the context's stream.  OIP_E_INVALID: a NULL or odd pointer, a pitch shorter than its line (4 w, 4 w, w,
 * 16 w), w or h < 1, lines outside [0, 4 h), max_gain outside [1, OIP_PANSHARPEN_MAX_GAIN], a product that overlaps an input.
 * A PAN or MSS base off an 8-byte boundary or pitch off a multiple of 4 samples, or a product off a 16-byte boundary or a pitch
 * off a multiple of 8, takes a slower kernel (2-byte accesses) with the same bytes. */
#define OIP_PANSHARPEN_SUFFIX ".PSH"
#define OIP_PANSHARPEN_DEF_GAIN 4
#define OIP_PANSHARPEN_MAX_GAIN 64
int oip_pansharpen_sfim_u16(oip_ctx *ctx, const uint16_t *d_pan, long pan_pitch, const uint16_t *d_mss, long mss_pitch,
                            const uint16_t *d_low, long low_pitch, int w, long h, uint16_t *d_dst, long dst_pitch, long out_row0,
                            long out_rows, int max_gain, uint64_t *d_stats);
/* host, no context needed: the geometry rule above.  out_w = 4 w, out_h = 4 hh, mss_lines = hh (each may be NULL).
 * OIP_E_INVALID for W != 4 w, w or h < 1, a negative line_offset, fewer than 4 PAN lines from line_offset on. */
int oip_pansharpen_geometry(long W, long Hp, long w, long h, long line_offset, long *out_w, long *out_h, long *mss_lines);

/* ---- instrumentation --------------------------------------------------------------- */
/* name + accumulated device time of the kernels launched through this context since the
 * last reset, measured with HIP events on the context's stream (off by default). */
/* ---- 8f rank 4: sub-image merge of the down-link de-framer ------------------------------------------
 * AuxSeparator::WriteImageData / MergeSubImage / the byte-order pass of InflateSubImage
 * (aux_separator.h:341-393) for uncompressed frames: d_tiles holds vparts*hparts sub-images of
 * sub_lines x sub_cols BIG-endian u16, tile r*hparts + c after tile r*hparts + c - 1; d_out receives
 * vparts stripes of sub_lines lines of hparts*sub_cols little-endian pixels
 * (reference frame: vparts = 4 PAN + 1 MSS, hparts = 8, 256 x 1536 sub-images).  Not in place. */
int oip_merge_subimages_be16(oip_ctx *ctx, const uint16_t *d_tiles, uint16_t *d_out, int vparts, int hparts,
                             int sub_lines, int sub_cols);

int oip_profile_enable(oip_ctx *ctx, int on);
int oip_profile_reset(oip_ctx *ctx);
/* Time only the kernels profiled under this name (NULL or "": every kernel).  The events themselves cost
   stream time (about 2 % of a correlation batch when every kernel is timed). */
int oip_profile_filter(oip_ctx *ctx, const char *kernel_name);
int oip_profile_count(oip_ctx *ctx);
int oip_profile_get(oip_ctx *ctx, int i, char *name, int namelen, double *total_ms, long *launches);

#ifdef __cplusplus
}
#endif
#endif /* OIP_C_H */
