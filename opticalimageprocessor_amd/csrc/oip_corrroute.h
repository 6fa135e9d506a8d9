// oip_corrroute.h -- the host planning arithmetic of the correlation drivers (phasecorr.hip): the switches of the environment,
// which of four routes an inter-band geometry takes, the FFT plans of its arrays, the geometry of the peak search and of the row
// stage's stored window, and where every array lies in the workspace.  Nothing of HIP in here: phasecorr.hip plans, carves
// and launches by these lines, oip_corr_route_describe (include/oip_c.h) states them, and tests/cpp/corrroute_test.cpp runs them
// on the CPU.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "oip_fftplan.h"

namespace oipcorr {

using oipfftplan::kPlanOk;
using oipfftplan::kPlanUnsupported;

// row lengths with a fused row stage (corr_rows_kernel; kFusedRow of phasecorr.hip has one entry per length).  The first is
// also the one length of corr_rows_up_kernel (kUpRowsN / 4-point band rows), the second the one of corr_rows_v_kernel.
constexpr int kUpRowsN = 3000, kUpRowsBandN = kUpRowsN / 4, kVRowsN = 1250, kStitchRowsN = 200;
inline bool fused_row_exists(int N) { return N == kUpRowsN || N == kVRowsN || N == kStitchRowsN; }
// The row stage stores only the columns of the lane tiles 0 .. R and T - R .. T - 1 (inter-band shifts are a few PAN
// pixels: the surfaces peak in tile 0 or across the wrap), R = OIP_ROWS_WINDOW or this; see correlate_units_up.
constexpr int kRowsWindowTiles = 8;
constexpr int kSelCols = 64, kSelMaxTiles = 1024;       // col_sel_first_kernel: columns per workgroup, tiles its LDS holds
constexpr int kMaxLines = 65535;                        // grid.y of the row-walking kernels

inline int optimal_dft_size(int n)
{
    // cv::getOptimalDFTSize: smallest 2^a 3^b 5^c >= n
    long best = -1;
    for (long p5 = 1; p5 < 2L * n + 1; p5 *= 5)
        for (long p35 = p5; p35 < 2L * n + 1; p35 *= 3) {
            long v = p35;
            while (v < n) v *= 2;
            if (best < 0 || v < best) best = v;
        }
    return (int)best;
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// a window of radius r exists for the tile lists of a search: tiles of whole pieces (two columns), and the two arms do not meet
inline bool rows_window_fits(bool lists, int vshift, int T, int r) { return r >= 0 && lists && vshift >= 1 && 2 * r + 1 < T; }

// ---- the switches of the environment, each read once per correlation call (CorrKnobs::from_env at the extern "C" entries)
struct CorrKnobs {
    int spectral_up = 2;                    // OIP_SPECTRAL_UP: 0 = image domain, 1 = horizontal axis on the spectra, 2 = both axes
    bool spectral_v = true;                 // OIP_SPECTRAL_V=0: the 1250-point geometry keeps the image-domain route
    bool fused_rows = true;                 // OIP_FUSED_ROWS=0: forward row passes, cross_power_kernel, inverse row passes
    bool peak_prune = true;                 // OIP_PEAK_PRUNE=0: the search lists every tile, so every column is stored
    int rows_window = kRowsWindowTiles;     // OIP_ROWS_WINDOW: radius of the stored window in lane tiles, 0 stores every column
    bool window_poison = false;             // OIP_ROWS_WINDOW_POISON=1 (debug): the output arrays are NaN before the row stage
    bool v_generic = false;                 // OIP_V_GENERIC=1 (test): the generic vertical up-sampling kernel

    static CorrKnobs from_env()
    {
        CorrKnobs k;
        auto num = [](const char *name, int unset) { const char *e = getenv(name); return e ? atoi(e) : unset; };
        k.spectral_up = num("OIP_SPECTRAL_UP", 2);
        k.spectral_v = num("OIP_SPECTRAL_V", 1) != 0;
        k.fused_rows = num("OIP_FUSED_ROWS", 1) > 0;
        k.peak_prune = num("OIP_PEAK_PRUNE", 1) != 0;
        k.rows_window = num("OIP_ROWS_WINDOW", kRowsWindowTiles);
        k.window_poison = num("OIP_ROWS_WINDOW_POISON", 0) > 0;
        k.v_generic = num("OIP_V_GENERIC", 0) != 0;
        return k;
    }
    bool operator==(const CorrKnobs &o) const
    {
        return spectral_up == o.spectral_up && spectral_v == o.spectral_v && fused_rows == o.fused_rows && peak_prune == o.peak_prune &&
               rows_window == o.rows_window && window_poison == o.window_poison && v_generic == o.v_generic;
    }
};

// ---- cv::hal::resize coefficient set-up (resize.cpp), on the host in the same float/double mix ---------------------------
// OpenCV imgwarp.cpp interpolateCubic, f32, evaluated exactly as OpenCV does (x86-64, no contraction: every TU is built with
// -ffp-contract=off)
inline void interpolate_cubic(float x, float *c)
{
    const float A = -0.75f;
    c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    c[3] = 1.f - c[0] - c[1] - c[2];
}
// one axis s -> d: ofs[i] is the source index of output i's second tap, coef[4 i ..] its four taps (null: offsets only)
inline void resize_axis(int s, int d, std::vector<int> *ofs, std::vector<float> *coef)
{
    const double scale = 1. / ((double)d / s);
    ofs->resize((size_t)d);
    if (coef) coef->resize((size_t)d * 4);
    for (int i = 0; i < d; ++i) {
        float f = (float)((i + 0.5) * scale - 0.5);
        const int si = (int)floorf(f);
        f -= si;
        (*ofs)[i] = si;
        if (coef) interpolate_cubic(f, &(*coef)[(size_t)i * 4]);
    }
}
// the exact x4 forms of an axis: every output's first tap inside its source pixel's 5-wide window (the x4 kernel), and
// ofs[i] == (i - 2) >> 2 throughout (the FFT loader, the sliding-window vertical kernel and the operators on spectra)
inline bool axis_in_x4_window(const std::vector<int> &ofs)
{
    for (int i = 0; i < (int)ofs.size(); ++i) { const int o = (ofs[i] - 1) - (i / 4 - 2); if (o != 0 && o != 1) return false; }
    return true;
}
inline bool axis_is_x4(const std::vector<int> &ofs)
{
    for (int i = 0; i < (int)ofs.size(); ++i) if (ofs[i] != ((i - 2) >> 2)) return false;
    return true;
}
// The x4 up-sampling n -> N of an axis has a form as an operator on spectra (oip_upsample_operator builds it; its own
// refusals, taps that are not 4-periodic, cannot occur for offsets of the x4 form: the tap phases are k/8, exact in f32)
inline bool axis_has_spectral_form(int n, int N, const std::vector<int> &ofs) { return N == 4 * n && n >= 8 && axis_is_x4(ofs); }

// ---- the plan ---------------------------------------------------------------------------------------------------------
enum CorrRoute {
    kImage,         // both axes up-sampled in the image domain: resize_cubic_v_kernel, horizontal taps in the FFT loader
    kSpectralH,     // horizontal axis on the spectra of M x band_cols (`_quarter`) transforms of the vertically up-sampled bands
    kSpectralHV,    // both axes on the spectra of the band windows themselves (band_rows x cols, four arrays side by side)
    kSpectralV,     // 1250-point rows: horizontal taps in the image domain (hpack_bands_kernel), vertical axis on the spectra
};
inline const char *route_name(CorrRoute r) { return r == kImage ? "image" : r == kSpectralH ? "H" : r == kSpectralHV ? "HV" : "V"; }

// The workspace of a correlation call, in address order: `count` parts of `bytes` each from `offset`; count 0: not there
enum CorrRegionId { kRegBound, kRegLists, kRegZ, kRegY, kRegFa, kRegFb, kRegSmall, kRegSlots, kNumRegions };
constexpr const char *kRegionNames[kNumRegions] = {"bound", "lists", "z", "y", "fa", "fb", "fsmall", "slots"};
struct CorrRegion {
    size_t offset, bytes;
    int count;
    size_t part(int i) const { return offset + (size_t)i * bytes; }
    size_t end() const { return part(count); }
};
// an array that lives inside a part of a region, `offset` bytes from that part's start; bytes 0: not there
struct CorrSubRegion {
    CorrRegionId in;
    int part;
    size_t offset, bytes;
};

struct CorrPlan {
    CorrKnobs knobs;            // what it was planned for: the switches, the window and its band window
    CorrRoute route;
    int rows, cols, band_rows, band_cols;
    int M, N;                   // the DFT size of the window
    int cu_count;               // CUs of the device: the grid of the row stage
    OipFftHostPlan main;        // M x N
    OipFftHostPlan band;        // H: M x band_cols; HV: band_rows x cols; V: band_rows x 4 N; image: not used
    bool fused_rows;            // a fused row stage exists for N (and OIP_FUSED_ROWS does not forbid it)
    // peak search of the H and HV routes (PruneWork): workgroups of the row stage, lane tiles of the column passes, log2 of
    // their width, and whether the plan has the list form of its column passes (else the exhaustive passes run)
    int groups, T, vshift;
    bool lists;
    int win_r;                  // radius of the row stage's stored window, -1: every column is stored
    CorrRegion reg[kNumRegions];
    CorrSubRegion band_sub;     // the band array(s): in z[1]
    CorrSubRegion raw_sub;      // the raw edge rows: behind the band array in z[1] (HV), or fsmall (V)
    size_t total;
};

// bytes of the list storage of a search over T tiles: bt [4][T] f32, flags [4][T], count [16], ticket [8], tiles [16][T]
inline size_t prune_list_bytes(int T) { return sizeof(int) * ((size_t)(4 + 4 + 16) * T + 16 + 8); }

// lay the regions out: nz spectrum and ny output slots of the main array, 1 + nfb f32 images of f_elems, small_elems floats
inline void lay_out(CorrPlan *p, size_t f_elems, size_t small_elems, int nz, int ny, int nfb, bool prune)
{
    const OipFftHostPlan &pl = p->main;
    p->groups = p->T = p->vshift = 0;
    p->lists = false;
    size_t bbytes = 0, tbytes = 0;
    if (prune) {
        p->groups = p->cu_count < pl.M / 2 + 1 ? p->cu_count : pl.M / 2 + 1;        // the row stage's grid
        p->T = pl.passes[0].lane_tiles;
        p->vshift = pl.passes[0].vshift;
        bbytes = align_up(sizeof(float) * (size_t)p->groups * 4 * pl.P, 256);
        p->lists = oipfftplan::col_list_ok(pl, 4) && (1 << p->vshift) <= kSelCols && p->T <= kSelMaxTiles;
        if (p->lists) tbytes = align_up(prune_list_bytes(p->T), 256);
    }
    const size_t zbytes = align_up(2 * sizeof(float) * (size_t)pl.M * pl.P, 256);
    const size_t fbytes = align_up(sizeof(float) * f_elems, 256);
    const size_t sizes[kNumRegions] = {bbytes, tbytes, zbytes, zbytes, fbytes, fbytes, align_up(sizeof(float) * (small_elems > 0 ? small_elems : 1), 256),
                                       align_up(sizeof(unsigned long long) * 4 * 2 * kPeakSlots, 256)};
    const int counts[kNumRegions] = {bbytes ? 1 : 0, tbytes ? 1 : 0, nz, ny, 1, nfb, 1, 1};
    size_t at = 0;
    for (int r = 0; r < kNumRegions; ++r) {
        p->reg[r] = CorrRegion{at, sizes[r], counts[r]};
        at = p->reg[r].end();
    }
    p->total = at;
    p->band_sub = p->raw_sub = CorrSubRegion{kRegZ, 1, 0, 0};
}
inline bool sub_fits(const CorrPlan &p, const CorrSubRegion &s) { return s.part < p.reg[s.in].count && s.offset + s.bytes <= p.reg[s.in].bytes; }

inline int refuse(char *why, size_t len, int code, const char *text) { snprintf(why, len, "%s", text); return code; }

// One pair of images of rows x cols (oip_phase_correlate_f32, the CCD-pair correlations): one spectrum slot, one output.
// `too_tall`: the caller's text for more than 65535 lines.
inline int plan_pair(int rows, int cols, const CorrKnobs &knobs, const char *too_tall, CorrPlan *p, char *why, size_t len)
{
    p->knobs = knobs;
    p->route = kImage;
    p->rows = rows; p->cols = cols; p->band_rows = p->band_cols = 0;
    p->M = optimal_dft_size(rows); p->N = optimal_dft_size(cols);
    p->win_r = -1;
    if (p->M > kMaxLines) return refuse(why, len, kPlanUnsupported, too_tall);
    if (int rc = oipfftplan::plan(p->M, p->N, &p->main, why, len)) return rc;
    p->fused_rows = knobs.fused_rows && p->main.xf.size() == 1 && fused_row_exists(p->N);
    p->cu_count = 0;
    lay_out(p, 1, 0, 1, 1, 0, false);
    return kPlanOk;
}

// The route of n inter-band units of rows x cols PAN against band_rows x band_cols bands, and its storage.  The conditions
// are tried in this order: HV, else H, else V, else the image domain -- a route whose arrays do not fit their slot falls back.
inline int plan_interband(int rows, int cols, int band_rows, int band_cols, int cu_count, const CorrKnobs &knobs, CorrPlan *p, char *why, size_t len)
{
    if (int rc = plan_pair(rows, cols, knobs, "oip_interband_correlate: more than 65535 correlation lines", p, why, len)) return rc;
    p->band_rows = band_rows; p->band_cols = band_cols;
    p->cu_count = cu_count;
    const int M = p->M, N = p->N, P = p->main.P;
    std::vector<int> xofs, yofs;
    resize_axis(band_cols, cols, &xofs, nullptr);
    resize_axis(band_rows, rows, &yofs, nullptr);
    // the band window up-sampled by exactly 4 fills the DFT's lines, and the bands' own height is a DFT size
    const bool exact4 = knobs.spectral_up > 0 && rows == 4 * band_rows && cols == 4 * band_cols && M == rows && p->fused_rows;
    const bool vaxis = optimal_dft_size(band_rows) == band_rows && band_rows >= 8 && axis_has_spectral_form(band_rows, rows, yofs);
    const size_t c8 = 2 * sizeof(float);
    // 3000 columns: the horizontal axis on the band spectra in the row stage (corr_rows_up_kernel), the vertical one too
    // where the band height allows
    if (exact4 && N == cols && N == kUpRowsN && axis_has_spectral_form(band_cols, cols, xofs)) {
        if (int rc = oipfftplan::plan(M, band_cols, &p->band, why, len)) return rc;
        if (4 * p->band.P <= P) {                   // the four narrow arrays share one array-sized slot
            p->route = kSpectralH;
            lay_out(p, (size_t)rows * band_cols, 0, 2, 4, 8, true);
            p->band_sub.bytes = 4 * c8 * (size_t)M * p->band.P;
            if (knobs.spectral_up > 1 && vaxis) {
                if (int rc = oipfftplan::plan(band_rows, cols, &p->band, why, len)) return rc;       // four arrays side by side
                p->route = kSpectralHV;
                p->band_sub.bytes = c8 * (size_t)band_rows * p->band.P;
                // raw16 [4 edge rows][4 arrays][band_cols] of (bX | bY << 16), one u32 a column, behind the band array
                p->raw_sub = CorrSubRegion{kRegZ, 1, p->band_sub.bytes, sizeof(unsigned) * 16 * (size_t)band_cols};
                if (knobs.rows_window > 0 && knobs.peak_prune && rows_window_fits(p->lists, p->vshift, p->T, knobs.rows_window)) p->win_r = knobs.rows_window;
            }
            if (sub_fits(*p, p->band_sub) && sub_fits(*p, p->raw_sub)) return kPlanOk;
        }
    }
    // the reference's own 12288-wide strips: 1228-column slices padded to 1250-point rows.  The horizontal taps stay in
    // the image domain (1250 is not 4 x the band width); the vertical axis (16000 = 4 x 4000) goes to the spectra
    // (corr_rows_v_kernel).
    if (knobs.spectral_v && exact4 && N == kVRowsN && (cols & 1) == 0 && vaxis && oipfftplan::smooth235(4L * N)) {
        if (int rc = oipfftplan::plan(band_rows, 4 * N, &p->band, why, len)) return rc;
        p->route = kSpectralV;
        lay_out(p, (size_t)rows * band_cols, 32 * (size_t)N, 2, 4, 8, false);
        p->band_sub.bytes = c8 * (size_t)band_rows * p->band.P;
        p->raw_sub = CorrSubRegion{kRegSmall, 0, 0, c8 * 16 * (size_t)N};       // [4 edge rows][4 arrays][N] complex
        if (sub_fits(*p, p->band_sub) && sub_fits(*p, p->raw_sub)) return kPlanOk;
    }
    // vertical taps as a kernel (u16 -> f32, rows x band_cols: the f32 scratch), horizontal taps inside the FFT loader
    p->route = kImage;
    p->win_r = -1;
    lay_out(p, (size_t)rows * band_cols, 0, 5, 2, 8, false);
    return kPlanOk;
}

// the kernels a route launches for its row stage and for bringing the bands into its arrays
inline const char *row_kernel(const CorrPlan &p)
{
    if (p.route == kSpectralV) return "corr_rows_v_kernel";
    if (p.route != kImage) return "corr_rows_up_kernel";
    return p.fused_rows ? "corr_rows_kernel" : "cross_power_kernel";
}
inline const char *pack_kernel(const CorrPlan &p)
{
    return p.route == kSpectralHV ? "pack_bands_kernel" : p.route == kSpectralV ? "hpack_bands_kernel" : "resize_cubic_v_kernel";
}

// A plan, or its refusal (rc and why of the planner), as one JSON object (include/oip_c.h: oip_corr_route_describe)
inline std::string describe(const CorrPlan &p, int rc, const char *why)
{
    char b[512];
    if (rc) {
        std::string s = "{\"refused\": \"";
        for (const char *c = why; *c; ++c) { if (*c == '"' || *c == '\\') s += '\\'; s += *c; }
        snprintf(b, sizeof b, "\", \"code\": %d}", rc);
        return s + b;
    }
    snprintf(b, sizeof b, "{\"route\": \"%s\", \"rows\": %d, \"cols\": %d, \"band_rows\": %d, \"band_cols\": %d, \"M\": %d, \"N\": %d, \"P\": %d, "
             "\"fused_rows\": %s, \"row_kernel\": \"%s\", \"pack_kernel\": \"%s\", ", route_name(p.route), p.rows, p.cols, p.band_rows, p.band_cols,
             p.M, p.N, p.main.P, p.fused_rows ? "true" : "false", row_kernel(p), pack_kernel(p));
    std::string s = b;
    if (p.route != kImage) {
        snprintf(b, sizeof b, "\"band\": {\"M\": %d, \"N\": %d, \"P\": %d}, ", p.band.M, p.band.N, p.band.P);
        s += b;
    }
    snprintf(b, sizeof b, "\"groups\": %d, \"tiles\": %d, \"tile_cols\": %d, \"lists\": %s, \"window\": %d, \"total\": %zu, \"regions\": [", p.groups,
             p.lists ? p.T : 0, p.lists ? 1 << p.vshift : 0, p.lists ? "true" : "false", p.win_r, p.total);
    s += b;
    for (int r = 0; r < kNumRegions; ++r) {
        snprintf(b, sizeof b, "%s{\"name\": \"%s\", \"offset\": %zu, \"bytes\": %zu, \"count\": %d}", r ? ", " : "", kRegionNames[r], p.reg[r].offset,
                 p.reg[r].bytes, p.reg[r].count);
        s += b;
    }
    s += "], \"inside\": [";
    const CorrSubRegion *subs[2] = {&p.band_sub, &p.raw_sub};
    for (int i = 0, n = 0; i < 2; ++i) {
        if (!subs[i]->bytes) continue;
        snprintf(b, sizeof b, "%s{\"name\": \"%s\", \"in\": \"%s\", \"part\": %d, \"offset\": %zu, \"bytes\": %zu}", n++ ? ", " : "", i ? "raw" : "band",
                 kRegionNames[subs[i]->in], subs[i]->part, subs[i]->offset, subs[i]->bytes);
        s += b;
    }
    return s + "]}";
}

}  // namespace oipcorr
