// oip_corrgeom.h -- the correlation-window geometry of the two strip work-flows as pure arithmetic: which lines and columns
// an inter-band unit (preproc.h:245-247, :257, :274-276, :284, :326) and a cross-CCD section (stitcher.h:151-152, :167,
// :175-176) read, the reference's argument checks in its wording (preproc.h:228-237, stitcher.h:75-77), the layout of the
// shift table, and the order in which the pipelined default action has the strip's lines arrive.  The C ABI's two whole-strip
// correlation calls (phasecorr.hip), the hosts of oip_host.hpp and the plans of oip_multigpu.hpp all take it from here.
// Nothing of HIP, the C ABI's calls or I/O in here: tests/cpp/corrgeom_test.cpp runs it on the CPU.
// (opticalimageprocessor_amd/dist.py keeps its own statement in Python: tests/test_dist_cpu.py compares the two.)
#pragma once

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "oip_c.h"                          // the reference's constants only

namespace OIPGPU {

// ---- inter-band units: `sections` x `slices` PAN windows, each against its four MSS band windows -------------------------
struct InterBandGeom {
    int W = 0, slices = 0, sections = 0, Wb = 0, n_units = 0;
    long Lp = 0, base_gap = 0, band_gap = 0;
    int base_rows = 0, base_cols = 0, band_rows = 0, band_cols = 0;

    InterBandGeom() = default;
    InterBandGeom(int W_, long Lp_, int slices_, int sections_, int corr_lines) : W(W_), slices(slices_), sections(sections_), Lp(Lp_)
    {
        base_rows = (int)std::min<long>(Lp, corr_lines);                              // preproc.h:245-247
        base_gap = (Lp - (long)base_rows * sections) / (sections + 1);
        base_cols = W / slices;
        band_rows = base_rows / OIP_MSS_BANDS;                                        // preproc.h:274-276: integer-divided by 4
        band_gap = base_gap / OIP_MSS_BANDS;
        band_cols = base_cols / OIP_MSS_BANDS;
        Wb = W / OIP_MSS_BANDS;
        n_units = sections * slices;
    }
    long pan_start(int sec) const { return base_gap + (long)sec * (base_rows + base_gap); }      // preproc.h:257
    long mss_start(int sec) const { return band_gap + (long)sec * (band_rows + band_gap); }      // preproc.h:284
    int centre_col(int unit) const { return (unit % slices) * base_cols + base_cols / 2; }       // preproc.h:326
    // The kernels take units two at a time, (2k, 2k+1), and a unit's last digits depend on its partner: the units that may be
    // computed once section `sec` is resident end at an even index, except behind the last section.
    int units_through(int sec) const { return sec == sections - 1 ? n_units : ((sec + 1) * slices) & ~1; }
};

// The reference's own argument checks (preproc.h:228-237) in its order: "" or the message.  Apart from the maker below,
// RunPipelined calls it: there these checks come first and its line-count check stands between them and the maker's others.
inline std::string InterBandArgCheck(long Lp, int slices, int sections, int corr_lines)
{
    if (slices < OIP_IBCV_MIN_SLICES) return "CalcInterBandCorrelation: at lease " + std::to_string(OIP_IBCV_MIN_SLICES) + " slice needed";
    if (sections <= 0) return "CalcInterBandCorrelation: section count should be a positive integer";
    if (sections > 1 && (long)sections * corr_lines > Lp)
        return "CalcInterBandCorrelation: too many sections (" + std::to_string(corr_lines) + " lines per section), not enough total PAN data lines";
    return "";
}
// The validating maker: the geometry into *g and "", or the message.  (The plans of oip_multigpu.hpp construct the geometry
// directly: they never had a minimum slice count, and say "too many sections" in fewer words.)
inline std::string MakeInterBandGeom(int W, long Lp, int slices, int sections, int corr_lines, InterBandGeom *g)
{
    if (W <= 0 || Lp <= 0 || corr_lines <= 0) return "oip_interband_correlate: bad argument";
    const std::string refused = InterBandArgCheck(Lp, slices, sections, corr_lines);
    if (!refused.empty()) return refused;
    *g = InterBandGeom(W, Lp, slices, sections, corr_lines);
    return g->band_rows <= 0 || g->band_cols <= 0 ? "oip_interband_correlate: slice too small" : "";
}

// ---- the shift table: [band][unit][dx, dy, rs, cx], what oip_filter_and_fit_mode takes -------------------------------------
// every unit not computed (yet, or on this rank): NaN shifts; cx is known from the geometry
inline void ShiftTableInit(const InterBandGeom &g, double *table)
{
    for (int b = 0; b < OIP_MSS_BANDS; ++b)
        for (int u = 0; u < g.n_units; ++u) {
            double *o = table + ((size_t)b * g.n_units + u) * 4;
            o[0] = o[1] = o[2] = NAN;
            o[3] = (double)g.centre_col(u);
        }
}
// one unit's result as the correlation calls return it, [band][dx, dy, rs], into its places
inline void ShiftTablePut(const InterBandGeom &g, double *table, int unit, const double *res)
{
    for (int b = 0; b < OIP_MSS_BANDS; ++b)
        for (int k = 0; k < 3; ++k) table[((size_t)b * g.n_units + unit) * 4 + k] = res[3 * b + k];
}

// ---- the order of arrival of the pipelined default action (PreProcessor::RunPipelined) -------------------------------------
// Per correlation section its MSS lines, then its PAN lines in blocks of at most pan_block_lines, then the section's units;
// the MSS lines between the sections (only the alignment reads them); the fit; the PAN lines between the sections last (no
// arithmetic of the action reads them: they are read and corrected as the reference does -- the strip's size is checked,
// --write-rrcpan wants them).  kMss / kPan: lines [a, b); kUnits: a = the section.
struct ArrivalItem {
    enum Kind { kMss, kPan, kUnits, kFit } kind;
    long a, b;
};

inline std::vector<ArrivalItem> ArrivalOrder(const InterBandGeom &g, long Lm, long pan_block_lines)
{
    std::vector<ArrivalItem> order;
    auto pan_blocks = [&](long a, long b) {
        for (long r = a; r < b; r += pan_block_lines) order.push_back({ArrivalItem::kPan, r, std::min(b, r + pan_block_lines)});
    };
    // the lines of [0, total) outside the sections' windows [start(sec), start(sec) + rows)
    auto between = [&](long total, long rows, auto start, auto emit) {
        long prev = 0;
        for (int sec = 0; sec <= g.sections; ++sec) {
            const long a = sec < g.sections ? start(sec) : total;
            if (prev < a) emit(prev, a);
            prev = a + rows;
        }
    };
    for (int sec = 0; sec < g.sections; ++sec) {
        order.push_back({ArrivalItem::kMss, g.mss_start(sec), g.mss_start(sec) + g.band_rows});
        pan_blocks(g.pan_start(sec), g.pan_start(sec) + g.base_rows);
        order.push_back({ArrivalItem::kUnits, sec, 0});
    }
    between(Lm, g.band_rows, [&](int sec) { return g.mss_start(sec); }, [&](long a, long b) { order.push_back({ArrivalItem::kMss, a, b}); });
    order.push_back({ArrivalItem::kFit, 0, 0});
    between(g.Lp, g.base_rows, [&](int sec) { return g.pan_start(sec); }, pan_blocks);
    return order;
}

// ---- cross-CCD sections: `sections` windows of lines_per_section lines in the columns the two CCDs share -------------------
struct CcdGeom {
    int W = 0, sections = 0, rows = 0, cols = 0;
    int col1 = 0, col2 = 0;                 // stitcher.h:175-176: PAN1 columns [W - ov, W - edge), PAN2 columns [edge, ov)
    long L = 0, gap = 0, step = 0;

    CcdGeom() = default;
    CcdGeom(int W_, long L_, int sections_, int lines_per_section, int overlap_cols, int edge_cols)
        : W(W_), sections(sections_), rows(lines_per_section), cols(overlap_cols - edge_cols), col1(W_ - overlap_cols), col2(edge_cols), L(L_)
    {
        gap = (L - (long)sections * lines_per_section) / (sections + 1);              // stitcher.h:151-152, :167
        step = gap + lines_per_section;
    }
    long section_start(int s) const { return gap + (long)s * step; }
};

constexpr const char *kCcdTooFewLines = "PAN line count less than sections times line-per-section, use smaller -s and/or -l value(s)";   // stitcher.h:75-77

inline std::string MakeCcdGeom(int W, long L, int sections, int lines_per_section, int overlap_cols, int edge_cols, CcdGeom *g)
{
    if (W <= 0 || L <= 0 || sections <= 0 || lines_per_section <= 0 || overlap_cols <= 0 || overlap_cols > W || edge_cols < 0 ||
        edge_cols >= overlap_cols || sections > 100000)
        return "oip_stt_correlate: bad argument";
    if (L < (long)sections * lines_per_section) return kCcdTooFewLines;
    *g = CcdGeom(W, L, sections, lines_per_section, overlap_cols, edge_cols);
    return "";
}

}  // namespace OIPGPU
