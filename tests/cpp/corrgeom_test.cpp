// corrgeom_test.cpp -- the correlation-window geometry (csrc/oip_corrgeom.h) on the CPU: hand-worked values from the
// reference's formulas (preproc.h:245-247, :257, :274-276, :284, :326; stitcher.h:151-152, :167, :175-176), the makers'
// refusals and the properties of what they accept over a sweep of small strips, the arrival order of the pipelined default
// action, and the shift table's layout.  Every expectation is restated here, independently of the header.  Built with
// ASan + UBSan by tests/test_corrgeom_cpu.py.
#include "oip_corrgeom.h"

#include <cstdio>

using namespace OIPGPU;

// what a maker gave: the geometry, or the message
template <typename Geom> struct Got {
    Geom g;
    std::string text;
    explicit operator bool() const { return text.empty(); }
};
static Got<InterBandGeom> ib(int W, long Lp, int slices, int sections, int corr)
{
    Got<InterBandGeom> m;
    m.text = MakeInterBandGeom(W, Lp, slices, sections, corr, &m.g);
    return m;
}
static Got<CcdGeom> ccdg(int W, long L, int sections, int lps, int ov, int edge)
{
    Got<CcdGeom> m;
    m.text = MakeCcdGeom(W, L, sections, lps, ov, edge, &m.g);
    return m;
}

static int bad = 0, n = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++bad; printf("%s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

// `sections` windows of `rows` lines from `first(sec)` on in a raster of `total` lines: in order, disjoint, inside, the gaps
// before and between them all `gap` lines, the last one gap + rest lines with rest = lastRest (or any rest >= 0 when < 0)
template <typename Start> static void windows(const char *what, int sections, long rows, long total, long gap, long lastRest, Start first, const char *at)
{
    long end = 0;                           // the end of the window before
    for (int s = 0; s < sections; ++s) {
        EXPECT(first(s) >= end && first(s) - end == gap, "%s window %d of %s starts at %ld, %ld after the one before, gap %ld", what, s, at, first(s), first(s) - end, gap);
        end = first(s) + rows;
        EXPECT(end <= total, "%s window %d of %s ends at %ld of %ld", what, s, at, end, total);
    }
    const long rest = total - end - gap;
    EXPECT(rest >= 0 && (lastRest < 0 || rest == lastRest), "%s of %s: last gap %ld, gap %ld", what, at, total - end, gap);
}

static const char *kSlices = "CalcInterBandCorrelation: at lease 8 slice needed";
static const char *kSections = "CalcInterBandCorrelation: section count should be a positive integer";
static const char *kSmall = "oip_interband_correlate: slice too small";
static const char *kCcdLines = "PAN line count less than sections times line-per-section, use smaller -s and/or -l value(s)";

static void interband(int W, long Lp, int slices, int sections, int corr)
{
    ++n;
    char at[128], many[160];
    snprintf(at, sizeof at, "W %d Lp %ld slices %d sections %d corr %d", W, Lp, slices, sections, corr);
    snprintf(many, sizeof many, "CalcInterBandCorrelation: too many sections (%d lines per section), not enough total PAN data lines", corr);
    const long rows = Lp < corr ? Lp : corr;
    // the reference's checks in the reference's order, then the window that integer division leaves empty
    std::string want;
    if (slices < 8) want = kSlices;
    else if (sections <= 0) want = kSections;
    else if (sections > 1 && (long)sections * corr > Lp) want = many;
    else if (rows / 4 <= 0 || W / slices / 4 <= 0) want = kSmall;
    const auto m = ib(W, Lp, slices, sections, corr);
    EXPECT(m.text == want && (bool)m == want.empty(), "%s: `%s', `%s' expected", at, m.text.c_str(), want.c_str());
    if (!m || !want.empty()) return;
    const InterBandGeom &g = m.g;
    const long gap = (Lp - rows * sections) / (sections + 1);
    EXPECT(g.base_rows == rows && g.base_gap == gap && g.band_rows == rows / 4 && g.band_gap == gap / 4 && g.base_cols == W / slices &&
               g.band_cols == W / slices / 4 && g.Wb == W / 4 && g.n_units == slices * sections,
           "%s: rows %d gap %ld cols %d, band rows %d gap %ld cols %d, Wb %d, %d units", at, g.base_rows, g.base_gap, g.base_cols, g.band_rows, g.band_gap, g.band_cols,
           g.Wb, g.n_units);
    windows("PAN", sections, rows, Lp, gap, (Lp - rows * sections) % (sections + 1), [&](int s) { return g.pan_start(s); }, at);
    windows("MSS", sections, rows / 4, Lp / 4, gap / 4, -1, [&](int s) { return g.mss_start(s); }, at);
    for (int u = 0; u < g.n_units; ++u) {
        const int i = u % slices, c = g.centre_col(u);
        EXPECT(c == i * (W / slices) + W / slices / 2 && c < W, "%s: unit %d centre %d", at, u, c);
    }
}

static void ccd(int W, long L, int sections, int lps, int ov, int edge)
{
    ++n;
    char at[128];
    snprintf(at, sizeof at, "W %d L %ld sections %d lps %d ov %d edge %d", W, L, sections, lps, ov, edge);
    const std::string want = L < (long)sections * lps ? kCcdLines : "";
    const auto m = ccdg(W, L, sections, lps, ov, edge);
    EXPECT(m.text == want && (bool)m == want.empty(), "%s: `%s', `%s' expected", at, m.text.c_str(), want.c_str());
    if (!m || !want.empty()) return;
    const CcdGeom &g = m.g;
    const long gap = (L - (long)sections * lps) / (sections + 1);
    EXPECT(g.gap == gap && g.step == gap + lps && g.rows == lps && g.cols == ov - edge && g.col1 == W - ov && g.col2 == edge, "%s: gap %ld step %ld, %d x %d at %d / %d", at,
           g.gap, g.step, g.rows, g.cols, g.col1, g.col2);
    EXPECT(g.col1 >= 0 && g.col1 + g.cols <= W && g.col2 + g.cols <= W, "%s: columns %d / %d + %d of %d", at, g.col1, g.col2, g.cols, W);
    windows("CCD", sections, lps, L, gap, (L - (long)sections * lps) % (sections + 1), [&](int s) { return g.section_start(s); }, at);
}

static void arrival(int sections, int slices, long block)
{
    ++n;
    const long Lp = 4000, Lm = Lp / 4;
    char at[96];
    snprintf(at, sizeof at, "%d sections, %d slices, blocks of %ld", sections, slices, block);
    const auto m = ib(352, Lp, slices, sections, 600);
    EXPECT((bool)m, "%s: `%s'", at, m.text.c_str());
    if (!m) return;
    const InterBandGeom &g = m.g;
    std::vector<int> pan(Lp, 0), mss(Lm, 0);
    int unitsItems = 0, fits = 0;
    auto all = [](const std::vector<int> &v, long a, long b) { for (long i = a; i < b; ++i) if (v[i] != 1) return false; return true; };
    for (const ArrivalItem &it : ArrivalOrder(g, Lm, block)) {
        if (it.kind == ArrivalItem::kPan || it.kind == ArrivalItem::kMss) {
            const bool p = it.kind == ArrivalItem::kPan;
            EXPECT(it.a >= 0 && it.a < it.b && it.b <= (p ? Lp : Lm) && (!p || it.b - it.a <= block), "%s: %s lines [%ld, %ld)", at, p ? "PAN" : "MSS", it.a, it.b);
            if (it.a < 0 || it.b > (p ? Lp : Lm)) continue;
            for (long i = it.a; i < it.b; ++i) ++(p ? pan : mss)[i];
        } else if (it.kind == ArrivalItem::kUnits) {
            const int sec = (int)it.a;
            EXPECT(sec == unitsItems && fits == 0, "%s: units item of section %d is number %d", at, sec, unitsItems);
            ++unitsItems;
            if (sec < 0 || sec >= sections) continue;
            EXPECT(all(pan, g.pan_start(sec), g.pan_start(sec) + g.base_rows) && all(mss, g.mss_start(sec), g.mss_start(sec) + g.band_rows),
                   "%s: section %d correlated before its lines", at, sec);
            // the units computed so far end at a pair boundary, except behind the last section
            const int hi = g.units_through(sec), full = (sec + 1) * slices;
            EXPECT(sec == sections - 1 ? hi == sections * slices : (hi % 2 == 0 && hi <= full && hi > full - 2), "%s: %d units through section %d", at, hi, sec);
        } else {
            EXPECT(unitsItems == sections && all(mss, 0, Lm), "%s: fit before %d sections or every MSS line", at, sections);
            ++fits;
        }
    }
    EXPECT(fits == 1 && unitsItems == sections && all(pan, 0, Lp) && all(mss, 0, Lm), "%s: %d fits, %d unit items, or a line not read exactly once", at, fits, unitsItems);
}

int main()
{
    // ---- hand-worked values
    {
        ++n;
        const auto m = ib(30000, 100000, 10, 5, 16000);
        const InterBandGeom &g = m.g;
        EXPECT((bool)m && g.base_rows == 16000 && g.base_gap == 3333 && g.band_rows == 4000 && g.band_gap == 833 && g.base_cols == 3000 && g.band_cols == 750 &&
                   g.Wb == 7500 && g.n_units == 50,
               "the 30000 x 100000 strip: `%s' rows %d gap %ld / %d gap %ld, cols %d / %d", m.text.c_str(), g.base_rows, g.base_gap, g.band_rows, g.band_gap, g.base_cols,
               g.band_cols);
        for (int sec = 0; m && sec < 5; ++sec)
            EXPECT(g.pan_start(sec) == 3333 + 19333L * sec && g.mss_start(sec) == 833 + 4833L * sec, "section %d starts at %ld / %ld", sec, g.pan_start(sec), g.mss_start(sec));
        for (int u = 0; m && u < 50; ++u) EXPECT(g.centre_col(u) == 3000 * (u % 10) + 1500, "unit %d centre %d", u, g.centre_col(u));
    }
    {
        ++n;
        const auto m = ccdg(30000, 262144, 10, 16000, 200, 0);
        EXPECT((bool)m && m.g.gap == 9285 && m.g.step == 25285 && m.g.cols == 200 && m.g.rows == 16000 && m.g.col1 == 30000 - 200 && m.g.col2 == 0 &&
                   m.g.section_start(0) == 9285 && m.g.section_start(9) == 9285 + 9 * 25285L,
               "the 262144-line CCD pair: `%s' gap %ld step %ld cols %d at %d / %d", m.text.c_str(), m.g.gap, m.g.step, m.g.cols, m.g.col1, m.g.col2);
    }
    {
        ++n;
        const auto m = ib(30000, 12000, 10, 1, 16000);
        EXPECT((bool)m && m.g.base_rows == 12000 && m.g.base_gap == 0 && m.g.pan_start(0) == 0, "a strip shorter than the window: `%s' rows %d gap %ld", m.text.c_str(),
               m.g.base_rows, m.g.base_gap);
    }
    // ---- the bad-argument checks, the reference's checks on their own, and the geometry the plans construct unchecked
    {
        ++n;
        const char *badIb = "oip_interband_correlate: bad argument";
        EXPECT(ib(0, 100, 8, 1, 64).text == badIb && ib(64, 0, 8, 1, 64).text == badIb && ib(64, 100, 8, 1, 0).text == badIb, "W, Lp or corr_lines of 0 accepted");
        EXPECT(InterBandArgCheck(0, 10, 5, 16000) == "CalcInterBandCorrelation: too many sections (16000 lines per section), not enough total PAN data lines" &&
                   InterBandArgCheck(0, 10, 1, 16000).empty() && InterBandArgCheck(4000, 4, 2, 600) == kSlices && InterBandArgCheck(4000, 8, 0, 600) == kSections &&
                   InterBandArgCheck(4000, 8, 6, 600).empty(), "the reference's checks alone, an empty strip included");
        EXPECT(ib(16, 4000, 8, 2, 600).text == kSmall, "a slice of 2 columns: `%s'", ib(16, 4000, 8, 2, 600).text.c_str());
        const InterBandGeom p(352, 4000, 4, 2, 600);
        EXPECT(p.base_cols == 88 && p.band_cols == 22 && p.n_units == 8 && p.base_rows == 600 && p.base_gap == 933, "a plan of 4 slices: cols %d rows %d gap %ld", p.base_cols,
               p.base_rows, p.base_gap);
        for (int k = 0; k < 9; ++k) {
            const int a[6] = {k == 0 ? 0 : 300, 4000, k == 2 ? 0 : k == 8 ? 100001 : 3, k == 3 ? 0 : 100, k == 4 ? 0 : k == 5 ? 301 : 40, k == 6 ? -1 : k == 7 ? 40 : 2};
            const auto m = ccdg(a[0], k == 1 ? 0 : a[1], a[2], a[3], a[4], a[5]);
            EXPECT(m.text == "oip_stt_correlate: bad argument", "bad CCD argument %d: `%s'", k, m.text.c_str());
        }
        EXPECT(std::string(kCcdTooFewLines) == kCcdLines, "the CCD plan's text");
    }
    // ---- properties over small strips
    for (long Lp = 16; Lp <= 4000; Lp += 16)
        for (int sections = 1; sections <= 6; ++sections)
            for (int slices = 2; slices <= 11; ++slices)
                for (int corr : {64, 100, 256, 700, 1200})
                    for (int W : {40, 352}) interband(W, Lp, slices, sections, corr);
    interband(352, 4000, 10, 0, 600);
    for (long L = 16; L <= 4000; L += 16)
        for (int sections = 1; sections <= 6; ++sections)
            for (int lps : {64, 100, 256, 700, 1200})
                for (int ov : {8, 200})
                    for (int edge : {0, 3}) ccd(300, L, sections, lps, ov, edge);
    // ---- the arrival order: a pair of units spans two sections with 9 slices, none does with 10
    for (int sections = 1; sections <= 4; ++sections)
        for (int slices : {9, 10})
            for (long block : {7L, 250L, 5000L}) arrival(sections, slices, block);
    // ---- the shift table: [unit][band][dx, dy, rs] -> [band][unit][dx, dy, rs, cx]
    {
        ++n;
        const auto m = ib(352, 4000, 9, 2, 600);
        const int units = 18;
        std::vector<double> table((size_t)4 * units * 4, -1.0), res(12);
        EXPECT((bool)m && m.g.n_units == units, "the table's geometry: `%s'", m.text.c_str());
        if (m) {
            ShiftTableInit(m.g, table.data());
            for (int u = 0; u < units; ++u) {
                if (u == 5) continue;                                   // a unit another rank computes
                for (int b = 0; b < 4; ++b)
                    for (int k = 0; k < 3; ++k) res[3 * b + k] = 100 * u + 10 * b + k;
                ShiftTablePut(m.g, table.data(), u, res.data());
            }
            for (int b = 0; b < 4; ++b)
                for (int u = 0; u < units; ++u) {
                    const double *e = &table[((size_t)b * units + u) * 4];
                    for (int k = 0; k < 3; ++k) EXPECT(u == 5 ? e[k] != e[k] : e[k] == 100 * u + 10 * b + k, "band %d unit %d value %d: %f", b, u, k, e[k]);
                    EXPECT(e[3] == (u % 9) * (352 / 9) + 352 / 9 / 2, "band %d unit %d cx %f", b, u, e[3]);
                }
        }
    }
    printf("%d cases, %d bad\n", n, bad);
    return bad ? 1 : 0;
}
