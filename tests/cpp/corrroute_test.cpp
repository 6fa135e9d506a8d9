// corrroute_test.cpp -- the host planner of the correlation drivers (csrc/oip_corrroute.h) on the CPU.
// 1. The route table: per geometry and switches the route worked out by hand from the conditions of plan_interband (exact x4
//    window that fills its DFT size, 3000-point rows -> H, and HV where the band height is a DFT size >= 8; 1250-point rows
//    -> V; else the image domain), the stored window's radius, and the refusal of more than 65535 correlation lines.
// 2. The property sweep: every 2^a 3^b 5^c line count from 8 to 16000 x {3000, 1228, 320, 200} columns x every combination
//    of OIP_SPECTRAL_UP, OIP_SPECTRAL_V and OIP_PEAK_PRUNE: the plan refuses with a text, or its regions are 256-byte
//    aligned, in order, disjoint and sum to `total`, every array inside a slot lies inside it, the four narrow arrays of the
//    H and HV routes fit one slot, the window radius is -1 or fits, and describe() is JSON that names the plan's route.
// Built with ASan + UBSan by tests/test_corrroute_cpu.py.  Prints "<n> cases, 0 bad" and exits 0 when everything holds.
#include "oip_corrroute.h"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>

using namespace oipcorr;

static long g_cases = 0, g_bad = 0;
#define CHECK(cond, ...)                                                                                               \
    do {                                                                                                               \
        if (!(cond)) {                                                                                                 \
            ok = false;                                                                                                \
            if (g_bad < 20) { printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                                                              \
    } while (0)

// ---- a JSON reader that only says whether the text is one value ---------------------------------------------------------
struct Json {
    const char *p;
    void ws() { while (*p == ' ' || *p == '\n' || *p == '\t') ++p; }
    bool lit(const char *s) { const size_t n = strlen(s); if (strncmp(p, s, n)) return false; p += n; return true; }
    bool string()
    {
        if (*p != '"') return false;
        for (++p; *p && *p != '"'; ++p) if (*p == '\\' && !*++p) return false;
        return *p == '"' ? (++p, true) : false;
    }
    bool number()
    {
        const char *q = p;
        if (*p == '-') ++p;
        while ((*p >= '0' && *p <= '9') || *p == '.' || *p == 'e' || *p == 'E' || *p == '+' || *p == '-') ++p;
        return p > q && p[-1] >= '0' && p[-1] <= '9';
    }
    bool list(char close, bool keyed)
    {
        ++p;
        ws();
        if (*p == close) { ++p; return true; }
        for (;;) {
            ws();
            if (keyed) { if (!string()) return false; ws(); if (*p++ != ':') return false; }
            if (!value()) return false;
            ws();
            if (*p == ',') { ++p; continue; }
            return *p++ == close;
        }
    }
    bool value()
    {
        ws();
        if (*p == '{') return list('}', true);
        if (*p == '[') return list(']', false);
        if (*p == '"') return string();
        return lit("true") || lit("false") || lit("null") || number();
    }
    static bool parses(const std::string &s) { Json j{s.c_str()}; if (!j.value()) return false; j.ws(); return *j.p == 0; }
};

static CorrKnobs knobs_of(int up, int v, int prune, int window = kRowsWindowTiles)
{
    CorrKnobs k;
    k.spectral_up = up; k.spectral_v = v != 0; k.peak_prune = prune != 0; k.rows_window = window;
    return k;
}

// what holds of every plan; returns the planner's code
static int check_plan(int rows, int cols, const CorrKnobs &k, CorrPlan *p)
{
    bool ok = true;
    char why[160] = "";
    const int rc = plan_interband(rows, cols, rows / 4, cols / 4, 256, k, p, why, sizeof why);
    const std::string d = describe(*p, rc, why);
    CHECK(Json::parses(d), "%d x %d: %s", rows, cols, d.c_str());
    if (rc) {
        CHECK(why[0] && d.find("\"refused\": \"") != std::string::npos && d.find(why) != std::string::npos, "%d x %d: %s", rows, cols, d.c_str());
    } else {
        CHECK(d.find(std::string("{\"route\": \"") + route_name(p->route) + "\"") == 0, "%d x %d: %s", rows, cols, d.c_str());
        size_t at = 0;
        for (int r = 0; r < kNumRegions; ++r) {
            const CorrRegion &g = p->reg[r];
            CHECK(g.offset == at && g.offset % 256 == 0 && g.bytes % 256 == 0 && g.count >= 0, "%d x %d: region %s at %zu (%zu bytes), expected at %zu", rows,
                  cols, kRegionNames[r], g.offset, g.bytes, at);
            at = g.end();
        }
        CHECK(at == p->total, "%d x %d: regions end at %zu, total %zu", rows, cols, at, p->total);
        for (int r : {kRegZ, kRegY, kRegFa, kRegSmall, kRegSlots}) CHECK(p->reg[r].count >= 1 && p->reg[r].bytes > 0, "%d x %d: no %s", rows, cols, kRegionNames[r]);
        CHECK(p->reg[kRegZ].bytes >= 8 * (size_t)p->M * p->main.P && p->main.P >= p->N && p->M >= rows && p->N >= cols, "%d x %d: slot of %zu bytes", rows, cols,
              p->reg[kRegZ].bytes);
        for (const CorrSubRegion *s : {&p->band_sub, &p->raw_sub})
            CHECK(!s->bytes || (s->part < p->reg[s->in].count && s->offset + s->bytes <= p->reg[s->in].bytes), "%d x %d: %zu + %zu bytes in a part of %zu of %s",
                  rows, cols, s->offset, s->bytes, p->reg[s->in].bytes, kRegionNames[s->in]);
        const bool spectral = p->route != kImage;
        CHECK(spectral == (p->band_sub.bytes > 0) && (p->raw_sub.bytes > 0) == (p->route == kSpectralHV || p->route == kSpectralV), "%d x %d: sub-regions of %s",
              rows, cols, route_name(p->route));
        CHECK(p->reg[kRegZ].count == (spectral ? 2 : 5) && p->reg[kRegY].count == (spectral ? 4 : 2), "%d x %d: %d + %d slots", rows, cols, p->reg[kRegZ].count,
              p->reg[kRegY].count);
        if (p->route == kSpectralH || p->route == kSpectralHV) {
            OipFftHostPlan narrow;
            char w2[160];
            CHECK(oipfftplan::plan(p->M, cols / 4, &narrow, w2, sizeof w2) == 0 && 4 * narrow.P <= p->main.P, "%d x %d: 4 x %d > %d", rows, cols, narrow.P, p->main.P);
            CHECK(p->N == kUpRowsN && p->fused_rows && p->reg[kRegBound].count == 1 && p->groups >= 1 && p->groups <= 256 &&
                  p->reg[kRegBound].bytes >= 4 * (size_t)p->groups * 4 * p->main.P, "%d x %d: bound storage", rows, cols);
            CHECK(p->lists == (p->reg[kRegLists].count == 1) && (!p->lists || p->reg[kRegLists].bytes >= prune_list_bytes(p->T)), "%d x %d: list storage", rows, cols);
        } else {
            CHECK(p->reg[kRegBound].count == 0 && p->reg[kRegLists].count == 0 && !p->lists, "%d x %d: search storage on the %s route", rows, cols, route_name(p->route));
        }
        if (p->route == kSpectralV) CHECK(p->N == kVRowsN && p->fused_rows && p->band.N == 4 * p->N, "%d x %d: V route", rows, cols);
        if (spectral) CHECK(p->M == rows && rows == 4 * (rows / 4) && cols == 4 * (cols / 4) && k.spectral_up > 0, "%d x %d: %s", rows, cols, route_name(p->route));
        CHECK(p->win_r == -1 || (p->route == kSpectralHV && k.peak_prune && p->win_r == k.rows_window && rows_window_fits(p->lists, p->vshift, p->T, p->win_r)),
              "%d x %d: window %d", rows, cols, p->win_r);
    }
    ++g_cases;
    if (!ok) ++g_bad;
    return rc;
}

static void expect(int rows, int cols, const CorrKnobs &k, CorrRoute route, int win_r)
{
    bool ok = true;
    CorrPlan p;
    const int rc = check_plan(rows, cols, k, &p);
    CHECK(rc == 0 && p.route == route && p.win_r == win_r, "%d x %d: rc %d, route %s (expected %s), window %d (expected %d)", rows, cols, rc, route_name(p.route),
          route_name(route), p.win_r, win_r);
    ++g_cases;
    if (!ok) ++g_bad;
}

int main()
{
    const CorrKnobs none = knobs_of(2, 1, 1);
    // ---- the route table (cu_count 256).  16000 x 3000: 128-point first column pass, 16-column tiles, T = 188; 64 and 400
    // lines: one 64- / two 20-point passes, 32-column tiles, T = 94: a window of radius 8 fits all of them.
    expect(16000, 3000, none, kSpectralHV, 8);
    expect(16000, 3000, knobs_of(2, 1, 1, 0), kSpectralHV, -1);         // OIP_ROWS_WINDOW=0
    expect(16000, 3000, knobs_of(2, 1, 0), kSpectralHV, -1);            // OIP_PEAK_PRUNE=0
    expect(16000, 3000, knobs_of(1, 1, 1), kSpectralH, -1);
    expect(16000, 3000, knobs_of(0, 1, 1), kImage, -1);
    expect(64, 3000, none, kSpectralHV, 8);
    expect(400, 3000, none, kSpectralHV, 8);
    expect(20, 3000, none, kSpectralH, -1);                             // band height 5 < 8
    expect(16000, 1228, none, kSpectralV, -1);
    expect(64, 1228, none, kSpectralV, -1);
    expect(400, 1228, none, kSpectralV, -1);
    expect(16000, 1228, knobs_of(2, 0, 1), kImage, -1);                 // OIP_SPECTRAL_V=0
    expect(16000, 1228, knobs_of(0, 1, 1), kImage, -1);
    expect(3200, 320, none, kImage, -1);
    expect(3201, 3000, none, kImage, -1);                               // M = 3240 != rows
    expect(750, 3000, none, kImage, -1);                                // 4 x 187 != 750
    {
        // the fused row stage is a condition of every spectral route
        CorrKnobs k = none;
        k.fused_rows = false;
        expect(16000, 3000, k, kImage, -1);
        expect(16000, 1228, k, kImage, -1);
    }
    for (int rows : {65536, 72000}) {
        bool ok = true;
        CorrPlan p;
        char why[160] = "";
        const int rc = plan_interband(rows, 3000, rows / 4, 750, 256, none, &p, why, sizeof why);
        CHECK(rc == kPlanUnsupported && !strcmp(why, "oip_interband_correlate: more than 65535 correlation lines"), "%d lines: rc %d, \"%s\"", rows, rc, why);
        const std::string d = describe(p, rc, why);
        CHECK(Json::parses(d) && d == "{\"refused\": \"oip_interband_correlate: more than 65535 correlation lines\", \"code\": 6}", "%s", d.c_str());
        CHECK(plan_pair(rows, 200, none, "too tall", &p, why, sizeof why) == kPlanUnsupported && !strcmp(why, "too tall"), "pair of %d lines: \"%s\"", rows, why);
        ++g_cases;
        if (!ok) ++g_bad;
    }
    {
        // one pair: one spectrum slot, one output, nothing of the search
        bool ok = true;
        CorrPlan p;
        char why[160] = "";
        CHECK(plan_pair(64, 200, none, "too tall", &p, why, sizeof why) == 0 && p.M == 64 && p.N == 200 && p.fused_rows && p.reg[kRegZ].count == 1 &&
              p.reg[kRegY].count == 1 && p.reg[kRegFb].count == 0 && p.reg[kRegBound].count == 0 && p.win_r == -1 && p.total == p.reg[kRegSlots].end(), "pair plan");
        CHECK(plan_pair(48, 5000, none, "too tall", &p, why, sizeof why) == 0 && !p.fused_rows && p.main.xf.size() == 2, "pair plan with two row passes");
        ++g_cases;
        if (!ok) ++g_bad;
    }
    // ---- the property sweep
    long routes[4] = {0, 0, 0, 0}, refused = 0;
    for (long a = 1; a <= 16000; a *= 2)
        for (long b = a; b <= 16000; b *= 3)
            for (long r = b; r <= 16000; r *= 5) {
                if (r < 8) continue;
                for (int cols : {3000, 1228, 320, 200})
                    for (int up = 0; up <= 2; ++up)
                        for (int v = 0; v <= 1; ++v)
                            for (int prune = 0; prune <= 1; ++prune) {
                                CorrPlan p;
                                if (check_plan((int)r, cols, knobs_of(up, v, prune), &p)) ++refused;
                                else ++routes[p.route];
                            }
            }
    // what planning costs a call (it is not cached): the benchmark's geometry
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < 20; ++i) { CorrPlan p; char why[160]; plan_interband(16000, 3000, 4000, 750, 256, none, &p, why, sizeof why); }
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() / 20;
    printf("sweep: image %ld, H %ld, HV %ld, V %ld, refused %ld; plan_interband(16000 x 3000): %.0f us\n", routes[kImage], routes[kSpectralH],
           routes[kSpectralHV], routes[kSpectralV], refused, us);
    printf("%ld cases, %ld bad\n", g_cases, g_bad);
    return g_bad ? 1 : 0;
}
