// fftplan_test.cpp -- the host planner of the FFT engine (csrc/oip_fftplan.h) on the CPU, over every length it can be asked for:
// every 2^a 3^b 5^c row length N <= 2^20 (planned with 8 rows) and every such column length 2 <= M <= 2^18 (planned with 16
// columns).  The two axes of a plan do not depend on each other, except that a leading row pass puts the M rows into its grid.
// Per plan: it exists; the factors multiply to the length and respect their limits; the radix chain of every pass fits
// OipFftPass::radix and multiplies to F; a generic tile fits kMaxTileElems and the LDS of a workgroup; nothing the launcher
// would refuse (grid dimensions, inter-pass twiddle rows); and oip_pos_to_freq / oip_freq_to_pos (csrc/oip_fft.h) invert
// each other with the plan's digits.  Then what the planner is known to give: see check_known.
// Built with ASan + UBSan by tests/test_host_cpu.py.  Prints "<n> checks, 0 bad" and exits 0 when everything holds.
#include "oip_fft.h"
#include "oip_fftplan.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace oipfftplan;

static long g_checks = 0, g_bad = 0;
#define CHECK(cond, ...)                                                                                               \
    do {                                                                                                               \
        ++g_checks;                                                                                                    \
        if (!(cond)) {                                                                                                 \
            if (++g_bad <= 20) { printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                                                              \
    } while (0)

static std::vector<int> smooth_up_to(long top)
{
    std::vector<int> v;
    for (long a = 1; a <= top; a *= 2)
        for (long b = a; b <= top; b *= 3)
            for (long c = b; c <= top; c *= 5) v.push_back((int)c);
    return v;
}

static int g_max_radices_4096 = 0, g_max_passes_x = 0, g_max_passes_y = 0, g_first_3pass_y = 0, g_first_2pass_x = 0;

// the passes of one axis of a plan: factors, limits, kernels, tiles, LDS, launch limits, digits
static void check_axis(const OipFftHostPlan &pl, int axis)
{
    const std::vector<int> &f = axis ? pl.yf : pl.xf;
    const int L = axis ? pl.M : pl.N;
    const char ax = axis ? 'y' : 'x';
    long prod = 1;
    for (int v : f) prod *= v;
    CHECK(!f.empty() && prod == L, "%c %d: factors multiply to %ld", ax, L, prod);
    CHECK(f.size() <= 4, "%c %d: %zu factors, OipAxisDigits holds 4", ax, L, f.size());
    for (size_t i = 0; i < f.size(); ++i) {
        const bool last = i + 1 == f.size();
        const int limit = !last ? kMaxLeadFactor : (axis ? kMaxLastColFactor : kMaxLastRowFactor);
        CHECK(f[i] >= 1 && f[i] <= limit && (f[i] >= 2 || L == 1), "%c %d: factor %d of %zu is %d, limit %d", ax, L, (int)i, f.size(), f[i], limit);
    }
    // the passes of the axis, in the plan's order
    size_t at = axis ? 0 : (size_t)pl.n_y;
    int T = L;
    for (size_t i = 0; i < f.size(); ++i, ++at) {
        CHECK(at < pl.passes.size(), "%c %d: pass %zu missing", ax, L, i);
        if (at >= pl.passes.size()) return;
        const OipFftPass &p = pl.passes[at];
        CHECK(p.F == f[i] && p.axis == axis && p.T == T && p.S == T / p.F && p.T % p.F == 0, "%c %d pass %zu: F %d axis %d T %d S %d", ax, L, i, p.F, p.axis, p.T, p.S);
        CHECK(p.mode == ((axis || p.S > 1) ? 0 : 1), "%c %d pass %zu: mode %d with S %d", ax, L, i, p.mode, p.S);
        CHECK(p.nradix >= (p.F > 1 ? 1 : 0) && p.nradix <= 16, "%c %d F %d: %d radices", ax, L, p.F, p.nradix);
        long rp = 1;
        for (int r = 0; r < p.nradix && r < 16; ++r) {
            CHECK(p.radix[r] == 2 || p.radix[r] == 3 || p.radix[r] == 4 || p.radix[r] == 5 || p.radix[r] == 8, "%c %d F %d: radix %d", ax, L, p.F, p.radix[r]);
            rp *= p.radix[r];
        }
        CHECK(rp == p.F, "%c %d F %d: radices multiply to %ld", ax, L, p.F, rp);
        if (p.F <= 4096 && p.nradix > g_max_radices_4096) g_max_radices_4096 = p.nradix;
        CHECK(p.vshift >= 0 && p.vshift <= 5, "%c %d F %d: vshift %d", ax, L, p.F, p.vshift);
        if (p.fast < 0) {
            CHECK(p.Vp == (p.vshift ? (1 << p.vshift) + 1 : 1), "%c %d F %d: vshift %d with Vp %d", ax, L, p.F, p.vshift, p.Vp);
            CHECK((long)p.F * p.Vp <= kMaxTileElems, "%c %d F %d: tile of %ld elements", ax, L, p.F, (long)p.F * p.Vp);
            CHECK(pass_lds_bytes(p) == 8 * ((size_t)2 * p.F * p.Vp + p.F), "%c %d F %d: %zu bytes of LDS", ax, L, p.F, pass_lds_bytes(p));
            CHECK(pass_lds_bytes(p) + kGenericStaticLds <= (size_t)kMaxLdsBytes, "%c %d F %d: %zu + %d bytes of LDS", ax, L, p.F, pass_lds_bytes(p), kGenericStaticLds);
            // the widest tile class that fits: the next one does not
            CHECK(p.vshift == 5 || (long)p.F * ((2 << p.vshift) + 1) > kMaxTileElems, "%c %d F %d: vshift %d, a wider tile fits", ax, L, p.F, p.vshift);
        } else {
            CHECK(p.fast < kNumFastKeys && kFastKeys[p.fast].F == p.F && kFastKeys[p.fast].mode == p.mode && kFastKeys[p.fast].vshift == p.vshift,
                  "%c %d F %d: fast %d", ax, L, p.F, p.fast);
            CHECK(pass_lds_bytes(p) <= (size_t)kMaxLdsBytes, "%c %d F %d: %zu bytes of LDS", ax, L, p.F, pass_lds_bytes(p));
        }
        if (p.mode == 0) {
            CHECK(p.O1 >= 1 && p.O1 <= 65535 && p.O2 >= 1 && p.O2 <= 65535, "%c %d F %d: O1 %d O2 %d", ax, L, p.F, p.O1, p.O2);
            CHECK((long)p.O1 * p.O2 * p.F * p.lanes == (long)pl.M * pl.N, "%c %d F %d: O1 %d O2 %d and %ld lanes do not cover the array", ax, L, p.F, p.O1, p.O2, p.lanes);
            CHECK(p.lane_tiles == (int)((p.lanes + (1 << p.vshift) - 1) >> p.vshift) && p.lane_tiles >= 1, "%c %d F %d: %d lane tiles of %ld lanes", ax, L, p.F, p.lane_tiles, p.lanes);
        }
        CHECK(p.tw_mode == (p.S > 1 ? (axis ? 2 : 1) : 0), "%c %d F %d: tw_mode %d with S %d", ax, L, p.F, p.tw_mode, p.S);
        if (p.tw_mode == 2) CHECK((long)p.T * 8 <= (16L << 20) && p.O1 == p.T / p.F, "%c %d F %d: T %d O1 %d", ax, L, p.F, p.T, p.O1);
        char why[128] = "";
        CHECK(launch_refusal(p, why, sizeof why) == kPlanOk, "%c %d F %d: the launcher refuses: %s", ax, L, p.F, why);
        T = p.S;
    }
    CHECK(T == 1, "%c %d: %d left after the last pass", ax, L, T);
    // the digit scramble of the axis, with the plan's factors
    OipAxisDigits d;
    d.n = (int)f.size();
    d.L = L;
    for (int i = 0; i < 4; ++i) d.f[i] = i < d.n ? f[i] : 1;
    long bad = 0;
    std::vector<char> seen(L, 0);
    for (int k = 0; k < L; ++k) {
        const int p = oip_freq_to_pos(d, k);
        if (p < 0 || p >= L || seen[p] || oip_pos_to_freq(d, p) != k) { ++bad; continue; }
        seen[p] = 1;
        const int q = oip_pos_to_freq(d, k);
        if (q < 0 || q >= L || oip_freq_to_pos(d, q) != k) ++bad;
    }
    CHECK(bad == 0, "%c %d: oip_pos_to_freq and oip_freq_to_pos disagree at %ld of %d", ax, L, bad, L);
}

static void check_all()
{
    char why[128];
    long nx = 0, ny = 0;
    for (int N : smooth_up_to(1L << 20)) {
        OipFftHostPlan pl;
        why[0] = 0;
        const int rc = plan(8, N, &pl, why, sizeof why);
        CHECK(rc == kPlanOk, "8 x %d: %s", N, why);
        if (rc) continue;
        ++nx;
        CHECK(pl.M == 8 && pl.N == N && pl.P % 16 == 0 && pl.P >= N && pl.P < N + 16, "8 x %d: M %d N %d P %d", N, pl.M, pl.N, pl.P);
        CHECK(pl.passes.size() == pl.xf.size() + pl.yf.size() && pl.n_y == (int)pl.yf.size(), "8 x %d: %zu passes", N, pl.passes.size());
        check_axis(pl, 0);
        if ((int)pl.xf.size() > g_max_passes_x) g_max_passes_x = (int)pl.xf.size();
        if (pl.xf.size() == 2 && (!g_first_2pass_x || N < g_first_2pass_x)) g_first_2pass_x = N;
    }
    for (int M : smooth_up_to(1L << 18)) {
        if (M < 2) continue;
        OipFftHostPlan pl;
        why[0] = 0;
        const int rc = plan(M, 16, &pl, why, sizeof why);
        CHECK(rc == kPlanOk, "%d x 16: %s", M, why);
        if (rc) continue;
        ++ny;
        CHECK(pl.passes.size() == pl.xf.size() + pl.yf.size() && pl.n_y == (int)pl.yf.size(), "%d x 16: %zu passes", M, pl.passes.size());
        check_axis(pl, 1);
        if ((int)pl.yf.size() > g_max_passes_y) g_max_passes_y = (int)pl.yf.size();
        if (pl.yf.size() == 3 && (!g_first_3pass_y || M < g_first_3pass_y)) g_first_3pass_y = M;
    }
    printf("%ld row lengths, %ld column lengths planned\n", nx, ny);
}

static std::string described(int M, int N, int *rc)
{
    char buf[4096];
    *rc = describe(M, N, buf, sizeof buf);
    return buf;
}

// What the planner gives today.  A change of the planner that moves one of these is a change of which kernels and tile classes
// tests/test_gpu_fft_routes.py has to reach: move both together.
static void check_known()
{
    CHECK(g_max_radices_4096 == 7, "longest radix chain up to 4096 points: %d", g_max_radices_4096);
    CHECK(g_first_2pass_x == 4320, "first two-pass row length: %d", g_first_2pass_x);
    CHECK(g_max_passes_x == 2, "most row passes up to 2^20: %d", g_max_passes_x);
    CHECK(g_first_3pass_y == 46875, "first three-pass column length: %d", g_first_3pass_y);
    CHECK(g_max_passes_y == 3, "most column passes up to 2^18: %d", g_max_passes_y);
    OipFftHostPlan pl;
    char why[128];
    // the two fixed column plans
    CHECK(plan(16000, 16, &pl, why, sizeof why) == kPlanOk && pl.yf == (std::vector<int>{128, 125}), "16000 is not 128 * 125");
    CHECK(plan(4000, 16, &pl, why, sizeof why) == kPlanOk && pl.yf == (std::vector<int>{32, 125}), "4000 is not 32 * 125");
    // tile classes of the generic kernel by factor: V = 32 up to 155, 16 up to 301, 8 up to 568, 4 up to 1024, 2 up to 1706
    const int edges[][2] = {{155, 5}, {156, 4}, {301, 4}, {302, 3}, {568, 3}, {569, 2}, {1024, 2}, {1025, 1}, {1706, 1}, {1707, 0}, {4096, 0}};
    for (const auto &e : edges) CHECK(pick_vshift(e[0], 32) == e[1], "pick_vshift(%d) = %d, expected %d", e[0], pick_vshift(e[0], 32), e[1]);
    // the radix chains named by the cases of the GPU suite
    CHECK(radix_list(729) == (std::vector<int>{3, 3, 3, 3, 3, 3}), "729");
    CHECK(radix_list(1458) == (std::vector<int>{3, 3, 3, 3, 3, 3, 2}), "1458");
    CHECK(radix_list(3888) == (std::vector<int>{3, 3, 3, 3, 3, 8, 2}), "3888");
    CHECK(radix_list(4096) == (std::vector<int>{8, 8, 8, 8}), "4096");
    CHECK(radix_list(3750) == (std::vector<int>{3, 2, 5, 5, 5, 5}), "3750");
    // the refusals, as oip_fft_plan_describe words them
    int rc;
    CHECK(described(14, 16, &rc) == "fft2d: 14 x 16 is not 2^a3^b5^c" && rc == kPlanInvalid, "14 x 16: %d %s", rc, described(14, 16, &rc).c_str());
    CHECK(described(1, 16, &rc) == "fft2d: fewer than 2 rows" && rc == kPlanUnsupported, "1 x 16: %d %s", rc, described(1, 16, &rc).c_str());
    // a leading row pass has the rows in its grid: more than 65535 rows of more than 4096 points are refused at the launch
    CHECK(described(65536, 8192, &rc) == "fft pass: more than 65535 rows or blocks" && rc == kPlanUnsupported, "65536 x 8192: %d %s", rc, described(65536, 8192, &rc).c_str());
    CHECK(described(65536, 4096, &rc).find("axis=x F=4096 mode=1 kind=generic vshift=0 Vp=1 radix=8,8,8,8 lds=98304\n") != std::string::npos && rc == kPlanOk,
          "65536 x 4096: %d %s", rc, described(65536, 4096, &rc).c_str());
    CHECK(described(16000, 3000, &rc) == "axis=y F=128 mode=0 kind=ct vshift=4 Vp=17 radix=8,8,2 lds=19456\n"
                                         "axis=y F=125 mode=0 kind=ct vshift=4 Vp=17 radix=5,5,5 lds=19000\n"
                                         "axis=x F=3000 mode=1 kind=ct vshift=1 Vp=2 radix=3,8,5,5,5 lds=72008\n" && rc == kPlanOk,
          "16000 x 3000: %d %s", rc, described(16000, 3000, &rc).c_str());
    char tiny[8];
    CHECK(describe(16000, 3000, tiny, sizeof tiny) == kPlanInvalid && tiny[0] == 0, "a short buffer is not refused");
    CHECK(describe(16000, 3000, nullptr, 0) == kPlanInvalid, "a null buffer is not refused");
}

int main()
{
    check_all();
    check_known();
    printf("%ld checks, %ld bad\n", g_checks, g_bad);
    return g_bad ? 1 : 0;
}
