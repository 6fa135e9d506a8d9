// fft_index_test.cpp -- the host/device index helpers of the FFT engine (csrc/oip_fft.h) on the CPU:
//   oip_pos_to_freq / oip_freq_to_pos: the digit scramble the forward transform leaves an axis in; the row stage, the cross-power
//     kernel and the plan's row table walk the spectrum by them;
//   oip_peak_pack / oip_peak_key: the 64-bit arg-max slot every workgroup of the last inverse pass folds its maximum into.
// Built with ASan + UBSan by tests/test_host_cpu.py.  Prints "<n> checks, 0 bad" and exits 0 when everything holds.
#include "oip_fft.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

static long g_checks = 0, g_bad = 0;
#define CHECK(cond, ...)                                                                                               \
    do {                                                                                                               \
        ++g_checks;                                                                                                    \
        if (!(cond)) {                                                                                                 \
            if (++g_bad <= 20) { printf("FAILED %s:%d  %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                                                              \
    } while (0)

// The definition in the header comment, restated without the helpers' loops: with factors (F1, F2, ..) position
// p = k1 (F2 F3 ..) + k2 (F3 ..) + .. holds frequency k = k1 + F1 (k2 + F2 (k3 ..)).  Enumerate every digit tuple and fill both
// tables from the two formulas.
static void tables_by_definition(const std::vector<int> &f, std::vector<int> *pos_to_freq, std::vector<int> *freq_to_pos)
{
    const int n = (int)f.size();
    long L = 1;
    for (int v : f) L *= v;
    pos_to_freq->assign(L, -1);
    freq_to_pos->assign(L, -1);
    std::vector<int> k(n, 0);
    for (long count = 0; count < L; ++count) {
        long p = 0, wp = 1;                      // weights of the position: product of the factors behind digit i
        for (int i = n - 1; i >= 0; --i) { p += k[i] * wp; wp *= f[i]; }
        long q = 0, wq = 1;                      // weights of the frequency: product of the factors before digit i
        for (int i = 0; i < n; ++i) { q += k[i] * wq; wq *= f[i]; }
        (*pos_to_freq)[p] = (int)q;
        (*freq_to_pos)[q] = (int)p;
        for (int i = 0; i < n; ++i) { if (++k[i] < f[i]) break; k[i] = 0; }      // next tuple
    }
}

static void check_axis(const std::vector<int> &f)
{
    OipAxisDigits d;
    d.n = (int)f.size();
    d.L = 1;
    for (int i = 0; i < 4; ++i) { d.f[i] = i < d.n ? f[i] : 1; d.L *= d.f[i]; }
    std::vector<int> p2f, f2p;
    tables_by_definition(f, &p2f, &f2p);
    std::vector<char> seen_f(d.L, 0), seen_p(d.L, 0);
    for (int i = 0; i < d.L; ++i) {
        const int k = oip_pos_to_freq(d, i), p = oip_freq_to_pos(d, i);
        CHECK(k >= 0 && k < d.L && p >= 0 && p < d.L, "L %d i %d: k %d p %d out of range", d.L, i, k, p);
        if (k < 0 || k >= d.L || p < 0 || p >= d.L) return;
        CHECK(k == p2f[i], "L %d (%d factors) pos %d: freq %d, definition %d", d.L, d.n, i, k, p2f[i]);
        CHECK(p == f2p[i], "L %d (%d factors) freq %d: pos %d, definition %d", d.L, d.n, i, p, f2p[i]);
        CHECK(oip_freq_to_pos(d, k) == i, "L %d: freq_to_pos(pos_to_freq(%d)) = %d", d.L, i, oip_freq_to_pos(d, k));
        CHECK(oip_pos_to_freq(d, p) == i, "L %d: pos_to_freq(freq_to_pos(%d)) = %d", d.L, i, oip_pos_to_freq(d, p));
        CHECK(!seen_f[k] && !seen_p[p], "L %d i %d: not a permutation", d.L, i);
        seen_f[k] = seen_p[p] = 1;
    }
    CHECK(oip_freq_to_pos(d, 0) == 0 && oip_pos_to_freq(d, 0) == 0, "L %d: DC moved", d.L);
}

static void check_axes()
{
    // what split_axis (csrc/oip_fftplan.h) emits for the column lengths of tests/test_gpu_fft_routes.py, the two fixed plans
    // (16000 = 128 * 125, 4000 = 32 * 125), the product's own shapes, the long rows, and the one-factor case
    const std::vector<std::vector<int>> lists = {
        {100, 100}, {160, 160}, {64, 64}, {125, 160}, {100, 128}, {128, 128}, {20, 32}, {100, 125}, {243},
        {128, 125}, {32, 125}, {20, 20}, {40, 40}, {50, 60}, {250}, {400}, {48}, {2},
        {50, 100}, {64, 128}, {75, 80},
        // the helpers take up to four factors (split_axis goes there for lengths past max_a * max_last)
        {2, 3}, {3, 2}, {5, 4, 3}, {16, 15, 9}, {2, 3, 5, 7}, {6, 5, 4, 3},
    };
    for (const auto &f : lists) check_axis(f);
}

static void check_peak_slots()
{
    const float inf = std::numeric_limits<float>::infinity();
    const float den = std::numeric_limits<float>::denorm_min();
    const float fmin = std::numeric_limits<float>::min(), fmax = std::numeric_limits<float>::max();
    // strictly increasing values: negative, denormal, zero, positive, inf
    const float sorted[] = {-inf, -fmax, -1.0e20f, -2.0f, -1.0f, -0.5f, -fmin, -2 * den, -den, 0.0f, den, 2 * den, fmin,
                            1.0e-20f, 0.5f, 1.0f, std::nextafterf(1.0f, 2.0f), 2.0f, 80000.0f, 4.8e7f, 1.0e20f, fmax, inf};
    const int nv = (int)(sizeof sorted / sizeof sorted[0]);
    const long keys[] = {0, 1, 2, 199, 200, 79999, 4799999, 0x7fffffffL, 0x80000000L, 0xfffffffdL, 0xfffffffeL};
    const long none = -7;
    for (long key : keys) {
        for (int i = 0; i < nv; ++i) {
            const unsigned long long p = oip_peak_pack(sorted[i], key);
            CHECK(p != 0ull, "value %g key %ld packs to the empty slot", (double)sorted[i], key);
            CHECK(oip_peak_key(p, none) == key, "value %g: key %ld came back as %ld", (double)sorted[i], key, oip_peak_key(p, none));
            if (i > 0) {
                CHECK(sorted[i - 1] < sorted[i], "the list itself is not sorted at %d", i);
                CHECK(oip_peak_pack(sorted[i - 1], key) < p, "order lost between %g and %g at key %ld", (double)sorted[i - 1], (double)sorted[i], key);
            }
        }
        // the value decides before the key: the smaller value with the best key loses against the larger value with the worst key
        for (int i = 1; i < nv; ++i)
            CHECK(oip_peak_pack(sorted[i - 1], 0) < oip_peak_pack(sorted[i], 0xfffffffeL), "key outranks value at %g", (double)sorted[i]);
        CHECK(oip_peak_pack(-0.0f, key) == oip_peak_pack(0.0f, key), "-0 and +0 differ at key %ld", key);
        CHECK(oip_peak_pack(std::numeric_limits<float>::quiet_NaN(), key) == 0ull, "NaN enters at key %ld", key);
        CHECK(oip_peak_pack(-std::numeric_limits<float>::quiet_NaN(), key) == 0ull, "-NaN enters at key %ld", key);
    }
    CHECK(oip_peak_key(0ull, none) == none, "the empty slot has a key");
    CHECK(oip_peak_key(0ull, 0) == 0, "the empty slot has a key");
    // at equal value the smaller key packs larger (atomicMax then keeps the first maximum in scan order)
    const int nk = (int)(sizeof keys / sizeof keys[0]);
    for (float v : {-inf, -1.0f, -0.0f, 0.0f, den, 1.0f, inf})
        for (int i = 1; i < nk; ++i)
            CHECK(oip_peak_pack(v, keys[i - 1]) > oip_peak_pack(v, keys[i]), "tie at %g: key %ld does not beat key %ld", (double)v, keys[i - 1], keys[i]);
}

int main()
{
    check_axes();
    check_peak_slots();
    printf("%ld checks, %ld bad\n", g_checks, g_bad);
    return g_bad ? 1 : 0;
}
