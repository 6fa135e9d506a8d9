// rescale_test.cpp -- the host arithmetic of `oip rescale` (csrc/oip_rescaleplan.h) as a stand-alone program, meant to be built
// with -fsanitize=address,undefined: the table builder (row sums, K, first[], the identity row, the residue rule, the limits
// n_in = 4 n_out, n_out = 16 n_in and n = 1, the refusals, tables of exactly n_out K values), the size and source-range
// arithmetic against a direct restatement, the scale parser, and the tile plan of rescale.hip: for every pair, kernel and tile
// position the source region the plan reserves holds what the tables read, and its LDS image fits the budget.
// Prints "rescale: N checks, 0 bad" and returns 0, or names what failed.
#include <cstdio>
#include <string>
#include <vector>

#include "oip_rescaleplan.h"

static long checks = 0, bad = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        ++checks;                                                    \
        if (!(c)) {                                                  \
            ++bad;                                                   \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
        }                                                            \
    } while (0)

static const long kPairs[][2] = {{64, 64}, {203, 152}, {203, 51}, {203, 162}, {61, 37}, {50, 200}, {37, 61}, {64, 17}, {517, 130}, {517, 1034}, {33, 528},
                                 {4, 1}, {1, 16}, {1, 1}, {8, 2}, {3, 48}, {6144, 4915}, {6144, 1536}, {6144, 24576}};

struct Table {
    std::vector<int> first;
    std::vector<int16_t> taps;                   // exactly n_out * K values: the sanitizer sees a write past them
    int K = 0;
};

static bool build(int kind, long n_in, long n_out, Table *t)
{
    char err[256] = "";
    if (oip_rescale_taps_impl(kind, n_in, n_out, nullptr, nullptr, 0, &t->K, err, sizeof err) != OIP_OK) return false;
    t->first.assign(n_out, 0);
    t->taps.assign((size_t)n_out * t->K, 0);
    return oip_rescale_taps_impl(kind, n_in, n_out, t->first.data(), t->taps.data(), t->taps.size(), &t->K, err, sizeof err) == OIP_OK;
}

static void tables()
{
    const int support[3] = {3, 2, 1};
    for (int kind = 0; kind < 3; ++kind)
        for (const auto &pr : kPairs) {
            const long n_in = pr[0], n_out = pr[1], mx = n_in > n_out ? n_in : n_out;
            Table t;
            CHECK(build(kind, n_in, n_out, &t));
            long k = 0;
            while (k * n_out < support[kind] * mx) ++k;          // ceil by counting
            CHECK(t.K == 2 * k && t.K >= 2 && t.K <= kOipRescaleMaxK);
            CHECK(t.K == oip_rescale_k(kind, n_in, n_out));
            bool sums = true, order = true, mags = true, centre = true;
            for (long o = 0; o < n_out; ++o) {
                int sum = 0, mag = 0;
                for (int j = 0; j < t.K; ++j) sum += t.taps[o * t.K + j], mag += std::abs((int)t.taps[o * t.K + j]);
                sums &= sum == kOipRescaleOne;
                mags &= mag <= 32767;
                order &= o == 0 || t.first[o] >= t.first[o - 1];
                // the centre of o lies between taps K/2 - 1 and K/2:  first + K/2 - 1 <= num / den < first + K/2
                const long num = (2 * o + 1) * n_in - n_out, den = 2 * n_out, c = t.first[o] + t.K / 2 - 1;
                centre &= c * den <= num && num < (c + 1) * den;
                centre &= t.first[o] == oip_rescale_first(n_in, n_out, t.K, o);
                const long near = oip_rescale_nearest(n_in, n_out, o);
                centre &= near >= 0 && near < n_in && near >= t.first[o] && near <= t.first[o] + t.K - 1;
            }
            CHECK(sums);
            CHECK(mags);
            CHECK(order);
            CHECK(centre);
            if (n_in == n_out) {
                bool ident = true;
                for (long o = 0; o < n_out; ++o)
                    for (int j = 0; j < t.K; ++j) ident &= t.taps[o * t.K + j] == (t.first[o] + j == o ? kOipRescaleOne : 0);
                CHECK(ident);
            }
            // the source range of every window of 1, 7 and all outputs against the tables themselves
            for (long outs : {1L, 7L, n_out}) {
                if (outs > n_out) continue;
                bool ok = true;
                for (long o = 0; o + outs <= n_out; o += (outs == n_out ? n_out : 3)) {
                    long s0 = -1, sn = -1;
                    ok &= oip_rescale_src_range_impl(n_in, n_out, t.K, o, outs, &s0, &sn) == OIP_OK;
                    long lo = t.first[o], hi = t.first[o + outs - 1] + t.K - 1;
                    lo = lo < 0 ? 0 : (lo > n_in - 1 ? n_in - 1 : lo);
                    hi = hi < 0 ? 0 : (hi > n_in - 1 ? n_in - 1 : hi);
                    ok &= s0 == lo && sn == hi - lo + 1 && s0 >= 0 && s0 + sn <= n_in;
                }
                CHECK(ok);
            }
            // the extent the tile plan reserves for T outputs holds what any T consecutive rows read
            for (int T : {1, 2, 4, 8, 16, 32, 64, 128}) {
                const int ext = oip_rescale_extent(T, n_in, n_out, t.K);
                bool ok = true;
                for (long o = 0; o < n_out; ++o) {
                    const long last = o + T - 1 < n_out ? o + T - 1 : n_out - 1;
                    ok &= t.first[last] + t.K - t.first[o] <= ext;
                }
                CHECK(ok);
            }
        }
    // the residue goes to the largest tap, the first of equal ones: 2 -> 1 with the triangle has rows 4096 8192 4096 (x 1/2 ...)
    Table t;
    CHECK(build(OIP_RESCALE_LINEAR, 2, 4, &t) && t.K == 2);
    CHECK(build(OIP_RESCALE_LINEAR, 4, 2, &t) && t.K == 4);
    CHECK(t.taps[0] == 2048 && t.taps[1] == 6144 && t.taps[2] == 6144 && t.taps[3] == 2048);
    CHECK(build(OIP_RESCALE_CUBIC, 3, 3, &t) && t.K == 4 && t.taps[1] == kOipRescaleOne);
}

static void refusals()
{
    char err[256];
    int K = 0;
    int first[64];
    int16_t taps[64 * 24];
    auto rc = [&](int kind, long a, long b, int *f, int16_t *t, size_t cap) {
        err[0] = 0;
        return oip_rescale_taps_impl(kind, a, b, f, t, cap, &K, err, sizeof err);
    };
    CHECK(rc(0, 4, 1, first, taps, 24) == OIP_OK && K == 24);
    CHECK(rc(0, 5, 1, first, taps, 64 * 24) == OIP_E_INVALID && std::string(err).find("overviews") != std::string::npos);
    CHECK(rc(0, 401, 100, nullptr, nullptr, 0) == OIP_E_INVALID);
    CHECK(rc(0, 1, 16, first, taps, 64 * 24) == OIP_OK && K == 6);
    CHECK(rc(0, 1, 17, first, taps, 64 * 24) == OIP_E_INVALID && std::string(err).find("16") != std::string::npos);
    CHECK(rc(0, 0, 5, first, taps, 64 * 24) == OIP_E_INVALID && std::string(err).find("empty") != std::string::npos);
    CHECK(rc(0, 5, 0, first, taps, 64 * 24) == OIP_E_INVALID);
    CHECK(rc(0, -1, 5, first, taps, 64 * 24) == OIP_E_INVALID);
    CHECK(rc(3, 5, 5, first, taps, 64 * 24) == OIP_E_INVALID);
    CHECK(rc(-1, 5, 5, first, taps, 64 * 24) == OIP_E_INVALID);
    CHECK(rc(0, 10, 10, first, taps, 59) == OIP_E_INVALID && K == 6);
    CHECK(rc(0, 10, 10, first, taps, 60) == OIP_OK);
    CHECK(rc(0, 10, 10, nullptr, taps, 60) == OIP_E_INVALID);
    CHECK(rc(0, 10, 10, first, nullptr, 60) == OIP_E_INVALID);
    CHECK(rc(0, 1L << 31, 1L << 31, nullptr, nullptr, 0) == OIP_E_INVALID);
    CHECK(oip_rescale_taps_impl(0, 5, 1, nullptr, nullptr, 0, nullptr, nullptr, 0) == OIP_E_INVALID);      // no text wanted
    char tiny[8];
    CHECK(oip_rescale_taps_impl(0, 5, 1, nullptr, nullptr, 0, nullptr, tiny, sizeof tiny) == OIP_E_INVALID && strlen(tiny) == 7);
    long a = 0, b = 0;
    CHECK(oip_rescale_src_range_impl(10, 10, 6, 0, 0, &a, &b) == OIP_OK && b == 0);
    CHECK(oip_rescale_src_range_impl(10, 10, 6, 0, 11, &a, &b) == OIP_E_INVALID);
    CHECK(oip_rescale_src_range_impl(10, 10, 6, 10, 1, &a, &b) == OIP_E_INVALID);
    CHECK(oip_rescale_src_range_impl(10, 10, 5, 0, 1, &a, &b) == OIP_E_INVALID);
    CHECK(oip_rescale_src_range_impl(10, 10, 26, 0, 1, &a, &b) == OIP_E_INVALID);
    CHECK(oip_rescale_src_range_impl(0, 10, 6, 0, 1, &a, &b) == OIP_E_INVALID);
    CHECK(oip_rescale_src_range_impl(10, 10, 6, -1, 1, &a, &b) == OIP_E_INVALID);
    CHECK(oip_rescale_src_range_impl(10, 10, 6, 0, 1, nullptr, &b) == OIP_E_INVALID);
    CHECK(oip_rescale_src_range_impl(1, 1, 6, 0, 1, &a, &b) == OIP_OK && a == 0 && b == 1);
}

static void sizes_and_scales()
{
    long n = 0;
    CHECK(oip_rescale_size_impl(203, 3, 4, &n) == OIP_OK && n == 152);                 // 152.25
    CHECK(oip_rescale_size_impl(203, 1, 4, &n) == OIP_OK && n == 51);                  // 50.75
    CHECK(oip_rescale_size_impl(10, 1, 4, &n) == OIP_OK && n == 3);                    // 2.5 rounds up
    CHECK(oip_rescale_size_impl(6, 1, 4, &n) == OIP_OK && n == 2);                     // 1.5 rounds up
    CHECK(oip_rescale_size_impl(1, 1, 3, &n) == OIP_OK && n == 0);                     // an empty axis is the caller's to refuse
    CHECK(oip_rescale_size_impl(517, 2, 1, &n) == OIP_OK && n == 1034);
    CHECK(oip_rescale_size_impl(60000, 8, 10, &n) == OIP_OK && n == 48000);
    CHECK(oip_rescale_size_impl((1L << 31) - 1, 1, 1, &n) == OIP_OK && n == (1L << 31) - 1);
    CHECK(oip_rescale_size_impl(1L << 31, 1, 1, &n) == OIP_E_INVALID);
    CHECK(oip_rescale_size_impl((1L << 31) - 1, 999999999, 1, &n) == OIP_E_INVALID);   // no overflow on the way
    CHECK(oip_rescale_size_impl(0, 1, 1, &n) == OIP_E_INVALID && oip_rescale_size_impl(5, 0, 1, &n) == OIP_E_INVALID &&
          oip_rescale_size_impl(5, 1, 0, &n) == OIP_E_INVALID && oip_rescale_size_impl(5, 1, 1, nullptr) == OIP_E_INVALID);
    // every pair as a fraction and back
    for (const auto &pr : kPairs) {
        const std::string s = std::to_string(pr[1]) + "/" + std::to_string(pr[0]);
        long p = 0, q = 0;
        CHECK(oip_rescale_parse_scale(s.c_str(), &p, &q) && p * pr[0] == q * pr[1]);
        CHECK(oip_rescale_size_impl(pr[0], p, q, &n) == OIP_OK && n == pr[1]);
    }
    struct { const char *s; long p, q; } good[] = {{"0.8", 4, 5}, {"1/2", 1, 2}, {"2/3", 2, 3}, {"4", 4, 1}, {"1.25", 5, 4}, {"0.25", 1, 4}, {"16", 16, 1},
                                                    {".5", 1, 2}, {"2.", 2, 1}, {"10/4", 5, 2}, {"0.33333333", 33333333, 100000000}, {"007", 7, 1},
                                                    {"1.000", 1, 1}, {"999999999/999999999", 1, 1}};
    for (const auto &g : good) {
        long p = 0, q = 0;
        CHECK(oip_rescale_parse_scale(g.s, &p, &q) && p == g.p && q == g.q);
    }
    for (const char *s : {"", "0", "0.0", "0/5", "5/0", "-1", "+2", "1e3", " 1", "1 ", "1/2/3", "1.2/3", "1/2.5", "/2", "1/", ".", "abc", "1.2.3",
                          "1234567890", "0.1234567890", "12345.67890", "0x10", "1,5"}) {
        long p = 7, q = 7;
        CHECK(!oip_rescale_parse_scale(s, &p, &q));
    }
    long p = 0;
    CHECK(!oip_rescale_parse_scale(nullptr, &p, &p) && !oip_rescale_parse_scale("1", nullptr, &p));
}

// the tile plan at the ratios of the pairs, both axes crossed: inside the budget, tiles of whole 16-byte stores, never empty
static void plans()
{
    for (int kind = 0; kind < 3; ++kind)
        for (const auto &px : kPairs)
            for (const auto &py : kPairs)
                for (int spp : {1, 4})
                    for (bool nodata : {false, true}) {
                        const int Kx = oip_rescale_k(kind, px[0], px[1]), Ky = oip_rescale_k(kind, py[0], py[1]);
                        const OipRescaleTile t = oip_rescale_tile(px[0], px[1], py[0], py[1], spp, Kx, Ky, nodata);
                        CHECK(t.lds <= kOipRescaleLds && t.lds == oip_rescale_tile_lds(t, spp, Kx, nodata));
                        CHECK(t.th >= kOipRescaleLines && t.th <= kOipRescaleTileH && t.th % kOipRescaleLines == 0 && t.tw >= 1 && t.tw * spp % 8 == 0 &&
                              t.tw * spp <= kOipRescaleTileWs);
                        CHECK(t.sh == oip_rescale_extent(t.th, py[0], py[1], Ky) && t.sw == oip_rescale_extent(t.tw, px[0], px[1], Kx) && t.sh >= Ky &&
                              t.sw >= Kx);
                        CHECK(t.pitch % 8 == 0 && t.pitch >= t.sw * spp + 7);
                    }
}

int main()
{
    tables();
    refusals();
    sizes_and_scales();
    plans();
    printf("rescale: %ld checks, %ld bad\n", checks, bad);
    return bad ? 1 : 0;
}
