// Stand-alone check of oip_seam_fit_blocks and oip_seam_line_tables (csrc/host.cpp) under ASan + UBSan: every output buffer
// has exactly the size include/oip_c.h states, at the sizes where an index is most easily one too far -- nb = 1, B = 1,
// L < B, L = 0, a merged tail -- and the nodes include the ends of the 32-bit range, whose products need 64 bits.  The
// values themselves are compared with the Python restatement in tests/test_seam_lines_cpu.py; here only a few identities.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>

#include "oip_c.h"

static int bad = 0, checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { ++bad; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

template <typename T> static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n]); }   // new T[0] is a valid, unusable pointer

static void tables(long L, long B, int spp)
{
    const long nb = L / B > 1 ? L / B : 1;
    auto g = exact<int32_t>((size_t)nb * spp), o = exact<int32_t>((size_t)nb * spp);
    for (long i = 0; i < nb * spp; ++i) {
        g[i] = 16384 + (int32_t)((i * 7919) % 245761);
        o[i] = i % 3 == 0 ? INT32_MIN : (i % 3 == 1 ? INT32_MAX : (int32_t)(-7 + i));
    }
    auto lg = exact<int32_t>((size_t)L * spp), lo = exact<int32_t>((size_t)L * spp);
    CHECK(oip_seam_line_tables(g.get(), o.get(), nb, spp, L, B, lg.get(), lo.get()) == OIP_OK);
    for (long r = 0; r < L; ++r)
        for (int c = 0; c < spp; ++c) {
            if (r <= B / 2 || nb == 1) CHECK(lg[r * spp + c] == g[c] && lo[r * spp + c] == o[c]);
            if (r >= (nb - 1) * B + B / 2) CHECK(lg[r * spp + c] == g[(nb - 1) * spp + c] && lo[r * spp + c] == o[(nb - 1) * spp + c]);
        }
    CHECK(oip_seam_line_tables(g.get(), o.get(), nb + 1, spp, L, B, lg.get(), lo.get()) == OIP_E_INVALID);
}

static void fits(long nb, int spp, int mode)
{
    const size_t plane = 6 * (size_t)spp;
    auto acc = exact<uint64_t>((size_t)nb * plane);
    for (long k = 0; k < nb; ++k)
        for (int c = 0; c < spp; ++c) {
            // 100 pairs of (a, b) = (1000 + k, 900 + c) and 100 of (2000 + k, 1800 + 2 c); every third block empty
            const uint64_t n = k % 3 == 2 ? 0 : 200, a0 = 1000 + k, b0 = 900 + c, a1 = 2000 + k, b1 = 1800 + 2 * c, h = n / 2;
            uint64_t *p = acc.get() + k * plane;
            p[c] = n; p[spp + c] = h * (a0 + a1); p[2 * spp + c] = h * (b0 + b1); p[3 * spp + c] = h * (a0 * a0 + a1 * a1);
            p[4 * spp + c] = h * (b0 * b0 + b1 * b1); p[5 * spp + c] = h * (a0 * b0 + a1 * b1);
        }
    auto G = exact<int32_t>((size_t)nb * spp), O = exact<int32_t>((size_t)nb * spp), G0 = exact<int32_t>(spp), O0 = exact<int32_t>(spp);
    auto sub = exact<int>((size_t)nb * spp), id0 = exact<int>(spp);
    auto rep = exact<double>((size_t)nb * spp * 6);
    char err[8] = "";                                              // a short buffer: messages are cut, not overrun
    for (int with_report = 0; with_report < 2; ++with_report) {
        const int rc = oip_seam_fit_blocks(acc.get(), nb, spp, mode, 0, G.get(), O.get(), sub.get(), G0.get(), O0.get(), id0.get(),
                                           with_report ? rep.get() : nullptr, err, sizeof err);
        CHECK(rc == OIP_OK);
        for (long k = 0; k < nb; ++k)
            for (int c = 0; c < spp; ++c) {
                CHECK(sub[k * spp + c] == (k % 3 == 2 ? 1 : 0));
                if (sub[k * spp + c]) CHECK(G[k * spp + c] == G0[c] && O[k * spp + c] == O0[c]);
            }
    }
    // a strip whose every pair has b = a / 8: the whole-strip error with a cut message
    for (size_t i = 0; i < (size_t)nb * plane; ++i) acc[i] = 0;
    for (long k = 0; k < nb; ++k)
        for (int c = 0; c < spp; ++c) {
            uint64_t *p = acc.get() + k * plane;
            p[c] = 2; p[spp + c] = 8000 + 16000; p[2 * spp + c] = 1000 + 2000; p[3 * spp + c] = 8000ull * 8000 + 16000ull * 16000;
            p[4 * spp + c] = 1000ull * 1000 + 2000ull * 2000; p[5 * spp + c] = 8000ull * 1000 + 16000ull * 2000;
        }
    const int rc = oip_seam_fit_blocks(acc.get(), nb, spp, mode, 0, G.get(), O.get(), sub.get(), G0.get(), O0.get(), id0.get(), nullptr, err, sizeof err);
    CHECK(rc == (mode == OIP_SEAM_OFFSET ? OIP_OK : OIP_E_INVALID));
    CHECK(oip_seam_fit_blocks(acc.get(), 0, spp, mode, 0, G.get(), O.get(), sub.get(), G0.get(), O0.get(), id0.get(), nullptr, nullptr, 0) == OIP_E_INVALID);
}

int main()
{
    const long LB[][2] = {{0, 1}, {0, 8}, {1, 1}, {1, 8}, {5, 8}, {8, 8}, {15, 8}, {16, 8}, {17, 8}, {40, 1}, {257, 50}, {255, 51}, {9, 2}, {1000, 64}};
    for (auto &lb : LB)
        for (int spp : {1, 4}) tables(lb[0], lb[1], spp);
    for (long nb : {1L, 2L, 3L, 7L})
        for (int spp : {1, 4})
            for (int mode : {OIP_SEAM_MOMENTS, OIP_SEAM_GAIN, OIP_SEAM_OFFSET}) fits(nb, spp, mode);
    printf("%d checks, %d bad\n", checks, bad);
    return bad ? 1 : 0;
}
