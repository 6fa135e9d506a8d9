// Stand-alone check of the host side of `oip regcheck` under ASan + UBSan: RegIntersect (csrc/oip_regreport.hpp) against a
// per-pixel restatement over every placement of two small images, WriteRegReport on record buffers of exactly the stated size
// (one tile, a grid, flagged tiles only) with the file read back, and oip_match_grid / oip_match_peak / oip_match_summary
// (csrc/host.cpp) at the ends of their ranges.  The values themselves are compared with the numpy restatement in
// tests/test_regcheck_cpu.py; here the identities that need no second implementation.
#include <cmath>
#include <cstring>
#include <memory>

#include "oip_regreport.hpp"

using namespace OIPGPU;

static int bad = 0, checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { ++bad; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

template <typename T> static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n]); }

static void intersections()
{
    for (long w1 = 1; w1 <= 4; ++w1)
        for (long w2 = 1; w2 <= 4; ++w2)
            for (long s = -6; s <= 6; ++s) {
                // pixels of image 1 (x in [0, w1)) that image 2 (x - s in [0, w2)) covers; the same rule serves both axes
                long lo = -1, n = 0;
                for (long x = 0; x < w1; ++x)
                    if (x - s >= 0 && x - s < w2) { if (lo < 0) lo = x; ++n; }
                RegOverlap o;
                const bool any = RegIntersect(w1, 3, w2, 2, s, 1, &o);
                CHECK(any == (n > 0));
                if (any) CHECK(o.ax == lo && o.w == n && o.bx == lo - s && o.ay == 1 && o.by == 0 && o.h == 2);
                RegOverlap t;
                const bool anyT = RegIntersect(3, w1, 2, w2, 1, s, &t);
                CHECK(anyT == (n > 0));
                if (anyT) CHECK(t.ay == lo && t.h == n && t.by == lo - s && t.ax == 1 && t.bx == 0 && t.w == 2);
            }
}

// a record with a clean peak at (dy, dx) = (pj - S, pi - S): template sums of variance > 0, the peak's sab above its neighbours'
static void fill(uint64_t *r, int T, int S, int pj, int pi, uint64_t bad_a, bool flat)
{
    const int K = 2 * S + 1;
    const uint64_t n = (uint64_t)T * T, sa = n * 100 + n, saa = n * 10000 + 200 * n + 3 * n, sb = n * 100, sbb = n * 10000 + 9000, base = sa * sb / n;
    memset(r, 0, OIP_MATCH_RECORD_WORDS * sizeof(uint64_t));
    r[0] = flat ? n * 100 : sa;
    r[1] = flat ? n * 10000 : saa;
    r[2] = bad_a;
    r[4] = (uint64_t)(pj * K + pi);
    const int nj[5] = {pj, pj, pj, pj - 1, pj + 1}, ni[5] = {pi, pi - 1, pi + 1, pi, pi};
    const uint64_t up[5] = {40, 10, 30, 20, 5};
    for (int k = 0; k < 5; ++k)
        if (nj[k] >= 0 && nj[k] < K && ni[k] >= 0 && ni[k] < K) { r[5 + 3 * k] = sb; r[6 + 3 * k] = sbb; r[7 + 3 * k] = base + up[k]; }
}

static void report(const char *path, int nx, long ny, int T, int S, int scale, bool all_flagged)
{
    const long n = (long)nx * ny;
    auto rec = exact<uint64_t>((size_t)n * OIP_MATCH_RECORD_WORDS);
    const int K = 2 * S + 1;
    for (long t = 0; t < n; ++t) fill(rec.get() + t * OIP_MATCH_RECORD_WORDS, T, S, (int)(t % K), (int)((t / K) % K), all_flagged ? 1 : 0, t % 7 == 6);
    RegGrid g;
    g.T = T; g.S = S; g.step = T / 2; g.x0 = S; g.y0 = S; g.nx = nx; g.ny = ny; g.scale = scale; g.originX = 3; g.originY = 5;
    FILE *f = fopen(path, "w");
    CHECK(f != nullptr);
    if (!f) return;
    RegSummary sum;
    CHECK(WriteRegReport(f, "params of the run", rec.get(), g, -1.0, &sum));
    fclose(f);
    CHECK(sum.tiles == n);
    // read back: the first line, n tile lines whose x, y follow the grid, `#` lines to the end
    f = fopen(path, "r");
    CHECK(f != nullptr);
    if (!f) return;
    char line[1024];
    CHECK(fgets(line, sizeof line, f) && strcmp(line, "# params of the run\n") == 0);
    long used = 0;
    for (long t = 0; t < n; ++t) {
        long x = 0, y = 0;
        double dx = 0, dy = 0, sc = 0;
        int fl = -1;
        CHECK(fgets(line, sizeof line, f) && sscanf(line, "%ld,%ld,%lf,%lf,%lf,%d", &x, &y, &dx, &dy, &sc, &fl) == 6);
        CHECK(x == (3 + S + (t % nx) * (T / 2) + T / 2) * scale && y == (5 + S + (t / nx) * (T / 2) + T / 2) * scale);
        const int pj = (int)(t % K), pi = (int)((t / K) % K);
        const bool edge = pj == 0 || pj == K - 1 || pi == 0 || pi == K - 1, flat = t % 7 == 6;
        CHECK(fl == ((all_flagged ? OIP_MATCH_NODATA : 0) | (edge ? OIP_MATCH_EDGE : 0) | (flat ? OIP_MATCH_FLAT | OIP_MATCH_WEAK : 0)));
        CHECK(fabs(dx - (pi - S)) <= 0.5 && fabs(dy - (pj - S)) <= 0.5 && (flat ? sc == OIP_MATCH_NO_SCORE : (sc > 0.0 && sc <= 1.0)));
        used += fl == 0;
    }
    int tail = 0;
    while (fgets(line, sizeof line, f)) { CHECK(line[0] == '#'); ++tail; }
    fclose(f);
    CHECK(tail == 3 && (long)sum.s[0] == used && (!all_flagged || used == 0));
    if (used == 0) for (int k = 0; k < 8; ++k) CHECK(sum.s[k] == 0.0);
}

static void entries()
{
    int x0 = -1, nx = -1;
    long y0 = -1, ny = -1;
    CHECK(oip_match_grid(8 + 2, 8 + 2, 8, 1, 1, &x0, &y0, &nx, &ny) == OIP_OK && x0 == 1 && y0 == 1 && nx == 1 && ny == 1);
    CHECK(oip_match_grid(2147483647, 1L << 40, 128, 16, 1, &x0, &y0, &nx, &ny) == OIP_OK && nx == 2147483647 - 160 + 1 && ny == (1L << 40) - 160 + 1);
    CHECK(oip_match_grid(9, 100, 8, 1, 1, &x0, &y0, &nx, &ny) == OIP_E_INVALID && nx == 0 && ny == 0);
    CHECK(oip_match_grid(100, 100, 8, 1, 1, nullptr, &y0, &nx, &ny) == OIP_E_INVALID);
    // sums at the top of their range: T = 128, every sample 65535 in both images but one (a variance of its own)
    uint64_t r[OIP_MATCH_RECORD_WORDS] = {0};
    const uint64_t n = 128 * 128, m = 65535;
    r[0] = n * m - 1; r[1] = (n - 1) * m * m + (m - 1) * (m - 1); r[4] = 16 * 33 + 16;
    for (int k = 0; k < 5; ++k) { r[5 + 3 * k] = r[0]; r[6 + 3 * k] = r[1]; r[7 + 3 * k] = r[1] - (uint64_t)k; }
    double dx = 9, dy = 9, sc = 9;
    int fl = -1;
    CHECK(oip_match_peak(r, 128, 16, 0.5, &dx, &dy, &sc, &fl) == OIP_OK && fl == 0 && sc == 1.0 && fabs(dx) <= 0.5 && fabs(dy) <= 0.5);
    CHECK(oip_match_peak(r, 128, 16, 0.5, &dx, &dy, &sc, nullptr) == OIP_E_INVALID);
    double out[8];
    CHECK(oip_match_summary(nullptr, nullptr, nullptr, 0, out) == OIP_OK && out[0] == 0.0);
    CHECK(oip_match_summary(nullptr, nullptr, nullptr, 1, out) == OIP_E_INVALID);
    const double one_x[1] = {3.0}, one_y[1] = {-4.0};
    const int one_f[1] = {0};
    CHECK(oip_match_summary(one_x, one_y, one_f, 1, out) == OIP_OK && out[0] == 1.0 && out[1] == 3.0 && out[2] == -4.0 && out[3] == 0.0 && out[5] == 5.0 &&
          out[6] == 5.0 && out[7] == 5.0);
}

int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: regreport_test REPORT.csv\n"); return 2; }
    intersections();
    entries();
    report(argv[1], 1, 1, 8, 1, 1, false);
    report(argv[1], 7, 5, 16, 3, 1, false);
    report(argv[1], 3, 11, 64, 4, 4, false);
    report(argv[1], 4, 4, 128, 16, 2, true);
    printf("%d checks, %d bad\n", checks, bad);
    return bad ? 1 : 0;
}
