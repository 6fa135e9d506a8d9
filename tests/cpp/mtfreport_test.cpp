// Stand-alone check of the report of `oip mtf` (csrc/oip_mtfreport.hpp) under ASan + UBSan: a report written by WriteMtfReport
// parses back with the pooled median, p75 and p90 bit for bit; its rows come out in (band, axis, ty, tx) order whatever order
// they went in; the parser is fed truncated, overlong, non-numeric, doubled and summary-less reports and refuses each with a
// message; MtfcValueOf clamps and refuses as `oip mtfc --mtf` states; and the three host entry points behind the report
// (csrc/host.cpp) run on tables of exactly the stated sizes.  The values themselves are compared with the Python restatement
// in tests/test_mtf_cpu.py.
#include <cmath>
#include <cstring>
#include <memory>

#include "oip_mtfreport.hpp"

using namespace OIPGPU;

static int bad = 0, checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { ++bad; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

static bool same_bits(double x, double y) { return memcmp(&x, &y, sizeof x) == 0; }

static void put(const std::string &path, const std::string &text)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) { printf("FAILED: cannot write %s\n", path.c_str()); ++bad; return; }
    fwrite(text.data(), 1, text.size(), f);
    fclose(f);
}

// values that need all 17 digits
static double value(int band, int axis, int k) { return 0.05 + 1.0 / (3.0 + band + 7.0 * axis + 0.37 * k); }

static void round_trip(const std::string &path)
{
    for (int nb : {1, 4})
        for (int axes : {1, 2, 3}) {
            std::vector<std::vector<MtfGroup>> groups(nb, std::vector<MtfGroup>(2));
            std::vector<MtfRow> rows;
            std::vector<double> pooled[2];
            for (int b = nb - 1; b >= 0; --b)                          // rows go in backwards
                for (int a = 1; a >= 0; --a) {
                    if (!(axes >> a & 1)) continue;
                    MtfGroup &g = groups[b][a];
                    const int n = (b == 2 && a == 0) ? 0 : 5 + 3 * b + a;      // a band without a value on x
                    g.tiles = 1000 + b;
                    g.status[0] = n + 2; g.emptybin = 2;
                    for (int k = 1; k < 8; ++k) g.status[k] = 10 * k + a;
                    for (int k = n - 1; k >= 0; --k) {
                        MtfRow r;
                        r.band = b + 1; r.axis = a; r.ty = 100000 + k / 3; r.tx = 50 - k % 3; r.polarity = k & 1 ? 1 : -1; r.slopeQ = (k & 1 ? 1 : -1) * (400000 + k);
                        r.sumS0 = 64001 + k; r.mtf = value(b, a, k);
                        rows.push_back(r);
                        g.values.push_back(r.mtf);
                        pooled[a].push_back(r.mtf);
                    }
                }
            FILE *f = fopen(path.c_str(), "w");
            CHECK(f != nullptr);
            if (!f) return;
            CHECK(WriteMtfReport(f, "oip mtf image=x axis=both columns=band,axis,ty,tx,polarity,slope_q,contrast,mtf", rows, groups, axes));
            CHECK(fclose(f) == 0);
            MtfAxisSummary s[2];
            std::string err;
            CHECK(ParseMtfReport(path, s, &err));
            for (int a = 0; a < 2; ++a) {
                CHECK(s[a].present == ((axes >> a & 1) != 0));
                if (!s[a].present) continue;
                CHECK(s[a].values == pooled[a].size());
                double med = 0, p75 = 0, p90 = 0;
                CHECK(oip_mtf_summary(pooled[a].data(), (long)pooled[a].size(), &med, &p75, &p90) == OIP_OK);
                CHECK(same_bits(s[a].median, med) && same_bits(s[a].p75, p75) && same_bits(s[a].p90, p90));
                CHECK(med <= p75 && p75 <= p90);
            }
            // the rows: one per value, sorted, the numbers as they went in
            f = fopen(path.c_str(), "r");
            CHECK(f != nullptr);
            if (!f) return;
            char line[4098];
            size_t n = 0;
            int summaries = 0;
            long prev[4] = {0, 0, 0, 0};
            while (fgets(line, sizeof line, f)) {
                if (line[0] == '#') { summaries += strncmp(line, "# band ", 7) == 0 || strncmp(line, "# all ", 6) == 0; continue; }
                int b = 0, pol = 0, q = 0;
                char ax = 0;
                long ty = 0, tx = 0;
                double c = 0, m = 0;
                CHECK(sscanf(line, "%d,%c,%ld,%ld,%d,%d,%lf,%lf", &b, &ax, &ty, &tx, &pol, &q, &c, &m) == 8);
                const long key[4] = {b, ax == 'y', ty, tx};
                CHECK(n == 0 || std::lexicographical_compare(prev, prev + 4, key, key + 4));
                memcpy(prev, key, sizeof key);
                const int k = (int)((ty - 100000) * 3 + (50 - tx));
                CHECK(same_bits(m, value(b - 1, ax == 'y', k)) && c == (64001 + k) / 32.0 && pol == (k & 1 ? 1 : -1) && q == pol * (400000 + k));
                ++n;
            }
            fclose(f);
            CHECK(n == rows.size());
            const int measured = (axes & 1) + (axes >> 1);
            CHECK(summaries == (nb + 1) * measured);
        }
}

static void hostile(const std::string &path)
{
    const std::string head = "# oip mtf image=x\n1,x,0,0,1,500000,2000.00000,0.25\n";
    const std::string x = "# all axis x: tiles 9 ok 3 nodata 0 flat 0 lowcontrast 0 textured 0 offcentre 0 slant 6 curved 0 emptybin 0 values 3 median 0.25 p75 0.3 p90 0.35\n";
    const std::string y = "# all axis y: tiles 9 ok 0 nodata 0 flat 0 lowcontrast 0 textured 0 offcentre 0 slant 9 curved 0 emptybin 0 values 0\n";
    MtfAxisSummary s[2];
    std::string err;
    put(path, head + x + y);
    CHECK(ParseMtfReport(path, s, &err) && s[0].present && s[1].present && s[0].values == 3 && s[1].values == 0 && s[0].p90 == 0.35);
    double m = 0;
    CHECK(MtfcValueOf(s[0], 0, "median", &m, &err) && m == 0.25);
    CHECK(MtfcValueOf(s[0], 0, "p75", &m, &err) && m == 0.3);
    CHECK(MtfcValueOf(s[0], 0, "p90", &m, &err) && m == 0.35);
    CHECK(!MtfcValueOf(s[1], 1, "median", &m, &err) && err.find("axis y") != std::string::npos);
    put(path, head + x);                                               // an axis that was not measured
    CHECK(ParseMtfReport(path, s, &err) && s[0].present && !s[1].present);
    CHECK(!MtfcValueOf(s[1], 1, "median", &m, &err));
    MtfAxisSummary big;
    big.present = true; big.values = 4; big.median = 1.0625; big.p75 = 0.0; big.p90 = 1.0;
    CHECK(MtfcValueOf(big, 0, "median", &m, &err) && m == 1.0);        // above 1: taken as 1
    CHECK(!MtfcValueOf(big, 0, "p75", &m, &err) && err.find("not above 0") != std::string::npos);
    CHECK(MtfcValueOf(big, 0, "p90", &m, &err) && m == 1.0);
    struct { const char *what; std::string text; } cases[] = {
        {"no summary", head},
        {"empty", ""},
        {"no axis", head + "# all axis z: values 3 median 0.25 p75 0.3 p90 0.35\n"},
        {"no colon", head + "# all axis x values 3 median 0.25 p75 0.3 p90 0.35\n"},
        {"no values", head + "# all axis x: tiles 9 median 0.25 p75 0.3 p90 0.35\n"},
        {"no p90", head + "# all axis x: tiles 9 values 3 median 0.25 p75 0.3\n"},
        {"not a number", head + "# all axis x: tiles 9 values 3 median abc p75 0.3 p90 0.35\n"},
        {"nan", head + "# all axis x: tiles 9 values 3 median nan p75 0.3 p90 0.35\n"},
        {"negative", head + "# all axis x: tiles 9 values 3 median -0.25 p75 0.3 p90 0.35\n"},
        {"fraction of a count", head + "# all axis x: tiles 9 values 2.5 median 0.25 p75 0.3 p90 0.35\n"},
        {"glued", head + "# all axis x: tiles 9 values 3 median 0.25x p75 0.3 p90 0.35\n"},
        {"twice", head + x + x},
        {"truncated", head + x.substr(0, x.size() - 30)},
        {"overlong", head + "# all axis x: values 3 " + std::string(5000, 'a') + " median 0.25 p75 0.3 p90 0.35\n"},
    };
    for (const auto &c : cases) {
        put(path, c.text);
        s[0].present = true;
        err.clear();
        const bool ok = ParseMtfReport(path, s, &err);
        CHECK(!ok && !err.empty() && !s[0].present && !s[1].present);
        if (ok) printf("  accepted: %s\n", c.what);
    }
    CHECK(!ParseMtfReport(path + ".missing", s, &err) && err.find("open") != std::string::npos);
}

static void host_entry_points()
{
    // exactly 64 + 64 entries, on the heap so that a read past either end is seen
    std::unique_ptr<uint32_t[]> sum(new uint32_t[64]), cnt(new uint32_t[64]);
    for (int b = 0; b < 64; ++b) { cnt[b] = 8; sum[b] = 8u * (b < 32 ? 1000u : 3000u); }
    double m = -1.0;
    CHECK(oip_mtf_tile(1, sum.get(), cnt.get(), &m) == OIP_OK && m > 1.05 && m < 1.06);   // a step between two bins: 1 / q^2
    double m2 = -1.0;
    for (int b = 0; b < 64; ++b) sum[b] = 8u * (b < 32 ? 3000u : 1000u);
    CHECK(oip_mtf_tile(-1, sum.get(), cnt.get(), &m2) == OIP_OK && same_bits(m, m2));     // the other polarity
    CHECK(oip_mtf_tile(1, sum.get(), cnt.get(), &m2) == OIP_MTF_NO_VALUE);                // A0 < 0
    cnt[63] = 0;
    CHECK(oip_mtf_tile(-1, sum.get(), cnt.get(), &m2) == OIP_MTF_NO_VALUE);
    cnt[63] = 8; cnt[0] = 0;
    CHECK(oip_mtf_tile(-1, sum.get(), cnt.get(), &m2) == OIP_MTF_NO_VALUE);
    cnt[0] = 8;
    for (int b = 0; b < 64; ++b) sum[b] = 8000u;
    CHECK(oip_mtf_tile(1, sum.get(), cnt.get(), &m2) == OIP_MTF_NO_VALUE);                // flat: A0 == 0
    CHECK(oip_mtf_tile(0, sum.get(), cnt.get(), &m2) == OIP_E_INVALID && oip_mtf_tile(2, sum.get(), cnt.get(), &m2) == OIP_E_INVALID);
    CHECK(oip_mtf_tile(1, nullptr, cnt.get(), &m2) == OIP_E_INVALID && oip_mtf_tile(1, sum.get(), cnt.get(), nullptr) == OIP_E_INVALID);
    for (long n : {1L, 2L, 3L, 4L, 5L, 10L, 11L, 100L, 1001L}) {
        std::unique_ptr<double[]> v(new double[n]);
        for (long i = 0; i < n; ++i) v[i] = (double)((i * 7919) % n);   // a permutation of 0..n-1 for these n
        double med = -1, p75 = -1, p90 = -1;
        CHECK(oip_mtf_summary(v.get(), n, &med, &p75, &p90) == OIP_OK);
        CHECK(med == (double)((n - 1) / 2) && p75 == (double)(3 * (n - 1) / 4) && p90 == (double)(9 * (n - 1) / 10));
        CHECK(v[n - 1] == (double)(((n - 1) * 7919) % n));              // the input is not sorted in place
    }
    double d = 0;
    const double one = 1.0, nan = std::nan("");
    CHECK(oip_mtf_summary(&one, 0, &d, &d, &d) == OIP_E_INVALID && oip_mtf_summary(nullptr, 1, &d, &d, &d) == OIP_E_INVALID);
    CHECK(oip_mtf_summary(&nan, 1, &d, &d, &d) == OIP_E_INVALID && oip_mtf_summary(&one, 1, nullptr, &d, &d) == OIP_E_INVALID);
    CHECK(oip_mtf_tv_slack(0.0) == 0 && oip_mtf_tv_slack(5.0) == 240 && oip_mtf_tv_slack(5.01) == 241 && oip_mtf_tv_slack(20.0) == 960);
    CHECK(oip_mtf_tv_slack(1365.3125) == 65535 && oip_mtf_tv_slack(1e300) == 65535 && oip_mtf_tv_slack(INFINITY) == 65535);
    CHECK(oip_mtf_tv_slack(-0.5) == -1 && oip_mtf_tv_slack(nan) == -1);
}

int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: mtfreport_test SCRATCH_FILE\n"); return 2; }
    round_trip(argv[1]);
    hostile(argv[1]);
    host_entry_points();
    remove(argv[1]);
    printf("%d checks, %d bad\n", checks, bad);
    return bad ? 1 : 0;
}
