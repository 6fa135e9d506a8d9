// Stand-alone check of the host side of `oip wallis` under ASan + UBSan: the report writer (csrc/oip_wallisreport.hpp) and
// oip_wallis_grid / oip_wallis_fit (csrc/host.cpp) on tables of exactly the stated sizes -- blocks that are substituted, a
// constant channel, pitched planes, given targets, each refusal.  argv[1]: a directory to write in.
#include <cmath>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <vector>

#include "oip_wallisreport.hpp"

using namespace OIPGPU;

static int bad = 0, checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { ++bad; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

static std::string slurp(const std::string &path)
{
    std::ifstream f(path, std::ios::binary);
    std::stringstream s;
    s << f.rdbuf();
    return s.str();
}

static void report(const std::string &dir)
{
    const std::string params = WallisParamsLine("a b.TIFF", 900, 3, 700, 1, 64, 0.8, 0.6, 0.25, 4.0, 0, 1, 65535, 4095);
    CHECK(params == "oip wallis image=a b.TIFF width=900 line-offset=3 lines=700 samples=1 block=64 contrast=0.80000000000000004 "
                    "brightness=0.59999999999999998 min-gain=0.25 max-gain=4 min-count=0 valid-min=1 valid-max=65535 max-value=4095");
    const double r[9] = {630000, 1249.5, 297.25, 1249.5, 0.1, 165, 2, 64992, 119027};
    const uint64_t counts[3] = {12345678901ull, 10, 0};
    const std::string path = dir + "/report.csv";
    FILE *f = fopen(path.c_str(), "w");
    CHECK(f != nullptr);
    if (!f) return;
    CHECK(WriteWallisReport(f, params, 1, r, counts));
    fclose(f);
    const std::string want = "# " + params +
                             "\nchannel,samples,mean,std,target_mean,target_std,nodes,substituted_nodes,min_gain_q16,max_gain_q16\n"
                             "1,630000,1249.5,297.25,1249.5,0.10000000000000001,165,2,64992,119027\n"
                             "transformed_samples,12345678901\nclamped_low,10\nclamped_high,0\n";
    CHECK(slurp(path) == want);
    CHECK(WallisSummaryLine(0, r).find("band 1: 630000 samples, mean 1249.50 std 297.25") != std::string::npos);
    CHECK(WallisSummaryLine(0, r).find("165 nodes (2 substituted)") != std::string::npos);
    CHECK(std::string(WallisReportNames()[8]) == "max_gain_q16" && std::string(WallisCounterNames()[2]) == "clamped_high");
}

static void grid()
{
    int gw = -1;
    long gh = -1;
    CHECK(oip_wallis_grid(203, 77, 32, &gw, &gh) == OIP_OK && gw == 7 && gh == 3);
    CHECK(oip_wallis_grid(256, 100000, 256, &gw, &gh) == OIP_OK && gw == 1 && gh == 391);
    CHECK(oip_wallis_grid(0, 0, 64, &gw, &gh) == OIP_OK && gw == 0 && gh == 0);
    CHECK(oip_wallis_grid(10, 10, 16, &gw, &gh) == OIP_E_INVALID);
    CHECK(oip_wallis_grid(-1, 10, 32, &gw, &gh) == OIP_E_INVALID);
    CHECK(oip_wallis_grid(10, -1, 32, &gw, &gh) == OIP_E_INVALID);
    CHECK(oip_wallis_grid(10, 10, 32, nullptr, &gh) == OIP_E_INVALID);
}

// moments of a block of n samples that are half `a`, half `b`
static void block(uint64_t n, uint64_t a, uint64_t b, uint64_t *pn, uint64_t *p1, uint64_t *p2)
{
    *pn = n;
    *p1 = n / 2 * a + n / 2 * b;
    *p2 = n / 2 * a * a + n / 2 * b * b;
}

static void fit()
{
    // 2 x 3 nodes, 1 channel, planes 4 apart per line (one entry of padding), heap arrays of exactly the stated size
    const int gw = 3, pitch = 4;
    const long gh = 2;
    const size_t plane = (size_t)(gh - 1) * pitch + gw;                  // the smallest stride the header allows
    std::unique_ptr<uint64_t[]> acc(new uint64_t[3 * plane]());
    uint64_t *n = acc.get(), *s1 = n + plane, *s2 = s1 + plane;
    block(1024, 900, 1100, n + 0, s1 + 0, s2 + 0);                       // mean 1000, std 100
    block(1024, 1900, 2100, n + 1, s1 + 1, s2 + 1);                      // mean 2000, std 100
    block(1024, 1500, 1500, n + 2, s1 + 2, s2 + 2);                      // constant: D == 0
    block(0, 0, 0, n + pitch, s1 + pitch, s2 + pitch);                   // empty
    block(2, 10, 30, n + pitch + 1, s1 + pitch + 1, s2 + pitch + 1);     // the smallest block with a fit: mean 20, std 10
    block(1024, 1000, 3000, n + pitch + 2, s1 + pitch + 2, s2 + pitch + 2);      // mean 2000, std 1000
    std::unique_ptr<int32_t[]> G(new int32_t[6]), O(new int32_t[6]);
    std::unique_ptr<int[]> sub(new int[6]);
    std::unique_ptr<double[]> rep(new double[9]);
    char err[256] = "";
    const double mean = 1000.0, std_ = 100.0;
    CHECK(oip_wallis_fit(acc.get(), pitch, plane, gw, gh, 1, 1.0, 1.0, 0.25, 4.0, 0, &mean, &std_, G.get(), O.get(), sub.get(), rep.get(), err,
                         sizeof err) == OIP_OK);
    // c = b = 1: g = s_t / s, o = m_t - g m
    CHECK(G[0] == 65536 && O[0] == 0 && sub[0] == 0);
    CHECK(G[1] == 65536 && O[1] == -1000 * 256 && sub[1] == 0);
    CHECK(sub[2] == 1 && sub[3] == 1);
    CHECK(G[2] == G[3] && O[2] == O[3]);                                // both take the totals' fit
    CHECK(G[4] == 4 * 65536 && O[4] == (1000 - 4 * 20) * 256 && sub[4] == 0);   // 10 clamped to 4
    CHECK(G[5] == 16384 && O[5] == (1000 - 2000 / 4) * 256 && sub[5] == 0);      // 0.1 clamped to 0.25
    CHECK(rep[0] == 4098.0 && rep[3] == 1000.0 && rep[4] == 100.0 && rep[5] == 6.0 && rep[6] == 2.0 && rep[7] == 16384.0 && rep[8] == 4 * 65536.0);
    CHECK(rep[1] > 1500.0 && rep[1] < 1700.0 && rep[2] > 0.0);
    // the totals' fit is fit(N, A, Q): with the image's own targets it is the identity up to rounding
    CHECK(oip_wallis_fit(acc.get(), pitch, plane, gw, gh, 1, 1.0, 1.0, 0.25, 4.0, 0, nullptr, nullptr, G.get(), O.get(), sub.get(), nullptr, err,
                         sizeof err) == OIP_OK);
    CHECK(G[2] == 65536 && std::abs(O[2]) <= 1);
    // min_count above every block: every node substituted
    CHECK(oip_wallis_fit(acc.get(), pitch, plane, gw, gh, 1, 0.8, 0.6, 0.25, 4.0, 2000, nullptr, nullptr, G.get(), O.get(), sub.get(), rep.get(), err,
                         sizeof err) == OIP_OK);
    CHECK(rep[6] == 6.0 && G[0] == G[5] && O[0] == O[5]);
    // refusals
    CHECK(oip_wallis_fit(acc.get(), pitch, plane, gw, gh, 1, 0.8, 0.6, 0.25, 4.0, 5000, nullptr, nullptr, G.get(), O.get(), sub.get(), nullptr, err,
                         sizeof err) == OIP_E_RUNTIME);
    CHECK(strstr(err, "channel 0") != nullptr);
    const double zero = 0.0, nan = std::nan(""), big = 70000.0, neg = -1.0;
    CHECK(oip_wallis_fit(acc.get(), pitch, plane, gw, gh, 1, 0.8, 0.6, 0.25, 4.0, 0, nullptr, &zero, G.get(), O.get(), sub.get(), nullptr, err, sizeof err) ==
          OIP_E_RUNTIME);
    CHECK(oip_wallis_fit(acc.get(), pitch, plane, gw, gh, 1, 0.8, 0.6, 0.25, 4.0, 0, &nan, &nan, G.get(), O.get(), sub.get(), nullptr, err, sizeof err) == OIP_OK);
    CHECK(oip_wallis_fit(acc.get(), pitch, plane, gw, gh, 1, 0.8, 0.6, 0.25, 4.0, 0, &big, nullptr, G.get(), O.get(), sub.get(), nullptr, err, sizeof err) ==
          OIP_E_INVALID);
    CHECK(oip_wallis_fit(acc.get(), pitch, plane, gw, gh, 1, 0.8, 0.6, 0.25, 4.0, 0, &neg, nullptr, G.get(), O.get(), sub.get(), nullptr, err, sizeof err) ==
          OIP_E_INVALID);
    CHECK(oip_wallis_fit(acc.get(), pitch, plane, gw, gh, 1, 0.8, 0.6, 0.25, 4.0, 0, nullptr, &big, G.get(), O.get(), sub.get(), nullptr, err, sizeof err) ==
          OIP_E_INVALID);
    const double cs[] = {0.0, 1.5, -1.0}, bs[] = {-0.1, 1.1};
    for (double c : cs)
        CHECK(oip_wallis_fit(acc.get(), pitch, plane, gw, gh, 1, c, 0.6, 0.25, 4.0, 0, nullptr, nullptr, G.get(), O.get(), sub.get(), nullptr, nullptr, 0) ==
              OIP_E_INVALID);
    for (double b : bs)
        CHECK(oip_wallis_fit(acc.get(), pitch, plane, gw, gh, 1, 0.8, b, 0.25, 4.0, 0, nullptr, nullptr, G.get(), O.get(), sub.get(), nullptr, nullptr, 0) ==
              OIP_E_INVALID);
    CHECK(oip_wallis_fit(acc.get(), pitch, plane, gw, gh, 1, 0.8, 0.6, 0.0, 4.0, 0, nullptr, nullptr, G.get(), O.get(), sub.get(), nullptr, nullptr, 0) == OIP_E_INVALID);
    CHECK(oip_wallis_fit(acc.get(), pitch, plane, gw, gh, 1, 0.8, 0.6, 0.25, 16.5, 0, nullptr, nullptr, G.get(), O.get(), sub.get(), nullptr, nullptr, 0) == OIP_E_INVALID);
    CHECK(oip_wallis_fit(acc.get(), pitch, plane, gw, gh, 2, 0.8, 0.6, 0.25, 4.0, 0, nullptr, nullptr, G.get(), O.get(), sub.get(), nullptr, nullptr, 0) == OIP_E_INVALID);
    CHECK(oip_wallis_fit(acc.get(), 2, plane, gw, gh, 1, 0.8, 0.6, 0.25, 4.0, 0, nullptr, nullptr, G.get(), O.get(), sub.get(), nullptr, nullptr, 0) == OIP_E_INVALID);
    // planes that overlap are refused at one sample per pixel too: there are three of them
    CHECK(oip_wallis_fit(acc.get(), pitch, plane - 1, gw, gh, 1, 0.8, 0.6, 0.25, 4.0, 0, nullptr, nullptr, G.get(), O.get(), sub.get(), nullptr, nullptr, 0) == OIP_E_INVALID);
    CHECK(oip_wallis_fit(nullptr, pitch, plane, gw, gh, 1, 0.8, 0.6, 0.25, 4.0, 0, nullptr, nullptr, G.get(), O.get(), sub.get(), nullptr, nullptr, 0) == OIP_E_INVALID);
    // a constant channel: its own std is no target; with one given, every node holds the identity
    std::unique_ptr<uint64_t[]> flat(new uint64_t[3]);
    block(4096, 1500, 1500, flat.get(), flat.get() + 1, flat.get() + 2);
    CHECK(oip_wallis_fit(flat.get(), 1, 1, 1, 1, 1, 0.8, 0.6, 0.25, 4.0, 0, nullptr, nullptr, G.get(), O.get(), sub.get(), nullptr, err, sizeof err) == OIP_E_RUNTIME);
    CHECK(strstr(err, "not positive") != nullptr);
    CHECK(oip_wallis_fit(flat.get(), 1, 1, 1, 1, 1, 0.8, 0.6, 0.25, 4.0, 0, nullptr, &std_, G.get(), O.get(), sub.get(), rep.get(), err, sizeof err) == OIP_OK);
    CHECK(G[0] == 65536 && O[0] == 0 && sub[0] == 1 && rep[2] == 0.0 && rep[6] == 1.0);
}

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    report(dir);
    grid();
    fit();
    printf("%d checks, %d bad\n", checks, bad);
    return bad ? 1 : 0;
}
