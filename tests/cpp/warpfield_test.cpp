// Stand-alone check of the host side of `oip regfix` under ASan + UBSan: oip_regfix_load_report (csrc/host.cpp over
// csrc/oip_warpfield.hpp) on minimal and malformed reports with node buffers of exactly the stated size, and oip_regfix_fill /
// oip_regfix_smooth on lattices of one node, one line and one column.  The values themselves are compared with the numpy
// restatement in tests/test_regfix_cpu.py; here: every malformed input is refused with a message and nothing is read or written
// outside a buffer.
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "oip_warpfield.hpp"

using namespace OIPGPU;

static int bad = 0, checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { ++bad; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

template <typename T> static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n ? n : 1]); }

static const char *kHead = "# oip regcheck image1=a b.TIFF image2=scale=9 x.TIFF band1=1 band2=3 scale=2 shift-x=-4 shift-y=6 tile=16 columns=x,y,dx,dy,score,flags\n";

static std::string path_;
static int load(const std::string &text, long w, long h, long cap, long *geom, int32_t *x, int32_t *y, std::string *msg = nullptr)
{
    FILE *f = fopen(path_.c_str(), "wb");
    if (!f) return -1;
    fwrite(text.data(), 1, text.size(), f);
    fclose(f);
    char err[256] = "";
    const int rc = oip_regfix_load_report(path_.c_str(), w, h, x, y, cap, geom, err, sizeof err);
    if (msg) *msg = err;
    return rc;
}

// the tile lines of an nx x ny lattice at (x0 + i step, y0 + j step) with dx = i + j / 4, dy = -j / 2 and the given flags
static std::string lattice(int nx, int ny, long x0, long y0, long stepx, long stepy, const std::vector<int> &flags)
{
    std::string s;
    char line[128];
    for (int j = 0; j < ny; ++j)
        for (int i = 0; i < nx; ++i) {
            snprintf(line, sizeof line, "%ld,%ld,%.4f,%.4f,%.6f,%d\n", x0 + i * stepx, y0 + j * stepy, i + j / 4.0, -j / 2.0, 0.9, flags.empty() ? 0 : flags[(size_t)j * nx + i]);
            s += line;
        }
    return s + "# tiles ...\n# count,mean_dx\n# 1,2\n";
}

static void good_reports()
{
    long g[8];
    // one tile: a 1 x 1 lattice, steps 1
    auto x = exact<int32_t>(1), y = exact<int32_t>(1);
    CHECK(load(std::string(kHead) + "20,40,1.5,-0.25,0.9,0\n", 0, 0, 1, g, x.get(), y.get()) == OIP_OK);
    CHECK(g[0] == 1 && g[1] == 1 && g[2] == 10 + 4 && g[3] == 20 - 6 && g[4] == 1 && g[5] == 1 && g[6] == 3 && g[7] == 1 && x[0] == 1536 && y[0] == -256);
    // no trailing newline, CR LF line ends
    CHECK(load(std::string(kHead) + "20,40,1.5,-0.25,0.9,0", 0, 0, 1, g, x.get(), y.get()) == OIP_OK && x[0] == 1536);
    std::string crlf = std::string(kHead) + "20,40,1.5,-0.25,0.9,0\r\n";
    crlf.insert(strlen(kHead) - 1, "\r");
    CHECK(load(crlf, 0, 0, 1, g, x.get(), y.get()) == OIP_OK && x[0] == 1536 && g[6] == 3);
    // grids: one line, one column, 5 x 3 with holes; buffers of exactly nx * ny
    for (auto dims : {std::pair<int, int>{4, 1}, {1, 5}, {5, 3}}) {
        const int nx = dims.first, ny = dims.second;
        std::vector<int> fl((size_t)nx * ny, 0);
        if (nx * ny > 2) { fl[1] = 4; fl[(size_t)nx * ny - 1] = 9; }
        auto X = exact<int32_t>((size_t)nx * ny), Y = exact<int32_t>((size_t)nx * ny);
        CHECK(load(std::string(kHead) + lattice(nx, ny, 20, 40, 32, 16, fl), 0, 0, (long)nx * ny, g, X.get(), Y.get()) == OIP_OK);
        CHECK(g[0] == nx && g[1] == ny && g[4] == (nx > 1 ? 16 : 1) && g[5] == (ny > 1 ? 8 : 1) && g[7] == nx * ny - (nx * ny > 2 ? 2 : 0));
        CHECK(X[0] == 0 && Y[0] == 0);
        for (int q = 0; q < nx * ny; ++q) CHECK(std::abs(X[q]) <= 65536 && std::abs(Y[q]) <= 65536);
        std::string msg;
        CHECK(load(std::string(kHead) + lattice(nx, ny, 20, 40, 32, 16, fl), 0, 0, (long)nx * ny - 1, g, X.get(), Y.get(), &msg) == OIP_E_INVALID && msg.find("room for") != std::string::npos);
        // the image the field is for: the last node at (14 + (nx - 1) 16, 14 + (ny - 1) 8)
        const long lx = 14 + (nx - 1) * 16, ly = 14 + (ny - 1) * 8;
        CHECK(load(std::string(kHead) + lattice(nx, ny, 20, 40, 32, 16, fl), lx + 1, ly + 1, (long)nx * ny, g, X.get(), Y.get()) == OIP_OK);
        CHECK(load(std::string(kHead) + lattice(nx, ny, 20, 40, 32, 16, fl), lx, ly + 1, (long)nx * ny, g, X.get(), Y.get(), &msg) == OIP_E_INVALID && msg.find("outside") != std::string::npos);
        CHECK(load(std::string(kHead) + lattice(nx, ny, 20, 40, 32, 16, fl), lx + 1, ly, (long)nx * ny, g, X.get(), Y.get()) == OIP_E_INVALID);
    }
}

static void malformed_reports()
{
    const std::string H = kHead, T = "20,40,1.5,-0.25,0.9,0\n";
    const std::string noScale = "# oip regcheck image1=a band2=1 shift-x=0 shift-y=0\n", noBand = "# oip regcheck scale=1 shift-x=0 shift-y=0\n";
    const std::string cases[] = {
        "", "\n", "# something else\n" + T, H, H + "# only comments\n", noScale + T, noBand + T, "# oip regcheck scale=1 band2=1 shift-y=0\n" + T,
        "# oip regcheck scale=1 band2=1 shift-x=0\n" + T, "# oip regcheck scale=0 band2=1 shift-x=0 shift-y=0\n" + T,
        "# oip regcheck scale=65 band2=1 shift-x=0 shift-y=0\n" + T, "# oip regcheck scale=1 band2=5 shift-x=0 shift-y=0\n" + T,
        "# oip regcheck scale=1 band2=0 shift-x=0 shift-y=0\n" + T, "# oip regcheck scale=x band2=1 shift-x=0 shift-y=0\n" + T,
        "# oip regcheck scale=1 band2=1 shift-x=99999999999999999999 shift-y=0\n" + T, "# oip regcheck scale= band2=1 shift-x=0 shift-y=0\n" + T,
        H + "20,40,1.5,-0.25,0.9\n", H + "20,40,1.5,-0.25,0.9,0,7\n", H + "20,40,1.5\n", H + ",,,,,\n", H + "20,40,nan,-0.25,0.9,0\n", H + "20,40,1.5,inf,0.9,0\n",
        H + "20,40,1.5,-0.25,-inf,0\n", H + "20,40,1e999,-0.25,0.9,0\n", H + "20,40,64.5,-0.25,0.9,0\n", H + "20,40,1.5,-64.001,0.9,0\n", H + "20,40,1.5x,-0.25,0.9,0\n",
        H + "20,40, 1.5,-0.25,0.9,0\n", H + "21,40,1.5,-0.25,0.9,0\n", H + "20,41,1.5,-0.25,0.9,0\n", H + "-20,40,1.5,-0.25,0.9,0\n", H + "20,40,1.5,-0.25,0.9,16\n",
        H + "20,40,1.5,-0.25,0.9,-1\n", H + "20,40,1.5,-0.25,0.9,1\n" /* no usable tile */, H + "2e1,40,1.5,-0.25,0.9,0\n", H + "99999999999999999999,40,1.5,-0.25,0.9,0\n",
        H + T + "52,40,1,1,0.9,0\n84,40,1,1,0.9,0\n20,56,1,1,0.9,0\n52,56,1,1,0.9,0\n" /* ragged: 3 + 2 */,
        H + T + "52,40,1,1,0.9,0\n20,56,1,1,0.9,0\n54,56,1,1,0.9,0\n" /* irregular in x */,
        H + T + "52,40,1,1,0.9,0\n20,56,1,1,0.9,0\n52,56,1,1,0.9,0\n20,74,1,1,0.9,0\n52,74,1,1,0.9,0\n" /* irregular in y */,
        H + T + "20,40,1,1,0.9,0\n" /* the same position twice */, H + "52,40,1,1,0.9,0\n20,40,1,1,0.9,0\n" /* descending */,
        H + T + "20,24,1,1,0.9,0\n" /* descending lines */, H + std::string("20,40,1.5,-0.25,0.9,0\0 20", 25) + "\n",
        H + "0,40,1,1,0.9,0\n262146,40,1,1,0.9,0\n" /* a step above 65536 image-2 pixels */,
    };
    long g[8];
    auto x = exact<int32_t>(8), y = exact<int32_t>(8);
    int k = 0;
    for (const std::string &c : cases) {
        std::string msg;
        const int rc = load(c, 0, 0, 8, g, x.get(), y.get(), &msg);
        if (rc != OIP_E_INVALID || msg.empty()) printf("case %d: rc %d `%s'\n", k, rc, msg.c_str());
        CHECK(rc == OIP_E_INVALID && !msg.empty());
        ++k;
    }
    char err[64];
    CHECK(oip_regfix_load_report("/nonexistent/report.csv", 0, 0, x.get(), y.get(), 8, g, err, sizeof err) == OIP_E_IO);
    CHECK(oip_regfix_load_report(nullptr, 0, 0, x.get(), y.get(), 8, g, err, sizeof err) == OIP_E_INVALID);
    CHECK(oip_regfix_load_report(path_.c_str(), 0, 0, nullptr, y.get(), 8, g, err, sizeof err) == OIP_E_INVALID);
    CHECK(oip_regfix_load_report(path_.c_str(), 0, 0, x.get(), y.get(), 8, nullptr, err, sizeof err) == OIP_E_INVALID);
    CHECK(oip_regfix_load_report(path_.c_str(), -1, 0, x.get(), y.get(), 8, g, nullptr, 0) == OIP_E_INVALID);
}

static void fill_and_smooth()
{
    for (auto dims : {std::pair<int, int>{1, 1}, {1, 6}, {6, 1}, {2, 2}, {7, 5}}) {
        const int nx = dims.first, ny = dims.second, n = nx * ny;
        auto X = exact<int32_t>(n), Y = exact<int32_t>(n);
        auto set = exact<uint8_t>(n);
        for (int q = 0; q < n; ++q) { X[q] = 12345; Y[q] = -54321; set[q] = 0; }
        CHECK(oip_regfix_fill(X.get(), Y.get(), set.get(), nx, ny) == OIP_E_INVALID);          // no node is set
        set[n - 1] = 1;
        X[n - 1] = -65536; Y[n - 1] = 65536;
        CHECK(oip_regfix_fill(X.get(), Y.get(), set.get(), nx, ny) == OIP_OK);
        for (int q = 0; q < n; ++q) CHECK(X[q] == -65536 && Y[q] == 65536);                    // one value spreads to every node
        for (int p = 0; p <= OIP_REGFIX_MAX_SMOOTH; p += 8) {
            CHECK(oip_regfix_smooth(X.get(), Y.get(), nx, ny, p) == OIP_OK);
            for (int q = 0; q < n; ++q) CHECK(X[q] == -65536 && Y[q] == 65536);                // a constant field stays as it is, at the range's ends
        }
        CHECK(oip_regfix_smooth(X.get(), Y.get(), nx, ny, -1) == OIP_E_INVALID && oip_regfix_smooth(X.get(), Y.get(), nx, ny, 17) == OIP_E_INVALID);
        X[0] = 65537;
        set[0] = 1;
        CHECK(oip_regfix_smooth(X.get(), Y.get(), nx, ny, 1) == OIP_E_INVALID && oip_regfix_fill(X.get(), Y.get(), set.get(), nx, ny) == OIP_E_INVALID);
    }
    int32_t v[1] = {0};
    const uint8_t s[1] = {1};
    CHECK(oip_regfix_fill(v, v, s, 0, 1) == OIP_E_INVALID && oip_regfix_fill(v, v, nullptr, 1, 1) == OIP_E_INVALID && oip_regfix_fill(nullptr, v, s, 1, 1) == OIP_E_INVALID);
    CHECK(oip_regfix_smooth(v, v, 1, 0, 1) == OIP_E_INVALID && oip_regfix_smooth(v, nullptr, 1, 1, 1) == OIP_E_INVALID);
    // the floor of a negative mean: (-3 + -4) / 2 = -3.5 -> floor((2 * -7 + 2) / 4) = -3
    int32_t X[3] = {-3, 0, -4}, Y[3] = {3, 0, 4};
    const uint8_t set[3] = {1, 0, 1};
    CHECK(oip_regfix_fill(X, Y, set, 3, 1) == OIP_OK && X[1] == -3 && Y[1] == 4);
    CHECK(WarpFloorDiv(-7, 2) == -4 && WarpFloorDiv(7, 2) == 3 && WarpFloorDiv(-8, 2) == -4 && WarpFloorDiv(0, 4) == 0);
}

int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: warpfield_test REPORT.csv\n"); return 2; }
    path_ = argv[1];
    good_reports();
    malformed_reports();
    fill_and_smooth();
    printf("%d checks, %d bad\n", checks, bad);
    return bad ? 1 : 0;
}
