// Stand-alone check of the host side of `oip denoise` under ASan + UBSan: the table function oip_denoise_thresholds
// (csrc/host.cpp) at the edges of its range, on a buffer of exactly 256 entries, and the path from a report of `oip noise` to the
// tables of a run (ParseNoiseReport, NoiseDenoiseTables of csrc/oip_noisereport.hpp), the band-count mismatch and a band without
// noise included.  The values themselves are compared with the Python restatement in tests/test_denoise_cpu.py.
#include <cmath>
#include <cstring>
#include <memory>

#include "oip_noisereport.hpp"

using namespace OIPGPU;

static int bad = 0, checks = 0;
#define CHECK(c) do { ++checks; if (!(c)) { ++bad; printf("FAILED line %d: %s\n", __LINE__, #c); } } while (0)

static void put(const std::string &path, const std::string &text)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) { printf("FAILED: cannot write %s\n", path.c_str()); ++bad; return; }
    fwrite(text.data(), 1, text.size(), f);
    fclose(f);
}

static void table_function()
{
    std::unique_ptr<uint16_t[]> t(new uint16_t[256]);                  // exactly the stated size
    char err[128] = "";
    // a constant model: sigma 3 at every level, K 2 -> 6; the ceiling of an exact product stays
    CHECK(oip_denoise_thresholds(9.0, 0.0, 2.0, t.get(), err, sizeof err) == OIP_OK);
    for (int l = 0; l < 256; ++l) CHECK(t[l] == 6);
    CHECK(oip_denoise_thresholds(9.0, 0.0, 2.1, t.get(), err, sizeof err) == OIP_OK && t[0] == 7 && t[255] == 7);
    // b alone: sqrt(0.02 * (256 l + 128)), rising with the level
    CHECK(oip_denoise_thresholds(0.0, 0.02, 2.0, t.get(), err, sizeof err) == OIP_OK);
    CHECK(t[0] == (uint16_t)std::ceil(2.0 * std::sqrt(0.02 * 128.0)) && t[255] == (uint16_t)std::ceil(2.0 * std::sqrt(0.02 * 65408.0)));
    for (int l = 1; l < 256; ++l) CHECK(t[l] >= t[l - 1]);
    // a tiny a: the threshold is 1, never 0
    CHECK(oip_denoise_thresholds(1e-300, 0.0, 1.0, t.get(), err, sizeof err) == OIP_OK && t[0] == 1 && t[255] == 1);
    CHECK(oip_denoise_thresholds(5e-324, 0.0, 1e-3, t.get(), err, sizeof err) == OIP_OK && t[0] == 1);
    // saturation: level 255 reaches 65535 first, then every level; a sum that overflows to infinity saturates as well
    CHECK(oip_denoise_thresholds(0.0, 1e6, 1.0, t.get(), err, sizeof err) == OIP_OK && t[0] == 11314 && t[255] == 65535);
    CHECK(oip_denoise_thresholds(1e10, 0.0, 1.0, t.get(), err, sizeof err) == OIP_OK && t[0] == 65535 && t[128] == 65535 && t[255] == 65535);
    CHECK(oip_denoise_thresholds(65535.0 * 65535.0, 0.0, 1.0, t.get(), err, sizeof err) == OIP_OK && t[0] == 65535);
    CHECK(oip_denoise_thresholds(65534.0 * 65534.0, 0.0, 1.0, t.get(), err, sizeof err) == OIP_OK && t[0] == 65534);
    CHECK(oip_denoise_thresholds(1e308, 1e308, 100.0, t.get(), err, sizeof err) == OIP_OK && t[0] == 65535 && t[255] == 65535);
    // refusals; a short or missing message buffer is respected
    char small[8];
    CHECK(oip_denoise_thresholds(0.0, 0.0, 2.0, t.get(), small, sizeof small) == OIP_E_RUNTIME && strlen(small) == 7);
    CHECK(oip_denoise_thresholds(0.0, 0.0, 2.0, t.get(), nullptr, 0) == OIP_E_RUNTIME);
    CHECK(oip_denoise_thresholds(0.0, 0.0, 2.0, t.get(), err, sizeof err) == OIP_E_RUNTIME && strstr(err, "sigma 0") != nullptr);
    CHECK(oip_denoise_thresholds(-1.0, 0.0, 2.0, t.get(), err, sizeof err) == OIP_E_INVALID);
    CHECK(oip_denoise_thresholds(1.0, -1e-9, 2.0, t.get(), err, sizeof err) == OIP_E_INVALID);
    CHECK(oip_denoise_thresholds(NAN, 0.0, 2.0, t.get(), err, sizeof err) == OIP_E_INVALID);
    CHECK(oip_denoise_thresholds(1.0, INFINITY, 2.0, t.get(), err, sizeof err) == OIP_E_INVALID);
    CHECK(oip_denoise_thresholds(1.0, 0.0, 0.0, t.get(), err, sizeof err) == OIP_E_INVALID);
    CHECK(oip_denoise_thresholds(1.0, 0.0, -2.0, t.get(), err, sizeof err) == OIP_E_INVALID);
    CHECK(oip_denoise_thresholds(1.0, 0.0, NAN, t.get(), err, sizeof err) == OIP_E_INVALID);
    CHECK(oip_denoise_thresholds(1.0, 0.0, INFINITY, t.get(), err, sizeof err) == OIP_E_INVALID);
    CHECK(oip_denoise_thresholds(1.0, 0.0, 2.0, nullptr, err, sizeof err) == OIP_E_INVALID);
}

static void report_to_tables(const std::string &path)
{
    std::string text = "# oip noise image=x\n1,0,15,100,2.5,3.2\n";
    const double A[4] = {9.0, 4.0, 0.0, 25.0}, B[4] = {0.02, 0.0, 0.05, 0.001};
    for (int k = 0; k < 4; ++k) {
        char line[256];
        snprintf(line, sizeof line, "# band %d: blocks 10 nodata 0 structured 2 levels 3 a %.17g b %.17g mu_ref 1896 sigma_ref 5.2 snr_ref 364.6\n", k + 1, A[k], B[k]);
        text += line;
    }
    put(path, text);
    std::vector<NoiseModel> m;
    std::string err;
    CHECK(ParseNoiseReport(path, &m, &err) && m.size() == 4);
    std::vector<uint16_t> thr;
    CHECK(NoiseDenoiseTables(m, 4, 2.0, &thr, &err) && thr.size() == 4 * 256);
    for (int k = 0; k < 4 && thr.size() == 4 * 256; ++k) {
        uint16_t one[256];
        CHECK(oip_denoise_thresholds(A[k], B[k], 2.0, one, nullptr, 0) == OIP_OK);
        CHECK(memcmp(one, thr.data() + k * 256, sizeof one) == 0);
    }
    CHECK(thr.size() == 4 * 256 && thr[256] == 4 && thr[256 + 255] == 4 && thr[0] != thr[255]);
    // another K, another table
    std::vector<uint16_t> thr3;
    CHECK(NoiseDenoiseTables(m, 4, 3.0, &thr3, &err) && thr3 != thr);
    // the band-count mismatch either way: the message names both counts, the tables stay empty
    err.clear();
    CHECK(!NoiseDenoiseTables(m, 1, 2.0, &thr, &err) && thr.empty());
    CHECK(err.find("4 bands") != std::string::npos && err.find("1 sample per pixel") != std::string::npos);
    m.resize(1);
    err.clear();
    CHECK(!NoiseDenoiseTables(m, 4, 2.0, &thr, &err) && thr.empty());
    CHECK(err.find("1 band,") != std::string::npos && err.find("4 samples per pixel") != std::string::npos);
    CHECK(NoiseDenoiseTables(m, 1, 2.0, &thr, &err) && thr.size() == 256);
    m.clear();
    CHECK(!NoiseDenoiseTables(m, 1, 2.0, &thr, &err) && thr.empty());
    // a band without noise is refused by name; so is a K the entry point refuses
    m.assign(2, NoiseModel{1, 4.0, 0.0, 100.0});
    m[1] = NoiseModel{2, 0.0, 0.0, 100.0};
    m.resize(4, NoiseModel{3, 1.0, 0.0, 1.0});
    err.clear();
    CHECK(!NoiseDenoiseTables(m, 4, 2.0, &thr, &err) && thr.empty() && err.find("band 2") != std::string::npos && err.find("sigma 0") != std::string::npos);
    m[1].a = 1.0;
    CHECK(NoiseDenoiseTables(m, 4, 2.0, &thr, &err));
    CHECK(!NoiseDenoiseTables(m, 4, 0.0, &thr, &err) && thr.empty() && err.find("band 1") != std::string::npos);
    // a report that does not parse gives no models, hence no tables
    put(path, "# band 1: a 1 b nan mu_ref 3\n");
    CHECK(!ParseNoiseReport(path, &m, &err) && m.empty() && !NoiseDenoiseTables(m, 1, 2.0, &thr, &err));
}

int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: denoise_test SCRATCH_FILE\n"); return 2; }
    table_function();
    report_to_tables(argv[1]);
    remove(argv[1]);
    printf("%d checks, %d bad\n", checks, bad);
    return bad ? 1 : 0;
}
