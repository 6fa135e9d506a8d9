// Stand-alone check of the report of `oip noise` (csrc/oip_noisereport.hpp) under ASan + UBSan: a report written by
// WriteNoiseReport parses back with a, b and mu_ref bit for bit; the parser is fed truncated, overlong, non-numeric, misordered
// and band-less reports and refuses each with a message; and the three host entry points behind the report (csrc/host.cpp)
// run on tables of exactly the stated sizes.  The values themselves are compared with the Python restatement in
// tests/test_noise_cpu.py.
#include <cmath>
#include <cstring>
#include <memory>

#include "oip_noisereport.hpp"

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

// a band whose numbers need all 17 digits
static NoiseBand band(int seed)
{
    NoiseBand n;
    n.nodata = 7 + seed;
    n.structured = 1000 * seed;
    for (int l = 3 + seed; l < 200; l += 7) {
        n.blocks[l] = 100 + (uint64_t)l * seed;
        n.sigma[l] = 0.125 + std::sqrt((double)l + 1.0 / (3.0 + seed));
        ++n.levels;
    }
    n.a = 4.0 + 1.0 / (3.0 + seed);
    n.b = 0.01 / (7.0 + seed);
    n.muRef = 16.0 * (100.5 + seed);
    return n;
}

static void round_trip(const std::string &path)
{
    for (int nb : {1, 4}) {
        std::vector<NoiseBand> bands;
        for (int k = 0; k < nb; ++k) bands.push_back(band(k));
        bands[0].a = 0.0;                                              // the clamps' values
        if (nb > 1) bands[1].b = 0.0;
        FILE *f = fopen(path.c_str(), "w");
        CHECK(f != nullptr);
        if (!f) return;
        CHECK(WriteNoiseReport(f, "oip noise image=x block=8 bits=12 columns=band,level_lo,level_hi,blocks,sigma,snr", bands, 4));
        CHECK(fclose(f) == 0);
        std::vector<NoiseModel> models;
        std::string err;
        CHECK(ParseNoiseReport(path, &models, &err));
        CHECK((int)models.size() == nb);
        for (int k = 0; k < (int)models.size() && k < nb; ++k) {
            CHECK(models[k].band == k + 1);
            CHECK(same_bits(models[k].a, bands[k].a) && same_bits(models[k].b, bands[k].b) && same_bits(models[k].muRef, bands[k].muRef));
        }
        // the rows: one per usable level and band, level bounds of the shift
        f = fopen(path.c_str(), "r");
        CHECK(f != nullptr);
        if (!f) return;
        char line[4098];
        int rows = 0, want = 0;
        for (const NoiseBand &n : bands) want += n.levels;
        while (fgets(line, sizeof line, f)) {
            if (line[0] == '#') continue;
            int b = 0, lo = 0, hi = 0;
            unsigned long long cnt = 0;
            double s = 0, snr = 0;
            CHECK(sscanf(line, "%d,%d,%d,%llu,%lf,%lf", &b, &lo, &hi, &cnt, &s, &snr) == 6);
            CHECK(b >= 1 && b <= nb && lo % 16 == 0 && hi == lo + 15 && cnt == bands[b - 1].blocks[lo / 16]);
            CHECK(std::fabs(s - bands[b - 1].sigma[lo / 16]) <= 5e-7 && std::fabs(snr - (lo + 8.0) / bands[b - 1].sigma[lo / 16]) <= 5e-5);
            ++rows;
        }
        fclose(f);
        CHECK(rows == want);
        int ta = 0, q8 = 0;
        CHECK(NoiseDespikeThreshold(models, 5.0, &ta, &q8, &err) && ta >= 1 && ta <= 65535 && q8 >= 0 && q8 <= 256);
    }
}

static void hostile(const std::string &path)
{
    const std::string good = "# band 1: blocks 10 nodata 0 structured 2 levels 3 a 4.25 b 0.0125 mu_ref 1896 sigma_ref 5.2 snr_ref 364.6\n";
    std::vector<NoiseModel> m;
    std::string err;
    put(path, "# oip noise image=x\n1,0,15,100,2.5,3.2\n" + good);
    CHECK(ParseNoiseReport(path, &m, &err) && m.size() == 1 && m[0].a == 4.25 && m[0].b == 0.0125 && m[0].muRef == 1896.0);
    // every truncation of a good report either parses to the same model or is refused with a message; none reads past its end
    for (size_t cut = 0; cut < good.size(); ++cut) {
        put(path, good.substr(0, cut));
        err.clear();
        const bool ok = ParseNoiseReport(path, &m, &err);
        CHECK(ok ? (m.size() == 1 && m[0].a == 4.25 && m[0].b == 0.0125 && m[0].muRef <= 1896.0) : (m.empty() && !err.empty()));
        if (cut < good.find(" mu_ref ") + 9) CHECK(!ok);
    }
    const char *refused[] = {
        "",                                                             // empty
        "# oip noise image=x\n1,0,15,100,2.5,3.2\n",                    // no band
        "# band x: a 1 b 2 mu_ref 3\n",                                 // no index
        "# band 2: a 1 b 2 mu_ref 3\n",                                 // out of order
        "# band 1 a 1 b 2 mu_ref 3\n",                                  // no colon
        "# band 1: a one b 2 mu_ref 3\n",                               // not numeric
        "# band 1: a 1 b 2x mu_ref 3\n",                                // trailing junk
        "# band 1: a 1 b nan mu_ref 3\n",                               // not finite
        "# band 1: a 1 b 2 mu_ref inf\n",
        "# band 1: a -1 b 2 mu_ref 3\n",                                // negative
        "# band 1: a 1 b 2\n",                                          // a field missing
        "# band 1: a 1 b 2 mu_ref\n",                                   // the value missing
        "# band 1: a 1 b 2 mu_ref 3\n# band 1: a 1 b 2 mu_ref 3\n",     // a band twice
        "# band 1: a 1 b 2 mu_ref 3\n# band 2: a 1 b 2 mu_ref 3\n# band 3: a 1 b 2 mu_ref 3\n# band 4: a 1 b 2 mu_ref 3\n# band 5: a 1 b 2 mu_ref 3\n",
        "# band 99999999999999999999: a 1 b 2 mu_ref 3\n",              // an index that overflows
    };
    for (const char *text : refused) {
        put(path, text);
        err.clear();
        CHECK(!ParseNoiseReport(path, &m, &err) && m.empty() && !err.empty());
    }
    // overlong lines: 4096 bytes and a line end pass as a line, one more byte is refused; a huge number is not finite
    for (size_t len : {4096u, 4097u, 5000u, 20000u}) {
        std::string line = "# band 1: a 1 b 2 mu_ref 3 ";
        line.resize(len, 'x');
        put(path, line + "\n");
        CHECK(ParseNoiseReport(path, &m, &err) == (len <= 4096));
        put(path, std::string(len, '7') + "\n" + good);
        CHECK(ParseNoiseReport(path, &m, &err) == (len <= 4096));
    }
    put(path, "# band 1: a 1 b 2 mu_ref 1" + std::string(400, '0') + "\n");
    CHECK(!ParseNoiseReport(path, &m, &err));
    put(path, good.substr(0, good.size() - 1));                       // no line end at the end of the file
    CHECK(ParseNoiseReport(path, &m, &err) && m.size() == 1);
    std::string bin = good;
    bin[20] = '\0';                                                    // a NUL inside a band line ends it: the fields are missing
    put(path, bin);
    CHECK(!ParseNoiseReport(path, &m, &err));
    CHECK(!ParseNoiseReport(path + ".missing", &m, &err) && !err.empty());
    // a model the threshold refuses
    m.assign(1, NoiseModel{1, 0.0, 0.0, 100.0});
    int ta = 0, q8 = 0;
    CHECK(!NoiseDespikeThreshold(m, 5.0, &ta, &q8, &err) && err.find("band 1") != std::string::npos);
    m.clear();
    CHECK(!NoiseDespikeThreshold(m, 5.0, &ta, &q8, &err));
}

// the host entry points on buffers of exactly the stated sizes
static void host_entry_points()
{
    std::unique_ptr<uint64_t[]> hist(new uint64_t[65536]), blocks(new uint64_t[256]);
    std::unique_ptr<double[]> sigma(new double[256]);
    for (int i = 0; i < 65536; ++i) hist[i] = 0;
    int usable = -1;
    CHECK(oip_noise_levels(hist.get(), 0, sigma.get(), blocks.get(), &usable) == OIP_OK && usable == 0);
    double a = -1, b = -1, mu = -1;
    char err[64] = "";
    CHECK(oip_noise_fit(sigma.get(), blocks.get(), 4, &a, &b, &mu, err, sizeof err) == OIP_E_RUNTIME && err[0] != '\0');
    CHECK(oip_noise_fit(sigma.get(), blocks.get(), 9, &a, &b, &mu, err, sizeof err) == OIP_E_INVALID);
    CHECK(oip_noise_fit(sigma.get(), blocks.get(), 4, &a, &b, &mu, nullptr, 0) == OIP_E_RUNTIME);
    // every level at both ends of the q range, the sentinels' bin full
    for (int l = 0; l < 256; ++l) { hist[l * 256] = 5; hist[l * 256 + 253] = 9; hist[l * 256 + 254] = 1; hist[l * 256 + 255] = 1000000; }
    CHECK(oip_noise_levels(hist.get(), 10, sigma.get(), blocks.get(), &usable) == OIP_OK && usable == 256);
    for (int l = 0; l < 256; ++l) CHECK(blocks[l] == 15 && sigma[l] == 0.25 * 253.5);
    CHECK(oip_noise_levels(hist.get(), 16, sigma.get(), blocks.get(), nullptr) == OIP_OK && sigma[0] == -1.0 && sigma[255] == -1.0);
    CHECK(oip_noise_levels(hist.get(), 10, sigma.get(), blocks.get(), &usable) == OIP_OK);
    for (int shift = 0; shift <= 8; ++shift) {
        CHECK(oip_noise_fit(sigma.get(), blocks.get(), shift, &a, &b, &mu, err, sizeof err) == OIP_OK);
        CHECK(b >= 0.0 && b < 1e-12 && a >= 0.0 && std::fabs(a - 63.375 * 63.375) < 1e-6 && mu == 127.5 * (1 << shift));
    }
    int ta = 0, q8 = 0;
    char small[8];
    CHECK(oip_noise_despike_threshold(0.0, 0.0, 10.0, 5.0, &ta, &q8, small, sizeof small) == OIP_E_RUNTIME && strlen(small) == 7);
    CHECK(oip_noise_despike_threshold(1.0, 1e9, 0.0, 5.0, &ta, &q8, err, sizeof err) == OIP_E_RUNTIME);
    CHECK(oip_noise_despike_threshold(1e12, 0.0, 0.0, 5.0, &ta, &q8, err, sizeof err) == OIP_E_RUNTIME);
    CHECK(oip_noise_despike_threshold(-1.0, 0.0, 0.0, 5.0, &ta, &q8, err, sizeof err) == OIP_E_INVALID);
    CHECK(oip_noise_despike_threshold(1.0, 0.0, 0.0, NAN, &ta, &q8, err, sizeof err) == OIP_E_INVALID);
    CHECK(oip_noise_despike_threshold(4.0, 0.0, 500.0, 5.0, &ta, &q8, err, sizeof err) == OIP_OK && ta == 11 && q8 == 0);
}

int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: noisereport_test SCRATCH_FILE\n"); return 2; }
    round_trip(argv[1]);
    hostile(argv[1]);
    host_entry_points();
    remove(argv[1]);
    printf("%d checks, %d bad\n", checks, bad);
    return bad ? 1 : 0;
}
