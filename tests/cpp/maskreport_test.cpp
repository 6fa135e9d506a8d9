// Stand-alone check of the host side of `oip mask` under ASan + UBSan: the q8 form of a fraction, the report writer
// (csrc/oip_maskreport.hpp), read_tiff_u8 (csrc/oip_tiff.hpp) on what write_tiff_u8 writes -- one strip and several -- and on
// what it must refuse by name (a truncated file, 16-bit samples, three samples, a compressed file), and oip_mask_grid /
// oip_mask_tile_flag (csrc/host.cpp) on a grid of exactly the stated size.  argv[1]: a directory to write in.
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>

#include "oip_maskreport.hpp"
#include "oip_tiff.hpp"

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

static void put(const std::string &path, const std::string &bytes)
{
    std::ofstream f(path, std::ios::binary);
    f.write(bytes.data(), (std::streamsize)bytes.size());
}

// what read_tiff_u8 says of a file it must refuse ("" if it accepts it)
static std::string refusal(const std::string &path)
{
    int w = 0;
    long h = 0;
    std::vector<uint8_t> px;
    try {
        read_tiff_u8(path, &w, &h, &px);
    } catch (const std::exception &e) {
        return e.what();
    }
    return "";
}

static void q8()
{
    const double F[] = {0.30, 0.15, 0.08, 0.20, 0.0, 1.0, 0.5, 1.5 / 256, 2.5 / 256, 0.001};
    const int want[] = {77, 38, 20, 51, 0, 256, 128, 2, 2, 0};        // 1.5 and 2.5 are ties: to even
    for (size_t k = 0; k < sizeof F / sizeof F[0]; ++k) CHECK(MaskQ8(F[k]) == want[k]);
}

static void report(const std::string &dir)
{
    const uint64_t counts[8] = {6144, 3, 1, 6100, 750, 703, 287, 12345678901ull};
    const int band[4] = {2, 1, 0, 3}, q[4] = {77, 38, 20, 51};
    const std::string params = MaskParamsLine("a b.TIFF", 8, 768, 512, 10, 1023, 1, band, q, 1, 2);
    CHECK(params == "oip mask image=a b.TIFF cell=8 width=768 height=512 bits=10 saturation=1023 valid-min=1 bands=3,2,1,4 bright-q8=77 white-q8=38 "
                    "hot-q8=20 ndvi-q8=51 open=1 buffer=2");
    const std::string path = dir + "/report.csv";
    FILE *f = fopen(path.c_str(), "w");
    CHECK(f != nullptr);
    if (!f) return;
    CHECK(WriteMaskReport(f, params, counts));
    fclose(f);
    const std::string want = "# " + params + "\ncells,6144\nnodata_cells,3\nsaturated_cells,1\ntested_cells,6100\ncandidate_cells,750\ncloud_cells,703\n"
                             "buffer_cells,287\nsaturated_pixels,12345678901\nnodata_pct,0.0488\nsaturated_pct,0.0163\ncloud_pct,11.4421\n"
                             "cloud_or_buffer_pct,16.1133\n";
    CHECK(slurp(path) == want);
    CHECK(MaskSummaryLine(counts).find("cloud 703 (11.4421 %)") != std::string::npos);
    const uint64_t none[8] = {0, 0, 0, 0, 0, 0, 0, 0};                 // an empty grid divides nothing
    const MaskShares s = MaskPercent(none);
    CHECK(s.nodata == 0.0 && s.saturated == 0.0 && s.cloud == 0.0 && s.cloudOrBuffer == 0.0);
    f = fopen("/dev/full", "w");                                       // a device that takes nothing: the writer says so
    if (f) {
        setvbuf(f, nullptr, _IONBF, 0);
        CHECK(!WriteMaskReport(f, params, counts));
        fclose(f);
    }
}

static void tiff(const std::string &dir)
{
    // one strip; an odd size, so that the directory is moved to an even offset
    {
        const int w = 37;
        const long h = 21;
        std::vector<uint8_t> px((size_t)w * h);
        for (size_t i = 0; i < px.size(); ++i) px[i] = (uint8_t)(i * 7 + 3);
        const std::string path = dir + "/one.TIFF";
        write_tiff_u8(path, px.data(), w, h, 1);
        int gw = 0;
        long gh = 0;
        std::vector<uint8_t> got;
        read_tiff_u8(path, &gw, &gh, &got);
        CHECK(gw == w && gh == h && got == px);
        // truncated: inside the pixels, inside the directory, an empty file
        const std::string bytes = slurp(path);
        put(dir + "/cut1.TIFF", bytes.substr(0, 100));
        CHECK(refusal(dir + "/cut1.TIFF").find("truncated file") != std::string::npos);
        put(dir + "/cut2.TIFF", bytes.substr(0, bytes.size() - 20));
        CHECK(refusal(dir + "/cut2.TIFF").find("truncated file") != std::string::npos);
        put(dir + "/cut3.TIFF", "");
        CHECK(refusal(dir + "/cut3.TIFF").find("truncated file") != std::string::npos);
        // compressed: the Compression tag (259, SHORT) of the same file set to LZW
        std::string lzw = bytes;
        uint32_t ifd = 0;
        memcpy(&ifd, lzw.data() + 4, 4);
        bool patched = false;
        for (int k = 0; k < 10; ++k) {
            uint16_t id = 0;
            memcpy(&id, lzw.data() + ifd + 2 + 12 * k, 2);
            if (id == 259) { lzw[ifd + 2 + 12 * k + 8] = 5; patched = true; }
        }
        CHECK(patched);
        put(dir + "/lzw.TIFF", lzw);
        CHECK(refusal(dir + "/lzw.TIFF").find("compression 5 is not supported") != std::string::npos);
        put(dir + "/junk.TIFF", std::string(64, 'x'));
        CHECK(refusal(dir + "/junk.TIFF").find("only little-endian TIFF") != std::string::npos);
        CHECK(refusal(dir + "/missing.TIFF").find("cannot open file") != std::string::npos);
    }
    // several strips: write_tiff_u8 cuts at about 8 MiB
    {
        const int w = 3001;
        const long h = 3003;
        std::vector<uint8_t> px((size_t)w * h);
        uint32_t s = 12345;
        for (size_t i = 0; i < px.size(); ++i) { s = s * 1664525u + 1013904223u; px[i] = (uint8_t)(s >> 24); }
        const std::string path = dir + "/strips.TIFF";
        write_tiff_u8(path, px.data(), w, h, 1);
        int gw = 0;
        long gh = 0;
        std::vector<uint8_t> got;
        read_tiff_u8(path, &gw, &gh, &got);
        CHECK(gw == w && gh == h && got == px);
        const std::string bytes = slurp(path);
        put(dir + "/cut4.TIFF", bytes.substr(0, bytes.size() / 2));
        CHECK(refusal(dir + "/cut4.TIFF").find("truncated file") != std::string::npos);
    }
    // three samples: what `oip quicklook` writes in colour
    {
        std::vector<uint8_t> px(5 * 4 * 3, 9);
        write_tiff_u8(dir + "/rgb.TIFF", px.data(), 5, 4, 3);
        CHECK(refusal(dir + "/rgb.TIFF").find("3 samples per pixel are not supported") != std::string::npos);
    }
    // 16-bit samples: a product
    {
        std::vector<uint16_t> px(6 * 5, 1000);
        write_tiff_u16(dir + "/u16.TIFF", px.data(), 6, 5, 1, false);
        CHECK(refusal(dir + "/u16.TIFF").find("16-bit samples are not supported") != std::string::npos);
    }
}

static void grid()
{
    int gw = -1;
    long gh = -1;
    CHECK(oip_mask_grid(203, 77, 8, &gw, &gh) == OIP_OK && gw == 26 && gh == 10);
    CHECK(oip_mask_grid(0, 0, 4, &gw, &gh) == OIP_OK && gw == 0 && gh == 0);
    CHECK(oip_mask_grid(16, 16, 16, &gw, &gh) == OIP_OK && gw == 1 && gh == 1);
    CHECK(oip_mask_grid(16, 16, 5, &gw, &gh) == OIP_E_INVALID && oip_mask_grid(-1, 16, 8, &gw, &gh) == OIP_E_INVALID);
    CHECK(oip_mask_grid(16, 16, 8, nullptr, &gh) == OIP_E_INVALID);
    // a 3 x 2 grid of cells of 4 on the heap, exactly its size: one cell set, asked from every side
    std::unique_ptr<uint8_t[]> f(new uint8_t[6]());
    f[1 * 3 + 2] = OIP_MASK_BUFFER;                                    // cell (1, 2): pixels [8, 12) x [4, 8)
    CHECK(oip_mask_tile_flag(f.get(), 3, 3, 2, 4, 8, 4, 1, 1, 12) == 1);
    CHECK(oip_mask_tile_flag(f.get(), 3, 3, 2, 4, 7, 4, 1, 1, 12) == 0 && oip_mask_tile_flag(f.get(), 3, 3, 2, 4, 7, 4, 2, 1, 12) == 1);
    CHECK(oip_mask_tile_flag(f.get(), 3, 3, 2, 4, 8, 3, 4, 1, 12) == 0 && oip_mask_tile_flag(f.get(), 3, 3, 2, 4, 8, 3, 4, 2, 12) == 1);
    CHECK(oip_mask_tile_flag(f.get(), 3, 3, 2, 4, 0, 0, 8, 8, 12) == 0 && oip_mask_tile_flag(f.get(), 3, 3, 2, 4, 0, 0, 9, 8, 12) == 1);
    CHECK(oip_mask_tile_flag(f.get(), 3, 3, 2, 4, 11, 7, 100, 100, 12) == 1 && oip_mask_tile_flag(f.get(), 3, 3, 2, 4, 12, 7, 100, 100, 12) == 0);
    CHECK(oip_mask_tile_flag(f.get(), 3, 3, 2, 4, -50, -50, 200, 200, 8) == 1 && oip_mask_tile_flag(f.get(), 3, 3, 2, 4, -50, -50, 200, 200, 4) == 0);
    CHECK(oip_mask_tile_flag(f.get(), 3, 3, 2, 4, -50, -50, 50, 50, 12) == 0 && oip_mask_tile_flag(f.get(), 3, 3, 2, 4, 8, 4, 0, 5, 12) == 0);
}

int main(int argc, char **argv)
{
    if (argc < 2) { printf("usage: maskreport_test DIR\n"); return 2; }
    q8();
    report(argv[1]);
    tiff(argv[1]);
    grid();
    printf("%d checks, %d bad\n", checks, bad);
    return bad ? 1 : 0;
}
