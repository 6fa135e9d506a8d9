// tiffcodec_pin.cpp -- what the TIFF codec (csrc/oip_tiff.hpp, csrc/oip_tifftiled.hpp) says of a list of files and what its three
// writers put into a directory, for tests/test_tiffcodec_pin_cpu.py to compare with tests/golden/tiff_refusals.json and
// tests/golden/tiff_writer_digests.json.  Built with ASan + UBSan by that test.
//   tiffcodec_pin read LIST   LIST: lines `u16|u8 file`.  Prints, per line, the file's name, the checked layout or the refusal,
//                             and the pixels (size and FNV-1a) or the refusal; the file's own path is printed as @.
//   tiffcodec_pin write DIR   writes the grid of files into DIR (the test hashes them); OIP_TIFF_FORCE_BIG as the caller set it
#include "oip_tifftiled.hpp"

#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

using namespace OIPGPU;

static std::string without(std::string s, const std::string &path)
{
    for (size_t p; (p = s.find(path)) != std::string::npos;) s.replace(p, path.size(), "@");
    return s;
}

static unsigned long long fnv(const void *p, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char *)p)[i]) * 1099511628211ull;
    return h;
}

static int read_list(const char *list)
{
    std::ifstream in(list);
    std::string kind, path;
    while (in >> kind >> path) {
        const std::string name = path.substr(path.rfind('/') + 1);
        int w = 0, s = 0;
        long h = 0;
        if (kind == "u8") {
            std::vector<uint8_t> px;
            try {
                read_tiff_u8(path, &w, &h, &px);
                printf("%s\tu8\tpixels %d %ld %zu %016llx\n", name.c_str(), w, h, px.size(), fnv(px.data(), px.size()));
            } catch (const std::exception &e) { printf("%s\tu8\trefused: %s\n", name.c_str(), without(e.what(), path).c_str()); }
            continue;
        }
        try {
            const TiffLayout lay = read_tiff_layout(path);
            unsigned long long sum = 0;
            for (uint64_t l : lay.lens) sum += l;
            printf("%s\tlayout\t%llu x %llu x %llu compression %llu predictor %llu rows/strip %llu tile %llu x %llu, %zu chunks from %llu, %llu bytes\n",
                   name.c_str(), (unsigned long long)lay.width, (unsigned long long)lay.height, (unsigned long long)lay.spp,
                   (unsigned long long)lay.compression, (unsigned long long)lay.predictor, (unsigned long long)lay.rows_per_strip,
                   (unsigned long long)lay.tile_width, (unsigned long long)lay.tile_length, lay.offs.size(), (unsigned long long)lay.offs[0], sum);
        } catch (const std::exception &e) { printf("%s\tlayout\trefused: %s\n", name.c_str(), without(e.what(), path).c_str()); }
        std::vector<uint16_t> px;
        try {
            read_tiff_u16(path, &w, &h, &s, &px);
            printf("%s\tpixels\t%d %ld %d %zu %016llx\n", name.c_str(), w, h, s, px.size(), fnv(px.data(), px.size() * 2));
        } catch (const std::exception &e) { printf("%s\tpixels\trefused: %s\n", name.c_str(), without(e.what(), path).c_str()); }
    }
    return 0;
}

static std::vector<uint16_t> samples(size_t n, unsigned seed)
{
    std::vector<uint16_t> v(n);
    for (size_t i = 0; i < n; ++i) v[i] = (uint16_t)((((i + seed) * 2654435761u) >> 9) & (i % 7 ? 0x0fff : 0xffff));
    return v;
}

static void put_at(const std::string &path, uint64_t at, const void *p, size_t n)
{
    FILE *f = fopen(path.c_str(), "r+b");
    if (!f || fseeko(f, (off_t)at, SEEK_SET) != 0 || fwrite(p, 1, n, f) != n || fclose(f) != 0) throw std::runtime_error("io error on " + path);
}

// the rows of one directory in blocks of 1, 3, 5, 7, 1, .. rows
static void rows_in_odd_counts(TiffWriterU16 &tw, const uint16_t *img, long h, size_t rowSamples)
{
    long step = 1;
    for (long r = 0; r < h; step = step % 7 + 2) {
        const long n = std::min(step, h - r);
        tw.write_rows(img + (size_t)r * rowSamples, n);
        r += n;
    }
}

static int write_grid(const std::string &dir)
{
    const int comps[2] = {TIFF_NONE, TIFF_LZW};
    for (int spp : {1, 4})
        for (int comp : comps) {
            const std::string tag = "_s" + std::to_string(spp) + (comp == TIFF_LZW ? "_lzw" : "_none") + ".tiff";
            // strips through write_rows: 37 x 21 (one strip), 1201 x 61 (LZW: several strips and a short last one; 4 samples are
            // written in OpenCV's order), and uncompressed 2100 x 1001 x 4 (three strips of 8 MiB and less)
            for (int big = 0; big < 2; ++big) {
                const int w = big ? 1201 : 37;
                const long h = big ? 61 : 21;
                const auto img = samples((size_t)w * h * spp, 1);
                TiffWriterU16 tw(dir + "/rows_" + std::to_string(w) + tag, w, h, spp, big != 0, comp);
                rows_in_odd_counts(tw, img.data(), h, (size_t)w * spp);
                tw.close();
            }
            if (comp == TIFF_NONE && spp == 4) {
                const auto img = samples((size_t)2100 * 1001 * 4, 2);
                TiffWriterU16 tw(dir + "/rows_2100" + tag, 2100, 1001, 4, false, comp);
                rows_in_odd_counts(tw, img.data(), 1001, (size_t)2100 * 4);
                tw.close();
            }
            // the external interfaces: the payload (uncompressed), the strips (LZW; odd lengths, so that pad bytes occur)
            {
                const int w = 1201;
                const long h = 61;
                const size_t rw = (size_t)w * spp;
                const auto img = samples(rw * h, 3);
                const std::string path = dir + "/external" + tag;
                TiffWriterU16 tw(path, w, h, spp, false, comp);
                if (comp == TIFF_NONE) {
                    tw.preallocate();
                    const uint64_t at = tw.begin_external_payload();
                    put_at(path, at, img.data(), img.size() * 2);
                    tw.end_external_payload();
                } else {
                    const long rps = tw.rows_per_strip();
                    const size_t nstrips = (size_t)((h + rps - 1) / rps);
                    std::vector<uint64_t> off(nstrips), len(nstrips);
                    std::vector<uint8_t> payload;
                    for (size_t k = 0; k < nstrips; ++k) {
                        const long r0 = (long)k * rps, nr = std::min<long>(rps, h - r0);
                        std::vector<uint16_t> rows(img.begin() + (size_t)r0 * rw, img.begin() + (size_t)(r0 + nr) * rw);
                        for (long r = 0; r < nr; ++r) tiffdetail::predictor2_encode(rows.data() + (size_t)r * rw, (size_t)w, spp);
                        std::vector<uint8_t> enc(tiffdetail::lzw_worst((size_t)nr * rw * 2));
                        const size_t m = tiffdetail::lzw_encode_to((const uint8_t *)rows.data(), (size_t)nr * rw * 2, enc.data());
                        if (payload.size() & 1) payload.push_back(0);
                        off[k] = payload.size();
                        len[k] = m;
                        payload.insert(payload.end(), enc.begin(), enc.begin() + (long)m);
                    }
                    const uint64_t bytes = payload.size();
                    if (payload.size() & 1) payload.push_back(0);
                    put_at(path, tw.begin_external_strips(), payload.data(), payload.size());
                    tw.end_external_strips(off.data(), len.data(), nstrips, bytes);
                }
                tw.close();
            }
            // an overview file of three levels of a 1201 x 61 product: 601 x 31, 301 x 16, 151 x 8
            {
                TiffWriterU16 tw(dir + "/overviews" + tag, 1201, 61, spp, false, comp, 3);
                for (int k = 0; k < 3; ++k) {
                    const auto img = samples((size_t)tw.width() * tw.height() * spp, 10 + k);
                    rows_in_odd_counts(tw, img.data(), tw.height(), (size_t)tw.width() * spp);
                    if (k < 2) tw.next_directory();
                }
                tw.close();
            }
            // tiled, 37 x 21 in tiles of 16 with two reduced levels (19 x 11, 10 x 6): edge tiles, odd payload lengths
            {
                TiffTiledWriterU16 tw(dir + "/tiled" + tag, 37, 21, spp, 16, comp, 2);
                for (int k = 0; k <= 2; ++k) {
                    const auto tiles = samples((size_t)tw.tiles_x() * tw.tiles_y() * 16 * 16 * spp, 20 + k);
                    tw.write_tiles(tiles.data());
                    if (k < 2) tw.next_directory();
                }
                tw.close();
            }
        }
    // the 8-bit writer: one strip, and two (3000 x 3000 is more than 8 MiB)
    for (int spp : {1, 3}) {
        std::vector<uint8_t> px((size_t)37 * 21 * spp);
        for (size_t i = 0; i < px.size(); ++i) px[i] = (uint8_t)((i * 2654435761u) >> 13);
        write_tiff_u8(dir + "/u8_37_s" + std::to_string(spp) + ".tiff", px.data(), 37, 21, spp);
    }
    {
        std::vector<uint8_t> px((size_t)3000 * 3000);
        for (size_t i = 0; i < px.size(); ++i) px[i] = (uint8_t)((i * 2654435761u) >> 13);
        write_tiff_u8(dir + "/u8_3000_s1.tiff", px.data(), 3000, 3000, 1);
    }
    return 0;
}

int main(int argc, char **argv)
{
    try {
        if (argc == 3 && std::string(argv[1]) == "read") return read_list(argv[2]);
        if (argc == 3 && std::string(argv[1]) == "write") return write_grid(argv[2]);
    } catch (const std::exception &e) {
        printf("failed: %s\n", e.what());
        return 1;
    }
    printf("usage: tiffcodec_pin read LIST | write DIR\n");
    return 2;
}
