// tiff_pyramid_test.cpp -- TiffWriterU16 as the writer of an overview file (overview_levels > 0: chained reduced-resolution
// directories, csrc/oip_tiff.hpp) on host arrays, and of a one-image file through the untouched path.  The levels come from
// the test (tests/test_overview_cpu.py writes them as raw files and reads the TIFFs back with a parser of its own); every
// pyramid is written three ways -- write_rows(), and the two external interfaces the device paths use (payload / strips) --
// which must give the same file.  Built with ASan + UBSan by the test.  usage: tiff_pyramid_test DIR
//   DIR/manifest.txt: one case per line, `name width height spp compression levels` (width x height: the image, level 0)
//   DIR/<name>.L<k>.raw: level k = 0 .. levels;  written: DIR/<name>.ovr, DIR/<name>.ext.ovr, DIR/<name>.one.tiff (level 0)
#include "oip_tiff.hpp"

#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

using namespace OIPGPU;

static std::vector<uint8_t> slurp(const std::string &p)
{
    std::vector<uint8_t> v;
    if (FILE *f = fopen(p.c_str(), "rb")) {
        fseeko(f, 0, SEEK_END);
        v.resize((size_t)ftello(f));
        rewind(f);
        if (fread(v.data(), 1, v.size(), f) != v.size()) v.clear();
        fclose(f);
    }
    return v;
}

static bool write_at(const std::string &path, uint64_t at, const void *p, size_t n)
{
    FILE *f = fopen(path.c_str(), "r+b");
    const bool ok = f && fseeko(f, (off_t)at, SEEK_SET) == 0 && fwrite(p, 1, n, f) == n;
    if (f) fclose(f);
    return ok;
}

// the current directory's pixels through the interface a device path uses for them
static bool external_level(TiffWriterU16 &tw, const std::string &path, const std::vector<uint16_t> &img, int spp, int comp)
{
    const int w = tw.width();
    const long h = tw.height();
    if (comp == TIFF_NONE) {
        const uint64_t at = tw.begin_external_payload();
        if (!write_at(path, at, img.data(), img.size() * 2)) return false;
        tw.end_external_payload();
        return true;
    }
    const long rps = tw.rows_per_strip();
    const size_t rw = (size_t)w * spp, nstrips = (size_t)((h + rps - 1) / rps);
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
    const uint64_t at = tw.begin_external_strips();
    if (!write_at(path, at, payload.data(), payload.size())) return false;
    tw.end_external_strips(off.data(), len.data(), nstrips, bytes);
    return true;
}

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    std::ifstream man(dir + "/manifest.txt");
    std::string name;
    int w = 0, spp = 0, comp = 0, levels = 0, n = 0, bad = 0;
    long h = 0;
    while (man >> name >> w >> h >> spp >> comp >> levels) {
        ++n;
        std::vector<std::vector<uint16_t>> lv;
        int lw = w;
        long lh = h;
        for (int k = 0; k <= levels; ++k) {
            const auto raw = slurp(dir + "/" + name + ".L" + std::to_string(k) + ".raw");
            if (raw.size() != (size_t)lw * lh * spp * 2) { printf("%s: level %d has %zu bytes\n", name.c_str(), k, raw.size()); return 2; }
            lv.emplace_back((const uint16_t *)raw.data(), (const uint16_t *)raw.data() + raw.size() / 2);
            lw = (lw + 1) / 2;
            lh = (lh + 1) / 2;
        }
        const std::string a = dir + "/" + name + ".ovr", b = dir + "/" + name + ".ext.ovr";
        {
            TiffWriterU16 tw(a, w, h, spp, false, comp, levels);
            for (int k = 1; k <= levels; ++k) {
                if (tw.levels_left() != levels - k + 1 || (size_t)tw.width() * tw.height() * spp != lv[k].size()) { ++bad; printf("%s: level %d geometry\n", name.c_str(), k); break; }
                // (in two calls: a strip left incomplete by the first is kept)
                const long first = tw.height() / 3;
                tw.write_rows(lv[k].data(), first);
                tw.write_rows(lv[k].data() + (size_t)first * tw.width() * spp, tw.height() - first);
                if (k < levels) tw.next_directory();
            }
            tw.close();
        }
        {
            TiffWriterU16 tw(b, w, h, spp, false, comp, levels);
            for (int k = 1; k <= levels; ++k) {
                if (!external_level(tw, b, lv[k], spp, comp)) { printf("io error\n"); return 2; }
                if (k < levels) tw.next_directory();
            }
            tw.close();
        }
        if (slurp(a).size() < 100 || slurp(a) != slurp(b)) { ++bad; printf("%s: the external interfaces write another file\n", name.c_str()); }
        write_tiff_u16(dir + "/" + name + ".one.tiff", lv[0].data(), w, h, spp, false, comp);
    }
    // misuse is refused
    try { TiffWriterU16 tw(dir + "/m.tiff", 8, 2, 1, false, TIFF_NONE); tw.next_directory(); ++bad; printf("a one-image writer went on to a second directory\n"); }
    catch (const std::logic_error &) {}
    try {
        TiffWriterU16 tw(dir + "/m.tiff", 8, 4, 1, false, TIFF_NONE, 2);
        const uint16_t px[8] = {0};
        tw.write_rows(px, 2);
        tw.close();
        ++bad; printf("an overview file closed with a level missing\n");
    } catch (const std::logic_error &) {}
    try { TiffWriterU16 tw(dir + "/m.tiff", 8, 4, 1, false, TIFF_NONE, 2); tw.next_directory(); ++bad; printf("a directory without its rows was accepted\n"); }
    catch (const std::logic_error &) {}
    printf("%d cases, %d bad\n", n, bad);
    return bad ? 1 : 0;
}
