// tifftiled_test.cpp -- TiffTiledWriterU16 (csrc/oip_tifftiled.hpp) and the tiled branch of read_tiff_u16 (csrc/oip_tiff.hpp) on
// host arrays.  Built with ASan + UBSan by tests/test_cog_cpu.py.  usage: tifftiled_test DIR
//   round trips: write_tiles() -> read_tiff_u16 at spp 1 and 4, none and LZW, w, h in {1, 15, 16, 17, 255, 256, 257}, T in {16,
//   256}, 0, 1 and 3 levels (classic or BigTIFF by OIP_TIFF_FORCE_BIG, which the test sets); every directory of every file lies
//   below the first payload offset and every tile at or above it; a file written through begin_tiles() / end_tiles() is the same
//   file; the refusals of the reader from hand-built headers; a strip file still reads.
//   A few files are kept for the test's own reader: DIR/<name>.tiff with DIR/<name>.L0.raw (the image) and DIR/kept.txt, one
//   `name w h spp compression T levels` per line.  The levels are 2 x 2 means that skip samples below 1 (oip_halve_u16).
#include "oip_tifftiled.hpp"

#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

using namespace OIPGPU;

static int bad = 0;
#define CHECK(c, ...) do { if (!(c)) { ++bad; printf(__VA_ARGS__); printf("\n"); } } while (0)

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
static void spit(const std::string &p, const void *d, size_t n)
{
    FILE *f = fopen(p.c_str(), "wb");
    if (!f || fwrite(d, 1, n, f) != n) { printf("cannot write %s\n", p.c_str()); exit(2); }
    fclose(f);
}

// the tile-major form of a w x h x spp image (include/oip_c.h: oip_retile_u16): what write_tiles() takes
static std::vector<uint16_t> retile_host(const uint16_t *img, int w, long h, int spp, int T)
{
    const long tx = ((long)w + T - 1) / T, ty = (h + T - 1) / T;
    std::vector<uint16_t> out((size_t)tx * ty * T * T * spp);
    uint16_t *o = out.data();
    for (long j = 0; j < ty; ++j)
        for (long i = 0; i < tx; ++i)
            for (int r = 0; r < T; ++r) {
                const uint16_t *line = img + (size_t)std::min<long>(j * T + r, h - 1) * w * spp;
                for (int c = 0; c < T; ++c) {
                    const uint16_t *px = line + (size_t)std::min<long>(i * T + c, w - 1) * spp;
                    for (int ch = 0; ch < spp; ++ch) *o++ = px[ch];
                }
            }
    return out;
}

// 12-bit noise with zeros and 65535 in it
static std::vector<uint16_t> noise(int w, long h, int spp, uint32_t seed)
{
    std::vector<uint16_t> v((size_t)w * h * spp);
    uint32_t s = seed * 2654435761u + 12345u;
    for (auto &x : v) {
        s = s * 1664525u + 1013904223u;
        const uint32_t r = s >> 8;
        x = (r & 15) < 4 ? 0 : ((r & 255) == 255 ? 65535 : (uint16_t)(1 + (r >> 8) % 4095));
    }
    return v;
}

// include/oip_c.h: oip_halve_u16 with valid_min 1
static std::vector<uint16_t> halve(const std::vector<uint16_t> &a, int w, long h, int spp)
{
    const int W = (w + 1) / 2;
    const long H = (h + 1) / 2;
    std::vector<uint16_t> o((size_t)W * H * spp);
    for (long y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            for (int c = 0; c < spp; ++c) {
                unsigned S = 0, n = 0;
                for (int j = 0; j < 2; ++j)
                    for (int i = 0; i < 2; ++i) {
                        if (2 * y + j >= h || 2 * x + i >= w) continue;
                        const unsigned v = a[((size_t)(2 * y + j) * w + (2 * x + i)) * spp + c];
                        if (v >= 1) { S += v; ++n; }
                    }
                o[((size_t)y * W + x) * spp + c] = (uint16_t)(n ? (S + n / 2) / n : 0);
            }
    return o;
}

static uint64_t rdv(const std::vector<uint8_t> &f, uint64_t at, int n)
{
    uint64_t v = 0;
    if (at + n > f.size()) return ~(uint64_t)0;
    for (int i = 0; i < n; ++i) v |= (uint64_t)f[at + i] << (8 * i);
    return v;
}

// every directory below `head`, every tile at or above it; returns the number of directories (-1: broken)
static int check_chain(const std::vector<uint8_t> &f, uint64_t head)
{
    const bool big = rdv(f, 2, 2) == 43;
    uint64_t ifd = big ? rdv(f, 8, 8) : rdv(f, 4, 4);
    int n = 0;
    while (ifd) {
        if (ifd >= head || ++n > 64) return -1;
        const uint64_t cnt = big ? rdv(f, ifd, 8) : rdv(f, ifd, 2);
        if (cnt > 64) return -1;
        const uint64_t ent = ifd + (big ? 8 : 2), esz = big ? 20 : 12, osz = big ? 8 : 4;
        for (uint64_t i = 0; i < cnt; ++i) {
            const uint64_t e = ent + i * esz, id = rdv(f, e, 2), type = rdv(f, e + 2, 2), c = rdv(f, e + 4, (int)osz);
            const uint64_t ts = type == 3 ? 2 : type == 4 ? 4 : 8;
            const bool outl = c * ts > osz;
            const uint64_t at = outl ? rdv(f, e + 4 + osz, (int)osz) : e + 4 + osz;
            if (outl && at + c * ts > head) return -1;                     // the tables lie in the head too
            if (id == 324)
                for (uint64_t k = 0; k < c; ++k)
                    if (rdv(f, at + k * ts, (int)ts) < head) return -1;
        }
        ifd = rdv(f, ent + cnt * esz, (int)osz);
    }
    return n;
}

static void round_trip(const std::string &dir, std::ofstream &kept, int w, long h, int spp, int comp, int T, int levels, int *files)
{
    char name[128];
    snprintf(name, sizeof name, "w%d_h%ld_s%d_c%d_t%d_l%d", w, h, spp, comp, T, levels);
    const bool keep = (T == 16 && (w == 17 || w == 257) && (h == 15 || h == 255)) || (T == 256 && w == 17 && h == 17) ||
                      (T == 256 && comp == TIFF_NONE && w == 257 && h == 257);
    const std::string path = dir + "/" + (keep ? std::string(name) : std::string("scratch")) + ".tiff";
    std::vector<std::vector<uint16_t>> lv;
    lv.push_back(noise(w, h, spp, (uint32_t)(w * 7 + h * 3 + spp + comp + T + levels)));
    int lw = w;
    long lh = h;
    for (int k = 0; k < levels; ++k) { lv.push_back(halve(lv.back(), lw, lh, spp)); lw = (lw + 1) / 2; lh = (lh + 1) / 2; }
    uint64_t head = 0;
    {
        TiffTiledWriterU16 tw(path, w, h, spp, T, comp, levels);
        head = tw.first_payload_offset();
        for (int k = 0; k <= levels; ++k) {
            CHECK(tw.level() == k && (size_t)tw.width() * tw.height() * spp == lv[k].size(), "%s: level %d geometry", name, k);
            const auto tm = retile_host(lv[k].data(), tw.width(), tw.height(), spp, T);
            CHECK(tm.size() == (size_t)tw.tiles_x() * tw.tiles_y() * T * T * spp, "%s: tile-major size", name);
            tw.write_tiles(tm.data());
            if (k < levels) tw.next_directory();
        }
        tw.close();
    }
    ++*files;
    const auto bytes = slurp(path);
    CHECK(check_chain(bytes, head) == levels + 1, "%s: a directory or table beyond the head, or a tile inside it", name);
    int rw = 0, rs = 0;
    long rh = 0;
    std::vector<uint16_t> back;
    try {
        read_tiff_u16(path, &rw, &rh, &rs, &back);
        CHECK(rw == w && rh == h && rs == spp && back == lv[0], "%s: reads back differently", name);
        const TiffLayout lay = read_tiff_layout(path);
        CHECK(lay.tiled() && lay.tile_width == (uint64_t)T && lay.tile_length == (uint64_t)T && lay.rows_per_strip == 0 &&
                  lay.offs.size() == (size_t)(((w + T - 1) / T) * ((h + T - 1) / T)), "%s: layout", name);
    } catch (const std::exception &e) { CHECK(false, "%s: %s", name, e.what()); }
    if (keep) {
        spit(dir + "/" + name + ".L0.raw", lv[0].data(), lv[0].size() * 2);
        kept << name << " " << w << " " << h << " " << spp << " " << comp << " " << T << " " << levels << "\n";
    }
}

// the interface the device path uses gives the file write_tiles() gives
static void external_equals_host(const std::string &dir)
{
    const int w = 40, spp = 4, T = 16, levels = 1;
    const long h = 21;
    for (int comp : {(int)TIFF_NONE, (int)TIFF_LZW}) {
        std::vector<std::vector<uint16_t>> lv{noise(w, h, spp, 99)};
        lv.push_back(halve(lv[0], w, h, spp));
        const std::string a = dir + "/ext_a.tiff", b = dir + "/ext_b.tiff";
        {
            TiffTiledWriterU16 tw(a, w, h, spp, T, comp, levels);
            for (int k = 0; k <= levels; ++k) { tw.write_tiles(retile_host(lv[k].data(), tw.width(), tw.height(), spp, T).data()); if (k < levels) tw.next_directory(); }
            tw.close();
        }
        {
            TiffTiledWriterU16 tw(b, w, h, spp, T, comp, levels);
            for (int k = 0; k <= levels; ++k) {
                const auto tm = retile_host(lv[k].data(), tw.width(), tw.height(), spp, T);
                const size_t n = (size_t)tw.tiles_x() * tw.tiles_y(), ts = (size_t)T * T * spp;
                std::vector<uint64_t> off(n), len(n);
                std::vector<uint8_t> payload;
                for (size_t t = 0; t < n; ++t) {
                    std::vector<uint16_t> tile(tm.begin() + t * ts, tm.begin() + (t + 1) * ts);
                    if (payload.size() & 1) payload.push_back(0);
                    off[t] = payload.size();
                    if (comp == TIFF_NONE) {
                        payload.insert(payload.end(), (uint8_t *)tile.data(), (uint8_t *)tile.data() + ts * 2);
                    } else {
                        for (int r = 0; r < T; ++r) tiffdetail::predictor2_encode(tile.data() + (size_t)r * T * spp, (size_t)T, spp);
                        std::vector<uint8_t> enc(tiffdetail::lzw_worst(ts * 2));
                        enc.resize(tiffdetail::lzw_encode_to((const uint8_t *)tile.data(), ts * 2, enc.data()));
                        payload.insert(payload.end(), enc.begin(), enc.end());
                    }
                    len[t] = payload.size() - off[t];
                }
                const uint64_t at = tw.begin_tiles();
                FILE *f = fopen(b.c_str(), "r+b");
                if (!f || fseeko(f, (off_t)at, SEEK_SET) != 0 || fwrite(payload.data(), 1, payload.size(), f) != payload.size()) { printf("io error\n"); exit(2); }
                fclose(f);
                tw.end_tiles(off.data(), len.data(), n, payload.size());
                if (k < levels) tw.next_directory();
            }
            tw.close();
        }
        CHECK(slurp(a).size() > 100 && slurp(a) == slurp(b), "compression %d: begin_tiles / end_tiles write another file", comp);
    }
    // misuse is refused
    try { TiffTiledWriterU16 tw(dir + "/m.tiff", 8, 8, 1, 16, TIFF_NONE, 1); tw.next_directory(); CHECK(false, "a directory without its tiles was accepted"); }
    catch (const std::logic_error &) {}
    try {
        TiffTiledWriterU16 tw(dir + "/m.tiff", 8, 8, 1, 16, TIFF_NONE, 1);
        tw.write_tiles(std::vector<uint16_t>(256, 7).data());
        tw.close();
        CHECK(false, "a file closed with a level missing");
    } catch (const std::logic_error &) {}
    for (int T : {0, 8, 24, 1040})
        try { TiffTiledWriterU16 tw(dir + "/m.tiff", 8, 8, 1, T, TIFF_NONE, 0); CHECK(false, "tile size %d was accepted", T); }
        catch (const std::invalid_argument &) {}
}

// ---- hand-built classic headers ---------------------------------------------------------------------------------------------
struct HTag { uint16_t id, type; uint32_t count, value; };
// header, `payload` from offset 8, then an out-of-line array of LONGs per entry of `arrays` (tag index -> values), the directory last
static void build(const std::string &path, std::vector<HTag> tags, const std::vector<uint8_t> &payload,
                  const std::vector<std::pair<int, std::vector<uint32_t>>> &arrays)
{
    std::vector<uint8_t> f{'I', 'I', 42, 0, 0, 0, 0, 0};
    auto put = [&](uint64_t v, int n) { for (int i = 0; i < n; ++i) f.push_back((uint8_t)(v >> (8 * i))); };
    f.insert(f.end(), payload.begin(), payload.end());
    if (f.size() & 1) f.push_back(0);
    for (auto &a : arrays) {
        tags[(size_t)a.first].value = (uint32_t)f.size();
        tags[(size_t)a.first].count = (uint32_t)a.second.size();
        for (uint32_t v : a.second) put(v, 4);
    }
    const uint32_t ifd = (uint32_t)f.size();
    for (int i = 0; i < 4; ++i) f[4 + i] = (uint8_t)(ifd >> (8 * i));
    put(tags.size(), 2);
    for (auto &t : tags) { put(t.id, 2); put(t.type, 2); put(t.count, 4); put(t.value, 4); }
    put(0, 4);
    spit(path, f.data(), f.size());
}

static void expect(const std::string &path, const char *what, const char *text)
{
    int w = 0, s = 0;
    long h = 0;
    std::vector<uint16_t> out;
    try {
        read_tiff_u16(path, &w, &h, &s, &out);
        CHECK(text == nullptr, "%s: accepted", what);
    } catch (const std::exception &e) {
        CHECK(text && std::string(e.what()).find(text) != std::string::npos, "%s: %s", what, e.what());
    }
}

static void refusals(const std::string &dir)
{
    // 20 x 20, one sample, 16 x 16 tiles: four uncompressed tiles of 512 bytes behind the header
    const std::vector<uint8_t> payload(4 * 512, 3);
    const std::vector<uint32_t> offs{8, 520, 1032, 1544}, lens{512, 512, 512, 512};
    const std::vector<HTag> base{{256, 4, 1, 20}, {257, 4, 1, 20}, {258, 3, 1, 16}, {259, 3, 1, 1}, {262, 3, 1, 1}, {277, 3, 1, 1}, {284, 3, 1, 1},
                                 {322, 4, 1, 16}, {323, 4, 1, 16}, {324, 4, 4, 0}, {325, 4, 4, 0}, {339, 3, 1, 1}};
    const std::string p = dir + "/hand.tiff";
    build(p, base, payload, {{9, offs}, {10, lens}});
    expect(p, "the well-formed file", nullptr);
    for (int drop : {7, 8}) {
        auto t = base;
        t.erase(t.begin() + drop);
        build(p, t, payload, {{8, offs}, {9, lens}});
        expect(p, "one tile tag of the pair", "TileWidth and TileLength");
    }
    { auto t = base; t[7].value = 0; build(p, t, payload, {{9, offs}, {10, lens}}); expect(p, "a TileWidth of 0", "TileWidth and TileLength"); }
    build(p, base, payload, {{9, {8, 520, 1032}}, {10, {512, 512, 512}}});
    expect(p, "three tiles for a 2 x 2 grid", "tile count");
    {
        auto t = base;
        t.insert(t.begin() + 5, HTag{273, 4, 1, 8});
        t.insert(t.begin() + 7, HTag{279, 4, 1, 512});
        build(p, t, payload, {{11, offs}, {12, lens}});
        expect(p, "strips and tiles", "both present");
    }
    build(p, base, payload, {{9, {8, 520, 1032, 1000000}}, {10, lens}});
    expect(p, "a tile beyond the end", "tile outside the file");
    build(p, base, payload, {{9, offs}, {10, {512, 512, 512, 511}}});
    expect(p, "a short uncompressed tile", "size of a tile");
    { auto t = base; t[7].value = 65536; t[8].value = 65536; build(p, t, payload, {{9, {8}}, {10, {512}}}); expect(p, "a tile of 8 GiB", "4 GiB"); }
}

// tiles that are neither square nor a multiple of 16, predictor 2, and a strip file through the untouched path
static void odd_tiles_and_strips(const std::string &dir)
{
    const int w = 37, spp = 1, TW = 12, TL = 5;
    const long h = 23;
    const auto img = noise(w, h, spp, 5);
    // a strip file of the strip writer still reads to the same samples
    for (int comp : {(int)TIFF_NONE, (int)TIFF_LZW}) {
        write_tiff_u16(dir + "/strips.tiff", img.data(), w, h, spp, false, comp);
        int rw = 0, rs = 0;
        long rh = 0;
        std::vector<uint16_t> back;
        read_tiff_u16(dir + "/strips.tiff", &rw, &rh, &rs, &back);
        const TiffLayout lay = read_tiff_layout(dir + "/strips.tiff");
        CHECK(back == img && rw == w && rh == h && !lay.tiled() && lay.tile_length == 0 && lay.rows_per_strip == (uint64_t)h, "strip file, compression %d", comp);
    }
    const int tx = (w + TW - 1) / TW, ty = (int)((h + TL - 1) / TL);
    std::vector<uint8_t> payload;
    std::vector<uint32_t> offs, lens;
    for (int j = 0; j < ty; ++j)
        for (int i = 0; i < tx; ++i) {
            std::vector<uint16_t> tile((size_t)TW * TL, 0xAAAA);                  // (zero-style padding another writer may leave)
            for (int r = 0; r < TL && j * TL + r < h; ++r)
                for (int c = 0; c < TW && i * TW + c < w; ++c) tile[(size_t)r * TW + c] = img[(size_t)(j * TL + r) * w + i * TW + c];
            for (int r = 0; r < TL; ++r) tiffdetail::predictor2_encode(tile.data() + (size_t)r * TW, TW, 1);
            std::vector<uint8_t> enc(tiffdetail::lzw_worst(tile.size() * 2));
            enc.resize(tiffdetail::lzw_encode_to((const uint8_t *)tile.data(), tile.size() * 2, enc.data()));
            if (payload.size() & 1) payload.push_back(0);
            offs.push_back((uint32_t)(8 + payload.size()));
            lens.push_back((uint32_t)enc.size());
            payload.insert(payload.end(), enc.begin(), enc.end());
        }
    const std::vector<HTag> tags{{256, 4, 1, (uint32_t)w}, {257, 4, 1, (uint32_t)h}, {258, 3, 1, 16}, {259, 3, 1, 5}, {262, 3, 1, 1}, {277, 3, 1, 1}, {284, 3, 1, 1},
                                 {317, 3, 1, 2}, {322, 4, 1, (uint32_t)TW}, {323, 4, 1, (uint32_t)TL}, {324, 4, 0, 0}, {325, 4, 0, 0}, {339, 3, 1, 1}};
    build(dir + "/odd.tiff", tags, payload, {{10, offs}, {11, lens}});
    int rw = 0, rs = 0;
    long rh = 0;
    std::vector<uint16_t> back;
    try {
        read_tiff_u16(dir + "/odd.tiff", &rw, &rh, &rs, &back);
        CHECK(back == img && rw == w && rh == h, "12 x 5 tiles read differently");
    } catch (const std::exception &e) { CHECK(false, "12 x 5 tiles: %s", e.what()); }
}

int main(int argc, char **argv)
{
    const std::string dir = argc > 1 ? argv[1] : ".";
    std::ofstream kept(dir + "/kept.txt");
    int files = 0;
    const int sizes[] = {1, 15, 16, 17, 255, 256, 257};
    for (int spp : {1, 4})
        for (int comp : {(int)TIFF_NONE, (int)TIFF_LZW})
            for (int T : {16, 256})
                for (int levels : {0, 1, 3})
                    for (int w : sizes)
                        for (int h : sizes) round_trip(dir, kept, w, h, spp, comp, T, levels, &files);
    kept.close();
    external_equals_host(dir);
    refusals(dir);
    odd_tiles_and_strips(dir);
    printf("%d files, %d bad\n", files, bad);
    return bad ? 1 : 0;
}
