// deflate_encode_test.cpp -- the host instantiation of csrc/oip_deflate.h (the encoder the device runs as well) and the Deflate
// branch of the two TIFF writers (csrc/oip_tiff.hpp, csrc/oip_tifftiled.hpp).  Built with ASan + UBSan by
// tests/test_deflate_encode_cpu.py.
//   deflate_encode_test streams DIR   every NAME of DIR/list.txt: DIR/NAME.bin is encoded into DIR/NAME.z and decoded again with the
//                                     project's host decoder.  Input and output are heap blocks of exactly n and stored_bound(n) bytes
//                                     at changing alignments, so a read or write past either is a report; a second encode into a block
//                                     one byte shorter than the stream must return 0 and stay inside it.
//   deflate_encode_test codes         the code builder alone: Fibonacci frequencies, whose Huffman tree is a path, under the 15-bit
//                                     and the 7-bit limit, and sets of zero, one and two used symbols.
//   deflate_encode_test tiff LIST     LIST: lines `strips|ovr|tiles out.tiff in.raw width height spp a b`; the image of in.raw through
//                                     TiffWriterU16 (strips; ovr: a = levels, every level the even pixels of the one before) or
//                                     TiffTiledWriterU16 (a = tile, b = levels, likewise) with TIFF_DEFLATE.
#include "oip_tifftiled.hpp"

#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

using namespace OIPGPU;

static long bad = 0;
#define CHECK(c, ...) do { if (!(c)) { ++bad; printf(__VA_ARGS__); printf("\n"); } } while (0)

static std::vector<uint8_t> slurp(const std::string &p)
{
    std::vector<uint8_t> v;
    FILE *f = fopen(p.c_str(), "rb");
    if (!f) { ++bad; printf("cannot open %s\n", p.c_str()); return v; }
    fseeko(f, 0, SEEK_END);
    v.resize((size_t)ftello(f));
    rewind(f);
    if (fread(v.data(), 1, v.size(), f) != v.size()) { ++bad; v.clear(); }
    fclose(f);
    return v;
}

static int streams(const std::string &dir)
{
    std::ifstream list(dir + "/list.txt");
    std::string name;
    long count = 0;
    std::unique_ptr<oipdeflate::Shared> enc(new oipdeflate::Shared);
    std::unique_ptr<oipinflate::Shared> dec(new oipinflate::Shared);
    while (list >> name) {
        const std::vector<uint8_t> file = slurp(dir + "/" + name + ".bin");
        const size_t n = file.size(), cap = oipdeflate::stored_bound(n), a = (size_t)(count * 7 % 16);
        // exact-size blocks: [a, a + n) of one, [a, a + cap) of another -- new[] of a + n bytes ends where the input ends
        std::unique_ptr<uint8_t[]> in(new uint8_t[a + n]), out(new uint8_t[a + cap]);
        if (n) memcpy(in.get() + a, file.data(), n);
        memset(out.get() + a, 0xA5, cap);
        const size_t size = oipdeflate::deflate_host(in.get() + a, n, out.get() + a, cap, enc.get());
        CHECK(size > 0 && size <= cap, "%s: size %zu of at most %zu", name.c_str(), size, cap);
        if (size == 0 || size > cap) continue;
        // the same bytes at another alignment of input and output
        {
            const size_t b = (a + 5) % 16;
            std::unique_ptr<uint8_t[]> in2(new uint8_t[b + n]), out2(new uint8_t[b + 3 + cap]);
            if (n) memcpy(in2.get() + b, file.data(), n);
            const size_t size2 = oipdeflate::deflate_host(in2.get() + b, n, out2.get() + b + 3, cap, enc.get());
            CHECK(size2 == size && memcmp(out.get() + a, out2.get() + b + 3, size) == 0, "%s: output depends on alignment", name.c_str());
        }
        // one byte too few: refused, nothing past the block
        {
            std::unique_ptr<uint8_t[]> small(new uint8_t[size - 1 ? size - 1 : 1]);
            CHECK(oipdeflate::deflate_host(in.get() + a, n, small.get(), size - 1, enc.get()) == 0, "%s: fits in %zu bytes?", name.c_str(), size - 1);
        }
        std::unique_ptr<uint8_t[]> back(new uint8_t[n ? n : 1]);
        size_t got = 0;
        const int st = oipinflate::inflate_host(out.get() + a, size, back.get(), n, &got, dec.get());
        CHECK(st == oipinflate::kOk && got == n && (n == 0 || memcmp(back.get(), file.data(), n) == 0), "%s: own decoder: status %d (%s), %zu of %zu bytes",
              name.c_str(), st, oipinflate::status_text(st), got, n);
        CHECK(out[a] == 0x78 && ((out[a] << 8) | out[a + 1]) % 31 == 0 && !(out[a + 1] & 0x20), "%s: header", name.c_str());
        FILE *f = fopen((dir + "/" + name + ".z").c_str(), "wb");
        if (!f || fwrite(out.get() + a, 1, size, f) != size) { ++bad; printf("cannot write %s.z\n", name.c_str()); }
        if (f) fclose(f);
        printf("stream %s %zu %zu\n", name.c_str(), n, size);
        ++count;
    }
    printf("%ld streams, %ld bad\n", count, bad);
    return bad ? 1 : 0;
}

// lengths of the used symbols of freq[0, nsym) under `maxbits`: complete (Kraft sum one), none longer than maxbits, a symbol that
// occurs more often never longer than one that occurs less; `deeper`: the unlimited tree is deeper than maxbits, so the limit acted
static void one_set(const char *what, const std::vector<unsigned> &freq, unsigned maxbits, bool deeper)
{
    std::unique_ptr<oipdeflate::Shared> sh(new oipdeflate::Shared);
    oipdeflate::HostLane lane;
    oipdeflate::ByteSource src{nullptr};
    uint8_t none[1];
    oipdeflate::Encoder<oipdeflate::HostLane, oipdeflate::ByteSource> e(lane, *sh, src, 0, none, 0);
    const unsigned nsym = (unsigned)freq.size();
    for (unsigned s = 0; s < nsym; ++s) sh->lfreq[s] = freq[s];
    e.build(sh->lfreq, nsym, maxbits, sh->llen, sh->lcode);
    unsigned long long kraft = 0;
    unsigned longest = 0, used = 0;
    for (unsigned s = 0; s < nsym; ++s) {
        const unsigned l = sh->llen[s];
        CHECK((l != 0) == (sh->lfreq[s] != 0), "%s: symbol %u: length %u, frequency %u", what, s, l, sh->lfreq[s]);
        if (!l) continue;
        ++used;
        kraft += 1ull << (32 - l);
        if (l > longest) longest = l;
        for (unsigned t = 0; t < nsym; ++t)
            if (sh->llen[t]) CHECK(!(freq[s] > freq[t] && l > sh->llen[t]), "%s: %u (%u times) longer than %u (%u times)", what, s, freq[s], t, freq[t]);
        // prefix-free by construction of canonical codes; the codes are distinct among equal lengths
        for (unsigned t = 0; t < s; ++t) CHECK(!(sh->llen[t] == l && sh->lcode[t] == sh->lcode[s]), "%s: symbols %u and %u share a code", what, t, s);
    }
    CHECK(used >= 2 && kraft == 1ull << 32, "%s: %u codes, Kraft sum %llu / 2^32", what, used, kraft);
    CHECK(longest <= maxbits && (!deeper || longest == maxbits), "%s: longest code %u of %u", what, longest, maxbits);
    printf("set %s: %u codes, longest %u\n", what, used, longest);
}

static int codes()
{
    std::vector<unsigned> fib = {1, 1};
    while (fib.size() < 24) fib.push_back(fib[fib.size() - 1] + fib[fib.size() - 2]);      // .. 4181 is not reached at 24: 1 .. 46368
    std::vector<unsigned> lit(286, 0);
    for (size_t i = 0; i < 24; ++i) lit[(i * 11) % 256] = fib[i];
    one_set("fibonacci 24 / 15 bits", lit, 15, true);
    std::vector<unsigned> cl(fib.begin(), fib.begin() + 19);
    one_set("fibonacci 19 / 7 bits", cl, 7, true);
    one_set("no symbol", std::vector<unsigned>(30, 0), 15, false);
    std::vector<unsigned> one(30, 0);
    one[7] = 5;
    one_set("one symbol", one, 15, false);
    one[0] = 9;
    one_set("two symbols", one, 15, false);
    std::vector<unsigned> flat(286, 3);
    one_set("286 equal", flat, 15, false);
    printf("codes, %ld bad\n", bad);
    return bad ? 1 : 0;
}

// the even pixels of an image: the next level of this program's pyramids
static std::vector<uint16_t> halve(const std::vector<uint16_t> &img, int w, long h, int spp)
{
    const int nw = (w + 1) / 2;
    const long nh = (h + 1) / 2;
    std::vector<uint16_t> out((size_t)nw * nh * spp);
    for (long y = 0; y < nh; ++y)
        for (int x = 0; x < nw; ++x)
            for (int c = 0; c < spp; ++c) out[((size_t)y * nw + x) * spp + c] = img[((size_t)(2 * y) * w + 2 * x) * spp + c];
    return out;
}

// tile-major form with the last column and line replicated (include/oip_c.h: oip_retile_u16)
static std::vector<uint16_t> retile(const std::vector<uint16_t> &img, int w, long h, int spp, int T)
{
    const long tx = (w + T - 1) / T, ty = (h + T - 1) / T;
    std::vector<uint16_t> out((size_t)tx * ty * T * T * spp);
    size_t o = 0;
    for (long j = 0; j < ty; ++j)
        for (long i = 0; i < tx; ++i)
            for (int y = 0; y < T; ++y)
                for (int x = 0; x < T; ++x) {
                    const long sy = std::min<long>(j * T + y, h - 1), sx = std::min<long>(i * T + x, w - 1);
                    for (int c = 0; c < spp; ++c) out[o++] = img[((size_t)sy * w + sx) * spp + c];
                }
    return out;
}

static int tiff(const std::string &listPath)
{
    std::ifstream list(listPath);
    std::string line;
    long count = 0;
    while (std::getline(list, line)) {
        std::istringstream ls(line);
        std::string kind, out, raw;
        int w, spp, a, b;
        long h;
        if (!(ls >> kind >> out >> raw >> w >> h >> spp >> a >> b)) continue;
        ++count;
        const std::vector<uint8_t> bytes = slurp(raw);
        CHECK(bytes.size() == (size_t)w * h * spp * 2, "%s: size", raw.c_str());
        if (bytes.size() != (size_t)w * h * spp * 2) continue;
        std::vector<uint16_t> img((size_t)w * h * spp);
        memcpy(img.data(), bytes.data(), bytes.size());
        try {
            if (kind == "strips") {
                TiffWriterU16 tw(out, w, h, spp, false, TIFF_DEFLATE);
                const long first = h / 3;                                      // rows arrive in two uneven parts: a strip is completed by the second
                if (first) tw.write_rows(img.data(), first);
                tw.write_rows(img.data() + (size_t)first * w * spp, h - first);
                tw.close();
            } else if (kind == "ovr") {
                TiffWriterU16 tw(out, w, h, spp, false, TIFF_DEFLATE, a);
                std::vector<uint16_t> cur = img;
                int cw = w;
                long ch = h;
                for (int k = 1; k <= a; ++k) {
                    cur = halve(cur, cw, ch, spp);
                    cw = (cw + 1) / 2; ch = (ch + 1) / 2;
                    CHECK(tw.width() == cw && tw.height() == ch, "%s: level %d geometry", out.c_str(), k);
                    tw.write_rows(cur.data(), ch);
                    if (k < a) tw.next_directory();
                }
                tw.close();
            } else {
                TiffTiledWriterU16 tw(out, w, h, spp, a, TIFF_DEFLATE, b);
                std::vector<uint16_t> cur = img;
                int cw = w;
                long ch = h;
                for (int k = 0; k <= b; ++k) {
                    tw.write_tiles(retile(cur, cw, ch, spp, a).data());
                    if (k < b) { cur = halve(cur, cw, ch, spp); cw = (cw + 1) / 2; ch = (ch + 1) / 2; tw.next_directory(); }
                }
                tw.close();
            }
            // and back through the project's own reader
            int rw = 0, rspp = 0;
            long rh = 0;
            std::vector<uint16_t> back;
            read_tiff_u16(out, &rw, &rh, &rspp, &back);
            const std::vector<uint16_t> want = kind == "ovr" ? halve(img, w, h, spp) : img;
            CHECK(rspp == spp && back == want, "%s: read_tiff_u16 returns another image", out.c_str());
        } catch (const std::exception &e) {
            CHECK(false, "%s: %s", out.c_str(), e.what());
        }
    }
    printf("%ld files, %ld bad\n", count, bad);
    return bad ? 1 : 0;
}

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "streams" && argc == 3) return streams(argv[2]);
    if (mode == "codes") return codes();
    if (mode == "tiff" && argc == 3) return tiff(argv[2]);
    fprintf(stderr, "usage: deflate_encode_test streams DIR | codes | tiff LIST\n");
    return 2;
}
