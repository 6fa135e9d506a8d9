// jpeg_encode_test.cpp -- the host instantiation of csrc/oip_jpeg.h (the baseline JPEG scan coder the device runs as well) and its
// file writer.  Built with ASan + UBSan by tests/test_jpeg_cpu.py.
//   jpeg_encode_test DIR   every line `NAME w h nch quality pitch` of DIR/list.txt: DIR/NAME.bin holds the image, (h - 1) * pitch +
//                          w * nch bytes.  Every interval is encoded from a heap block of exactly that size into a heap block of
//                          exactly its bound (416 bytes a block), at changing alignments, so a read or write past either is a
//                          report; the same bytes must come out at another alignment, and an encode into a block one byte shorter
//                          than the interval must return 0 and stay inside it.  DIR/NAME.iv gets, per interval, its length (4 bytes,
//                          little-endian) and its bytes; DIR/NAME.jpg the file the writer makes of them.
#include "oip_jpeg.h"

#include <cstdio>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

static long bad = 0;
#define CHECK(c, ...) do { if (!(c)) { ++bad; printf(__VA_ARGS__); printf("\n"); } } while (0)

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: jpeg_encode_test DIR\n"); return 2; }
    const std::string dir = argv[1];
    std::ifstream list(dir + "/list.txt");
    std::string name;
    int w, h, nch, quality;
    long pitch, count = 0;
    std::unique_ptr<oipjpeg::Shared<1>> work(new oipjpeg::Shared<1>);
    while (list >> name >> w >> h >> nch >> quality >> pitch) {
        const size_t n = (size_t)(h - 1) * pitch + (size_t)w * nch, a = (size_t)(count * 7 % 16), b = (a + 5) % 16;
        std::unique_ptr<uint8_t[]> in(new uint8_t[a + n]), in2(new uint8_t[b + n]);
        FILE *f = fopen((dir + "/" + name + ".bin").c_str(), "rb");
        if (!f || fread(in.get() + a, 1, n, f) != n) { ++bad; printf("cannot read %s.bin\n", name.c_str()); if (f) fclose(f); continue; }
        fclose(f);
        memcpy(in2.get() + b, in.get() + a, n);
        const size_t cap = (size_t)((w + 7) / 8) * nch * oipjpeg::kBlockBytes;
        const long intervals = (h + 7) / 8;
        std::vector<uint8_t> payload;
        std::vector<uint64_t> off, len;
        for (long k = 0; k < intervals; ++k) {
            std::unique_ptr<uint8_t[]> out(new uint8_t[a + cap]), out2(new uint8_t[b + 3 + cap]);
            const size_t size = oipjpeg::interval_host(in.get() + a, pitch, w, h, nch, quality, k, out.get() + a, cap, work.get());
            CHECK(size > 0 && size <= cap, "%s interval %ld: size %zu of at most %zu", name.c_str(), k, size, cap);
            if (size == 0 || size > cap) continue;
            const size_t size2 = oipjpeg::interval_host(in2.get() + b, pitch, w, h, nch, quality, k, out2.get() + b + 3, cap, work.get());
            CHECK(size2 == size && memcmp(out.get() + a, out2.get() + b + 3, size) == 0, "%s interval %ld: output depends on alignment", name.c_str(), k);
            std::unique_ptr<uint8_t[]> small(new uint8_t[size - 1 ? size - 1 : 1]);
            CHECK(oipjpeg::interval_host(in.get() + a, pitch, w, h, nch, quality, k, small.get(), size - 1, work.get()) == 0, "%s interval %ld: fits in %zu bytes?",
                  name.c_str(), k, size - 1);
            CHECK(size - 1 == 0 || memcmp(small.get(), out.get() + a, size - 1) == 0, "%s interval %ld: the bytes that fitted differ", name.c_str(), k);
            off.push_back(payload.size());
            len.push_back(size);
            payload.insert(payload.end(), out.get() + a, out.get() + a + size);
        }
        if ((long)off.size() != intervals) continue;
        FILE *g = fopen((dir + "/" + name + ".iv").c_str(), "wb");
        bool ok = g != nullptr;
        for (long k = 0; k < intervals && ok; ++k) {
            const uint8_t l4[4] = {(uint8_t)len[k], (uint8_t)(len[k] >> 8), (uint8_t)(len[k] >> 16), (uint8_t)(len[k] >> 24)};
            ok = fwrite(l4, 1, 4, g) == 4 && fwrite(payload.data() + off[k], 1, (size_t)len[k], g) == (size_t)len[k];
        }
        if (g) fclose(g);
        CHECK(ok, "cannot write %s.iv", name.c_str());
        CHECK(oipjpeg::write_file((dir + "/" + name + ".jpg").c_str(), payload.data(), off.data(), len.data(), w, h, nch, quality), "cannot write %s.jpg", name.c_str());
        printf("image %s %d x %d x %d quality %d: %ld intervals, %zu bytes\n", name.c_str(), w, h, nch, quality, intervals, payload.size());
        ++count;
    }
    printf("%ld images, %ld bad\n", count, bad);
    return bad ? 1 : 0;
}
