// stripplan_test.cpp -- the block geometry of the strip-streaming raster tools (csrc/oip_stripplan.hpp) on the CPU: the
// blocks of a plan tile their line range exactly once, read the clamped halo, fit the buffers the plan sizes, alternate the
// two slots; the default block size follows its rule; byte offsets hold past 2^32.  Every expectation is restated here,
// independently of the header.  Built with ASan + UBSan by tests/test_stripplan_cpu.py.
#include "oip_stripplan.hpp"

#include <cstdio>

using namespace OIPGPU;

static int bad = 0, n = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { ++bad; printf("%s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void tiling(long L, long first, long cnt, long blockLines, long halo)
{
    ++n;
    const StripPlan p{first, cnt, L, halo, blockLines, 6};
    const long blocks = cnt / blockLines + (cnt % blockLines ? 1 : 0);
    const long cap = blockLines < cnt ? blockLines : cnt;
    long inCap = cap + 2 * halo;
    if (inCap > L) inCap = L;
    EXPECT(p.blocks() == blocks, "L %ld first %ld n %ld block %ld: %ld blocks, %ld expected", L, first, cnt, blockLines, p.blocks(), blocks);
    EXPECT(p.secondSlot() == (blocks > 1), "L %ld n %ld block %ld: second slot %d with %ld blocks", L, cnt, blockLines, (int)p.secondSlot(), blocks);
    EXPECT(p.outLines() == cap && p.inLines() == inCap, "L %ld n %ld block %ld halo %ld: capacities %ld / %ld, %ld / %ld expected", L, cnt, blockLines, halo,
           p.outLines(), p.inLines(), cap, inCap);
    long next = first;                      // the first line no block has produced yet
    for (long i = 0; i < p.blocks(); ++i) {
        const StripBlock b = p.block(i);
        const char *at = "L %ld first %ld n %ld block %ld halo %ld, block %ld";
        EXPECT(b.dstFirst == next && b.dstLines >= 1 && b.dstFirst + b.dstLines <= first + cnt, at, L, first, cnt, blockLines, halo, i);
        EXPECT(i == p.blocks() - 1 ? b.dstFirst + b.dstLines == first + cnt : b.dstLines == blockLines, at, L, first, cnt, blockLines, halo, i);
        long s0 = b.dstFirst - halo, s1 = b.dstFirst + b.dstLines + halo;
        if (s0 < 0) s0 = 0;
        if (s1 > L) s1 = L;
        EXPECT(b.srcFirst == s0 && b.srcLines == s1 - s0, at, L, first, cnt, blockLines, halo, i);
        EXPECT(b.srcLines <= p.inLines() && b.dstLines <= p.outLines(), at, L, first, cnt, blockLines, halo, i);
        EXPECT(b.slot == (int)(i % 2), at, L, first, cnt, blockLines, halo, i);
        EXPECT(b.srcOffset == (size_t)s0 * 6 && b.srcBytes == (size_t)(s1 - s0) * 6, at, L, first, cnt, blockLines, halo, i);
        EXPECT(b.dstOffset == (size_t)(next - first) * 6 && b.dstBytes == (size_t)b.dstLines * 6, at, L, first, cnt, blockLines, halo, i);
        next += b.dstLines;
    }
    EXPECT(next == first + cnt, "L %ld first %ld n %ld block %ld: tiled up to %ld", L, first, cnt, blockLines, next);
}

int main()
{
    // exhaustive tiling: whole images and ranges inside them, blocks smaller than, equal to and larger than the range, halos
    // larger than a block and larger than the image
    for (long L = 1; L <= 70; ++L)
        for (long first : {0L, 3L}) {
            if (first >= L) continue;
            const long whole = L - first, shorter = (whole + 1) / 2;
            for (long cnt : {whole, shorter})
                for (long blockLines = 1; blockLines <= 20; ++blockLines)
                    for (long halo = 0; halo <= 4; ++halo) tiling(L, first, cnt, blockLines, halo);
        }

    // default block lines: 64 MiB of lines, a multiple of q, at least q
    const size_t MiB64 = (size_t)64 * 1024 * 1024;
    for (size_t lineBytes : {(size_t)2, (size_t)24576, MiB64, MiB64 + 2, 3 * MiB64})
        for (long q = 1; q <= 64; q *= 2) {
            ++n;
            long want = (long)(MiB64 / lineBytes);
            want -= want % q;
            if (want < q) want = q;
            const long got = StripBlockLines(lineBytes, q);
            EXPECT(got == want && got > 0 && got % q == 0, "%zu bytes per line, q %ld: %ld lines, %ld expected", lineBytes, q, got, want);
            if (lineBytes >= MiB64) EXPECT(got == q, "%zu bytes per line, q %ld: %ld lines", lineBytes, q, got);
            EXPECT(StripBlockLines(lineBytes, q, 7) == 7, "%zu bytes per line, q %ld: an override of 7 gives %ld", lineBytes, q, StripBlockLines(lineBytes, q, 7));
            EXPECT(StripBlockLines(lineBytes, q, 0) == want && StripBlockLines(lineBytes, q, -5) == want, "%zu bytes per line, q %ld: overrides 0 / -5 give %ld / %ld",
                   lineBytes, q, StripBlockLines(lineBytes, q, 0), StripBlockLines(lineBytes, q, -5));
        }
    ++n;
    EXPECT(StripBlockLines(24576) == 2730 && StripBlockLines(24576, 16) == 2720 && StripBlockLines(2) == 33554432, "a 12288-sample line: %ld / %ld lines",
           StripBlockLines(24576), StripBlockLines(24576, 16));

    // byte offsets past 2^32: 200 000 lines of 24 576 bytes in the default blocks, the last block, with a halo and a range
    for (long first : {0L, 1000L}) {
        ++n;
        const long L = 200000, cnt = L - first, halo = 4, blockLines = 2730;
        const StripPlan p{first, cnt, L, halo, blockLines, 24576};
        const long last = (cnt - 1) / blockLines;
        const StripBlock b = p.block(last);
        const unsigned __int128 lb = 24576;
        const long r = first + last * blockLines, m = first + cnt - r, s0 = r - halo;
        EXPECT(p.blocks() == last + 1 && b.dstFirst == r && b.dstLines == m && b.srcFirst == s0 && b.srcLines == L - s0, "last block %ld: lines %ld + %ld from %ld + %ld", last,
               b.dstFirst, b.dstLines, b.srcFirst, b.srcLines);
        EXPECT((unsigned __int128)b.srcOffset == lb * (unsigned __int128)s0 && (unsigned __int128)b.srcBytes == lb * (unsigned __int128)(L - s0),
               "source bytes %zu + %zu", b.srcOffset, b.srcBytes);
        EXPECT((unsigned __int128)b.dstOffset == lb * (unsigned __int128)(r - first) && (unsigned __int128)b.dstBytes == lb * (unsigned __int128)m,
               "destination bytes %zu + %zu", b.dstOffset, b.dstBytes);
        EXPECT(b.srcOffset > ((size_t)1 << 32) && b.dstOffset > ((size_t)1 << 32) && b.srcOffset + b.srcBytes == (size_t)4915200000ull, "offsets %zu / %zu do not pass 2^32",
               b.srcOffset, b.dstOffset);
    }
    printf("%d cases, %d bad\n", n, bad);
    return bad ? 1 : 0;
}
