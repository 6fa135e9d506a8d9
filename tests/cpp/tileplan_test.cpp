// tileplan_test.cpp -- the tile arithmetic of the neighbourhood filters (csrc/oip_tileplan.h) on the CPU.  For every case the
// plan's tiles are walked and the header's own fill indexing is run into a host array that stands in for LDS: every sample a
// lane would read is the replicate-border sample (pixel clamped to the line or the column group, channel kept, line clamped
// to the raster), no index leaves the resident window or the LDS image, the tiles partition the output once; and the plan
// refuses what the three entry points refuse.  Every expectation is restated here, independently of the header.  The source
// window and the LDS image are heap blocks of exactly their size: built with ASan + UBSan by tests/test_tileplan_cpu.py.
#include "oip_tileplan.h"

#include <algorithm>
#include <cstdio>
#include <vector>

static long bad = 0, n = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (++bad < 40) { printf("%s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// the raster [line][pixel][channel]: a 16-bit hash of the three, made once per shape
static const uint16_t *raster(int spp, int W, long L)
{
    static std::vector<uint16_t> img;
    static long shape[3] = {0, 0, 0};
    if (shape[0] == spp && shape[1] == W && shape[2] == L) return img.data();
    shape[0] = spp, shape[1] = W, shape[2] = L;
    img.resize((size_t)(L * W * spp));
    for (long v = 0, i = 0; v < L; ++v)
        for (long p = 0; p < W; ++p)
            for (int ch = 0; ch < spp; ++ch, ++i) {
                uint32_t h = (uint32_t)v * 2654435761u ^ (uint32_t)p * 40503u ^ (uint32_t)ch * 9176u;
                h ^= h >> 15;
                img[(size_t)i] = (uint16_t)(h * 2246822519u >> 16);
            }
    return img.data();
}

static long clampl(long v, long lo, long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one call: output lines [out0, out0 + outn) of a W x L x spp raster in `groups` column groups, exactly the lines it needs
// resident, filters of radius (rx, ry); `odd`: bases that are not 16-byte aligned
static void walk(int spp, int rx, int ry, int W, long L, long out0, long outn, int groups, bool odd)
{
    ++n;
    const char *at = "spp %d rx %d ry %d W %d L %ld out %ld + %ld groups %d odd %d";
#define AT spp, rx, ry, W, L, out0, outn, groups, (int)odd
    const long Ws = (long)W * spp, gws = Ws / groups;
    const long src0 = clampl(out0 - ry, 0, L - 1), src1 = clampl(out0 + outn - 1 + ry, 0, L - 1) + 1;
    // the resident window, a heap block that ends with it; odd: it starts 2 bytes behind a 16-byte boundary.  Nothing is written to dst.
    std::vector<uint16_t> src((size_t)((src1 - src0) * Ws + (odd ? 1 : 0))), dst(8);
    uint16_t *s = src.data() + (odd ? 1 : 0), *d = dst.data();
    const uint16_t *img = raster(spp, W, L);
    std::copy(img + src0 * Ws, img + src1 * Ws, s);
    const OipTilePlan p = oip_tile_plan(s, src0, src1 - src0, d, out0, outn, W, L, spp, 0, ry, groups, W / groups);
    EXPECT(p.refused == OIP_TILE_OK, at, AT);
    if (p.refused != OIP_TILE_OK) return;
    const bool aligned = Ws % 8 == 0 && gws % 8 == 0 && ((uintptr_t)s & 15) == 0 && ((uintptr_t)d & 15) == 0;
    EXPECT(odd ? !aligned : ((uintptr_t)s & 15) == 0, at, AT);
    const long tiles_g = (gws + 511) / 512, tiles_y = (outn + 15) / 16;
    EXPECT(p.aligned == aligned && p.tiles_g == tiles_g && p.args.tiles_x == tiles_g * groups && p.blocks == tiles_g * groups * tiles_y, at, AT);
    EXPECT(p.args.src == s && p.args.dst == d && p.args.Ws == Ws && p.args.L == L && p.args.src_row0 == src0 && p.args.out_row0 == out0 &&
               p.args.out_rows == outn && p.args.W == W && p.args.vmin == 0,
           at, AT);
    const int hp = oip_tile_hp(spp, rx), pitch = oip_tile_pitch(hp);
    EXPECT(hp % 8 == 0 && hp >= rx * spp && hp < rx * spp + 8 && pitch == 512 + 2 * hp && oip_tile_nch(hp) * 8 == pitch, at, AT);
    std::vector<int> written((size_t)(outn * Ws), 0);
    for (long b = 0; b < (long)p.blocks; ++b) {
        const OipTile t = oip_tile_of<true>(p.args, b, spp, hp, ry, p.tiles_g, W / groups);
        if (groups == 1) {                  // the form for a line that is one group gives the same tile
            const OipTile u = oip_tile_of(p.args, b, spp, hp, ry);
            EXPECT(u.y0 == t.y0 && u.x0 == t.x0 && u.rows == t.rows && u.cols == t.cols && u.nch == t.nch && u.nfill == t.nfill && u.g0 == t.g0 &&
                       u.g1 == t.g1,
                   at, AT);
        }
        // the tile, restated: blocks run along a line first, a group's tiles together
        const long ty = b / (tiles_g * groups), tx = b % (tiles_g * groups), g = tx / tiles_g, tg = tx % tiles_g;
        const long y0 = out0 + ty * 16, x0 = g * gws + tg * 512;
        const long rows = out0 + outn - y0 < 16 ? out0 + outn - y0 : 16, cols = (g + 1) * gws - x0 < 512 ? (g + 1) * gws - x0 : 512;
        EXPECT(t.y0 == y0 && t.x0 == x0 && t.rows == rows && t.cols == cols && t.g0 == g * gws && t.g1 == (g + 1) * gws && rows >= 1 && cols >= 1, at, AT);
        for (long r = 0; r < rows; ++r)
            for (long c = 0; c < cols; ++c) {
                const long o = (y0 - out0 + r) * Ws + x0 + c;
                EXPECT(o >= 0 && o < outn * Ws, at, AT);
                if (o >= 0 && o < outn * Ws) ++written[(size_t)o];
            }
        // the fill, by the header's indexing, into an LDS image of exactly the kernels' size
        std::vector<uint16_t> lds((size_t)((16 + 2 * ry) * pitch));
        std::vector<char> filled(lds.size(), 0);
        EXPECT(t.nfill * 8L <= (long)lds.size(), at, AT);
        for (int e = 0; e < t.nfill && e * 8L + 8 <= (long)lds.size(); ++e) {
            const OipTileChunk ch = oip_tile_chunk(p.args, t, e, hp, ry);
            if (!ch.read) continue;
            EXPECT(ch.row >= 0 && ch.row < src1 - src0, at, AT);
            if (ch.row < 0 || ch.row >= src1 - src0) continue;
            const uint16_t *line = p.args.src + ch.row * Ws;
            for (int k = 0; k < 8; ++k) {
                long px = -1, i = ch.s + k;
                if (!oip_tile_chunk_wide(t, p.aligned, ch.s)) {
                    i = oip_tile_border_sample(t, ch.s, k, spp, &px);
                    EXPECT(px >= g * (W / groups) && px < (g + 1) * (W / groups) && i / spp == px, at, AT);
                }
                EXPECT(i >= t.g0 && i < t.g1, at, AT);
                if (i < 0 || i >= Ws) continue;
                lds[(size_t)e * 8 + k] = line[i];
                filled[(size_t)e * 8 + k] = 1;
            }
        }
        // what the lanes read: lane `lane` of the wave on output line r reads samples [lane * 8, lane * 8 + 8 + 2 hp) of LDS lines r .. r + 2 ry
        const long lanes = (cols + 7) / 8;
        for (long i = 0; i < lanes * 8 + 2 * hp; ++i) {
            const long x = x0 - hp + i, ch = ((x % spp) + spp) % spp, px = clampl((x - ch) / spp, g * (W / groups), (g + 1) * (W / groups) - 1);
            for (long lr = 0; lr < rows + 2 * ry; ++lr) {
                const long idx = lr * pitch + i, v = clampl(y0 - ry + lr, 0, L - 1);
                EXPECT(idx < (long)lds.size() && filled[(size_t)idx], at, AT);
                if (idx >= (long)lds.size() || !filled[(size_t)idx]) continue;
                EXPECT(lds[(size_t)idx] == img[(v * W + px) * spp + ch], at, AT);
            }
        }
    }
    for (size_t o = 0; o < written.size(); ++o)
        if (written[o] != 1) { EXPECT(written[o] == 1, at, AT); break; }
#undef AT
}

// what oip_convolve_u16, oip_despike_u16 and oip_sigma_filter_u16 refuse of the arguments they share, in their order
static OipTileRefusal refusal(uintptr_t src, long src0, long srcn, uintptr_t dst, long out0, long outn, int W, long L, int spp, int vmin, int ry, int groups)
{
    if (!src || !dst || (src & 1) || (dst & 1) || (spp != 1 && spp != 4) || (groups == 4 && (spp != 1 || W % 4 != 0)) || W < 1 || L < 1 || vmin < 0 ||
        vmin > 65535 || src0 < 0 || srcn < 0 || out0 < 0 || outn < 0 || outn > L || out0 > L - outn)
        return OIP_TILE_BAD_ARGUMENT;
    if (src == dst) return OIP_TILE_IN_PLACE;
    if (outn == 0) return OIP_TILE_OK;
    if (clampl(out0 - ry, 0, L - 1) < src0 || clampl(out0 + outn - 1 + ry, 0, L - 1) >= src0 + srcn) return OIP_TILE_WINDOW;
    const unsigned __int128 tiles = (unsigned __int128)(((long)(W / groups) * spp + 511) / 512 * groups) * (unsigned __int128)((outn + 15) / 16);
    return tiles >= ((unsigned __int128)1 << 31) ? OIP_TILE_TOO_MANY : OIP_TILE_OK;
}

static void refuse(OipTileRefusal want, uintptr_t src, long src0, long srcn, uintptr_t dst, long out0, long outn, int W, long L, int spp, int vmin, int ry,
                   int groups)
{
    ++n;
    const OipTilePlan p = oip_tile_plan((const uint16_t *)src, src0, srcn, (uint16_t *)dst, out0, outn, W, L, spp, vmin, ry, groups, W / groups);
    const OipTileRefusal today = refusal(src, src0, srcn, dst, out0, outn, W, L, spp, vmin, ry, groups);
    EXPECT(p.refused == want && today == want, "src %#lx %ld + %ld dst %#lx out %ld + %ld W %d L %ld spp %d vmin %d ry %d groups %d: %d, %d today, %d expected",
           (unsigned long)src, src0, srcn, (unsigned long)dst, out0, outn, W, L, spp, vmin, ry, groups, (int)p.refused, (int)today, (int)want);
    if (want == OIP_TILE_WINDOW)
        EXPECT(p.window[0] == clampl(out0 - ry, 0, L - 1) && p.window[1] == clampl(out0 + outn - 1 + ry, 0, L - 1) && p.window[2] == src0 &&
                   p.window[3] == src0 + srcn,
               "window [%ld, %ld] of [%ld, %ld)", p.window[0], p.window[1], p.window[2], p.window[3]);
    if (want == OIP_TILE_OK && outn == 0) EXPECT(p.blocks == 0, "%u blocks for no lines", p.blocks);
}

int main()
{
    // whole rasters: every width, height, filter radius and sample layout; with odd bases too where the lines alone would
    // allow the 16-byte path (elsewhere the bases change nothing in the indexing)
    for (int spp : {1, 4})
        for (int W : {1, 2, 3, 7, 8, 9, 127, 128, 129, 511, 512, 513, 1025})
            for (long L : {1L, 2L, 5L, 16L, 17L, 33L})
                for (int rx = 0; rx <= 4; ++rx)
                    for (int ry = 0; ry <= 4; ++ry) {
                        walk(spp, rx, ry, W, L, 0, L, 1, false);
                        if (W * spp % 8 == 0) walk(spp, rx, ry, W, L, 0, L, 1, true);
                    }
    // output ranges and resident windows cut at every line: two calls, each with exactly the lines it needs
    for (int spp : {1, 4})
        for (int W : {9, 513})
            for (long L : {2L, 5L, 16L, 17L, 33L})
                for (int ry = 0; ry <= 4; ++ry)
                    for (long cut = 1; cut < L; ++cut) {
                        walk(spp, ry == 0 ? 1 : ry - 1, ry, W, L, 0, cut, 1, cut % 2);
                        walk(spp, ry == 0 ? 1 : ry - 1, ry, W, L, cut, L - cut, 1, cut % 2 == 0);
                    }
    // four column groups (the bands of a BIL line, 1 sample per pixel): the border is the group's
    for (int W : {4, 8, 148, 2048})
        for (long L : {1L, 17L, 33L})
            for (int rx = 0; rx <= 4; ++rx)
                for (long cut = 0; cut < L; cut += 16) {
                    walk(1, rx, 1, W, L, cut, L - cut, 4, false);
                    walk(1, rx, rx, W, L, 0, L - cut, 4, true);
                }

    // the refusals.  A call that passes: lines [10, 50) of a 100 x 64 raster with lines [8, 52) resident, radius 2
    const uintptr_t S = 0x10000, D = 0x20000;
    refuse(OIP_TILE_OK, S, 8, 44, D, 10, 40, 100, 64, 1, 0, 2, 1);
    refuse(OIP_TILE_OK, S + 2, 8, 44, D + 6, 10, 40, 100, 64, 4, 65535, 2, 1);
    refuse(OIP_TILE_OK, S, 8, 44, D, 10, 40, 100, 64, 1, 0, 2, 4);
    refuse(OIP_TILE_OK, S, 0, 0, D, 64, 0, 100, 64, 1, 0, 2, 1);                    // no lines: nothing resident is needed
    refuse(OIP_TILE_BAD_ARGUMENT, 0, 8, 44, D, 10, 40, 100, 64, 1, 0, 2, 1);
    refuse(OIP_TILE_BAD_ARGUMENT, S, 8, 44, 0, 10, 40, 100, 64, 1, 0, 2, 1);
    refuse(OIP_TILE_BAD_ARGUMENT, S + 1, 8, 44, D, 10, 40, 100, 64, 1, 0, 2, 1);    // odd bases
    refuse(OIP_TILE_BAD_ARGUMENT, S, 8, 44, D + 1, 10, 40, 100, 64, 1, 0, 2, 1);
    for (int spp : {-1, 0, 2, 3, 5, 8}) refuse(OIP_TILE_BAD_ARGUMENT, S, 8, 44, D, 10, 40, 100, 64, spp, 0, 2, 1);
    refuse(OIP_TILE_BAD_ARGUMENT, S, 8, 44, D, 10, 40, 0, 64, 1, 0, 2, 1);
    refuse(OIP_TILE_BAD_ARGUMENT, S, 8, 44, D, 10, 40, -4, 64, 1, 0, 2, 4);
    refuse(OIP_TILE_BAD_ARGUMENT, S, 0, 0, D, 0, 0, 100, 0, 1, 0, 2, 1);
    refuse(OIP_TILE_BAD_ARGUMENT, S, 8, 44, D, 10, 40, 100, 64, 1, -1, 2, 1);
    refuse(OIP_TILE_BAD_ARGUMENT, S, 8, 44, D, 10, 40, 100, 64, 1, 65536, 2, 1);
    refuse(OIP_TILE_BAD_ARGUMENT, S, -1, 53, D, 10, 40, 100, 64, 1, 0, 2, 1);
    refuse(OIP_TILE_BAD_ARGUMENT, S, 8, -1, D, 10, 40, 100, 64, 1, 0, 2, 1);
    refuse(OIP_TILE_BAD_ARGUMENT, S, 0, 64, D, -1, 40, 100, 64, 1, 0, 2, 1);
    refuse(OIP_TILE_BAD_ARGUMENT, S, 0, 64, D, 10, -1, 100, 64, 1, 0, 2, 1);
    refuse(OIP_TILE_BAD_ARGUMENT, S, 0, 64, D, 0, 65, 100, 64, 1, 0, 2, 1);
    refuse(OIP_TILE_BAD_ARGUMENT, S, 0, 64, D, 25, 40, 100, 64, 1, 0, 2, 1);        // out_row0 > L - out_rows
    refuse(OIP_TILE_OK, S, 0, 64, D, 24, 40, 100, 64, 1, 0, 2, 1);
    refuse(OIP_TILE_BAD_ARGUMENT, S, 0, 64, D, 65, 0, 100, 64, 1, 0, 2, 1);
    refuse(OIP_TILE_BAD_ARGUMENT, S, 8, 44, D, 10, 40, 100, 64, 4, 0, 2, 4);        // groups only at 1 sample per pixel
    for (int W : {101, 102, 103}) refuse(OIP_TILE_BAD_ARGUMENT, S, 8, 44, D, 10, 40, W, 64, 1, 0, 2, 4);
    refuse(OIP_TILE_BAD_ARGUMENT, S, 8, 44, S, 10, 40, 0, 64, 1, 0, 2, 1);          // a bad argument comes before "not in place"
    refuse(OIP_TILE_IN_PLACE, S, 8, 44, S, 10, 40, 100, 64, 1, 0, 2, 1);
    refuse(OIP_TILE_IN_PLACE, S, 0, 0, S, 10, 40, 100, 64, 1, 0, 2, 1);             // ... and "not in place" before the window
    refuse(OIP_TILE_IN_PLACE, S, 0, 0, S, 10, 0, 100, 64, 1, 0, 2, 1);
    refuse(OIP_TILE_WINDOW, S, 9, 43, D, 10, 40, 100, 64, 1, 0, 2, 1);              // one line short at the top
    refuse(OIP_TILE_WINDOW, S, 8, 43, D, 10, 40, 100, 64, 1, 0, 2, 1);              // ... at the bottom
    refuse(OIP_TILE_WINDOW, S, 8, 44, D, 10, 40, 100, 64, 1, 0, 3, 1);
    refuse(OIP_TILE_OK, S, 10, 40, D, 10, 40, 100, 64, 1, 0, 0, 1);
    refuse(OIP_TILE_OK, S, 0, 64, D, 0, 64, 100, 64, 1, 0, 4, 1);                   // the halo beyond the raster is not asked for
    refuse(OIP_TILE_WINDOW, S, 1, 63, D, 0, 64, 100, 64, 1, 0, 0, 1);
    refuse(OIP_TILE_WINDOW, S, 0, 63, D, 0, 64, 100, 64, 1, 0, 0, 1);
    // 2^21 tiles across x 1024 down = 2^31, and one row of tiles fewer
    refuse(OIP_TILE_TOO_MANY, S, 0, 16384, D, 0, 16384, 1 << 30, 16384, 1, 0, 1, 1);
    refuse(OIP_TILE_TOO_MANY, S, 0, 16384, D, 0, 16384 - 15, 1 << 30, 16384, 1, 0, 1, 4);
    refuse(OIP_TILE_TOO_MANY, S, 0, 16384, D, 0, 16384, 1 << 28, 16384, 4, 0, 1, 1);
    refuse(OIP_TILE_OK, S, 0, 16384, D, 0, 16384 - 16, 1 << 30, 16384, 1, 0, 1, 1);
    refuse(OIP_TILE_OK, S, 0, 16384, D, 0, 16384 - 16, 1 << 30, 16384, 1, 0, 1, 4);
    {
        const OipTilePlan p = oip_tile_plan((const uint16_t *)S, 0, 16384, (uint16_t *)D, 0, 16384 - 16, 1 << 30, 16384, 1, 0, 1, 1, 1 << 30);
        EXPECT(p.blocks == 0x7fe00000u && p.args.tiles_x == 1 << 21, "%u blocks, %d across", p.blocks, p.args.tiles_x);
        const OipTile t = oip_tile_of(p.args, p.blocks - 1, 1, 8, 1);                 // the last tile of such a call
        EXPECT(t.y0 == 16384 - 32 && t.rows == 16 && t.x0 == (1L << 30) - 512 && t.cols == 512, "tile at %ld, %ld: %d x %d", t.y0, t.x0, t.rows, t.cols);
    }
    printf("%ld cases, %ld bad\n", n, bad);
    return bad ? 1 : 0;
}
