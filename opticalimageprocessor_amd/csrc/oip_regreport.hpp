// oip_regreport.hpp -- the host side of `oip regcheck` that needs no device: where the two images overlap, and the report
// (CSV + summary) made from the tile records of oip_match_tiles_u16 through oip_match_peak and oip_match_summary.  Free of
// HIP, so tests/cpp/regreport_test.cpp runs it under ASan + UBSan.
#pragma once

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "oip_c.h"

namespace OIPGPU {

// Image 2's origin lies at (shiftX, shiftY) in image-1 coordinates.  The intersection of the w1 x h1 and w2 x h2 images:
// its origin in image 1 (ax, ay), in image 2 (bx, by), and its size; false if it is empty.
struct RegOverlap {
    long ax = 0, ay = 0, bx = 0, by = 0, w = 0, h = 0;
};
inline bool RegIntersect(long w1, long h1, long w2, long h2, long shiftX, long shiftY, RegOverlap *o)
{
    const long x0 = shiftX > 0 ? shiftX : 0, y0 = shiftY > 0 ? shiftY : 0;
    const long x1 = w1 < shiftX + w2 ? w1 : shiftX + w2, y1 = h1 < shiftY + h2 ? h1 : shiftY + h2;
    if (x1 <= x0 || y1 <= y0) return false;
    o->ax = x0; o->ay = y0; o->bx = x0 - shiftX; o->by = y0 - shiftY; o->w = x1 - x0; o->h = y1 - y0;
    return true;
}

// the grid of one oip_match_tiles_u16 call inside the overlap, and what maps a tile to image-1 pixels: the template centre of
// tile (j, i) is at ((originX + x0 + i step) + T / 2) * scale, likewise y (scale: the --scale factor, 1 without one)
struct RegGrid {
    int T = 0, S = 0, step = 0, x0 = 0, nx = 0, scale = 1;
    long y0 = 0, ny = 0, originX = 0, originY = 0;
};

// the mask of image 1 that `oip regcheck --mask` hands in: gw x gh bytes of `oip mask` with cells of `cell` pixels; a tile
// whose template footprint touches a cell with a bit of `bits` set gets OIP_MATCH_MASKED
struct RegMask {
    const uint8_t *flags = nullptr;
    int gw = 0, cell = 8, bits = OIP_MASK_CLOUD | OIP_MASK_BUFFER;
    long gh = 0;
};

struct RegSummary {
    long tiles = 0, nodata = 0, flat = 0, edge = 0, weak = 0;
    long masked = -1;                           // -1: no mask was given, and the summary line does not speak of one
    double s[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // oip_match_summary: count, mean dx, mean dy, std dx, std dy, rms, ce90, max
};

// the one line of the summary that the log and the report's tail share
inline std::string RegSummaryLine(const RegSummary &r)
{
    char buf[512];
    const std::string masked = r.masked >= 0 ? ", masked " + std::to_string(r.masked) : "";
    snprintf(buf, sizeof buf, "tiles %ld, used %.0f (nodata %ld, flat %ld, edge %ld, weak %ld%s): mean dx %.4f dy %.4f, std dx %.4f dy %.4f, rms %.4f, ce90 %.4f, max %.4f",
             r.tiles, r.s[0], r.nodata, r.flat, r.edge, r.weak, masked.c_str(), r.s[1], r.s[2], r.s[3], r.s[4], r.s[5], r.s[6], r.s[7]);
    return buf;
}

// `# params`, one `x,y,dx,dy,score,flags` line per tile (row-major), then the summary as `#` lines.  records: nx * ny records of
// OIP_MATCH_RECORD_WORDS words.  mask (may be NULL): a tile whose template footprint in image-1 pixels, [x, x + T scale) x
// [y, y + T scale), touches a masked cell gets OIP_MATCH_MASKED on top of what oip_match_peak gave it.  Returns false where a
// record is refused by oip_match_peak or the file cannot be written.
inline bool WriteRegReport(FILE *f, const std::string &params, const uint64_t *records, const RegGrid &g, double minScore, RegSummary *sum,
                           const RegMask *mask = nullptr)
{
    const long n = (long)g.nx * g.ny;
    std::vector<double> dx((size_t)n), dy((size_t)n);
    std::vector<int> flags((size_t)n);
    RegSummary r;
    r.tiles = n;
    if (mask) r.masked = 0;
    if (fprintf(f, "# %s\n", params.c_str()) < 0) return false;
    for (long j = 0; j < g.ny; ++j)
        for (int i = 0; i < g.nx; ++i) {
            const long t = j * g.nx + i;
            double sc = 0.0;
            if (oip_match_peak(records + (size_t)t * OIP_MATCH_RECORD_WORDS, g.T, g.S, minScore, &dx[t], &dy[t], &sc, &flags[t]) != OIP_OK) return false;
            r.nodata += (flags[t] & OIP_MATCH_NODATA) != 0;
            r.flat += (flags[t] & OIP_MATCH_FLAT) != 0;
            r.edge += (flags[t] & OIP_MATCH_EDGE) != 0;
            r.weak += (flags[t] & OIP_MATCH_WEAK) != 0;
            if (mask) {
                const long fx = (g.originX + g.x0 + (long)i * g.step) * g.scale, fy = (g.originY + g.y0 + j * g.step) * g.scale, side = (long)g.T * g.scale;
                if (oip_mask_tile_flag(mask->flags, mask->gw, mask->gw, mask->gh, mask->cell, fx, fy, side, side, mask->bits)) {
                    flags[t] |= OIP_MATCH_MASKED;
                    ++r.masked;
                }
            }
            const long x = (g.originX + g.x0 + (long)i * g.step + g.T / 2) * g.scale, y = (g.originY + g.y0 + j * g.step + g.T / 2) * g.scale;
            if (fprintf(f, "%ld,%ld,%.4f,%.4f,%.6f,%d\n", x, y, dx[t], dy[t], sc, flags[t]) < 0) return false;
        }
    if (oip_match_summary(dx.data(), dy.data(), flags.data(), n, r.s) != OIP_OK) return false;
    if (fprintf(f, "# %s\n", RegSummaryLine(r).c_str()) < 0) return false;
    if (fprintf(f, "# count,mean_dx,mean_dy,std_dx,std_dy,rms,ce90,max\n# %.0f,%.6f,%.6f,%.6f,%.6f,%.6f,%.6f,%.6f\n", r.s[0], r.s[1], r.s[2], r.s[3],
                r.s[4], r.s[5], r.s[6], r.s[7]) < 0)
        return false;
    *sum = r;
    return true;
}

}  // namespace OIPGPU
