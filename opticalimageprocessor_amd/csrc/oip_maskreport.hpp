// oip_maskreport.hpp -- the host side of `oip mask` that needs no device: the q8 form of a fraction, and the report
// (<stem>.MASK.CSV) made from the eight counters of oip_mask_cells_u16 and oip_mask_morph_u8.  Free of HIP, so
// tests/cpp/maskreport_test.cpp runs it under ASan + UBSan.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

#include "oip_c.h"

namespace OIPGPU {

// the q8 parameter of a fraction F in 0..1: rint(256 F) in fp64, ties to even (the default rounding mode)
inline int MaskQ8(double F) { return (int)std::nearbyint(256.0 * F); }

// the names of the eight counters, in the order of include/oip_c.h
inline const char *const *MaskCounterNames()
{
    static const char *const names[8] = {"cells", "nodata_cells", "saturated_cells", "tested_cells", "candidate_cells", "cloud_cells", "buffer_cells",
                                         "saturated_pixels"};
    return names;
}

// the first line of the report (without its `# `): the image, its size and every parameter of the run; band: 0-based channels
inline std::string MaskParamsLine(const std::string &image, int cell, int width, long height, int bits, int saturation, int validMin, const int band[4],
                                  const int q8[4], int open, int buffer)
{
    char buf[384];
    snprintf(buf, sizeof buf, " cell=%d width=%d height=%ld bits=%d saturation=%d valid-min=%d bands=%d,%d,%d,%d bright-q8=%d white-q8=%d hot-q8=%d ndvi-q8=%d open=%d buffer=%d",
             cell, width, height, bits, saturation, validMin, band[0] + 1, band[1] + 1, band[2] + 1, band[3] + 1, q8[0], q8[1], q8[2], q8[3], open, buffer);
    return "oip mask image=" + image + buf;
}

// the four shares of the report, each 100 * count / cells in fp64 (0 for an empty grid)
struct MaskShares {
    double nodata = 0.0, saturated = 0.0, cloud = 0.0, cloudOrBuffer = 0.0;
};
inline MaskShares MaskPercent(const uint64_t counts[8])
{
    MaskShares s;
    if (counts[0] == 0) return s;
    const double cells = (double)counts[0];
    s.nodata = 100.0 * (double)counts[1] / cells;
    s.saturated = 100.0 * (double)counts[2] / cells;
    s.cloud = 100.0 * (double)counts[5] / cells;
    s.cloudOrBuffer = 100.0 * (double)(counts[5] + counts[6]) / cells;
    return s;
}

// the one line of figures that the log carries
inline std::string MaskSummaryLine(const uint64_t counts[8])
{
    const MaskShares s = MaskPercent(counts);
    char buf[512];
    snprintf(buf, sizeof buf,
             "cells %llu, nodata %llu (%.4f %%), saturated %llu (%.4f %%, %llu pixels), tested %llu, candidate %llu, cloud %llu (%.4f %%), buffer %llu "
             "(cloud or buffer %.4f %%)",
             (unsigned long long)counts[0], (unsigned long long)counts[1], s.nodata, (unsigned long long)counts[2], s.saturated, (unsigned long long)counts[7],
             (unsigned long long)counts[3], (unsigned long long)counts[4], (unsigned long long)counts[5], s.cloud, (unsigned long long)counts[6],
             s.cloudOrBuffer);
    return buf;
}

// `# params`, a `name,value` line per counter, then the four shares with %.4f.  Returns whether every line went out.
inline bool WriteMaskReport(FILE *f, const std::string &params, const uint64_t counts[8])
{
    if (fprintf(f, "# %s\n", params.c_str()) < 0) return false;
    for (int k = 0; k < 8; ++k)
        if (fprintf(f, "%s,%llu\n", MaskCounterNames()[k], (unsigned long long)counts[k]) < 0) return false;
    const MaskShares s = MaskPercent(counts);
    return fprintf(f, "nodata_pct,%.4f\nsaturated_pct,%.4f\ncloud_pct,%.4f\ncloud_or_buffer_pct,%.4f\n", s.nodata, s.saturated, s.cloud, s.cloudOrBuffer) >= 0;
}

}  // namespace OIPGPU
