// oip_wallisreport.hpp -- the host side of `oip wallis` that needs no device: the report (<stem>.WAL.CSV) made from the nine
// values per channel of oip_wallis_fit, the three counters of oip_wallis_apply_u16 and the options of the run.  Free of HIP, so
// tests/cpp/wallisreport_test.cpp runs it under ASan + UBSan.
#pragma once

#include <cstdint>
#include <cstdio>
#include <string>

#include "oip_c.h"

namespace OIPGPU {

// the names of the nine report values of a channel, in the order of include/oip_c.h
inline const char *const *WallisReportNames()
{
    static const char *const names[9] = {"samples", "mean", "std", "target_mean", "target_std", "nodes", "substituted_nodes", "min_gain_q16", "max_gain_q16"};
    return names;
}

// the names of the three counters
inline const char *const *WallisCounterNames()
{
    static const char *const names[3] = {"transformed_samples", "clamped_low", "clamped_high"};
    return names;
}

// the first line of the report (without its `# `): the image, the raster the filter ran on and every option, doubles in %.17g
inline std::string WallisParamsLine(const std::string &image, int width, long firstLine, long lines, int spp, int block, double contrast, double brightness,
                                    double gMin, double gMax, long minCount, int validMin, int validMax, int maxValue)
{
    char buf[512];
    snprintf(buf, sizeof buf,
             " width=%d line-offset=%ld lines=%ld samples=%d block=%d contrast=%.17g brightness=%.17g min-gain=%.17g max-gain=%.17g min-count=%ld valid-min=%d "
             "valid-max=%d max-value=%d",
             width, firstLine, lines, spp, block, contrast, brightness, gMin, gMax, minCount, validMin, validMax, maxValue);
    return "oip wallis image=" + image + buf;
}

// the one line of figures per channel that the log carries
inline std::string WallisSummaryLine(int channel, const double r[9])
{
    char buf[384];
    snprintf(buf, sizeof buf, "band %d: %.0f samples, mean %.2f std %.2f -> target %.2f / %.2f, %.0f nodes (%.0f substituted), gain %.4f .. %.4f", channel + 1,
             r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7] / 65536.0, r[8] / 65536.0);
    return buf;
}

// `# params`, a header line, a line of nine values per channel (1-based, %.17g), then a `name,value` line per counter.  Returns
// whether every line went out.
inline bool WriteWallisReport(FILE *f, const std::string &params, int spp, const double *report, const uint64_t counts[3])
{
    if (fprintf(f, "# %s\nchannel", params.c_str()) < 0) return false;
    for (int k = 0; k < 9; ++k)
        if (fprintf(f, ",%s", WallisReportNames()[k]) < 0) return false;
    if (fprintf(f, "\n") < 0) return false;
    for (int c = 0; c < spp; ++c) {
        if (fprintf(f, "%d", c + 1) < 0) return false;
        for (int k = 0; k < 9; ++k)
            if (fprintf(f, ",%.17g", report[9 * (size_t)c + k]) < 0) return false;
        if (fprintf(f, "\n") < 0) return false;
    }
    for (int k = 0; k < 3; ++k)
        if (fprintf(f, "%s,%llu\n", WallisCounterNames()[k], (unsigned long long)counts[k]) < 0) return false;
    return true;
}

}  // namespace OIPGPU
