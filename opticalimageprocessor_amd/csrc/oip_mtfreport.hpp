// oip_mtfreport.hpp -- the report of `oip mtf` (<stem>.MTF.CSV): written from the tiles that gave a value and the status counts
// of every band and axis, and read back by `oip mtfc --mtf`, which needs the pooled median / p75 / p90 of either axis.  Free of
// HIP, so tests/cpp/mtfreport_test.cpp runs it under ASan + UBSan.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "oip_c.h"

namespace OIPGPU {

// a tile that gave a value
struct MtfRow {
    int band = 0;                           // 1-based
    int axis = 0;                           // 0 x, 1 y
    long ty = 0, tx = 0;                    // in tiles of the measured line range
    int polarity = 0, slopeQ = 0;           // s and Num of the record: the edge moves Num / 87296 Q7 samples per profile
    long sumS0 = 0;                         // contrast = sumS0 / 32
    double mtf = 0.0;
};

// what `oip mtf` knows of one band and axis, or of all bands of an axis
struct MtfGroup {
    uint64_t tiles = 0, status[8] = {0, 0, 0, 0, 0, 0, 0, 0}, emptybin = 0;   // status[0] counts the EMPTYBIN tiles too
    std::vector<double> values;
    void add(const MtfGroup &g)
    {
        tiles += g.tiles;
        emptybin += g.emptybin;
        for (int k = 0; k < 8; ++k) status[k] += g.status[k];
        values.insert(values.end(), g.values.begin(), g.values.end());
    }
};

// the pooled numbers of one axis as the report holds them
struct MtfAxisSummary {
    bool present = false;                   // the report has an `# all` line for the axis
    uint64_t values = 0;
    double median = 0.0, p75 = 0.0, p90 = 0.0;
};

inline const char *MtfAxisName(int axis) { return axis == 0 ? "x" : "y"; }

// the one line per band and axis (`head` = "band k") or per axis (`head` = "all") that the log and the report share; the three
// statistics in %.17g (they read back bit for bit) and only where there is a value
inline std::string MtfGroupLine(const std::string &head, int axis, const MtfGroup &g)
{
    char buf[768];
    int n = snprintf(buf, sizeof buf, "%s axis %s: tiles %llu ok %llu nodata %llu flat %llu lowcontrast %llu textured %llu offcentre %llu slant %llu curved %llu emptybin %llu values %zu",
                     head.c_str(), MtfAxisName(axis), (unsigned long long)g.tiles, (unsigned long long)g.status[0], (unsigned long long)g.status[1],
                     (unsigned long long)g.status[2], (unsigned long long)g.status[3], (unsigned long long)g.status[4], (unsigned long long)g.status[5],
                     (unsigned long long)g.status[6], (unsigned long long)g.status[7], (unsigned long long)g.emptybin, g.values.size());
    double med = 0.0, p75 = 0.0, p90 = 0.0;
    if (!g.values.empty() && oip_mtf_summary(g.values.data(), (long)g.values.size(), &med, &p75, &p90) == OIP_OK)
        snprintf(buf + n, sizeof buf - (size_t)n, " median %.17g p75 %.17g p90 %.17g", med, p75, p90);
    return buf;
}

// `# params`, one `band,axis,ty,tx,polarity,slope_q,contrast,mtf` row per tile with a value in (band, axis, ty, tx) order, one
// `# band k axis a: ...` line per band and measured axis, one `# all axis a: ...` line per measured axis.  groups[band][axis];
// axes: bit 0 x, bit 1 y.  Returns false where the file cannot be written.
inline bool WriteMtfReport(FILE *f, const std::string &params, std::vector<MtfRow> rows, const std::vector<std::vector<MtfGroup>> &groups, int axes)
{
    if (fprintf(f, "# %s\n", params.c_str()) < 0) return false;
    std::sort(rows.begin(), rows.end(), [](const MtfRow &a, const MtfRow &b) {
        if (a.band != b.band) return a.band < b.band;
        if (a.axis != b.axis) return a.axis < b.axis;
        if (a.ty != b.ty) return a.ty < b.ty;
        return a.tx < b.tx;
    });
    for (const MtfRow &r : rows)
        if (fprintf(f, "%d,%s,%ld,%ld,%d,%d,%.5f,%.17g\n", r.band, MtfAxisName(r.axis), r.ty, r.tx, r.polarity, r.slopeQ, (double)r.sumS0 / 32.0, r.mtf) < 0)
            return false;
    for (size_t k = 0; k < groups.size(); ++k)
        for (int a = 0; a < 2; ++a)
            if ((axes >> a & 1) && fprintf(f, "# %s\n", MtfGroupLine("band " + std::to_string(k + 1), a, groups[k][a]).c_str()) < 0) return false;
    for (int a = 0; a < 2; ++a) {
        if (!(axes >> a & 1)) continue;
        MtfGroup all;
        for (const auto &g : groups) all.add(g[a]);
        if (fprintf(f, "# %s\n", MtfGroupLine("all", a, all).c_str()) < 0) return false;
    }
    return true;
}

// The value behind ` name ` in a summary line, as a finite double >= 0; false if it is missing or not a number.
inline bool MtfField(const std::string &line, const char *name, double *out)
{
    const std::string key = std::string(" ") + name + " ";
    const size_t at = line.find(key);
    if (at == std::string::npos) return false;
    const char *s = line.c_str() + at + key.size();
    char *e = nullptr;
    const double v = strtod(s, &e);
    if (e == s || (*e != '\0' && *e != ' ' && *e != '\n' && *e != '\r') || !std::isfinite(v) || v < 0.0) return false;
    *out = v;
    return true;
}

// The `# all axis x: ...` and `# all axis y: ...` lines of a report into out[0] and out[1]; everything else is skipped.  An
// axis that was not measured stays !present, one without a value has values == 0.  Returns false with a message where the
// file cannot be read, a line is longer than 4096 bytes, an `# all` line names no axis, lacks `values`, lacks one of the
// three statistics while it has values, or comes twice, or the report holds no `# all` line.
inline bool ParseMtfReport(const std::string &path, MtfAxisSummary out[2], std::string *err)
{
    out[0] = out[1] = MtfAxisSummary();
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) { *err = "open file [" + path + "] failed"; return false; }
    char buf[4098];
    bool ok = true;
    long n = 0;
    while (ok && fgets(buf, sizeof buf, f)) {
        ++n;
        const size_t len = strlen(buf);
        if (len == sizeof buf - 1 && buf[len - 1] != '\n') { *err = "MTF report [" + path + "]: line " + std::to_string(n) + " is too long"; ok = false; break; }
        if (strncmp(buf, "# all axis ", 11) != 0) continue;
        const std::string line(buf);
        const int a = buf[11] == 'x' ? 0 : buf[11] == 'y' ? 1 : -1;
        double cnt = 0.0;
        MtfAxisSummary s;
        s.present = true;
        if (a < 0 || buf[12] != ':' || out[a].present || !MtfField(line, "values", &cnt) || cnt != std::floor(cnt) || cnt > 9e15 ||
            (cnt > 0.0 && (!MtfField(line, "median", &s.median) || !MtfField(line, "p75", &s.p75) || !MtfField(line, "p90", &s.p90)))) {
            *err = "MTF report [" + path + "]: line " + std::to_string(n) + " is not a summary line of oip mtf";
            ok = false;
            break;
        }
        s.values = (uint64_t)cnt;
        out[a] = s;
    }
    if (ok && ferror(f)) { *err = "read of file [" + path + "] failed"; ok = false; }
    fclose(f);
    if (ok && !out[0].present && !out[1].present) { *err = "MTF report [" + path + "] holds no summary line"; ok = false; }
    if (!ok) out[0] = out[1] = MtfAxisSummary();
    return ok;
}

// The M of one axis that `oip mtfc --mtf REPORT --mtf-stat median|p75|p90` designs its filter from: the statistic of the pooled
// line, a value above 1 (noise on a very sharp edge) taken as 1.  False with a message where the axis has no value or the value
// is not above 0.
inline bool MtfcValueOf(const MtfAxisSummary &s, int axis, const std::string &stat, double *m, std::string *err)
{
    if (!s.present || s.values == 0) { *err = std::string("no value for axis ") + MtfAxisName(axis); return false; }
    const double v = stat == "p75" ? s.p75 : stat == "p90" ? s.p90 : s.median;
    if (!(v > 0.0)) { *err = std::string("the ") + stat + " of axis " + MtfAxisName(axis) + " is not above 0"; return false; }
    *m = v > 1.0 ? 1.0 : v;
    return true;
}

}  // namespace OIPGPU
