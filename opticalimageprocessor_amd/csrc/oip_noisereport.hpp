// oip_noisereport.hpp -- the report of `oip noise` (<stem>.NOISE.CSV): written from the per-level table and the fit of every
// band, and read back by `oip despike --noise` and `oip denoise --noise`, which need each band's (a, b, mu_ref).  Free of HIP, so
// tests/cpp/noisereport_test.cpp runs it under ASan + UBSan.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "oip_c.h"

namespace OIPGPU {

// what `oip noise` knows of one band: the key histogram's tail counts, oip_noise_levels' table and oip_noise_fit's model
struct NoiseBand {
    uint64_t nodata = 0, structured = 0;
    double sigma[256];
    uint64_t blocks[256];
    int levels = 0;                         // usable levels
    double a = 0.0, b = 0.0, muRef = 0.0;
    NoiseBand()
    {
        for (int l = 0; l < 256; ++l) { sigma[l] = -1.0; blocks[l] = 0; }
    }
    uint64_t realBlocks() const
    {
        uint64_t n = 0;
        for (int l = 0; l < 256; ++l) n += blocks[l];
        return n;
    }
};

// the model of one band as the report holds it
struct NoiseModel {
    int band = 0;                           // 1-based
    double a = 0.0, b = 0.0, muRef = 0.0;
};

// the one line per band that the log and the report share; a, b and mu_ref in %.17g (they read back bit for bit)
inline std::string NoiseBandLine(int band, const NoiseBand &n)
{
    const double sr = std::sqrt(n.a + n.b * n.muRef);
    char buf[512];
    snprintf(buf, sizeof buf, "band %d: blocks %llu nodata %llu structured %llu levels %d a %.17g b %.17g mu_ref %.17g sigma_ref %.6f snr_ref %.4f", band,
             (unsigned long long)n.realBlocks(), (unsigned long long)n.nodata, (unsigned long long)n.structured, n.levels, n.a, n.b, n.muRef, sr,
             sr > 0.0 ? n.muRef / sr : 0.0);
    return buf;
}

// `# params`, one `band,level_lo,level_hi,blocks,sigma,snr` row per usable level and band, then one `# band k: ...` line per
// band.  Returns false where the file cannot be written.
inline bool WriteNoiseReport(FILE *f, const std::string &params, const std::vector<NoiseBand> &bands, int levelShift)
{
    if (fprintf(f, "# %s\n", params.c_str()) < 0) return false;
    for (size_t k = 0; k < bands.size(); ++k)
        for (int l = 0; l < 256; ++l) {
            const double s = bands[k].sigma[l];
            if (!(s >= 0.0)) continue;
            const double mu = ((double)l + 0.5) * (double)(1 << levelShift);
            if (fprintf(f, "%zu,%d,%d,%llu,%.6f,%.4f\n", k + 1, l << levelShift, ((l + 1) << levelShift) - 1, (unsigned long long)bands[k].blocks[l], s,
                        s > 0.0 ? mu / s : 0.0) < 0)
                return false;
        }
    for (size_t k = 0; k < bands.size(); ++k)
        if (fprintf(f, "# %s\n", NoiseBandLine((int)k + 1, bands[k]).c_str()) < 0) return false;
    return true;
}

// The value behind ` name ` in a `# band` line, as a finite double >= 0; false if it is missing or not a number.
inline bool NoiseField(const std::string &line, const char *name, double *out)
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

// The models of a report: every `# band k: ... a A b B mu_ref M ...` line, k = 1, 2, ... in this order (at most 4).  Everything
// else is skipped.  Returns false with a message where the file cannot be read, a line is longer than 4096 bytes, a band line is
// out of order or lacks one of the three numbers, or the report holds no band.
inline bool ParseNoiseReport(const std::string &path, std::vector<NoiseModel> *out, std::string *err)
{
    out->clear();
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) { *err = "open file [" + path + "] failed"; return false; }
    char buf[4098];
    bool ok = true;
    long n = 0;
    while (ok && fgets(buf, sizeof buf, f)) {
        ++n;
        const size_t len = strlen(buf);
        if (len == sizeof buf - 1 && buf[len - 1] != '\n') { *err = "noise report [" + path + "]: line " + std::to_string(n) + " is too long"; ok = false; break; }
        if (strncmp(buf, "# band ", 7) != 0) continue;
        const std::string line(buf);
        char *e = nullptr;
        const long k = strtol(buf + 7, &e, 10);
        NoiseModel m;
        if (e == buf + 7 || *e != ':' || k != (long)out->size() + 1 || k > 4 || !NoiseField(line, "a", &m.a) || !NoiseField(line, "b", &m.b) ||
            !NoiseField(line, "mu_ref", &m.muRef)) {
            *err = "noise report [" + path + "]: line " + std::to_string(n) + " is not a band line of oip noise";
            ok = false;
            break;
        }
        m.band = (int)k;
        out->push_back(m);
    }
    if (ok && ferror(f)) { *err = "read of file [" + path + "] failed"; ok = false; }
    fclose(f);
    if (ok && out->empty()) { *err = "noise report [" + path + "] holds no band"; ok = false; }
    if (!ok) out->clear();
    return ok;
}

// The two threshold parameters `oip despike --noise` uses: each the maximum over the report's bands of
// oip_noise_despike_threshold.  Returns false with the entry point's message where a band's model cannot be used.
inline bool NoiseDespikeThreshold(const std::vector<NoiseModel> &models, double kSigma, int *thrAbs, int *thrRelQ8, std::string *err)
{
    *thrAbs = 0;
    *thrRelQ8 = 0;
    for (const NoiseModel &m : models) {
        int ta = 0, q8 = 0;
        char msg[512] = "";
        if (oip_noise_despike_threshold(m.a, m.b, m.muRef, kSigma, &ta, &q8, msg, sizeof msg) != OIP_OK) {
            *err = "band " + std::to_string(m.band) + ": " + msg;
            return false;
        }
        if (ta > *thrAbs) *thrAbs = ta;
        if (q8 > *thrRelQ8) *thrRelQ8 = q8;
    }
    return !models.empty();
}

// The threshold tables `oip denoise --noise` uses: thr[band][256] from oip_denoise_thresholds(a, b, kSigma), one per band of the
// report, which must hold as many bands as the image has samples per pixel.  Returns false with a message that names both counts,
// or with the entry point's where a band's model cannot be used.
inline bool NoiseDenoiseTables(const std::vector<NoiseModel> &models, int spp, double kSigma, std::vector<uint16_t> *thr, std::string *err)
{
    thr->clear();
    if ((int)models.size() != spp) {
        *err = "holds " + std::to_string(models.size()) + " band" + (models.size() == 1 ? "" : "s") + ", the image has " + std::to_string(spp) +
               " sample" + (spp == 1 ? "" : "s") + " per pixel";
        return false;
    }
    thr->resize((size_t)spp * 256);
    for (int c = 0; c < spp; ++c) {
        char msg[512] = "";
        if (oip_denoise_thresholds(models[c].a, models[c].b, kSigma, thr->data() + (size_t)c * 256, msg, sizeof msg) != OIP_OK) {
            *err = "band " + std::to_string(models[c].band) + ": " + msg;
            thr->clear();
            return false;
        }
    }
    return true;
}

}  // namespace OIPGPU
