// host.cpp -- host-side pieces of the path that carry no raster arithmetic:
// the RRC parameter file loader, its counterpart (column fit + writer), the seam fits of `oip stitch --balance` (per strip, per
// block of lines, and the per-line tables), the shift
// filtering / polynomial fit, the contrast stretch of `oip quicklook` (percentile limits, 8-bit table, 8-bit TIFF) and the
// taps of `oip mtfc` (design, quantisation, kernel file), the column lists and column table of `oip despike`, the field of
// `oip regfix` (report, fill, smoothing: oip_warpfield.hpp), the geometry rule of `oip pansharpen`, the noise model of `oip noise`
// and the tile value, order statistics and slack of `oip mtf`.
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "oip_c.h"
#include "oip_corrroute.h"
#include "oip_fftplan.h"
#include "oip_rescaleplan.h"
#include "oip_tiff.hpp"
#include "oip_warpfield.hpp"

// IMO::LoadRRCParamFile (imageop.h:140-192): three header lines (only the second -- the
// column count -- is checked outside DEBUG builds), then one "k , b" row per column parsed
// with sscanf(" %lf , %lf") from a 1024-byte fgets buffer; the row count must match exactly
// and any unparsable line (a trailing blank one included) is an error.  errno_error maps to
// OIP_E_IO, std::runtime_error to OIP_E_RUNTIME.
extern "C" int oip_load_rrc_param_file(const char *path, int expected_lines, double *kb_out, char *err, int errlen)
{
    auto fail = [&](int code, const char *fmt, auto... a) {
        if (err && errlen > 0) snprintf(err, errlen, fmt, a...);
        return code;
    };
    if (!path || expected_lines <= 0 || !kb_out) return fail(OIP_E_INVALID, "%s", "oip_load_rrc_param_file: bad argument");
    FILE *f = fopen(path, "rb");
    if (!f) return fail(OIP_E_IO, "%s", "open RRC Param file failed");
    const int bn = 1024;
    char buff[bn];
    if (!fgets(buff, bn, f)) { fclose(f); return fail(OIP_E_IO, "%s", "LoadRRCParamFile([1]): read file content failed"); }
    if (!fgets(buff, bn, f)) { fclose(f); return fail(OIP_E_IO, "%s", "LoadRRCParamFile([2]): read file content failed"); }
    int lines = atoi(buff);
    if (lines != expected_lines) {
        fclose(f);
        return fail(OIP_E_RUNTIME, "LoadRRCParamFile([2]): expected %d lines while %d found in file content", expected_lines, lines);
    }
    if (!fgets(buff, bn, f)) { fclose(f); return fail(OIP_E_IO, "%s", "LoadRRCParamFile([3]): read file content failed"); }
    int index = 0;
    double k = .0, b = .0;
    for (; fgets(buff, bn, f); ++index) {
        if (sscanf(buff, " %lf , %lf", &k, &b) != 2) {
            fclose(f);
            return fail(OIP_E_RUNTIME, "line #%d of RRC param file [%s] found invalid", index, path);
        }
        if (index < expected_lines) {   // the reference overruns its array here; we only count
            kb_out[2 * index] = k;
            kb_out[2 * index + 1] = b;
        }
    }
    fclose(f);
    if (index != expected_lines)
        return fail(OIP_E_RUNTIME, "RRC Param file [%s] invalid: %d lines of param expected, %d lines parsed.", path, expected_lines, index);
    return OIP_OK;
}

// Is column x of the totals usable for the fit?  The ONE statement of the rule: oip_rrc_fit_columns fits the columns it
// accepts, oip_rrc_dead_columns lists the ones it refuses.  D (may be NULL) receives n*S2 - S1*S1 of a usable column in
// moments mode.
static bool rrc_column_usable(const uint64_t *acc, int w, int x, bool moments, uint64_t min_count, unsigned __int128 *D)
{
    const uint64_t need = min_count > (moments ? 2u : 1u) ? min_count : (moments ? 2u : 1u);
    const uint64_t n = acc[x], S1 = acc[(size_t)w + x], S2 = acc[2 * (size_t)w + x];
    if (n < need) return false;
    if (!moments) return S1 != 0;
    const unsigned __int128 a = (unsigned __int128)n * S2, b = (unsigned __int128)S1 * S1;
    if (a <= b) return false;                                      // D == 0: a constant column (a < b cannot come from real totals)
    if (D) *D = a - b;
    return true;
}

// Moment matching on the per-column totals of oip_colstats_u16 (include/oip_c.h states the operation order; a Python
// restatement in tests/_colstats_ref.py follows it step by step).  Every step is one correctly rounded fp64
// operation: the 128-bit D converts to the nearest double, S1 < 2^47 and n < 2^53 convert exactly.
extern "C" int oip_rrc_fit_columns(const uint64_t *acc, int w, int groups, int mode, uint64_t min_count, double *kb_out, int *dead_out,
                                   double *ref_out, char *err, int errlen)
{
    auto fail = [&](int code, const char *fmt, auto... a) {
        if (err && errlen > 0) snprintf(err, errlen, fmt, a...);
        return code;
    };
    if (!acc || !kb_out || w <= 0 || groups <= 0 || w % groups != 0 || (mode != OIP_RRCFIT_MOMENTS && mode != OIP_RRCFIT_GAIN))
        return fail(OIP_E_INVALID, "%s", "oip_rrc_fit_columns: bad argument");
    const bool moments = mode == OIP_RRCFIT_MOMENTS;
    const int gw = w / groups;
    const uint64_t *N = acc, *S1 = acc + w;
    std::vector<double> mu(gw), sigma(gw);
    std::vector<char> usable(gw);
    for (int g = 0; g < groups; ++g) {
        double muSum = 0.0, sigmaSum = 0.0;
        int count = 0;
        for (int i = 0; i < gw; ++i) {
            const int x = g * gw + i;
            unsigned __int128 D = 0;
            usable[i] = rrc_column_usable(acc, w, x, moments, min_count, &D);
            if (!usable[i]) continue;
            mu[i] = (double)S1[x] / (double)N[x];
            if (moments) {
                sigma[i] = std::sqrt((double)D) / (double)N[x];
                sigmaSum += sigma[i];
            }
            muSum += mu[i];
            ++count;
        }
        if (count == 0) return fail(OIP_E_RUNTIME, "oip_rrc_fit_columns: group %d has no usable column", g);
        const double muRef = muSum / (double)count, sigmaRef = moments ? sigmaSum / (double)count : 0.0;
        for (int i = 0; i < gw; ++i) {
            double k = 1.0, b = 0.0;
            if (usable[i]) {
                if (moments) {
                    k = sigmaRef / sigma[i];
                    const double km = k * mu[i];
                    b = muRef - km;
                } else {
                    k = muRef / mu[i];
                }
            }
            kb_out[2 * (size_t)(g * gw + i)] = k;
            kb_out[2 * (size_t)(g * gw + i) + 1] = b;
        }
        if (dead_out) dead_out[g] = gw - count;
        if (ref_out) { ref_out[2 * g] = muRef; ref_out[2 * g + 1] = sigmaRef; }
    }
    return OIP_OK;
}

extern "C" int oip_rrc_dead_columns(const uint64_t *acc, int w, int mode, uint64_t min_count, int *cols, int *n)
{
    if (!acc || !cols || !n || w <= 0 || (mode != OIP_RRCFIT_MOMENTS && mode != OIP_RRCFIT_GAIN)) return OIP_E_INVALID;
    int k = 0;
    for (int x = 0; x < w; ++x)
        if (!rrc_column_usable(acc, w, x, mode == OIP_RRCFIT_MOMENTS, min_count, nullptr)) cols[k++] = x;
    *n = k;
    return OIP_OK;
}

// Gain and offset of image 2 relative to image 1 from the overlap totals of oip_seam_moments_u16 (include/oip_c.h states
// the operation order; tests/_seam_ref.py restates it).  n <= 2^32 and Sa, Sb < 2^48 convert exactly; Saa, Sbb, Sab < 2^64
// enter only through the exact 128-bit D's, which convert to the nearest double.
// The ONE statement of the arithmetic, for one channel: oip_seam_fit runs it on a strip's totals, oip_seam_fit_blocks on the
// sum of the blocks' and on each block's.  t: n, Sa, Sb, Saa, Sbb, Sab.  rep (may be NULL): 6 doubles.  G, O: the rounded
// values as doubles, in range or not (the identity when the result is SEAM_FIT_IDENTITY).
enum SeamFitResult { SEAM_FIT_OK, SEAM_FIT_IDENTITY, SEAM_FIT_GAIN_RANGE, SEAM_FIT_OFFSET_RANGE };
static SeamFitResult seam_fit_channel(const uint64_t t[6], int mode, uint64_t need, double *rep, double *Gout, double *Oout)
{
    const uint64_t n = t[0], Sa = t[1], Sb = t[2], Saa = t[3], Sbb = t[4], Sab = t[5];
    // (a D below zero cannot come from real totals; it is treated as 0)
    const unsigned __int128 na = (unsigned __int128)n * Saa, sa2 = (unsigned __int128)Sa * Sa;
    const unsigned __int128 nb = (unsigned __int128)n * Sbb, sb2 = (unsigned __int128)Sb * Sb;
    const unsigned __int128 Da = na > sa2 ? na - sa2 : 0, Db = nb > sb2 ? nb - sb2 : 0;
    const __int128 Dab = (__int128)((unsigned __int128)n * Sab) - (__int128)((unsigned __int128)Sa * Sb);
    double meanA = 0.0, meanB = 0.0, sigmaA = 0.0, sigmaB = 0.0, r = 0.0;
    if (n > 0) {
        const double nd = (double)n;
        meanA = (double)Sa / nd;
        meanB = (double)Sb / nd;
        const double ra = std::sqrt((double)Da), rb = std::sqrt((double)Db);
        sigmaA = ra / nd;
        sigmaB = rb / nd;
        if (Da != 0 && Db != 0) {
            const double den = ra * rb;
            r = (double)Dab / den;
        }
    }
    if (rep) { rep[0] = (double)n; rep[1] = meanA; rep[2] = meanB; rep[3] = sigmaA; rep[4] = sigmaB; rep[5] = r; }
    *Gout = 65536.0;
    *Oout = 0.0;
    if (n < need) return SEAM_FIT_IDENTITY;
    double g = 1.0;
    if (mode == OIP_SEAM_MOMENTS) {
        if (Da == 0 || Db == 0) return SEAM_FIT_IDENTITY;
        const double q = (double)Da / (double)Db;
        g = std::sqrt(q);
    } else if (mode == OIP_SEAM_GAIN) {
        if (Sb == 0) return SEAM_FIT_IDENTITY;
        g = (double)Sa / (double)Sb;
    }
    const double G = std::rint(g * 65536.0);
    *Gout = G;
    if (!(G >= 16384.0 && G <= 262144.0)) return SEAM_FIT_GAIN_RANGE;
    double O = 0.0;
    if (mode != OIP_SEAM_GAIN) {
        const double gq = G / 65536.0;
        const double tt = gq * meanB;
        const double d = meanA - tt;
        O = std::rint(d * 65536.0);
        *Oout = O;
        if (!(O >= -2147483648.0 && O <= 2147483647.0)) return SEAM_FIT_OFFSET_RANGE;
    }
    return SEAM_FIT_OK;
}

static bool seam_mode_ok(int mode) { return mode == OIP_SEAM_MOMENTS || mode == OIP_SEAM_GAIN || mode == OIP_SEAM_OFFSET; }

extern "C" int oip_seam_fit(const uint64_t *acc, int spp, int mode, uint64_t min_count, int32_t *gain_q16, int32_t *offset_q16, double *report,
                            int *identity, char *err, int errlen)
{
    auto fail = [&](int code, const char *fmt, auto... a) {
        if (err && errlen > 0) snprintf(err, errlen, fmt, a...);
        return code;
    };
    if (!acc || !gain_q16 || !offset_q16 || !identity || spp <= 0 || !seam_mode_ok(mode))
        return fail(OIP_E_INVALID, "%s", "oip_seam_fit: bad argument");
    const uint64_t need = min_count > 2u ? min_count : 2u;
    for (int c = 0; c < spp; ++c) {
        const uint64_t t[6] = {acc[c], acc[spp + c], acc[2 * spp + c], acc[3 * spp + c], acc[4 * spp + c], acc[5 * spp + c]};
        double G = 0.0, O = 0.0;
        const SeamFitResult res = seam_fit_channel(t, mode, need, report ? report + 6 * (size_t)c : nullptr, &G, &O);
        gain_q16[c] = 65536;
        offset_q16[c] = 0;
        identity[c] = 1;
        if (res == SEAM_FIT_IDENTITY) continue;
        if (res == SEAM_FIT_GAIN_RANGE)
            return fail(OIP_E_INVALID, "oip_seam_fit: channel %d: gain_q16 %.0f outside [16384, 262144] -- the overlaps do not show the same ground (--fold-cols?)", c, G);
        if (res == SEAM_FIT_OFFSET_RANGE) return fail(OIP_E_INVALID, "oip_seam_fit: channel %d: offset_q16 %.0f does not fit 32 bits", c, O);
        gain_q16[c] = (int32_t)G;
        offset_q16[c] = (int32_t)O;
        identity[c] = 0;
    }
    return OIP_OK;
}

// A fit per block of lines from the (nb, 6, spp) totals of oip_seam_moments_blocks_u16 (include/oip_c.h).  The whole-strip
// fit on the sum of the planes is oip_seam_fit itself, errors and texts included; a block channel whose own fit is the
// identity or out of range takes the strip's pair and is flagged -- a block of zero-filled lines, water or cloud is no error.
extern "C" int oip_seam_fit_blocks(const uint64_t *acc, long nb, int spp, int mode, uint64_t min_count, int32_t *gain_q16, int32_t *offset_q16,
                                   int *substituted, int32_t *gain0_q16, int32_t *offset0_q16, int *identity0, double *report, char *err,
                                   int errlen)
{
    auto fail = [&](int code, const char *fmt, auto... a) {
        if (err && errlen > 0) snprintf(err, errlen, fmt, a...);
        return code;
    };
    if (!acc || !gain_q16 || !offset_q16 || !substituted || !gain0_q16 || !offset0_q16 || !identity0 || nb < 1 || spp <= 0 || !seam_mode_ok(mode))
        return fail(OIP_E_INVALID, "%s", "oip_seam_fit_blocks: bad argument");
    const size_t plane = 6 * (size_t)spp;
    std::vector<uint64_t> sum(plane, 0);
    for (long k = 0; k < nb; ++k)
        for (size_t i = 0; i < plane; ++i) sum[i] += acc[(size_t)k * plane + i];
    const int rc = oip_seam_fit(sum.data(), spp, mode, min_count, gain0_q16, offset0_q16, nullptr, identity0, err, errlen);
    if (rc != OIP_OK) return rc;
    const uint64_t need = min_count > 2u ? min_count : 2u;
    for (long k = 0; k < nb; ++k)
        for (int c = 0; c < spp; ++c) {
            const uint64_t *a = acc + (size_t)k * plane;
            const uint64_t t[6] = {a[c], a[spp + c], a[2 * spp + c], a[3 * spp + c], a[4 * spp + c], a[5 * spp + c]};
            double G = 0.0, O = 0.0;
            const size_t e = (size_t)k * spp + c;
            const bool own = seam_fit_channel(t, mode, need, report ? report + 6 * e : nullptr, &G, &O) == SEAM_FIT_OK;
            gain_q16[e] = own ? (int32_t)G : gain0_q16[c];
            offset_q16[e] = own ? (int32_t)O : offset0_q16[c];
            substituted[e] = own ? 0 : 1;
        }
    return OIP_OK;
}

// The block values as nodes at the blocks' nominal centres, interpolated to one value per line and channel in 64-bit
// integers (include/oip_c.h).  The division floors toward minus infinity: offsets are negative as often as not.
extern "C" int oip_seam_line_tables(const int32_t *gain_q16, const int32_t *offset_q16, long nb, int spp, long L, long block_lines,
                                    int32_t *line_gain_q16, int32_t *line_offset_q16)
{
    if (!gain_q16 || !offset_q16 || spp <= 0 || L < 0 || L >= (1L << 31) || block_lines < 1 || nb != (L / block_lines > 1 ? L / block_lines : 1) ||
        (L > 0 && (!line_gain_q16 || !line_offset_q16)))
        return OIP_E_INVALID;
    const long B = block_lines, half = B / 2;
    auto floordiv = [](long long a, long long b) { return a / b - ((a % b != 0 && a < 0) ? 1 : 0); };      // b > 0
    for (long r = 0; r < L; ++r) {
        long k = 0, k1 = 0, t = 0;
        if (nb > 1) {                              // (B <= L < 2^31 here: |V| * B < 2^62)
            const long u = r - half;
            k = u < 0 ? 0 : u / B;
            if (k > nb - 2) k = nb - 2;
            t = u - k * B;
            t = t < 0 ? 0 : (t > B ? B : t);
            k1 = k + 1;
        }
        for (int c = 0; c < spp; ++c) {
            const size_t e = (size_t)r * spp + c;
            if (nb == 1) {                         // one node: constant (the formula's value, without B in the products)
                line_gain_q16[e] = gain_q16[c];
                line_offset_q16[e] = offset_q16[c];
                continue;
            }
            const long long g0 = gain_q16[k * spp + c], g1 = gain_q16[k1 * spp + c], o0 = offset_q16[k * spp + c], o1 = offset_q16[k1 * spp + c];
            line_gain_q16[e] = (int32_t)floordiv(g0 * (B - t) + g1 * t + half, B);
            line_offset_q16[e] = (int32_t)floordiv(o0 * (B - t) + o1 * t + half, B);
        }
    }
    return OIP_OK;
}

// The writer for IMO::LoadRRCParamFile's format (imageop.h:148-188; oip_load_rrc_param_file above reads it back).
extern "C" int oip_write_rrc_param_file(const char *path, const double *kb, int n, char *err, int errlen)
{
    auto fail = [&](int code, const char *fmt, auto... a) {
        if (err && errlen > 0) snprintf(err, errlen, fmt, a...);
        return code;
    };
    if (!path || !kb || n <= 0) return fail(OIP_E_INVALID, "%s", "oip_write_rrc_param_file: bad argument");
    FILE *f = fopen(path, "wb");
    if (!f) return fail(OIP_E_IO, "open RRC Param file [%s] for writing failed: %s", path, strerror(errno));
    bool ok = fprintf(f, "1\n%d\n0\n", n) > 0;
    for (int i = 0; i < n && ok; ++i) ok = fprintf(f, "%.17g , %.17g\n", kb[2 * (size_t)i], kb[2 * (size_t)i + 1]) > 0;
    if (fclose(f) != 0) ok = false;
    if (!ok) return fail(OIP_E_IO, "write of RRC Param file [%s] failed: %s", path, strerror(errno));
    return OIP_OK;
}

// Least-squares polynomial, coefficients in ascending order, solved WELL: Householder QR on the
// abscissa centred and scaled to [-1,1], then the coefficients are expanded back to powers of x --
// the exact least-squares solution to fp64 accuracy (OIP_FIT_LSTSQ).  This is NOT what the reference
// computes (see oip_polyfit_reference below); it is offered as `--fit lstsq`.  Every rank calls this
// with identical inputs and gets identical bits (single thread, fixed order).
extern "C" int oip_polyfit(const double *x, const double *y, int n, int deg, double *coeffs)
{
    if (!x || !y || !coeffs || deg < 0 || deg > 8 || n <= deg) return OIP_E_INVALID;
    const int m = deg + 1;
    double mu = 0.0;
    for (int i = 0; i < n; ++i) mu += x[i];
    mu /= n;
    double sc = 0.0;
    for (int i = 0; i < n; ++i) sc = std::fmax(sc, std::fabs(x[i] - mu));
    if (sc == 0.0) sc = 1.0;
    std::vector<double> A((size_t)n * m), rhs(y, y + n);
    for (int i = 0; i < n; ++i) {
        double t = (x[i] - mu) / sc, p = 1.0;
        for (int j = 0; j < m; ++j) { A[(size_t)i * m + j] = p; p *= t; }
    }
    // Householder QR, applied to rhs on the fly
    for (int j = 0; j < m; ++j) {
        double norm = 0.0;
        for (int i = j; i < n; ++i) norm += A[(size_t)i * m + j] * A[(size_t)i * m + j];
        norm = std::sqrt(norm);
        if (norm == 0.0) return OIP_E_RUNTIME;
        double alpha = A[(size_t)j * m + j] > 0 ? -norm : norm;
        std::vector<double> v(n - j);
        for (int i = j; i < n; ++i) v[i - j] = A[(size_t)i * m + j];
        v[0] -= alpha;
        double vnorm2 = 0.0;
        for (double e : v) vnorm2 += e * e;
        if (vnorm2 == 0.0) continue;
        for (int c = j; c < m; ++c) {
            double dot = 0.0;
            for (int i = j; i < n; ++i) dot += v[i - j] * A[(size_t)i * m + c];
            double f = 2.0 * dot / vnorm2;
            for (int i = j; i < n; ++i) A[(size_t)i * m + c] -= f * v[i - j];
        }
        double dot = 0.0;
        for (int i = j; i < n; ++i) dot += v[i - j] * rhs[i];
        double f = 2.0 * dot / vnorm2;
        for (int i = j; i < n; ++i) rhs[i] -= f * v[i - j];
    }
    std::vector<double> c(m);
    for (int j = m - 1; j >= 0; --j) {
        double s = rhs[j];
        for (int k = j + 1; k < m; ++k) s -= A[(size_t)j * m + k] * c[k];
        double d = A[(size_t)j * m + j];
        if (d == 0.0) return OIP_E_RUNTIME;
        c[j] = s / d;
    }
    // sum_j c_j ((x-mu)/sc)^j  ->  ascending powers of x
    std::vector<double> p(m, 0.0);
    for (int j = 0; j < m; ++j) {
        double binom = 1.0;                       // C(j, i)
        double scj = std::pow(sc, j);
        for (int i = 0; i <= j; ++i) {
            if (i > 0) binom = binom * (j - i + 1) / i;
            p[i] += c[j] * binom * std::pow(-mu, j - i) / scj;
        }
    }
    for (int j = 0; j < m; ++j) coeffs[j] = p[j];
    return OIP_OK;
}

// nc::polynomial::Poly1d<double>::fit(x, y, deg) as the reference calls it (preproc.h:535-536), restated
// from NumCpp (un-vendored, version unpinned: PARITY UNPINNED):
//   A[i][j] = x_i^j by repeated multiplication (utils::power), raw abscissa;
//   non-square A:  aInv = inv(A^T A) . A^T ;  coefficients = aInv . y
//   NdArray::dot = one std::inner_product per element (k ascending, starting from 0);
//   linalg::inv  = in-place Gauss-Jordan sweep over the diagonal without pivoting (rows are only
//                  swapped for exactly-zero diagonal entries, which cannot occur for A^T A here).
// At cx up to 12288..30000 and degree 2 cond(A^T A) is 1e16..1e18, so the low digits of the result
// are set by this very operation order -- which is why it is reproduced operation by operation
// instead of being replaced by a better-conditioned solver: the product's default (OIP_FIT_REFERENCE)
// must give the maps the reference gives.  No FMA (the library is built -ffp-contract=off, like the
// reference's x86-64 build).
extern "C" int oip_polyfit_reference(const double *x, const double *y, int n, int deg, double *coeffs)
{
    if (!x || !y || !coeffs || deg < 0 || deg > 8 || n <= deg) return OIP_E_INVALID;
    const int m = deg + 1;
    std::vector<double> A((size_t)n * m);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < m; ++j) {
            double v = 1.0;
            if (j > 0) { v = x[i]; for (int e = 1; e < j; ++e) v *= x[i]; }
            A[(size_t)i * m + j] = v;
        }
    // aT.dot(a)
    std::vector<double> G((size_t)m * m), R((size_t)m * m);
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) {
            double acc = 0.0;
            for (int k = 0; k < n; ++k) acc = acc + A[(size_t)k * m + i] * A[(size_t)k * m + j];
            G[(size_t)i * m + j] = acc;
        }
    // linalg::inv: sweep k = 0..m-1, each sweep builds `result` from the current matrix and replaces it
    for (int k = 0; k < m; ++k) {
        if (G[(size_t)k * m + k] == 0.0) return OIP_E_RUNTIME;      // degenerate abscissae
        R[(size_t)k * m + k] = -1.0 / G[(size_t)k * m + k];
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < m; ++j) {
                if (i != k && j != k) R[(size_t)i * m + j] = G[(size_t)i * m + j] + G[(size_t)k * m + j] * G[(size_t)i * m + k] * R[(size_t)k * m + k];
                else if (i != k && j == k) R[(size_t)i * m + k] = G[(size_t)i * m + k] * R[(size_t)k * m + k];
                else if (i == k && j != k) R[(size_t)k * m + j] = G[(size_t)k * m + j] * R[(size_t)k * m + k];
            }
        G = R;
    }
    for (double &v : R) v *= -1.0;
    // aTaInv.dot(aT), then .dot(y)
    std::vector<double> P((size_t)m * n);
    for (int i = 0; i < m; ++i)
        for (int c = 0; c < n; ++c) {
            double acc = 0.0;
            for (int k = 0; k < m; ++k) acc = acc + R[(size_t)i * m + k] * A[(size_t)c * m + k];
            P[(size_t)i * n + c] = acc;
        }
    for (int i = 0; i < m; ++i) {
        double acc = 0.0;
        for (int c = 0; c < n; ++c) acc = acc + P[(size_t)i * n + c] * y[c];
        if (!(acc == acc) || std::isinf(acc)) return OIP_E_RUNTIME;
        coeffs[i] = acc;
    }
    return OIP_OK;
}

// FilterInterBandShiftValues (preproc.h:492-512) + DoCorrelationPolynomialFitting
// (preproc.h:514-550): per band keep the shifts whose response reaches the threshold,
// require at least min_count of them, fit dx(cx) with degree 1 and dy(cx) with degree 2.
extern "C" int oip_filter_and_fit_mode(const double *shifts, int n, double threshold, int min_count, int fit_mode,
                                       double *cx_out, double *cy_out, char *err, int errlen)
{
    if (!shifts || n <= 0 || !cx_out || !cy_out || (fit_mode != OIP_FIT_REFERENCE && fit_mode != OIP_FIT_LSTSQ)) return OIP_E_INVALID;
    auto fit = fit_mode == OIP_FIT_LSTSQ ? oip_polyfit : oip_polyfit_reference;
    std::vector<double> cxv(n), xv(n), yv(n);
    for (int b = 0; b < OIP_MSS_BANDS; ++b) {
        // Two tests, as the reference has them: FilterInterBandShiftValues counts a unit unless `rs < threshold`
        // (preproc.h:498-503) -- a NaN response, which the f32 cross-power spectrum produces when |P|^2 overflows, is
        // not below the threshold and counts towards min_count -- while DoCorrelationPolynomialFitting takes a unit
        // into the fit when `rs >= threshold` (preproc.h:527), which a NaN fails.
        int vvi = 0, fc = 0;
        for (int i = 0; i < n; ++i) {
            const double *s = shifts + ((size_t)b * n + i) * 4;
            if (!(s[2] < threshold)) ++fc;
            if (s[2] >= threshold) {
                cxv[vvi] = s[3];
                xv[vvi] = s[0];
                yv[vvi] = s[1];
                ++vvi;
            }
        }
        if (fc < min_count) {
            if (err && errlen > 0)
                snprintf(err, errlen, "Not enough valid correlation values for band#%d: %d valid values found, %d expected at least",
                         b + 1, fc, min_count);
            return OIP_E_RUNTIME;
        }
        int rc = fit(cxv.data(), xv.data(), vvi, 1, cx_out + b * 2);
        if (rc == OIP_OK) rc = fit(cxv.data(), yv.data(), vvi, 2, cy_out + b * 3);
        if (rc != OIP_OK) {
            if (err && errlen > 0) snprintf(err, errlen, "polynomial fit failed for band#%d (degenerate abscissae)", b + 1);
            return OIP_E_RUNTIME;
        }
    }
    return OIP_OK;
}

extern "C" int oip_filter_and_fit(const double *shifts, int n, double threshold, int min_count, double *cx_out,
                                  double *cy_out, char *err, int errlen)
{
    return oip_filter_and_fit_mode(shifts, n, threshold, min_count, OIP_FIT_REFERENCE, cx_out, cy_out, err, errlen);
}

// The accumulation of Stitcher::CalcSttParameters (stitcher.h:181-198): sections in order, a section is
// valid when resp >= threshold and (max_delta_y <= 0 or |dy| <= max_delta_y); arithmetic means in fp64.
// NaN rows (sections no rank computed) fail the comparison like any low response.  Every rank of a
// multi-GPU run calls this on the all-gathered table and gets identical bits.
extern "C" int oip_stt_mean(const double *table, int sections, double threshold, double max_delta_y, double *dx,
                            double *dy, double *response, int *valid_out)
{
    if (!table || sections <= 0) return OIP_E_INVALID;
    double sx = 0.0, sy = 0.0, sr = 0.0;
    int valid = 0;
    for (int i = 0; i < sections; ++i) {
        const double x = table[3 * i], y = table[3 * i + 1], r = table[3 * i + 2];
        const bool ok = r >= threshold && (max_delta_y <= 0.0 || std::fabs(y) <= max_delta_y);
        if (ok) { sx += x; sy += y; sr += r; ++valid; }
    }
    if (valid_out) *valid_out = valid;
    if (valid == 0) return OIP_E_RUNTIME;       // "No valid delta value found for stitching parameter calculating"
    if (dx) *dx = sx / valid;
    if (dy) *dy = sy / valid;
    if (response) *response = sr / valid;
    return OIP_OK;
}

// cv::resize(INTER_CUBIC) by exactly 4 along one axis as an operator on spectra: with R = C + E the
// n -> N = 4 n up-sampling matrix (C circulant: zero-stuff, convolve with the 16-tap kernel h; E: what clamping instead
// of wrapping the out-of-image taps adds, non-zero in columns J = {0, 1, n-2, n-1} only),
//     DFT_N(R s)[k] = H[k] DFT_n(s)[k mod n] + sum_j G_j[k] s[J_j],     H = DFT_N(h), G_j = DFT_N(E[:, J_j]).
// out[(t * N + k) * 2 + {0,1}] = re, im of H (t = 0) and G_0..G_3 (t = 1..4), as float.  Built in double from the f32
// taps of cv::hal::resize's coefficient set-up (fx = (float)((d + 0.5) * scale - 0.5), interpolateCubic(fx - floor)),
// the same the image-domain kernels apply.  OIP_E_UNSUPPORTED when the taps are not 4-periodic or n < 8.
// ---- the plan of an M x N transform, stated by the planner itself (include/oip_c.h; arithmetic: oip_fftplan.h)
static_assert(oipfftplan::kPlanOk == OIP_OK && oipfftplan::kPlanInvalid == OIP_E_INVALID && oipfftplan::kPlanRuntime == OIP_E_RUNTIME &&
              oipfftplan::kPlanUnsupported == OIP_E_UNSUPPORTED, "the planner's codes are the C interface's");
extern "C" int oip_fft_plan_describe(int M, int N, char *buf, int len)
{
    if (!buf || len < 1) return OIP_E_INVALID;
    return oipfftplan::describe(M, N, buf, (size_t)len);
}

// ---- the route and storage of an inter-band correlation call, stated by its planner (include/oip_c.h; arithmetic: oip_corrroute.h)
extern "C" int oip_corr_route_describe(int rows, int cols, int cu_count, char *buf, int len)
{
    if (!buf || len < 1) return OIP_E_INVALID;
    buf[0] = 0;
    if (rows < OIP_MSS_BANDS || cols < OIP_MSS_BANDS || cu_count < 1) return OIP_E_INVALID;
    oipcorr::CorrPlan plan;
    char why[160] = "";
    const int rc = oipcorr::plan_interband(rows, cols, rows / OIP_MSS_BANDS, cols / OIP_MSS_BANDS, cu_count, oipcorr::CorrKnobs::from_env(), &plan, why, sizeof why);
    const std::string s = oipcorr::describe(plan, rc, why);
    if (s.size() >= (size_t)len) return OIP_E_INVALID;
    memcpy(buf, s.c_str(), s.size() + 1);
    return rc;
}

extern "C" int oip_upsample_operator(int n, float *out)
{
    if (n < 8 || !out) return OIP_E_UNSUPPORTED;
    const int N = 4 * n;
    const double scale = 1. / ((double)N / n);
    std::vector<double> h(N, 0.0), g[4];
    std::vector<char> hset(N, 0);
    for (auto &v : g) v.assign(N, 0.0);
    const int J[4] = {0, 1, n - 2, n - 1};
    auto jidx = [&](int p) { for (int j = 0; j < 4; ++j) if (J[j] == p) return j; return -1; };
    for (int d = 0; d < N; ++d) {
        float fx = (float)((d + 0.5) * scale - 0.5);
        const int sx = (int)floorf(fx);
        fx -= sx;
        float w[4];
        oipcorr::interpolate_cubic(fx, w);
        for (int j = 0; j < 4; ++j) {
            const int p = sx - 1 + j;
            const int e = ((d - 4 * p) % N + N) % N;
            if (!hset[e]) { h[e] = w[j]; hset[e] = 1; }
            else if (h[e] != (double)w[j]) return OIP_E_UNSUPPORTED;     // taps not periodic in d: no circulant part
            if (p < 0 || p >= n) {
                const int a = jidx(p < 0 ? 0 : n - 1), b = jidx(((p % n) + n) % n);
                if (a < 0 || b < 0) return OIP_E_UNSUPPORTED;
                g[a][d] += w[j];
                g[b][d] -= w[j];
            }
        }
    }
    const double step = -2.0 * 3.14159265358979323846 / N;
    auto dft = [&](const std::vector<double> &v, float *dst) {
        std::vector<int> nz;
        for (int d = 0; d < N; ++d) if (v[d] != 0.0) nz.push_back(d);
        for (int k = 0; k < N; ++k) {
            double re = 0.0, im = 0.0;
            for (int d : nz) {
                const double ang = step * (double)(((long)k * d) % N);
                re += v[d] * cos(ang);
                im += v[d] * sin(ang);
            }
            dst[2 * k] = (float)re;
            dst[2 * k + 1] = (float)im;
        }
    };
    dft(h, out);
    for (int j = 0; j < 4; ++j) dft(g[j], out + (size_t)(1 + j) * N * 2);
    return OIP_OK;
}

// ---- oip quicklook, host side: the contrast stretch between the histogram and the look-up kernel (include/oip_c.h states
// the arithmetic; tests/_quicklook_ref.py restates it) ------------------------------------------------------------------
extern "C" int oip_stretch_limits(const uint64_t *hist, int valid_min, int valid_max, double p_lo, double p_hi, int *lo, int *hi,
                                  uint64_t *n_valid)
{
    if (!hist || !lo || !hi || valid_min < 0 || valid_max > 65535 || valid_min > valid_max || !(p_lo >= 0.0) || !(p_hi <= 100.0) || !(p_lo <= p_hi))
        return OIP_E_INVALID;
    uint64_t N = 0;
    for (int v = valid_min; v <= valid_max; ++v) N += hist[v];
    if (n_valid) *n_valid = N;
    *lo = *hi = 0;
    if (N == 0) return OIP_OK;
    auto at = [&](double p) {
        const double f = std::floor((double)N * p / 100.0);
        uint64_t r = f >= 18446744073709551616.0 ? N - 1 : (uint64_t)f;
        if (r > N - 1) r = N - 1;
        uint64_t cum = 0;
        for (int v = valid_min; v <= valid_max; ++v) {
            cum += hist[v];
            if (cum > r) return v;
        }
        return valid_max;                                    // not reached: cum ends at N > r
    };
    *lo = at(p_lo);
    *hi = at(p_hi);
    return OIP_OK;
}

extern "C" int oip_stretch_lut_u8(int lo, int hi, uint8_t *lut)
{
    if (!lut || lo < 0 || hi > 65535 || lo > hi) return OIP_E_INVALID;
    const uint32_t span = (uint32_t)(hi - lo);
    for (int v = 0; v < 65536; ++v) {
        if (span == 0) { lut[v] = v < lo ? 0 : 255; continue; }
        const uint32_t c = (uint32_t)((v < lo ? lo : (v > hi ? hi : v)) - lo);
        lut[v] = (uint8_t)((c * 510u + span) / (2u * span));           // 65535 * 510 + 65535 < 2^32
    }
    return OIP_OK;
}

extern "C" int oip_overview_levels(int w, long h)
{
    int n = 1;
    while (n < 16 && ((((long)w - 1) >> n) + 1 > 256 || ((h - 1) >> n) + 1 > 256)) ++n;      // ceil(v / 2^n) of v >= 1
    return n;
}

// ---- regcheck: the host side of oip_match_tiles_u16 (include/oip_c.h) ---------------------------------------------------
static bool match_sizes_ok(int T, int S)
{
    return T >= OIP_MATCH_MIN_T && T <= OIP_MATCH_MAX_T && T % 8 == 0 && S >= 1 && S <= OIP_MATCH_MAX_S;
}

extern "C" int oip_match_grid(int w, long rows, int T, int S, int step, int *x0, long *y0, int *nx, long *ny)
{
    if (!x0 || !y0 || !nx || !ny) return OIP_E_INVALID;
    *x0 = 0; *y0 = 0; *nx = 0; *ny = 0;
    if (!match_sizes_ok(T, S) || step < 1 || w < T + 2 * S || rows < T + 2 * S) return OIP_E_INVALID;
    *x0 = S;
    *y0 = S;
    *nx = (w - 2 * S - T) / step + 1;
    *ny = (rows - 2 * S - T) / step + 1;
    return OIP_OK;
}

// the score of one (sb, sbb, sab) against the tile's sa, saa: the ONE statement of it on the host
static double match_score(int64_t n, int64_t sa, int64_t saa, const uint64_t *q)
{
    const int64_t sb = (int64_t)q[0], sbb = (int64_t)q[1], sab = (int64_t)q[2];
    const int64_t va = n * saa - sa * sa, vb = n * sbb - sb * sb;
    if (va <= 0 || vb <= 0) return OIP_MATCH_NO_SCORE;
    return (double)(n * sab - sa * sb) / sqrt((double)va * (double)vb);
}

static double match_subpixel(double l, double c, double r)
{
    if (l <= OIP_MATCH_NO_SCORE || c <= OIP_MATCH_NO_SCORE || r <= OIP_MATCH_NO_SCORE) return 0.0;
    const double den = l - 2.0 * c + r;
    if (!(den < 0.0)) return 0.0;
    const double f = (l - r) / (2.0 * den);
    return f > 0.5 ? 0.5 : (f < -0.5 ? -0.5 : f);
}

extern "C" int oip_match_peak(const uint64_t *record, int T, int S, double min_score, double *dx, double *dy, double *score, int *flags)
{
    if (!record || !dx || !dy || !score || !flags || !match_sizes_ok(T, S)) return OIP_E_INVALID;
    const int K = 2 * S + 1;
    if (record[4] >= (uint64_t)(K * K)) return OIP_E_INVALID;
    const int j = (int)record[4] / K, i = (int)record[4] % K;
    const int64_t n = (int64_t)T * T, sa = (int64_t)record[0], saa = (int64_t)record[1];
    double sc[5];                                                // peak, left, right, upper, lower
    for (int k = 0; k < 5; ++k) sc[k] = match_score(n, sa, saa, record + 5 + 3 * k);
    const double fx = i > 0 && i < K - 1 ? match_subpixel(sc[1], sc[0], sc[2]) : 0.0;
    const double fy = j > 0 && j < K - 1 ? match_subpixel(sc[3], sc[0], sc[4]) : 0.0;
    int f = 0;
    if (record[2] + record[3] > 0) f |= OIP_MATCH_NODATA;
    if (sc[0] <= OIP_MATCH_NO_SCORE) f |= OIP_MATCH_FLAT;
    if (i == 0 || i == K - 1 || j == 0 || j == K - 1) f |= OIP_MATCH_EDGE;
    if (sc[0] < min_score) f |= OIP_MATCH_WEAK;
    *dx = (double)(i - S) + fx;
    *dy = (double)(j - S) + fy;
    *score = sc[0];
    *flags = f;
    return OIP_OK;
}

extern "C" int oip_match_summary(const double *dx, const double *dy, const int *flags, long n, double *out)
{
    if (!out || n < 0 || (n > 0 && (!dx || !dy || !flags))) return OIP_E_INVALID;
    for (int k = 0; k < 8; ++k) out[k] = 0.0;
    std::vector<double> r;
    double sx = 0.0, sy = 0.0;
    for (long t = 0; t < n; ++t)
        if (flags[t] == 0) {
            sx += dx[t];
            sy += dy[t];
            r.push_back(sqrt(dx[t] * dx[t] + dy[t] * dy[t]));
        }
    const size_t m = r.size();
    if (m == 0) return OIP_OK;
    const double mx = sx / (double)m, my = sy / (double)m;
    double vx = 0.0, vy = 0.0, rr = 0.0;
    for (long t = 0; t < n; ++t)
        if (flags[t] == 0) {
            vx += (dx[t] - mx) * (dx[t] - mx);
            vy += (dy[t] - my) * (dy[t] - my);
            rr += dx[t] * dx[t] + dy[t] * dy[t];
        }
    std::sort(r.begin(), r.end());
    const size_t rank = (9 * m + 9) / 10;                        // ceil(0.9 m), exact in integers
    out[0] = (double)m;
    out[1] = mx;
    out[2] = my;
    out[3] = sqrt(vx / (double)m);
    out[4] = sqrt(vy / (double)m);
    out[5] = sqrt(rr / (double)m);
    out[6] = r[rank - 1];
    out[7] = r[m - 1];
    return OIP_OK;
}

extern "C" int oip_write_tiff_u8(const char *path, const uint8_t *data, int width, long height, int spp, char *err, int errlen)
{
    auto fail = [&](int code, const char *msg) {
        if (err && errlen > 0) snprintf(err, errlen, "%s", msg);
        return code;
    };
    if (!path) return fail(OIP_E_INVALID, "oip_write_tiff_u8: bad argument");
    try {
        OIPGPU::write_tiff_u8(path, data, width, height, spp);
    } catch (const std::invalid_argument &e) {
        return fail(OIP_E_INVALID, e.what());
    } catch (const std::exception &e) {
        return fail(OIP_E_IO, e.what());
    }
    return OIP_OK;
}

// ---- oip mtfc, host side: the taps of oip_convolve_u16 (include/oip_c.h states the operation order; tests/_mtfc_ref.py
// restates it).  fp64 throughout, one rounded operation per step (-ffp-contract=off) ------------------------------------
static bool mtfc_size_ok(int ky, int kx) { return ky >= 1 && kx >= 1 && ky <= OIP_CONVOLVE_MAX_K && kx <= OIP_CONVOLVE_MAX_K && ky % 2 == 1 && kx % 2 == 1; }

extern "C" int oip_mtfc_quantise(const double *c, int ky, int kx, int32_t *taps, char *err, int errlen)
{
    auto fail = [&](int code, const char *fmt, auto... a) {
        if (err && errlen > 0) snprintf(err, errlen, fmt, a...);
        return code;
    };
    if (!c || !taps || !mtfc_size_ok(ky, kx)) return fail(OIP_E_INVALID, "%s", "oip_mtfc_quantise: bad argument (odd sizes 1..9 expected)");
    const int n = ky * kx;
    double t[OIP_CONVOLVE_MAX_K * OIP_CONVOLVE_MAX_K];
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
        const double s = c[i] * 4096.0;
        t[i] = std::rint(s);                                  // ties to even (default rounding mode)
        sum += c[i];
    }
    const double dev = std::fabs(sum - 1.0);
    if (!(dev <= 1e-6)) return fail(OIP_E_INVALID, "oip_mtfc_quantise: the coefficients sum to %.9g, not to 1 (within 1e-6)", sum);
    long tsum = 0;
    for (int i = 0; i < n; ++i) {
        if (!(std::fabs(t[i]) <= 1073741824.0)) return fail(OIP_E_INVALID, "oip_mtfc_quantise: coefficient %d (%g) is out of range", i, c[i]);
        taps[i] = (int32_t)t[i];
        tsum += taps[i];
    }
    taps[(ky / 2) * kx + kx / 2] += (int32_t)(4096 - tsum);   // DC gain exactly 1: flat areas stay as they are
    long abssum = 0;
    for (int i = 0; i < n; ++i) abssum += taps[i] < 0 ? -(long)taps[i] : (long)taps[i];
    if (abssum > 32767)
        return fail(OIP_E_INVALID, "oip_mtfc_quantise: sum |taps| = %ld above 32767 (the int32 accumulator of oip_convolve_u16): lower the gain", abssum);
    return OIP_OK;
}

extern "C" int oip_mtfc_design3(double mtf_x, double mtf_y, double max_gain, double *c9)
{
    if (!c9 || !(mtf_x > 0.0 && mtf_x <= 1.0) || !(mtf_y > 0.0 && mtf_y <= 1.0) || !(max_gain >= 1.0)) return OIP_E_INVALID;
    double f[2][3];
    const double m[2] = {mtf_x, mtf_y};
    for (int k = 0; k < 2; ++k) {
        const double inv = 1.0 / m[k];
        const double g = inv < max_gain ? inv : max_gain;
        const double d = g - 1.0;
        const double a = d / 4.0;
        const double a2 = 2.0 * a;
        f[k][0] = -a;
        f[k][1] = 1.0 + a2;
        f[k][2] = -a;
    }
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) c9[j * 3 + i] = f[1][j] * f[0][i];
    return OIP_OK;
}

extern "C" int oip_mtfc_load_kernel(const char *path, double *c, int *ky, int *kx, char *err, int errlen)
{
    auto fail = [&](int code, const char *fmt, auto... a) {
        if (err && errlen > 0) snprintf(err, errlen, fmt, a...);
        return code;
    };
    if (!path || !c || !ky || !kx) return fail(OIP_E_INVALID, "%s", "oip_mtfc_load_kernel: bad argument");
    FILE *f = fopen(path, "rb");
    if (!f) return fail(OIP_E_IO, "open kernel file [%s] failed: %s", path, strerror(errno));
    std::string text;
    char buff[4096];
    size_t got = 0;
    while (text.size() <= 65536 && (got = fread(buff, 1, sizeof buff, f)) > 0) text.append(buff, got);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) return fail(OIP_E_IO, "read of kernel file [%s] failed", path);
    if (text.size() > 65536 || text.find('\0') != std::string::npos) return fail(OIP_E_INVALID, "kernel file [%s] invalid: not a small text file", path);
    const char *p = text.c_str();
    char *e = nullptr;
    long dims[2] = {0, 0};
    for (int k = 0; k < 2; ++k) {
        dims[k] = strtol(p, &e, 10);
        if (e == p) return fail(OIP_E_INVALID, "kernel file [%s] invalid: first line `ky kx' expected", path);
        p = e;
    }
    if (dims[0] < 1 || dims[1] < 1 || dims[0] > OIP_CONVOLVE_MAX_K || dims[1] > OIP_CONVOLVE_MAX_K || dims[0] % 2 == 0 || dims[1] % 2 == 0)
        return fail(OIP_E_INVALID, "kernel file [%s] invalid: size %ld x %ld, odd sizes 1..%d expected", path, dims[0], dims[1], OIP_CONVOLVE_MAX_K);
    const int n = (int)(dims[0] * dims[1]);
    for (int i = 0; i < n; ++i) {
        c[i] = strtod(p, &e);
        if (e == p) return fail(OIP_E_INVALID, "kernel file [%s] invalid: %d numbers expected, %d found", path, n, i);
        p = e;
    }
    while (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r' || *p == '\f' || *p == '\v') ++p;
    if (*p) return fail(OIP_E_INVALID, "kernel file [%s] invalid: text behind the %d numbers", path, n);
    *ky = (int)dims[0];
    *kx = (int)dims[1];
    return OIP_OK;
}

// ---- oip despike, host side: the list of bad columns (a text file) and the (Lx, Rx) table oip_despike_u16 reads
// (include/oip_c.h states both; tests/_despike_ref.py restates them) ---------------------------------------------------------
extern "C" int oip_load_column_list(const char *path, int w, int *cols, int cap, int *n, char *err, int errlen)
{
    auto fail = [&](int code, const char *fmt, auto... a) {
        if (err && errlen > 0) snprintf(err, errlen, fmt, a...);
        return code;
    };
    if (!path || w <= 0 || cap < 0 || (!cols && cap > 0) || !n) return fail(OIP_E_INVALID, "%s", "oip_load_column_list: bad argument");
    FILE *f = fopen(path, "rb");
    if (!f) return fail(OIP_E_IO, "open column list [%s] failed: %s", path, strerror(errno));
    const size_t limit = (size_t)16 << 20;                        // twelve bytes a column of the widest line is far below
    std::string text;
    char buff[4096];
    size_t got = 0;
    while (text.size() <= limit && (got = fread(buff, 1, sizeof buff, f)) > 0) text.append(buff, got);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) return fail(OIP_E_IO, "read of column list [%s] failed", path);
    if (text.size() > limit || text.find('\0') != std::string::npos) return fail(OIP_E_INVALID, "column list [%s] invalid: not a text file of that kind", path);
    std::vector<int> list;
    const char *p = text.c_str();
    for (;;) {
        while (*p == ' ' || *p == '\t' || *p == '\n' || *p == '\r' || *p == '\f' || *p == '\v') ++p;
        if (*p == '#') {                                           // a comment runs to the end of the line
            while (*p && *p != '\n') ++p;
            continue;
        }
        if (!*p) break;
        const char *t = p;
        while (*p && *p != '#' && *p != ' ' && *p != '\t' && *p != '\n' && *p != '\r' && *p != '\f' && *p != '\v') ++p;
        const std::string tok(t, p);
        const char *d = tok.c_str();
        if (*d == '+' || *d == '-') ++d;
        if (!*d || strspn(d, "0123456789") != strlen(d)) return fail(OIP_E_INVALID, "column list [%s] invalid: `%.32s' is not a number", path, tok.c_str());
        errno = 0;
        const long v = strtol(tok.c_str(), nullptr, 10);
        if (errno == ERANGE || v < 0 || v >= w) return fail(OIP_E_INVALID, "column list [%s] invalid: column %.32s outside [0, %d)", path, tok.c_str(), w);
        list.push_back((int)v);
    }
    std::sort(list.begin(), list.end());
    list.erase(std::unique(list.begin(), list.end()), list.end());
    if (list.size() > (size_t)cap) return fail(OIP_E_INVALID, "column list [%s] invalid: %zu columns, room for %d", path, list.size(), cap);
    for (size_t i = 0; i < list.size(); ++i) cols[i] = list[i];
    *n = (int)list.size();
    return OIP_OK;
}

extern "C" int oip_write_column_list(const char *path, const int *cols, int n, const char *comment, char *err, int errlen)
{
    auto fail = [&](int code, const char *fmt, auto... a) {
        if (err && errlen > 0) snprintf(err, errlen, fmt, a...);
        return code;
    };
    if (!path || n < 0 || (!cols && n > 0)) return fail(OIP_E_INVALID, "%s", "oip_write_column_list: bad argument");
    FILE *f = fopen(path, "wb");
    if (!f) return fail(OIP_E_IO, "open column list [%s] for writing failed: %s", path, strerror(errno));
    std::string head = comment ? comment : "";
    for (char &c : head)
        if (c == '\n' || c == '\r') c = ' ';                        // the comment stays one line
    bool ok = fprintf(f, "# %s\n", head.c_str()) > 0;
    for (int i = 0; i < n && ok; ++i) ok = fprintf(f, "%d\n", cols[i]) > 0;
    ok = fclose(f) == 0 && ok;
    if (!ok) return fail(OIP_E_IO, "write of column list [%s] failed", path);
    return OIP_OK;
}

extern "C" int oip_despike_column_table(const int *bad, int nbad, int w, int groups, int32_t *tab, int *longest_run, char *err, int errlen)
{
    auto fail = [&](int code, const char *fmt, auto... a) {
        if (err && errlen > 0) snprintf(err, errlen, fmt, a...);
        return code;
    };
    if (!tab || nbad < 0 || (!bad && nbad > 0) || w <= 0 || (groups != 1 && groups != 4) || w % groups != 0)
        return fail(OIP_E_INVALID, "%s", "oip_despike_column_table: bad argument");
    std::vector<char> isBad((size_t)w, 0);
    for (int i = 0; i < nbad; ++i) {
        if (bad[i] < 0 || bad[i] >= w) return fail(OIP_E_INVALID, "oip_despike_column_table: column %d outside [0, %d)", bad[i], w);
        isBad[bad[i]] = 1;
    }
    const int gw = w / groups;
    int longest = 0;
    for (int g = 0; g < groups; ++g) {
        const int g0 = g * gw, g1 = g0 + gw;
        int good = -1, run = 0;                                     // the nearest good column on the left, inside the group
        for (int x = g0; x < g1; ++x) {
            if (!isBad[x]) { good = x; run = 0; }
            else if (++run > longest) longest = run;
            tab[2 * (size_t)x] = good;
        }
        if (good < 0) return fail(OIP_E_INVALID, "oip_despike_column_table: group %d has no good column", g);
        good = -1;
        for (int x = g1 - 1; x >= g0; --x) {                        // ... and on the right; a missing side copies the other
            if (!isBad[x]) good = x;
            tab[2 * (size_t)x + 1] = good >= 0 ? good : tab[2 * (size_t)x];
            if (tab[2 * (size_t)x] < 0) tab[2 * (size_t)x] = tab[2 * (size_t)x + 1];
        }
    }
    if (longest_run) *longest_run = longest;
    return OIP_OK;
}

// ---- oip regfix, host side: the node lattice of oip_warp_grid_bicubic_u16 from a regcheck report (oip_warpfield.hpp;
// include/oip_c.h states the steps, tests/_regfix_ref.py restates them) ----------------------------------------------------
extern "C" int oip_regfix_load_report(const char *path, long w, long h, int32_t *nodes_x, int32_t *nodes_y, long cap, long *geom, char *err, int errlen)
{
    auto fail = [&](int code, const char *msg) {
        if (err && errlen > 0) snprintf(err, errlen, "%s", msg);
        return code;
    };
    if (!path || !geom || cap < 0 || (cap > 0 && (!nodes_x || !nodes_y)) || w < 0 || h < 0) return fail(OIP_E_INVALID, "oip_regfix_load_report: bad argument");
    try {
        const OIPGPU::WarpField f = OIPGPU::ParseRegReport(OIPGPU::ReadRegReport(path), w, h);
        const long n = (long)f.nx * f.ny;
        if (n > cap) return fail(OIP_E_INVALID, ("oip_regfix_load_report: " + std::to_string(n) + " nodes, room for " + std::to_string(cap)).c_str());
        std::copy(f.X.begin(), f.X.end(), nodes_x);
        std::copy(f.Y.begin(), f.Y.end(), nodes_y);
        const long g[8] = {f.nx, f.ny, f.gx0, f.gy0, f.sx, f.sy, f.band2, f.used};
        std::copy(g, g + 8, geom);
    } catch (const std::invalid_argument &e) {
        return fail(OIP_E_INVALID, e.what());
    } catch (const std::exception &e) {
        return fail(OIP_E_IO, e.what());
    }
    return OIP_OK;
}

static bool regfix_lattice_ok(const int32_t *nodes_x, const int32_t *nodes_y, int nx, int ny)
{
    return nodes_x && nodes_y && nx >= 1 && ny >= 1 && (long)nx * ny <= OIPGPU::kWarpMaxNodes;
}

extern "C" int oip_regfix_fill(int32_t *nodes_x, int32_t *nodes_y, const uint8_t *set, int nx, int ny)
{
    if (!regfix_lattice_ok(nodes_x, nodes_y, nx, ny) || !set) return OIP_E_INVALID;
    for (long q = 0; q < (long)nx * ny; ++q)                       // the sums of four stay far inside 64 bits whatever is given; the results
        if (set[q] && (nodes_x[q] < -OIP_WARP_MAX_Q10 || nodes_x[q] > OIP_WARP_MAX_Q10 || nodes_y[q] < -OIP_WARP_MAX_Q10 || nodes_y[q] > OIP_WARP_MAX_Q10))
            return OIP_E_INVALID;                                  // lie between the values they average, so inside the range as well
    return OIPGPU::FillField(nodes_x, nodes_y, set, nx, ny) ? OIP_OK : OIP_E_INVALID;
}

extern "C" int oip_regfix_smooth(int32_t *nodes_x, int32_t *nodes_y, int nx, int ny, int passes)
{
    if (!regfix_lattice_ok(nodes_x, nodes_y, nx, ny) || passes < 0 || passes > OIP_REGFIX_MAX_SMOOTH) return OIP_E_INVALID;
    for (long q = 0; q < (long)nx * ny; ++q)                       // (a + 2 b + c + 2 stays inside int32)
        if (nodes_x[q] < -OIP_WARP_MAX_Q10 || nodes_x[q] > OIP_WARP_MAX_Q10 || nodes_y[q] < -OIP_WARP_MAX_Q10 || nodes_y[q] > OIP_WARP_MAX_Q10) return OIP_E_INVALID;
    OIPGPU::SmoothField(nodes_x, nx, ny, passes);
    OIPGPU::SmoothField(nodes_y, nx, ny, passes);
    return OIP_OK;
}

// ---- oip pansharpen, host side: which MSS lines a PAN raster covers from line_offset on, and the product's size
// (include/oip_c.h states the rule, tests/_pansharpen_ref.py restates it) ------------------------------------------------
extern "C" int oip_pansharpen_geometry(long W, long Hp, long w, long h, long line_offset, long *out_w, long *out_h, long *mss_lines)
{
    if (w < 1 || h < 1 || w > (1L << 26) || W != 4 * w || line_offset < 0 || Hp < 4 || line_offset > Hp - 4) return OIP_E_INVALID;
    const long hh = std::min(h, (Hp - line_offset) / 4);
    if (out_w) *out_w = 4 * w;
    if (out_h) *out_h = 4 * hh;
    if (mss_lines) *mss_lines = hh;
    return OIP_OK;
}

// ---- oip noise, host side: the sigma of every signal level from a band's key histogram, the fit sigma^2 = a + b mu, and the
// despike threshold that follows from it (include/oip_c.h states the operation order, tests/_noise_ref.py restates it) ------
extern "C" int oip_noise_levels(const uint64_t *hist, uint64_t min_blocks, double *sigma, uint64_t *blocks, int *n_usable)
{
    if (!hist || !sigma || !blocks) return OIP_E_INVALID;
    const uint64_t need = min_blocks > 1 ? min_blocks : 1;
    int usable = 0;
    for (int l = 0; l < 256; ++l) {
        const uint64_t *h = hist + (size_t)l * 256;
        uint64_t N = 0;
        for (int q = 0; q <= 254; ++q) N += h[q];
        blocks[l] = N;
        sigma[l] = -1.0;
        if (N < need) continue;
        int mode = -1;
        for (int q = 0; q <= 253; ++q)
            if (h[q] > (mode < 0 ? 0 : h[mode])) mode = q;
        if (mode < 0) continue;
        const int r = mode / 8 + 1, lo = std::max(0, mode - r), hi = std::min(253, mode + r);
        uint64_t cw = 0;
        for (int q = lo; q <= hi; ++q) cw += h[q];
        // (N < 2^61 for any histogram of real blocks: the products below do not wrap)
        if (10 * cw < 3 * N) continue;
        double sum = 0.0;
        for (int q = lo; q <= hi; ++q) sum += ((double)q + 0.5) * (double)h[q];
        sigma[l] = 0.25 * sum / (double)cw;
        ++usable;
    }
    if (n_usable) *n_usable = usable;
    return OIP_OK;
}

extern "C" int oip_noise_fit(const double *sigma, const uint64_t *blocks, int level_shift, double *a, double *b, double *mu_ref, char *err, int errlen)
{
    auto fail = [&](int code, const char *msg) {
        if (err && errlen > 0) snprintf(err, errlen, "%s", msg);
        return code;
    };
    if (!sigma || !blocks || !a || !b || !mu_ref || level_shift < 0 || level_shift > 8) return fail(OIP_E_INVALID, "oip_noise_fit: bad argument");
    const double scale = (double)(1 << level_shift);
    auto mu_of = [&](int l) { return ((double)l + 0.5) * scale; };
    double sw = 0.0, swx = 0.0, swv = 0.0, swxv = 0.0, swxx = 0.0;
    uint64_t total = 0;
    int count = 0;
    for (int l = 0; l < 256; ++l) {
        if (!(sigma[l] >= 0.0)) continue;
        const double mu = mu_of(l), v = sigma[l] * sigma[l], w = (double)blocks[l];
        sw += w; swx += w * mu; swv += w * v; swxv += w * mu * v; swxx += w * mu * mu;
        total += blocks[l];
        ++count;
    }
    if (count == 0 || total == 0) return fail(OIP_E_RUNTIME, "oip_noise_fit: no usable signal level");
    const double mx = swx / sw, mv = swv / sw;
    double sxx = 0.0, sxy = 0.0;
    for (int l = 0; l < 256; ++l) {
        if (!(sigma[l] >= 0.0)) continue;
        const double mu = mu_of(l), v = sigma[l] * sigma[l], w = (double)blocks[l];
        sxx += w * (mu - mx) * (mu - mx);
        sxy += w * (mu - mx) * (v - mv);
    }
    double bb = 0.0, aa = mv;
    if (count >= 2 && sxx != 0.0) {
        bb = sxy / sxx;
        aa = mv - bb * mx;
        if (bb < 0.0) { bb = 0.0; aa = mv; }
        else if (aa < 0.0) { aa = 0.0; bb = swxv / swxx; }
    }
    uint64_t cum = 0;
    for (int l = 0; l < 256; ++l) {
        if (!(sigma[l] >= 0.0)) continue;
        cum += blocks[l];
        if (2 * cum >= total) { *mu_ref = mu_of(l); break; }
    }
    *a = aa;
    *b = bb;
    return OIP_OK;
}

extern "C" int oip_noise_despike_threshold(double a, double b, double mu_ref, double k, int *thr_abs, int *thr_rel_q8, char *err, int errlen)
{
    auto fail = [&](int code, const char *fmt, auto... v) {
        if (err && errlen > 0) snprintf(err, errlen, fmt, v...);
        return code;
    };
    if (!thr_abs || !thr_rel_q8 || !std::isfinite(a) || !std::isfinite(b) || !std::isfinite(mu_ref) || !std::isfinite(k) || a < 0.0 || b < 0.0 ||
        mu_ref < 0.0 || !(k > 0.0))
        return fail(OIP_E_INVALID, "%s", "oip_noise_despike_threshold: bad argument");
    const double st = std::sqrt(a + b * mu_ref);
    if (st == 0.0) return fail(OIP_E_RUNTIME, "%s", "oip_noise_despike_threshold: the noise model gives sigma 0 at the reference level");
    const double R = k * b / (2.0 * st), N0 = k * st - R * mu_ref;
    const double q8 = std::ceil(256.0 * R), ta = std::ceil(N0) + 1.0;
    if (!(q8 <= 256.0)) return fail(OIP_E_RUNTIME, "oip_noise_despike_threshold: the slope %.6g of the threshold exceeds 1", R);
    if (!(ta <= 65535.0)) return fail(OIP_E_RUNTIME, "oip_noise_despike_threshold: the threshold %.6g exceeds 65535", ta);
    *thr_abs = (int)ta;
    *thr_rel_q8 = (int)q8;
    return OIP_OK;
}

// ---- oip denoise, host side: the threshold table of oip_sigma_filter_u16 from a noise model (include/oip_c.h states the
// operation order, tests/_denoise_ref.py restates it) ------------------------------------------------------------------------
extern "C" int oip_denoise_thresholds(double a, double b, double k, uint16_t *thr256, char *err, int errlen)
{
    auto fail = [&](int code, const char *msg) {
        if (err && errlen > 0) snprintf(err, errlen, "%s", msg);
        return code;
    };
    if (!thr256 || !std::isfinite(a) || !std::isfinite(b) || !std::isfinite(k) || a < 0.0 || b < 0.0 || !(k > 0.0))
        return fail(OIP_E_INVALID, "oip_denoise_thresholds: bad argument");
    if (a == 0.0 && b == 0.0) return fail(OIP_E_RUNTIME, "oip_denoise_thresholds: the noise model gives sigma 0 at every level");
    for (int l = 0; l < 256; ++l) {
        const double t = std::ceil(k * std::sqrt(a + b * (double)(256 * l + 128)));
        thr256[l] = (uint16_t)(t < 65535.0 ? t : 65535.0);       // (a + b * level can overflow to inf with finite a, b: inf -> 65535)
    }
    return OIP_OK;
}

// ---- oip mtf, host side: the MTF at Nyquist of a tile from its edge-spread sums, the order statistics of a band, and the slack
// that follows from a noise level (include/oip_c.h states the operation order, tests/_mtf_ref.py restates it) ---------------
extern "C" int oip_mtf_tile(int s, const uint32_t *sum, const uint32_t *cnt, double *mtf)
{
    if ((s != 1 && s != -1) || !sum || !cnt || !mtf) return OIP_E_INVALID;
    static const double H = 0.70710678118654752;
    static const double C8[8] = {1.0, H, 0.0, -H, -1.0, -H, 0.0, H}, S8[8] = {0.0, H, 1.0, H, 0.0, -H, -1.0, -H};
    const double pi = 3.14159265358979323846;
    double E[64];
    for (int b = 0; b < 64; ++b) {
        if (cnt[b] == 0) return OIP_MTF_NO_VALUE;
        E[b] = (double)s * (double)sum[b] / (double)cnt[b];
    }
    double A0 = 0.0, Re = 0.0, Im = 0.0;
    for (int j = 0; j < 63; ++j) {
        const double w = 0.54 - 0.46 * std::cos(2.0 * pi * (double)j / 62.0);
        const double t = w * (E[j + 1] - E[j]);
        const int k = (j - 31) & 7;
        A0 += t;
        Re += t * C8[k];
        Im += t * S8[k];
    }
    if (!(A0 > 0.0)) return OIP_MTF_NO_VALUE;
    const double q = std::sin(pi / 8.0) / (pi / 8.0);
    *mtf = std::hypot(Re, Im) / A0 / (q * q);
    return OIP_OK;
}

extern "C" int oip_mtf_summary(const double *values, long n, double *median, double *p75, double *p90)
{
    if (!values || n < 1 || !median || !p75 || !p90) return OIP_E_INVALID;
    for (long i = 0; i < n; ++i)
        if (!std::isfinite(values[i])) return OIP_E_INVALID;
    std::vector<double> v(values, values + n);
    std::sort(v.begin(), v.end());
    *median = v[(size_t)((n - 1) / 2)];
    *p75 = v[(size_t)(3 * (n - 1) / 4)];
    *p90 = v[(size_t)(9 * (n - 1) / 10)];
    return OIP_OK;
}

extern "C" int oip_mtf_tv_slack(double sigma_ref)
{
    if (!(sigma_ref >= 0.0)) return -1;
    const double t = std::ceil(48.0 * sigma_ref);
    return t < 65535.0 ? (int)t : 65535;
}

// ---- mask: the grid of cells and the question `oip regcheck --mask` asks per tile (include/oip_c.h) --------------------------
extern "C" int oip_mask_grid(int w, long h, int cell, int *gw, long *gh)
{
    if ((cell != 4 && cell != 8 && cell != 16) || w < 0 || h < 0 || !gw || !gh) return OIP_E_INVALID;
    *gw = (w + cell - 1) / cell;
    *gh = (h + cell - 1) / cell;
    return OIP_OK;
}

extern "C" int oip_mask_tile_flag(const uint8_t *flags, long flag_pitch, int gw, long gh, int cell, long x, long y, long tw, long th, int bits)
{
    if (!flags || (cell != 4 && cell != 8 && cell != 16) || gw < 0 || gh < 0 || flag_pitch < gw) return 0;
    if (tw <= 0 || th <= 0) return 0;
    // floor division: a rectangle may begin left of or above the image
    const long x1 = x + tw - 1, y1 = y + th - 1;
    if (x1 < 0 || y1 < 0) return 0;
    long i0 = x < 0 ? 0 : x / cell, i1 = x1 / cell, j0 = y < 0 ? 0 : y / cell, j1 = y1 / cell;
    if (i1 > gw - 1) i1 = gw - 1;
    if (j1 > gh - 1) j1 = gh - 1;
    for (long j = j0; j <= j1; ++j)
        for (long i = i0; i <= i1; ++i)
            if (flags[j * flag_pitch + i] & bits) return 1;
    return 0;
}

// ---- wallis: the grid of blocks and the step from block moments to node gains and offsets (include/oip_c.h) ------------------
extern "C" int oip_wallis_grid(int w, long h, int block, int *gw, long *gh)
{
    if ((block != 32 && block != 64 && block != 128 && block != 256) || w < 0 || h < 0 || !gw || !gh) return OIP_E_INVALID;
    *gw = (w + block - 1) / block;
    *gh = (h + block - 1) / block;
    return OIP_OK;
}

namespace {
struct WallisFit {
    double c, b, gmin, gmax, mt, st;
    uint64_t need;
};
// fit(n, S1, S2) of include/oip_c.h: false where the block has too few samples or no variance.  tests/_wallis_ref.py restates
// the operation order.
bool wallis_fit_one(const WallisFit &f, uint64_t n, uint64_t S1, uint64_t S2, int32_t *G, int32_t *O)
{
    if (n < f.need) return false;
    const unsigned __int128 a = (unsigned __int128)n * S2, q = (unsigned __int128)S1 * S1;
    if (a <= q) return false;                // (a D below zero cannot come from real moments; it is treated as 0)
    const unsigned __int128 D = a - q;
    const double nd = (double)n;
    const double m = (double)S1 / nd;
    const double r = std::sqrt((double)D);
    const double s = r / nd;
    const double t1 = f.c * s;
    const double u = 1.0 - f.c;
    const double t2 = u * f.st;
    const double den = t1 + t2;
    const double num = f.c * f.st;
    double g = num / den;
    g = g < f.gmin ? f.gmin : g;
    g = g > f.gmax ? f.gmax : g;
    const double p1 = f.b * f.mt;
    const double v = 1.0 - f.b;
    const double p2 = v * m;
    const double p = p1 + p2;
    const double gm = g * m;
    const double o = p - gm;
    *G = (int32_t)std::rint(g * 65536.0);
    *O = (int32_t)std::rint(o * 256.0);
    return true;
}
}  // namespace

extern "C" int oip_wallis_fit(const uint64_t *acc, long acc_pitch, size_t acc_plane_stride, int gw, long gh, int spp, double contrast, double brightness,
                              double g_min, double g_max, uint64_t min_count, const double *target_mean, const double *target_std,
                              int32_t *node_gain_q16, int32_t *node_offset_q8, int *substituted, double *report, char *err, int errlen)
{
    auto fail = [&](int code, const char *fmt, auto... a) {
        if (err && errlen > 0) snprintf(err, errlen, fmt, a...);
        return code;
    };
    bool ok = acc && node_gain_q16 && node_offset_q8 && substituted && (spp == 1 || spp == 4) && gw >= 1 && gh >= 1 && acc_pitch >= gw &&
              contrast > 0.0 && contrast <= 1.0 && brightness >= 0.0 && brightness <= 1.0 && g_min > 0.0 && g_min <= 1.0 && g_max >= 1.0 && g_max <= 16.0;
    if (ok && acc_plane_stride < (size_t)((gh - 1) * acc_pitch + gw)) ok = false;              // the 3 * spp planes overlap
    for (int c = 0; ok && c < spp; ++c) {
        if (target_mean && !std::isnan(target_mean[c]) && !(target_mean[c] >= 0.0 && target_mean[c] <= 65535.0)) ok = false;
        if (target_std && !std::isnan(target_std[c]) && !(target_std[c] <= 65535.0)) ok = false;
    }
    if (!ok) return fail(OIP_E_INVALID, "%s", "oip_wallis_fit: bad argument");
    const uint64_t need = min_count > 2u ? min_count : 2u;
    for (int c = 0; c < spp; ++c) {
        const uint64_t *pn = acc + (size_t)(0 * spp + c) * acc_plane_stride, *p1 = acc + (size_t)(1 * spp + c) * acc_plane_stride,
                       *p2 = acc + (size_t)(2 * spp + c) * acc_plane_stride;
        uint64_t N = 0;
        unsigned __int128 A128 = 0, Q = 0;
        for (long j = 0; j < gh; ++j)
            for (int i = 0; i < gw; ++i) {
                N += pn[j * acc_pitch + i];
                A128 += p1[j * acc_pitch + i];
                Q += p2[j * acc_pitch + i];
            }
        if (N < need) return fail(OIP_E_RUNTIME, "oip_wallis_fit: channel %d: %llu valid samples, %llu needed", c, (unsigned long long)N, (unsigned long long)need);
        if ((A128 >> 64) || (Q >> 64)) return fail(OIP_E_INVALID, "oip_wallis_fit: channel %d: the sum or the sum of squares does not fit 64 bits", c);
        const uint64_t A = (uint64_t)A128;
        const unsigned __int128 nq = (unsigned __int128)N * (uint64_t)Q, aa = (unsigned __int128)A * A;
        const unsigned __int128 D0 = nq > aa ? nq - aa : 0;
        const double Nd = (double)N;
        const double m0 = (double)A / Nd;
        const double r0 = std::sqrt((double)D0);
        const double s0 = r0 / Nd;
        WallisFit f;
        f.c = contrast; f.b = brightness; f.gmin = g_min; f.gmax = g_max; f.need = need;
        f.mt = target_mean && !std::isnan(target_mean[c]) ? target_mean[c] : m0;
        f.st = target_std && !std::isnan(target_std[c]) ? target_std[c] : s0;
        if (!(f.st > 0.0))
            return fail(OIP_E_RUNTIME, "oip_wallis_fit: channel %d: the target standard deviation %g is not positive (a constant channel needs --std)", c, f.st);
        int32_t G0 = 65536, O0 = 0;
        if (D0 != 0) wallis_fit_one(f, N, A, (uint64_t)Q, &G0, &O0);
        long subs = 0;
        int32_t lo = INT32_MAX, hi = INT32_MIN;
        for (long j = 0; j < gh; ++j)
            for (int i = 0; i < gw; ++i) {
                const size_t e = ((size_t)j * gw + i) * spp + c;
                int32_t G = G0, O = O0;
                const bool own = wallis_fit_one(f, pn[j * acc_pitch + i], p1[j * acc_pitch + i], p2[j * acc_pitch + i], &G, &O);
                if (!own) { G = G0; O = O0; ++subs; }
                node_gain_q16[e] = G;
                node_offset_q8[e] = O;
                substituted[e] = own ? 0 : 1;
                lo = G < lo ? G : lo;
                hi = G > hi ? G : hi;
            }
        if (report) {
            double *r = report + 9 * (size_t)c;
            r[0] = Nd; r[1] = m0; r[2] = s0; r[3] = f.mt; r[4] = f.st; r[5] = (double)gh * (double)gw; r[6] = (double)subs; r[7] = (double)lo; r[8] = (double)hi;
        }
    }
    return OIP_OK;
}

// ---- rescale: the tap tables, the size of a scaled axis and the lines a window needs (include/oip_c.h; arithmetic: oip_rescaleplan.h)
extern "C" int oip_rescale_taps(int kind, long n_in, long n_out, int *first, int16_t *taps, size_t cap, int *K, char *err, int errlen)
{
    return oip_rescale_taps_impl(kind, n_in, n_out, first, taps, cap, K, err, errlen);
}

extern "C" int oip_rescale_size(long n_in, long p, long q, long *n_out) { return oip_rescale_size_impl(n_in, p, q, n_out); }

extern "C" int oip_rescale_src_range(long n_in, long n_out, int K, long out0, long outs, long *src0, long *srcs)
{
    return oip_rescale_src_range_impl(n_in, n_out, K, out0, outs, src0, srcs);
}
