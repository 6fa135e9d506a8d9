// oip_fftplan.h -- the host planning arithmetic of the 2-D FFT engine (fft.hip): which pass factors an axis is split into,
// which kernel and lane-tile class a pass gets, its radix chain, its LDS bytes, and what the planner and the launcher refuse.
// Nothing of HIP in here: fft.hip plans and launches by these lines, oip_fft_plan_describe (include/oip_c.h) states them, and
// tests/cpp/fftplan_test.cpp runs them on the CPU over every 2^a 3^b 5^c length.
#pragma once

#include <cstddef>
#include <cstdio>
#include <cstring>

#include <functional>
#include <vector>

struct OipFftPass {
    int F;              // sub-transform length of this pass
    int nradix;
    int radix[16];      // Stockham radices, product == F (generic kernel)
    int vshift;         // log2(V): V adjacent transforms per workgroup tile
    int Vp;             // LDS row pitch (V+1, or 1 when V == 1)
    int mode;           // 0: points strided, lanes contiguous; 1: points contiguous
    int axis;           // 0: x (rows), 1: y (columns)
    long nstride;       // mode 0: elements between consecutive points
    long lanes;         // mode 0: lanes in the contiguous direction; mode 1: number of vectors
    int lane_tiles;
    int O1;             // mode 0 outer dimension 1 (count, element stride)
    long o1_stride;
    int O2;
    long o2_stride;
    int tw_mode;        // 0 none; 1: j = lane index; 2: j = o1 index  (twiddle w_T^(j*k))
    int T;
    int S;              // stride of the sub-transform in axis elements (T / F)
    int N;              // row length of the array (to turn offsets into coordinates)
    int M;
    int P;              // row pitch in elements (N rounded up to whole 128-byte lines)
    int inverse;
    long ntiles;        // tiles of this launch (persistent specialised kernels walk them)
    int fast;           // index of a compile-time specialised kernel, -1: generic
    int grid3;          // mode 0 launched as a (lane tile, o1, o2) grid: the tile needs no divisions to decode
    int xcd_chunk;      // grid3: lane tiles per XCD (grid x = 8 * xcd_chunk >= lane tiles); see decode_tile
};

// What the planner hands to the engine: the part of OipFft2dPlan that needs no device
struct OipFftHostPlan {
    int M, N;
    int P;                            // row pitch of the complex array, elements
    std::vector<int> xf, yf;          // pass factors per axis, in forward order
    std::vector<OipFftPass> passes;   // forward order: y passes then x passes
    int n_y;
};

constexpr int kPeakSlots = 256;       // arg-max slots per correlation surface (oip_fft.h: oip_peak_pack)

namespace oipfftplan {

// codes of a refusal: the values of OIP_OK, OIP_E_INVALID, OIP_E_RUNTIME and OIP_E_UNSUPPORTED (include/oip_c.h; host.cpp asserts it)
enum { kPlanOk = 0, kPlanInvalid = 1, kPlanRuntime = 2, kPlanUnsupported = 6 };

constexpr int kFftBlock = 256;            // threads of the generic kernel
constexpr int kMaxTileElems = 5120;       // generic kernel: F * (V+1) complex elements per LDS buffer
constexpr int kGenericStaticLds = kFftBlock * (int)(sizeof(float) + sizeof(long));        // its sval / skey reduction arrays
constexpr int kMaxLdsBytes = 160 * 1024;  // LDS of a gfx950 workgroup
constexpr int kMaxLeadFactor = 256, kMaxLastColFactor = 256, kMaxLastRowFactor = 4096;

// keys of the specialised kernels, (F, log2 V, mode): entry i names the kernels of kFast[i] (fft.hip)
struct FastKey {
    int F, vshift, mode;
};
constexpr FastKey kFastKeys[] = {
    // column passes of 16000 = 125 * 128 (and other 5^3 / 2^7 factors): 16 lanes = 128-byte
    // segments, 17 KiB of LDS per workgroup -> 8 workgroups per CU (measured faster than 32 lanes)
    {125, 4, 0}, {128, 4, 0}, {100, 4, 0}, {160, 4, 0}, {64, 5, 0},
    // 4000 = 32 * 125: the column transform of the band windows themselves (a quarter of the correlation lines)
    {32, 5, 0},
    // row passes: 30000/10, 12288/10 -> 1250, the 200-column stitch overlap
    {3000, 1, 1}, {1250, 1, 1}, {200, 4, 1},
};
constexpr int kNumFastKeys = sizeof(kFastKeys) / sizeof(kFastKeys[0]);

inline bool smooth235(long n)
{
    if (n < 1) return false;
    for (int p : {2, 3, 5}) while (n % p == 0) n /= p;
    return n == 1;
}

inline std::vector<int> radix_list(int F)
{
    std::vector<int> r;
    int twos = 0;
    while (F % 2 == 0) { F /= 2; ++twos; }
    while (F % 3 == 0) { F /= 3; r.push_back(3); }
    for (; twos >= 3; twos -= 3) r.push_back(8);
    if (twos == 2) r.push_back(4);
    if (twos == 1) r.push_back(2);
    while (F % 5 == 0) { F /= 5; r.push_back(5); }
    return r;
}

// split L into pass factors: all but the last limited by max_a (mode A tiles), the last by
// max_last; fewest passes, then the most balanced split; 125*128 preferred for 16000
inline bool split_axis(int L, int max_a, int max_last, std::vector<int> *out)
{
    if (L <= max_last) { *out = {L}; return true; }
    for (int passes = 2; passes <= 4; ++passes) {
        std::vector<int> best;
        double best_score = -1;
        std::vector<int> cur;
        std::function<void(int, int)> rec = [&](int rem, int left) {
            if (left == 1) {
                if (rem <= max_last && rem >= 2) {
                    cur.push_back(rem);
                    int mn = 1 << 30;
                    for (int f : cur) mn = f < mn ? f : mn;
                    if (mn > best_score) { best_score = mn; best = cur; }
                    cur.pop_back();
                }
                return;
            }
            for (int f = 2; f <= max_a && f <= rem; ++f) {
                if (rem % f) continue;
                cur.push_back(f);
                rec(rem / f, left - 1);
                cur.pop_back();
            }
        };
        rec(L, passes);
        if (!best.empty()) { *out = best; return true; }
    }
    return false;
}

inline int pick_vshift(int F, int want)
{
    int vs = 0;
    while ((1 << (vs + 1)) <= want && (long)F * ((1 << (vs + 1)) + 1) <= kMaxTileElems) ++vs;
    return vs;
}

inline void choose_kernel(OipFftPass *p, int want_v)
{
    p->fast = -1;
    for (int i = 0; i < kNumFastKeys; ++i)
        if (kFastKeys[i].F == p->F && kFastKeys[i].mode == p->mode) {
            p->fast = i;
            p->vshift = kFastKeys[i].vshift;
            p->Vp = p->vshift > 1 ? (1 << p->vshift) + 1 : (1 << p->vshift);
            return;
        }
    p->vshift = pick_vshift(p->F, want_v);
    p->Vp = p->vshift ? (1 << p->vshift) + 1 : 1;
}

inline void fill_radix(OipFftPass *p)
{
    std::vector<int> r = radix_list(p->F);
    p->nradix = (int)r.size();
    for (int i = 0; i < p->nradix; ++i) p->radix[i] = r[i];
}

// dynamic LDS of a generic launch: two F x Vp tile buffers and the F stage twiddles
inline size_t generic_lds_bytes(const OipFftPass &p) { return 2 * sizeof(float) * ((size_t)2 * p.F * p.Vp + p.F); }

// LDS of a pass: the dynamic bytes of a generic launch (kGenericStaticLds of static arrays come on top); for a specialised
// kernel its one tile buffer and an upper bound of its two twiddle arrays (at most F stage twiddles, F inter-pass twiddles)
inline size_t pass_lds_bytes(const OipFftPass &p)
{
    if (p.fast < 0) return generic_lds_bytes(p);
    return 2 * sizeof(float) * ((size_t)p.F * p.Vp + p.F + (p.mode == 0 ? p.F : 1));
}

inline long pass_blocks(const OipFftPass &p)
{
    if (p.mode == 0) return (long)p.lane_tiles * p.O1 * p.O2;
    return (p.lanes + (1 << p.vshift) - 1) >> p.vshift;
}

// The list forms of the inverse column passes (oip_fft_col_list_pass) take a plan whose column passes all work on lane tiles of
// one width (the list names tiles of that width) and whose work items fit an int.
inline bool col_list_ok(const OipFftHostPlan &pl, int narr)
{
    if (pl.n_y < 1) return false;
    for (int i = 0; i < pl.n_y; ++i) {
        const OipFftPass &p = pl.passes[i];
        if (p.mode != 0 || p.axis != 1 || p.vshift != pl.passes[0].vshift || p.tw_mode == 1) return false;
        if ((long)narr * p.lane_tiles * p.O1 * p.O2 > 0x7fffffffL) return false;
    }
    return pl.passes[0].O2 == 1;       // the last inverse pass spans the whole axis
}

// What the launcher refuses of a planned pass: kPlanOk, or the code with its text in `why`.  A tw_mode 2 pass is a column
// pass with T = F S and O1 = S; its inter-pass twiddle rows are a [T / F][F] table of at most 16 MiB.
inline int launch_refusal(const OipFftPass &p, char *why, size_t len)
{
    if (p.tw_mode == 2 && (p.T % p.F != 0 || p.O1 != p.T / p.F || (long)p.T * 8 > (16L << 20))) {
        snprintf(why, len, "fft pass: no inter-pass twiddle rows for T = %d, F = %d", p.T, p.F);
        return kPlanRuntime;
    }
    const long blocks = pass_blocks(p);
    if (blocks <= 0 || blocks > 0x7fffffffL) { snprintf(why, len, "fft pass grid too large"); return kPlanUnsupported; }
    if (p.mode == 0 && (p.O1 > 65535 || p.O2 > 65535)) { snprintf(why, len, "fft pass: more than 65535 rows or blocks"); return kPlanUnsupported; }
    return kPlanOk;
}

// The plan of an M x N transform, or the planner's refusal: its code, and its text in `why`
inline int plan(int M, int N, OipFftHostPlan *out, char *why, size_t len)
{
    if (!smooth235(M) || !smooth235(N)) { snprintf(why, len, "fft2d: %d x %d is not 2^a3^b5^c", M, N); return kPlanInvalid; }
    if (M < 2) { snprintf(why, len, "fft2d: fewer than 2 rows"); return kPlanUnsupported; }
    OipFftHostPlan pl;
    pl.M = M; pl.N = N;
    // row pitch padded to whole 128-byte lines (16 complex): every pass stores full lines
    const int P = (N + 15) / 16 * 16;
    pl.P = P;
    if (!split_axis(N, kMaxLeadFactor, kMaxLastRowFactor, &pl.xf)) { snprintf(why, len, "fft2d: cannot factor row length %d", N); return kPlanUnsupported; }
    // 16000 = 128 * 125 with the 128-point pass first: its points are 125 rows apart, an odd multiple of
    // 512 B for the padded pitches, so a tile spreads over the HBM channels (125 * 128 would put all
    // points of a tile 47 * 2^16 B apart -- same channel -- and ran at half the bandwidth)
    if (M == 16000) pl.yf = std::vector<int>{128, 125};
    else if (M == 4000) pl.yf = std::vector<int>{32, 125};          // the band windows of 16000 correlation lines
    else if (!split_axis(M, kMaxLeadFactor, kMaxLastColFactor, &pl.yf)) { snprintf(why, len, "fft2d: cannot factor column length %d", M); return kPlanUnsupported; }
    // column (y) passes first: always mode A with lanes = x
    {
        int T = M;
        for (size_t i = 0; i < pl.yf.size(); ++i) {
            OipFftPass p;
            memset(&p, 0, sizeof p);
            p.F = pl.yf[i];
            p.M = M; p.N = N; p.P = P;
            p.axis = 1;
            fill_radix(&p);
            const int S = T / p.F;
            p.mode = 0;
            choose_kernel(&p, 32);
            p.nstride = (long)S * P;
            p.lanes = N;
            p.lane_tiles = (N + (1 << p.vshift) - 1) >> p.vshift;
            p.O1 = S;     p.o1_stride = P;              // j: row offset inside the block
            p.O2 = M / T; p.o2_stride = (long)T * P;    // blocks
            p.tw_mode = S > 1 ? 2 : 0; p.T = T; p.S = S;
            pl.passes.push_back(p);
            T = S;
        }
    }
    pl.n_y = (int)pl.passes.size();
    // row (x) passes: leading factors in mode A (lanes = j), last factor as whole contiguous
    // sub-rows in mode B
    {
        int T = N;
        for (size_t i = 0; i < pl.xf.size(); ++i) {
            OipFftPass p;
            memset(&p, 0, sizeof p);
            p.F = pl.xf[i];
            p.M = M; p.N = N; p.P = P;
            p.axis = 0;
            fill_radix(&p);
            const int S = T / p.F;
            p.T = T; p.S = S;
            if (S == 1) {
                p.mode = 1;
                choose_kernel(&p, 32);
                p.lanes = (long)M * (N / p.F);          // contiguous F-point vectors
                p.tw_mode = 0;
            } else {
                p.mode = 0;
                choose_kernel(&p, 32);
                p.nstride = S;
                p.lanes = S;
                p.lane_tiles = (S + (1 << p.vshift) - 1) >> p.vshift;
                p.O1 = N / T; p.o1_stride = T;          // blocks of the current sub-problem
                p.O2 = M;     p.o2_stride = P;          // rows
                p.tw_mode = 1;
            }
            pl.passes.push_back(p);
            T = S;
        }
    }
    for (auto &p : pl.passes)
        if (p.fast < 0 && (long)p.F * p.Vp > kMaxTileElems) { snprintf(why, len, "fft2d: factor %d too long for one LDS tile", p.F); return kPlanUnsupported; }
    *out = pl;
    return kPlanOk;
}

// One line per pass of the plan, in forward order (include/oip_c.h: oip_fft_plan_describe), or the refusal of the planner
// or of the launcher in its place.  Returns the code; kPlanInvalid with an empty text when `len` is too short.
inline int describe(int M, int N, char *buf, size_t len)
{
    if (!buf || len < 1) return kPlanInvalid;
    buf[0] = 0;
    OipFftHostPlan pl;
    int rc = plan(M, N, &pl, buf, len);
    if (rc) return rc;
    for (const OipFftPass &p : pl.passes)
        if ((rc = launch_refusal(p, buf, len))) return rc;
    size_t at = 0;
    for (const OipFftPass &p : pl.passes) {
        char radix[80] = "";
        int r = 0;
        for (int i = 0; i < p.nradix; ++i) r += snprintf(radix + r, sizeof radix - r, i ? ",%d" : "%d", p.radix[i]);
        const int n = snprintf(buf + at, len - at, "axis=%c F=%d mode=%d kind=%s vshift=%d Vp=%d radix=%s lds=%zu\n", p.axis ? 'y' : 'x', p.F,
                               p.mode, p.fast >= 0 ? "ct" : "generic", p.vshift, p.Vp, radix, pass_lds_bytes(p));
        if (n < 0 || (size_t)n >= len - at) { buf[0] = 0; return kPlanInvalid; }
        at += (size_t)n;
    }
    return kPlanOk;
}

}  // namespace oipfftplan
