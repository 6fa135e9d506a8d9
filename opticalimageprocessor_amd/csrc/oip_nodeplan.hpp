// oip_nodeplan.hpp -- the plans of the N-GPU host (oip_multigpu.hpp) as pure arithmetic: which rank computes which
// correlation unit, which window pieces and halo lines move between the ranks' line blocks, and the `oip plan` printers.
// They mirror dist.py's assign_groups_by_cost / StripPlan / CcdPlan; tests/test_dist_cpu.py compares the two through `oip plan`.
// Nothing of HIP or RCCL in here (oip_c.h only declares the two *_src_range calls the halo plans ask): tests/cpp/nodeplan_test.cpp
// checks on the CPU the invariants that the host's exchange-and-correlate driver rests on.
#pragma once

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <stdexcept>
#include <utility>
#include <vector>

#include "oip_c.h"
#include "oip_corrgeom.h"

namespace OIPGPU {

struct Piece {
    int src, dst;
    int kind;           // 0 pan (or pan1), 1 mss (all four planes) (or pan2)
    int unit;
    long row0, rows;
    int col0, cols;
    long dst_row;
};
struct LineTransfer {
    int src, dst;
    long row0, rows;
};
// one of a unit's two windows: `rows` lines from row0 x `cols` columns from col0 x `planes` planes of a raster that is cut
// into blocks of `block` lines per rank
struct Window {
    long row0;
    int rows, col0, cols, planes;
    long block;
};
// the units computed together and the pieces of those among them that are not entirely on their rank
struct ExchangeGroup {
    std::vector<int> units;
    std::vector<Piece> pieces;
};

// ---- cost-aware placement (mirrors dist.py's assign_groups_by_cost operation by operation; integer microseconds) -----
// A group (a pair of inter-band units, or one CCD section) costs compute_us wherever it runs, plus the time to bring in the
// window bytes that rank lacks: they arrive over one xGMI link at bytes_per_us, one group after the other from time 0, under
// the resident groups' kernels; a rank computes its resident groups first, then the others in index order as they arrive.
// Every group starts where most of its bytes are; then single groups move, best move first, while a move lowers the ranks'
// finish times sorted from the latest down.  The constants are dist.py's (LINK_GBS etc.; unmeasured on hardware).
// OIP_LINK_GBS (an integer, GB/s) overrides the link figure in both hosts; `oip plan` prints what was used.
constexpr long kPairUs16000x3000 = 2500, kCcdSectionUs16000x200 = 150;
inline long link_gbs()
{
    const char *e = getenv("OIP_LINK_GBS");
    const long v = e ? atol(e) : 50;
    return v > 0 ? v : 50;
}

inline long rank_finish_us(const std::vector<long> &costs, long compute_us, long bytes_per_us)
{
    long t = 0, arrived = 0;
    for (long c : costs) if (c == 0) t += compute_us;
    for (long c : costs)
        if (c) {
            arrived += (c + bytes_per_us - 1) / bytes_per_us;
            t = std::max(t, arrived) + compute_us;
        }
    return t;
}

inline std::vector<int> assign_groups_by_cost(const std::vector<std::vector<long>> &missing, int world, long compute_us, long bytes_per_us,
                                              std::vector<long> *finish_out = nullptr)
{
    const int ng = (int)missing.size();
    std::vector<int> where(ng, 0);
    for (int g = 0; g < ng; ++g)
        for (int q = 1; q < world; ++q) if (missing[g][q] < missing[g][where[g]]) where[g] = q;
    auto finish = [&](int r, const std::vector<int> &w) {
        std::vector<long> costs;
        for (int g = 0; g < ng; ++g) if (w[g] == r) costs.push_back(missing[g][r]);
        return rank_finish_us(costs, compute_us, bytes_per_us);
    };
    std::vector<long> fin(world);
    for (int r = 0; r < world; ++r) fin[r] = finish(r, where);
    auto sorted_desc = [](std::vector<long> v) { std::sort(v.begin(), v.end(), std::greater<long>()); return v; };
    for (int it = 0; it < 4 * ng * world; ++it) {
        const std::vector<long> cur = sorted_desc(fin);
        bool have = false;
        std::vector<long> best_key, best_fin;
        int best_g = -1, best_q = -1;
        for (int g = ng - 1; g >= 0; --g) {
            const int r = where[g];
            for (int q = 0; q < world; ++q) {
                if (q == r) continue;
                std::vector<int> w2 = where;
                w2[g] = q;
                std::vector<long> f2 = fin;
                f2[r] = finish(r, w2);
                f2[q] = finish(q, w2);
                const std::vector<long> key = sorted_desc(f2);
                if (key < cur && (!have || key < best_key)) { have = true; best_key = key; best_fin = f2; best_g = g; best_q = q; }
            }
        }
        if (!have) break;
        where[best_g] = best_q;
        fin = best_fin;
    }
    if (finish_out) *finish_out = fin;
    return where;
}

// What the two plans share.  The kernels take GroupSize units per launch -- pairs (2k, 2k+1) of inter-band units, whose
// last digits depend on the partner, or single CCD sections -- so a group is placed, exchanged and computed as a whole.
// Plan gives world, n_units and unit_windows(u): the two windows (kind 0, kind 1) a unit reads.
template <typename Plan, int GroupSize> struct PlanUnits {
    std::vector<int> assign;
    std::vector<long> predicted_finish_us;
    const Plan &plan() const { return static_cast<const Plan &>(*this); }
    static int group_of(int u) { return u / GroupSize; }
    int n_groups() const { return (plan().n_units + GroupSize - 1) / GroupSize; }
    std::vector<int> group_units(int g) const
    {
        std::vector<int> v;
        for (int u = g * GroupSize; u < std::min((g + 1) * GroupSize, plan().n_units); ++u) v.push_back(u);
        return v;
    }
    // every group on the rank that finishes it soonest by the cost model; compute_us: what a group costs wherever it runs
    void place(long compute_us)
    {
        const int world = plan().world;
        std::vector<std::vector<long>> missing(n_groups(), std::vector<long>(world, 0));      // window bytes (u16) each rank lacks
        for (int u = 0; u < plan().n_units; ++u)
            for (const Window &w : plan().unit_windows(u))
                for (int q = 0; q < world; ++q) {
                    const long held = std::max(0L, std::min(w.row0 + w.rows, (q + 1) * w.block) - std::max(w.row0, q * w.block));
                    missing[group_of(u)][q] += (w.rows - held) * w.cols * w.planes * 2;
                }
        const std::vector<int> where = assign_groups_by_cost(missing, world, compute_us, link_gbs() * 1000, &predicted_finish_us);
        assign.resize(plan().n_units);
        for (int u = 0; u < plan().n_units; ++u) assign[u] = where[group_of(u)];
    }
    std::vector<int> units_of(int r) const
    {
        std::vector<int> v;
        for (int u = 0; u < plan().n_units; ++u) if (assign[u] == r) v.push_back(u);
        return v;
    }
    // a unit's windows cut at the ranks' block boundaries, each part on its way to the unit's rank
    std::vector<Piece> unit_pieces(int u) const
    {
        std::vector<Piece> out;
        const std::vector<Window> ws = plan().unit_windows(u);
        for (int kind = 0; kind < (int)ws.size(); ++kind)
            for (int r = 0; r < plan().world; ++r) {
                const Window &w = ws[kind];
                const long lo = std::max(w.row0, r * w.block), hi = std::min(w.row0 + w.rows, (r + 1) * w.block);
                if (lo < hi) out.push_back(Piece{r, assign[u], kind, u, lo, hi - lo, w.col0, w.cols, lo - w.row0});
            }
        return out;
    }
    bool unit_is_local(int u) const
    {
        for (const Piece &p : unit_pieces(u)) if (p.src != p.dst) return false;
        return true;
    }
    bool group_is_local(int g) const
    {
        for (int u : group_units(g)) if (!unit_is_local(u)) return false;
        return true;
    }
    // the groups that are not entirely local, in unit order: the posting order of the overlapped exchange (identical on all
    // ranks).  A local unit of such a group (odd slice count: a pair spans two sections) moves nothing and waits for its partner.
    std::vector<ExchangeGroup> exchange_groups() const
    {
        std::vector<ExchangeGroup> out;
        for (int g = 0; g < n_groups(); ++g) {
            if (group_is_local(g)) continue;
            out.push_back({group_units(g), {}});
            for (int u : out.back().units)
                if (!unit_is_local(u)) for (const Piece &p : unit_pieces(u)) out.back().pieces.push_back(p);
        }
        return out;
    }
    std::vector<Piece> correlation_pieces() const
    {
        std::vector<Piece> out;
        for (const ExchangeGroup &g : exchange_groups()) out.insert(out.end(), g.pieces.begin(), g.pieces.end());
        return out;
    }
};

// halo lines: rank r reads lines need[r] = [first, last) of a raster cut into blocks of `block` lines; what it lacks comes from
// the blocks' owners
inline std::vector<LineTransfer> line_transfers(const std::vector<std::pair<long, long>> &need, long block)
{
    std::vector<LineTransfer> out;
    const int world = (int)need.size();
    for (int r = 0; r < world; ++r)
        for (int q = 0; q < world; ++q) {
            if (q == r) continue;
            const long lo = std::max(need[r].first, q * block), hi = std::min(need[r].second, (q + 1) * block);
            if (lo < hi) out.push_back(LineTransfer{q, r, lo, hi - lo});
        }
    return out;
}

// the windows are InterBandGeom's (oip_corrgeom.h); the plan adds the ranks' line blocks and the alignment's parameters
struct StripPlanC : InterBandGeom, PlanUnits<StripPlanC, 2> {
    int world, lps, line_offset, overlap, keep, min_lines, halo_cap;
    long Lm, pb, mb, out_rows;

    StripPlanC(int W_, long Lp_total, int world_, int slices_ = OIP_IBCV_DEF_SLICES, int sections_ = OIP_IBCV_DEF_SECTIONS,
               int corr = OIP_CORRELATION_LINES, int lps_ = OIP_IBPA_DEFAULT_BATCHLINES, int line_offset_ = 0,
               int overlap_ = OIP_IBPA_DEFAULT_LINEOVERLAP, bool keep_ = false, int min_lines_ = OIP_IBPA_MIN_PROCESSLINES,
               int halo_cap_ = 64)
        : InterBandGeom(W_, Lp_total, slices_, sections_, corr), world(world_), lps(lps_),
          line_offset(line_offset_), overlap(overlap_), keep(keep_), min_lines(min_lines_), halo_cap(halo_cap_)
    {
        if (Lp_total % (4L * world)) throw std::invalid_argument("PAN line count must be a multiple of 4 x the GPU count");
        if (sections > 1 && (long)sections * corr > Lp_total)                         // preproc.h:234-237, in the plan's own words
            throw std::invalid_argument("CalcInterBandCorrelation: too many sections, not enough total PAN data lines");
        Lm = Lp / 4; pb = Lp / world; mb = pb / 4;
        out_rows = Lm - line_offset - (keep ? 0 : overlap);
        place(std::max(1L, kPairUs16000x3000 * base_rows * base_cols / (16000L * 3000L)));
    }
    std::vector<Window> unit_windows(int u) const                                     // the PAN window, the four MSS band windows
    {
        const int sec = u / slices, i = u % slices;
        return {{pan_start(sec), base_rows, i * base_cols, base_cols, 1, pb}, {mss_start(sec), band_rows, i * band_cols, band_cols, OIP_MSS_BANDS, mb}};
    }
    void align_out_rows(int r, long *o0, long *o1) const
    {
        const long shift = line_offset + (keep ? 0 : overlap);
        const long b0 = r * mb, b1 = (r + 1) * mb;
        *o0 = r == 0 ? 0 : std::min(std::max(b0 - shift, 0L), out_rows);
        *o1 = r == world - 1 ? out_rows : std::min(std::max(b1 - shift, 0L), out_rows);
        if (*o1 < *o0) *o1 = *o0;
    }
    // need[r] = [first, last) MSS lines rank r's output rows read
    std::vector<LineTransfer> align_transfers(const double *cy, std::vector<std::pair<long, long>> *need) const
    {
        need->clear();
        for (int r = 0; r < world; ++r) {
            long o0, o1, f = 0, l = 0;
            align_out_rows(r, &o0, &o1);
            if (o1 > o0 && oip_align_mss_src_range(o0, o1 - o0, Lm, cy, Wb, lps, line_offset, overlap, keep, min_lines, &f, &l) != OIP_OK)
                throw std::runtime_error("oip_align_mss_src_range failed");
            need->push_back({f, l});
        }
        return line_transfers(*need, mb);
    }
};

// the windows are CcdGeom's (oip_corrgeom.h); the plan adds the ranks' line blocks and the remap's section length
struct CcdPlanC : CcdGeom, PlanUnits<CcdPlanC, 1> {
    int world, section_rows, n_units;
    long pb;

    CcdPlanC(int W_, long L_, int world_, int sections_ = OIP_STT_DEF_SECTIONS, int lps_ = OIP_STT_DEF_SECLINES,
             int ov_ = OIP_STT_DEF_OVERLAPPX, int edge_ = 0, int section_rows_ = OIP_REMAP_SECTION_ROWS)
        : CcdGeom(W_, L_, sections_, lps_, ov_, edge_), world(world_), section_rows(section_rows_), n_units(sections_), pb(L_ / world_)
    {
        if (L % world) throw std::invalid_argument("line count must be a multiple of the GPU count");
        if (L < (long)sections * rows) throw std::invalid_argument(kCcdTooFewLines);
        place(std::max(1L, kCcdSectionUs16000x200 * rows * cols / (16000L * 200L)));
    }
    std::vector<Window> unit_windows(int u) const                                     // stitcher.h:175-176: PAN1, PAN2
    {
        return {{section_start(u), rows, col1, cols, 1, pb}, {section_start(u), rows, col2, cols, 1, pb}};
    }
    std::vector<LineTransfer> remap_transfers(double dy, std::vector<std::pair<long, long>> *need) const
    {
        need->clear();
        for (int r = 0; r < world; ++r) {
            long f = 0, l = 0;
            if (oip_remap_shift_src_range(r * pb, pb, L, dy, section_rows, &f, &l) != OIP_OK)
                throw std::runtime_error("oip_remap_shift_src_range failed");
            need->push_back({f, l});
        }
        return line_transfers(*need, pb);
    }
};

// `oip plan`: the plans as JSON, for the test that compares them with dist.py's
template <typename T, typename F> void print_list(const std::vector<T> &v, F item)
{
    printf("[");
    for (size_t i = 0; i < v.size(); ++i) { if (i) printf(","); item(v[i]); }
    printf("]");
}
template <typename Plan> void print_plan_head(const Plan &p)
{
    printf("{\"assign\":");
    print_list(p.assign, [](int a) { printf("%d", a); });
    printf(",\"pieces\":");
    print_list(p.correlation_pieces(), [](const Piece &q) {
        printf("[%d,%d,%d,%d,%ld,%ld,%d,%d,%ld]", q.src, q.dst, q.kind, q.unit, q.row0, q.rows, q.col0, q.cols, q.dst_row);
    });
}
inline void print_transfers(const char *name, const std::vector<LineTransfer> &tr)
{
    printf(",\"%s\":", name);
    print_list(tr, [](const LineTransfer &t) { printf("[%d,%d,%ld,%ld]", t.src, t.dst, t.row0, t.rows); });
}
inline void print_row_ranges(const char *name, const std::vector<std::pair<long, long>> &v)
{
    printf(",\"%s\":", name);
    print_list(v, [](const std::pair<long, long> &a) { printf("[%ld,%ld]", a.first, a.second); });
}
template <typename Plan> void print_plan_tail(const Plan &p)
{
    printf(",\"link_gbs\":%ld,\"predicted_finish_us\":", link_gbs());
    print_list(p.predicted_finish_us, [](long us) { printf("%d", (int)us); });
    printf("}\n");
}
inline void PrintStripPlan(const StripPlanC &p, const double *cy)
{
    std::vector<std::pair<long, long>> rows(p.world), need;
    for (int r = 0; r < p.world; ++r) p.align_out_rows(r, &rows[r].first, &rows[r].second);
    print_plan_head(p);
    print_row_ranges("align_rows", rows);
    print_transfers("align_transfers", p.align_transfers(cy, &need));
    print_plan_tail(p);
}
inline void PrintCcdPlan(const CcdPlanC &p, double dy)
{
    std::vector<std::pair<long, long>> need;
    print_plan_head(p);
    print_transfers("remap_transfers", p.remap_transfers(dy, &need));
    print_row_ranges("need", need);
    print_plan_tail(p);
}

}  // namespace OIPGPU
