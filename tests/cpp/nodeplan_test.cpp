// nodeplan_test.cpp -- the plans of the N-GPU host (csrc/oip_nodeplan.hpp) on the CPU, under ASan + UBSan: the invariants that
// Node::exchange_and_correlate (csrc/oip_multigpu.hpp) rests on, for the strips of tests/test_gpu_multigpu_loopback.py at
// N = 2, 3, 4.  The driver computes a rank's entirely local groups first and then, in posting order, the exchange groups it
// owns, each whole; that is every unit exactly once only if
//   - all units of a group have one owner;
//   - the local groups and exchange_groups() together cover every unit exactly once, in ascending order;
//   - a group is in exchange_groups() exactly when one of its units has a piece with src != dst;
//   - (9 x 2 at N = 2) the mixed pair (8, 9) -- unit 8 local, unit 9 not -- is one exchange group of rank 0;
// and the halo exchange addresses lines a rank holds only if the transfers never name src == dst and lie inside the source
// rank's block.  No HIP: the two *_src_range calls the halo plans ask are stand-ins here, the output rows +- a few lines.
#include <cstdio>

#include "oip_nodeplan.hpp"

static const long kHalo = 5;
extern "C" int oip_align_mss_src_range(long out_row0, long out_rows, long Lm, const double *, int, int, int line_offset, int overlap, int keep,
                                       int, long *first, long *last)
{
    const long shift = line_offset + (keep ? 0 : overlap);
    *first = std::max(0L, out_row0 + shift - kHalo);
    *last = std::min(Lm, out_row0 + out_rows + shift + kHalo);
    return OIP_OK;
}
extern "C" int oip_remap_shift_src_range(long out_row0, long out_rows, long L, double, int, long *first, long *last)
{
    *first = std::max(0L, out_row0 - kHalo);
    *last = std::min(L, out_row0 + out_rows + kHalo);
    return OIP_OK;
}

using namespace OIPGPU;

static int checks = 0, bad = 0;
#define CHECK(cond, ...) do { ++checks; if (!(cond)) { ++bad; printf("BAD %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } } while (0)

template <typename Plan> static void check_groups(const Plan &p, const char *name)
{
    const std::vector<ExchangeGroup> ex = p.exchange_groups();
    size_t next_ex = 0;
    int next_unit = 0, moved_groups = 0;
    for (int g = 0; g < p.n_groups(); ++g) {
        const std::vector<int> units = p.group_units(g);
        CHECK(!units.empty(), "%s N=%d group %d", name, p.world, g);
        bool moves = false;
        for (int u : units) {
            CHECK(u == next_unit++, "%s N=%d group %d: unit %d out of order", name, p.world, g, u);
            CHECK(p.group_of(u) == g, "%s N=%d unit %d", name, p.world, u);
            CHECK(p.assign[u] == p.assign[units[0]], "%s N=%d group %d: units %d and %d on ranks %d and %d", name, p.world, g, units[0], u,
                  p.assign[units[0]], p.assign[u]);
            bool unit_moves = false;
            for (const Piece &q : p.unit_pieces(u)) {
                CHECK(q.unit == u && q.dst == p.assign[u] && q.src >= 0 && q.src < p.world, "%s N=%d unit %d", name, p.world, u);
                unit_moves = unit_moves || q.src != q.dst;
            }
            CHECK(p.unit_is_local(u) == !unit_moves, "%s N=%d unit %d", name, p.world, u);
            moves = moves || unit_moves;
        }
        CHECK(p.group_is_local(g) == !moves, "%s N=%d group %d", name, p.world, g);
        // local, or the next exchange group: with all its units, and the pieces of those that move
        if (!moves) continue;
        ++moved_groups;
        CHECK(next_ex < ex.size() && ex[next_ex].units == units, "%s N=%d group %d is not exchange group %zu", name, p.world, g, next_ex);
        if (next_ex < ex.size()) {
            size_t n = 0;
            bool crosses = false;
            for (int u : units) if (!p.unit_is_local(u)) n += p.unit_pieces(u).size();
            for (const Piece &q : ex[next_ex].pieces) crosses = crosses || q.src != q.dst;
            CHECK(ex[next_ex].pieces.size() == n && crosses, "%s N=%d exchange group %zu: %zu pieces, %zu expected", name, p.world, next_ex,
                  ex[next_ex].pieces.size(), n);
        }
        ++next_ex;
    }
    CHECK(next_unit == p.n_units && next_ex == ex.size(), "%s N=%d: %d of %d units, %zu of %zu exchange groups", name, p.world, next_unit,
          p.n_units, next_ex, ex.size());
    CHECK(moved_groups > 0, "%s N=%d moves nothing: the case is vacuous", name, p.world);
    // what each rank computes, the way the driver walks it: every unit once
    std::vector<int> times(p.n_units, 0);
    for (int r = 0; r < p.world; ++r) {
        for (int u : p.units_of(r)) if (p.group_is_local(p.group_of(u))) ++times[u];
        for (const ExchangeGroup &g : ex) if (p.assign[g.units[0]] == r) for (int u : g.units) ++times[u];
    }
    for (int u = 0; u < p.n_units; ++u) CHECK(times[u] == 1, "%s N=%d unit %d computed %d times", name, p.world, u, times[u]);
}

static void check_transfers(const std::vector<LineTransfer> &tr, const std::vector<std::pair<long, long>> &need, long block, int world,
                            const char *name)
{
    CHECK(!tr.empty() && (int)need.size() == world, "%s N=%d: no halo line moves: the case is vacuous", name, world);
    for (const LineTransfer &t : tr) {
        CHECK(t.src != t.dst && t.src >= 0 && t.src < world && t.dst >= 0 && t.dst < world, "%s N=%d: %d -> %d", name, world, t.src, t.dst);
        CHECK(t.rows > 0 && t.row0 >= t.src * block && t.row0 + t.rows <= (t.src + 1) * block, "%s N=%d: lines [%ld, %ld) are not in rank %d's block",
              name, world, t.row0, t.row0 + t.rows, t.src);
        CHECK(t.row0 >= need[t.dst].first && t.row0 + t.rows <= need[t.dst].second, "%s N=%d: rank %d does not read lines [%ld, %ld)", name, world,
              t.dst, t.row0, t.row0 + t.rows);
    }
    // and nothing a rank reads outside its own block is left out
    for (int r = 0; r < world; ++r) {
        long lacking = std::max(0L, need[r].second - need[r].first) -
                       std::max(0L, std::min(need[r].second, (r + 1) * block) - std::max(need[r].first, r * block));
        for (const LineTransfer &t : tr) if (t.dst == r) lacking -= t.rows;
        CHECK(lacking == 0, "%s N=%d: rank %d lacks %ld lines after the exchange", name, world, r, lacking);
    }
}

int main()
{
    const double cy[12] = {0};
    std::vector<std::pair<long, long>> need;
    for (int n = 2; n <= 4; ++n) {
        const StripPlanC s81(1024, 33024, n, 8, 1, OIP_CORRELATION_LINES, 3000, 0, 100), s92(1024, 33024, n, 9, 2, OIP_CORRELATION_LINES, 3000, 0, 100);
        check_groups(s81, "strip 8x1");
        check_groups(s92, "strip 9x2");
        check_transfers(s81.align_transfers(cy, &need), need, s81.mb, n, "strip 8x1");
        check_transfers(s92.align_transfers(cy, &need), need, s92.mb, n, "strip 9x2");
        if (n == 2) {
            const std::vector<ExchangeGroup> ex = s92.exchange_groups();
            CHECK(ex.size() == 1 && ex[0].units == std::vector<int>({8, 9}) && s92.assign[8] == 0 && s92.assign[9] == 0,
                  "9x2 at N=2: %zu exchange groups", ex.size());
            CHECK(s92.unit_is_local(8) && !s92.unit_is_local(9), "9x2 at N=2: the pair (8, 9) is not mixed");
            for (const Piece &q : ex.empty() ? std::vector<Piece>() : ex[0].pieces) CHECK(q.unit == 9, "9x2 at N=2: a piece of unit %d moves", q.unit);
        }
        const CcdPlanC c(1024, 33024, n, 5, 1600, 64);
        check_groups(c, "ccd");
        check_transfers(c.remap_transfers(0.0, &need), need, c.pb, n, "ccd");
    }
    printf("%d checks, %d bad\n", checks, bad);
    return bad ? 1 : 0;
}
