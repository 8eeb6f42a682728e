// quad_plan_check.cpp -- the host decisions of the quad record pipelines (kpal_amd/csrc/quad_plan.hpp) as a CPU program: it
// answers the queries on its standard input (blank-separated words, a query may span lines), one line each, and knows no
// expected value -- those are the literals and the restatement of tests/test_quad_plan_host.py.  Doubles are printed with 17
// digits.  One QuadTileCache lives as long as the program.
//   grid     TOTAL_STEPS                            -> groups stride sample_steps sampled_steps
//   geo1     TOTAL_STEPS STEPS NUM_CU               -> too_large tiles G tpb pool_bytes
//   geo2     K TOTAL_STEPS STEPS1 STEPS2 NUM_CU     -> too_large1 NB1 REP S1 tiles1 G1 tpb1 cap1 pool1_bytes
//                                                      too_large2 units G2 upw unit_cap tiles2 cap2 pool2_bytes nseg
//   verdict  BUCKETS NFINE(0 | 512) REPEAT_ITEMS SAMPLED_STEPS IS_AUTO  ROW_LOADS... FINE_LOADS...
//            -> use_chunked budget hot_rows hot_percent top3_percent  n loads[0] loads[n-1] sorted  nfine fine[0] fine[nfine-1] sorted
//   backlog  SLOTS N MU...                          -> expected backlog
//   walk1    SLOTS BUDGET NC CANDIDATES... N LOADS...  -> steps tried backlog...
//   walk2    STEPS1 N FINE...                       -> steps2
//   forced   FORCED NC CANDIDATES...                -> steps or 0
//   tile1    STEPS SAMPLED HOT_ROWS STEPS_FORCED REPEAT_FORCED  -> steps repeat counted
//   tile2    FORCED1 CHOSEN HOT_ROWS REPEAT_FORCED  -> steps repeat counted
//   hit      FEED_BYTES LEVELS                      -> 0 | 1
//   store    STEPS1 STEPS2 FEED_BYTES | hot V | clear   -> steps1 steps2 uses bytes hot_rows
// Test infrastructure.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../kpal_amd/csrc/quad_plan.hpp"

using namespace kpal;

static bool word(char *w)
{
    return scanf("%31s", w) == 1;
}

static long long integer()
{
    long long v = 0;
    if (scanf("%lld", &v) != 1) exit(3);
    return v;
}

static double real()
{
    double v = 0;
    if (scanf("%lf", &v) != 1) exit(3);
    return v;
}

static std::vector<double> reals()
{
    std::vector<double> v((size_t)integer());
    for (double &x : v) x = real();
    return v;
}

static std::vector<int> integers()
{
    std::vector<int> v((size_t)integer());
    for (int &x : v) x = (int)integer();
    return v;
}

template <class V>
static int sorted(const V &v)
{
    return std::is_sorted(v.begin(), v.end()) ? 1 : 0;
}

int main()
{
    char what[32];
    int answered = 0;
    QuadTileCache cache;
    while (word(what)) {
        if (!strcmp(what, "grid")) {
            const QuadSampleGrid g = quad_sample_grid((uint64_t)integer());
            printf("%u %" PRIu64 " %u %" PRIu64 "\n", g.groups, g.stride, g.sample_steps, g.sampled_steps);
        } else if (!strcmp(what, "geo1")) {
            const uint64_t total = (uint64_t)integer();
            const int steps = (int)integer(), cu = (int)integer();
            const Quad1Geometry g = quad1_geometry(total, steps, cu);
            printf("%d %" PRIu64 " %u %" PRIu64 " %zu\n", (int)g.too_large, g.tiles, g.G, g.tpb, g.pool_bytes);
        } else if (!strcmp(what, "geo2")) {
            const int k = (int)integer();
            const uint64_t total = (uint64_t)integer();
            const int steps1 = (int)integer(), steps2 = (int)integer(), cu = (int)integer();
            const Quad2Level1 a = quad2_level1(k, total, steps1, cu);
            const Quad2Level2 b = quad2_level2(a, steps2, cu);
            const Quad2Rows r = quad2_rows(k);
            if (r.NB1 != a.NB1 || r.REP != a.REP || r.S1 != a.S1) return 4;
            printf("%d %u %u %u %" PRIu64 " %u %" PRIu64 " %" PRIu64 " %zu  %d %u %u %u %" PRIu64 " %" PRIu64 " %" PRIu64 " %zu %u\n", (int)a.too_large,
                   a.NB1, a.REP, a.S1, a.tiles1, a.G1, a.tpb1, a.cap1, a.pool1_bytes, (int)b.too_large, b.units, b.G2, b.upw, b.unit_cap, b.tiles2, b.cap2,
                   b.pool2_bytes, b.nseg);
        } else if (!strcmp(what, "verdict")) {
            const int buckets = (int)integer(), nfine = (int)integer();
            const uint32_t repeat_items = (uint32_t)integer();
            const uint64_t sampled = (uint64_t)integer();
            const bool is_auto = integer() != 0;
            if (nfine != 0 && nfine != kQuadFineRows) return 4;
            std::vector<uint32_t> h((size_t)(buckets + nfine));
            for (uint32_t &x : h) x = (uint32_t)integer();
            const QuadVerdict v = quad_sample_verdict(h.data(), buckets, nfine ? h.data() + buckets : nullptr, repeat_items, sampled, is_auto);
            printf("%d %.17g %d %.17g %.17g  %zu %.17g %.17g %d  %zu %.17g %.17g %d\n", (int)v.use_chunked, v.budget, (int)v.hot_rows, v.hot_percent,
                   v.top3_percent, v.loads.size(), v.loads.front(), v.loads.back(), sorted(v.loads), v.fine.size(), v.fine.empty() ? 0.0 : v.fine.front(),
                   v.fine.empty() ? 0.0 : v.fine.back(), sorted(v.fine));
        } else if (!strcmp(what, "backlog")) {
            const int slots = (int)integer();
            printf("%.17g\n", quad_expected_backlog(reals(), slots));
        } else if (!strcmp(what, "walk1")) {
            const int slots = (int)integer();
            const double budget = real();
            const std::vector<int> cand = integers();
            const QuadWalk w = quad_walk_level1(reals(), slots, cand.data(), cand.size(), budget);
            printf("%d %zu", w.steps, w.tried);
            for (size_t i = 0; i < w.tried; ++i) printf(" %.17g", w.backlog[i]);
            printf("\n");
        } else if (!strcmp(what, "walk2")) {
            const int steps1 = (int)integer();
            printf("%d\n", quad_walk_level2(reals(), steps1));
        } else if (!strcmp(what, "forced")) {
            const int forced = (int)integer();
            const std::vector<int> cand = integers();
            printf("%d\n", quad_forced_steps(forced, cand.data(), cand.size()));
        } else if (!strcmp(what, "tile1")) {
            const int steps = (int)integer(), sampled = (int)integer(), hot = (int)integer(), forced = (int)integer(), repeat_forced = (int)integer();
            const QuadTile t = quad1_tile(steps, sampled != 0, hot != 0, forced, repeat_forced);
            printf("%d %d %d\n", t.steps, (int)t.repeat, (int)t.counted);
        } else if (!strcmp(what, "tile2")) {
            const int forced1 = (int)integer(), chosen = (int)integer(), hot = (int)integer(), repeat_forced = (int)integer();
            const QuadTile t = quad2_tile1(forced1, chosen, hot != 0, repeat_forced);
            printf("%d %d %d\n", t.steps, (int)t.repeat, (int)t.counted);
        } else if (!strcmp(what, "hit")) {
            const size_t bytes = (size_t)integer();
            printf("%d\n", (int)cache.hit(bytes, (int)integer()));
        } else if (!strcmp(what, "store") || !strcmp(what, "hot") || !strcmp(what, "clear")) {
            if (what[0] == 's') {
                const int s1 = (int)integer(), s2 = (int)integer();
                cache.store(s1, s2, (size_t)integer());
            } else if (what[0] == 'h') cache.hot_rows = integer() != 0;
            else cache.clear();
            printf("%d %d %u %zu %d\n", cache.steps1, cache.steps2, cache.uses, cache.bytes, (int)cache.hot_rows);
        } else {
            printf("bad query: %s\n", what);
            return 1;
        }
        ++answered;
    }
    printf("QUAD_PLAN_DONE %d\n", answered);
    return 0;
}
