// Stand-alone driver of kpal_amd/csrc/nearest_plan.hpp for tests/test_nearest_plan_host.py (no GPU; built with the address and
// undefined-behaviour sanitizers).  One query per input line, one line of numbers per answer, then NEAREST_PLAN_DONE <count>.
//   plan CU bins route groups Q R budget capq capr -> tile_q tile_r tiles covered ascending indexable within capped max_bytes
//   kind balance positive smooth scale metric      -> route groups_per_slot
//   refused CU Q R bins                            -> partials_too_many of the one-call staged grid
//   order k d0 i0 ... d(k-1) i(k-1)                -> violations of "entry a precedes entry b" over all a < b (and b, a; a, a)
//   merge n have count first h.. (d i) c.. (d)     -> kept, then the kept (index) values
//   default                                        -> kNearestBudgetBytes
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "../../kpal_amd/csrc/nearest_plan.hpp"

using namespace kpal;

static double number(const std::string &w) { return w == "nan" ? std::nan("") : strtod(w.c_str(), nullptr); }

int main()
{
    std::string line;
    long answered = 0;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "plan") {
            int cu, route, Q, R, capq, capr;
            uint64_t bins, budget;
            uint32_t groups;
            in >> cu >> bins >> route >> groups >> Q >> R >> budget >> capq >> capr;
            const NearestKind kind = {route, groups};
            const NearestPlan plan = nearest_plan(bins, cu, kind, Q, R, budget, capq, capr);
            // cover: bands [q0, q1) follow each other from 0 to Q; within a band the tiles follow each other from 0 to R
            bool covered = !plan.tiles.empty() && plan.tiles.front().q0 == 0 && plan.tiles.front().r0 == 0, ascending = true;
            bool indexable = true, within = true, capped = true;
            uint64_t max_bytes = 0, area = 0;
            for (size_t t = 0; t < plan.tiles.size(); ++t) {
                const NearestTile &a = plan.tiles[t];
                if (!(a.q0 < a.q1 && a.r0 < a.r1 && a.q1 <= Q && a.r1 <= R)) covered = false;
                area += (uint64_t)(a.q1 - a.q0) * (uint64_t)(a.r1 - a.r0);
                if (t + 1 < plan.tiles.size()) {
                    const NearestTile &b = plan.tiles[t + 1];
                    if (a.r1 < R) {   // the band goes on
                        if (!(b.q0 == a.q0 && b.q1 == a.q1 && b.r0 == a.r1)) covered = false;
                        if (!(b.r0 > a.r0)) ascending = false;
                    } else if (!(b.q0 == a.q1 && b.r0 == 0)) covered = false;
                } else if (!(a.q1 == Q && a.r1 == R)) covered = false;
                const NearestCost cost = nearest_tile_cost(bins, cu, kind, a.q1 - a.q0, a.r1 - a.r0);
                indexable = indexable && cost.indexable;
                within = within && cost.bytes <= budget;
                max_bytes = std::max(max_bytes, cost.bytes);
                if ((capq > 0 && a.q1 - a.q0 > capq) || (capr > 0 && a.r1 - a.r0 > capr)) capped = false;
            }
            if (area != (uint64_t)Q * (uint64_t)R) covered = false;
            if ((uint64_t)Q * (uint64_t)R <= 4000000) {   // small enough: every pair counted
                std::vector<unsigned char> seen((size_t)Q * R, 0);
                for (const NearestTile &a : plan.tiles)
                    for (int q = a.q0; q < a.q1; ++q)
                        for (int r = a.r0; r < a.r1; ++r) ++seen[(size_t)q * R + r];
                for (unsigned char s : seen)
                    if (s != 1) covered = false;
            }
            printf("%d %d %zu %d %d %d %d %d %llu\n", plan.tile_q, plan.tile_r, plan.tiles.size(), (int)covered, (int)ascending, (int)indexable,
                   (int)within, (int)capped, (unsigned long long)max_bytes);
        } else if (what == "kind") {
            kpal_distance_options o = {};
            in >> o.do_balance >> o.do_positive >> o.do_smooth >> o.do_scale >> o.metric;
            const NearestKind kind = nearest_kind(&o);
            printf("%d %u\n", kind.route, kind.groups_per_slot);
        } else if (what == "refused") {
            int cu, Q, R;
            uint64_t bins;
            in >> cu >> Q >> R >> bins;
            const CrossSets c = {nullptr, nullptr, Q, R, bins, 0};
            const CrossGrid g = cross_grid(cu, c, cross_staged(Q, R, bins));
            printf("%d\n", (int)partials_too_many(g.slots, g.gx));
        } else if (what == "order") {
            int count;
            in >> count;
            std::vector<NearestCand> v(count);
            for (auto &c : v) {
                std::string d;
                in >> d >> c.index;
                c.dist = number(d);
            }
            long bad = 0;
            for (int a = 0; a < count; ++a) {
                if (nearest_before(v[a], v[a])) ++bad;
                for (int b = a + 1; b < count; ++b) bad += (nearest_before(v[a], v[b]) ? 0 : 1) + (nearest_before(v[b], v[a]) ? 1 : 0);
            }
            printf("%ld\n", bad);
        } else if (what == "merge") {
            int n, have;
            int64_t count, first;
            in >> n >> have >> count >> first;
            std::vector<NearestCand> best(n);
            for (int j = 0; j < have; ++j) {
                std::string d;
                in >> d >> best[j].index;
                best[j].dist = number(d);
            }
            std::vector<double> dist(count);
            for (auto &d : dist) {
                std::string w;
                in >> w;
                d = number(w);
            }
            const int kept = nearest_merge_host(best.data(), have, n, dist.data(), count, first);
            printf("%d", kept);
            for (int j = 0; j < kept; ++j) printf(" %lld", (long long)best[j].index);
            printf("\n");
        } else if (what == "default") {
            printf("%llu\n", (unsigned long long)kNearestBudgetBytes);
        } else {
            printf("unknown query %s\n", what.c_str());
            return 2;
        }
        ++answered;
    }
    printf("NEAREST_PLAN_DONE %ld\n", answered);
    return 0;
}
