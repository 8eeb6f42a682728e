// matrix_plan_check.cpp -- the host decisions and the finishing arithmetic of the distances of sets of profiles
// (kpal_amd/csrc/matrix_plan.hpp) as a CPU program: it answers the queries on its standard input, one line each, and knows no
// expected value -- those are the literals of tests/test_matrix_plan_host.py.  Numbers are read as integers but for `finish`,
// `gram` and `scale`; a double is printed with %.17g.
//   tiled    N                                            -> matrix_tiled
//   staged   Q R N                                        -> cross_staged
//   plain    POSITIVE SMOOTH SCALE METRIC                 -> options_plain
//   route    P N METRIC TILED_AGREED MFMA SUPER ALL RDIFF -> gram all all_wide staged recip
//   grid     NUM_CU Q R N TRI STAGED                      -> units gx slots sideR superR
//   toomany  GROUPS GX                                    -> partials_too_many
//   gram     NUM_CU P N                                   -> nd no gx_d gx_o, then the blocks I J ...
//   gramidx  NUM_CU P N I J                               -> gram_index
//   xgramidx BLOCKS_R Q R                                 -> cross_gram_index
//   xgramgx  NUM_CU NBLOCKS N                             -> cross_gram_gx
//   allgx    NUM_CU N WIDE                                -> matrix_all_gx
//   gxt      NUM_CU NPROF N                               -> option_totals_gx
//   nacc     METRIC SCALED POSITIVE                       -> option_nacc option_nacc_max
//   slot     TRI SIDE_R I J                               -> cross_slot
//   tri      I J                                          -> triangle_index
//   finish   METRIC SCALED S0 M0 S1 M1 S2 M2              -> finish_distance (M: unsigned 64-bit)
//   gramdist NORM_I NORM_J DOT                            -> gram_distance exact
//   scale    TL TR DOWN                                   -> ls rs
// Test infrastructure.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../kpal_amd/csrc/matrix_plan.hpp"

using namespace kpal;

int main()
{
    char what[16], line[512];
    int answered = 0;
    while (fgets(line, sizeof line, stdin)) {
        unsigned long long a[8] = {};
        double d[3] = {};
        int at = 0;
        if (sscanf(line, "%15s%n", what, &at) < 1) continue;
        const char *rest = line + at;
        const int got = sscanf(rest, "%llu %llu %llu %llu %llu %llu %llu %llu", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5], &a[6], &a[7]);
        if (!strcmp(what, "tiled") && got == 1) printf("%d\n", (int)matrix_tiled(a[0]));
        else if (!strcmp(what, "staged") && got == 3) printf("%d\n", (int)cross_staged((int)a[0], (int)a[1], a[2]));
        else if (!strcmp(what, "plain") && got == 4) {
            kpal_distance_options o = {};
            o.do_positive = (int)a[0];
            o.do_smooth = (int)a[1];
            o.do_scale = (int)a[2];
            o.metric = (int)a[3];
            printf("%d\n", (int)options_plain(&o));
        } else if (!strcmp(what, "route") && got == 8) {
            const MatrixSwitches sw = {a[4] != 0, a[5] != 0, a[6] != 0, a[7] != 0};
            const MatrixRoute r = matrix_route((int)a[0], a[1], (int)a[2], (int)a[3], sw);
            printf("%d %d %d %d %d\n", (int)r.gram, (int)r.all, (int)r.all_wide, (int)r.staged, (int)r.recip);
        } else if (!strcmp(what, "grid") && got == 6) {
            const CrossSets c = {nullptr, nullptr, (int)a[1], (int)a[2], a[3], (int)a[4]};
            const CrossGrid g = cross_grid((int)a[0], c, a[5] != 0);
            printf("%u %u %" PRIu64 " %d %d\n", g.units, g.gx, g.slots, g.sideR, g.superR);
        } else if (!strcmp(what, "toomany") && got == 2) printf("%d\n", (int)partials_too_many(a[0], (uint32_t)a[1]));
        else if (!strcmp(what, "gram") && got == 3) {
            const GramPlan g = gram_plan((int)a[0], (int)a[1], a[2]);
            printf("%u %u %u %u", g.nd, g.no, g.gx_d, g.gx_o);
            for (const GramBlock &b : g.blocks) printf(" %d %d", b.I, b.J);
            printf("\n");
        } else if (!strcmp(what, "gramidx") && got == 5) printf("%zu\n", gram_index(gram_plan((int)a[0], (int)a[1], a[2]), (int)a[3], (int)a[4]));
        else if (!strcmp(what, "xgramidx") && got == 3) printf("%zu\n", cross_gram_index((int)a[0], (int)a[1], (int)a[2]));
        else if (!strcmp(what, "xgramgx") && got == 3) printf("%u\n", cross_gram_gx((int)a[0], (uint32_t)a[1], a[2]));
        else if (!strcmp(what, "allgx") && got == 3) printf("%u\n", matrix_all_gx((int)a[0], a[1], a[2] != 0));
        else if (!strcmp(what, "gxt") && got == 3) printf("%u\n", option_totals_gx((int)a[0], (uint32_t)a[1], a[2]));
        else if (!strcmp(what, "nacc") && got == 3) printf("%u %u\n", option_nacc((int)a[0]), option_nacc_max((int)a[0], a[1] != 0, a[2] != 0));
        else if (!strcmp(what, "slot") && got == 4) {
            const CrossSets c = {nullptr, nullptr, 0, 0, 0, (int)a[0]};
            printf("%" PRIu64 "\n", cross_slot(c, (int)a[1], (int)a[2], (int)a[3]));
        } else if (!strcmp(what, "tri") && got == 2) printf("%zu\n", triangle_index((int)a[0], (int)a[1]));
        else if (!strcmp(what, "finish")) {
            Partial p[3] = {};
            if (sscanf(rest, "%llu %llu %lf %llu %lf %llu %lf %llu", &a[0], &a[1], &p[0].s, &p[0].m, &p[1].s, &p[1].m, &p[2].s, &p[2].m) != 8) return 1;
            printf("%.17g\n", finish_distance((int)a[0], a[1] != 0, p[0], p[1], p[2]));
        } else if (!strcmp(what, "gramdist")) {
            if (sscanf(rest, "%lf %lf %lf", &d[0], &d[1], &d[2]) != 3) return 1;
            bool exact = false;
            const double v = gram_distance(d[0], d[1], d[2], &exact);
            printf("%.17g %d\n", v, (int)exact);
        } else if (!strcmp(what, "scale")) {
            long long tl = 0, tr = 0;
            int down = 0;
            if (sscanf(rest, "%lld %lld %d", &tl, &tr, &down) != 3) return 1;
            double ls = 0.0, rs = 0.0;
            scale_factors(tl, tr, down != 0, &ls, &rs);
            printf("%.17g %.17g\n", ls, rs);
        } else {
            printf("bad query: %s", line);
            return 1;
        }
        ++answered;
    }
    printf("MATRIX_PLAN_DONE %d\n", answered);
    return 0;
}
