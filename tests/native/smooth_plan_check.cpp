// smooth_plan_check.cpp -- the pyramid layout, the scratch size and the route of dynamic smoothing over sets of profiles
// (kpal_amd/csrc/smooth_plan.hpp) as a CPU program: it answers the queries on its standard input, one line each, and knows no
// expected value -- those are the literals of tests/test_smooth_plan_host.py.  Every number is an unsigned integer.
//   nodes    K                            -> smooth_nodes
//   stride   K                            -> smooth_stride
//   level    K H                          -> smooth_level_offset smooth_level_nodes
//   element  K E                          -> height node (height -1: padding)
//   scratch  K NPROF                      -> smooth_scratch_bytes
//   batched  K Q R DO_POSITIVE BUDGET     -> smooth_batched
//   budget                                -> kSmoothBudgetBytes
// Test infrastructure.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../kpal_amd/csrc/smooth_plan.hpp"

using namespace kpal;

int main()
{
    char what[16], line[512];
    int answered = 0;
    while (fgets(line, sizeof line, stdin)) {
        unsigned long long a[5] = {};
        int at = 0;
        if (sscanf(line, "%15s%n", what, &at) < 1) continue;
        const int got = sscanf(line + at, "%llu %llu %llu %llu %llu", &a[0], &a[1], &a[2], &a[3], &a[4]);
        if (!strcmp(what, "nodes") && got == 1) printf("%" PRIu64 "\n", smooth_nodes((int)a[0]));
        else if (!strcmp(what, "stride") && got == 1) printf("%" PRIu64 "\n", smooth_stride((int)a[0]));
        else if (!strcmp(what, "level") && got == 2) printf("%" PRIu64 " %" PRIu64 "\n", smooth_level_offset((int)a[0], (int)a[1]), smooth_level_nodes((int)a[0], (int)a[1]));
        else if (!strcmp(what, "element") && got == 2) {
            const SmoothElement e = smooth_element((int)a[0], a[1]);
            printf("%d %" PRIu64 "\n", e.height, e.node);
        } else if (!strcmp(what, "scratch") && got == 2) printf("%" PRIu64 "\n", smooth_scratch_bytes((int)a[0], a[1]));
        else if (!strcmp(what, "batched") && got == 5) printf("%d\n", (int)smooth_batched((int)a[0], (int)a[1], (int)a[2], a[3] != 0, a[4]));
        else if (!strcmp(what, "budget") && got < 1) printf("%" PRIu64 "\n", kSmoothBudgetBytes);
        else {
            printf("bad query: %s", line);
            return 1;
        }
        ++answered;
    }
    printf("SMOOTH_PLAN_DONE %d\n", answered);
    return 0;
}
