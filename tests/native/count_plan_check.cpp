// count_plan_check.cpp -- the host decisions of the counting front end (kpal_amd/csrc/count_plan.hpp) as a CPU program: it
// answers the queries on its standard input, one line each, and knows no expected value -- those are the literals of
// tests/test_count_plan_host.py.  argv: the four constants of the kernel headers (PlanLimits).
//   resolve  REQUESTED K                                  -> strategy, or the (negative) error code
//   strategy RESOLVED IS_AUTO K N FRESH_CANDIDATE         -> strategy of the piece
//   piece    STRATEGY K N NUM_CU BATCH_BYTES BATCH_SET    -> bytes per piece
//   grid     STEPS NUM_CU BLOCKS_PER_CU WAVES_PER_BLOCK   -> steps per wave, workgroups
// Test infrastructure.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../kpal_amd/csrc/count_plan.hpp"

using namespace kpal;

int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    const PlanLimits lim = {strtoull(argv[1], nullptr, 10), strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10), strtoull(argv[4], nullptr, 10)};
    char what[16];
    unsigned long long a[6];
    char line[256];
    int answered = 0;
    while (fgets(line, sizeof line, stdin)) {
        const int got = sscanf(line, "%15s %llu %llu %llu %llu %llu %llu", what, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]);
        if (got < 1) continue;
        if (!strcmp(what, "resolve") && got == 3) printf("%d\n", plan_resolve((int)a[0], (int)a[1]));
        else if (!strcmp(what, "strategy") && got == 6) printf("%d\n", plan_strategy((int)a[0], a[1] != 0, (int)a[2], (size_t)a[3], a[4] != 0));
        else if (!strcmp(what, "piece") && got == 7)
            printf("%zu\n", plan_piece_bytes((int)a[0], (int)a[1], (size_t)a[2], (int)a[3], (size_t)a[4], a[5] != 0, lim));
        else if (!strcmp(what, "grid") && got == 5) {
            const WaveGrid w = wave_grid(a[0], (int)a[1], (int)a[2], (int)a[3]);
            printf("%" PRIu64 " %u\n", w.spw, w.grid);
        } else {
            printf("bad query: %s", line);
            return 1;
        }
        ++answered;
    }
    printf("COUNT_PLAN_DONE %d\n", answered);
    return 0;
}
