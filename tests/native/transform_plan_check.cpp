// transform_plan_check.cpp -- the balance grid, the pool slices and the overlap test of the transforms of whole sets of tables
// (kpal_amd/csrc/transform_plan.hpp) as a CPU program: it answers the queries on its standard input, one line each, and knows
// no expected value -- those are the literals of tests/test_transform_plan_host.py.  Every argument is an unsigned integer,
// every answer too.
//   sizes                          -> kBalanceSetSlotsPerCu kBalanceSetThreads kBalanceSetSmallMaxK kPoolThreads kPoolUnroll
//                                     kPoolGroupsPerCu kPoolMinSliceTables kPoolOneSliceBins
//   items    TABLES NCANON         -> balance_set_items
//   slots    NUM_CU                -> balance_set_slots
//   grid     ITEMS SLOTS           -> balance_set_rounds balance_set_workgroups
//   shares   ITEMS SLOTS           -> smallest share, largest share, sum of the shares, over all workgroups of that grid
//   share    ITEMS GRID G          -> balance_set_share
//   shrinkl  K TABLES              -> kShrinkSetPerTableMinK shrink_set_launches
//   cols     BINS                  -> pool_column_pairs pool_column_groups
//   slices   TABLES BINS NUM_CU    -> pool_slices
//   slice    TABLES SLICES S       -> pool_slice_begin pool_slice_end
//   cover    TABLES SLICES         -> 1 if the slices are consecutive, begin at 0, end at TABLES and none is empty, else 0;
//                                     the shortest and the longest slice
//   pscratch SLICES BINS           -> pool_scratch_bytes
//   overlap  A ABYTES B BBYTES     -> transform_overlap
//   fit      TABLES BINS           -> transform_bytes_fit
// Test infrastructure.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../kpal_amd/csrc/transform_plan.hpp"

using namespace kpal;

int main()
{
    char what[16], line[512];
    int answered = 0;
    while (fgets(line, sizeof line, stdin)) {
        unsigned long long a[4] = {};
        int at = 0;
        if (sscanf(line, "%15s%n", what, &at) < 1) continue;
        const int got = sscanf(line + at, "%llu %llu %llu %llu", &a[0], &a[1], &a[2], &a[3]);
        if (!strcmp(what, "sizes") && got < 1)
            printf("%d %d %d %d %d %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", kBalanceSetSlotsPerCu, kBalanceSetThreads, kBalanceSetSmallMaxK, kPoolThreads,
                   kPoolUnroll, kPoolGroupsPerCu, kPoolMinSliceTables, kPoolOneSliceBins);
        else if (!strcmp(what, "items") && got == 2) printf("%" PRIu64 "\n", balance_set_items(a[0], a[1]));
        else if (!strcmp(what, "slots") && got == 1) printf("%" PRIu64 "\n", balance_set_slots(a[0]));
        else if (!strcmp(what, "grid") && got == 2) printf("%" PRIu64 " %" PRIu64 "\n", balance_set_rounds(a[0], a[1]), balance_set_workgroups(a[0], a[1]));
        else if (!strcmp(what, "shares") && got == 2) {
            const uint64_t grid = balance_set_workgroups(a[0], a[1]);
            uint64_t lo = UINT64_MAX, hi = 0, sum = 0;
            for (uint64_t g = 0; g < grid; ++g) {
                const uint64_t s = balance_set_share(a[0], grid, g);
                lo = s < lo ? s : lo;
                hi = s > hi ? s : hi;
                sum += s;
            }
            printf("%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", lo, hi, sum);
        } else if (!strcmp(what, "share") && got == 3) printf("%" PRIu64 "\n", balance_set_share(a[0], a[1], a[2]));
        else if (!strcmp(what, "shrinkl") && got == 2) printf("%d %" PRIu64 "\n", kShrinkSetPerTableMinK, shrink_set_launches((int)a[0], a[1]));
        else if (!strcmp(what, "cols") && got == 1) printf("%" PRIu64 " %" PRIu64 "\n", pool_column_pairs(a[0]), pool_column_groups(a[0]));
        else if (!strcmp(what, "slices") && got == 3) printf("%" PRIu64 "\n", pool_slices(a[0], a[1], a[2]));
        else if (!strcmp(what, "slice") && got == 3) printf("%" PRIu64 " %" PRIu64 "\n", pool_slice_begin(a[0], a[1], a[2]), pool_slice_end(a[0], a[1], a[2]));
        else if (!strcmp(what, "cover") && got == 2) {
            uint64_t expect = 0, lo = UINT64_MAX, hi = 0;
            int ok = 1;
            for (uint64_t s = 0; s < a[1]; ++s) {
                const uint64_t b = pool_slice_begin(a[0], a[1], s), e = pool_slice_end(a[0], a[1], s);
                if (b != expect || e <= b) ok = 0;
                expect = e;
                lo = e - b < lo ? e - b : lo;
                hi = e - b > hi ? e - b : hi;
            }
            if (expect != a[0]) ok = 0;
            printf("%d %" PRIu64 " %" PRIu64 "\n", ok, lo, hi);
        } else if (!strcmp(what, "pscratch") && got == 2) printf("%" PRIu64 "\n", pool_scratch_bytes(a[0], a[1]));
        else if (!strcmp(what, "overlap") && got == 4) printf("%d\n", transform_overlap(a[0], a[1], a[2], a[3]));
        else if (!strcmp(what, "fit") && got == 2) printf("%d\n", transform_bytes_fit(a[0], a[1]) ? 1 : 0);
        else {
            printf("bad query: %s", line);
            return 1;
        }
        ++answered;
    }
    printf("TRANSFORM_PLAN_DONE %d\n", answered);
    return 0;
}
