// pair_smooth_plan_check.cpp -- the items, the grid, the partial layout, the chunks and the table indices of dynamic smoothing over
// linked pairs (kpal_amd/csrc/pair_smooth_plan.hpp) as a CPU program: it answers the queries on its standard input, one line each,
// and knows no expected value -- those are the literals and the rules of tests/test_pair_smooth_plan_host.py.  Every argument is
// an integer, every answer too.
//   sizes                          -> kPairSmoothSliceNodes kSmoothBudgetBytes kSmoothElementBytes
//   slices   K                     -> pair_smooth_bin_slices pair_smooth_node_slices pair_smooth_slices smooth_stride
//   nodes    K                     -> 1 if the node slices are consecutive, begin at 0, end at smooth_stride(K), none is empty and
//                                     every bound is even, else 0; the height of the first element of the last node slice
//                                     (smooth_element; -1: padding) and the number of elements of that slice
//   walk     K N NUM_CU            -> pair_smooth_units pair_smooth_workgroups; 1 if the grid is within the slots and the units,
//                                     the shares of the workgroups sum to the units and differ by at most one, else 0
//   partial  K N NACC              -> 1 if pair_set_partial over pair_smooth_slices(K) is a bijection onto [0, NACC * N * slices)
//                                     (enumerated up to 2^22 values, else checked at both ends and 4096 places between); that size
//   chunk    K N BALANCE CHUNK ALIAS LAG -> pair_smooth_chunk, pair_set_tables of that chunk, smooth_scratch_bytes of those
//   tables   CHUNK ALIAS LAG PAIR  -> pair_set_union pair_set_tables pair_smooth_left pair_smooth_right
//   batched  SMOOTH POSITIVE       -> pair_smooth_batched
// Test infrastructure.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kpal_amd/csrc/pair_smooth_plan.hpp"

using namespace kpal;

int main()
{
    char what[16], line[512];
    int answered = 0;
    while (fgets(line, sizeof line, stdin)) {
        long long a[6] = {};
        int at = 0;
        if (sscanf(line, "%15s%n", what, &at) < 1) continue;
        const int got = sscanf(line + at, "%lld %lld %lld %lld %lld %lld", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]);
        const int k = a[0] >= 1 && a[0] <= 16 ? (int)a[0] : 0;   // (of the queries whose first word is K)
        if (!strcmp(what, "sizes") && got < 1) printf("%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", kPairSmoothSliceNodes, kSmoothBudgetBytes, kSmoothElementBytes);
        else if (!strcmp(what, "slices") && got == 1 && k)
            printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", pair_smooth_bin_slices(k), pair_smooth_node_slices(k), pair_smooth_slices(k), smooth_stride(k));
        else if (!strcmp(what, "nodes") && got == 1 && k) {
            const uint64_t slices = pair_smooth_node_slices(k);
            uint64_t next = 0, b = 0, e = 0;
            int ok = 1;
            for (uint64_t s = 0; s < slices; ++s) {
                b = pair_smooth_node_begin(s);
                e = pair_smooth_node_end(k, s);
                ok = ok && b == next && e > b && b % 2 == 0 && e % 2 == 0;
                next = e;
            }
            printf("%d %d %" PRIu64 "\n", ok && next == smooth_stride(k), smooth_element(k, b).height, e - b);
        } else if (!strcmp(what, "walk") && got == 3 && k) {
            const uint64_t n = (uint64_t)a[1], units = pair_smooth_units(n, k), grid = pair_smooth_workgroups(n, k, (uint64_t)a[2]);
            uint64_t lo = UINT64_MAX, hi = 0, sum = 0;
            for (uint64_t g = 0; g < grid; ++g) {
                const uint64_t s = balance_set_share(units, grid, g);
                lo = s < lo ? s : lo;
                hi = s > hi ? s : hi;
                sum += s;
            }
            printf("%" PRIu64 " %" PRIu64 " %d\n", units, grid, grid >= 1 && grid <= units && grid <= pair_set_slots((uint64_t)a[2]) && sum == units && hi - lo <= 1);
        } else if (!strcmp(what, "partial") && got == 3 && k) {
            const uint64_t n = (uint64_t)a[1], nacc = (uint64_t)a[2], slices = pair_smooth_slices(k), size = nacc * n * slices;
            int ok = 1;
            if (size <= (1ULL << 22)) {
                std::vector<uint8_t> seen(size, 0);
                for (uint64_t c = 0; c < nacc; ++c)
                    for (uint64_t p = 0; p < n; ++p)
                        for (uint64_t s = 0; s < slices; ++s) {
                            const uint64_t i = pair_set_partial(c, n, slices, p, s);
                            if (i >= size || seen[i]++) ok = 0;
                        }
                for (uint64_t i = 0; i < size; ++i) ok = ok && seen[i] == 1;
            } else {
                for (uint64_t j = 0; j <= 4097; ++j) {
                    const uint64_t i = j == 4097 ? size - 1 : (size / 4097) * j;
                    ok = ok && pair_set_partial(i / slices / n, n, slices, (i / slices) % n, i % slices) == i;
                }
            }
            printf("%d %" PRIu64 "\n", ok, size);
        } else if (!strcmp(what, "chunk") && got == 6 && k) {
            const uint64_t c = pair_smooth_chunk(k, (uint64_t)a[1], a[2] != 0, (uint64_t)a[3], (int)a[4], (int64_t)a[5]);
            const uint64_t t = pair_set_tables(c, (int)a[4], (int64_t)a[5]);
            printf("%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", c, t, smooth_scratch_bytes(k, t));
        } else if (!strcmp(what, "tables") && got == 4)
            printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", pair_set_union((uint64_t)a[0], (int)a[1], (int64_t)a[2]),
                   pair_set_tables((uint64_t)a[0], (int)a[1], (int64_t)a[2]), pair_smooth_left((uint64_t)a[0], (int)a[1], (int64_t)a[2], (uint64_t)a[3]),
                   pair_smooth_right((uint64_t)a[0], (int)a[1], (int64_t)a[2], (uint64_t)a[3]));
        else if (!strcmp(what, "batched") && got == 2) printf("%d\n", pair_smooth_batched(a[0] != 0, a[1] != 0) ? 1 : 0);
        else {
            printf("bad query: %s", line);
            return 2;
        }
        ++answered;
    }
    printf("PAIR_SMOOTH_PLAN_DONE %d\n", answered);
    return 0;
}
