// pair_set_plan_check.cpp -- the items, the grid, the partial layout, the chunks and the alias test of the distances of linked
// pairs (kpal_amd/csrc/pair_set_plan.hpp) as a CPU program: it answers the queries on its standard input, one line each, and
// knows no expected value -- those are the literals and the rules of tests/test_pair_set_plan_host.py.  Every argument is an
// integer, every answer too.
//   sizes                          -> kPairSetThreads kPairSetWaves kPairSetUnroll kPairSetSliceBins kPairSetWaveMaxBins
//                                     kPairSetSlotsPerCu kPairSetBalanceBytes kPairSetMaxAcc
//   slices   K                     -> pair_set_slices(4^K) pair_set_wave_form(4^K)
//   tile     K                     -> 1 if the slices are consecutive, begin at 0, end at 4^K, none is empty and every bound is a
//                                     multiple of two bins (16 bytes), else 0; the shortest and the longest slice
//   walk     K N NUM_CU            -> pair_set_units pair_set_workgroups; 1 if the round-robin walk of that grid (every wave of
//                                     every unit of every workgroup) reaches every (pair, slice) item exactly once and nothing
//                                     else, else 0; the smallest and the largest number of units of a workgroup.  Past 2^23
//                                     items the walk is not enumerated: the shares must sum to the units and unit <-> item must
//                                     round-trip at both ends and at 4096 units spread between
//   partial  K N NACC              -> 1 if pair_set_partial is a bijection onto [0, NACC * N * slices) (enumerated up to 2^23
//                                     values, else: strictly increasing in (acc, pair, slice) order at both ends and at 4096
//                                     places between, first 0, last the size - 1), else 0; that size
//   chunk    K N BALANCE CHUNK     -> pair_set_chunk pair_set_chunks(N, that)
//   alias    LEFT RIGHT N BINS     -> pair_set_alias, lag (signed)
//   union    CHUNK LAG             -> pair_set_union_tables (LAG signed)
//   bbytes   CHUNK BINS UNION      -> pair_set_balance_bytes
// Test infrastructure.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../kpal_amd/csrc/pair_set_plan.hpp"

using namespace kpal;

static const uint64_t kEnumerate = 1ULL << 23;

static int walk(uint64_t bins, uint64_t n, uint64_t num_cu, uint64_t *units_out, uint64_t *grid_out, uint64_t *lo_out, uint64_t *hi_out)
{
    const uint64_t units = pair_set_units(n, bins), grid = pair_set_workgroups(n, bins, num_cu), items = pair_set_items(n, bins);
    const uint64_t slices = pair_set_slices(bins);
    *units_out = units;
    *grid_out = grid;
    uint64_t lo = UINT64_MAX, hi = 0, sum = 0;
    int ok = grid >= 1 && grid <= units && grid <= pair_set_slots(num_cu);
    for (uint64_t g = 0; g < grid; ++g) {
        const uint64_t s = balance_set_share(units, grid, g);
        lo = s < lo ? s : lo;
        hi = s > hi ? s : hi;
        sum += s;
    }
    *lo_out = lo;
    *hi_out = hi;
    ok = ok && sum == units;
    const uint32_t waves = pair_set_wave_form(bins) ? kPairSetWaves : 1;   // (slice form: every wave works on the unit's one item)
    if (items <= kEnumerate) {
        std::vector<uint8_t> seen(items, 0);
        for (uint64_t g = 0; g < grid; ++g)
            for (uint64_t u = g; u < units; u += grid)
                for (uint32_t w = 0; w < waves; ++w) {
                    uint64_t p = 0, s = 0;
                    if (!pair_set_item(n, bins, u, w, &p, &s)) {
                        ok = ok && pair_set_wave_form(bins) && u == units - 1;   // nothing but the ragged last unit has idle waves
                        continue;
                    }
                    if (s >= slices || p >= n || seen[p * slices + s]++) ok = 0;
                }
        for (uint64_t i = 0; i < items; ++i) ok = ok && seen[i] == 1;
    } else {
        for (uint64_t i = 0; i <= 4097; ++i) {
            const uint64_t u = i == 4097 ? units - 1 : (units / 4097) * i;
            for (uint32_t w = 0; w < waves; ++w) {
                uint64_t p = 0, s = 0;
                const bool valid = pair_set_item(n, bins, u, w, &p, &s);
                if (!valid) continue;
                const uint64_t back = pair_set_wave_form(bins) ? p / kPairSetWaves : p * slices + s;
                ok = ok && back == u && s < slices && p < n && (!pair_set_wave_form(bins) || p % kPairSetWaves == w);
            }
        }
    }
    return ok;
}

static int partial_bijection(uint64_t bins, uint64_t n, uint64_t nacc, uint64_t *size_out)
{
    const uint64_t slices = pair_set_slices(bins), size = nacc * n * slices;
    *size_out = size;
    int ok = 1;
    if (size <= kEnumerate) {
        std::vector<uint8_t> seen(size, 0);
        for (uint64_t a = 0; a < nacc; ++a)
            for (uint64_t p = 0; p < n; ++p)
                for (uint64_t s = 0; s < slices; ++s) {
                    const uint64_t at = pair_set_partial(a, n, slices, p, s);
                    if (at >= size || seen[at]++) ok = 0;
                }
        for (uint64_t i = 0; i < size; ++i) ok = ok && seen[i] == 1;
        return ok;
    }
    // (acc, pair, slice) in lexicographic order is the number i = (acc * n + pair) * slices + slice: the index must be i itself
    for (uint64_t j = 0; j <= 4097; ++j) {
        const uint64_t i = j == 4097 ? size - 1 : (size / 4097) * j;
        const uint64_t s = i % slices, p = (i / slices) % n, a = i / slices / n;
        ok = ok && pair_set_partial(a, n, slices, p, s) == i;
    }
    return ok;
}

int main()
{
    char what[16], line[512];
    int answered = 0;
    while (fgets(line, sizeof line, stdin)) {
        long long a[4] = {};
        int at = 0;
        if (sscanf(line, "%15s%n", what, &at) < 1) continue;
        const int got = sscanf(line + at, "%lld %lld %lld %lld", &a[0], &a[1], &a[2], &a[3]);
        const uint64_t bins = a[0] >= 1 && a[0] <= 16 ? 1ULL << (2 * a[0]) : 0;   // (of the queries whose first word is K)
        if (!strcmp(what, "sizes") && got < 1)
            printf("%d %d %d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %u\n", kPairSetThreads, kPairSetWaves, kPairSetUnroll, kPairSetSliceBins,
                   kPairSetWaveMaxBins, kPairSetSlotsPerCu, kPairSetBalanceBytes, kPairSetMaxAcc);
        else if (!strcmp(what, "slices") && got == 1 && bins) printf("%" PRIu64 " %d\n", pair_set_slices(bins), pair_set_wave_form(bins) ? 1 : 0);
        else if (!strcmp(what, "tile") && got == 1 && bins) {
            const uint64_t slices = pair_set_slices(bins);
            uint64_t lo = UINT64_MAX, hi = 0, next = 0;
            int ok = 1;
            for (uint64_t s = 0; s < slices; ++s) {
                const uint64_t b = pair_set_slice_begin(s), e = pair_set_slice_end(bins, s);
                ok = ok && b == next && e > b && b % 2 == 0 && e % 2 == 0;
                next = e;
                lo = e - b < lo ? e - b : lo;
                hi = e - b > hi ? e - b : hi;
            }
            printf("%d %" PRIu64 " %" PRIu64 "\n", ok && next == bins, lo, hi);
        } else if (!strcmp(what, "walk") && got == 3 && bins) {
            uint64_t units = 0, grid = 0, lo = 0, hi = 0;
            const int ok = walk(bins, (uint64_t)a[1], (uint64_t)a[2], &units, &grid, &lo, &hi);
            printf("%" PRIu64 " %" PRIu64 " %d %" PRIu64 " %" PRIu64 "\n", units, grid, ok, lo, hi);
        } else if (!strcmp(what, "partial") && got == 3 && bins) {
            uint64_t size = 0;
            const int ok = partial_bijection(bins, (uint64_t)a[1], (uint64_t)a[2], &size);
            printf("%d %" PRIu64 "\n", ok, size);
        } else if (!strcmp(what, "chunk") && got == 4 && bins) {
            const uint64_t c = pair_set_chunk((uint64_t)a[1], bins, a[2] != 0, (uint64_t)a[3]);
            printf("%" PRIu64 " %" PRIu64 "\n", c, pair_set_chunks((uint64_t)a[1], c));
        } else if (!strcmp(what, "alias") && got == 4) {
            int64_t lag = 0;
            const int c = pair_set_alias((uint64_t)a[0], (uint64_t)a[1], (uint64_t)a[2], (uint64_t)a[3], &lag);
            printf("%d %" PRId64 "\n", c, lag);
        } else if (!strcmp(what, "union") && got == 2) printf("%" PRIu64 "\n", pair_set_union_tables((uint64_t)a[0], (int64_t)a[1]));
        else if (!strcmp(what, "bbytes") && got == 3) printf("%" PRIu64 "\n", pair_set_balance_bytes((uint64_t)a[0], (uint64_t)a[1], (uint64_t)a[2]));
        else {
            printf("bad query: %s", line);
            return 2;
        }
        ++answered;
    }
    printf("PAIR_SET_PLAN_DONE %d\n", answered);
    return 0;
}
