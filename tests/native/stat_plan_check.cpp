// stat_plan_check.cpp -- the slices, the scratch, the passes and the shared arithmetic of the summaries and the strand balance
// of whole sets of profiles (kpal_amd/csrc/stat_plan.hpp) as a CPU program: it answers the queries on its standard input, one
// line each, and knows no expected value -- those are the literals of tests/test_stat_plan_host.py.  Every argument is an
// unsigned integer; a double is answered as its bit pattern.
//   slices   BINS                  -> stat_slices
//   slice    BINS S                -> stat_slice_begin stat_slice_end
//   scratch  BINS                  -> stat_scratch_bytes
//   sizes                          -> kStatSetThreads kStatSliceBins kStatPartialBytes kStatHistBytes kStatStateBytes kStatOutBytes
//   limits                         -> kStatSetBudgetBytes kStatSetMaxProfiles
//   per      SCRATCH BUDGET CAP    -> stat_profiles_per_pass
//   chunks   N PER                 -> first count first count ...
//   upload   BINS                  -> stat_upload_tables kSetUploadBytes
//   bgrid    K                     -> balance_set_grid balance_set_scratch_bytes
//   sum128   LO HI                 -> stat_sum128_to_double (HI: the two's complement word)
//   mean     LO HI BINS            -> stat_mean
//   top      KMIN KMAX             -> stat_top_byte
//   mask     BYTE                  -> stat_mask_above
// Test infrastructure.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../kpal_amd/csrc/stat_plan.hpp"

using namespace kpal;

static uint64_t bits(double v)
{
    uint64_t u;
    memcpy(&u, &v, sizeof u);
    return u;
}

int main()
{
    char what[16], line[512];
    int answered = 0;
    while (fgets(line, sizeof line, stdin)) {
        unsigned long long a[3] = {};
        int at = 0;
        if (sscanf(line, "%15s%n", what, &at) < 1) continue;
        const int got = sscanf(line + at, "%llu %llu %llu", &a[0], &a[1], &a[2]);
        if (!strcmp(what, "slices") && got == 1) printf("%" PRIu64 "\n", stat_slices(a[0]));
        else if (!strcmp(what, "slice") && got == 2) printf("%" PRIu64 " %" PRIu64 "\n", stat_slice_begin(a[1]), stat_slice_end(a[0], a[1]));
        else if (!strcmp(what, "scratch") && got == 1) printf("%" PRIu64 "\n", stat_scratch_bytes(a[0]));
        else if (!strcmp(what, "sizes") && got < 1)
            printf("%d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", kStatSetThreads, kStatSliceBins, kStatPartialBytes, kStatHistBytes,
                   kStatStateBytes, kStatOutBytes);
        else if (!strcmp(what, "limits") && got < 1) printf("%" PRIu64 " %" PRIu64 "\n", kStatSetBudgetBytes, kStatSetMaxProfiles);
        else if (!strcmp(what, "per") && got == 3) printf("%" PRIu64 "\n", stat_profiles_per_pass(a[0], a[1], a[2]));
        else if (!strcmp(what, "chunks") && got == 2) {
            const std::vector<StatChunk> chunks = stat_chunks(a[0], a[1]);
            for (size_t i = 0; i < chunks.size(); ++i) printf("%s%" PRIu64 " %" PRIu64, i ? " " : "", chunks[i].first, chunks[i].count);
            printf("\n");
        } else if (!strcmp(what, "upload") && got == 1) printf("%" PRIu64 " %" PRIu64 "\n", stat_upload_tables(a[0]), kSetUploadBytes);
        else if (!strcmp(what, "bgrid") && got == 1) printf("%" PRIu64 " %" PRIu64 "\n", balance_set_grid((int)a[0]), balance_set_scratch_bytes((int)a[0]));
        else if (!strcmp(what, "sum128") && got == 2) printf("%" PRIu64 "\n", bits(stat_sum128_to_double(a[0], (int64_t)a[1])));
        else if (!strcmp(what, "mean") && got == 3) printf("%" PRIu64 "\n", bits(stat_mean(a[0], (int64_t)a[1], a[2])));
        else if (!strcmp(what, "top") && got == 2) printf("%d\n", stat_top_byte(a[0], a[1]));
        else if (!strcmp(what, "mask") && got == 1) printf("%" PRIu64 "\n", stat_mask_above((int)a[0]));
        else {
            printf("bad query: %s", line);
            return 1;
        }
        ++answered;
    }
    printf("STAT_PLAN_DONE %d\n", answered);
    return 0;
}
