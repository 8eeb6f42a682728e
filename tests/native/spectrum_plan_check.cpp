// spectrum_plan_check.cpp -- the window, the scratch, the passes and the key arithmetic of the count-of-counts spectra of whole
// sets of tables (kpal_amd/csrc/spectrum_plan.hpp) as a CPU program: it answers the queries on its standard input, one line
// each, and knows no expected value -- those are the literals of tests/test_spectrum_plan_host.py.  Every argument is an
// unsigned integer (a value: its two's complement word), every answer too.
//   sizes                          -> kSpectrumWindowCap kSpectrumLdsBins kSpectrumPeels kSpectrumWindowSlice kSpectrumScanThreads
//                                     kSpectrumRangeBytes kSpectrumOverflowBytes sizeof(SpectrumRange) sizeof(SpectrumOverflow)
//   key      VALUE                 -> spectrum_key
//   value    KEY                   -> spectrum_value
//   offset   KEY KMIN              -> spectrum_offset
//   inside   KEY KMIN WINDOW       -> spectrum_in_window
//   window   WIDE BINS             -> spectrum_window (WIDE: largest key - smallest key of the pass)
//   lds      WINDOW                -> spectrum_lds_bins
//   wslices  WINDOW                -> spectrum_window_slices
//   scratch  BINS WINDOW           -> spectrum_scratch_bytes
//   per      BINS BUDGET CAP       -> spectrum_tables_per_pass
// Test infrastructure.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../kpal_amd/csrc/spectrum_plan.hpp"

using namespace kpal;

int main()
{
    char what[16], line[512];
    int answered = 0;
    while (fgets(line, sizeof line, stdin)) {
        unsigned long long a[3] = {};
        int at = 0;
        if (sscanf(line, "%15s%n", what, &at) < 1) continue;
        const int got = sscanf(line + at, "%llu %llu %llu", &a[0], &a[1], &a[2]);
        if (!strcmp(what, "sizes") && got < 1)
            printf("%" PRIu64 " %u %d %" PRIu64 " %d %" PRIu64 " %" PRIu64 " %zu %zu\n", kSpectrumWindowCap, kSpectrumLdsBins, kSpectrumPeels,
                   kSpectrumWindowSlice, kSpectrumScanThreads, kSpectrumRangeBytes, kSpectrumOverflowBytes, sizeof(SpectrumRange), sizeof(SpectrumOverflow));
        else if (!strcmp(what, "key") && got == 1) printf("%" PRIu64 "\n", spectrum_key((int64_t)a[0]));
        else if (!strcmp(what, "value") && got == 1) printf("%" PRIu64 "\n", (uint64_t)spectrum_value(a[0]));
        else if (!strcmp(what, "offset") && got == 2) printf("%" PRIu64 "\n", spectrum_offset(a[0], a[1]));
        else if (!strcmp(what, "inside") && got == 3) printf("%d\n", spectrum_in_window(a[0], a[1], a[2]) ? 1 : 0);
        else if (!strcmp(what, "window") && got == 2) printf("%" PRIu64 "\n", spectrum_window(a[0], a[1]));
        else if (!strcmp(what, "lds") && got == 1) printf("%u\n", spectrum_lds_bins(a[0]));
        else if (!strcmp(what, "wslices") && got == 1) printf("%" PRIu64 "\n", spectrum_window_slices(a[0]));
        else if (!strcmp(what, "scratch") && got == 2) printf("%" PRIu64 "\n", spectrum_scratch_bytes(a[0], a[1]));
        else if (!strcmp(what, "per") && got == 3) printf("%" PRIu64 "\n", spectrum_tables_per_pass(a[0], a[1], a[2]));
        else {
            printf("bad query: %s", line);
            return 1;
        }
        ++answered;
    }
    printf("SPECTRUM_PLAN_DONE %d\n", answered);
    return 0;
}
