// window_index_check W S k L0 L1 ... : prints what kpal_amd/csrc/window_index.hpp makes of the records of L0, L1, ...
// bases (tests/test_windows_host.py compares every line with a brute-force enumeration).  No GPU in it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../kpal_amd/csrc/window_index.hpp"

using namespace kpal;

int main(int argc, char **argv)
{
    if (argc < 4) return 2;
    const uint64_t W = strtoull(argv[1], nullptr, 10), S = strtoull(argv[2], nullptr, 10);
    const int k = atoi(argv[3]);
    const bool ok = win_args_ok(k, W, S);
    printf("args %d\n", ok ? 1 : 0);
    if (!ok) return 0;
    const uint64_t R = (uint64_t)(argc - 4);
    std::vector<uint64_t> starts(R + 1, 0);
    for (uint64_t r = 0; r < R; ++r) starts[r + 1] = starts[r] + 1 + strtoull(argv[4 + r], nullptr, 10);
    std::vector<uint64_t> fw(R + 1), ft(R + 1);
    win_layout(starts.data(), R, W, S, fw.data(), ft.data());
    for (uint64_t r = 0; r < R; ++r) {
        const uint64_t L = win_record_bases(starts.data(), r);
        printf("record %llu %llu %llu %llu %llu %llu\n", (unsigned long long)r, (unsigned long long)L, (unsigned long long)win_count(L, W, S),
               (unsigned long long)win_tiles(L, S), (unsigned long long)fw[r], (unsigned long long)ft[r]);
    }
    printf("total %llu %llu\n", (unsigned long long)fw[R], (unsigned long long)ft[R]);
    for (uint64_t w = 0; w < fw[R]; ++w) {
        const uint64_t r = win_find(fw.data(), R, w), j = w - fw[r];
        const uint64_t L = win_record_bases(starts.data(), r);
        printf("window %llu %llu %llu %llu %llu %llu %llu %d\n", (unsigned long long)w, (unsigned long long)r, (unsigned long long)j,
               (unsigned long long)(j * S), (unsigned long long)win_end(j, L, W, S), (unsigned long long)(ft[r] + j),
               (unsigned long long)(ft[r] + win_tile_end(j, L, W, S)), win_trimmed(j, L, W, S) ? 1 : 0);
    }
    for (uint64_t first = 0; first < fw[R]; ++first)
        for (uint64_t n = 1; first + n <= fw[R]; ++n) {
            const WinRange g = win_range(starts.data(), fw.data(), ft.data(), R, k, W, S, first, n);
            printf("range %llu %llu %llu %llu %llu %llu\n", (unsigned long long)first, (unsigned long long)n, (unsigned long long)g.tile0,
                   (unsigned long long)g.tile1, (unsigned long long)g.byte0, (unsigned long long)g.byte1);
        }
    return 0;
}
