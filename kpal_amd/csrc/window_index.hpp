// window_index.hpp -- layout arithmetic of Profile.from_fasta_by_window: which windows a record has, which tiles they are
// summed from, which of them lose k-mers at their end.  No GPU in it: the kernels of window_kernels.hpp, the host side
// of kpal_fasta_windows_* and a CPU program (tests/test_windows_host.py) read the same functions.
//
// A record of L bases, window W, step S (S divides W, m = W / S):
//   * windows   : none for L = 0, one for L <= W, else ceil((L - W) / S) + 1; window j covers bases [j S, min(j S + W, L));
//   * tiles     : ceil(L / S) of them, tile t = bases [t S, min((t + 1) S, L)); a k-mer belongs to the tile its FIRST base
//                 lies in, whatever it runs into;
//   * window j  = tiles j .. min(j + m, tiles) - 1, minus -- when the window ends before the record does -- the k-mers
//                 that begin in its last k - 1 bases (they run past its end; with S < k - 1 over several tile borders).
// Over the records of a piece, windows and tiles are numbered record-major: first_window[r] and first_tile[r] are the
// running sums (R + 1 values each).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KPAL_WIN_HD __host__ __device__
#else
#define KPAL_WIN_HD
#endif

namespace kpal {

// the (k, window, step) a call accepts
KPAL_WIN_HD inline bool win_args_ok(int k, uint64_t W, uint64_t S)
{
    return k >= 1 && S >= 1 && S <= W && (uint64_t)k <= W && W % S == 0;
}

KPAL_WIN_HD inline uint64_t win_count(uint64_t L, uint64_t W, uint64_t S)
{
    if (L == 0) return 0;
    if (L <= W) return 1;
    return (L - W + S - 1) / S + 1;
}

KPAL_WIN_HD inline uint64_t win_tiles(uint64_t L, uint64_t S) { return L / S + (L % S != 0); }

// one past the last base of window j
KPAL_WIN_HD inline uint64_t win_end(uint64_t j, uint64_t L, uint64_t W, uint64_t S)
{
    const uint64_t e = j * S + W;
    return e < L ? e : L;
}

// window j ends before its record does: the k-mers beginning in bases [j S + W - k + 1, j S + W) are taken off again
KPAL_WIN_HD inline bool win_trimmed(uint64_t j, uint64_t L, uint64_t W, uint64_t S) { return j * S + W < L; }

// one past the last tile of window j (its first one is tile j)
KPAL_WIN_HD inline uint64_t win_tile_end(uint64_t j, uint64_t L, uint64_t W, uint64_t S)
{
    const uint64_t nt = win_tiles(L, S), e = j + W / S;
    return e < nt ? e : nt;
}

// largest r in [0, R) with first[r] <= x, for ascending first[0 .. R] with first[0] <= x < first[R] (records without
// windows or tiles repeat their value: the search passes them)
KPAL_WIN_HD inline uint64_t win_find(const uint64_t *first, uint64_t R, uint64_t x)
{
    uint64_t lo = 0, hi = R;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (first[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// starts[r] = position of record r's separator in the flattened stream (its bases follow), starts[R] = stream length
KPAL_WIN_HD inline uint64_t win_record_bases(const uint64_t *starts, uint64_t r) { return starts[r + 1] - starts[r] - 1; }

// first_window / first_tile (R + 1 values each) of the R records of a piece
inline void win_layout(const uint64_t *starts, uint64_t R, uint64_t W, uint64_t S, uint64_t *first_window, uint64_t *first_tile)
{
    uint64_t w = 0, t = 0;
    for (uint64_t r = 0; r < R; ++r) {
        first_window[r] = w;
        first_tile[r] = t;
        const uint64_t L = win_record_bases(starts, r);
        w += win_count(L, W, S);
        t += win_tiles(L, S);
    }
    first_window[R] = w;
    first_tile[R] = t;
}

// What windows [first, first + n) of a piece (n >= 1) are made from: the tiles [tile0, tile1) -- the first tile of the
// first window to the last tile of the last one; every tile between them belongs to a window of the range -- and the
// bytes [byte0, byte1) of the flattened stream those tiles' k-mers lie in.
struct WinRange {
    uint64_t rec0, win0;     // record and window-in-record of window `first`
    uint64_t rec1, win1;     // ... of window first + n - 1
    uint64_t tile0, tile1;
    uint64_t byte0, byte1;
};

inline WinRange win_range(const uint64_t *starts, const uint64_t *first_window, const uint64_t *first_tile, uint64_t R, int k,
                          uint64_t W, uint64_t S, uint64_t first, uint64_t n)
{
    WinRange g;
    g.rec0 = win_find(first_window, R, first);
    g.win0 = first - first_window[g.rec0];
    g.rec1 = win_find(first_window, R, first + n - 1);
    g.win1 = first + n - 1 - first_window[g.rec1];
    const uint64_t L1 = win_record_bases(starts, g.rec1);
    const uint64_t t1 = win_tile_end(g.win1, L1, W, S);
    g.tile0 = first_tile[g.rec0] + g.win0;
    g.tile1 = first_tile[g.rec1] + t1;
    g.byte0 = starts[g.rec0] + 1 + g.win0 * S;
    const uint64_t last = t1 * S + (uint64_t)(k - 1);   // k-mers of the last tile run up to k - 1 bases past it
    g.byte1 = starts[g.rec1] + 1 + (last < L1 ? last : L1);
    return g;
}

}  // namespace kpal
