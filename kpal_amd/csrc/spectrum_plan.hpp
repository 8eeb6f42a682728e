// spectrum_plan.hpp -- what the host decides about the count-of-counts spectra (metrics.distribution, kpal/metrics.py:22-33) of
// whole SETS of tables before it launches anything (kpal_distribution_set_device; the kernels: spectrum_kernels.hpp).  No GPU
// in it: kpal_spectrum.hip, the kernels and a CPU program (tests/test_spectrum_plan_host.py) read the same definitions.
//
// Values are handled as order-preserving uint64 KEYS (the sign bit flipped, as the radix select does), so INT64_MIN and
// INT64_MAX in one table are a spread of 2^64 - 1 and nothing overflows.  Table t of a pass has a dense WINDOW of W uint64
// counters for the keys [min_t, min_t + W); W is one number for the pass:
//
//     W = min(widest (max - min + 1) of the pass, bins, kSpectrumWindowCap)        (spectrum_window)
//
// (a table of `bins` entries has at most `bins` distinct values: a wider window could only hold more zeros).  The first
// min(W, kSpectrumLdsBins) counters of a window are built in LDS, one private copy per workgroup, and flushed once; the rest
// takes global atomics.  Keys at or past min_t + W go to an overflow list that the host finishes with a sort: exact for any
// input, and what a table gives does not depend on W -- so not on the set it is in, its place there or where the passes are cut.
//
// The tables of a pass are decided BEFORE its spreads are known, from the widest window `bins` allows (spectrum_tables_per_pass).
#pragma once
#include "stat_plan.hpp"

namespace kpal {

constexpr uint64_t kSpectrumWindowCap = 1ULL << 20;   // counters of the widest window (8 MiB a table)
constexpr uint32_t kSpectrumLdsBins = 4096;           // window counters a workgroup keeps in LDS (uint32: a slice is 8192 bins)
constexpr int kSpectrumPeels = 1;                     // values a wave counts with a ballot each before its lanes go one by one (measured: 1, 2, 4, 8, 16)
constexpr int kSpectrumCompactPerThread = 8;          // consecutive window counters one thread of the compaction looks at
constexpr uint64_t kSpectrumWindowSlice = (uint64_t)kStatSetThreads * kSpectrumCompactPerThread;   // 2048: one compaction workgroup
constexpr int kSpectrumScanThreads = 1024;            // the one workgroup that scans the non-zero counts of a pass
constexpr uint64_t kSpectrumRangeBytes = 16;          // SpectrumRange
constexpr uint64_t kSpectrumOverflowBytes = 16;       // SpectrumOverflow

// Smallest key of a table and (largest - smallest): the spread minus one, which always fits.
struct SpectrumRange {
    uint64_t kmin, wide;
};
// One entry of the overflow list: a key at or past the window of table `table` of the pass.
struct SpectrumOverflow {
    uint64_t key, table;
};

KPAL_MATRIX_HD uint64_t spectrum_key(int64_t v) { return (uint64_t)v ^ 0x8000000000000000ULL; }
KPAL_MATRIX_HD int64_t spectrum_value(uint64_t key) { return (int64_t)(key ^ 0x8000000000000000ULL); }
// Where `key` (>= kmin) falls, counted from the window's first counter; inside the window iff that is below W.
KPAL_MATRIX_HD uint64_t spectrum_offset(uint64_t key, uint64_t kmin) { return key - kmin; }
KPAL_MATRIX_HD bool spectrum_in_window(uint64_t key, uint64_t kmin, uint64_t window) { return spectrum_offset(key, kmin) < window; }

// W from the widest (max - min) of a pass, in keys.
KPAL_MATRIX_HD uint64_t spectrum_window(uint64_t wide, uint64_t bins)
{
    uint64_t w = wide >= kSpectrumWindowCap ? kSpectrumWindowCap : wide + 1;
    return w < bins ? w : bins;
}
KPAL_MATRIX_HD uint32_t spectrum_lds_bins(uint64_t window) { return window < kSpectrumLdsBins ? (uint32_t)window : kSpectrumLdsBins; }
KPAL_MATRIX_HD uint64_t spectrum_window_slices(uint64_t window) { return (window + kSpectrumWindowSlice - 1) / kSpectrumWindowSlice; }

// Scratch of one table: the min/max partials of its slices, its range, its window, a non-zero count per window slice (a scanned
// offset afterwards) and its number of overflowing entries.  (The finished pairs and the overflow list are sized by what the pass
// finds: at most 16 bytes per window counter and per overflowing entry.)
inline uint64_t spectrum_scratch_bytes(uint64_t bins, uint64_t window)
{
    return stat_slices(bins) * kStatPartialBytes + kSpectrumRangeBytes + window * 8 + spectrum_window_slices(window) * 8 + 8;
}
inline uint64_t spectrum_tables_per_pass(uint64_t bins, uint64_t budget_bytes, uint64_t cap)
{
    return stat_profiles_per_pass(spectrum_scratch_bytes(bins, spectrum_window(UINT64_MAX, bins)), budget_bytes, cap);
}

}  // namespace kpal
