// stat_plan.hpp -- what the host decides about the summaries and the strand balance of whole SETS of profiles before it launches
// anything (kpal_stats_set_device, kpal_strand_balance_set_device; the kernels: stat_set_kernels.hpp).  No GPU in it:
// kpal_sets.hip, kpal_vec.hip (the mean of a 128-bit sum), table_host.hpp (the tables of one upload of a host set), the kernels
// (the slice bounds, the select state) and a CPU program (tests/test_stat_plan_host.py) read the same definitions.
//
// A table of `bins` entries is cut into SLICES of kStatSliceBins entries, one workgroup each; the grid of a pass is
// slices x profiles.  The number of slices depends on `bins` alone, and a profile's slices are combined in slice order: what a
// table gives does not depend on the set it is in, on its place there, or on how the set is cut into passes.
#pragma once
#include "matrix_plan.hpp"

namespace kpal {

constexpr int kStatSetThreads = 256;                 // threads of a slice's workgroup
constexpr int kStatSetRounds = 32;                   // entries a thread takes from its slice, kStatSetThreads apart
constexpr uint64_t kStatSliceBins = (uint64_t)kStatSetThreads * kStatSetRounds;   // 8192: one workgroup's worth of bins

// Slices of one table: one up to a workgroup's worth of bins (k <= 6, and every short vector), else as many as cover it --
// the last one is short when `bins` is no multiple.
KPAL_MATRIX_HD uint64_t stat_slices(uint64_t bins) { return bins <= kStatSliceBins ? 1 : (bins + kStatSliceBins - 1) / kStatSliceBins; }
KPAL_MATRIX_HD uint64_t stat_slice_begin(uint64_t slice) { return slice * kStatSliceBins; }
KPAL_MATRIX_HD uint64_t stat_slice_end(uint64_t bins, uint64_t slice)
{
    const uint64_t end = (slice + 1) * kStatSliceBins;
    return end < bins ? end : bins;
}

// What the radix select of one profile carries from digit to digit, in device memory (select_pick_set_kernel).
struct StatSetState {
    uint64_t prefix;   // the digits chosen so far (below them: those of the smallest key)
    uint64_t below;    // entries whose key is smaller than every key with these digits
    uint64_t equal;    // entries whose key has these digits
    uint64_t next;     // the smallest key above the lower middle one (select_next_set_kernel), UINT64_MAX: none seen
    double mean;       // read by the variance pass
    int32_t top;       // the highest byte in which the smallest and the largest key differ; -1: all entries are equal
    int32_t reserved;
};

constexpr uint64_t kStatPartialBytes = 40;           // StatPartial (stat_kernels.hpp): 128-bit sum, non-zero count, min, max
constexpr uint64_t kStatHistBins = 256;              // one 8-bit digit
constexpr uint64_t kStatHistBytes = kStatHistBins * 8;
constexpr uint64_t kStatStateBytes = sizeof(StatSetState);
constexpr uint64_t kStatOutBytes = sizeof(kpal_profile_stats);

// Scratch of one profile: a partial per slice (the variance pass writes its doubles over them), the digit histogram, the
// select state and the finished summary.
inline uint64_t stat_scratch_bytes(uint64_t bins)
{
    return stat_slices(bins) * kStatPartialBytes + kStatHistBytes + kStatStateBytes + kStatOutBytes;
}

// The strand balance of a set (one profile, kpal_strand_balance, is a set of one): workgroups per profile (one per 64 x 64 tile
// of the LDS-tiled form, k >= 6; one per 256 bins
// below that) and a (sum, count) partial for each.
inline uint64_t balance_set_grid(int k) { return k >= 6 ? 1ULL << (2 * (k - 6)) : (k >= 4 ? 1ULL << (2 * (k - 4)) : 1ULL); }
inline uint64_t balance_set_scratch_bytes(int k) { return balance_set_grid(k) * sizeof(Partial); }

constexpr uint64_t kStatSetBudgetBytes = 256ULL << 20;   // scratch of one pass
constexpr uint64_t kStatSetMaxProfiles = 65535;          // the second dimension of a grid

// Profiles of one pass: what the budget holds of their scratch, at most the second dimension of a grid, at most `cap` if the
// caller gives one (0: none) -- and never less than one.
inline uint64_t stat_profiles_per_pass(uint64_t scratch_bytes_per_profile, uint64_t budget_bytes, uint64_t cap)
{
    uint64_t per = budget_bytes / std::max<uint64_t>(1, scratch_bytes_per_profile);
    per = std::min(per, kStatSetMaxProfiles);
    if (cap > 0) per = std::min(per, cap);
    return std::max<uint64_t>(1, per);
}

struct StatChunk {
    uint64_t first, count;
};
inline std::vector<StatChunk> stat_chunks(uint64_t n, uint64_t per_pass)
{
    std::vector<StatChunk> out;
    per_pass = std::max<uint64_t>(1, per_pass);
    for (uint64_t at = 0; at < n; at += per_pass) out.push_back(StatChunk{at, std::min(per_pass, n - at)});
    return out;
}

// Host tables go up through the context's scratch, at most kSetUploadBytes of them at a time -- and never less than one table
// (table_host.hpp: for_uploaded_chunks; the chunks are stat_chunks of this).
constexpr uint64_t kSetUploadBytes = 1ULL << 30;
inline uint64_t stat_upload_tables(uint64_t bins) { return std::max<uint64_t>(1, kSetUploadBytes / (std::max<uint64_t>(1, bins) * 8)); }

// The 128-bit two's complement sum (hi, lo) as a double: magnitude first, so that a small negative sum does not cancel.
KPAL_MATRIX_HD double stat_sum128_to_double(uint64_t lo, int64_t hi)
{
    uint64_t mag_lo = lo, mag_hi = (uint64_t)hi;
    const bool negative = hi < 0;
    if (negative) {
        mag_lo = ~mag_lo + 1ULL;
        mag_hi = ~mag_hi + (mag_lo == 0 ? 1ULL : 0ULL);
    }
    const double magnitude = (double)mag_hi * 18446744073709551616.0 + (double)mag_lo;   // (2^64: the scaling is exact)
    return negative ? -magnitude : magnitude;
}
KPAL_MATRIX_HD double stat_mean(uint64_t lo, int64_t hi, uint64_t bins) { return stat_sum128_to_double(lo, hi) / (double)bins; }

// The highest byte in which two order-preserving keys differ, -1 if they are equal: the digits a radix select has to run.
KPAL_MATRIX_HD int stat_top_byte(uint64_t kmin, uint64_t kmax)
{
    int top = 7;
    while (top >= 0 && ((kmin >> (8 * top)) & 255u) == ((kmax >> (8 * top)) & 255u)) --top;
    return top;
}
// The bits above byte `byte`: what the digits chosen before it cover.
KPAL_MATRIX_HD uint64_t stat_mask_above(int byte) { return byte >= 7 ? 0ULL : ~0ULL << (8 * (byte + 1)); }

}  // namespace kpal
