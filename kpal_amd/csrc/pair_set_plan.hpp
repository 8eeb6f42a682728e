// pair_set_plan.hpp -- what the host decides about the distances of the LINKED pairs of two sets of profiles -- pair p is
// (left table p, right table p) -- before it launches anything (kpal_paired_distance[_device]; the kernels:
// pair_set_kernels.hpp).  No GPU in it: kpal_paired.hip, the kernels and a CPU program (tests/test_pair_set_plan_host.py) read
// the same definitions.
//
// ITEMS.  The work of a call is the flat list of items (pair p, slice s), item = p * slices + s.  A slice is a fixed run of
// kPairSetSliceBins bins; how many a pair has depends on 4^k alone -- not on N, on the device or on the chunking -- and a pair's
// slices are added in slice order (reduce_partials): that is what makes a pair's bits independent of the set it is in.
// UNITS.  What a workgroup of the persistent grid takes at a time.  A table of more than kPairSetWaveMaxBins bins: a unit is an
// item, streamed by the workgroup's four waves (SLICE form).  A smaller table is one slice and a WAVE streams it alone: a unit is
// four consecutive pairs, one per wave, and needs no LDS and no barrier (WAVE form; the last unit may be ragged).
// GRID.  Workgroup g takes the units g, g + grid, ...; the grid is the smallest one that needs no more rounds than `slots`
// workgroups would (balance_set_workgroups).
// PARTIALS.  Accumulator a of pair p, slice s at (a * N + p) * slices + s: nacc * N groups of `slices` for reduce_partials.
// CHUNKS.  With do_balance the balanced copies of a chunk's tables live in scratch: the pairs are cut into chunks whose copies
// fit kPairSetBalanceBytes (a single pair may exceed it); a chunk never has more partial groups than 32 bits index.
#pragma once
#include "transform_plan.hpp"

namespace kpal {

constexpr int kPairSetThreads = 256;                         // threads of a workgroup: four waves
constexpr int kPairSetWaves = kPairSetThreads / 64;
constexpr int kPairSetUnroll = 4;                            // 16-byte loads per table a lane has in flight
constexpr uint64_t kPairSetSliceBins = 1ULL << 16;           // k = 8 is exactly one slice, k = 9 four
constexpr uint64_t kPairSetWaveMaxBins = 1ULL << 12;         // up to k = 6 a table is one wave's: 32 loads of 16 bytes a lane
constexpr uint64_t kPairSetSlotsPerCu = 8;                   // workgroups a CU holds at once (pair_set_kernel: <= 64 registers)
constexpr uint64_t kPairSetBalanceBytes = 32ULL << 30;       // balanced copies of one chunk (what the smoothing pyramids take)
constexpr uint32_t kPairSetMaxAcc = 3;                       // accumulators of the widest pass (the cosine)

static_assert((kPairSetSliceBins & (kPairSetSliceBins - 1)) == 0 && kPairSetSliceBins >= 512, "a slice is a power of two >= 512");
static_assert(kPairSetWaveMaxBins <= kPairSetSliceBins, "a wave's table is one slice");

// ---- items ------------------------------------------------------------------------------------------------------------------------
KPAL_MATRIX_HD bool pair_set_wave_form(uint64_t bins) { return bins <= kPairSetWaveMaxBins; }
KPAL_MATRIX_HD uint64_t pair_set_slices(uint64_t bins) { return bins <= kPairSetSliceBins ? 1 : (bins + kPairSetSliceBins - 1) / kPairSetSliceBins; }
KPAL_MATRIX_HD uint64_t pair_set_slice_begin(uint64_t slice) { return slice * kPairSetSliceBins; }
KPAL_MATRIX_HD uint64_t pair_set_slice_end(uint64_t bins, uint64_t slice)
{
    const uint64_t end = (slice + 1) * kPairSetSliceBins;
    return end < bins ? end : bins;
}
KPAL_MATRIX_HD uint64_t pair_set_items(uint64_t n_pairs, uint64_t bins) { return n_pairs * pair_set_slices(bins); }

// ---- units and the grid -----------------------------------------------------------------------------------------------------------
KPAL_MATRIX_HD uint64_t pair_set_units(uint64_t n_pairs, uint64_t bins)
{
    return pair_set_wave_form(bins) ? (n_pairs + kPairSetWaves - 1) / kPairSetWaves : pair_set_items(n_pairs, bins);
}
KPAL_MATRIX_HD uint64_t pair_set_slots(uint64_t num_cu) { return (num_cu > 0 ? num_cu : 1) * kPairSetSlotsPerCu; }
KPAL_MATRIX_HD uint64_t pair_set_workgroups(uint64_t n_pairs, uint64_t bins, uint64_t num_cu)
{
    return balance_set_workgroups(pair_set_units(n_pairs, bins), pair_set_slots(num_cu));
}
// The item of wave `wave` of unit `unit`: slice form -- the unit's item, whichever wave asks; wave form -- pair 4 * unit + wave,
// none (false) past the last pair.
KPAL_MATRIX_HD bool pair_set_item(uint64_t n_pairs, uint64_t bins, uint64_t unit, uint32_t wave, uint64_t *pair, uint64_t *slice)
{
    if (pair_set_wave_form(bins)) {
        *pair = unit * kPairSetWaves + wave;
        *slice = 0;
    } else {
        const uint64_t slices = pair_set_slices(bins);
        *pair = unit / slices;
        *slice = unit % slices;
    }
    return *pair < n_pairs;
}

// ---- partials ---------------------------------------------------------------------------------------------------------------------
KPAL_MATRIX_HD uint64_t pair_set_partial(uint64_t acc, uint64_t n_pairs, uint64_t slices, uint64_t pair, uint64_t slice)
{
    return (acc * n_pairs + pair) * slices + slice;
}

// ---- chunks -----------------------------------------------------------------------------------------------------------------------
// Pairs of one chunk: all of them, cut down by the 32-bit partial index, by the bytes of the balanced copies (two tables a pair;
// never below one pair) and by the caller's chunk_pairs (> 0), which only lowers it.
KPAL_MATRIX_HD uint64_t pair_set_chunk(uint64_t n_pairs, uint64_t bins, bool do_balance, uint64_t chunk_pairs)
{
    uint64_t chunk = n_pairs;
    const uint64_t by_index = (0x7fffffffULL / pair_set_slices(bins)) / kPairSetMaxAcc;
    if (chunk > by_index) chunk = by_index;
    if (do_balance) {
        const uint64_t by_bytes = kPairSetBalanceBytes / (2 * bins * 8);
        if (chunk > by_bytes) chunk = by_bytes;
    }
    if (chunk_pairs > 0 && chunk > chunk_pairs) chunk = chunk_pairs;
    return chunk < 1 ? 1 : chunk;
}
KPAL_MATRIX_HD uint64_t pair_set_chunks(uint64_t n_pairs, uint64_t chunk) { return (n_pairs + chunk - 1) / chunk; }

// ---- the two input ranges ---------------------------------------------------------------------------------------------------------
enum PairSetAlias { kPairSetDisjoint = 0, kPairSetSame = 1, kPairSetLag = 2, kPairSetOther = 3 };
// n_pairs tables of `bins` int64 entries at byte address `left` and as many at `right` (neither range wraps): disjoint, the SAME
// range, `right` a whole number of tables behind or before `left` (*lag = (right - left) / table bytes, not 0) -- or anything
// else, which takes no shortcut.
KPAL_MATRIX_HD int pair_set_alias(uint64_t left, uint64_t right, uint64_t n_pairs, uint64_t bins, int64_t *lag)
{
    const uint64_t table = bins * 8, bytes = n_pairs * table;
    *lag = 0;
    if (left == right) return kPairSetSame;
    const uint64_t gap = right > left ? right - left : left - right;
    if (gap >= bytes) return kPairSetDisjoint;
    if (gap % table != 0) return kPairSetOther;
    *lag = right > left ? (int64_t)(gap / table) : -(int64_t)(gap / table);
    return kPairSetLag;
}
// Tables of the union of the two sides of a chunk of `chunk` pairs that lie `lag` tables apart, when balancing the union once is
// less work than balancing both sides: chunk + |lag|; 0: the sides of this chunk do not overlap.
KPAL_MATRIX_HD uint64_t pair_set_union_tables(uint64_t chunk, int64_t lag)
{
    const uint64_t d = lag < 0 ? (uint64_t)(-lag) : (uint64_t)lag;
    return d < chunk ? chunk + d : 0;
}
// Tables of the union that serves both sides of a chunk of `chunk` pairs (alias, lag: pair_set_alias), 0: two separate sides.
KPAL_MATRIX_HD uint64_t pair_set_union(uint64_t chunk, int alias, int64_t lag)
{
    return alias == kPairSetSame ? chunk : alias == kPairSetLag ? pair_set_union_tables(chunk, lag) : 0;
}
// The distinct tables of such a chunk: those of the union, or of the two sides.
KPAL_MATRIX_HD uint64_t pair_set_tables(uint64_t chunk, int alias, int64_t lag)
{
    const uint64_t un = pair_set_union(chunk, alias, lag);
    return un ? un : 2 * chunk;
}
// Bytes of the balanced copies of such a chunk (union_tables: 0 for two separate sides).
KPAL_MATRIX_HD uint64_t pair_set_balance_bytes(uint64_t chunk, uint64_t bins, uint64_t union_tables)
{
    return (union_tables ? union_tables : 2 * chunk) * bins * 8;
}

}  // namespace kpal
