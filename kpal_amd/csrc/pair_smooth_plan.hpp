// pair_smooth_plan.hpp -- what the host decides about DYNAMIC SMOOTHING over the linked pairs of two sets of profiles before it
// launches anything (kpal_paired_smooth_distance[_device], kpal_paired_smooth_device; the kernels: pair_smooth_kernels.hpp).  No
// GPU in it: kpal_paired_smooth.hip, the kernels and a CPU program (tests/test_pair_smooth_plan_host.py) read the same
// definitions.  It joins pair_set_plan.hpp (items, units, the persistent grid, chunks, the alias test) and smooth_plan.hpp (one
// pyramid of node sums and codes per profile).
//
// ITEMS.  An item is (pair p, slice s).  A pair's slices are its pair_set_slices(4^k) BIN slices followed by its NODE slices: a
// node slice is a run of kPairSmoothSliceNodes elements of the smooth_stride(k) elements of a pyramid -- one up to k = 8, two at
// k = 9, where the second one is exactly the heights >= 1 (height 0 has 4^8 = 2^16 nodes).  How many there are depends on k alone.
// UNITS.  The wave form (pair_set_wave_form, k <= 6): a wave streams the bins of a pair and then its pyramid and writes ONE
// partial per accumulator; a unit is four pairs.  Otherwise a unit is one item, taken by a four-wave workgroup.
// GRID.  Persistent, pair_set_workgroups' rule over these units.
// PARTIALS.  Accumulator a of pair p, slice s at (a * N + p) * slices + s (pair_set_partial), added in slice order: the bits of
// a pair depend on its two tables and the options alone, not on N, its position, the chunking or how the ranges alias.
// CHUNKS.  pair_set_chunk, cut further by the 32-bit index of these partials and so that the pyramids of a chunk's distinct
// tables stay within kSmoothBudgetBytes -- never below one pair (two k = 16 pyramids fit); chunk_pairs > 0 only lowers it.
// TABLES.  The pyramids of a chunk are those of its two sides, left first (pair p: p and N + p), or -- when the ranges are the
// same range or lie a whole number of tables apart and meet within the chunk -- of the union of the two ranges once (pair p:
// p + max(-lag, 0) and p + max(lag, 0)).
#pragma once
#include "pair_set_plan.hpp"
#include "smooth_plan.hpp"

namespace kpal {

constexpr uint64_t kPairSmoothSliceNodes = 1ULL << 16;   // pyramid elements of a node slice

// ---- items ------------------------------------------------------------------------------------------------------------------------
KPAL_MATRIX_HD uint64_t pair_smooth_bin_slices(int k) { return pair_set_slices(1ULL << (2 * k)); }
KPAL_MATRIX_HD uint64_t pair_smooth_node_slices(int k) { return (smooth_stride(k) + kPairSmoothSliceNodes - 1) / kPairSmoothSliceNodes; }
// Partials of one accumulator of one pair: the wave form adds bins and pyramid in the wave.
KPAL_MATRIX_HD uint64_t pair_smooth_slices(int k)
{
    return pair_set_wave_form(1ULL << (2 * k)) ? 1 : pair_smooth_bin_slices(k) + pair_smooth_node_slices(k);
}
KPAL_MATRIX_HD uint64_t pair_smooth_node_begin(uint64_t node_slice) { return node_slice * kPairSmoothSliceNodes; }
KPAL_MATRIX_HD uint64_t pair_smooth_node_end(int k, uint64_t node_slice)
{
    const uint64_t end = (node_slice + 1) * kPairSmoothSliceNodes, stride = smooth_stride(k);
    return end < stride ? end : stride;
}

// ---- units and the grid -----------------------------------------------------------------------------------------------------------
KPAL_MATRIX_HD uint64_t pair_smooth_units(uint64_t n_pairs, int k)
{
    return pair_set_wave_form(1ULL << (2 * k)) ? (n_pairs + kPairSetWaves - 1) / kPairSetWaves : n_pairs * pair_smooth_slices(k);
}
KPAL_MATRIX_HD uint64_t pair_smooth_workgroups(uint64_t n_pairs, int k, uint64_t num_cu)
{
    return balance_set_workgroups(pair_smooth_units(n_pairs, k), pair_set_slots(num_cu));
}
// The units of the apply kernel are those of the bins alone: pair_set_units(n_pairs, 4^k).

// ---- the pyramid set of a chunk -------------------------------------------------------------------------------------------------------
// The pyramids of a chunk are those of its distinct tables: pair_set_union / pair_set_tables (pair_set_plan.hpp), which the
// balanced copies share, under this plan's names.
KPAL_MATRIX_HD uint64_t pair_smooth_union(uint64_t chunk, int alias, int64_t lag) { return pair_set_union(chunk, alias, lag); }
KPAL_MATRIX_HD uint64_t pair_smooth_tables(uint64_t chunk, int alias, int64_t lag) { return pair_set_tables(chunk, alias, lag); }
// The pyramid of pair p's left / right table in the set of such a chunk.
KPAL_MATRIX_HD uint64_t pair_smooth_left(uint64_t chunk, int alias, int64_t lag, uint64_t pair)
{
    return pair_smooth_union(chunk, alias, lag) && lag < 0 ? pair + (uint64_t)(-lag) : pair;
}
KPAL_MATRIX_HD uint64_t pair_smooth_right(uint64_t chunk, int alias, int64_t lag, uint64_t pair)
{
    if (!pair_smooth_union(chunk, alias, lag)) return chunk + pair;
    return lag > 0 ? pair + (uint64_t)lag : pair;
}

// ---- chunks -----------------------------------------------------------------------------------------------------------------------
KPAL_MATRIX_HD uint64_t pair_smooth_chunk(int k, uint64_t n_pairs, bool do_balance, uint64_t chunk_pairs, int alias, int64_t lag)
{
    uint64_t chunk = pair_set_chunk(n_pairs, 1ULL << (2 * k), do_balance, chunk_pairs);
    const uint64_t by_index = (0x7fffffffULL / pair_smooth_slices(k)) / kPairSetMaxAcc;
    if (chunk > by_index) chunk = by_index;
    const uint64_t fit = kSmoothBudgetBytes / (smooth_stride(k) * kSmoothElementBytes);   // pyramids within the budget
    if (pair_smooth_tables(chunk, alias, lag) > fit) {
        const uint64_t d = lag < 0 ? (uint64_t)(-lag) : (uint64_t)lag;
        if (alias == kPairSetSame) chunk = fit;
        else if (alias == kPairSetLag && fit > 2 * d) chunk = fit - d;   // (more than |lag| pairs: the union still serves)
        else chunk = fit / 2;
    }
    return chunk < 1 ? 1 : chunk;
}

// Whether the smoothed linked pairs of a call run from per-profile pyramids (smooth_batched's rule: with do_positive the masks
// come first and node sums depend on the partner).
KPAL_MATRIX_HD bool pair_smooth_batched(bool do_smooth, bool do_positive) { return do_smooth && !do_positive; }

}  // namespace kpal
