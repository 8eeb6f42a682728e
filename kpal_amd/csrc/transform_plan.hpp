// transform_plan.hpp -- what the host decides about the transforms of whole SETS of tables lying one behind the other before it
// launches anything: the balance of every table, the shrink of every table and the pool (the sum) of all of them
// (kpal_balance_set_device, kpal_shrink_set_device, kpal_pool_set_device; the kernels: transform_set_kernels.hpp).  No GPU in
// it: kpal_transform.hip, the kernels and a CPU program (tests/test_transform_plan_host.py) read the same definitions.
//
// BALANCE, k >= 6.  The work of a set is the flat list of ITEMS (table t, canonical tile pair c), item = t * ncanon + c; at
// k = 6 an item is a whole table.  Persistent workgroups take the items round robin: workgroup g has g, g + grid, g + 2 grid ...
// The grid is the smallest one that needs no more rounds than `slots` workgroups would: every workgroup gets the same number of
// items to within one.
//
// POOL.  A workgroup of kPoolThreads threads owns kPoolThreads column pairs (16 bytes each) and walks the tables of one SLICE
// of the set; with more than one slice the partial rows are added by a second launch of the same kernel.  The slices are as
// many as fill the device with column groups x slices workgroups, never shorter than kPoolMinSliceTables tables (a slice costs a
// row of partials), and one when the columns alone fill it (bins >= kPoolOneSliceBins).
#pragma once
#include "matrix_plan.hpp"

namespace kpal {

constexpr int kBalanceSetSlotsPerCu = 2;             // LDS-tiled workgroups a CU holds (two 66 KiB tile pairs)
constexpr int kBalanceSetThreads = 1024;             // threads of a tile pair's workgroup
constexpr int kBalanceSetSmallMaxK = 5;              // up to here a table has no 64 x 64 tile: the flat kernel

// ---- balance: the persistent grid over the flat item list ---------------------------------------------------------------------
KPAL_MATRIX_HD uint64_t balance_set_items(uint64_t n_tables, uint64_t ncanon) { return n_tables * ncanon; }
KPAL_MATRIX_HD uint64_t balance_set_slots(uint64_t num_cu) { return (num_cu > 0 ? num_cu : 1) * (uint64_t)kBalanceSetSlotsPerCu; }
KPAL_MATRIX_HD uint64_t balance_set_rounds(uint64_t items, uint64_t slots)
{
    if (slots == 0) slots = 1;
    return items / slots + (items % slots != 0 ? 1 : 0);
}
KPAL_MATRIX_HD uint64_t balance_set_workgroups(uint64_t items, uint64_t slots)
{
    const uint64_t rounds = balance_set_rounds(items, slots);
    return rounds == 0 ? 0 : items / rounds + (items % rounds != 0 ? 1 : 0);
}
// Items of workgroup g of `grid`: g, g + grid, ... below `items`.
KPAL_MATRIX_HD uint64_t balance_set_share(uint64_t items, uint64_t grid, uint64_t g)
{
    return g >= items || grid == 0 ? 0 : (items - g - 1) / grid + 1;
}

// ---- shrink: one launch over all entries, or one per table ------------------------------------------------------------------------
// The shrink of a set is the flat shrink of its entries, and for small tables one launch is what pays (tools/transformbench.py:
// 20 000 x k = 6 570 times, 4 000 x k = 8 35 times the loop).  At 64 x k = 12 the one launch over 2^30 entries LOST to 64
// launches of 2^24: 1.77 - 1.82 ms against 1.60 ms, the same kernel on the same grid -- its workgroups stride through the whole
// set and drift apart, a launch per table brings them together every 128 MiB.  So from k = 12 on a table is a launch.
constexpr int kShrinkSetPerTableMinK = 12;
KPAL_MATRIX_HD uint64_t shrink_set_launches(int k, uint64_t n_tables) { return k >= kShrinkSetPerTableMinK ? n_tables : (n_tables > 0 ? 1 : 0); }

// ---- pool: column groups and table slices -----------------------------------------------------------------------------------------
constexpr int kPoolThreads = 256;                    // threads of a column group: one 16-byte column pair each
constexpr int kPoolUnroll = 4;                       // tables a thread has in flight
constexpr uint64_t kPoolGroupsPerCu = 8;             // workgroups a CU should see before the tables are cut no further
constexpr uint64_t kPoolMinSliceTables = 16;         // a slice shorter than this is not worth its row of partials
constexpr uint64_t kPoolOneSliceBins = 1ULL << 20;   // from here (k = 10) the column groups alone fill the device

KPAL_MATRIX_HD uint64_t pool_column_pairs(uint64_t bins) { return bins / 2 + (bins & 1); }
KPAL_MATRIX_HD uint64_t pool_column_groups(uint64_t bins)
{
    const uint64_t pairs = pool_column_pairs(bins);
    return pairs / kPoolThreads + (pairs % kPoolThreads != 0 ? 1 : 0);
}
KPAL_MATRIX_HD uint64_t pool_slices(uint64_t n_tables, uint64_t bins, uint64_t num_cu)
{
    if (n_tables <= 1 || bins >= kPoolOneSliceBins) return 1;
    const uint64_t groups = pool_column_groups(bins), want_groups = (num_cu > 0 ? num_cu : 1) * kPoolGroupsPerCu;
    const uint64_t by_device = want_groups / groups + (want_groups % groups != 0 ? 1 : 0);
    const uint64_t by_tables = n_tables / kPoolMinSliceTables + (n_tables % kPoolMinSliceTables != 0 ? 1 : 0);
    uint64_t s = by_device < by_tables ? by_device : by_tables;
    if (s > n_tables) s = n_tables;
    return s < 1 ? 1 : s;
}
// Slice s of `slices` takes the tables [begin, end): the first n_tables % slices slices are one table longer.
KPAL_MATRIX_HD uint64_t pool_slice_begin(uint64_t n_tables, uint64_t slices, uint64_t s)
{
    const uint64_t q = n_tables / slices, r = n_tables % slices;
    return s * q + (s < r ? s : r);
}
KPAL_MATRIX_HD uint64_t pool_slice_end(uint64_t n_tables, uint64_t slices, uint64_t s) { return pool_slice_begin(n_tables, slices, s + 1); }
inline uint64_t pool_scratch_bytes(uint64_t slices, uint64_t bins) { return slices > 1 ? slices * bins * 8 : 0; }

// ---- input against output ---------------------------------------------------------------------------------------------------------
enum TransformOverlap { kTransformDisjoint = 0, kTransformSame = 1, kTransformPartial = 2 };
// The byte ranges [a, a + a_bytes) and [b, b + b_bytes) (neither wraps): disjoint, the SAME range, or anything else.
KPAL_MATRIX_HD int transform_overlap(uint64_t a, uint64_t a_bytes, uint64_t b, uint64_t b_bytes)
{
    if (a == b && a_bytes == b_bytes) return kTransformSame;
    if (a_bytes == 0 || b_bytes == 0) return kTransformDisjoint;
    if (a < b ? b - a >= a_bytes : a - b >= b_bytes) return kTransformDisjoint;
    return kTransformPartial;
}

// n_tables tables of `bins` int64 entries: whether their bytes fit a size_t (bins > 0, n_tables > 0).
KPAL_MATRIX_HD bool transform_bytes_fit(uint64_t n_tables, uint64_t bins)
{
    return bins <= (UINT64_MAX / 8) / n_tables && bins <= ((uint64_t)SIZE_MAX / 8) / n_tables;
}

}  // namespace kpal
