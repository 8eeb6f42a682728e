// pool_groups_plan.hpp -- what the host decides about the pool of a set of tables BY LABEL before it launches anything: which
// tables every group adds up, how the long lists are cut, and what goes to the device as the index of the kernels
// (kpal_pool_groups_device; the kernels: pool_groups_kernels.hpp).  No GPU in it: kpal_pool_groups.hip, the kernels and a CPU
// program (tests/test_pool_groups_plan_host.py) read the same definitions.  The column groups, the unroll and the three numbers
// of the cut are those of the pool of a whole set (transform_plan.hpp).
//
// labels[t] of the n_tables consecutive tables: a label in [0, n_groups) names the group of table t, a negative one no group, a
// label >= n_groups is refused.  The plan is an inverted index and a cut of its long lists:
//   MEMBERS  a stable counting sort gives every group the list of its tables in ascending table order; the lists lie one
//            behind the other in group order.
//   CHUNKS   a list of L members is cut into ceil(L / chunk_tables) chunks of the same length to within one (the first L %
//            chunks of them are one longer), so none is longer than chunk_tables.  chunk_tables comes from n_tables, bins and
//            the device alone -- ceil(n_tables / (kPoolGroupsPerCu x CUs / column groups)), so that the chunks of ALL lists
//            together fill the device however the tables are spread over the groups, and never below kPoolMinSliceTables (a
//            chunk costs a row of partials); from kPoolOneSliceBins on the column groups alone fill the device and no list is
//            cut.  One group of everything gets the slices of pool_slices; a group of 90 % of the tables gets 90 % of the chunks
//            and no workgroup walks more than chunk_tables tables.
//   ITEMS    NOT CUT (no list has two chunks): item g is group g, its list may be empty, its row is row g of the output -- one
//            launch.  CUT: the items of the first pass are the chunks of all groups in group order, item i writes row i of the
//            partial rows in context scratch; the second pass has item g = group g again, whose list is the RANGE of its
//            partial rows (consecutive, in chunk order: no member list) -- two launches.  Integer addition is order-free: the
//            bits do not depend on the cut.  An item with an empty list writes zeros, or with `accumulate` nothing.
//   PACKING  a table of fewer than kPoolThreads column pairs leaves most of a column group idle: an item then takes `lanes`
//            threads -- the power of two that holds its column pairs -- and a workgroup takes kPoolThreads / lanes items.  From
//            64 lanes on an item is still the same for a whole wave.
// The index is ONE array of 32-bit words for one upload: members | begin of every first-pass item (items + 1) | with a cut the
// begin of every group's partial rows (n_groups + 1).
#pragma once
#include <vector>

#include "transform_plan.hpp"

namespace kpal {

constexpr uint64_t kPoolGroupsMaxIndex = 0x7FFFFFFFULL;   // tables, groups, items: 32-bit words the kernels may add an unroll to
constexpr int kPoolGroupsFinalUnroll = 16;                // partial rows a thread of the second pass has in flight (kPoolUnroll tables in the first)
constexpr uint32_t kPoolGroupsMaxGridY = 65535;           // workgroups of items side by side; the kernel strides over the rest

enum PoolGroupsStatus { kPoolGroupsOk = 0, kPoolGroupsBadLabel = 1, kPoolGroupsTooMany = 2 };

// ---- the cut ----------------------------------------------------------------------------------------------------------------------
KPAL_MATRIX_HD uint64_t pool_groups_chunk_tables(uint64_t n_tables, uint64_t bins, uint64_t num_cu)
{
    if (bins >= kPoolOneSliceBins) return n_tables > 0 ? n_tables : 1;
    const uint64_t groups = pool_column_groups(bins), want_groups = (num_cu > 0 ? num_cu : 1) * kPoolGroupsPerCu;
    const uint64_t by_device = want_groups / groups + (want_groups % groups != 0 ? 1 : 0);
    const uint64_t c = n_tables / by_device + (n_tables % by_device != 0 ? 1 : 0);
    return c < kPoolMinSliceTables ? kPoolMinSliceTables : c;
}
KPAL_MATRIX_HD uint64_t pool_groups_chunks(uint64_t members, uint64_t chunk_tables)
{
    return members / chunk_tables + (members % chunk_tables != 0 ? 1 : 0);
}
// Chunk q of `chunks` of a list of `members` begins at this place of the list (q == chunks: its end).
KPAL_MATRIX_HD uint64_t pool_groups_chunk_begin(uint64_t members, uint64_t chunks, uint64_t q) { return pool_slice_begin(members, chunks, q); }

// ---- the packing of small tables ------------------------------------------------------------------------------------------------
// log2 of the threads of an item: kPoolThreads of them (8) unless fewer column pairs fill the table.
KPAL_MATRIX_HD int pool_groups_lane_shift(uint64_t bins)
{
    const uint64_t pairs = pool_column_pairs(bins);
    int s = 0;
    while (s < 8 && (1ULL << s) < pairs) ++s;
    return s;
}
KPAL_MATRIX_HD uint64_t pool_groups_items_per_workgroup(uint64_t bins) { return (uint64_t)kPoolThreads >> pool_groups_lane_shift(bins); }
KPAL_MATRIX_HD uint64_t pool_groups_item_workgroups(uint64_t items, uint64_t bins)
{
    const uint64_t per = pool_groups_items_per_workgroup(bins);
    return items / per + (items % per != 0 ? 1 : 0);
}

// ---- sizes ------------------------------------------------------------------------------------------------------------------------
// Whether tables, groups and the bytes of tables and output fit the 32-bit words of the index and a size_t (all > 0).
KPAL_MATRIX_HD bool pool_groups_fit(uint64_t n_tables, uint64_t n_groups, uint64_t bins)
{
    return n_tables <= kPoolGroupsMaxIndex && n_groups <= kPoolGroupsMaxIndex && pool_column_groups(bins) <= kPoolGroupsMaxIndex &&
           transform_bytes_fit(n_tables, bins) && transform_bytes_fit(n_groups, bins);
}
inline uint64_t pool_groups_scratch_bytes(bool cut, uint64_t items, uint64_t bins) { return cut ? items * bins * 8 : 0; }

struct PoolGroupsPlan {
    uint64_t chunk_tables = 0;
    uint64_t members = 0;          // tables with a label
    uint64_t items = 0;            // items of the first (or only) pass
    uint64_t n_groups = 0;
    bool cut = false;              // a second pass adds the partial rows
    uint64_t scratch_bytes = 0;    // partial rows
    int64_t bad_table = -1;        // kPoolGroupsBadLabel: the first table whose label is >= n_groups
    std::vector<uint32_t> index;   // members | begin[items + 1] | cut: group_begin[n_groups + 1]
    size_t members_at() const { return 0; }
    size_t begin_at() const { return (size_t)members; }
    size_t group_begin_at() const { return (size_t)(members + items + 1); }
    uint64_t index_bytes() const { return (uint64_t)index.size() * 4; }
};

// The plan of labels[0, n_tables) over n_groups groups (n_tables, n_groups, bins > 0 and pool_groups_fit: the caller's).
inline int pool_groups_plan(const int64_t *labels, uint64_t n_tables, uint64_t n_groups, uint64_t bins, uint64_t num_cu, PoolGroupsPlan &plan)
{
    plan = PoolGroupsPlan();
    plan.n_groups = n_groups;
    plan.chunk_tables = pool_groups_chunk_tables(n_tables, bins, num_cu);
    // counting sort, pass 1: the length of every list
    std::vector<uint32_t> first(n_groups + 1, 0);
    for (uint64_t t = 0; t < n_tables; ++t) {
        const int64_t l = labels[t];
        if (l < 0) continue;
        if ((uint64_t)l >= n_groups) {
            plan.bad_table = (int64_t)t;
            plan.members = 0;
            return kPoolGroupsBadLabel;
        }
        ++first[(size_t)l + 1];
        ++plan.members;
    }
    uint64_t chunks_all = 0;
    for (uint64_t g = 0; g < n_groups; ++g) {
        const uint64_t c = pool_groups_chunks(first[g + 1], plan.chunk_tables);
        if (c > 1) plan.cut = true;
        chunks_all += c;
        first[g + 1] += first[g];
    }
    plan.items = plan.cut ? chunks_all : n_groups;
    if (plan.items > kPoolGroupsMaxIndex || (plan.cut && !transform_bytes_fit(plan.items, bins))) return kPoolGroupsTooMany;
    plan.scratch_bytes = pool_groups_scratch_bytes(plan.cut, plan.items, bins);
    plan.index.resize((size_t)(plan.members + plan.items + 1 + (plan.cut ? n_groups + 1 : 0)));
    // pass 2, stable: the tables of a group in ascending order
    {
        std::vector<uint32_t> at(first.begin(), first.end() - 1);
        uint32_t *members = plan.index.data() + plan.members_at();
        for (uint64_t t = 0; t < n_tables; ++t)
            if (labels[t] >= 0) members[at[(size_t)labels[t]]++] = (uint32_t)t;
    }
    uint32_t *begin = plan.index.data() + plan.begin_at();
    if (!plan.cut) {
        for (uint64_t g = 0; g <= n_groups; ++g) begin[g] = first[g];
        return kPoolGroupsOk;
    }
    uint32_t *group_begin = plan.index.data() + plan.group_begin_at();
    uint64_t item = 0;
    for (uint64_t g = 0; g < n_groups; ++g) {
        const uint64_t len = first[g + 1] - first[g], c = pool_groups_chunks(len, plan.chunk_tables);
        group_begin[g] = (uint32_t)item;
        for (uint64_t q = 0; q < c; ++q) begin[item++] = (uint32_t)(first[g] + pool_groups_chunk_begin(len, c, q));
    }
    group_begin[n_groups] = (uint32_t)item;
    begin[item] = (uint32_t)plan.members;
    return kPoolGroupsOk;
}

}  // namespace kpal
