// kpal_pool_groups.hip -- the part of the C-ABI that pools a SET of count tables lying one behind the other BY LABEL: one row per
// group, the sum of the tables that carry the group's label, in one launch, or in two when a long list is cut (planned by
// pool_groups_plan.hpp; the kernel: pool_groups_kernels.hpp).  Every table is read once, where it lies.  The index of the plan
// goes up in one copy; the launches are queued on the context's stream and nothing is downloaded.
#include "kpal_host.hpp"
#include "table_host.hpp"

#include "pool_groups_kernels.hpp"

// One pass of the kernel: `n_items` rows at `out` from the rows at `tables` -- LISTED: item i adds the rows members[begin[i]] ..
// members[begin[i + 1] - 1], else the rows begin[i] .. begin[i + 1] - 1 themselves.
template <bool LISTED>
static int launch_pool_groups(kpal_ctx *ctx, const char *name, const int64_t *tables, uint64_t bins, const uint32_t *members, const uint32_t *begin,
                              uint64_t n_items, int accumulate, int64_t *out)
{
    const int shift = pool_groups_lane_shift(bins);
    const uint64_t item_workgroups = pool_groups_item_workgroups(n_items, bins);
    const dim3 grid((unsigned)pool_column_groups(bins), (unsigned)std::min<uint64_t>(item_workgroups, kPoolGroupsMaxGridY)), block(kPoolThreads);
    const bool vec = pool_rows_by_16(bins, tables, out);
    const bool wave = shift >= 6;
    if (vec && wave) LAUNCH(ctx, name, (pool_groups_kernel<true, true, LISTED>), grid, block, tables, bins, members, begin, (uint32_t)n_items, shift, accumulate, out);
    else if (vec) LAUNCH(ctx, name, (pool_groups_kernel<true, false, LISTED>), grid, block, tables, bins, members, begin, (uint32_t)n_items, shift, accumulate, out);
    else if (wave) LAUNCH(ctx, name, (pool_groups_kernel<false, true, LISTED>), grid, block, tables, bins, members, begin, (uint32_t)n_items, shift, accumulate, out);
    else LAUNCH(ctx, name, (pool_groups_kernel<false, false, LISTED>), grid, block, tables, bins, members, begin, (uint32_t)n_items, shift, accumulate, out);
    return KPAL_OK;
}

KPAL_API int kpal_pool_groups_device(kpal_ctx *ctx, size_t n_tables, size_t bins, const int64_t *dev_tables, const int64_t *labels, size_t n_groups,
                                     int accumulate, int64_t *dev_out)
{
    CTX_ENTER(ctx);
    CHK(check_set(dev_tables && labels && dev_out, n_tables));
    CHK(check_vector(bins));
    if (n_groups == 0) return set_err(KPAL_E_INVALID, "no groups");
    CHK(check_aligned(dev_tables, dev_out));
    if (!pool_groups_fit(n_tables, n_groups, bins))
        return set_err(KPAL_E_INVALID, "%zu tables of %zu bins in %zu groups: too many bytes", n_tables, bins, n_groups);
    if (tables_overlap(dev_tables, (uint64_t)n_tables * bins * 8, dev_out, (uint64_t)n_groups * bins * 8) != kTransformDisjoint)
        return set_err(KPAL_E_INVALID, "pool of groups: the output overlaps the tables");
    PoolGroupsPlan plan;
    const int status = pool_groups_plan(labels, n_tables, n_groups, bins, (uint64_t)ctx->num_cu, plan);
    if (status == kPoolGroupsBadLabel)
        return set_err(KPAL_E_INVALID, "table %lld has label %lld: there are %zu groups", (long long)plan.bad_table, (long long)labels[plan.bad_table], n_groups);
    if (status != kPoolGroupsOk) return set_err(KPAL_E_INVALID, "%zu tables of %zu bins in %zu groups: too many bytes", n_tables, bins, n_groups);
    // the index: one copy, behind whatever still reads the index of an earlier call; its source is this call's, so it is waited for
    CHK(ensure(ctx, ctx->scratch[0], (size_t)plan.index_bytes()));
    if (plan.cut) CHK(ensure(ctx, ctx->partials, (size_t)plan.scratch_bytes));
    HIPCHK(hipMemcpyAsync(ctx->scratch[0].p, plan.index.data(), (size_t)plan.index_bytes(), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    const uint32_t *index = (const uint32_t *)ctx->scratch[0].p;
    const uint32_t *members = index + plan.members_at(), *begin = index + plan.begin_at();
    if (!plan.cut) return launch_pool_groups<true>(ctx, "pool_groups", dev_tables, bins, members, begin, plan.items, accumulate ? 1 : 0, dev_out);
    // integer addition is order-free: the partial rows of the chunks, then every group's sum of its own, give the bits of one walk
    int64_t *rows = (int64_t *)ctx->partials.p;
    CHK(launch_pool_groups<true>(ctx, "pool_groups", dev_tables, bins, members, begin, plan.items, 0, rows));
    return launch_pool_groups<false>(ctx, "pool_groups_final", rows, bins, nullptr, index + plan.group_begin_at(), n_groups, accumulate ? 1 : 0, dev_out);
}
