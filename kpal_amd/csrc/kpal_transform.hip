// kpal_transform.hip -- the part of the C-ABI that makes new tables out of a whole SET of count tables lying one behind the
// other: the balance and the shrink of every table and the pool (the sum) of all of them, in a number of launches that does not
// grow with the set -- but for the shrink of tables of k >= 12, which was measured to be faster a launch per table -- (planned by
// transform_plan.hpp; the kernels: transform_set_kernels.hpp; the shrink is shrink_launch of kpal_vec.hip).  Everything is
// queued on the context's stream; nothing here waits for the device.  The rungs of the checks: table_host.hpp.  (The merge of two
// sets is kpal_merge_device over all their entries: kpal_vec.hip.)
#include "kpal_host.hpp"
#include "table_host.hpp"

#include "transform_set_kernels.hpp"

// What follows k (and the factor of a shrink) for n_tables tables of 4^k entries at `in` and as many or fewer at `out`.
static int transform_set_check(int k, size_t n_tables, const int64_t *in, const int64_t *out)
{
    CHK(check_set(in && out, n_tables));
    CHK(check_aligned(in, out));
    return check_bytes_at_k(n_tables, k);
}

// The balance of n_tables consecutive tables (checked by the caller; dev_out the input itself or disjoint from it): one launch.
int balance_set_launch(kpal_ctx *ctx, int k, size_t n_tables, const int64_t *dev_in, int64_t *dev_out)
{
    const uint64_t total = (uint64_t)n_tables << (2 * k);
    if (k <= kBalanceSetSmallMaxK) {
        LAUNCH(ctx, "balance_set", balance_set_kernel, dim3(stream_grid(ctx, total)), dim3(256), dev_in, dev_out, k, total);
        return KPAL_OK;
    }
    const uint32_t *canon = nullptr;
    uint32_t ncanon = 0;
    unsigned one_table_grid = 1;
    CHK(canon_tiles(ctx, k, kBalanceSetSlotsPerCu, &canon, &ncanon, &one_table_grid));
    const uint64_t items = balance_set_items(n_tables, ncanon);
    const uint64_t grid = balance_set_workgroups(items, balance_set_slots((uint64_t)ctx->num_cu));
    LAUNCH(ctx, "balance_tiled_set", balance_tiled_set_kernel, dim3((unsigned)grid), dim3(kBalanceSetThreads), dev_in, dev_out, k, canon, ncanon, items);
    return KPAL_OK;
}

KPAL_API int kpal_balance_set_device(kpal_ctx *ctx, int k, size_t n_tables, const int64_t *dev_in, int64_t *dev_out)
{
    CTX_ENTER(ctx);
    CHK(check_k(k));
    CHK(transform_set_check(k, n_tables, dev_in, dev_out));
    const uint64_t total = (uint64_t)n_tables << (2 * k);
    if (tables_overlap(dev_in, total * 8, dev_out, total * 8) == kTransformPartial)
        return set_err(KPAL_E_INVALID, "balance of a set: the output overlaps the input without being the input");
    return balance_set_launch(ctx, k, n_tables, dev_in, dev_out);
}

KPAL_API int kpal_shrink_set_device(kpal_ctx *ctx, int k, int factor, size_t n_tables, const int64_t *dev_in, int64_t *dev_out)
{
    CTX_ENTER(ctx);
    CHK(check_shrink(k, factor));
    CHK(transform_set_check(k, n_tables, dev_in, dev_out));
    // 4^factor divides 4^k: the shrink of the tables is the flat shrink of all their entries
    const uint64_t n = (uint64_t)n_tables << (2 * k), m = 1ULL << (2 * factor), n_out = n / m;
    if (tables_overlap(dev_in, n * 8, dev_out, n_out * 8) != kTransformDisjoint) return set_err(KPAL_E_INVALID, "shrink of a set: the output overlaps the input");
    // ... in one launch, or in one per table where that was measured to be faster (transform_plan.hpp); the shuffle form's 16-byte loads only from an aligned input
    const uint64_t launches = shrink_set_launches(k, n_tables), ln = n / launches, ln_out = n_out / launches;
    for (uint64_t l = 0; l < launches; ++l) CHK(shrink_launch(ctx, "shrink_set", dev_in + l * ln, ln, m, dev_out + l * ln_out, (uintptr_t)dev_in % 16 == 0));
    return KPAL_OK;
}

// One pass of the pool kernel: `slices` rows at `out` from the tables at `tables`.
static int launch_pool(kpal_ctx *ctx, const char *name, const int64_t *tables, uint64_t n_tables, uint64_t bins, uint64_t slices, int accumulate, int64_t *out)
{
    const dim3 grid((unsigned)pool_column_groups(bins), (unsigned)slices), block(kPoolThreads);
    if (pool_rows_by_16(bins, tables, out)) LAUNCH(ctx, name, (pool_set_kernel<true>), grid, block, tables, n_tables, bins, (uint32_t)slices, accumulate, out);
    else LAUNCH(ctx, name, (pool_set_kernel<false>), grid, block, tables, n_tables, bins, (uint32_t)slices, accumulate, out);
    return KPAL_OK;
}

KPAL_API int kpal_pool_set_device(kpal_ctx *ctx, size_t n_tables, size_t bins, const int64_t *dev_tables, int accumulate, int64_t *dev_out)
{
    CTX_ENTER(ctx);
    CHK(check_set(dev_tables && dev_out, n_tables));
    CHK(check_vector(bins));
    CHK(check_aligned(dev_tables, dev_out));
    if (!transform_bytes_fit(n_tables, bins) || pool_column_groups(bins) > 0x7FFFFFFFULL) return too_many_bins(n_tables, bins);
    if (tables_overlap(dev_tables, (uint64_t)n_tables * bins * 8, dev_out, (uint64_t)bins * 8) != kTransformDisjoint)
        return set_err(KPAL_E_INVALID, "pool of a set: the output overlaps the tables");
    const uint64_t slices = pool_slices(n_tables, bins, (uint64_t)ctx->num_cu);
    if (slices == 1) return launch_pool(ctx, "pool_set", dev_tables, n_tables, bins, 1, accumulate ? 1 : 0, dev_out);
    // integer addition is order-free: the partial rows of the slices, then their sum, give the same bits as one walk
    CHK(ensure(ctx, ctx->partials, (size_t)pool_scratch_bytes(slices, bins)));
    int64_t *rows = (int64_t *)ctx->partials.p;
    CHK(launch_pool(ctx, "pool_set", dev_tables, n_tables, bins, slices, 0, rows));
    return launch_pool(ctx, "pool_set_final", rows, slices, bins, 1, accumulate ? 1 : 0, dev_out);
}
