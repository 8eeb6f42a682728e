// kpal_transform.hip -- the part of the C-ABI that makes new tables out of a whole SET of count tables lying one behind the
// other: the balance and the shrink of every table and the pool (the sum) of all of them, in a number of launches that does not
// grow with the set -- but for the shrink of tables of k >= 12, which was measured to be faster a launch per table -- (planned by
// transform_plan.hpp; the kernels: transform_set_kernels.hpp, and stat_kernels.hpp for the shrink).  Everything is queued on the context's stream; nothing here waits for the device.  (The merge of two sets is
// kpal_merge_device over all their entries: kpal_vec.hip.)
#include "kpal_host.hpp"

#include "stat_kernels.hpp"
#include "transform_set_kernels.hpp"

static int transform_set_check(int k, size_t n_tables, const int64_t *in, const int64_t *out)
{
    if (k < 1 || k > KPAL_MAX_K) return set_err(KPAL_E_INVALID, "k=%d out of range", k);
    if (!in || !out) return set_err(KPAL_E_INVALID, "NULL pointer");
    if (n_tables == 0) return set_err(KPAL_E_INVALID, "empty set");
    if ((uintptr_t)in % 8 != 0 || (uintptr_t)out % 8 != 0) return set_err(KPAL_E_INVALID, "tables are not 8-byte aligned");
    if (!transform_bytes_fit(n_tables, 1ULL << (2 * k))) return set_err(KPAL_E_INVALID, "%zu tables at k=%d: too many bytes", n_tables, k);
    return KPAL_OK;
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
    CHK(transform_set_check(k, n_tables, dev_in, dev_out));
    const uint64_t total = (uint64_t)n_tables << (2 * k);
    if (transform_overlap((uint64_t)(uintptr_t)dev_in, total * 8, (uint64_t)(uintptr_t)dev_out, total * 8) == kTransformPartial)
        return set_err(KPAL_E_INVALID, "balance of a set: the output overlaps the input without being the input");
    return balance_set_launch(ctx, k, n_tables, dev_in, dev_out);
}

KPAL_API int kpal_shrink_set_device(kpal_ctx *ctx, int k, int factor, size_t n_tables, const int64_t *dev_in, int64_t *dev_out)
{
    CTX_ENTER(ctx);
    if (k < 1 || k > KPAL_MAX_K) return set_err(KPAL_E_INVALID, "k=%d out of range", k);
    if (factor < 1 || factor >= k) return set_err(KPAL_E_INVALID, "Reduction factor should be smaller than k-mer size.");
    CHK(transform_set_check(k, n_tables, dev_in, dev_out));
    // 4^factor divides 4^k: the shrink of the tables is the flat shrink of all their entries
    const uint64_t n = (uint64_t)n_tables << (2 * k), m = 1ULL << (2 * factor), n_out = n / m;
    if (transform_overlap((uint64_t)(uintptr_t)dev_in, n * 8, (uint64_t)(uintptr_t)dev_out, n_out * 8) != kTransformDisjoint)
        return set_err(KPAL_E_INVALID, "shrink of a set: the output overlaps the input");
    // ... in one launch, or in one per table where that was measured to be faster (transform_plan.hpp)
    const uint64_t launches = shrink_set_launches(k, n_tables), ln = n / launches, ln_out = n_out / launches;
    for (uint64_t l = 0; l < launches; ++l) {
        const int64_t *in = dev_in + l * ln;
        int64_t *out = dev_out + l * ln_out;
        if (m <= 64 && (uintptr_t)dev_in % 16 == 0) {   // (the shuffle form reads 16 bytes at a time)
            LAUNCH(ctx, "shrink_set", shrink_small_kernel, dim3(stream_grid(ctx, ln / 2)), dim3(256), in, ln / 2, (int)(m / 2), out);
        } else {
            LAUNCH(ctx, "shrink_set", shrink_large_kernel, dim3(stream_grid(ctx, ln_out * 64)), dim3(256), in, ln_out, m, out);
        }
    }
    return KPAL_OK;
}

// One pass of the pool kernel: `slices` rows at `out` from the tables at `tables`.
static int launch_pool(kpal_ctx *ctx, const char *name, const int64_t *tables, uint64_t n_tables, uint64_t bins, uint64_t slices, int accumulate, int64_t *out)
{
    const dim3 grid((unsigned)pool_column_groups(bins), (unsigned)slices), block(kPoolThreads);
    const bool vec = bins % 2 == 0 && (uintptr_t)tables % 16 == 0 && (uintptr_t)out % 16 == 0;
    if (vec) LAUNCH(ctx, name, (pool_set_kernel<true>), grid, block, tables, n_tables, bins, (uint32_t)slices, accumulate, out);
    else LAUNCH(ctx, name, (pool_set_kernel<false>), grid, block, tables, n_tables, bins, (uint32_t)slices, accumulate, out);
    return KPAL_OK;
}

KPAL_API int kpal_pool_set_device(kpal_ctx *ctx, size_t n_tables, size_t bins, const int64_t *dev_tables, int accumulate, int64_t *dev_out)
{
    CTX_ENTER(ctx);
    if (!dev_tables || !dev_out) return set_err(KPAL_E_INVALID, "NULL pointer");
    if (n_tables == 0) return set_err(KPAL_E_INVALID, "empty set");
    if (bins == 0) return set_err(KPAL_E_INVALID, "empty vector");
    if ((uintptr_t)dev_tables % 8 != 0 || (uintptr_t)dev_out % 8 != 0) return set_err(KPAL_E_INVALID, "tables are not 8-byte aligned");
    if (!transform_bytes_fit(n_tables, bins) || pool_column_groups(bins) > 0x7FFFFFFFULL)
        return set_err(KPAL_E_INVALID, "%zu tables of %zu bins: too many bytes", n_tables, bins);
    if (transform_overlap((uint64_t)(uintptr_t)dev_tables, (uint64_t)n_tables * bins * 8, (uint64_t)(uintptr_t)dev_out, (uint64_t)bins * 8) != kTransformDisjoint)
        return set_err(KPAL_E_INVALID, "pool of a set: the output overlaps the tables");
    const uint64_t slices = pool_slices(n_tables, bins, (uint64_t)ctx->num_cu);
    if (slices == 1) return launch_pool(ctx, "pool_set", dev_tables, n_tables, bins, 1, accumulate ? 1 : 0, dev_out);
    // integer addition is order-free: the partial rows of the slices, then their sum, give the same bits as one walk
    CHK(ensure(ctx, ctx->partials, (size_t)pool_scratch_bytes(slices, bins)));
    int64_t *rows = (int64_t *)ctx->partials.p;
    CHK(launch_pool(ctx, "pool_set", dev_tables, n_tables, bins, slices, 0, rows));
    return launch_pool(ctx, "pool_set_final", rows, slices, bins, 1, accumulate ? 1 : 0, dev_out);
}
