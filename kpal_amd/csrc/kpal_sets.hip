// kpal_sets.hip -- the part of the C-ABI that works on a whole SET of count vectors lying one behind the other: the summaries
// and the strand balance of every profile, in a number of launches that does not grow with the set (planned by stat_plan.hpp,
// the kernels in stat_set_kernels.hpp).  The strand balance of ONE vector is here too: a set of one table, no other implementation.
#include "kpal_host.hpp"
#include "table_host.hpp"

#include "stat_set_kernels.hpp"

// The summaries of `count` consecutive tables: 8 launches and 2 per digit, 2 synchronisations.
static int stats_set_pass(kpal_ctx *ctx, uint64_t count, uint64_t bins, const int64_t *dev_tables, kpal_profile_stats *host_out)
{
    const uint64_t slices = stat_slices(bins);
    // the pass's scratch, one array behind the other (every size a multiple of 8): partials, histograms, states, summaries, two words
    const uint64_t partial_bytes = count * slices * kStatPartialBytes, hist_bytes = count * kStatHistBytes;
    const uint64_t state_bytes = count * kStatStateBytes, out_bytes = count * kStatOutBytes;
    CHK(ensure(ctx, ctx->partials, (size_t)(count * stat_scratch_bytes(bins) + 8)));
    uint8_t *base = (uint8_t *)ctx->partials.p;
    StatPartial *partial = (StatPartial *)base;
    unsigned long long *hist = (unsigned long long *)(base + partial_bytes);
    StatSetState *state = (StatSetState *)(base + partial_bytes + hist_bytes);
    kpal_profile_stats *out = (kpal_profile_stats *)(base + partial_bytes + hist_bytes + state_bytes);
    int *top_max = (int *)(base + partial_bytes + hist_bytes + state_bytes + out_bytes);
    uint32_t *error = (uint32_t *)(top_max + 1);
    HIPCHK(hipMemsetAsync(hist, 0, (size_t)hist_bytes, ctx->stream));
    HIPCHK(hipMemsetAsync(top_max, 0xFF, 4, ctx->stream));   // -1
    HIPCHK(hipMemsetAsync(error, 0, 4, ctx->stream));
    const dim3 grid((unsigned)slices, (unsigned)count), block(kStatSetThreads);
    LAUNCH(ctx, "stats_set", stats_set_kernel, grid, block, dev_tables, bins, partial);
    LAUNCH(ctx, "stats_set_final", stats_set_final_kernel, dim3((unsigned)count), dim3(64), (const StatPartial *)partial, (uint32_t)slices, bins,
           state, out, top_max);
    LAUNCH(ctx, "var_set", var_set_kernel, grid, block, dev_tables, bins, (const StatSetState *)state, (double *)partial);
    LAUNCH(ctx, "var_set_final", var_set_final_kernel, dim3((unsigned)count), dim3(64), (const double *)partial, (uint32_t)slices, bins, out);
    int top = -1;
    HIPCHK(hipMemcpyAsync(&top, top_max, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // the one decision of the host: how many digits any profile of the pass needs
    if (top < -1 || top > 7) return set_err(KPAL_E_HIP, "stats of a set: top byte %d", top);
    for (int byte = top; byte >= 0; --byte) {
        LAUNCH(ctx, "select_hist_set", select_hist_set_kernel, grid, block, dev_tables, bins, (const StatSetState *)state, byte, hist);
        LAUNCH(ctx, "select_pick_set", select_pick_set_kernel, dim3((unsigned)count), dim3((unsigned)kStatHistBins), state, hist, bins, byte, error);
    }
    LAUNCH(ctx, "select_next_set", select_next_set_kernel, grid, block, dev_tables, bins, state);
    LAUNCH(ctx, "median_set", median_set_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), (const StatSetState *)state, bins, (uint32_t)count,
           out, error);
    uint32_t err = 0;
    HIPCHK(hipMemcpyAsync(host_out, out, (size_t)out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(&err, error, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (err & kStatErrRank) return set_err(KPAL_E_HIP, "median of a set: rank not found");
    if (err & kStatErrNext) return set_err(KPAL_E_HIP, "median of a set: upper middle value not found");
    return KPAL_OK;
}

KPAL_API int kpal_stats_set_device(kpal_ctx *ctx, size_t n_tables, size_t bins, const int64_t *dev_tables, kpal_profile_stats *host_out)
{
    CTX_ENTER(ctx);
    CHK(check_counted_set(n_tables, bins, dev_tables, host_out));
    const uint64_t per = stat_profiles_per_pass(stat_scratch_bytes(bins), kStatSetBudgetBytes, stat_set_cap());
    for (const StatChunk &c : stat_chunks(n_tables, per))
        CHK(stats_set_pass(ctx, c.count, bins, dev_tables + c.first * (uint64_t)bins, host_out + c.first));
    return KPAL_OK;
}

KPAL_API int kpal_stats_set(kpal_ctx *ctx, size_t n_tables, size_t bins, const int64_t *host_tables, kpal_profile_stats *host_out)
{
    CTX_ENTER(ctx);
    CHK(check_counted_set(n_tables, bins, host_tables, host_out));
    return for_uploaded_chunks(ctx, n_tables, bins, host_tables, [&](uint64_t first, uint64_t count, const int64_t *dev) {
        return kpal_stats_set_device(ctx, (size_t)count, bins, dev, host_out + first);
    });
}

// (the pairwise stands between the empty set and the alignment)
static int balance_set_check(int k, size_t n_tables, const int64_t *tables, int pairwise, const double *out)
{
    CHK(check_k(k));
    CHK(check_set(tables && out, n_tables));
    if (pairwise != KPAL_PAIRWISE_PROD && pairwise != KPAL_PAIRWISE_SUM) return set_err(KPAL_E_INVALID, "pairwise must be prod or sum");
    CHK(check_aligned(tables));
    return check_bytes_at_k(n_tables, k);
}

KPAL_API int kpal_strand_balance_set_device(kpal_ctx *ctx, int k, size_t n_tables, const int64_t *dev_tables, int pairwise, double *host_out)
{
    CTX_ENTER(ctx);
    CHK(balance_set_check(k, n_tables, dev_tables, pairwise, host_out));
    const uint64_t n = 1ULL << (2 * k);
    const unsigned gx = (unsigned)balance_set_grid(k);
    const uint64_t per = stat_profiles_per_pass(balance_set_scratch_bytes(k), kStatSetBudgetBytes, stat_set_cap());
    std::vector<Partial> res;
    for (const StatChunk &c : stat_chunks(n_tables, per)) {
        CHK(ensure(ctx, ctx->partials, (size_t)(c.count * balance_set_scratch_bytes(k))));
        const int64_t *dc = dev_tables + c.first * n;
        Partial *pp = (Partial *)ctx->partials.p;
        const dim3 grid(gx, (unsigned)c.count);
        if (k >= 6) {
            if (pairwise == KPAL_PAIRWISE_PROD) LAUNCH(ctx, "strand_balance_tiled_set", (strand_balance_tiled_set_kernel<0>), grid, dim3(1024), dc, k, pp);
            else LAUNCH(ctx, "strand_balance_tiled_set", (strand_balance_tiled_set_kernel<1>), grid, dim3(1024), dc, k, pp);
        } else {
            if (pairwise == KPAL_PAIRWISE_PROD) LAUNCH(ctx, "strand_balance_set", (strand_balance_set_kernel<0>), grid, dim3(256), dc, k, n, pp);
            else LAUNCH(ctx, "strand_balance_set", (strand_balance_set_kernel<1>), grid, dim3(256), dc, k, n, pp);
        }
        CHK(finish_partials(ctx, (uint32_t)c.count, gx, res));
        for (uint64_t i = 0; i < c.count; ++i) host_out[c.first + i] = finish_value(pairwise, res[i], nullptr);
    }
    return KPAL_OK;
}

KPAL_API int kpal_strand_balance_set(kpal_ctx *ctx, int k, size_t n_tables, const int64_t *host_tables, int pairwise, double *host_out)
{
    CTX_ENTER(ctx);
    CHK(balance_set_check(k, n_tables, host_tables, pairwise, host_out));
    return for_uploaded_chunks(ctx, n_tables, 1ULL << (2 * k), host_tables, [&](uint64_t first, uint64_t count, const int64_t *dev) {
        return kpal_strand_balance_set_device(ctx, k, (size_t)count, dev, pairwise, host_out + first);
    });
}

// One vector is a set of one table: the same checks with the same texts, the same kernels on the same grid, the same bits.
KPAL_API int kpal_strand_balance(kpal_ctx *ctx, int k, const int64_t *host_counts, int pairwise, double *out)
{
    return kpal_strand_balance_set(ctx, k, 1, host_counts, pairwise, out);
}
