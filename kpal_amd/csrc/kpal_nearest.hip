// kpal_nearest.hip -- kpal_cross_nearest[_device]: the n nearest right profiles of every left profile, selected on the device.
// The Q x R rectangle is cut into tiles (nearest_plan.hpp); a tile is the launches of the rectangle cores of kpal_cross.hip up
// to where their host loops begin, one reduction, a kernel that finishes the tile's distances where the host loops would
// (nearest_kernels.hpp) and one that merges every row of them into the n best of that row, which stay on the device over the
// tiles of a band and are downloaded once per band.  Option sets with dynamic smoothing compute a tile with
// kpal_cross_smooth_distance_device into a host buffer of that tile and merge on the host, under the same order.
#include "kpal_host.hpp"
#include "dist_host.hpp"

#include "nearest_kernels.hpp"

// Workspace of a tile: nearest_plan.hpp's default, or KPAL_NEAREST_BUDGET bytes (read on every call: timing, tests).
static uint64_t nearest_budget()
{
    const char *e = getenv("KPAL_NEAREST_BUDGET");
    const unsigned long long v = e ? strtoull(e, nullptr, 10) : 0ULL;
    return v ? (uint64_t)v : kNearestBudgetBytes;
}

static int reduce_to_result(kpal_ctx *ctx, uint64_t groups, uint32_t gx)
{
    CHK(ensure(ctx, ctx->result, (size_t)groups * sizeof(Partial)));
    return reduce_partials(ctx, (const Partial *)ctx->partials.p, (uint32_t)groups, gx, (Partial *)ctx->result.p);
}

// The distances of every pair of the (balanced) tile c at dd, row-major: the route of cross_core / cross_option_core, finished
// on the device.  flag: one device word for the exactness test of the Gram path.
static int tile_distances(kpal_ctx *ctx, const CrossSets &c, const kpal_distance_options *opt, const NearestKind &kind, double *dd, uint32_t *flag)
{
    const unsigned grid = stream_grid(ctx, (uint64_t)c.Q * (uint64_t)c.R);
    if (kind.route == kNearestOption) {
        CrossGrid g;
        CHK(cross_option_launch(ctx, c, opt, &g));
        const uint32_t nacc = option_nacc(opt->metric);
        CHK(reduce_to_result(ctx, g.slots * nacc, g.gx));
        LAUNCH(ctx, "nearest_finish", nearest_finish_slots_kernel, dim3(grid), dim3(256), (const Partial *)ctx->result.p, c, g.sideR, g.slots, nacc,
               opt->metric, opt->do_scale ? 1 : 0, dd);
        return KPAL_OK;
    }
    const bool staged = cross_staged(c.Q, c.R, c.n);
    if (kind.route == kNearestGram && staged) {
        CrossGramLayout lay;
        CHK(cross_gram_launch(ctx, c, &lay));
        CHK(reduce_to_result(ctx, lay.groups, lay.gx));
        HIPCHK(hipMemsetAsync(flag, 0, sizeof(uint32_t), ctx->stream));
        LAUNCH(ctx, "nearest_finish_gram", nearest_finish_gram_kernel, dim3(grid), dim3(256), (const Partial *)ctx->result.p, c.Q, c.R, lay.blocksR,
               (uint64_t)lay.dots, dd, flag);
        uint32_t inexact = 0;
        HIPCHK(hipMemcpyAsync(&inexact, flag, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (!inexact) return KPAL_OK;   // else some |x|^2 >= 2^53: the wrapping-int64 kernels, as cross_core
    }
    CrossGrid g;
    CHK(cross_pairs_launch(ctx, c, opt->metric, staged, true, &g));
    CHK(reduce_to_result(ctx, g.slots, g.gx));
    LAUNCH(ctx, "nearest_finish", nearest_finish_slots_kernel, dim3(grid), dim3(256), (const Partial *)ctx->result.p, c, g.sideR, g.slots, 1u, opt->metric, 0, dd);
    return KPAL_OK;
}

// Dynamic smoothing: every tile through the existing entry into a host buffer of one tile, merged row by row on the host.
static int nearest_host_select(kpal_ctx *ctx, int k, int Q, const int64_t *dev_left, int R, const int64_t *dev_right, const kpal_distance_options *opt,
                               int n, int64_t right_first, int have, const NearestPlan &plan, double *dist, int64_t *index)
{
    const uint64_t bins = 1ULL << (2 * k);
    std::vector<double> tile((size_t)plan.tile_q * (size_t)plan.tile_r);
    std::vector<NearestCand> best(n);
    for (const NearestTile &t : plan.tiles) {
        const int Qt = t.q1 - t.q0, Rt = t.r1 - t.r0;
        CHK(kpal_cross_smooth_distance_device(ctx, k, Qt, dev_left + (uint64_t)t.q0 * bins, Rt, dev_right + (uint64_t)t.r0 * bins, opt, tile.data()));
        const int had = (int)std::min<int64_t>(n, (int64_t)have + t.r0);
        for (int q = 0; q < Qt; ++q) {
            double *d = dist + (size_t)(t.q0 + q) * n;
            int64_t *x = index + (size_t)(t.q0 + q) * n;
            for (int j = 0; j < had; ++j) best[j] = NearestCand{d[j], x[j]};
            const int kept = nearest_merge_host(best.data(), had, n, tile.data() + (size_t)q * Rt, Rt, right_first + t.r0);
            for (int j = 0; j < n; ++j) {
                d[j] = j < kept ? best[j].dist : std::nan("");
                x[j] = j < kept ? best[j].index : -1;
            }
        }
    }
    return KPAL_OK;
}

KPAL_API int kpal_cross_nearest_device(kpal_ctx *ctx, int k, int Q, const int64_t *dev_left, int R, const int64_t *dev_right,
                                       const kpal_distance_options *opt, int n, int64_t right_first, int have, int tile_q, int tile_r,
                                       double *dist_inout, int64_t *index_inout)
{
    CTX_ENTER(ctx);
    CHK(check_options(opt));
    CHK(cross_check(k, Q, R, 0, dev_left, dev_right, index_inout ? dist_inout : nullptr));   // (both outputs)
    CHK(tables_aligned(dev_left, dev_right));
    if (n < 1 || n > KPAL_NEAREST_MAX) return set_err(KPAL_E_INVALID, "nearest: n=%d out of range 1..%d", n, KPAL_NEAREST_MAX);
    if (have < 0 || have > n) return set_err(KPAL_E_INVALID, "nearest: have=%d out of range 0..n=%d", have, n);
    if (tile_q < 0 || tile_r < 0) return set_err(KPAL_E_INVALID, "nearest: negative tile cap");
    const uint64_t bins = 1ULL << (2 * k);
    const NearestKind kind = nearest_kind(opt);
    const NearestPlan plan = nearest_plan(bins, ctx->num_cu, kind, Q, R, nearest_budget(), tile_q, tile_r);
    if (kind.route == kNearestSmooth)
        return nearest_host_select(ctx, k, Q, dev_left, R, dev_right, opt, n, right_first, have, plan, dist_inout, index_inout);

    const size_t tq = (size_t)plan.tile_q, tr = (size_t)plan.tile_r;
    CHK(ensure(ctx, ctx->near_dist, tq * tr * sizeof(double) + 16));
    CHK(ensure(ctx, ctx->near_best, tq * (size_t)n * 16));
    if (opt->do_balance) CHK(ensure(ctx, ctx->scratch[kScratchBalanced], (tq + tr) * bins * 8));
    double *dd = (double *)ctx->near_dist.p;
    uint32_t *flag = (uint32_t *)(dd + tq * tr);
    double *best_d = (double *)ctx->near_best.p;
    int64_t *best_i = (int64_t *)(best_d + tq * (size_t)n);
    int64_t *bal_left = (int64_t *)ctx->scratch[kScratchBalanced].p, *bal_right = bal_left ? bal_left + tq * bins : nullptr;
    const int64_t *band_left = nullptr;
    for (const NearestTile &t : plan.tiles) {
        const int Qt = t.q1 - t.q0, Rt = t.r1 - t.r0;
        const size_t row0 = (size_t)t.q0 * (size_t)n, band = (size_t)Qt * (size_t)n;
        if (t.r0 == 0) {   // a band begins: its running best from the caller, its left tables balanced once
            if (have > 0) {
                HIPCHK(hipMemcpyAsync(best_d, dist_inout + row0, band * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
                HIPCHK(hipMemcpyAsync(best_i, index_inout + row0, band * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream));
            }
            band_left = dev_left + (uint64_t)t.q0 * bins;
            if (opt->do_balance) {
                CHK(balance_set(ctx, k, Qt, band_left, bal_left));
                band_left = bal_left;
            }
        }
        const int64_t *right = dev_right + (uint64_t)t.r0 * bins;
        if (opt->do_balance) {
            CHK(balance_set(ctx, k, Rt, right, bal_right));
            right = bal_right;
        }
        const CrossSets c = {band_left, right, Qt, Rt, bins, 0};
        CHK(tile_distances(ctx, c, opt, kind, dd, flag));
        const int had = (int)std::min<int64_t>(n, (int64_t)have + t.r0);
        LAUNCH(ctx, "nearest_select", nearest_select_kernel, dim3((unsigned)Qt), dim3(kNearestThreads), (const double *)dd, (uint32_t)Rt,
               right_first + (int64_t)t.r0, n, had, best_d, best_i);
        if (t.r1 == R) {   // the band ends: Qt x n distances and indices
            HIPCHK(hipMemcpyAsync(dist_inout + row0, best_d, band * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipMemcpyAsync(index_inout + row0, best_i, band * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
        }
    }
    return KPAL_OK;
}

KPAL_API int kpal_cross_nearest(kpal_ctx *ctx, int k, int Q, const int64_t *const *host_left, int R, const int64_t *const *host_right,
                                const kpal_distance_options *opt, int n, int64_t right_first, int have, int tile_q, int tile_r,
                                double *dist_inout, int64_t *index_inout)
{
    CTX_ENTER(ctx);
    CHK(check_options(opt));
    CHK(cross_check(k, Q, R, 0, host_left, host_right, index_inout ? dist_inout : nullptr));   // (both outputs)
    int64_t *dl = nullptr, *dr = nullptr;
    CHK(upload_rectangle(ctx, 1ULL << (2 * k), Q, host_left, R, host_right, &dl, &dr));
    return kpal_cross_nearest_device(ctx, k, Q, dl, R, dr, opt, n, right_first, have, tile_q, tile_r, dist_inout, index_inout);
}
