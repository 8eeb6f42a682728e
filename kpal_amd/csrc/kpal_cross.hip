// kpal_cross.hip -- kpal_cross_distance[_device]: the Q x R rectangle of distances between a left and a right set of
// profiles in separate allocations (cross_kernels.hpp); cross_pairs also runs the lower triangle of kpal_vec.hip's matrices.  One call is a fixed number of launches whatever Q and R are:
// the balance of each profile (do_balance), one rectangle kernel (two when a fast form gives up on the values), one
// fixed-order reduction of the per-workgroup partials.
// kpal_cross_profile_distance[_device] / kpal_profile_distance_matrix_device: the same rectangle, and the lower triangle of one
// set, for a ProfileDistance with options (cross_option_kernels.hpp) -- a totals pass or a masked-totals rectangle pass more when
// the profiles are scaled; dynamic smoothing alone stays one pair pipeline per pair, on tables balanced once.
#include "kpal_host.hpp"

#include "cross_kernels.hpp"
#include "cross_option_kernels.hpp"

// Euclidean from the fp64 dot products of cross_gram_kernel and the norms of cross_norm_kernel.  *exact = false (and
// `out` untouched) when some |x|^2 >= 2^53 -- gram_euclidean's rule: the caller then takes the wrapping-int64 kernel.
static int cross_gram_euclidean(kpal_ctx *ctx, const CrossSets &c, double *out, bool *exact)
{
    const int blocksQ = (c.Q + 63) / 64, blocksR = (c.R + 63) / 64;
    const uint32_t nblocks = (uint32_t)blocksQ * (uint32_t)blocksR, nprof = (uint32_t)c.Q + (uint32_t)c.R;
    const uint64_t slabs = c.n / kGramBins;
    // one 132 KiB workgroup per CU
    const uint32_t gx = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(slabs, (uint64_t)ctx->num_cu / nblocks));
    const size_t dots = (size_t)nblocks * 4096, groups = dots + nprof;
    if (groups > 0x7fffffffu / gx) return set_err(KPAL_E_INVALID, "cross distance: %d x %d profiles are too many for one call", c.Q, c.R);
    CHK(ensure(ctx, ctx->partials, groups * gx * sizeof(Partial)));
    Partial *pp = (Partial *)ctx->partials.p;
    LAUNCH(ctx, "cross_gram", cross_gram_kernel, dim3(nblocks * gx), dim3(256), c, gx, blocksR, pp);
    LAUNCH(ctx, "cross_norm", cross_norm_kernel, dim3(nprof * gx), dim3(256), c, gx, pp + dots * gx);
    std::vector<Partial> res;
    CHK(finish_partials(ctx, (uint32_t)groups, gx, res));
    const double limit = 9007199254740992.0;     // 2^53
    for (uint32_t p = 0; p < nprof; ++p)
        if (!(res[dots + p].s < limit)) {
            *exact = false;
            return KPAL_OK;
        }
    for (int q = 0; q < c.Q; ++q)
        for (int r = 0; r < c.R; ++r) {
            const size_t block = (size_t)(q / 64) * blocksR + (size_t)(r / 64);
            const size_t tile = (size_t)((q % 64) / 16) * 4 + (size_t)((r % 64) / 16);
            const double dot = res[(block * 16 + tile) * 256 + (size_t)((q % 16) * 16 + (r % 16))].s;
            // exact integers below 2^53 each: the int64 expression is the reference's sum of squared differences
            const int64_t d2 = (int64_t)res[dots + q].s + (int64_t)res[dots + c.Q + r].s - 2 * (int64_t)dot;
            out[(size_t)q * c.R + r] = std::sqrt((double)d2);   // metrics.py:46: np.sqrt(np.dot(v, v))
        }
    *exact = true;
    return KPAL_OK;
}

// Tiles, slots and the grid of one pass of cross_tile_kernel / cross_super_kernel (or cross_recip_kernel) over c.
struct CrossGrid {
    int sideR, superR;
    uint32_t units;   // what the grid counts: super-tiles (staged) or 4 x 4 tiles
    uint32_t gx;      // workgroups per unit = partials per slot
    uint64_t slots;   // 16 * tiles
};
static CrossGrid cross_grid(kpal_ctx *ctx, const CrossSets &c, bool staged)
{
    const int sideQ = (c.Q + 3) / 4, sideR = (c.R + 3) / 4, superQ = (c.Q + 15) / 16, superR = (c.R + 15) / 16;
    const uint64_t ntiles = c.tri ? (uint64_t)sideQ * (sideQ + 1) / 2 : (uint64_t)sideQ * sideR;
    const uint64_t nsuper = c.tri ? (uint64_t)superQ * (superQ + 1) / 2 : (uint64_t)superQ * superR;
    uint32_t gx;
    if (staged) {
        gx = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(c.n / kSuperBins, std::max<uint64_t>(1, (uint64_t)ctx->num_cu * 8 / nsuper)));
        gx = std::max(8u, gx / 8u * 8u);   // (cross_block deals bin-groups to the 8 XCDs; n / 64 >= 64 for k >= 6)
    } else {
        gx = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((c.n + 255) / 256, std::max<uint64_t>(1, (uint64_t)ctx->num_cu * 16 / ntiles)));
    }
    return CrossGrid{sideR, superR, (uint32_t)(staged ? nsuper : ntiles), gx, ntiles * 16};
}

// cross_slot on the host: where the reduced partial of pair (i, j) lies
static size_t cross_slot_host(const CrossSets &c, int sideR, int i, int j)
{
    const size_t tile = c.tri ? (size_t)(i / 4) * (size_t)(i / 4 + 1) / 2 + (size_t)(j / 4) : (size_t)(i / 4) * sideR + (size_t)(j / 4);
    return tile * 16 + (size_t)((i % 4) * 4 + j % 4);
}

template <class Acc>
static int launch_cross(kpal_ctx *ctx, const char *name, bool staged, const CrossOpt &o, const CrossGrid &g, Partial *pp)
{
    if (staged) LAUNCH(ctx, name, (cross_super_kernel<Acc>), dim3(g.gx * g.units), dim3(256), o, g.units, g.superR, pp);
    else LAUNCH(ctx, name, (cross_tile_kernel<Acc>), dim3(g.gx * g.units), dim3(256), o, g.gx, pp);
    return KPAL_OK;
}

// Every pair of c for a plain metric: the register-tile kernel, or (staged: c.n is a multiple of 64) the LDS-staged ones --
// with `recip` the reciprocal form of 'prod' / 'sum' first, valid while every count is below 2^16 ('prod') or fits the table
// ('sum'): the kernel says whether it saw a larger one, and the pair-of-counts kernel then runs after all.  res: the reduced
// partial of pair (i, j) at tile number * 16 + (i % 4) * 4 + j % 4 (cross_kernels.hpp); the triangle's launches keep the
// names they always had.
int cross_pairs(kpal_ctx *ctx, const CrossSets &c, int metric, bool staged, bool recip, bool allreduce, std::vector<Partial> &res)
{
    const CrossGrid g = cross_grid(ctx, c, staged);
    if (g.slots > 0x7fffffffu / g.gx) return set_err(KPAL_E_INVALID, "%d x %d profiles are too many for one call", c.Q, c.R);
    CHK(ensure(ctx, ctx->partials, g.slots * g.gx * sizeof(Partial)));
    Partial *pp = (Partial *)ctx->partials.p;
    const CrossOpt o = {c, 0, nullptr, 0u, (uint32_t)g.slots};
    bool done = false;
    if (staged && recip && metric != KPAL_EUCLIDEAN) {
        CHK(ensure(ctx, ctx->scratch[3], 16));
        uint32_t *big = (uint32_t *)ctx->scratch[3].p;
        HIPCHK(hipMemsetAsync(big, 0, sizeof(uint32_t), ctx->stream));
        HIPCHK(hipMemsetAsync(pp, 0, g.slots * g.gx * sizeof(Partial), ctx->stream));   // (.s / .m of a slot come from different threads)
        const dim3 grid(g.gx * g.units);   // (gx: a multiple of 8)
        if (metric == KPAL_PAIRWISE_PROD) LAUNCH(ctx, c.tri ? "matrix_rdiff" : "cross_rdiff", (cross_recip_kernel<0>), grid, dim3(256), c, g.units, g.superR, pp, big);
        else LAUNCH(ctx, c.tri ? "matrix_rsum" : "cross_rsum", (cross_recip_kernel<1>), grid, dim3(256), c, g.units, g.superR, pp, big);
        uint32_t saw_big = 0;
        HIPCHK(hipMemcpyAsync(&saw_big, big, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        done = saw_big == 0;
    }
    if (!done) {
        const char *name = staged ? (c.tri ? "matrix_super" : "cross_super") : (c.tri ? "matrix_tile" : "cross_tile");
        if (metric == KPAL_PAIRWISE_PROD) CHK(launch_cross<PlainAcc<0>>(ctx, name, staged, o, g, pp));
        else if (metric == KPAL_PAIRWISE_SUM) CHK(launch_cross<PlainAcc<1>>(ctx, name, staged, o, g, pp));
        else CHK(launch_cross<PlainAcc<2>>(ctx, name, staged, o, g, pp));
    }
    return finish_partials(ctx, (uint32_t)g.slots, g.gx, res, allreduce);
}

static int cross_core(kpal_ctx *ctx, const CrossSets &c, int metric, double *out)
{
    // the LDS-staged kernels take 64 bins at a time (k >= 6) and pay when both sides fill more than one register tile; with
    // at most four profiles on a side the register-tile kernel already reads the long side once
    const bool staged = c.n >= 4096 && c.Q > 4 && c.R > 4;
    if (metric == KPAL_EUCLIDEAN && staged) {
        bool exact = false;
        CHK(cross_gram_euclidean(ctx, c, out, &exact));
        if (exact) return KPAL_OK;
    }
    std::vector<Partial> res;
    CHK(cross_pairs(ctx, c, metric, staged, true, false, res));
    const int sideR = (c.R + 3) / 4;
    for (int q = 0; q < c.Q; ++q)
        for (int r = 0; r < c.R; ++r) out[(size_t)q * c.R + r] = finish_value(metric, res[cross_slot_host(c, sideR, q, r)], nullptr);
    return KPAL_OK;
}

static int cross_check(int k, int Q, int R, int metric, const void *left, const void *right, const double *out)
{
    if (Q < 1 || R < 1) return set_err(KPAL_E_INVALID, "Q and R must be >= 1");
    if (k < 1 || k > KPAL_MAX_K) return set_err(KPAL_E_INVALID, "k=%d out of range", k);
    if (metric < 0 || metric > 2) return set_err(KPAL_E_INVALID, "unknown metric %d", metric);
    if (!left || !right || !out) return set_err(KPAL_E_INVALID, "NULL pointer");
    return KPAL_OK;
}

KPAL_API int kpal_cross_distance_device(kpal_ctx *ctx, int k, int Q, const int64_t *dev_left, int R, const int64_t *dev_right,
                                        int metric, int do_balance, double *out)
{
    CTX_ENTER(ctx);
    CHK(cross_check(k, Q, R, metric, dev_left, dev_right, out));
    if (((uintptr_t)dev_left & 15) || ((uintptr_t)dev_right & 15)) return set_err(KPAL_E_INVALID, "device tables must be 16-byte aligned");
    const uint64_t n = 1ULL << (2 * k);
    CrossSets c = {dev_left, dev_right, Q, R, n, 0};
    if (do_balance) {
        // balance once per profile: identical to the reference balancing copies per pair (kdistlib.py:136-141)
        CHK(ensure(ctx, ctx->scratch[2], ((size_t)Q + (size_t)R) * n * 8));
        int64_t *bl = (int64_t *)ctx->scratch[2].p, *br = bl + (uint64_t)Q * n;
        for (int q = 0; q < Q; ++q) CHK(launch_balance(ctx, k, dev_left + (uint64_t)q * n, bl + (uint64_t)q * n));
        for (int r = 0; r < R; ++r) CHK(launch_balance(ctx, k, dev_right + (uint64_t)r * n, br + (uint64_t)r * n));
        c.left = bl;
        c.right = br;
    }
    return cross_core(ctx, c, metric, out);
}

KPAL_API int kpal_cross_distance(kpal_ctx *ctx, int k, int Q, const int64_t *const *host_left, int R,
                                 const int64_t *const *host_right, int metric, int do_balance, double *out)
{
    CTX_ENTER(ctx);
    CHK(cross_check(k, Q, R, metric, host_left, host_right, out));
    const uint64_t n = 1ULL << (2 * k);
    CHK(ensure(ctx, ctx->scratch[0], ((size_t)Q + (size_t)R) * n * 8));
    int64_t *dl = (int64_t *)ctx->scratch[0].p, *dr = dl + (uint64_t)Q * n;
    for (int p = 0; p < Q + R; ++p) {
        const int64_t *src = p < Q ? host_left[p] : host_right[p - Q];
        if (!src) return set_err(KPAL_E_INVALID, "%s profile %d is NULL", p < Q ? "left" : "right", p < Q ? p : p - Q);
        HIPCHK(hipMemcpyAsync(dl + (uint64_t)p * n, src, n * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    return kpal_cross_distance_device(ctx, k, Q, dl, R, dr, metric, do_balance, out);
}

// ----------------------------------------------------------------------------------------------
// ProfileDistance with options over a rectangle / a lower triangle (cross_option_kernels.hpp)
// ----------------------------------------------------------------------------------------------
static bool plain_options(const kpal_distance_options *opt)
{
    return !opt->do_positive && !opt->do_smooth && !opt->do_scale && opt->metric <= KPAL_EUCLIDEAN;
}

template <int MODE>
static int launch_cross_option_metric(kpal_ctx *ctx, const char *name, bool staged, bool scaled, bool positive, const CrossOpt &o,
                                      const CrossGrid &g, Partial *pp)
{
    if (scaled) return positive ? launch_cross<OptAcc<MODE, true, true>>(ctx, name, staged, o, g, pp)
                                : launch_cross<OptAcc<MODE, true, false>>(ctx, name, staged, o, g, pp);
    if (positive) return launch_cross<OptAcc<MODE, false, true>>(ctx, name, staged, o, g, pp);
    if constexpr (MODE == KPAL_COSINE) return launch_cross<OptAcc<MODE, false, false>>(ctx, name, staged, o, g, pp);
    return set_err(KPAL_E_STATE, "plain options belong to the plain rectangle");   // (delegated by the callers)
}

// Every pair of c (c.tri: pairs below the diagonal only) for a batched option set -- no smoothing, not plain -- from tables
// that are already balanced.  out: Q x R row-major, or the lower triangle in distance_matrix order.
static int cross_option_core(kpal_ctx *ctx, const CrossSets &c, const kpal_distance_options *opt, double *out)
{
    const bool scaled = opt->do_scale != 0, positive = opt->do_positive != 0, tri = c.tri != 0;
    const bool staged = c.n >= 4096 && c.Q > 4 && c.R > 4;   // (cross_core's rule)
    const CrossGrid g = cross_grid(ctx, c, staged);
    const uint64_t slots = g.slots;
    const uint32_t gx = g.gx;
    const uint32_t nacc = opt->metric == KPAL_COSINE ? 3 : 1, nacc_max = std::max(nacc, scaled && positive ? 2u : 1u);
    if (slots * nacc_max > 0x7fffffffu / gx) return set_err(KPAL_E_INVALID, "cross distance: %d x %d profiles are too many for one call", c.Q, c.R);
    const uint32_t nprof = tri ? (uint32_t)c.Q : (uint32_t)c.Q + (uint32_t)c.R;
    const uint32_t gxt = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((c.n + 255) / 256, std::max<uint64_t>(1, (uint64_t)ctx->num_cu * 8 / nprof)));
    CHK(ensure(ctx, ctx->partials, std::max<size_t>((size_t)slots * nacc_max * gx, (size_t)nprof * gxt) * sizeof(Partial)));
    CHK(ensure(ctx, ctx->scratch[3], std::max<size_t>((size_t)slots * 2, nprof) * sizeof(Partial)));
    Partial *pp = (Partial *)ctx->partials.p, *totals = (Partial *)ctx->scratch[3].p;
    const CrossOpt o = {c, opt->down ? 1 : 0, totals, tri ? 0u : (uint32_t)c.Q, (uint32_t)slots};
    if (scaled && !positive) {
        // np.sum of every (balanced) profile once; the pairs' factors are derived from them inside the rectangle kernel
        LAUNCH(ctx, "cross_option_totals", cross_option_totals_kernel, dim3(nprof * gxt), dim3(256), c, gxt, pp);
        CHK(reduce_partials(ctx, pp, nprof, gxt, totals));
    } else if (scaled) {
        // after positive the totals depend on the partner: a first rectangle pass for the two masked totals of every pair
        CHK((launch_cross<OptAcc<kOptTotals, false, true>>(ctx, staged ? "cross_option_masked_super" : "cross_option_masked_tile", staged, o, g, pp)));
        CHK(reduce_partials(ctx, pp, (uint32_t)slots * 2, gx, totals));
    }
    const char *name = staged ? "cross_option_super" : "cross_option_tile";
    switch (opt->metric) {
    case KPAL_PAIRWISE_PROD: CHK(launch_cross_option_metric<0>(ctx, name, staged, scaled, positive, o, g, pp)); break;
    case KPAL_PAIRWISE_SUM: CHK(launch_cross_option_metric<1>(ctx, name, staged, scaled, positive, o, g, pp)); break;
    case KPAL_EUCLIDEAN: CHK(launch_cross_option_metric<2>(ctx, name, staged, scaled, positive, o, g, pp)); break;
    default: CHK(launch_cross_option_metric<3>(ctx, name, staged, scaled, positive, o, g, pp)); break;
    }
    std::vector<Partial> res;
    CHK(finish_partials(ctx, (uint32_t)(slots * nacc), gx, res));
    auto value = [&](int i, int j) -> double {
        const size_t slot = cross_slot_host(c, g.sideR, i, j);
        const Partial &p0 = res[slot];
        if (opt->metric <= KPAL_PAIRWISE_SUM) return p0.s / (double)(p0.m + 1ULL);   // metrics.py:123
        if (opt->metric == KPAL_EUCLIDEAN) return scaled ? std::sqrt(p0.s) : std::sqrt((double)(int64_t)p0.m);   // metrics.py:135,46
        const Partial &p1 = res[slots + slot], &p2 = res[2 * slots + slot];          // metrics.py:147: dot(l, r) / (|l| * |r|)
        if (scaled) return p0.s / (std::sqrt(p1.s) * std::sqrt(p2.s));
        return (double)(int64_t)p0.m / (std::sqrt((double)(int64_t)p1.m) * std::sqrt((double)(int64_t)p2.m));
    };
    if (tri) {
        for (int i = 1; i < c.Q; ++i)
            for (int j = 0; j < i; ++j) out[(size_t)i * (i - 1) / 2 + j] = value(i, j);
    } else {
        for (int q = 0; q < c.Q; ++q)
            for (int r = 0; r < c.R; ++r) out[(size_t)q * c.R + r] = value(q, r);
    }
    return KPAL_OK;
}

// Balanced copies of `count` consecutive tables at `dst` (one launch_balance per profile, as kpal_cross_distance_device).
static int balance_set(kpal_ctx *ctx, int k, int count, const int64_t *src, int64_t *dst)
{
    const uint64_t n = 1ULL << (2 * k);
    for (int p = 0; p < count; ++p) CHK(launch_balance(ctx, k, src + (uint64_t)p * n, dst + (uint64_t)p * n));
    return KPAL_OK;
}

KPAL_API int kpal_cross_profile_distance_device(kpal_ctx *ctx, int k, int Q, const int64_t *dev_left, int R, const int64_t *dev_right,
                                                const kpal_distance_options *opt, double *out)
{
    CTX_ENTER(ctx);
    CHK(check_options(opt));
    if (plain_options(opt)) return kpal_cross_distance_device(ctx, k, Q, dev_left, R, dev_right, opt->metric, opt->do_balance, out);
    CHK(cross_check(k, Q, R, 0, dev_left, dev_right, out));
    if (((uintptr_t)dev_left & 15) || ((uintptr_t)dev_right & 15)) return set_err(KPAL_E_INVALID, "device tables must be 16-byte aligned");
    const uint64_t n = 1ULL << (2 * k);
    CrossSets c = {dev_left, dev_right, Q, R, n, 0};
    if (opt->do_balance) {
        // balance once per profile: identical to the reference balancing copies per pair (kdistlib.py:136-141)
        CHK(ensure(ctx, ctx->scratch[2], ((size_t)Q + (size_t)R) * n * 8));
        int64_t *bl = (int64_t *)ctx->scratch[2].p, *br = bl + (uint64_t)Q * n;
        CHK(balance_set(ctx, k, Q, dev_left, bl));
        CHK(balance_set(ctx, k, R, dev_right, br));
        c.left = bl;
        c.right = br;
    }
    if (opt->do_smooth) {
        // smoothed tables exist per pair only (a node collapses by both partners' counts): the pair pipeline on the balanced tables
        for (int q = 0; q < Q; ++q)
            for (int r = 0; r < R; ++r)
                CHK(profile_distance_pair(ctx, k, c.left + (uint64_t)q * n, c.right + (uint64_t)r * n, opt, true, &out[(size_t)q * R + r]));
        return KPAL_OK;
    }
    return cross_option_core(ctx, c, opt, out);
}

KPAL_API int kpal_cross_profile_distance(kpal_ctx *ctx, int k, int Q, const int64_t *const *host_left, int R,
                                         const int64_t *const *host_right, const kpal_distance_options *opt, double *out)
{
    CTX_ENTER(ctx);
    CHK(check_options(opt));
    CHK(cross_check(k, Q, R, 0, host_left, host_right, out));
    const uint64_t n = 1ULL << (2 * k);
    CHK(ensure(ctx, ctx->scratch[0], ((size_t)Q + (size_t)R) * n * 8));
    int64_t *dl = (int64_t *)ctx->scratch[0].p, *dr = dl + (uint64_t)Q * n;
    for (int p = 0; p < Q + R; ++p) {
        const int64_t *src = p < Q ? host_left[p] : host_right[p - Q];
        if (!src) return set_err(KPAL_E_INVALID, "%s profile %d is NULL", p < Q ? "left" : "right", p < Q ? p : p - Q);
        HIPCHK(hipMemcpyAsync(dl + (uint64_t)p * n, src, n * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    return kpal_cross_profile_distance_device(ctx, k, Q, dl, R, dr, opt, out);
}

KPAL_API int kpal_profile_distance_matrix_device(kpal_ctx *ctx, int P, int k, const int64_t *dev_profiles,
                                                 const kpal_distance_options *opt, double *out_lower)
{
    CTX_ENTER(ctx);
    if (P < 1) return set_err(KPAL_E_INVALID, "P must be >= 1");
    if (k < 1 || k > KPAL_MAX_K) return set_err(KPAL_E_INVALID, "k=%d out of range", k);
    CHK(check_options(opt));
    if (P == 1) return KPAL_OK;
    if (!dev_profiles || !out_lower) return set_err(KPAL_E_INVALID, "NULL pointer");
    if (plain_options(opt)) return kpal_distance_matrix_device(ctx, P, k, dev_profiles, opt->metric, opt->do_balance, out_lower);
    if ((uintptr_t)dev_profiles & 15) return set_err(KPAL_E_INVALID, "device tables must be 16-byte aligned");
    const uint64_t n = 1ULL << (2 * k);
    const int64_t *prof = dev_profiles;
    if (opt->do_balance) {
        CHK(ensure(ctx, ctx->scratch[2], (size_t)P * n * 8));
        CHK(balance_set(ctx, k, P, dev_profiles, (int64_t *)ctx->scratch[2].p));
        prof = (const int64_t *)ctx->scratch[2].p;
    }
    if (opt->do_smooth) {
        for (int i = 1; i < P; ++i)
            for (int j = 0; j < i; ++j)
                CHK(profile_distance_pair(ctx, k, prof + (uint64_t)i * n, prof + (uint64_t)j * n, opt, true, &out_lower[(size_t)i * (i - 1) / 2 + j]));
        return KPAL_OK;
    }
    const CrossSets c = {prof, prof, P, P, n, 1};
    return cross_option_core(ctx, c, opt, out_lower);
}
