// kpal_cross.hip -- everything of the C-ABI that works on SETS of profiles: the lower triangle of one set
// (kpal_distance_matrix[_device], kdistlib.distance_matrix) and the Q x R rectangle between a left and a right set in separate
// allocations (kpal_cross_distance[_device]), plain and -- kpal_profile_distance_matrix[_device],
// kpal_cross_profile_distance[_device] -- for a ProfileDistance with options.  What is decided before a launch (which kernels,
// the grids, where a pair's partial lies) is matrix_plan.hpp.
//   plain: one call is a fixed number of launches whatever P, Q and R are -- the balance of each profile (do_balance), one
// kernel over all pairs (cross_kernels.hpp: the triangle is the set crossed with itself; two kernels when a fast form gives up
// on the values; matrix_all_kernels.hpp for a multiset triangle of 17..64 profiles; the fp64 Gram matrix on the matrix cores
// for euclidean), one fixed-order reduction of the per-workgroup partials.
//   with options (cross_option_kernels.hpp): a totals pass or a masked-totals rectangle pass more when the profiles are scaled;
// dynamic smoothing in those entries is one pair pipeline (kpal_pair.hip) per pair, on tables balanced once.
//   dynamic smoothing over whole sets (kpal_cross_smooth_distance_device, kpal_smooth_distance_matrix_device; smooth_plan.hpp,
// smooth_set_kernels.hpp): one pyramid of node sums and codes per profile (k + 1 launches for all of them), then two passes of
// the rectangle kernels, over the bins and over the pyramids, and one reduction.  The pyramids (smooth_set_pyramids) also serve
// the linked pairs of kpal_paired_smooth.hip; the launch functions of the cores serve the tiles of kpal_nearest.hip.
#include "kpal_host.hpp"
#include "dist_host.hpp"

#include "cross_kernels.hpp"
#include "cross_option_kernels.hpp"
#include "matrix_all_kernels.hpp"
#include "smooth_set_kernels.hpp"

static const MatrixSwitches &matrix_switches()
{
    static const MatrixSwitches sw = [] {
        auto on = [](const char *name) { const char *e = getenv(name); return !e || atoi(e) != 0; };
        return MatrixSwitches{on("KPAL_MATRIX_MFMA"), on("KPAL_MATRIX_SUPER"), on("KPAL_MATRIX_ALL"), on("KPAL_MATRIX_RDIFF")};
    }();
    return sw;
}

// `count` host profiles of n bins, one behind the other at dst; what: "profile", "left profile", "right profile".
static int upload_set(kpal_ctx *ctx, int64_t *dst, int count, uint64_t n, const int64_t *const *host, const char *what)
{
    for (int p = 0; p < count; ++p) {
        if (!host[p]) return set_err(KPAL_E_INVALID, "%s %d is NULL", what, p);
        HIPCHK(hipMemcpyAsync(dst + (uint64_t)p * n, host[p], n * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    return KPAL_OK;
}

// The left and the right set of a rectangle, one behind the other in scratch[kScratchUpload].
int upload_rectangle(kpal_ctx *ctx, uint64_t n, int Q, const int64_t *const *host_left, int R, const int64_t *const *host_right,
                     int64_t **dl, int64_t **dr)
{
    CHK(ensure(ctx, ctx->scratch[kScratchUpload], ((size_t)Q + (size_t)R) * n * 8));
    *dl = (int64_t *)ctx->scratch[kScratchUpload].p;
    *dr = *dl + (uint64_t)Q * n;
    CHK(upload_set(ctx, *dl, Q, n, host_left, "left profile"));
    return upload_set(ctx, *dr, R, n, host_right, "right profile");
}

// Balanced copies of `count` consecutive tables at `dst` (one launch_balance per profile).
int balance_set(kpal_ctx *ctx, int k, int count, const int64_t *src, int64_t *dst)
{
    const uint64_t n = 1ULL << (2 * k);
    for (int p = 0; p < count; ++p) CHK(launch_balance(ctx, k, src + (uint64_t)p * n, dst + (uint64_t)p * n));
    return KPAL_OK;
}

// Balanced copies of the sets of c (a triangle: of its one set) in scratch[kScratchBalanced]; c names them from here on.  Balanced once per
// profile: identical to the reference balancing copies per pair (kdistlib.py:136-141).
static int balance_sets(kpal_ctx *ctx, int k, CrossSets &c)
{
    CHK(ensure(ctx, ctx->scratch[kScratchBalanced], ((size_t)c.Q + (c.tri ? 0 : (size_t)c.R)) * c.n * 8));
    int64_t *bl = (int64_t *)ctx->scratch[kScratchBalanced].p, *br = c.tri ? bl : bl + (uint64_t)c.Q * c.n;
    CHK(balance_set(ctx, k, c.Q, c.left, bl));
    if (!c.tri) CHK(balance_set(ctx, k, c.R, c.right, br));
    c.left = bl;
    c.right = br;
    return KPAL_OK;
}

// A reciprocal form (cross_recip_kernel, matrix_r*_all_kernel) over the `count` cleared partials at pp: `launch` runs it, and
// *done says whether it saw no count it is not valid for -- the word `big`, of which big_bytes are cleared before, stayed 0.
template <class Launch>
static int try_recip(kpal_ctx *ctx, uint32_t *big, size_t big_bytes, Partial *pp, size_t count, Launch launch, bool *done)
{
    HIPCHK(hipMemsetAsync(big, 0, big_bytes, ctx->stream));
    HIPCHK(hipMemsetAsync(pp, 0, count * sizeof(Partial), ctx->stream));   // (.s / .m of a slot come from different threads)
    CHK(launch());
    uint32_t saw_big = 0;
    HIPCHK(hipMemcpyAsync(&saw_big, big, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *done = saw_big == 0;
    return KPAL_OK;
}

// ----------------------------------------------------------------------------------------------
// plain metrics
// ----------------------------------------------------------------------------------------------
// Euclidean distances of all pairs of a triangle from the fp64 Gram matrix (gram_kernels.hpp).  *exact = false (and
// out_lower untouched) when some |x|^2 >= 2^53: the caller then takes the wrapping-int64 path.
static int gram_euclidean(kpal_ctx *ctx, int P, uint64_t n, const int64_t *prof, double *out_lower, bool *exact, bool allreduce)
{
    static_assert(sizeof(GramBlock) == sizeof(int2), "gram_mfma_kernel reads the block list as int2");
    const GramPlan g = gram_plan(ctx->num_cu, P, n);
    const uint32_t nd = g.nd, no = g.no;
    CHK(ensure(ctx, ctx->scratch[kScratchTotals], g.blocks.size() * sizeof(GramBlock)));
    HIPCHK(hipMemcpyAsync(ctx->scratch[kScratchTotals].p, g.blocks.data(), g.blocks.size() * sizeof(GramBlock), hipMemcpyHostToDevice, ctx->stream));
    const size_t part_d = (size_t)nd * 4096 * g.gx_d, part_o = (size_t)no * 4096 * g.gx_o;
    CHK(ensure(ctx, ctx->partials, (part_d + part_o) * sizeof(Partial)));
    CHK(ensure(ctx, ctx->result, (size_t)(nd + no) * 4096 * sizeof(Partial)));
    Partial *pp = (Partial *)ctx->partials.p;
    Partial *res_d = (Partial *)ctx->result.p;
    const int2 *dt = (const int2 *)ctx->scratch[kScratchTotals].p;
    // a diagonal block writes only its 10 tiles with gj <= gi; the reduction below runs over all 16: the other six read zeros
    HIPCHK(hipMemsetAsync(pp, 0, part_d * sizeof(Partial), ctx->stream));
    LAUNCH(ctx, "gram_mfma", (gram_mfma_kernel<true>), dim3(g.gx_d, nd), dim3(256), prof, P, n, dt, pp);
    CHK(reduce_partials(ctx, pp, nd * 4096, g.gx_d, res_d));
    if (no) {
        LAUNCH(ctx, "gram_mfma", (gram_mfma_kernel<false>), dim3(g.gx_o, no), dim3(256), prof, P, n, dt + nd, pp + part_d);
        CHK(reduce_partials(ctx, pp + part_d, no * 4096, g.gx_o, res_d + (size_t)nd * 4096));
    }
    if (allreduce) CHK(comm_allreduce_partials(ctx, res_d, (size_t)(nd + no) * 4096));   // (sums of exact integers: exact in any order below 2^53)
    std::vector<Partial> res((size_t)(nd + no) * 4096);
    HIPCHK(hipMemcpyAsync(res.data(), res_d, res.size() * sizeof(Partial), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // also: `g.blocks` was read by the asynchronous copy above
    std::vector<double> norm(P);
    for (int i = 0; i < P; ++i) {
        norm[i] = res[gram_index(g, i, i)].s;
        if (!gram_exact(norm[i])) {
            *exact = false;
            return KPAL_OK;
        }
    }
    for (int i = 1; i < P; ++i)
        for (int j = 0; j < i; ++j) out_lower[triangle_index(i, j)] = gram_distance(norm[i], norm[j], res[gram_index(g, i, j)].s, exact);
    *exact = true;
    return KPAL_OK;
}

// The fp64 dot products of cross_gram_kernel and the norms of cross_norm_kernel of a rectangle, as workgroup partials in
// ctx->partials: lay->groups groups of lay->gx, the dots at cross_gram_index, the Q + R norms behind them.
int cross_gram_launch(kpal_ctx *ctx, const CrossSets &c, CrossGramLayout *lay)
{
    const int blocksQ = (c.Q + 63) / 64, blocksR = (c.R + 63) / 64;
    const uint32_t nblocks = (uint32_t)blocksQ * (uint32_t)blocksR, nprof = (uint32_t)c.Q + (uint32_t)c.R;
    const uint32_t gx = cross_gram_gx(ctx->num_cu, nblocks, c.n);
    const size_t dots = (size_t)nblocks * 4096, groups = dots + nprof;
    if (partials_too_many(groups, gx)) return set_err(KPAL_E_INVALID, "cross distance: %d x %d profiles are too many for one call", c.Q, c.R);
    CHK(ensure(ctx, ctx->partials, groups * gx * sizeof(Partial)));
    Partial *pp = (Partial *)ctx->partials.p;
    LAUNCH(ctx, "cross_gram", cross_gram_kernel, dim3(nblocks * gx), dim3(256), c, gx, blocksR, pp);
    LAUNCH(ctx, "cross_norm", cross_norm_kernel, dim3(nprof * gx), dim3(256), c, gx, pp + dots * gx);
    *lay = CrossGramLayout{blocksR, gx, dots, groups};
    return KPAL_OK;
}

// ... of a rectangle, from those dot products and norms: the same rule.
static int cross_gram_euclidean(kpal_ctx *ctx, const CrossSets &c, double *out, bool *exact)
{
    CrossGramLayout lay;
    CHK(cross_gram_launch(ctx, c, &lay));
    const int blocksR = lay.blocksR;
    const uint32_t nprof = (uint32_t)c.Q + (uint32_t)c.R;
    const size_t dots = lay.dots;
    std::vector<Partial> res;
    CHK(finish_partials(ctx, (uint32_t)lay.groups, lay.gx, res));
    for (uint32_t p = 0; p < nprof; ++p)
        if (!gram_exact(res[dots + p].s)) {
            *exact = false;
            return KPAL_OK;
        }
    for (int q = 0; q < c.Q; ++q)
        for (int r = 0; r < c.R; ++r)
            out[(size_t)q * c.R + r] = gram_distance(res[dots + q].s, res[dots + c.Q + r].s, res[cross_gram_index(blocksR, q, r)].s, exact);
    *exact = true;
    return KPAL_OK;
}

template <class Acc>
static int launch_cross(kpal_ctx *ctx, const char *name, bool staged, const typename Acc::Opt &o, const CrossGrid &g, Partial *pp)
{
    if (staged) LAUNCH(ctx, name, (cross_super_kernel<Acc>), dim3(g.gx * g.units), dim3(256), o, g.units, g.superR, pp);
    else LAUNCH(ctx, name, (cross_tile_kernel<Acc>), dim3(g.gx * g.units), dim3(256), o, g.gx, pp);
    return KPAL_OK;
}

// Every pair of c for a plain metric: the register-tile kernel, or (staged: c.n is a multiple of 64) the LDS-staged ones --
// with `recip` the reciprocal form of 'prod' / 'sum' first, valid while every count is below 2^16 ('prod') or fits the table
// ('sum'): the kernel says whether it saw a larger one, and the pair-of-counts kernel then runs after all.  res: the reduced
// partial of pair (i, j) at cross_slot(i, j); the triangle's launches keep the names they always had.  cross_pairs_launch:
// the kernels alone -- the workgroup partials lie in ctx->partials, g->slots groups of g->gx.
int cross_pairs_launch(kpal_ctx *ctx, const CrossSets &c, int metric, bool staged, bool recip, CrossGrid *grid)
{
    const CrossGrid g = *grid = cross_grid(ctx->num_cu, c, staged);
    if (partials_too_many(g.slots, g.gx)) return set_err(KPAL_E_INVALID, "%d x %d profiles are too many for one call", c.Q, c.R);
    CHK(ensure(ctx, ctx->partials, g.slots * g.gx * sizeof(Partial)));
    Partial *pp = (Partial *)ctx->partials.p;
    const CrossOpt o = {c, 0, nullptr, 0u, (uint32_t)g.slots};
    bool done = false;
    if (staged && recip && metric != KPAL_EUCLIDEAN) {
        CHK(ensure(ctx, ctx->scratch[kScratchTotals], 16));
        uint32_t *big = (uint32_t *)ctx->scratch[kScratchTotals].p;
        CHK(try_recip(ctx, big, sizeof(uint32_t), pp, g.slots * g.gx, [&]() -> int {
            const dim3 grid(g.gx * g.units);   // (gx: a multiple of 8)
            if (metric == KPAL_PAIRWISE_PROD) LAUNCH(ctx, c.tri ? "matrix_rdiff" : "cross_rdiff", (cross_recip_kernel<0>), grid, dim3(256), c, g.units, g.superR, pp, big);
            else LAUNCH(ctx, c.tri ? "matrix_rsum" : "cross_rsum", (cross_recip_kernel<1>), grid, dim3(256), c, g.units, g.superR, pp, big);
            return KPAL_OK;
        }, &done));
    }
    if (!done) {
        const char *name = staged ? (c.tri ? "matrix_super" : "cross_super") : (c.tri ? "matrix_tile" : "cross_tile");
        CHK(with_metric<KPAL_EUCLIDEAN>(metric, [&](auto m) { return launch_cross<PlainAcc<m>>(ctx, name, staged, o, g, pp); }));
    }
    return KPAL_OK;
}

static int cross_pairs(kpal_ctx *ctx, const CrossSets &c, int metric, bool staged, bool recip, bool allreduce, std::vector<Partial> &res)
{
    CrossGrid g;
    CHK(cross_pairs_launch(ctx, c, metric, staged, recip, &g));
    return finish_partials(ctx, (uint32_t)g.slots, g.gx, res, allreduce);
}

// The lower triangle over n bins per profile (profile p at prof + p * n).  allreduce: this rank holds a bin RANGE of every
// profile -- the per-pair sums / term counts / dot products of all ranks are added (one all-reduce) before they are finished;
// the ranks agreed on `tiled_agreed` (kpal_comm_distance_matrix_device): the Gram path and the others all-reduce different things.
int distance_matrix_core(kpal_ctx *ctx, int P, uint64_t n, const int64_t *prof, int metric, double *out_lower, bool allreduce, int tiled_agreed)
{
    const MatrixRoute route = matrix_route(P, n, metric, tiled_agreed, matrix_switches());
    if (route.gram) {
        bool exact = false;
        CHK(gram_euclidean(ctx, P, n, prof, out_lower, &exact, allreduce));
        if (exact) return KPAL_OK;
    }
    const CrossSets c = {prof, prof, P, P, n, 1};   // the triangle is the set crossed with itself
    const size_t slots = (size_t)cross_grid(ctx->num_cu, c, false).slots;   // (the *_all kernels write the slots of cross_kernels.hpp)
    unsigned gx = 0;
    bool all_done = false;
    if (route.all) {
        const bool wide = route.all_wide;
        gx = matrix_all_gx(ctx->num_cu, n, wide);
        CHK(ensure(ctx, ctx->scratch[kScratchTotals], 32));
        CHK(ensure(ctx, ctx->partials, slots * gx * sizeof(Partial)));
        Partial *pp = (Partial *)ctx->partials.p;
        uint32_t *big = (uint32_t *)ctx->scratch[kScratchTotals].p;
        CHK(try_recip(ctx, big, 32, pp, slots * gx, [&]() -> int {
            if (metric == 0) {
                if (wide) LAUNCH(ctx, "matrix_rdiff_all", (matrix_rdiff_all_kernel<16, kMatrixAllBins, kMatrixAllUnits>), dim3(gx), dim3(1024 / kMatrixAllUnits), prof, P, n, pp, big);
                else LAUNCH(ctx, "matrix_rdiff_all", (matrix_rdiff_all_kernel<8, 64, 1>), dim3(gx), dim3(256), prof, P, n, pp, big);
            } else {
                if (wide) LAUNCH(ctx, "matrix_rsum_all", (matrix_rsum_all_kernel<16, 64>), dim3(gx), dim3(1024), prof, P, n, pp, big);
                else LAUNCH(ctx, "matrix_rsum_all", (matrix_rsum_all_kernel<8, 64>), dim3(gx), dim3(256), prof, P, n, pp, big);
            }
            return KPAL_OK;
        }, &all_done));
#if defined(KPAL_MALL_CLOCK)
        {
            unsigned long long clk[4] = {0, 0, 0, 0};
            HIPCHK(hipMemcpy(clk, big, sizeof(clk), hipMemcpyDeviceToHost));
            fprintf(stderr, "matrix_all: %llu shader cycles in %.1f us = %.0f MHz\n", clk[1], (double)clk[2] / 100.0, 100.0 * (double)clk[1] / (double)clk[2]);
        }
#endif
    }
    std::vector<Partial> res;
    if (all_done) CHK(finish_partials(ctx, (uint32_t)slots, gx, res, allreduce));
    else CHK(cross_pairs(ctx, c, metric, route.staged, route.recip, allreduce, res));
    fill_pairs(c, 0, out_lower, [&](uint64_t slot) { return finish_value(metric, res[slot], nullptr); });   // (a triangle's slots know no side)
    return KPAL_OK;
}

static int cross_core(kpal_ctx *ctx, const CrossSets &c, int metric, double *out)
{
    const bool staged = cross_staged(c.Q, c.R, c.n);
    if (metric == KPAL_EUCLIDEAN && staged) {
        bool exact = false;
        CHK(cross_gram_euclidean(ctx, c, out, &exact));
        if (exact) return KPAL_OK;
    }
    std::vector<Partial> res;
    CHK(cross_pairs(ctx, c, metric, staged, true, false, res));
    fill_pairs(c, (c.R + 3) / 4, out, [&](uint64_t slot) { return finish_value(metric, res[slot], nullptr); });
    return KPAL_OK;
}

KPAL_API int kpal_distance_matrix_device(kpal_ctx *ctx, int P, int k, const int64_t *dev_profiles, int metric,
                                         int do_balance, double *out_lower)
{
    CTX_ENTER(ctx);
    if (P < 1) return set_err(KPAL_E_INVALID, "P must be >= 1");
    if (k < 1 || k > KPAL_MAX_K) return set_err(KPAL_E_INVALID, "k=%d out of range", k);
    if (metric < 0 || metric > 2) return set_err(KPAL_E_INVALID, "unknown metric %d", metric);
    if (P == 1) return KPAL_OK;
    if (!dev_profiles || !out_lower) return set_err(KPAL_E_INVALID, "NULL pointer");
    const uint64_t n = 1ULL << (2 * k);
    CrossSets c = {dev_profiles, dev_profiles, P, P, n, 1};
    if (do_balance) CHK(balance_sets(ctx, k, c));
    return distance_matrix_core(ctx, P, n, c.left, metric, out_lower, false);
}

KPAL_API int kpal_distance_matrix(kpal_ctx *ctx, int P, int k, const int64_t *const *host_profiles, int metric,
                                  int do_balance, double *out_lower)
{
    CTX_ENTER(ctx);
    if (P < 1) return set_err(KPAL_E_INVALID, "P must be >= 1");
    if (k < 1 || k > KPAL_MAX_K) return set_err(KPAL_E_INVALID, "k=%d out of range", k);
    if (P == 1) return KPAL_OK;
    if (!host_profiles || !out_lower) return set_err(KPAL_E_INVALID, "NULL pointer");
    const uint64_t n = 1ULL << (2 * k);
    CHK(ensure(ctx, ctx->scratch[kScratchUpload], (size_t)P * n * 8));
    int64_t *prof = (int64_t *)ctx->scratch[kScratchUpload].p;
    CHK(upload_set(ctx, prof, P, n, host_profiles, "profile"));
    return kpal_distance_matrix_device(ctx, P, k, prof, metric, do_balance, out_lower);
}

KPAL_API int kpal_cross_distance_device(kpal_ctx *ctx, int k, int Q, const int64_t *dev_left, int R, const int64_t *dev_right,
                                        int metric, int do_balance, double *out)
{
    CTX_ENTER(ctx);
    CHK(cross_check(k, Q, R, metric, dev_left, dev_right, out));
    CHK(tables_aligned(dev_left, dev_right));
    CrossSets c = {dev_left, dev_right, Q, R, 1ULL << (2 * k), 0};
    if (do_balance) CHK(balance_sets(ctx, k, c));
    return cross_core(ctx, c, metric, out);
}

KPAL_API int kpal_cross_distance(kpal_ctx *ctx, int k, int Q, const int64_t *const *host_left, int R,
                                 const int64_t *const *host_right, int metric, int do_balance, double *out)
{
    CTX_ENTER(ctx);
    CHK(cross_check(k, Q, R, metric, host_left, host_right, out));
    int64_t *dl = nullptr, *dr = nullptr;
    CHK(upload_rectangle(ctx, 1ULL << (2 * k), Q, host_left, R, host_right, &dl, &dr));
    return kpal_cross_distance_device(ctx, k, Q, dl, R, dr, metric, do_balance, out);
}

// ----------------------------------------------------------------------------------------------
// ProfileDistance with options over a rectangle / a lower triangle (cross_option_kernels.hpp)
// ----------------------------------------------------------------------------------------------
// Every pair of c (c.tri: pairs below the diagonal only) for a batched option set -- no smoothing, not plain -- from tables
// that are already balanced.  cross_option_launch: the kernels alone -- the workgroup partials of the option_nacc(metric)
// accumulators lie in ctx->partials, accumulator a of a pair at a * g->slots + its slot, g->gx of each.
int cross_option_launch(kpal_ctx *ctx, const CrossSets &c, const kpal_distance_options *opt, CrossGrid *grid)
{
    const bool scaled = opt->do_scale != 0, positive = opt->do_positive != 0, tri = c.tri != 0;
    const bool staged = cross_staged(c.Q, c.R, c.n);
    const CrossGrid g = *grid = cross_grid(ctx->num_cu, c, staged);
    const uint64_t slots = g.slots;
    const uint32_t gx = g.gx;
    const uint32_t nacc_max = option_nacc_max(opt->metric, scaled, positive);
    if (partials_too_many(slots * nacc_max, gx)) return set_err(KPAL_E_INVALID, "cross distance: %d x %d profiles are too many for one call", c.Q, c.R);
    const uint32_t nprof = tri ? (uint32_t)c.Q : (uint32_t)c.Q + (uint32_t)c.R;
    const uint32_t gxt = option_totals_gx(ctx->num_cu, nprof, c.n);
    CHK(ensure(ctx, ctx->partials, std::max<size_t>((size_t)slots * nacc_max * gx, (size_t)nprof * gxt) * sizeof(Partial)));
    CHK(ensure(ctx, ctx->scratch[kScratchTotals], std::max<size_t>((size_t)slots * 2, nprof) * sizeof(Partial)));
    Partial *pp = (Partial *)ctx->partials.p, *totals = (Partial *)ctx->scratch[kScratchTotals].p;
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
    return with_metric(opt->metric, [&](auto m, auto s, auto p) -> int {
        // unscaled, not positive: the cosine alone is an option set (the callers delegate the others)
        if constexpr (!s && !p && m != KPAL_COSINE) return set_err(KPAL_E_STATE, "plain options belong to the plain rectangle");
        else return launch_cross<OptAcc<m, s, p>>(ctx, name, staged, o, g, pp);
    }, scaled, positive);
}

// out: Q x R row-major, or the lower triangle in distance_matrix order.
static int cross_option_core(kpal_ctx *ctx, const CrossSets &c, const kpal_distance_options *opt, double *out)
{
    const bool scaled = opt->do_scale != 0;
    CrossGrid g;
    CHK(cross_option_launch(ctx, c, opt, &g));
    const uint64_t slots = g.slots;
    const uint32_t nacc = option_nacc(opt->metric);
    std::vector<Partial> res;
    CHK(finish_partials(ctx, (uint32_t)(slots * nacc), g.gx, res));
    fill_pairs(c, g.sideR, out, [&](uint64_t slot) { return option_value(opt->metric, scaled, res.data(), nacc, slots, slot); });
    return KPAL_OK;
}

KPAL_API int kpal_cross_profile_distance_device(kpal_ctx *ctx, int k, int Q, const int64_t *dev_left, int R, const int64_t *dev_right,
                                                const kpal_distance_options *opt, double *out)
{
    CTX_ENTER(ctx);
    CHK(check_options(opt));
    if (options_plain(opt)) return kpal_cross_distance_device(ctx, k, Q, dev_left, R, dev_right, opt->metric, opt->do_balance, out);
    CHK(cross_check(k, Q, R, 0, dev_left, dev_right, out));
    CHK(tables_aligned(dev_left, dev_right));
    const uint64_t n = 1ULL << (2 * k);
    CrossSets c = {dev_left, dev_right, Q, R, n, 0};
    if (opt->do_balance) CHK(balance_sets(ctx, k, c));
    if (opt->do_smooth) {
        // this entry materialises the smoothed tables of every pair: the pair pipeline on the balanced tables
        // (kpal_cross_smooth_distance_device runs the rectangle from per-profile pyramids instead)
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
    int64_t *dl = nullptr, *dr = nullptr;
    CHK(upload_rectangle(ctx, 1ULL << (2 * k), Q, host_left, R, host_right, &dl, &dr));
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
    if (options_plain(opt)) return kpal_distance_matrix_device(ctx, P, k, dev_profiles, opt->metric, opt->do_balance, out_lower);
    CHK(tables_aligned(dev_profiles, dev_profiles));
    const uint64_t n = 1ULL << (2 * k);
    CrossSets c = {dev_profiles, dev_profiles, P, P, n, 1};
    if (opt->do_balance) CHK(balance_sets(ctx, k, c));
    if (opt->do_smooth) {
        for (int i = 1; i < P; ++i)
            for (int j = 0; j < i; ++j)
                CHK(profile_distance_pair(ctx, k, c.left + (uint64_t)i * n, c.left + (uint64_t)j * n, opt, true, &out_lower[triangle_index(i, j)]));
        return KPAL_OK;
    }
    return cross_option_core(ctx, c, opt, out_lower);
}

KPAL_API int kpal_profile_distance_matrix(kpal_ctx *ctx, int P, int k, const int64_t *const *host_profiles,
                                          const kpal_distance_options *opt, double *out_lower)
{
    CTX_ENTER(ctx);
    if (P < 1) return set_err(KPAL_E_INVALID, "P must be >= 1");
    if (k < 1 || k > KPAL_MAX_K) return set_err(KPAL_E_INVALID, "k=%d out of range", k);
    CHK(check_options(opt));
    if (P == 1) return KPAL_OK;
    if (!host_profiles || !out_lower) return set_err(KPAL_E_INVALID, "NULL pointer");
    if (options_plain(opt)) return kpal_distance_matrix(ctx, P, k, host_profiles, opt->metric, opt->do_balance, out_lower);
    const uint64_t n = 1ULL << (2 * k);
    CHK(ensure(ctx, ctx->opt_profiles, (size_t)P * n * 8));
    int64_t *prof = (int64_t *)ctx->opt_profiles.p;
    CHK(upload_set(ctx, prof, P, n, host_profiles, "profile"));
    // uploaded once; balanced once per profile and every pair in a fixed number of launches
    return kpal_profile_distance_matrix_device(ctx, P, k, prof, opt, out_lower);
}

// ----------------------------------------------------------------------------------------------
// dynamic smoothing over a rectangle / a lower triangle (smooth_plan.hpp, smooth_set_kernels.hpp)
// ----------------------------------------------------------------------------------------------
// The pyramids of the nprof profiles of c (smooth_set_kernels.hpp: left 0 .. Q-1, then right; nprof = Q reads the left set
// alone) in the context's opt_levels, their roots in scratch[kScratchTotals]: k level launches and the codes launch.
int smooth_set_pyramids(kpal_ctx *ctx, int k, const CrossSets &c, uint32_t nprof, int summary, double threshold, SmoothPyramids *out)
{
    const uint64_t stride = smooth_stride(k), elements = (uint64_t)nprof * stride;
    CHK(ensure(ctx, ctx->opt_levels, (size_t)smooth_scratch_bytes(k, nprof)));
    CHK(ensure(ctx, ctx->scratch[kScratchTotals], (size_t)nprof * sizeof(Partial)));
    int64_t *sums = (int64_t *)ctx->opt_levels.p;
    uint8_t *codes = (uint8_t *)(sums + elements);
    Partial *totals = (Partial *)ctx->scratch[kScratchTotals].p;
    const SmoothSet set = {c, nprof, k, stride, sums, codes, codes + elements, totals};
    for (int h = 0; h < k; ++h) {
        const uint32_t per = option_totals_gx(ctx->num_cu, nprof, smooth_level_nodes(k, h));
        LAUNCH(ctx, "smooth_set_level", smooth_set_level_kernel, dim3(nprof * per), dim3(256), set, h, per, summary, threshold);
    }
    const uint32_t per = option_totals_gx(ctx->num_cu, nprof, stride);
    LAUNCH(ctx, "smooth_set_codes", smooth_set_codes_kernel, dim3(nprof * per), dim3(256), set, per);
    *out = SmoothPyramids{sums, codes, totals, stride};
    return KPAL_OK;
}

// Every pair of c (c.tri: below the diagonal) with dynamic smoothing and no positive step, from tables that are already
// balanced and are not written.  out: Q x R row-major, or the lower triangle in distance_matrix order.
static int cross_smooth_core(kpal_ctx *ctx, int k, const CrossSets &c, const kpal_distance_options *opt, double *out)
{
    const bool scaled = opt->do_scale != 0, tri = c.tri != 0;
    const uint32_t nprof = tri ? (uint32_t)c.Q : (uint32_t)c.Q + (uint32_t)c.R;
    const uint64_t stride = smooth_stride(k);
    // both passes take the kernel kind and the grid of the bins: groups without a chunk of the (three times shorter) pyramids
    // write zeros, and the pyramid pass is `nacc` accumulators more of ONE partial layout
    const bool staged = cross_staged(c.Q, c.R, c.n);
    const CrossGrid g = cross_grid(ctx->num_cu, c, staged);
    const uint32_t nacc = option_nacc(opt->metric), gx = g.gx;
    const uint64_t slots = g.slots;
    if (partials_too_many(slots * nacc * 2, gx)) return set_err(KPAL_E_INVALID, "cross distance: %d x %d profiles are too many for one call", c.Q, c.R);
    CHK(ensure(ctx, ctx->partials, (size_t)slots * nacc * 2 * gx * sizeof(Partial)));
    SmoothPyramids pyr;
    CHK(smooth_set_pyramids(ctx, k, c, nprof, opt->summary, opt->threshold, &pyr));
    int64_t *sums = pyr.sums;
    uint8_t *codes = pyr.codes;
    Partial *pp = (Partial *)ctx->partials.p, *totals = pyr.totals;
    const uint8_t *rcodes = tri ? codes : codes + (uint64_t)c.Q * stride;
    const CrossCodeOpt bins = {{c, opt->down ? 1 : 0, totals, tri ? 0u : (uint32_t)c.Q, (uint32_t)slots}, codes, rcodes, stride, 2};
    const CrossSets pyramids = {sums, tri ? sums : sums + (uint64_t)c.Q * stride, c.Q, c.R, stride, c.tri};
    const CrossCodeOpt nodes = {{pyramids, bins.down, totals, bins.roff, bins.slots}, codes, rcodes, stride, 0};
    Partial *pass[2] = {pp, pp + slots * nacc * gx};
    const CrossCodeOpt *of[2] = {&bins, &nodes};
    const char *name = staged ? "smooth_set_super" : "smooth_set_tile";
    for (int i = 0; i < 2; ++i)
        CHK(with_metric(opt->metric, [&](auto m, auto s) { return launch_cross<SmoothAcc<m, s>>(ctx, name, staged, *of[i], g, pass[i]); }, scaled));
    std::vector<Partial> res;
    CHK(finish_partials(ctx, (uint32_t)(slots * nacc * 2), gx, res));
    fill_pairs(c, g.sideR, out, [&](uint64_t slot) {
        Partial p[3];
        for (uint32_t a = 0; a < nacc; ++a) {   // bins, then nodes: a fixed order
            const Partial &b = res[a * slots + slot], &n = res[(nacc + a) * slots + slot];
            p[a] = Partial{b.s + n.s, b.m + n.m};
        }
        return option_value(opt->metric, scaled, p, nacc, 1, 0);
    });
    return KPAL_OK;
}

KPAL_API int kpal_cross_smooth_distance_device(kpal_ctx *ctx, int k, int Q, const int64_t *dev_left, int R, const int64_t *dev_right,
                                               const kpal_distance_options *opt, double *out)
{
    CTX_ENTER(ctx);
    CHK(check_options(opt));
    if (!opt->do_smooth) return kpal_cross_profile_distance_device(ctx, k, Q, dev_left, R, dev_right, opt, out);
    CHK(cross_check(k, Q, R, 0, dev_left, dev_right, out));
    CHK(tables_aligned(dev_left, dev_right));
    // with positive, or past the budget: one pair pipeline per pair
    if (!smooth_batched(k, Q, R, opt->do_positive != 0, kSmoothBudgetBytes)) return kpal_cross_profile_distance_device(ctx, k, Q, dev_left, R, dev_right, opt, out);
    CrossSets c = {dev_left, dev_right, Q, R, 1ULL << (2 * k), 0};
    if (opt->do_balance) CHK(balance_sets(ctx, k, c));
    return cross_smooth_core(ctx, k, c, opt, out);
}

KPAL_API int kpal_smooth_distance_matrix_device(kpal_ctx *ctx, int P, int k, const int64_t *dev_profiles,
                                                const kpal_distance_options *opt, double *out_lower)
{
    CTX_ENTER(ctx);
    if (P < 1) return set_err(KPAL_E_INVALID, "P must be >= 1");
    if (k < 1 || k > KPAL_MAX_K) return set_err(KPAL_E_INVALID, "k=%d out of range", k);
    CHK(check_options(opt));
    if (P == 1) return KPAL_OK;
    if (!dev_profiles || !out_lower) return set_err(KPAL_E_INVALID, "NULL pointer");
    if (!opt->do_smooth || !smooth_batched(k, P, 0, opt->do_positive != 0, kSmoothBudgetBytes))
        return kpal_profile_distance_matrix_device(ctx, P, k, dev_profiles, opt, out_lower);
    CHK(tables_aligned(dev_profiles, dev_profiles));
    CrossSets c = {dev_profiles, dev_profiles, P, P, 1ULL << (2 * k), 1};
    if (opt->do_balance) CHK(balance_sets(ctx, k, c));
    return cross_smooth_core(ctx, k, c, opt, out_lower);
}
