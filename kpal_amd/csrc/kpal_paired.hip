// kpal_paired.hip -- the part of the C-ABI that compares two sets of profiles pair by LINKED pair: out[i] = the ProfileDistance
// of (left table i, right table i) for all i (kpal_paired_distance[_device]; kdistlib.paired_distances / successive_distances,
// `kpal distance`).  Planned by pair_set_plan.hpp, the kernels are pair_set_kernels.hpp.  Per chunk of pairs a fixed number of
// launches whatever N is:
//   no scale          the metric kernel, one reduction
//   scale             the totals kernel (masked under positive), a reduction, the metric kernel, a reduction
//   do_balance        before them one launch of the set balance per distinct input range, into context scratch: the union of
//                     the two ranges once when they are the same range or lie a whole number of tables apart
//   do_smooth         the pair pipeline (kpal_pair.hip) once per pair on the once-balanced tables (the smoothed pair kernel over
//                     per-profile pyramids is kpal_paired_smooth_distance_device, kpal_paired_smooth.hip)
// The inputs are never written and may alias in any way.
#include "kpal_host.hpp"

#include "pair_set_kernels.hpp"

template <int MODE, bool WAVE>
static int launch_pair_set_metric(kpal_ctx *ctx, bool scaled, bool positive, unsigned grid, const PairSetArgs &a, Partial *pp)
{
    const dim3 g(grid), b(kPairSetThreads);
    if (scaled && positive) LAUNCH(ctx, "pair_set", (pair_set_kernel<MODE, true, true, WAVE>), g, b, a, pp);
    else if (scaled) LAUNCH(ctx, "pair_set", (pair_set_kernel<MODE, true, false, WAVE>), g, b, a, pp);
    else if (positive) LAUNCH(ctx, "pair_set", (pair_set_kernel<MODE, false, true, WAVE>), g, b, a, pp);
    else LAUNCH(ctx, "pair_set", (pair_set_kernel<MODE, false, false, WAVE>), g, b, a, pp);
    return KPAL_OK;
}

template <bool WAVE>
static int launch_pair_set(kpal_ctx *ctx, int metric, bool scaled, bool positive, unsigned grid, const PairSetArgs &a, Partial *pp)
{
    switch (metric) {
    case KPAL_PAIRWISE_PROD: return launch_pair_set_metric<0, WAVE>(ctx, scaled, positive, grid, a, pp);
    case KPAL_PAIRWISE_SUM: return launch_pair_set_metric<1, WAVE>(ctx, scaled, positive, grid, a, pp);
    case KPAL_EUCLIDEAN: return launch_pair_set_metric<2, WAVE>(ctx, scaled, positive, grid, a, pp);
    default: return launch_pair_set_metric<3, WAVE>(ctx, scaled, positive, grid, a, pp);
    }
}

template <bool WAVE>
static int launch_pair_set_totals(kpal_ctx *ctx, bool positive, unsigned grid, const PairSetArgs &a, Partial *pp)
{
    const dim3 g(grid), b(kPairSetThreads);
    if (positive) LAUNCH(ctx, "pair_set_totals", (pair_set_totals_kernel<true, WAVE>), g, b, a, pp);
    else LAUNCH(ctx, "pair_set_totals", (pair_set_totals_kernel<false, WAVE>), g, b, a, pp);
    return KPAL_OK;
}

// The cn pairs (left + i * bins, right + i * bins) of one chunk, from tables that are already balanced: no smoothing.
static int paired_chunk(kpal_ctx *ctx, uint64_t bins, uint64_t cn, const int64_t *left, const int64_t *right, const kpal_distance_options *opt,
                        double *out)
{
    const bool scaled = opt->do_scale != 0, positive = opt->do_positive != 0, wave = pair_set_wave_form(bins);
    const uint64_t slices = pair_set_slices(bins);
    const uint32_t nacc = option_nacc(opt->metric), nacc_max = std::max(nacc, scaled ? 2u : 1u);
    if (partials_too_many(cn * nacc_max, (uint32_t)slices)) return set_err(KPAL_E_INVALID, "paired distance: %llu pairs are too many for one chunk", (unsigned long long)cn);
    CHK(ensure(ctx, ctx->partials, (size_t)(cn * nacc_max * slices) * sizeof(Partial)));
    if (scaled) CHK(ensure(ctx, ctx->scratch[3], (size_t)cn * 2 * sizeof(Partial)));
    Partial *pp = (Partial *)ctx->partials.p, *totals = scaled ? (Partial *)ctx->scratch[3].p : nullptr;
    const PairSetArgs a = {left, right, bins, (uint32_t)cn, (uint32_t)slices, (uint32_t)pair_set_units(cn, bins), opt->down ? 1 : 0, totals};
    const unsigned grid = (unsigned)pair_set_workgroups(cn, bins, (uint64_t)ctx->num_cu);
    if (scaled) {
        // the totals of every pair, reduced on the device: the metric pass derives the factors from them, no host round trip
        if (wave) CHK(launch_pair_set_totals<true>(ctx, positive, grid, a, pp));
        else CHK(launch_pair_set_totals<false>(ctx, positive, grid, a, pp));
        CHK(reduce_partials(ctx, pp, (uint32_t)(cn * 2), (uint32_t)slices, totals));
    }
    if (wave) CHK(launch_pair_set<true>(ctx, opt->metric, scaled, positive, grid, a, pp));
    else CHK(launch_pair_set<false>(ctx, opt->metric, scaled, positive, grid, a, pp));
    std::vector<Partial> res;
    CHK(finish_partials(ctx, (uint32_t)(cn * nacc), (uint32_t)slices, res));
    for (uint64_t p = 0; p < cn; ++p)   // (accumulators 1 and 2 exist for the cosine only: p0 again, unread)
        out[p] = finish_distance(opt->metric, scaled, res[p], res[(nacc / 2) * cn + p], res[(nacc - 1) * cn + p]);
    return KPAL_OK;
}

KPAL_API int kpal_paired_distance_device(kpal_ctx *ctx, int k, int64_t N, const int64_t *dev_left, const int64_t *dev_right,
                                         const kpal_distance_options *opt, int64_t chunk_pairs, double *out)
{
    CTX_ENTER(ctx);
    if (N < 1) return set_err(KPAL_E_INVALID, "N must be >= 1");
    if (k < 1 || k > KPAL_MAX_K) return set_err(KPAL_E_INVALID, "k=%d out of range", k);
    if (!dev_left || !dev_right || !out) return set_err(KPAL_E_INVALID, "NULL pointer");
    if (((uintptr_t)dev_left & 15) || ((uintptr_t)dev_right & 15)) return set_err(KPAL_E_INVALID, "device tables must be 16-byte aligned");
    CHK(check_options(opt));
    if (chunk_pairs < 0) return set_err(KPAL_E_INVALID, "chunk_pairs must be >= 0");
    const uint64_t bins = 1ULL << (2 * k);
    if (!transform_bytes_fit((uint64_t)N, bins) || (uint64_t)N > SIZE_MAX / 8) return set_err(KPAL_E_INVALID, "%lld pairs at k=%d: too many bytes", (long long)N, k);
    const bool do_balance = opt->do_balance != 0;
    const uint64_t chunk = pair_set_chunk((uint64_t)N, bins, do_balance, (uint64_t)chunk_pairs);
    int64_t lag = 0;
    const int alias = pair_set_alias((uint64_t)(uintptr_t)dev_left, (uint64_t)(uintptr_t)dev_right, (uint64_t)N, bins, &lag);
    for (uint64_t c0 = 0; c0 < (uint64_t)N; c0 += chunk) {
        const uint64_t cn = std::min<uint64_t>(chunk, (uint64_t)N - c0);
        const int64_t *cl = dev_left + c0 * bins, *cr = dev_right + c0 * bins;
        if (do_balance) {
            // balanced once per table: identical to the reference balancing copies per pair (kdistlib.py:136-141)
            const uint64_t un = alias == kPairSetSame ? cn : alias == kPairSetLag ? pair_set_union_tables(cn, lag) : 0;
            CHK(ensure(ctx, ctx->scratch[2], (size_t)pair_set_balance_bytes(cn, bins, un)));
            int64_t *b = (int64_t *)ctx->scratch[2].p;
            if (un) {   // one range covers both sides: its tables once, both sides point into the copy
                CHK(balance_set_launch(ctx, k, (size_t)un, lag < 0 ? cr : cl, b));
                cl = b + (lag < 0 ? (uint64_t)(-lag) : 0) * bins;
                cr = b + (lag > 0 ? (uint64_t)lag : 0) * bins;
            } else {
                CHK(balance_set_launch(ctx, k, (size_t)cn, cl, b));
                CHK(balance_set_launch(ctx, k, (size_t)cn, cr, b + cn * bins));
                cl = b;
                cr = b + cn * bins;
            }
        }
        if (opt->do_smooth) {
            // the smoothed tables of a pair are materialised: the pair pipeline on the balanced tables, pair by pair
            for (uint64_t p = 0; p < cn; ++p) CHK(profile_distance_pair(ctx, k, cl + p * bins, cr + p * bins, opt, true, &out[c0 + p]));
            continue;
        }
        CHK(paired_chunk(ctx, bins, cn, cl, cr, opt, out + c0));
    }
    return KPAL_OK;
}

KPAL_API int kpal_paired_distance(kpal_ctx *ctx, int k, int64_t N, const int64_t *const *host_left, const int64_t *const *host_right,
                                  const kpal_distance_options *opt, double *out)
{
    CTX_ENTER(ctx);
    if (N < 1) return set_err(KPAL_E_INVALID, "N must be >= 1");
    if (k < 1 || k > KPAL_MAX_K) return set_err(KPAL_E_INVALID, "k=%d out of range", k);
    if (!host_left || !host_right || !out) return set_err(KPAL_E_INVALID, "NULL pointer");
    CHK(check_options(opt));
    const uint64_t bins = 1ULL << (2 * k);
    if (N > 0x3fffffff || !transform_bytes_fit((uint64_t)N * 2, bins)) return set_err(KPAL_E_INVALID, "%lld pairs at k=%d: too many bytes", (long long)N, k);
    for (int64_t p = 0; p < N; ++p)
        if (!host_left[p] || !host_right[p]) return set_err(KPAL_E_INVALID, "%s profile %lld is NULL", host_left[p] ? "right" : "left", (long long)p);
    int64_t *dl = nullptr, *dr = nullptr;
    CHK(upload_rectangle(ctx, bins, (int)N, host_left, (int)N, host_right, &dl, &dr));
    return kpal_paired_distance_device(ctx, k, N, dl, dr, opt, 0, out);
}
