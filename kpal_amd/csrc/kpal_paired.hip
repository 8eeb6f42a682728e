// kpal_paired.hip -- the part of the C-ABI that compares two sets of profiles pair by LINKED pair: out[i] = the ProfileDistance
// of (left table i, right table i) for all i (kpal_paired_distance[_device]; kdistlib.paired_distances / successive_distances,
// `kpal distance`).  Planned by pair_set_plan.hpp, the kernels are pair_set_kernels.hpp.  Per chunk of pairs a fixed number of
// launches whatever N is:
//   no scale          the metric kernel, one reduction
//   scale             the totals kernel (masked under positive), a reduction, the metric kernel, a reduction
//   do_balance        before them one launch of the set balance per distinct input range (balanced_pair_chunk, dist_host.hpp): the union of
//                     the two ranges once when they are the same range or lie a whole number of tables apart
//   do_smooth         the pair pipeline (kpal_pair.hip) once per pair on the once-balanced tables (the smoothed pair kernel over
//                     per-profile pyramids is kpal_paired_smooth_distance_device, kpal_paired_smooth.hip)
// The inputs are never written and may alias in any way.
#include "kpal_host.hpp"
#include "dist_host.hpp"

#include "pair_set_kernels.hpp"

// The cn pairs (left + i * bins, right + i * bins) of one chunk, from tables that are already balanced: no smoothing.
static int paired_chunk(kpal_ctx *ctx, uint64_t bins, uint64_t cn, const int64_t *left, const int64_t *right, const kpal_distance_options *opt,
                        double *out)
{
    const bool scaled = opt->do_scale != 0, positive = opt->do_positive != 0, wave = pair_set_wave_form(bins);
    const uint64_t slices = pair_set_slices(bins);
    const uint32_t nacc = option_nacc(opt->metric), nacc_max = std::max(nacc, scaled ? 2u : 1u);
    if (partials_too_many(cn * nacc_max, (uint32_t)slices)) return set_err(KPAL_E_INVALID, "paired distance: %llu pairs are too many for one chunk", (unsigned long long)cn);
    CHK(ensure(ctx, ctx->partials, (size_t)(cn * nacc_max * slices) * sizeof(Partial)));
    if (scaled) CHK(ensure(ctx, ctx->scratch[kScratchTotals], (size_t)cn * 2 * sizeof(Partial)));
    Partial *pp = (Partial *)ctx->partials.p, *totals = scaled ? (Partial *)ctx->scratch[kScratchTotals].p : nullptr;
    const PairSetArgs a = {left, right, bins, (uint32_t)cn, (uint32_t)slices, (uint32_t)pair_set_units(cn, bins), opt->down ? 1 : 0, totals};
    const dim3 grid((unsigned)pair_set_workgroups(cn, bins, (uint64_t)ctx->num_cu)), block(kPairSetThreads);
    if (scaled) {
        // the totals of every pair, reduced on the device: the metric pass derives the factors from them, no host round trip
        CHK(with_flags([&](auto p, auto w) -> int {
            LAUNCH(ctx, "pair_set_totals", (pair_set_totals_kernel<p, w>), grid, block, a, pp);
            return KPAL_OK;
        }, positive, wave));
        CHK(reduce_partials(ctx, pp, (uint32_t)(cn * 2), (uint32_t)slices, totals));
    }
    CHK(with_metric(opt->metric, [&](auto m, auto s, auto p, auto w) -> int {
        LAUNCH(ctx, "pair_set", (pair_set_kernel<m, s, p, w>), grid, block, a, pp);
        return KPAL_OK;
    }, scaled, positive, wave));
    std::vector<Partial> res;
    CHK(finish_partials(ctx, (uint32_t)(cn * nacc), (uint32_t)slices, res));
    for (uint64_t p = 0; p < cn; ++p) out[p] = option_value(opt->metric, scaled, res.data(), nacc, cn, p);
    return KPAL_OK;
}

KPAL_API int kpal_paired_distance_device(kpal_ctx *ctx, int k, int64_t N, const int64_t *dev_left, const int64_t *dev_right,
                                         const kpal_distance_options *opt, int64_t chunk_pairs, double *out)
{
    CTX_ENTER(ctx);
    CHK(paired_checks(k, N, dev_left, dev_right, out));
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
        if (do_balance) CHK(balanced_pair_chunk(ctx, k, cn, bins, pair_set_union(cn, alias, lag), lag, &cl, &cr));
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
    return paired_host_entry(ctx, k, N, host_left, host_right, opt, out, kpal_paired_distance_device);
}
