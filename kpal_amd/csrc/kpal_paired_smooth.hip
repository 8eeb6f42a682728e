// kpal_paired_smooth.hip -- the part of the C-ABI that smooths the LINKED pairs of two sets of profiles dynamically in a fixed
// number of launches: out[i] = the ProfileDistance with do_smooth of (left table i, right table i)
// (kpal_paired_smooth_distance[_device]; kdistlib.paired_distances / successive_distances, `kpal distance -m`), and the smoothed
// tables themselves (kpal_paired_smooth_device; klib.smooth_profiles, `kpal smooth`).  Planned by pair_smooth_plan.hpp, the
// kernels are pair_smooth_kernels.hpp.  Per chunk of pairs, whatever N is:
//   do_balance        one launch of the set balance per distinct input range: kpal_paired_distance_device's balanced_pair_chunk (dist_host.hpp)
//   the pyramids      of the chunk's distinct tables once (the union of the two ranges when they are the same range or lie a
//                     whole number of tables apart): k level launches and the codes launch (smooth_set_pyramids, kpal_cross.hip)
//   distances         ONE launch of pair_smooth over all (pair, slice) items and ONE reduction -- no totals pass under scale:
//                     the roots of the pyramids are the totals
//   tables            ONE launch of pair_smooth_apply, which writes both output sets
// Without do_smooth, and with do_positive (the masks come first: node sums depend on the partner), kpal_paired_distance_device
// serves the call.  The inputs are never written and may alias in any way.
#include "kpal_host.hpp"
#include "dist_host.hpp"

#include "pair_smooth_kernels.hpp"

// The pyramids of the distinct tables of the cn pairs (cl + i * bins, cr + i * bins): of the union of the two ranges (un tables
// from the lower one on) or of the two sides, left first.  -> the kernels' arguments but for the grid.
static int pair_smooth_pyramids(kpal_ctx *ctx, int k, uint64_t cn, const int64_t *cl, const int64_t *cr, uint64_t un, int alias, int64_t lag,
                                int summary, double threshold, int down, PairSmoothArgs *a)
{
    const uint64_t bins = 1ULL << (2 * k);
    const CrossSets c = un ? CrossSets{lag < 0 ? cr : cl, nullptr, (int)un, 0, bins, 0} : CrossSets{cl, cr, (int)cn, (int)cn, bins, 0};
    SmoothPyramids pyr;
    CHK(smooth_set_pyramids(ctx, k, c, (uint32_t)(un ? un : 2 * cn), summary, threshold, &pyr));
    *a = PairSmoothArgs{cl, cr, pyr.sums, pyr.codes, pyr.totals, bins, pyr.stride, (uint32_t)cn, (uint32_t)pair_smooth_bin_slices(k), (uint32_t)pair_smooth_slices(k), 0,
                        (uint32_t)pair_smooth_left(cn, alias, lag, 0), (uint32_t)pair_smooth_right(cn, alias, lag, 0), k, down};
    return KPAL_OK;
}

KPAL_API int kpal_paired_smooth_distance_device(kpal_ctx *ctx, int k, int64_t N, const int64_t *dev_left, const int64_t *dev_right,
                                                const kpal_distance_options *opt, int64_t chunk_pairs, double *out)
{
    CTX_ENTER(ctx);
    CHK(paired_checks(k, N, dev_left, dev_right, out));
    CHK(check_options(opt));
    if (chunk_pairs < 0) return set_err(KPAL_E_INVALID, "chunk_pairs must be >= 0");
    const uint64_t bins = 1ULL << (2 * k);
    if (!transform_bytes_fit((uint64_t)N, bins) || (uint64_t)N > SIZE_MAX / 8) return set_err(KPAL_E_INVALID, "%lld pairs at k=%d: too many bytes", (long long)N, k);
    if (!pair_smooth_batched(opt->do_smooth != 0, opt->do_positive != 0)) return kpal_paired_distance_device(ctx, k, N, dev_left, dev_right, opt, chunk_pairs, out);
    const bool do_balance = opt->do_balance != 0, scaled = opt->do_scale != 0, wave = pair_set_wave_form(bins);
    int64_t lag = 0;
    const int alias = pair_set_alias((uint64_t)(uintptr_t)dev_left, (uint64_t)(uintptr_t)dev_right, (uint64_t)N, bins, &lag);
    const uint64_t chunk = pair_smooth_chunk(k, (uint64_t)N, do_balance, (uint64_t)chunk_pairs, alias, lag);
    const uint32_t nacc = option_nacc(opt->metric), slices = (uint32_t)pair_smooth_slices(k);
    for (uint64_t c0 = 0; c0 < (uint64_t)N; c0 += chunk) {
        const uint64_t cn = std::min<uint64_t>(chunk, (uint64_t)N - c0);
        const int64_t *cl = dev_left + c0 * bins, *cr = dev_right + c0 * bins;
        const uint64_t un = pair_set_union(cn, alias, lag);
        if (do_balance) CHK(balanced_pair_chunk(ctx, k, cn, bins, un, lag, &cl, &cr));   // as kpal_paired_distance_device balances them
        if (partials_too_many(cn * nacc, slices)) return set_err(KPAL_E_INVALID, "paired distance: %llu pairs are too many for one chunk", (unsigned long long)cn);
        CHK(ensure(ctx, ctx->partials, (size_t)(cn * nacc * slices) * sizeof(Partial)));
        PairSmoothArgs a;
        CHK(pair_smooth_pyramids(ctx, k, cn, cl, cr, un, alias, lag, opt->summary, opt->threshold, opt->down ? 1 : 0, &a));
        a.units = (uint32_t)pair_smooth_units(cn, k);
        Partial *pp = (Partial *)ctx->partials.p;
        const dim3 grid((unsigned)pair_smooth_workgroups(cn, k, (uint64_t)ctx->num_cu)), block(kPairSetThreads);
        CHK(with_metric(opt->metric, [&](auto m, auto s, auto w) -> int {
            LAUNCH(ctx, "pair_smooth", (pair_smooth_kernel<m, s, w>), grid, block, a, pp);
            return KPAL_OK;
        }, scaled, wave));
        std::vector<Partial> res;
        CHK(finish_partials(ctx, (uint32_t)(cn * nacc), slices, res));
        for (uint64_t p = 0; p < cn; ++p) out[c0 + p] = option_value(opt->metric, scaled, res.data(), nacc, cn, p);
    }
    return KPAL_OK;
}

KPAL_API int kpal_paired_smooth_distance(kpal_ctx *ctx, int k, int64_t N, const int64_t *const *host_left, const int64_t *const *host_right,
                                         const kpal_distance_options *opt, double *out)
{
    return paired_host_entry(ctx, k, N, host_left, host_right, opt, out, kpal_paired_smooth_distance_device);
}

// Whether the byte ranges [a, a + n) and [b, b + n) meet.
static bool ranges_meet(const void *a, const void *b, uint64_t n)
{
    const uint64_t x = (uint64_t)(uintptr_t)a, y = (uint64_t)(uintptr_t)b;
    return (x > y ? x - y : y - x) < n;
}

KPAL_API int kpal_paired_smooth_device(kpal_ctx *ctx, int k, int64_t N, const int64_t *dev_left, const int64_t *dev_right, int summary,
                                       double threshold, int64_t chunk_pairs, int64_t *dev_out_left, int64_t *dev_out_right)
{
    CTX_ENTER(ctx);
    CHK(paired_checks(k, N, dev_left, dev_right, dev_out_left));
    if (!dev_out_right) return set_err(KPAL_E_INVALID, "NULL pointer");
    if (summary < 0 || summary > KPAL_SUMMARY_MEDIAN) return set_err(KPAL_E_INVALID, "unknown summary function %d", summary);
    if (chunk_pairs < 0) return set_err(KPAL_E_INVALID, "chunk_pairs must be >= 0");
    const uint64_t bins = 1ULL << (2 * k);
    if (!transform_bytes_fit((uint64_t)N, bins) || (uint64_t)N > SIZE_MAX / 8) return set_err(KPAL_E_INVALID, "%lld pairs at k=%d: too many bytes", (long long)N, k);
    if (((uintptr_t)dev_out_left & 15) || ((uintptr_t)dev_out_right & 15)) return set_err(KPAL_E_INVALID, "output tables must be 16-byte aligned");
    const uint64_t bytes = (uint64_t)N * bins * 8;
    if (ranges_meet(dev_out_left, dev_out_right, bytes) || ranges_meet(dev_out_left, dev_left, bytes) || ranges_meet(dev_out_left, dev_right, bytes) ||
        ranges_meet(dev_out_right, dev_left, bytes) || ranges_meet(dev_out_right, dev_right, bytes))
        return set_err(KPAL_E_INVALID, "output tables overlap each other or the inputs");
    const bool wave = pair_set_wave_form(bins);
    int64_t lag = 0;
    const int alias = pair_set_alias((uint64_t)(uintptr_t)dev_left, (uint64_t)(uintptr_t)dev_right, (uint64_t)N, bins, &lag);
    const uint64_t chunk = pair_smooth_chunk(k, (uint64_t)N, false, (uint64_t)chunk_pairs, alias, lag);
    for (uint64_t c0 = 0; c0 < (uint64_t)N; c0 += chunk) {
        const uint64_t cn = std::min<uint64_t>(chunk, (uint64_t)N - c0);
        PairSmoothArgs a;
        CHK(pair_smooth_pyramids(ctx, k, cn, dev_left + c0 * bins, dev_right + c0 * bins, pair_set_union(cn, alias, lag), alias, lag, summary, threshold, 0, &a));
        a.units = (uint32_t)pair_set_units(cn, bins);
        const dim3 g((unsigned)pair_set_workgroups(cn, bins, (uint64_t)ctx->num_cu)), b(kPairSetThreads);
        if (wave) LAUNCH(ctx, "pair_smooth_apply", pair_smooth_apply_kernel<true>, g, b, a, dev_out_left + c0 * bins, dev_out_right + c0 * bins);
        else LAUNCH(ctx, "pair_smooth_apply", pair_smooth_apply_kernel<false>, g, b, a, dev_out_left + c0 * bins, dev_out_right + c0 * bins);
    }
    return KPAL_OK;
}
