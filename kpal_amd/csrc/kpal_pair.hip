// kpal_pair.hip -- everything of the C-ABI that works on ONE PAIR of count vectors: the plain pair distances (with the balance
// fused in LDS tiles for k >= 6), and the ProfileDistance option pipeline of a pair -- balance, positive, dynamic smoothing,
// scaling, the metric (option_kernels.hpp) -- which kpal_cross.hip and kpal_paired.hip fall back to where an option exists per pair only.
#include "kpal_host.hpp"
#include "dist_host.hpp"

#include "vec_kernels.hpp"
#include "option_kernels.hpp"

// A pair of host vectors of n 8-byte elements in scratch[kScratchUpload] and the buffer behind it.
template <typename T>
static int upload_pair(kpal_ctx *ctx, size_t n, const T *host_left, const T *host_right, const T **dl, const T **dr)
{
    DevBuf &bl = ctx->scratch[kScratchUpload], &br = ctx->scratch[kScratchUpload + 1];
    CHK(ensure(ctx, bl, n * 8));
    CHK(ensure(ctx, br, n * 8));
    HIPCHK(hipMemcpyAsync(bl.p, host_left, n * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(br.p, host_right, n * 8, hipMemcpyHostToDevice, ctx->stream));
    *dl = (const T *)bl.p;
    *dr = (const T *)br.p;
    return KPAL_OK;
}

template <typename T>
static int pair_distance_launch(kpal_ctx *ctx, size_t n, const T *dl, const T *dr, int metric, double *out, int64_t *aux)
{
    const unsigned grid = stream_grid(ctx, (n + 1) / 2);
    CHK(ensure(ctx, ctx->partials, (size_t)grid * sizeof(Partial)));
    Partial *pp = (Partial *)ctx->partials.p;
    CHK(with_metric<KPAL_EUCLIDEAN>(metric, [&](auto m) -> int {
        if constexpr (m == KPAL_EUCLIDEAN && !std::is_same<T, int64_t>::value) return set_err(KPAL_E_INVALID, "euclidean is int64 only");
        else LAUNCH(ctx, "pair_distance", (pair_distance_kernel<m, T>), dim3(grid), dim3(256), dl, dr, (uint64_t)n, pp);
        return KPAL_OK;
    }));
    std::vector<Partial> res;
    CHK(finish_partials(ctx, 1, grid, res));
    *out = finish_value(metric, res[0], aux);
    return KPAL_OK;
}

KPAL_API int kpal_pair_distance_device(kpal_ctx *ctx, size_t n, const int64_t *dev_left, const int64_t *dev_right,
                                       int metric, int do_balance, int k, double *out, int64_t *aux_out)
{
    CTX_ENTER(ctx);
    if (!dev_left || !dev_right || !out) return set_err(KPAL_E_INVALID, "NULL pointer");
    if (metric < 0 || metric > 2) return set_err(KPAL_E_INVALID, "unknown metric %d", metric);
    if (((uintptr_t)dev_left & 15) || ((uintptr_t)dev_right & 15)) return set_err(KPAL_E_INVALID, "device vectors must be 16-byte aligned");
    const int64_t *l = dev_left, *r = dev_right;
    if (do_balance) {
        if (k < 1 || k > KPAL_MAX_K || n != (1ULL << (2 * k))) return set_err(KPAL_E_INVALID, "do_balance needs n == 4^k");
        if (k >= 6) {   // fused balance + distance: balanced values are formed in LDS tiles, never written
            const uint32_t *canon = nullptr;
            uint32_t ncanon = 0;
            unsigned grid = 1;
            // persistent workgroups with prefetch, ONE per CU (120 registers), the pairs dealt round robin: every workgroup the same
            // number of pairs (k = 12: 0.099 -> 0.059 ms with the balanced deal)
            CHK(canon_tiles(ctx, k, 1, &canon, &ncanon, &grid));
            CHK(ensure(ctx, ctx->partials, (size_t)grid * sizeof(Partial)));
            Partial *pp = (Partial *)ctx->partials.p;
            CHK(with_metric<KPAL_EUCLIDEAN>(metric, [&](auto m) -> int {
                LAUNCH(ctx, "pair_distance_balanced", (pair_distance_balanced_kernel<m>), dim3(grid), dim3(1024), l, r, k, canon, ncanon, pp);
                return KPAL_OK;
            }));
            std::vector<Partial> res;
            CHK(finish_partials(ctx, 1, grid, res));
            *out = finish_value(metric, res[0], aux_out);
            return KPAL_OK;
        }
        DevBuf &bl = ctx->scratch[kScratchBalanced], &br = ctx->scratch[kScratchBalanced + 1];   // (no totals in this entry)
        CHK(ensure(ctx, bl, n * 8));
        CHK(ensure(ctx, br, n * 8));
        CHK(launch_balance(ctx, k, l, (int64_t *)bl.p));
        CHK(launch_balance(ctx, k, r, (int64_t *)br.p));
        l = (const int64_t *)bl.p;
        r = (const int64_t *)br.p;
    }
    return pair_distance_launch<int64_t>(ctx, n, l, r, metric, out, aux_out);
}

KPAL_API int kpal_pair_distance(kpal_ctx *ctx, size_t n, const int64_t *host_left, const int64_t *host_right,
                                int metric, int do_balance, int k, double *out, int64_t *aux_out)
{
    CTX_ENTER(ctx);
    if (!host_left || !host_right || !out) return set_err(KPAL_E_INVALID, "NULL pointer");
    const int64_t *dl = nullptr, *dr = nullptr;
    CHK(upload_pair(ctx, n, host_left, host_right, &dl, &dr));
    return kpal_pair_distance_device(ctx, n, dl, dr, metric, do_balance, k, out, aux_out);
}

KPAL_API int kpal_pair_distance_f64(kpal_ctx *ctx, size_t n, const double *host_left, const double *host_right,
                                    int pairwise, double *out, int64_t *aux_out)
{
    CTX_ENTER(ctx);
    if (!host_left || !host_right || !out) return set_err(KPAL_E_INVALID, "NULL pointer");
    if (pairwise != KPAL_PAIRWISE_PROD && pairwise != KPAL_PAIRWISE_SUM) return set_err(KPAL_E_INVALID, "pairwise must be prod or sum");
    const double *dl = nullptr, *dr = nullptr;
    CHK(upload_pair(ctx, n, host_left, host_right, &dl, &dr));
    return pair_distance_launch<double>(ctx, n, dl, dr, pairwise, out, aux_out);
}

// ----------------------------------------------------------------------------------------------
// ProfileDistance with options (kdistlib.py:126-161)
// ----------------------------------------------------------------------------------------------
int check_options(const kpal_distance_options *opt)
{
    if (!opt) return set_err(KPAL_E_INVALID, "options are NULL");
    if (opt->metric < 0 || opt->metric > KPAL_COSINE) return set_err(KPAL_E_INVALID, "unknown metric %d", opt->metric);
    if (opt->do_smooth && (opt->summary < KPAL_SUMMARY_MIN || opt->summary > KPAL_SUMMARY_MEDIAN))
        return set_err(KPAL_E_INVALID, "unknown summary function %d", opt->summary);
    return KPAL_OK;
}

// Dynamic smoothing of (l, r) into (lo, ro); in == out allowed.
static int launch_smooth(kpal_ctx *ctx, int k, const int64_t *l, const int64_t *r, int64_t *lo, int64_t *ro,
                         int summary, double threshold)
{
    // level d = 0..k-1 has 4^d nodes: two int64 sums and one decision byte each
    // (level starts padded to even entries: the kernels read 16 bytes at a time)
    const uint64_t total = ((1ULL << (2 * k)) - 1) / 3 + (uint64_t)k;
    CHK(ensure(ctx, ctx->opt_levels, (size_t)total * 17 + 64));
    int64_t *sl = (int64_t *)ctx->opt_levels.p, *sr = sl + total;
    uint8_t *dec = (uint8_t *)(sr + total);
    SmoothLevels lv = {};
    uint64_t at = 0;
    for (int d = 0; d < k; ++d) {
        lv.sum_l[d] = sl + at;
        lv.sum_r[d] = sr + at;
        lv.decide[d] = dec + at;
        at += (1ULL << (2 * d)) + (d == 0 ? 1 : 0);
    }
    for (int d = k - 1; d >= 0; --d) {
        const uint64_t nparent = 1ULL << (2 * d);
        const int64_t *cl = d == k - 1 ? l : lv.sum_l[d + 1];
        const int64_t *cr = d == k - 1 ? r : lv.sum_r[d + 1];
        LAUNCH(ctx, "smooth_level", smooth_level_kernel, dim3(stream_grid(ctx, nparent)), dim3(256), cl, cr, nparent,
               (int64_t *)lv.sum_l[d], (int64_t *)lv.sum_r[d], (uint8_t *)lv.decide[d], summary, threshold);
    }
    LAUNCH(ctx, "smooth_apply", smooth_apply_kernel, dim3(stream_grid(ctx, 1ULL << (2 * (k - 1)))), dim3(256), l, r, k, lv, lo, ro);
    return KPAL_OK;
}

// One pair, both vectors on the device and 16-byte aligned; `balanced`: the inputs are already
// balanced (matrix path), so opt->do_balance is not applied again.
int profile_distance_pair(kpal_ctx *ctx, int k, const int64_t *dl, const int64_t *dr, const kpal_distance_options *opt, bool balanced,
                          double *out)
{
    const uint64_t n = 1ULL << (2 * k);
    const bool do_balance = opt->do_balance && !balanced;
    if (options_plain(opt)) return kpal_pair_distance_device(ctx, n, dl, dr, opt->metric, do_balance, k, out, nullptr);
    const int64_t *l = dl, *r = dr;
    if (do_balance || opt->do_positive || opt->do_smooth) {
        CHK(ensure(ctx, ctx->opt_l, n * 8));
        CHK(ensure(ctx, ctx->opt_r, n * 8));
    }
    int64_t *wl = (int64_t *)ctx->opt_l.p, *wr = (int64_t *)ctx->opt_r.p;
    if (do_balance) {
        CHK(launch_balance(ctx, k, l, wl));
        CHK(launch_balance(ctx, k, r, wr));
        l = wl;
        r = wr;
    }
    if (opt->do_positive) {
        LAUNCH(ctx, "positive", positive_kernel, dim3(stream_grid(ctx, n)), dim3(256), l, r, wl, wr, n);
        l = wl;
        r = wr;
    }
    if (opt->do_smooth) {
        CHK(launch_smooth(ctx, k, l, r, wl, wr, opt->summary, opt->threshold));
        l = wl;
        r = wr;
    }
    const unsigned grid = stream_grid(ctx, n);
    CHK(ensure(ctx, ctx->partials, (size_t)grid * 3 * sizeof(Partial)));
    Partial *pp = (Partial *)ctx->partials.p;
    std::vector<Partial> res;
    double ls = 1.0, rs = 1.0;
    if (opt->do_scale) {
        LAUNCH(ctx, "totals", totals_kernel, dim3(grid), dim3(256), l, r, n, pp);
        CHK(finish_partials(ctx, 2, grid, res));
        scale_factors((int64_t)res[0].m, (int64_t)res[1].m, opt->down != 0, &ls, &rs);
    }
    const bool scaled = opt->do_scale != 0;
    CHK(with_metric(opt->metric, [&](auto m, auto s) -> int {
        LAUNCH(ctx, "option_distance", (option_distance_kernel<m, s>), dim3(grid), dim3(256), l, r, n, ls, rs, pp);
        return KPAL_OK;
    }, scaled));
    const uint32_t nacc = option_nacc(opt->metric);   // 1, or the cosine's 3: the dot and the two norms
    CHK(finish_partials(ctx, nacc, grid, res));
    *out = option_value(opt->metric, scaled, res.data(), nacc, 1, 0);
    return KPAL_OK;
}

KPAL_API int kpal_profile_distance_device(kpal_ctx *ctx, int k, const int64_t *dev_left, const int64_t *dev_right,
                                          const kpal_distance_options *opt, double *out)
{
    CTX_ENTER(ctx);
    if (k < 1 || k > KPAL_MAX_K) return set_err(KPAL_E_INVALID, "k=%d out of range", k);
    if (!dev_left || !dev_right || !out) return set_err(KPAL_E_INVALID, "NULL pointer");
    if (((uintptr_t)dev_left & 15) || ((uintptr_t)dev_right & 15)) return set_err(KPAL_E_INVALID, "device vectors must be 16-byte aligned");
    CHK(check_options(opt));
    return profile_distance_pair(ctx, k, dev_left, dev_right, opt, false, out);
}

KPAL_API int kpal_profile_distance(kpal_ctx *ctx, int k, const int64_t *host_left, const int64_t *host_right,
                                   const kpal_distance_options *opt, double *out)
{
    CTX_ENTER(ctx);
    if (k < 1 || k > KPAL_MAX_K) return set_err(KPAL_E_INVALID, "k=%d out of range", k);
    if (!host_left || !host_right || !out) return set_err(KPAL_E_INVALID, "NULL pointer");
    CHK(check_options(opt));
    const uint64_t n = 1ULL << (2 * k);
    const int64_t *dl = nullptr, *dr = nullptr;
    CHK(upload_pair(ctx, n, host_left, host_right, &dl, &dr));
    return profile_distance_pair(ctx, k, dl, dr, opt, false, out);
}

KPAL_API int kpal_dynamic_smooth(kpal_ctx *ctx, int k, int64_t *host_left_inout, int64_t *host_right_inout,
                                 int summary, double threshold)
{
    CTX_ENTER(ctx);
    if (k < 1 || k > KPAL_MAX_K) return set_err(KPAL_E_INVALID, "k=%d out of range", k);
    if (!host_left_inout || !host_right_inout) return set_err(KPAL_E_INVALID, "NULL pointer");
    if (summary < KPAL_SUMMARY_MIN || summary > KPAL_SUMMARY_MEDIAN) return set_err(KPAL_E_INVALID, "unknown summary function %d", summary);
    const uint64_t n = 1ULL << (2 * k);
    CHK(ensure(ctx, ctx->opt_l, n * 8));
    CHK(ensure(ctx, ctx->opt_r, n * 8));
    int64_t *wl = (int64_t *)ctx->opt_l.p, *wr = (int64_t *)ctx->opt_r.p;
    HIPCHK(hipMemcpyAsync(wl, host_left_inout, n * 8, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(wr, host_right_inout, n * 8, hipMemcpyHostToDevice, ctx->stream));
    CHK(launch_smooth(ctx, k, wl, wr, wl, wr, summary, threshold));
    HIPCHK(hipMemcpyAsync(host_left_inout, wl, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(host_right_inout, wr, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return KPAL_OK;
}
