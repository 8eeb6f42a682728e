// dist_host.hpp -- the host front end the five distance units share (kpal_pair.hip, kpal_cross.hip, kpal_paired.hip,
// kpal_paired_smooth.hip, kpal_nearest.hip; included after kpal_host.hpp, host code only): runtime metric and flags -> one kernel
// instantiation, a pair's distance from its reduced accumulators, the loop that fills a triangle or a rectangle, the balanced
// working copies of a chunk of linked pairs, the argument checks entries have in common, and what one of these units calls in
// another.  Which workspace buffer holds what, and who may grow it: the table at kpal_ctx::scratch (kpal_host.hpp).
#pragma once
#include "pair_set_plan.hpp"

// ---- dispatch ---------------------------------------------------------------------------------------------------------------
// with_flags(f, b...) calls f(std::true_type / std::false_type ...), with_metric<LAST>(metric, f, b...) puts
// std::integral_constant<int, M> before them: M = metric for 0 .. 2 and LAST for anything else -- KPAL_COSINE, or
// KPAL_EUCLIDEAN where a kernel family ends there (its entries have refused a larger metric).  The constants convert to the
// template arguments of a kernel; f returns the error code.  EVERY combination of f is instantiated: a combination that has no
// kernel is an `if constexpr` in f.
template <class C, class F>
static auto bound(F &f)
{
    return [&f](auto... c) -> int { return f(C{}, c...); };
}
template <class F>
static int with_flags(F f) { return f(); }
template <class F, class... Flags>
static int with_flags(F f, bool b, Flags... flags)
{
    return b ? with_flags(bound<std::true_type>(f), flags...) : with_flags(bound<std::false_type>(f), flags...);
}
template <int LAST = KPAL_COSINE, class F, class... Flags>
static int with_metric(int metric, F f, Flags... flags)
{
    switch (metric) {
    case KPAL_PAIRWISE_PROD: return with_flags(bound<std::integral_constant<int, KPAL_PAIRWISE_PROD>>(f), flags...);
    case KPAL_PAIRWISE_SUM: return with_flags(bound<std::integral_constant<int, KPAL_PAIRWISE_SUM>>(f), flags...);
    case KPAL_EUCLIDEAN: return with_flags(bound<std::integral_constant<int, KPAL_EUCLIDEAN>>(f), flags...);
    default: return with_flags(bound<std::integral_constant<int, LAST>>(f), flags...);
    }
}

// ---- finishing ----------------------------------------------------------------------------------------------------------------
// The distance of pair i from its reduced accumulators, accumulator a at res[a * groups + i]: option_nacc(metric) of them --
// accumulators 1 and 2 exist for the cosine only (else: accumulator 0 again, unread).
inline double option_value(int metric, bool scaled, const Partial *res, uint32_t nacc, uint64_t groups, uint64_t i)
{
    return finish_distance(metric, scaled, res[i], res[(nacc / 2) * groups + i], res[(nacc - 1) * groups + i]);
}

// out: the lower triangle of c in distance_matrix order (c.tri), or Q x R row-major; value(slot): the distance of the pair whose
// partials lie at cross_slot(c, sideR, i, j).
template <class Value>
static void fill_pairs(const CrossSets &c, int sideR, double *out, Value value)
{
    for (int i = c.tri ? 1 : 0; i < c.Q; ++i)
        for (int j = 0; j < (c.tri ? i : c.R); ++j) out[c.tri ? triangle_index(i, j) : (size_t)i * c.R + j] = value(cross_slot(c, sideR, i, j));
}

// ---- argument checks ----------------------------------------------------------------------------------------------------------
// An entry shares one of these only where the ORDER of its checks is this one already (tests/test_gpu_set_arguments.py,
// test_gpu_distance_arguments.py pin the order with double faults).
inline int tables_aligned(const void *left, const void *right)
{
    if (((uintptr_t)left & 15) || ((uintptr_t)right & 15)) return set_err(KPAL_E_INVALID, "device tables must be 16-byte aligned");
    return KPAL_OK;
}
// A rectangle: Q and R, k, the metric (an option entry passes 0), the pointers (host or device).
inline int cross_check(int k, int Q, int R, int metric, const void *left, const void *right, const void *out)
{
    if (Q < 1 || R < 1) return set_err(KPAL_E_INVALID, "Q and R must be >= 1");
    if (k < 1 || k > KPAL_MAX_K) return set_err(KPAL_E_INVALID, "k=%d out of range", k);
    if (metric < 0 || metric > 2) return set_err(KPAL_E_INVALID, "unknown metric %d", metric);
    if (!left || !right || !out) return set_err(KPAL_E_INVALID, "NULL pointer");
    return KPAL_OK;
}
// The linked pairs on the device: N, k, the pointers, the alignment of the inputs.
inline int paired_checks(int k, int64_t N, const void *dev_left, const void *dev_right, const void *out)
{
    if (N < 1) return set_err(KPAL_E_INVALID, "N must be >= 1");
    if (k < 1 || k > KPAL_MAX_K) return set_err(KPAL_E_INVALID, "k=%d out of range", k);
    if (!dev_left || !dev_right || !out) return set_err(KPAL_E_INVALID, "NULL pointer");
    return tables_aligned(dev_left, dev_right);
}
int check_options(const kpal_distance_options *opt);                       // kpal_pair.hip

// ---- what one distance unit calls in another ------------------------------------------------------------------------------------
int profile_distance_pair(kpal_ctx *ctx, int k, const int64_t *dl, const int64_t *dr, const kpal_distance_options *opt, bool balanced,
                          double *out);   // kpal_pair.hip: the option pipeline of one pair of 16-byte aligned device tables (balanced: do_balance is not applied again)
// kpal_cross.hip: the launches of the rectangle cores up to where their host loops begin -- the workgroup partials are left in
// ctx->partials for finish_partials, or for kpal_nearest.hip, which reduces and finishes them on the device
struct CrossGramLayout {
    int blocksR;
    uint32_t gx;
    size_t dots, groups;   // reduced: the dot of (q, r) at cross_gram_index(blocksR, q, r), the Q + R norms from `dots` on
};
int balance_set(kpal_ctx *ctx, int k, int count, const int64_t *src, int64_t *dst);
int upload_rectangle(kpal_ctx *ctx, uint64_t n, int Q, const int64_t *const *host_left, int R, const int64_t *const *host_right,
                     int64_t **dl, int64_t **dr);   // the left and the right set, one behind the other in scratch[kScratchUpload]
int cross_gram_launch(kpal_ctx *ctx, const CrossSets &c, CrossGramLayout *lay);
int cross_pairs_launch(kpal_ctx *ctx, const CrossSets &c, int metric, bool staged, bool recip, CrossGrid *grid);
int cross_option_launch(kpal_ctx *ctx, const CrossSets &c, const kpal_distance_options *opt, CrossGrid *grid);
struct SmoothPyramids {   // smooth_plan.hpp: one pyramid per profile, in the context's workspace
    int64_t *sums;
    uint8_t *codes;
    Partial *totals;   // .m: the root of every pyramid, its table's np.sum
    uint64_t stride;
};
int smooth_set_pyramids(kpal_ctx *ctx, int k, const CrossSets &c, uint32_t nprof, int summary, double threshold,
                        SmoothPyramids *out);   // kpal_cross.hip: the k level launches and the codes launch of dynamic smoothing over sets

// ---- linked pairs ---------------------------------------------------------------------------------------------------------------
// Balanced working copies of the cn linked pairs (*cl + i * bins, *cr + i * bins) in scratch[kScratchBalanced], *cl and *cr
// pointed at them: the un = pair_set_union() tables of the union of the two ranges once, both sides `lag` tables apart in that
// copy, or (un = 0) the two sides, left first.  Balanced once per table: identical to the reference balancing copies per pair
// (kdistlib.py:136-141).
inline int balanced_pair_chunk(kpal_ctx *ctx, int k, uint64_t cn, uint64_t bins, uint64_t un, int64_t lag, const int64_t **cl, const int64_t **cr)
{
    CHK(ensure(ctx, ctx->scratch[kScratchBalanced], (size_t)pair_set_balance_bytes(cn, bins, un)));
    int64_t *b = (int64_t *)ctx->scratch[kScratchBalanced].p;
    if (un) {
        CHK(balance_set_launch(ctx, k, (size_t)un, lag < 0 ? *cr : *cl, b));
        *cl = b + (lag < 0 ? (uint64_t)(-lag) : 0) * bins;
        *cr = b + (lag > 0 ? (uint64_t)lag : 0) * bins;
    } else {
        CHK(balance_set_launch(ctx, k, (size_t)cn, *cl, b));
        CHK(balance_set_launch(ctx, k, (size_t)cn, *cr, b + cn * bins));
        *cl = b;
        *cr = b + cn * bins;
    }
    return KPAL_OK;
}

// The host entry of linked pairs: checked, uploaded into scratch[kScratchUpload], handed to its device entry.
template <class DeviceEntry>
static int paired_host_entry(kpal_ctx *ctx, int k, int64_t N, const int64_t *const *host_left, const int64_t *const *host_right,
                             const kpal_distance_options *opt, double *out, DeviceEntry device_entry)
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
    return device_entry(ctx, k, N, dl, dr, opt, 0, out);
}
