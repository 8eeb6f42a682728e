// kpal_vec.hip -- everything of the C-ABI that works on ONE count vector: balance, split, the reduction of (sum, count)
// partials every distance ends with, profile summaries, merge and shrink (shrink_launch serves the shrink of a set too).  (The strand balance of one vector: kpal_sets.hip.)
#include "kpal_host.hpp"
#include "table_host.hpp"

#include "vec_kernels.hpp"
#include "stat_kernels.hpp"

KPAL_API uint64_t kpal_reverse_complement(uint64_t number, int k)
{
    if (k < 1 || k > 32) return 0;
    return revcomp(number, k);
}

// out[i] = in[i] + in[rc(i)]; in == out allowed.  LDS-tiled for k >= 6, pairwise kernels below that.
// The canonical tile pairs of the LDS-tiled balance family (balance_tiled_kernel, pair_distance_balanced_kernel; k >= 6): the
// tiles M of k - 6 digits with M <= rc(M), as a device list in the order the persistent workgroups take them, and a grid that
// gives every workgroup the same number of pairs with `per_cu` workgroups on a CU.
//   ORDER (k >= 13).  A tile's 64 runs lie 4^(k-3) entries apart -- 64 pages whatever M is -- and the partner's page numbers are
// the reverse complement of M's LOW digits: with M counting up, every workgroup in flight had 64 partner pages of its own and the
// balance ran at 2.9 TB/s (k = 15) -- address translation, as in quad2_finalize_kernel.  So the sequence runs through M with the
// bits that are page bits on NEITHER side (M bits 2 md - 12 .. 11: index bits below 18 here and in the partner) fastest: tiles
// worked on at the same time share their pages on both sides.
int canon_tiles(kpal_ctx *ctx, int k, int per_cu, const uint32_t **list, uint32_t *count, unsigned *grid)
{
    const int md = k - 6;
    if (ctx->canon_k != k) {
        const uint64_t nM = 1ULL << (2 * md);
        const int lo = 2 * md - 12 > 0 ? 2 * md - 12 : 0, hi = 2 * md - 1 < 11 ? 2 * md - 1 : 11;
        const int nn = hi - lo + 1;
        auto tile_of = [&](uint64_t m) -> uint64_t {
            if (lo == 0 || nn <= 0) return m;
            return ((m & ((1ULL << nn) - 1ULL)) << lo) | ((m >> nn) & ((1ULL << lo) - 1ULL)) | ((m >> (nn + lo)) << (nn + lo));
        };
        std::vector<uint32_t> host;
        host.reserve((size_t)(nM / 2 + 1024));
        for (uint64_t m = 0; m < nM; ++m) {
            const uint64_t M = tile_of(m);
            if (md == 0 || M <= kpal_reverse_complement(M, md)) host.push_back((uint32_t)M);
        }
        CHK(ensure(ctx, ctx->canon, host.size() * sizeof(uint32_t)));
        HIPCHK(hipStreamSynchronize(ctx->stream));   // (a previous list may still be read; and `canon_host` is the copy's source)
        ctx->canon_host.swap(host);
        HIPCHK(hipMemcpyAsync(ctx->canon.p, ctx->canon_host.data(), ctx->canon_host.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));   // (once per k; the list is then read by launches on either of the context's streams)
        ctx->canon_k = k;
    }
    const uint32_t n = (uint32_t)ctx->canon_host.size();
    const uint32_t slots = (uint32_t)(ctx->num_cu * per_cu);
    const uint32_t rounds = (n + slots - 1) / slots;
    *list = (const uint32_t *)ctx->canon.p;
    *count = n;
    *grid = (n + rounds - 1) / rounds;                                  // every workgroup `rounds` pairs (the last ones one fewer)
    return KPAL_OK;
}

int launch_balance(kpal_ctx *ctx, int k, const int64_t *in, int64_t *out)
{
    const uint64_t n = 1ULL << (2 * k);
    if (k >= 6) {
        const uint32_t *canon = nullptr;
        uint32_t ncanon = 0;
        unsigned grid = 1;
        CHK(canon_tiles(ctx, k, 2, &canon, &ncanon, &grid));   // two 66 KiB workgroups per CU
        LAUNCH(ctx, "balance_tiled", balance_tiled_kernel, dim3(grid), dim3(1024), in, out, k, canon, ncanon);
    } else if (in == out) {
        LAUNCH(ctx, "balance_inplace", balance_inplace_kernel, dim3(stream_grid(ctx, n)), dim3(256), out, k, n);
    } else {
        LAUNCH(ctx, "balance_oop", balance_oop_kernel, dim3(stream_grid(ctx, n)), dim3(256), in, out, k, n);
    }
    return KPAL_OK;
}

KPAL_API int kpal_balance_device(kpal_ctx *ctx, int k, int64_t *dev_inout)
{
    CTX_ENTER(ctx);
    CHK(check_k(k));
    if (!dev_inout) return set_err(KPAL_E_INVALID, "dev_inout is NULL");
    if (ctx->counting && dev_inout == (int64_t *)ctx->table.p && k == ctx->k) return kpal_count_balance(ctx);   // (fuses with a pending finalisation)
    return launch_balance(ctx, k, dev_inout, dev_inout);
}

KPAL_API int kpal_balance(kpal_ctx *ctx, int k, int64_t *host_inout)
{
    CTX_ENTER(ctx);
    CHK(check_k(k));
    if (!host_inout) return set_err(KPAL_E_INVALID, "host_inout is NULL");
    const uint64_t n = 1ULL << (2 * k);
    int64_t *d = nullptr;
    CHK(upload_vector(ctx, 0, host_inout, n, &d));
    CHK(kpal_balance_device(ctx, k, d));
    return download_wait(ctx, host_inout, d, n);
}

KPAL_API int kpal_split(kpal_ctx *ctx, int k, const int64_t *host_counts, int64_t *host_forward,
                        int64_t *host_reverse, uint64_t *n_out)
{
    CTX_ENTER(ctx);
    CHK(check_k(k));
    CHK(check_pointers(host_counts && host_forward && host_reverse));
    const uint64_t n = 1ULL << (2 * k);
    const uint64_t pal = (k % 2 == 0) ? (1ULL << k) : 0ULL;   // 4^(k/2) palindromes for even k
    const uint64_t m = (n + pal) / 2;
    const uint32_t nseg = (uint32_t)((n + kSplitSeg - 1) / kSplitSeg);
    int64_t *dc = nullptr;
    CHK(upload_vector(ctx, 0, host_counts, n, &dc));
    CHK(ensure(ctx, ctx->scratch[1], m * 8));
    CHK(ensure(ctx, ctx->scratch[2], m * 8));
    CHK(ensure(ctx, ctx->scratch[3], (size_t)nseg * 16));
    uint32_t *dcount = (uint32_t *)ctx->scratch[3].p;
    uint64_t *doffs = (uint64_t *)((uint8_t *)ctx->scratch[3].p + (size_t)nseg * 4 + ((size_t)nseg * 4) % 8);
    LAUNCH(ctx, "split_count", split_count_kernel, dim3(nseg), dim3(256), k, n, dcount);
    std::vector<uint32_t> hc(nseg);
    HIPCHK(hipMemcpyAsync(hc.data(), dcount, (size_t)nseg * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    std::vector<uint64_t> ho(nseg);
    uint64_t run = 0;
    for (uint32_t i = 0; i < nseg; ++i) {
        ho[i] = run;
        run += hc[i];
    }
    if (run != m) return set_err(KPAL_E_HIP, "split: canonical count %llu != expected %llu", (unsigned long long)run, (unsigned long long)m);
    HIPCHK(hipMemcpyAsync(doffs, ho.data(), (size_t)nseg * 8, hipMemcpyHostToDevice, ctx->stream));
    LAUNCH(ctx, "split_write", split_write_kernel, dim3(nseg), dim3(256), (const int64_t *)dc, k, n,
           (const uint64_t *)doffs, (int64_t *)ctx->scratch[1].p, (int64_t *)ctx->scratch[2].p);
    HIPCHK(hipMemcpyAsync(host_forward, ctx->scratch[1].p, m * 8, hipMemcpyDeviceToHost, ctx->stream));
    CHK(download_wait(ctx, host_reverse, (const int64_t *)ctx->scratch[2].p, m));
    if (n_out) *n_out = m;
    return KPAL_OK;
}

// out[q] = the `nblocks` partials of group q added in a fixed order, q < nq.
int reduce_partials(kpal_ctx *ctx, const Partial *partials, uint32_t nq, uint32_t nblocks, Partial *out)
{
    LAUNCH(ctx, "reduce_partials", reduce_partials_kernel, dim3(nq), dim3(256), partials, nblocks, out);
    return KPAL_OK;
}

// Reduce `nq` groups of `nblocks` partials and fetch them.
int finish_partials(kpal_ctx *ctx, uint32_t nq, uint32_t nblocks, std::vector<Partial> &out, bool allreduce)
{
    CHK(ensure(ctx, ctx->result, (size_t)nq * sizeof(Partial)));
    CHK(reduce_partials(ctx, (const Partial *)ctx->partials.p, nq, nblocks, (Partial *)ctx->result.p));
    if (allreduce) CHK(comm_allreduce_partials(ctx, (Partial *)ctx->result.p, nq));   // bin-range shards: the sums and counts of all ranks
    out.resize(nq);
    HIPCHK(hipMemcpyAsync(out.data(), ctx->result.p, (size_t)nq * sizeof(Partial), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return KPAL_OK;
}

double finish_value(int metric, const Partial &p, int64_t *aux)
{
    if (aux) *aux = (int64_t)p.m;
    return finish_distance(metric, false, p, p, p);
}

// ----------------------------------------------------------------------------------------------
// profile summaries, merge, shrink (stat_kernels.hpp)
// ----------------------------------------------------------------------------------------------
KPAL_API int kpal_stats_device(kpal_ctx *ctx, size_t n, const int64_t *dev_counts, kpal_profile_stats *out)
{
    CTX_ENTER(ctx);
    CHK(check_pointers(dev_counts && out));
    CHK(check_vector(n));
    const unsigned grid = stream_grid(ctx, n, kStatThreads);
    CHK(ensure(ctx, ctx->partials, (size_t)grid * sizeof(StatPartial) + 256 * 8));
    StatPartial *dp = (StatPartial *)ctx->partials.p;
    LAUNCH(ctx, "stats", stats_kernel, dim3(grid), dim3(kStatThreads), dev_counts, (uint64_t)n, dp);
    std::vector<StatPartial> hp(grid);
    HIPCHK(hipMemcpyAsync(hp.data(), dp, (size_t)grid * sizeof(StatPartial), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    StatPartial t = hp[0];
    for (unsigned b = 1; b < grid; ++b) {
        const uint64_t lo = t.sum_lo + hp[b].sum_lo;
        t.sum_hi += hp[b].sum_hi + (lo < t.sum_lo ? 1 : 0);
        t.sum_lo = lo;
        t.non_zero += hp[b].non_zero;
        t.mn = std::min(t.mn, hp[b].mn);
        t.mx = std::max(t.mx, hp[b].mx);
    }
    out->total = (int64_t)t.sum_lo;
    out->non_zero = (int64_t)t.non_zero;
    out->min = t.mn;
    out->max = t.mx;
    out->mean = stat_mean(t.sum_lo, t.sum_hi, (uint64_t)n);   // the 128-bit sum as a double, magnitude first (stat_plan.hpp: the set entry's mean is this one)
    // std: sum((x - mean)^2) / n, kpal/klib.py:220-225 (ndarray.std)
    double *dv = (double *)ctx->partials.p;
    LAUNCH(ctx, "stats_var", stats_var_kernel, dim3(grid), dim3(kStatThreads), dev_counts, (uint64_t)n, out->mean, dv);
    std::vector<double> hv(grid);
    HIPCHK(hipMemcpyAsync(hv.data(), dv, (size_t)grid * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    double ss = 0.0;
    for (unsigned b = 0; b < grid; ++b) ss += hv[b];
    out->std = std::sqrt(ss / (double)n);
    // median: radix select of rank (n-1)/2 over the bytes in which min and max differ
    const uint64_t r0 = (n - 1) / 2, r1 = n / 2;
    if (t.mn == t.mx) {
        out->median = (double)t.mn;
        return KPAL_OK;
    }
    const uint64_t kmin = select_key(t.mn), kmax = select_key(t.mx);
    int top = 7;
    while (((kmin >> (8 * top)) & 255u) == ((kmax >> (8 * top)) & 255u)) --top;   // kmin != kmax: terminates at >= 0
    uint64_t mask = top == 7 ? 0ULL : ~0ULL << (8 * (top + 1));
    uint64_t prefix = kmin & mask;
    uint64_t below = 0, equal = 0;      // elements with key < / == the digits chosen so far
    unsigned long long *dh = (unsigned long long *)ctx->partials.p;
    unsigned long long hh[256];
    for (int byte = top; byte >= 0; --byte) {
        HIPCHK(hipMemsetAsync(dh, 0, 256 * 8, ctx->stream));
        LAUNCH(ctx, "select_hist", select_hist_kernel, dim3(grid), dim3(kStatThreads), dev_counts, (uint64_t)n, mask, prefix,
               8 * byte, dh);
        HIPCHK(hipMemcpyAsync(hh, dh, sizeof(hh), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        int d = 0;
        uint64_t acc = below;
        for (; d < 256; ++d) {
            if (r0 < acc + hh[d]) break;
            acc += hh[d];
        }
        if (d == 256) return set_err(KPAL_E_HIP, "median: rank %llu not found", (unsigned long long)r0);
        below = acc;
        equal = hh[d];
        prefix |= (uint64_t)d << (8 * byte);
        mask |= 255ULL << (8 * byte);
    }
    const int64_t v0 = (int64_t)(prefix ^ 0x8000000000000000ULL);
    int64_t v1 = v0;
    if (r1 >= below + equal) {   // the upper middle element is the next larger value
        LAUNCH(ctx, "select_next", select_next_kernel, dim3(grid), dim3(kStatThreads), dev_counts, (uint64_t)n, prefix, dh);
        std::vector<unsigned long long> hm(grid);
        HIPCHK(hipMemcpyAsync(hm.data(), dh, (size_t)grid * 8, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        unsigned long long m = ~0ULL;
        for (unsigned b = 0; b < grid; ++b) m = std::min(m, hm[b]);
        v1 = (int64_t)(m ^ 0x8000000000000000ULL);
    }
    out->median = ((double)v0 + (double)v1) / 2.0;   // np.median: mean of the two middle elements
    return KPAL_OK;
}

KPAL_API int kpal_stats(kpal_ctx *ctx, size_t n, const int64_t *host_counts, kpal_profile_stats *out)
{
    CTX_ENTER(ctx);
    CHK(check_pointers(host_counts && out));
    CHK(check_vector(n));
    int64_t *d = nullptr;
    CHK(upload_vector(ctx, 0, host_counts, n, &d));
    return kpal_stats_device(ctx, n, d, out);
}

static int merge_check(bool pointers_given, int merger)   // the pointers, then the merger; n == 0 is taken, after both
{
    CHK(check_pointers(pointers_given));
    return merger < KPAL_MERGE_SUM || merger > KPAL_MERGE_NINT ? set_err(KPAL_E_INVALID, "unknown merger %d", merger) : KPAL_OK;
}

KPAL_API int kpal_merge_device(kpal_ctx *ctx, size_t n, const int64_t *dev_left, const int64_t *dev_right, int merger,
                               int64_t *dev_out)
{
    CTX_ENTER(ctx);
    CHK(merge_check(dev_left && dev_right && dev_out, merger));
    if (n == 0) return KPAL_OK;
    const unsigned grid = stream_grid(ctx, n);
    switch (merger) {
    case KPAL_MERGE_SUM: LAUNCH(ctx, "merge", (merge_kernel<0>), dim3(grid), dim3(256), dev_left, dev_right, (uint64_t)n, dev_out); break;
    case KPAL_MERGE_XOR: LAUNCH(ctx, "merge", (merge_kernel<1>), dim3(grid), dim3(256), dev_left, dev_right, (uint64_t)n, dev_out); break;
    case KPAL_MERGE_INT: LAUNCH(ctx, "merge", (merge_kernel<2>), dim3(grid), dim3(256), dev_left, dev_right, (uint64_t)n, dev_out); break;
    default: LAUNCH(ctx, "merge", (merge_kernel<3>), dim3(grid), dim3(256), dev_left, dev_right, (uint64_t)n, dev_out); break;
    }
    return KPAL_OK;
}

KPAL_API int kpal_merge(kpal_ctx *ctx, size_t n, const int64_t *host_left, const int64_t *host_right, int merger,
                        int64_t *host_out)
{
    CTX_ENTER(ctx);
    CHK(merge_check(host_left && host_right && host_out, merger));
    if (n == 0) return KPAL_OK;
    int64_t *dl = nullptr, *dr = nullptr;
    CHK(upload_vector(ctx, 0, host_left, n, &dl));
    CHK(upload_vector(ctx, 1, host_right, n, &dr));
    CHK(kpal_merge_device(ctx, n, dl, dr, merger, dl));
    return download_wait(ctx, host_out, dl, n);
}

int shrink_launch(kpal_ctx *ctx, const char *name, const int64_t *in, uint64_t n, uint64_t m, int64_t *out, bool in_aligned_16)
{
    if (m <= 64 && in_aligned_16) LAUNCH(ctx, name, shrink_small_kernel, dim3(stream_grid(ctx, n / 2)), dim3(256), in, n / 2, (int)(m / 2), out);
    else LAUNCH(ctx, name, shrink_large_kernel, dim3(stream_grid(ctx, n / m * 64)), dim3(256), in, n / m, m, out);
    return KPAL_OK;
}

KPAL_API int kpal_shrink_device(kpal_ctx *ctx, int k, int factor, const int64_t *dev_counts, int64_t *dev_out)
{
    CTX_ENTER(ctx);
    CHK(check_shrink(k, factor));
    CHK(check_pointers(dev_counts && dev_out));
    return shrink_launch(ctx, "shrink", dev_counts, 1ULL << (2 * k), 1ULL << (2 * factor), dev_out, (uintptr_t)dev_counts % 16 == 0);
}

KPAL_API int kpal_shrink(kpal_ctx *ctx, int k, int factor, const int64_t *host_counts, int64_t *host_out)
{
    CTX_ENTER(ctx);
    CHK(check_shrink(k, factor));
    CHK(check_pointers(host_counts && host_out));
    const uint64_t n = 1ULL << (2 * k), n_out = n >> (2 * factor);
    int64_t *d = nullptr;
    CHK(upload_vector(ctx, 0, host_counts, n, &d));
    CHK(ensure(ctx, ctx->scratch[1], n_out * 8));
    CHK(kpal_shrink_device(ctx, k, factor, d, (int64_t *)ctx->scratch[1].p));
    return download_wait(ctx, host_out, (const int64_t *)ctx->scratch[1].p, n_out);
}
