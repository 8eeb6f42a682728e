// kpal_spectrum.hip -- the count-of-counts spectrum (metrics.distribution, kpal/metrics.py:22-33) of every table of a SET of
// count vectors lying one behind the other, in a number of launches that does not grow with the set (planned by
// spectrum_plan.hpp, the kernels in spectrum_kernels.hpp).  One table is a set of one: there is no other implementation.  The
// result is ragged, so the entries are a begin / fetch pair: the pairs stay with the context.
#include "kpal_host.hpp"
#include "table_host.hpp"

#include "stat_set_kernels.hpp"
#include "spectrum_kernels.hpp"

// The spectra of `count` consecutive tables, appended to the context's pairs; offsets[t + 1] = where table t's pairs end.
// 6 launches (7 if any entry lies past its table's window), 3 synchronisations.
static int spectrum_pass(kpal_ctx *ctx, uint64_t count, uint64_t bins, const int64_t *dev_tables, uint64_t *offsets)
{
    const uint64_t slices = stat_slices(bins);
    // what does not depend on the window: partials, ranges, overflow counts, two words
    const uint64_t partial_bytes = count * slices * kStatPartialBytes, range_bytes = count * kSpectrumRangeBytes, over_bytes = count * 8;
    const uint64_t fixed_bytes = partial_bytes + range_bytes + over_bytes + 16;
    CHK(ensure(ctx, ctx->partials, (size_t)(count * spectrum_scratch_bytes(bins, spectrum_window(UINT64_MAX, bins)) + 32)));
    uint8_t *base = (uint8_t *)ctx->partials.p;
    StatPartial *partial = (StatPartial *)base;
    SpectrumRange *range = (SpectrumRange *)(base + partial_bytes);
    unsigned long long *overflow = (unsigned long long *)(base + partial_bytes + range_bytes);
    unsigned long long *widest = overflow + count, *cursor = widest + 1;
    HIPCHK(hipMemsetAsync(overflow, 0, (size_t)(over_bytes + 16), ctx->stream));   // ... the two words with them
    const dim3 grid((unsigned)slices, (unsigned)count), block(kStatSetThreads);
    LAUNCH(ctx, "stats_set", stats_set_kernel, grid, block, dev_tables, bins, partial);
    LAUNCH(ctx, "spectrum_range", spectrum_range_kernel, dim3((unsigned)count), block, (const StatPartial *)partial, (uint32_t)slices, range, widest);
    unsigned long long wide = 0;
    HIPCHK(hipMemcpyAsync(&wide, widest, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // the first decision of the host: the window of the pass

    const uint64_t window = spectrum_window(wide, bins), wslices = spectrum_window_slices(window), m = count * wslices;
    unsigned long long *windows = (unsigned long long *)(base + fixed_bytes);
    unsigned long long *nz = windows + count * window;   // m + 1 words
    HIPCHK(hipMemsetAsync(windows, 0, (size_t)(count * window * 8), ctx->stream));
    const dim3 wgrid((unsigned)wslices, (unsigned)count);
    LAUNCH(ctx, "spectrum_hist", spectrum_hist_kernel, grid, block, dev_tables, bins, (const SpectrumRange *)range, window, windows, overflow);
    LAUNCH(ctx, "spectrum_nonzero", spectrum_nonzero_kernel, wgrid, block, (const unsigned long long *)windows, window, nz);
    LAUNCH(ctx, "spectrum_scan", spectrum_scan_kernel, dim3(1), dim3(kSpectrumScanThreads), nz, m);
    std::vector<unsigned long long> scanned((size_t)m + 1), over((size_t)count);
    HIPCHK(hipMemcpyAsync(scanned.data(), nz, (size_t)((m + 1) * 8), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(over.data(), overflow, (size_t)over_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // the second: how many pairs the windows hold, how many entries lie past them

    const uint64_t in_window = scanned[(size_t)m];
    uint64_t past = 0;
    for (uint64_t t = 0; t < count; ++t) past += over[(size_t)t];
    if (in_window > count * window || past > count * bins) return set_err(KPAL_E_HIP, "distribution of a set: %llu pairs, %llu past the window", (unsigned long long)in_window, (unsigned long long)past);
    std::vector<int64_t> wvalues((size_t)in_window);
    std::vector<uint64_t> wnumbers((size_t)in_window);
    std::vector<SpectrumOverflow> list((size_t)past);
    if (in_window) {
        CHK(ensure(ctx, ctx->scratch[1], (size_t)(in_window * 16)));
        int64_t *dvalues = (int64_t *)ctx->scratch[1].p;
        unsigned long long *dnumbers = (unsigned long long *)(dvalues + in_window);
        LAUNCH(ctx, "spectrum_compact", spectrum_compact_kernel, wgrid, block, (const unsigned long long *)windows, window, (const SpectrumRange *)range,
               (const unsigned long long *)nz, dvalues, dnumbers);
        HIPCHK(hipMemcpyAsync(wvalues.data(), dvalues, (size_t)(in_window * 8), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(wnumbers.data(), dnumbers, (size_t)(in_window * 8), hipMemcpyDeviceToHost, ctx->stream));
    }
    unsigned long long appended = 0;
    if (past) {
        CHK(ensure(ctx, ctx->scratch[2], (size_t)(past * kSpectrumOverflowBytes)));
        SpectrumOverflow *dlist = (SpectrumOverflow *)ctx->scratch[2].p;
        LAUNCH(ctx, "spectrum_overflow", spectrum_overflow_kernel, grid, block, dev_tables, bins, (const SpectrumRange *)range, window,
               (const unsigned long long *)overflow, cursor, dlist, past);
        HIPCHK(hipMemcpyAsync(list.data(), dlist, (size_t)(past * kSpectrumOverflowBytes), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(&appended, cursor, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (appended != past) return set_err(KPAL_E_HIP, "distribution of a set: %llu entries past the window, %llu listed", (unsigned long long)past, appended);

    // the entries past the windows: sorted by table and key, runs of one key counted.  Every key of them lies above its table's
    // window, so a table's pairs are those of its window and then these.
    std::sort(list.begin(), list.end(), [](const SpectrumOverflow &a, const SpectrumOverflow &b) { return a.table != b.table ? a.table < b.table : a.key < b.key; });
    size_t at = 0;
    for (uint64_t t = 0; t < count; ++t) {
        const size_t w0 = (size_t)scanned[(size_t)(t * wslices)], w1 = (size_t)scanned[(size_t)((t + 1) * wslices)];
        ctx->spec_values.insert(ctx->spec_values.end(), wvalues.begin() + w0, wvalues.begin() + w1);
        ctx->spec_numbers.insert(ctx->spec_numbers.end(), wnumbers.begin() + w0, wnumbers.begin() + w1);
        while (at < list.size() && list[at].table == t) {
            size_t run = at + 1;
            while (run < list.size() && list[run].table == t && list[run].key == list[at].key) ++run;
            ctx->spec_values.push_back(spectrum_value(list[at].key));
            ctx->spec_numbers.push_back((uint64_t)(run - at));
            at = run;
        }
        offsets[t + 1] = (uint64_t)ctx->spec_values.size();
    }
    if (at != list.size()) return set_err(KPAL_E_HIP, "distribution of a set: an entry past the window names table %llu of %llu", (unsigned long long)list[at].table, (unsigned long long)count);
    return KPAL_OK;
}

static void spectrum_reset(kpal_ctx *ctx)
{
    ctx->spec_pending = false;
    ctx->spec_values.clear();
    ctx->spec_numbers.clear();
}

// The passes of a set whose first table is table `first` of the call: offsets[first] is set already.
static int spectrum_device(kpal_ctx *ctx, size_t n_tables, size_t bins, const int64_t *dev_tables, uint64_t *offsets)
{
    const uint64_t per = spectrum_tables_per_pass(bins, kStatSetBudgetBytes, stat_set_cap());
    for (const StatChunk &c : stat_chunks(n_tables, per))
        CHK(spectrum_pass(ctx, c.count, bins, dev_tables + c.first * (uint64_t)bins, offsets + c.first));
    return KPAL_OK;
}

// What the two entries do around their passes: the pairs of the call before are dropped first, even by a call that is refused.
template <class Passes>
static int spectrum_entry(kpal_ctx *ctx, size_t n_tables, size_t bins, const int64_t *tables, uint64_t *host_offsets, Passes passes)
{
    CTX_ENTER(ctx);
    spectrum_reset(ctx);
    CHK(check_counted_set(n_tables, bins, tables, host_offsets));
    host_offsets[0] = 0;
    try {
        CHK(passes());
    } catch (const std::bad_alloc &) {
        spectrum_reset(ctx);
        return set_err(KPAL_E_NOMEM, "distribution of a set: out of host memory");
    }
    ctx->spec_pending = true;
    return KPAL_OK;
}

KPAL_API int kpal_distribution_set_device(kpal_ctx *ctx, size_t n_tables, size_t bins, const int64_t *dev_tables, uint64_t *host_offsets)
{
    return spectrum_entry(ctx, n_tables, bins, dev_tables, host_offsets, [&] { return spectrum_device(ctx, n_tables, bins, dev_tables, host_offsets); });
}

KPAL_API int kpal_distribution_set(kpal_ctx *ctx, size_t n_tables, size_t bins, const int64_t *host_tables, uint64_t *host_offsets)
{
    return spectrum_entry(ctx, n_tables, bins, host_tables, host_offsets, [&] {
        return for_uploaded_chunks(ctx, n_tables, bins, host_tables, [&](uint64_t first, uint64_t count, const int64_t *dev) {
            return spectrum_device(ctx, (size_t)count, bins, dev, host_offsets + first);
        });
    });
}

KPAL_API int kpal_distribution_fetch(kpal_ctx *ctx, uint64_t first_pair, uint64_t n_pairs, int64_t *host_values, uint64_t *host_numbers)
{
    if (!ctx) return set_err(KPAL_E_INVALID, "ctx is NULL");
    if (!ctx->spec_pending) return set_err(KPAL_E_INVALID, "no distribution pending");
    const uint64_t have = (uint64_t)ctx->spec_values.size();
    if (first_pair > have || n_pairs > have - first_pair)
        return set_err(KPAL_E_INVALID, "pairs %llu .. +%llu of %llu", (unsigned long long)first_pair, (unsigned long long)n_pairs, (unsigned long long)have);
    if (n_pairs && (!host_values || !host_numbers)) return set_err(KPAL_E_INVALID, "NULL pointer");
    if (n_pairs) {
        memcpy(host_values, ctx->spec_values.data() + first_pair, (size_t)n_pairs * 8);
        memcpy(host_numbers, ctx->spec_numbers.data() + first_pair, (size_t)n_pairs * 8);
    }
    return KPAL_OK;
}
