// table_host.hpp -- the host front end the five units share that take count tables and make summaries, spectra or new tables
// (kpal_vec.hip, kpal_sets.hip, kpal_spectrum.hip, kpal_transform.hip, kpal_pool_groups.hip; included after kpal_host.hpp, host
// code only): the cap on the tables of a pass, the argument checks entries have in common, the walk over a host set in uploaded
// chunks, the upload and the download of one vector, the 16-byte form of a pool row, and what one of these units calls in another.
#pragma once
#include "stat_plan.hpp"
#include "transform_plan.hpp"

// KPAL_STAT_SET_PROFILES: a lower cap on the tables of one pass of a set entry (read on every call: tests put a pass seam into small sets).
inline uint64_t stat_set_cap()
{
    const char *e = getenv("KPAL_STAT_SET_PROFILES");
    const long long v = e ? atoll(e) : 0;
    return v > 0 ? (uint64_t)v : 0;
}

// ---- argument checks ----------------------------------------------------------------------------------------------------------
// One rung each, so that every entry keeps the ORDER of its checks (tests/test_gpu_table_arguments.py pins it with double faults);
// an entry shares a ladder of them only where its order is that one already.
inline int check_k(int k) { return k < 1 || k > KPAL_MAX_K ? set_err(KPAL_E_INVALID, "k=%d out of range", k) : KPAL_OK; }
inline int check_shrink(int k, int factor)   // k, then the factor (the reference's ValueError text)
{
    CHK(check_k(k));
    return factor < 1 || factor >= k ? set_err(KPAL_E_INVALID, "Reduction factor should be smaller than k-mer size.") : KPAL_OK;
}
inline int check_pointers(bool all_given) { return all_given ? KPAL_OK : set_err(KPAL_E_INVALID, "NULL pointer"); }
inline int check_set(bool pointers_given, size_t n_tables)   // the pointers, then the set
{
    CHK(check_pointers(pointers_given));
    return n_tables == 0 ? set_err(KPAL_E_INVALID, "empty set") : KPAL_OK;
}
inline int check_vector(size_t bins) { return bins == 0 ? set_err(KPAL_E_INVALID, "empty vector") : KPAL_OK; }
inline int check_aligned(const void *a, const void *b = nullptr) { return (uintptr_t)a % 8 || (uintptr_t)b % 8 ? set_err(KPAL_E_INVALID, "tables are not 8-byte aligned") : KPAL_OK; }
// The bytes of n_tables tables (n_tables > 0, bins > 0) do not fit a size_t: the two texts the entries have for it.
inline int too_many_bins(size_t n_tables, size_t bins) { return set_err(KPAL_E_INVALID, "%zu tables of %zu bins: too many bytes", n_tables, bins); }
inline int check_bytes_at_k(size_t n_tables, int k) { return transform_bytes_fit(n_tables, 1ULL << (2 * k)) ? KPAL_OK : set_err(KPAL_E_INVALID, "%zu tables at k=%d: too many bytes", n_tables, k); }
// A set of tables of `bins` entries each and what is written on the host for it: the ladder of the summaries and the spectra.
inline int check_counted_set(size_t n_tables, size_t bins, const int64_t *tables, const void *host_out)
{
    CHK(check_set(tables && host_out, n_tables));
    CHK(check_vector(bins));
    CHK(check_aligned(tables));
    return transform_bytes_fit(n_tables, bins) ? KPAL_OK : too_many_bins(n_tables, bins);
}
// Input against output (transform_plan.hpp): kTransformDisjoint, kTransformSame or kTransformPartial.
inline int tables_overlap(const void *in, uint64_t in_bytes, const void *out, uint64_t out_bytes) { return transform_overlap((uint64_t)(uintptr_t)in, in_bytes, (uint64_t)(uintptr_t)out, out_bytes); }

// ---- host tables, launches ----------------------------------------------------------------------------------------------------
// A host set goes through scratch[0], stat_upload_tables(bins) tables at a time: body(first, count, device tables) per chunk.
template <class Body>
static int for_uploaded_chunks(kpal_ctx *ctx, size_t n_tables, uint64_t bins, const int64_t *host_tables, Body body)
{
    for (const StatChunk &c : stat_chunks(n_tables, stat_upload_tables(bins))) {
        CHK(ensure(ctx, ctx->scratch[0], (size_t)(c.count * bins * 8)));
        HIPCHK(hipMemcpyAsync(ctx->scratch[0].p, host_tables + c.first * bins, (size_t)(c.count * bins * 8), hipMemcpyHostToDevice, ctx->stream));
        CHK(body(c.first, c.count, (const int64_t *)ctx->scratch[0].p));
    }
    return KPAL_OK;
}
// One host vector of n entries into scratch[slot] (grown to hold it), queued; n entries back to the host, waited for.
inline int upload_vector(kpal_ctx *ctx, int slot, const int64_t *host, uint64_t n, int64_t **dev)
{
    CHK(ensure(ctx, ctx->scratch[slot], (size_t)(n * 8)));
    *dev = (int64_t *)ctx->scratch[slot].p;
    HIPCHK(hipMemcpyAsync(*dev, host, (size_t)(n * 8), hipMemcpyHostToDevice, ctx->stream));
    return KPAL_OK;
}
inline int download_wait(kpal_ctx *ctx, int64_t *host, const int64_t *dev, uint64_t n)
{
    HIPCHK(hipMemcpyAsync(host, dev, (size_t)(n * 8), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return KPAL_OK;
}
// Whether a pool kernel may take the rows of `bins` entries 16 bytes at a time.
inline bool pool_rows_by_16(uint64_t bins, const void *tables, const void *out) { return bins % 2 == 0 && (uintptr_t)tables % 16 == 0 && (uintptr_t)out % 16 == 0; }
// kpal_vec.hip: the shrink of n entries by m = 4^factor.  Up to m = 64 the shuffle form runs, which reads 16 bytes at a time --
// unless the caller says the input is not aligned for that, and then the form that reads 8 bytes at a time: both entries look.
int shrink_launch(kpal_ctx *ctx, const char *name, const int64_t *in, uint64_t n, uint64_t m, int64_t *out, bool in_aligned_16);
