// kpal_count.hip -- the counting front end of the C-ABI (begin / feed / feed_device / feed_pinned / finish / balance), the
// pieces of a feed (count_device_range; the strategy and size of a piece: count_plan.hpp), H2D staging, and the launchers of
// the LDS-direct, global-atomic and round-1 partition pipelines.  The quad record pipelines live in kpal_quads.hip /
// kpal_quads2.hip, the FASTA / FASTQ ingests in kpal_text.hip, the per-record and per-window profiles in kpal_records.hip.
#include "kpal_host.hpp"

#include "count_kernels.hpp"
#include "count_plan.hpp"
#include "partition_kernels.hpp"
#include "chunk_kernels.hpp"
#include "fasta_host.hpp"

#include <sys/syscall.h>
#include <unistd.h>

static_assert(sizeof(ChunkPool) <= sizeof(kpal_ctx::chunk_pool_sent), "kpal_ctx::chunk_pool_sent holds a ChunkPool");

// ----------------------------------------------------------------------------------------------
// counting
// ----------------------------------------------------------------------------------------------
KPAL_API int kpal_count_begin(kpal_ctx *ctx, int k)
{
    CTX_ENTER(ctx);
    if (k < 1 || k > KPAL_MAX_K) return set_err(KPAL_E_INVALID, "k=%d out of range 1..%d", k, KPAL_MAX_K);
    if (ctx->merged && (ctx->merged_bins != (1ULL << (2 * k)) || ctx->merged == ctx->table.p)) {
        // another k, or the merged table WAS the count table (serial reduce) which is about to be zeroed / reallocated
        ctx->merged = nullptr;
        ctx->merged_bins = 0;
    }
    ctx->k = k;
    ctx->bins = 1ULL << (2 * k);
    CHK(ensure(ctx, ctx->table, ctx->bins * sizeof(int64_t)));
    // k >= 13: the zeroing of the table (8.6 GB at k = 15) is deferred -- a first piece on the two-level quad pipeline writes the whole
    // table in its finalisation and never needs it (kpal_quads2.hip, FRESH); whatever else touches the table first zeroes it (table_ready)
    static const bool allow_fresh = [] { const char *e = getenv("KPAL_FRESH"); return !e || atoi(e) != 0; }();
    ctx->table_zero_pending = allow_fresh && k >= 13 && (ctx->strategy == KPAL_STRATEGY_AUTO || ctx->strategy == KPAL_STRATEGY_PARTITION2_QUADS);
    if (!ctx->table_zero_pending) HIPCHK(hipMemsetAsync(ctx->table.p, 0, ctx->bins * sizeof(int64_t), ctx->stream));
    if (ctx->chunk_error_word) HIPCHK(hipMemsetAsync(ctx->chunk_error_word, 0, sizeof(uint32_t), ctx->stream));
    if (ctx->quad_error_word) HIPCHK(hipMemsetAsync(ctx->quad_error_word, 0, sizeof(uint32_t), ctx->stream));
    ctx->chunk_error_armed = false;
    ctx->fin.clear();                       // (staged forms of an abandoned count)
    ctx->tiles.clear();                     // (tile sizes and verdict of a sample of THIS count only)
    ctx->plan_strategy = ctx->plan_steps1 = ctx->plan_steps2 = 0;
    fq_reset(ctx);                          // (the unfinished FASTQ record of an abandoned count)
    ctx->counting = true;
    return KPAL_OK;
}

KPAL_API int kpal_count_set_strategy(kpal_ctx *ctx, int strategy)
{
    if (!ctx) return set_err(KPAL_E_INVALID, "ctx is NULL");
    if (strategy < KPAL_STRATEGY_AUTO || strategy > KPAL_STRATEGY_PARTITION2_QUADS)
        return set_err(KPAL_E_INVALID, "unknown strategy %d", strategy);
    ctx->strategy = strategy;
    return KPAL_OK;
}

constexpr PlanLimits kPlanLimits = {kChunkIdBits, kChunkKeys, kNumBuckets, kStepsPerBlockQuantum};

static int resolve_strategy(int requested, int k, int *out)
{
    const int s = plan_resolve(requested, k);
    if (s == kPlanNeedsLdsK) return set_err(KPAL_E_INVALID, "LDS-direct strategy needs k <= 7 (k=%d)", k);
    if (s == kPlanNeedsOneLevelK) return set_err(KPAL_E_INVALID, "partition strategy needs 8 <= k <= 12 (k=%d)", k);
    if (s == kPlanNeedsTwoLevelK) return set_err(KPAL_E_INVALID, "two-level partition strategy needs 13 <= k <= 16 (k=%d)", k);
    *out = s;
    return KPAL_OK;
}

// Span for emitting the k-mers that end in [addr, addr+n), with `halo` readable bytes of the
// same feed to the left of addr.
Span make_span(const uint8_t *addr, size_t n, size_t halo)
{
    const uintptr_t first = (uintptr_t)addr - halo;
    const uintptr_t base = first & ~(uintptr_t)15;
    Span s;
    s.base = reinterpret_cast<const uint4 *>(base);
    s.lo = first - base;
    s.emit_from = s.lo + halo;
    s.hi = s.emit_from + n;
    s.nchunks = (s.hi + 15) / 16;
    return s;
}

static int launch_global_atomic(kpal_ctx *ctx, const Span &s)
{
    const WaveGrid w = wave_grid((s.nchunks + 63) / 64, ctx->num_cu, 8, 4);   // 8 blocks of 4 waves per CU
    unsigned long long *table = (unsigned long long *)ctx->table.p;
    DISPATCH_K_1_16(ctx->k, LAUNCH(ctx, "count_global_atomic", (count_global_atomic_kernel<K>), dim3(w.grid), dim3(256), s, w.spw, table));
    return KPAL_OK;
}

static int launch_lds_direct(kpal_ctx *ctx, const Span &s)
{
    const WaveGrid w = wave_grid((s.nchunks + 63) / 64, ctx->num_cu, 2, 8);   // 2 blocks of 8 waves per CU
    unsigned long long *table = (unsigned long long *)ctx->table.p;
    DISPATCH_K_1_7(ctx->k, LAUNCH(ctx, "count_lds_direct", (count_lds_direct_kernel<K>), dim3(w.grid), dim3(512), s, w.spw, table));
    return KPAL_OK;
}

// One-level partition, k = 8..12 (partition_kernels.hpp: A1, A2, A3, B).
static int launch_partition(kpal_ctx *ctx, const Span &s)
{
    const uint64_t total_steps = (s.nchunks + 63) / 64;
    if (total_steps == 0) return KPAL_OK;
    // steps per block: a multiple of 24 (8 waves x 3 steps per tile), ~4 blocks per CU
    const uint64_t want_blocks = (uint64_t)ctx->num_cu * 4;
    uint64_t spb = (total_steps + want_blocks - 1) / want_blocks;
    spb = (spb + kStepsPerBlockQuantum - 1) / kStepsPerBlockQuantum * kStepsPerBlockQuantum;
    const uint32_t G = (uint32_t)((total_steps + spb - 1) / spb);
    const uint64_t max_keys = s.nchunks * 16;
    CHK(ensure(ctx, ctx->keys, max_keys * sizeof(uint16_t) + 64));
    CHK(ensure(ctx, ctx->cntmat, (size_t)kNumBuckets * G * sizeof(uint32_t)));
    CHK(ensure(ctx, ctx->offs, (size_t)kNumBuckets * G * sizeof(uint32_t)));
    CHK(ensure(ctx, ctx->bucket_start, (size_t)(2 * kNumBuckets + 2) * sizeof(uint64_t)));
    CHK(ensure(ctx, ctx->slice_start, (size_t)(kNumBuckets + 1) * sizeof(uint32_t)));
    uint32_t *cntmat = (uint32_t *)ctx->cntmat.p;
    uint32_t *offs = (uint32_t *)ctx->offs.p;
    uint64_t *bstart = (uint64_t *)ctx->bucket_start.p;
    uint64_t *btotal = bstart + kNumBuckets + 1;
    uint32_t *sstart = (uint32_t *)ctx->slice_start.p;
    uint16_t *keys = (uint16_t *)ctx->keys.p;
    unsigned long long *table = (unsigned long long *)ctx->table.p;
    const uint64_t *no_base = nullptr;
    DISPATCH_K_8_12(ctx->k, {
        LAUNCH(ctx, "part_count", (part_count_kernel<K>), dim3(G), dim3(kScatterThreads), s, spb, cntmat);
        LAUNCH(ctx, "part_rowscan", part_rowscan_kernel, dim3(kNumBuckets), dim3(256), (const uint32_t *)cntmat, G, offs, btotal);
        LAUNCH(ctx, "part_bucketscan", part_bucketscan_kernel, dim3(1), dim3(kNumBuckets), (const uint64_t *)btotal,
               (uint32_t)kNumBuckets, no_base, bstart, sstart);
        LAUNCH(ctx, "part_scatter", (part_scatter_kernel<K>), dim3(G), dim3(kScatterThreads), s, spb,
               (const uint32_t *)offs, (const uint64_t *)bstart, keys);
        // one workgroup per bucket (exclusive table slice -> plain read-modify-write merge, measured
        // fastest); oversized buckets of skewed input are cut into slices by the bucket scan
        LAUNCH(ctx, "part_hist", (part_hist_kernel<PartCfg<K>::kKeyBits>), dim3(kHistGridX), dim3(1024),
               (const uint16_t *)keys, (const uint64_t *)bstart, (const uint32_t *)sstart, table);
    });
    return KPAL_OK;
}

// Workspace of one chunked scatter + histogram over Y coarse buckets (Y = 1: one-level path):
// pool of 8 KiB key chunks, table rows, overflow lists, per-coarse-bucket meta words and the device
// copy of the pool descriptor.  meta words per coarse bucket y: nlist[512] ovf_n[512] (all y first,
// so one memset clears them), then ovf_count[Y] error, then ostart[Y][513] ocur[Y][512]
// slice_start[Y][513], then the descriptor.
struct ChunkLaunch {
    ChunkPool p;
    ChunkPool *dpool;
    uint32_t *ostart, *ocur, *sstart;
    uint32_t Y;
};

static int chunk_prepare(kpal_ctx *ctx, uint32_t Y, uint32_t G, uint64_t R, ChunkLaunch &cl)
{
    const uint64_t per_y = (uint64_t)G * R;
    if (per_y >= (1ull << kChunkIdBits)) return set_err(KPAL_E_INVALID, "chunked partition: batch too large");
    const uint64_t cap = per_y * Y;
    CHK(ensure(ctx, ctx->keys, cap * kChunkKeys * sizeof(uint16_t)));
    CHK(ensure(ctx, ctx->chunk_table, (size_t)Y * kNumBuckets * G * kChunkRow * sizeof(uint32_t)));
    CHK(ensure(ctx, ctx->chunk_ovf, cap * sizeof(uint2)));
    CHK(ensure(ctx, ctx->chunk_sorted, cap * sizeof(uint32_t)));
    const size_t clear_words = (size_t)Y * 2 * kNumBuckets + Y;   // nlist, ovf_n, ovf_count
    const size_t pool_words = (sizeof(ChunkPool) + 3) / 4 + 8;
    const size_t meta_words = clear_words + 1 + (size_t)Y * (2 * (kNumBuckets + 1) + kNumBuckets) + 4 + pool_words;
    const bool fresh = ctx->chunk_meta.cap < meta_words * sizeof(uint32_t);
    CHK(ensure(ctx, ctx->chunk_meta, meta_words * sizeof(uint32_t)));
    uint32_t *meta = (uint32_t *)ctx->chunk_meta.p;
    if (fresh || Y != ctx->chunk_meta_y) {
        HIPCHK(hipMemsetAsync(meta, 0, meta_words * sizeof(uint32_t), ctx->stream));
        ctx->chunk_meta_y = Y;
        ctx->chunk_pool_dev = nullptr;
    }
    ChunkPool &p = cl.p;
    memset(&p, 0, sizeof(p));   // padding too: the descriptor is compared bytewise below
    p.keys = (uint16_t *)ctx->keys.p;
    p.per_block = (uint32_t)R;
    p.groups = G;
    p.table = (uint32_t *)ctx->chunk_table.p;
    p.nlist = meta;
    p.ovf_n = meta + (size_t)Y * kNumBuckets;
    p.ovf_count = meta + (size_t)Y * 2 * kNumBuckets;
    p.error = meta + clear_words;
    p.ovf = (uint2 *)ctx->chunk_ovf.p;
    cl.ostart = meta + clear_words + 1;
    cl.ocur = cl.ostart + (size_t)Y * (kNumBuckets + 1);
    cl.sstart = cl.ocur + (size_t)Y * kNumBuckets;
    cl.dpool = (ChunkPool *)(((uintptr_t)(cl.sstart + (size_t)Y * (kNumBuckets + 1)) + 15) & ~(uintptr_t)15);
    cl.Y = Y;
    ctx->chunk_error_word = p.error;
    // the device copy changes only when a buffer was reallocated or the geometry changed: a
    // synchronous copy then -- an asynchronous one would read this stack frame after it is gone
    if (memcmp(&p, ctx->chunk_pool_sent, sizeof(ChunkPool)) != 0 || (void *)cl.dpool != ctx->chunk_pool_dev) {
        HIPCHK(hipStreamSynchronize(ctx->stream));
        HIPCHK(hipMemcpy(cl.dpool, &p, sizeof(ChunkPool), hipMemcpyHostToDevice));
        memcpy(ctx->chunk_pool_sent, &p, sizeof(ChunkPool));
        ctx->chunk_pool_dev = cl.dpool;
    }
    ctx->chunk_error_armed = true;
    // per batch: counts restart at 0; the error word is sticky until count_finish
    HIPCHK(hipMemsetAsync(meta, 0, clear_words * sizeof(uint32_t), ctx->stream));
    return KPAL_OK;
}

// The kernels after the scatter: slice plan, overflow grouping, histogram + merge.
template <int KB>
static int chunk_histogram(kpal_ctx *ctx, const ChunkLaunch &cl)
{
    unsigned long long *table = (unsigned long long *)ctx->table.p;
    LAUNCH(ctx, "chunk_plan", chunk_plan_kernel, dim3(cl.Y), dim3(kNumBuckets), (const uint32_t *)cl.p.nlist,
           (const uint32_t *)cl.p.ovf_n, cl.ostart, cl.ocur, cl.sstart);
    LAUNCH(ctx, "chunk_list", chunk_list_kernel, dim3(64, cl.Y), dim3(256), cl.p, (const uint32_t *)cl.ostart, cl.ocur,
           (uint32_t *)ctx->chunk_sorted.p);
    LAUNCH(ctx, "chunk_hist", (chunk_hist_kernel<KB>), dim3(kHistGridX, cl.Y), dim3(1024), cl.p, (const uint32_t *)cl.ostart,
           (const uint32_t *)ctx->chunk_sorted.p, (const uint32_t *)cl.sstart, table);
    return KPAL_OK;
}

// Chunked one-level partition, k = 8..12 (chunk_kernels.hpp): scatter into per-workgroup 8 KiB
// chunks, record them in (bucket, workgroup) table rows, histogram every bucket's chunks.
static int launch_partition_chunked(kpal_ctx *ctx, const Span &s)
{
    const uint64_t total_steps = (s.nchunks + 63) / 64;
    if (total_steps == 0) return KPAL_OK;
    // one round of two resident workgroups per CU: every workgroup leaves a partly filled and an
    // unused chunk per bucket behind, so fewer, longer workgroups than the exact-offset path
    const uint64_t want_blocks = (uint64_t)ctx->num_cu * 2;
    uint64_t spb = (total_steps + want_blocks - 1) / want_blocks;
    spb = (spb + kStepsPerBlockQuantum - 1) / kStepsPerBlockQuantum * kStepsPerBlockQuantum;
    const uint32_t G = (uint32_t)((total_steps + spb - 1) / spb);
    // chunks per workgroup, worst case: spb*1024/4096 full ones + a partly filled and a
    // pre-assigned next one per bucket (+ slack)
    // (the stride of the ranges is harmless except at exact powers of two: R = 2048 -> 16 MiB costs 10 %)
    const uint64_t R = spb * 1024 / kChunkKeys + 2 * kNumBuckets + 64;
    ChunkLaunch cl;
    CHK(chunk_prepare(ctx, 1, G, R, cl));
    unsigned long long *table = (unsigned long long *)ctx->table.p;
    DISPATCH_K_8_12(ctx->k, {
        LAUNCH(ctx, "chunk_scatter", (chunk_scatter_kernel<K>), dim3(G), dim3(kScatterThreads), s, spb, (const ChunkPool *)cl.dpool,
               cl.p.keys, cl.p.per_block, table);
        CHK(chunk_histogram<PartCfg<K>::kKeyBits>(ctx, cl));
    });
    return KPAL_OK;
}



// Two-level partition, k = 13..16: coarse count/scan/scatter into 24-bit residuals, then the
// one-level pipeline on every coarse bucket's residual stream (2-D launches over coarse buckets).
static int launch_partition2(kpal_ctx *ctx, const Span &s)
{
    const uint64_t total_steps = (s.nchunks + 63) / 64;
    if (total_steps == 0) return KPAL_OK;
    const int NB1 = 1 << (2 * ctx->k - kResidualBits);
    const uint64_t want_blocks = (uint64_t)ctx->num_cu * 8;   // measured: coarse_count 8 % faster than with 4 per CU, coarse_scatter indifferent
    uint64_t spb = (total_steps + want_blocks - 1) / want_blocks;
    spb = (spb + 7) / 8 * 8;   // 8 waves, one step per wave per tile
    const uint32_t G1 = (uint32_t)((total_steps + spb - 1) / spb);
    const uint64_t max_keys = s.nchunks * 16;
    if (ensure(ctx, ctx->residuals, max_keys * sizeof(uint32_t) + 64) != KPAL_OK ||
        (ctx->level2_mode == 0 && ensure(ctx, ctx->keys, max_keys * sizeof(uint16_t) + 64) != KPAL_OK)) {
        if (max_keys <= ((uint64_t)1 << 30)) return KPAL_E_NOMEM;
        return kSplitBatch;   // not enough HBM for a batch of this size: retry with half
    }
    CHK(ensure(ctx, ctx->cnt1, (size_t)NB1 * G1 * sizeof(uint32_t)));
    CHK(ensure(ctx, ctx->offs1, (size_t)NB1 * G1 * sizeof(uint32_t)));
    CHK(ensure(ctx, ctx->start1, (size_t)(2 * NB1 + 2) * sizeof(uint64_t)));
    uint32_t *res = (uint32_t *)ctx->residuals.p;
    uint32_t *cnt1 = (uint32_t *)ctx->cnt1.p;
    uint32_t *offs1 = (uint32_t *)ctx->offs1.p;
    uint64_t *start1 = (uint64_t *)ctx->start1.p;
    uint64_t *total1 = start1 + NB1 + 1;
    uint16_t *keys = (uint16_t *)ctx->keys.p;
    unsigned long long *table = (unsigned long long *)ctx->table.p;
    const uint64_t *no_base = nullptr;
    DISPATCH_K_13_16(ctx->k, {
        LAUNCH(ctx, "coarse_count", (coarse_count_kernel<K>), dim3(G1), dim3(kCoarseThreads), s, spb, cnt1);
        LAUNCH(ctx, "part_rowscan", part_rowscan_kernel, dim3(NB1), dim3(256), (const uint32_t *)cnt1, G1, offs1, total1);
        LAUNCH(ctx, "part_bucketscan", part_bucketscan_kernel, dim3(1), dim3(kNumBuckets), (const uint64_t *)total1,
               (uint32_t)NB1, no_base, start1, (uint32_t *)nullptr);
    });
    // coarse bucket sizes: they size the level-2 launches and guard the 32-bit in-bucket offsets
    // (one small D2H + sync per batch)
    std::vector<uint64_t> h1((size_t)NB1 + 1);
    HIPCHK(hipMemcpyAsync(h1.data(), start1, h1.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    uint64_t maxn = 0;
    for (int c = 0; c < NB1; ++c) maxn = std::max(maxn, h1[c + 1] - h1[c]);
    if (maxn == 0) return KPAL_OK;
    if (maxn > ctx->split_above && s.nchunks > 64) return kSplitBatch;   // skewed batch: the caller halves it
    DISPATCH_K_13_16(ctx->k, {
        LAUNCH(ctx, "coarse_scatter", (coarse_scatter_kernel<K>), dim3(G1), dim3(kCoarseThreads), s, spb,
               (const uint32_t *)offs1, (const uint64_t *)start1, res);
    });
    if (ctx->level2_mode != 0) {
        // level 2 as a chunked scatter (chunk_kernels.hpp): no counting pass over the residuals.
        // Two resident workgroups per CU in total; every workgroup leaves ~1000 unused 8 KiB chunks.
        const bool lines = ctx->level2_mode == 2;   // aligned-line staging: one 1024-thread workgroup per CU
        // workgroups per coarse bucket: 8 per CU in total when the coarse buckets are equal (fewer, longer
        // workgroups are 6 % faster); unequal buckets (AT-rich input) leave most workgroups of the small
        // ones empty, so the granularity is doubled (AT-rich 1 GiB: 3.1 -> 2.2 ms)
        const uint64_t total1 = h1[NB1] - h1[0];
        const bool unequal = (double)maxn * NB1 > 1.25 * (double)total1;
        uint64_t g2t = std::max<uint64_t>(2, (uint64_t)ctx->num_cu * (lines ? (unequal ? 16 : 8) : 2) / NB1);
        g2t = std::min<uint64_t>(g2t, std::max<uint64_t>(2, 4096 / NB1));   // every workgroup reserves ~1000 chunks (9 MB) of pool address space
        const uint64_t quantum = lines ? (uint64_t)kKeysPerBlockQuantum : (uint64_t)kScatterWaves * kScatterSteps * kMacroKeys;
        uint64_t kpb2 = 0, R2 = 0;
        uint32_t G2c = 0;
        for (;; g2t = (g2t + 1) / 2) {   // few coarse buckets (k = 13): keep a coarse bucket's chunk ids below 2^20
            kpb2 = (maxn + g2t - 1) / g2t;
            kpb2 = (kpb2 + quantum - 1) / quantum * quantum;
            if (kpb2 > 0xFFFFFFFFull) return set_err(KPAL_E_INVALID, "two-level partition: batch too large");
            G2c = (uint32_t)((maxn + kpb2 - 1) / kpb2);
            R2 = kpb2 / kChunkKeys + 2 * kNumBuckets + 64;
            if ((uint64_t)G2c * R2 < (1ull << kChunkIdBits) || g2t <= 2) break;
        }
        if ((uint64_t)G2c * R2 >= (1ull << kChunkIdBits) && max_keys > ((uint64_t)1 << 30)) return kSplitBatch;   // one coarse bucket holds (almost) everything
        ChunkLaunch cl;
        const int rc = chunk_prepare(ctx, (uint32_t)NB1, G2c, R2, cl);
        if (rc == KPAL_E_NOMEM && max_keys > ((uint64_t)1 << 30)) return kSplitBatch;   // retry with half the batch
        if (rc != KPAL_OK) return rc;
        if (lines)
            LAUNCH(ctx, "chunk_key_lines", chunk_key_lines_kernel, dim3(G2c, NB1), dim3(kLineThreads), (const uint32_t *)res,
                   (const uint64_t *)start1, (uint32_t)kpb2, (const ChunkPool *)cl.dpool, cl.p.keys, cl.p.per_block, table);
        else
            LAUNCH(ctx, "chunk_key_scatter", chunk_key_scatter_kernel, dim3(G2c, NB1), dim3(kScatterThreads), (const uint32_t *)res,
                   (const uint64_t *)start1, (uint32_t)kpb2, (const ChunkPool *)cl.dpool, cl.p.keys, cl.p.per_block, table);
        return chunk_histogram<kResKeyBits>(ctx, cl);
    }
    const uint64_t g2_target = std::max<uint64_t>(8, (uint64_t)ctx->num_cu * 8 / NB1);
    uint64_t kpb = (maxn + g2_target - 1) / g2_target;
    kpb = (kpb + kKeysPerBlockQuantum - 1) / kKeysPerBlockQuantum * kKeysPerBlockQuantum;
    if (kpb > 0xFFFFFFFFull) return set_err(KPAL_E_INVALID, "two-level partition: batch too large");
    const uint32_t G2 = (uint32_t)((maxn + kpb - 1) / kpb);
    const size_t rows2 = (size_t)NB1 * kNumBuckets;
    CHK(ensure(ctx, ctx->cntmat, rows2 * G2 * sizeof(uint32_t)));
    CHK(ensure(ctx, ctx->offs, rows2 * G2 * sizeof(uint32_t)));
    CHK(ensure(ctx, ctx->bucket_start, ((size_t)NB1 * (kNumBuckets + 1) + rows2) * sizeof(uint64_t)));
    uint32_t *cntmat2 = (uint32_t *)ctx->cntmat.p;
    uint32_t *offs2 = (uint32_t *)ctx->offs.p;
    uint64_t *bstart2 = (uint64_t *)ctx->bucket_start.p;
    uint64_t *total2 = bstart2 + (size_t)NB1 * (kNumBuckets + 1);
    CHK(ensure(ctx, ctx->slice_start, (size_t)NB1 * (kNumBuckets + 1) * sizeof(uint32_t)));
    uint32_t *sstart2 = (uint32_t *)ctx->slice_start.p;
    LAUNCH(ctx, "key_count", key_count_kernel, dim3(G2, NB1), dim3(kScatterThreads), (const uint32_t *)res,
           (const uint64_t *)start1, (uint32_t)kpb, cntmat2);
    LAUNCH(ctx, "part_rowscan", part_rowscan_kernel, dim3(kNumBuckets, NB1), dim3(256), (const uint32_t *)cntmat2, G2, offs2, total2);
    LAUNCH(ctx, "part_bucketscan", part_bucketscan_kernel, dim3(NB1), dim3(kNumBuckets), (const uint64_t *)total2,
           (uint32_t)kNumBuckets, (const uint64_t *)start1, bstart2, sstart2);
    LAUNCH(ctx, "key_scatter", key_scatter_kernel, dim3(G2, NB1), dim3(kLineThreads), (const uint32_t *)res,
           (const uint64_t *)start1, (uint32_t)kpb, (const uint32_t *)offs2, (const uint64_t *)bstart2, keys);
    LAUNCH(ctx, "part_hist", (part_hist_kernel<kResKeyBits>), dim3(kHistGridX, NB1), dim3(1024),
           (const uint16_t *)keys, (const uint64_t *)bstart2, (const uint32_t *)sstart2, table);
    return KPAL_OK;
}

// Count all k-mers ending in [addr, addr+n) of a device buffer; `halo` bytes left of addr are
// readable and belong to the same feed.  strategy / batch_bytes (-1 / 0: the context's own) are for the pieces this
// function counts again: the pipeline a quad launcher sent one to, the narrower batches of the halves of one.
int count_device_range(kpal_ctx *ctx, const uint8_t *addr, size_t n, size_t halo, int strategy, size_t batch_bytes)
{
    const int requested = strategy >= 0 ? strategy : ctx->strategy;
    int resolved = 0;
    CHK(resolve_strategy(requested, ctx->k, &resolved));
    const bool fresh_candidate = ctx->table_zero_pending && ctx->fresh_feed && halo == 0;
    const int strat = plan_strategy(resolved, requested == KPAL_STRATEGY_AUTO, ctx->k, n, fresh_candidate);
    const size_t km1 = (size_t)ctx->k - 1;
    const size_t piece = plan_piece_bytes(strat, ctx->k, n, ctx->num_cu, batch_bytes ? batch_bytes : ctx->batch_bytes, ctx->batch_bytes_set, kPlanLimits);
    const bool quads = strat == KPAL_STRATEGY_PARTITION_QUADS || strat == KPAL_STRATEGY_PARTITION2_QUADS;
    const bool two_level = strat == KPAL_STRATEGY_PARTITION2 || strat == KPAL_STRATEGY_PARTITION2_QUADS;
    for (size_t off = 0; off < n; off += piece) {
        const size_t len = std::min(piece, n - off);
        // FRESH: the first piece of a count, a whole device feed on the two-level quad pipeline, leaves the table unzeroed
        const bool fresh = fresh_candidate && strat == KPAL_STRATEGY_PARTITION2_QUADS && off == 0 && len == n;
        if (!fresh) CHK(table_ready(ctx));   // zeros materialised; the staged forms of the previous piece added before their buffer is reused
        const size_t h = std::min(km1, halo + off);
        const Span s = make_span(addr + off, len, h);
        if (!quads) {
            ctx->plan_strategy = strat;
            ctx->plan_steps1 = ctx->plan_steps2 = 0;
        }
        if (strat == KPAL_STRATEGY_PARTITION || strat == KPAL_STRATEGY_PARTITION_CHUNKED || strat == KPAL_STRATEGY_PARTITION2) ++ctx->stat_chunked_pieces;
        int rc;
        if (strat == KPAL_STRATEGY_GLOBAL_ATOMIC) rc = launch_global_atomic(ctx, s);
        else if (strat == KPAL_STRATEGY_LDS_DIRECT) rc = launch_lds_direct(ctx, s);
        else if (strat == KPAL_STRATEGY_PARTITION) rc = launch_partition(ctx, s);
        else if (strat == KPAL_STRATEGY_PARTITION_CHUNKED) rc = launch_partition_chunked(ctx, s);
        else if (strat == KPAL_STRATEGY_PARTITION2_QUADS) rc = launch_partition2_quads(ctx, s, fresh);
        else if (strat == KPAL_STRATEGY_PARTITION_QUADS) rc = launch_partition_quads(ctx, s);
        else rc = launch_partition2(ctx, s);
        if (quads) {
            if (rc == KPAL_OK) {
                ++ctx->stat_quad_pieces;
                if (fresh) ++ctx->stat_fresh_pieces;
            }
            if (rc == kSplitBatch) ++ctx->stat_split_pieces;
            if (two_level && (rc == kQuadsUseChunked || rc == kSplitBatch)) CHK(table_ready(ctx));   // (nothing was launched: the other paths need the zeros)
        }
        // A piece its launcher sent back is counted again: through the round-1 pipeline of its k, in that pipeline's own piece
        // size (kQuadsUseChunked: AUTO only), or as two halves (kSplitBatch: a record pool or a coarse bucket too large; rare),
        // which the round-1 two-level pipeline must not join into one batch again.
        if (rc == kQuadsUseChunked) {
            CHK(count_device_range(ctx, addr + off, len, halo + off, two_level ? KPAL_STRATEGY_PARTITION2 : KPAL_STRATEGY_PARTITION_CHUNKED, batch_bytes));
        } else if (rc == kSplitBatch) {
            const size_t half = (len / 2 + 15) & ~(size_t)15;
            const size_t bb = quads ? batch_bytes : std::max<size_t>(half / (ctx->k == 13 ? 4 : 16), 16);
            CHK(count_device_range(ctx, addr + off, half, halo + off, strategy, bb));
            if (len > half) CHK(count_device_range(ctx, addr + off + half, len - half, halo + off + half, strategy, bb));
        } else if (rc != KPAL_OK) {
            return rc;
        }
    }
    return KPAL_OK;
}

KPAL_API int kpal_count_feed_device(kpal_ctx *ctx, const void *dev_buf, size_t nbytes)
{
    CTX_ENTER(ctx);
    if (!ctx->counting) return set_err(KPAL_E_STATE, "kpal_count_feed_device before kpal_count_begin");
    if (nbytes == 0) return KPAL_OK;
    if (!dev_buf) return set_err(KPAL_E_INVALID, "dev_buf is NULL");
    ctx->fresh_feed = true;
    int rc = count_device_range(ctx, (const uint8_t *)dev_buf, nbytes, 0);
    ctx->fresh_feed = false;
    // a FRESH piece whose lists overflowed is counted again from dev_buf: settled here, so that the buffer is the caller's again
    // (stream-ordered, as with every other pipeline) when this call returns
    if (rc == KPAL_OK) rc = quad2_resolve_fresh(ctx);
    return rc;
}

// Host copy into a pinned staging buffer on several cores (fa_read, host_pool.hpp): one core's memcpy (~9 GB/s) is what limits a
// pageable-memory feed otherwise, the PCIe link takes six times that.  Pieces below 4 MiB are not split.
void staged_memcpy(void *dst, const void *src, size_t n)
{
    FaSource s;
    s.mem = (const uint8_t *)src;
    s.end = n;
    (void)fa_read(s, (uint8_t *)dst, 0, n);   // (a memory source cannot fail)
}

// Page-locked host memory on the NUMA node the GPU is attached to: the calling thread's memory policy is set to "prefer that node"
// around the allocation (raw set_mempolicy: libnuma is not a dependency) and hipHostMallocNumaUser lets the runtime honour it.  A
// staging buffer on the other socket puts the inter-socket link into every DMA.  The policy the thread had is saved and put back
// (a policy that cannot be read is left alone: plain allocation).  Any failure falls back to a plain allocation.
int host_alloc_near_gpu(kpal_ctx *ctx, void **out, size_t nbytes)
{
    *out = nullptr;
    const int node = ctx->numa_node;
    hipError_t e = hipErrorUnknown;
    if (node >= 0 && node < 64) {
        unsigned long mask = 1ul << node;
        const long kPreferred = 1;   // MPOL_PREFERRED
        // the thread's own policy (numactl --membind / --interleave, the application's set_mempolicy) is put back afterwards
        int old_mode = 0;
        unsigned long old_mask[16] = {};   // 1024 nodes
        const bool saved = syscall(SYS_get_mempolicy, &old_mode, old_mask, (unsigned long)(sizeof(old_mask) * 8), nullptr, 0ul) == 0;
        if (saved && syscall(SYS_set_mempolicy, kPreferred, &mask, 65ul) == 0) {
            e = hipHostMalloc(out, nbytes, hipHostMallocNumaUser);
            (void)syscall(SYS_set_mempolicy, (long)old_mode, old_mask, (unsigned long)(sizeof(old_mask) * 8 + 1));
            if (e != hipSuccess) {
                (void)hipGetLastError();
                *out = nullptr;
            }
        }
    }
    if (!*out) e = hipHostMalloc(out, nbytes, hipHostMallocDefault);
    if (e != hipSuccess) return set_err(KPAL_E_NOMEM, "hipHostMalloc(%zu bytes) failed: %s", nbytes, hipGetErrorString(e));
    return KPAL_OK;
}

int ensure_pinned(kpal_ctx *ctx)
{
    for (int i = 0; i < 2; ++i)
        if (!ctx->pinned[i]) CHK(host_alloc_near_gpu(ctx, &ctx->pinned[i], kpal_ctx::kStage + kpal_ctx::kStagePad));
    return KPAL_OK;
}

// The reuse protocol of the pinned staging buffers, for every path that writes ctx->pinned[slot]: pinned_wait before the buffer
// is written (the DMA out of its previous contents has finished), pinned_h2d for the DMA out of it (ev_copied[slot] marks its
// end; ctx->stream waits for it).
int pinned_wait(kpal_ctx *ctx, int slot)
{
    if (ctx->stage_used[slot]) HIPCHK(hipEventSynchronize(ctx->ev_copied[slot]));
    return KPAL_OK;
}

int pinned_h2d(kpal_ctx *ctx, int slot, void *dst, const void *src, size_t n)
{
    HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, ctx->copy_stream));
    HIPCHK(hipEventRecord(ctx->ev_copied[slot], ctx->copy_stream));
    HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->ev_copied[slot], 0));
    ctx->stage_used[slot] = true;
    return KPAL_OK;
}

// pinned_source: host_buf came from kpal_host_alloc -- the DMA engine reads it in place, no staging copy; the call returns
// when the last copy has left it (the kernels may still run).
static int count_feed_host(kpal_ctx *ctx, const uint8_t *host_buf, size_t nbytes, bool pinned_source)
{
    const size_t km1 = (size_t)ctx->k - 1;
    const size_t stage = kpal_ctx::kStage;
    const size_t pad = kpal_ctx::kStagePad;  // room for the halo, keeps the payload 16-byte aligned
    CHK(ensure_pinned(ctx));
    for (int i = 0; i < 2; ++i) CHK(ensure(ctx, ctx->dstage[i], stage + pad));
    int slot = 0;
    for (size_t off = 0; off < nbytes; off += stage, slot ^= 1) {
        const size_t len = std::min(stage, nbytes - off);
        const size_t h = std::min(km1, off);
        // the pinned/device slot is free once the H2D copy (pinned) and the kernels (device) that used it are done
        CHK(pinned_wait(ctx, slot));
        if (ctx->stage_used[slot]) HIPCHK(hipStreamWaitEvent(ctx->copy_stream, ctx->ev_done[slot], 0));
        const uint8_t *hp = host_buf + off - h;
        if (!pinned_source) {
            uint8_t *staged = (uint8_t *)ctx->pinned[slot] + (pad - h);
            staged_memcpy(staged, host_buf + off - h, len + h);
            hp = staged;
        }
        uint8_t *dp = (uint8_t *)ctx->dstage[slot].p + (pad - h);
        CHK(pinned_h2d(ctx, slot, dp, hp, len + h));
        CHK(count_device_range(ctx, dp + h, len, h));
        HIPCHK(hipEventRecord(ctx->ev_done[slot], ctx->stream));
    }
    if (pinned_source) HIPCHK(hipStreamSynchronize(ctx->copy_stream));   // the caller may refill its buffer
    return KPAL_OK;
}

KPAL_API int kpal_count_feed(kpal_ctx *ctx, const uint8_t *host_buf, size_t nbytes)
{
    CTX_ENTER(ctx);
    if (!ctx->counting) return set_err(KPAL_E_STATE, "kpal_count_feed before kpal_count_begin");
    if (nbytes == 0) return KPAL_OK;
    if (!host_buf) return set_err(KPAL_E_INVALID, "host_buf is NULL");
    return count_feed_host(ctx, host_buf, nbytes, false);
}

KPAL_API int kpal_count_feed_pinned(kpal_ctx *ctx, const uint8_t *pinned_buf, size_t nbytes)
{
    CTX_ENTER(ctx);
    if (!ctx->counting) return set_err(KPAL_E_STATE, "kpal_count_feed_pinned before kpal_count_begin");
    if (nbytes == 0) return KPAL_OK;
    if (!pinned_buf) return set_err(KPAL_E_INVALID, "pinned_buf is NULL");
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, pinned_buf) != hipSuccess || attr.type != hipMemoryTypeHost) {
        (void)hipGetLastError();
        return set_err(KPAL_E_INVALID, "kpal_count_feed_pinned needs memory from kpal_host_alloc");
    }
    return count_feed_host(ctx, pinned_buf, nbytes, true);
}

KPAL_API int kpal_host_alloc(kpal_ctx *ctx, size_t nbytes, void **host_out)
{
    CTX_ENTER(ctx);
    if (!host_out) return set_err(KPAL_E_INVALID, "host_out is NULL");
    CHK(host_alloc_near_gpu(ctx, host_out, nbytes ? nbytes : 16));
    ctx->host_allocs.push_back(*host_out);
    return KPAL_OK;
}

KPAL_API int kpal_host_free(kpal_ctx *ctx, void *host)
{
    CTX_ENTER(ctx);
    if (!host) return KPAL_OK;
    auto it = std::find(ctx->host_allocs.begin(), ctx->host_allocs.end(), host);
    if (it == ctx->host_allocs.end()) return set_err(KPAL_E_INVALID, "not a buffer of kpal_host_alloc of this context");
    HIPCHK(hipStreamSynchronize(ctx->copy_stream));
    HIPCHK(hipHostFree(host));
    ctx->host_allocs.erase(it);
    return KPAL_OK;
}


KPAL_API int kpal_count_finish(kpal_ctx *ctx, int64_t *host_out)
{
    CTX_ENTER(ctx);
    if (!ctx->counting) return set_err(KPAL_E_STATE, "kpal_count_finish before kpal_count_begin");
    CHK(count_end_text(ctx));   // the end of a FASTQ text: its last record
    CHK(table_ready(ctx));
    uint32_t pool_error = 0, quad_error = 0;
    if (ctx->chunk_error_armed)
        HIPCHK(hipMemcpyAsync(&pool_error, ctx->chunk_error_word, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (ctx->quad_error_word)
        HIPCHK(hipMemcpyAsync(&quad_error, ctx->quad_error_word, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    // (a double-buffered pinned staging path was measured slower than the runtime's pageable copy)
    if (host_out)
        HIPCHK(hipMemcpyAsync(host_out, ctx->table.p, ctx->bins * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (pool_error) {
        HIPCHK(hipMemsetAsync(ctx->chunk_error_word, 0, sizeof(uint32_t), ctx->stream));
        return set_err(KPAL_E_HIP, "chunked partition: the chunk pool ran out (internal sizing error %u); counts are invalid", pool_error);
    }
    if (quad_error) {
        HIPCHK(hipMemsetAsync(ctx->quad_error_word, 0, sizeof(uint32_t), ctx->stream));
        return set_err(KPAL_E_HIP, "quad partition: internal sizing error %u; counts are invalid", quad_error);
    }
    return KPAL_OK;
}

KPAL_API int kpal_count_balance(kpal_ctx *ctx)
{
    CTX_ENTER(ctx);
    if (!ctx->counting) return set_err(KPAL_E_STATE, "kpal_count_balance before kpal_count_begin");
    CHK(count_end_text(ctx));   // (a FASTQ record still carried belongs to the table that is balanced)
    // two-level quad pipeline: the pending finalisation of the table balances it in the same pass
    if (ctx->fin.pending) return quad2_finalize(ctx, true);
    CHK(table_ready(ctx));
    return launch_balance(ctx, ctx->k, (const int64_t *)ctx->table.p, (int64_t *)ctx->table.p);
}

KPAL_API int kpal_count_last_plan(kpal_ctx *ctx, int *strategy, int *steps1, int *steps2)
{
    if (!ctx) return set_err(KPAL_E_INVALID, "ctx is NULL");
    if (strategy) *strategy = ctx->plan_strategy;
    if (steps1) *steps1 = ctx->plan_steps1;
    if (steps2) *steps2 = ctx->plan_steps2;
    return KPAL_OK;
}

KPAL_API int kpal_count_stats(kpal_ctx *ctx, uint64_t *out, int n)
{
    CTX_ENTER(ctx);
    if (!out || n < 1) return set_err(KPAL_E_INVALID, "out is NULL");
    uint32_t words[4] = {0, 0, 0, 0};
    if (ctx->quad_error_word) {
        HIPCHK(hipMemcpyAsync(words, ctx->quad_error_word, sizeof(words), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    const uint64_t all[KPAL_COUNT_STATS] = {words[1], words[2], words[3], ctx->stat_fresh_pieces, ctx->stat_fresh_reruns, ctx->stat_quad_pieces,
                                            ctx->stat_chunked_pieces, ctx->stat_split_pieces, ctx->stat_repeat_pieces};
    for (int i = 0; i < n; ++i) out[i] = i < KPAL_COUNT_STATS ? all[i] : 0;
    return KPAL_OK;
}

KPAL_API int kpal_count_table(kpal_ctx *ctx, void **dev_table, uint64_t *n_bins)
{
    if (!ctx) return set_err(KPAL_E_INVALID, "ctx is NULL");
    if (!ctx->counting) return set_err(KPAL_E_STATE, "no count table (call kpal_count_begin)");
    HIPCHK(hipSetDevice(ctx->device));
    CHK(table_ready(ctx));   // the caller is about to use the table
    if (dev_table) *dev_table = ctx->table.p;
    if (n_bins) *n_bins = ctx->bins;
    return KPAL_OK;
}

KPAL_API int kpal_synth_reads_device(kpal_ctx *ctx, uint64_t seed, uint64_t first_read, uint64_t n_reads,
                                     int read_len, int noisy, void *dev_out)
{
    CTX_ENTER(ctx);
    if (read_len < 1) return set_err(KPAL_E_INVALID, "read_len must be >= 1");
    if (n_reads == 0) return KPAL_OK;
    if (!dev_out || ((uintptr_t)dev_out & 15)) return set_err(KPAL_E_INVALID, "dev_out must be a 16-byte aligned device pointer");
    const uint64_t total = n_reads * (uint64_t)(read_len + 1);
    const uint64_t nvec = (total + 15) / 16;
    const unsigned grid = (unsigned)std::min<uint64_t>((nvec + 255) / 256, (uint64_t)ctx->num_cu * 16);
    LAUNCH(ctx, "synth_reads", synth_reads_kernel, dim3(grid), dim3(256), seed, first_read, n_reads,
           (uint32_t)read_len, noisy, (uint8_t *)dev_out);
    return KPAL_OK;
}
