// kpal_quads2.hip -- launcher of the two-level quad record pipeline, k = 13..16 (quad_kernels.hpp, second half; planned by
// quad_plan.hpp), and the pending finalisation of the table (kpal_host.hpp: QuadFinalize).
#include "kpal_host.hpp"

#include "quad_kernels.hpp"

// level 1, eight steps per tile: input chunks requested FOUR steps ahead (4 KiB per wave in flight) -- with a ring of eight the
// kernel sits at 128 registers and the sink handling of its epilogue spills; kernels that use scratch at all ran 8 % slower
#ifndef KPAL_L1_DEPTH8
#define KPAL_L1_DEPTH8 4
#endif

// Two-level partition of quads, k = 13..16 (quad_kernels.hpp, end): level-1 records by coarse bucket, level-2 records
// by (coarse, fine) bucket, histogram per (coarse, fine) bucket.
int launch_partition2_quads(kpal_ctx *ctx, const Span &s, bool fresh)
{
    const uint64_t total_steps = (s.nchunks + 63) / 64;
    if (total_steps == 0) return KPAL_OK;
    QuadMeta meta;
    CHK(quad_meta(ctx, &meta));
    uint32_t *nrounds1 = meta.nrounds, *error = meta.error;
    // ---- plan.  Level 1: 16 waves x 7 wave-steps per tile bring 107 items per 128-slot row (26.7 per 32 at k = 16) for uniform
    // k-mers; the sampled row loads say whether THIS feed needs a smaller tile, or (AUTO) the round-1 pipeline.  Level 2 has the
    // finer list of candidates (quad_plan.hpp: kQuadCandidates2).
    static const int candidates[] = {8, 7, 6, 3};
    const size_t feed_bytes = (size_t)(s.hi - s.emit_from);
    const bool cached = ctx->tiles.hit(feed_bytes, 2);
    std::vector<double> fine;                    // items per fine row of level 2 per wave-step of INPUT (sorted)
    int chosen = ctx->tiles.steps1;
    if (!cached) {   // (also when KPAL_QUAD_STEPS forces level 1: level 2 needs the sample)
        const Quad2Rows rows = quad2_rows(ctx->k);
        CHK(quad_choose_steps(ctx, s, meta.load, (int)(rows.NB1 * rows.REP), (int)rows.S1, candidates, 4, &chosen, &fine));
    }
    const QuadTile tile1 = quad2_tile1(quad_forced_steps(ctx->quad_steps_forced, candidates, 4), chosen, ctx->tiles.hot_rows, ctx->quad_repeat_forced);
    const int steps1 = tile1.steps;
    const bool repeat1 = tile1.repeat;
    if (tile1.counted) ++ctx->stat_repeat_pieces;
    // ---- check.  A piece that is refused or halved here has been sampled but leaves no tile sizes behind: its halves sample again.
    const Quad2Level1 l1 = quad2_level1(ctx->k, total_steps, steps1, ctx->quad_cus());
    if (l1.too_large) return set_err(KPAL_E_INVALID, "quad partition: batch too large");
    if (l1.pool1_bytes > ctx->quad_pool_max && s.nchunks > 64) return kSplitBatch;
    int steps2 = cached ? ctx->tiles.steps2 : quad_walk_level2(fine, steps1);
    const int forced2 = quad_forced_steps(ctx->quad_steps2_forced, kQuadCandidates2, sizeof(kQuadCandidates2) / sizeof(kQuadCandidates2[0]));
    const Quad2Level2 l2 = quad2_level2(l1, forced2 ? forced2 : steps2, ctx->quad_cus());
    if (l2.too_large) return set_err(KPAL_E_INVALID, "quad partition: batch too large");
    if (!cached) ctx->tiles.store(steps1, steps2, feed_bytes);
    if (forced2) steps2 = forced2;               // (KPAL_QUAD_STEPS2: applied after the sizes are kept, so never kept itself)
    ctx->plan_strategy = KPAL_STRATEGY_PARTITION2_QUADS;
    ctx->plan_steps1 = steps1;
    ctx->plan_steps2 = steps2;
    constexpr int kWaves2 = kQuadWaves;
    const uint32_t NB1 = l1.NB1, G1 = l1.G1, G2 = l2.G2, upw = l2.upw, nseg = l2.nseg;
    const uint64_t tpb1 = l1.tpb1, cap1 = l1.cap1, tiles2 = l2.tiles2, cap2 = l2.cap2;
    // ---- buffers.  Level-1 records; level-2 records (64 items packed into 192 bytes) and their rounds.
    // the staged forms of the histogram stage (four 8-bit counts per table entry: 4.3 GB at k = 15) reuse the level-1 pool's buffer:
    // level 2 has read it completely before the histogram kernel starts (same stream)
    CHK(ensure(ctx, ctx->residuals, std::max<size_t>(l1.pool1_bytes, (size_t)ctx->bins * 4 * sizeof(quad2_stage_t))));
    CHK(ensure(ctx, ctx->keys, l2.pool2_bytes));
    CHK(ensure(ctx, ctx->quad_meta2, (size_t)NB1 * G2 * sizeof(uint32_t)));
    uint32_t *pool1 = (uint32_t *)ctx->residuals.p;
    uint32_t *stage = pool1;
    uint32_t *pool2 = (uint32_t *)ctx->keys.p;
    uint32_t *nrounds2 = (uint32_t *)ctx->quad_meta2.p;
    // Counts that bypass the records (TableSink, quad_kernels.hpp): classic -> atomic adds into the (zeroed) table; FRESH -> lists,
    // one segment per scatter workgroup (level 1: G1, level 2: G2 x NB1) and one shared segment for the histogram stage
    uint32_t seg = 0, seg_h = 0;
    TableSink table = {(unsigned long long *)ctx->table.p, nullptr, nullptr, 0u, nullptr};
    TableSink table2 = table, table_h = table;
    if (fresh) {
        // the histogram stage's shared segment also takes every count that does not fit a staged form (>= 256 within one form and
        // piece: repeats of real genomes): room for 4 M entries (unless the tests force small segments)
        // (a feed whose sample showed hot rows sends more counts past the records -- the k-mer entries of the hot-item tables leave as
        // they age, a few hundred per workgroup and four tiles: sixteen times the room (2.7 GB at k = 15), or the piece would overflow its lists and run again)
        seg = (repeat1 && !ctx->direct_seg_forced) ? ctx->direct_seg * 16u : ctx->direct_seg;
        seg_h = ctx->direct_seg_forced ? seg : std::max<uint32_t>(seg, 1u << 22);
        CHK(ensure(ctx, ctx->direct_list, ((size_t)(nseg - 1) * seg + seg_h) * sizeof(unsigned long long)));
        CHK(ensure(ctx, ctx->direct_meta, ((size_t)nseg + 4) * sizeof(uint32_t)));
        unsigned long long *list = (unsigned long long *)ctx->direct_list.p;
        uint32_t *counts = (uint32_t *)ctx->direct_meta.p, *overflow = counts + nseg;
        HIPCHK(hipMemsetAsync(counts, 0, ((size_t)nseg + 4) * sizeof(uint32_t), ctx->stream));
        table = TableSink{nullptr, list, counts, seg, overflow};                                             // (the kernels add their workgroup's offset)
        table2 = TableSink{nullptr, list + (size_t)G1 * seg, counts + G1, seg, overflow};
        table_h = TableSink{nullptr, list + (size_t)(nseg - 1) * seg, counts + (nseg - 1), seg_h, overflow};   // global counter
    }
    // ---- launch
#define KPAL_QUAD2_LAUNCH(S2)                                                                                                          \
    do {                                                                                                                               \
        if (repeat1)                                                                                                                   \
            LAUNCH(ctx, "quad2_scatter", (quad2_scatter_kernel<K, kWaves2, S2, true>), dim3(G2, NB1), dim3(kWaves2 * 64), (const uint32_t *)pool1, \
                   (const uint32_t *)nrounds1, G1, (uint32_t)cap1, upw, (uint32_t)tiles2, pool2, (uint32_t)cap2, nrounds2, error, table2); \
        else                                                                                                                           \
            LAUNCH(ctx, "quad2_scatter", (quad2_scatter_kernel<K, kWaves2, S2, false>), dim3(G2, NB1), dim3(kWaves2 * 64), (const uint32_t *)pool1, \
                   (const uint32_t *)nrounds1, G1, (uint32_t)cap1, upw, (uint32_t)tiles2, pool2, (uint32_t)cap2, nrounds2, error, table2); \
    } while (0)
    // (REPEAT: the level-1 instantiation with the repeat lanes' shortcut, when the sample shows hot rows -- kpal_quads.hip; the
        // seven-step tile has no such instantiation: at 128 registers the call site cost it spilled ones)
#define KPAL_QUAD1_LAUNCH(S, D)                                                                                                        \
    do {                                                                                                                               \
        if (repeat1 && S != 7)                                                                                                         \
            LAUNCH(ctx, "quad_scatter", (quad_scatter_kernel<K, 16, S, D, TableSink, (S != 7)>), dim3(G1), dim3(1024), s, tpb1, pool1, (uint32_t)cap1, nrounds1, error, table); \
        else                                                                                                                           \
            LAUNCH(ctx, "quad_scatter", (quad_scatter_kernel<K, 16, S, D, TableSink, false>), dim3(G1), dim3(1024), s, tpb1, pool1, (uint32_t)cap1, nrounds1, error, table);    \
    } while (0)
    DISPATCH_K_13_16(ctx->k, {
        if (steps1 == 8) KPAL_QUAD1_LAUNCH(8, KPAL_L1_DEPTH8);
        else if (steps1 == 7) KPAL_QUAD1_LAUNCH(7, 7);
        else if (steps1 == 6) KPAL_QUAD1_LAUNCH(6, 6);
        else KPAL_QUAD1_LAUNCH(3, 3);
        switch (steps2) {
        case 8: KPAL_QUAD2_LAUNCH(8); break;
        case 7: KPAL_QUAD2_LAUNCH(7); break;
        case 6: KPAL_QUAD2_LAUNCH(6); break;
        case 4: KPAL_QUAD2_LAUNCH(4); break;
        case 3: KPAL_QUAD2_LAUNCH(3); break;
        default: KPAL_QUAD2_LAUNCH(2); break;
        }

        // (packed bins: two forms per word, two workgroups per CU -- safe while a histogram workgroup's stream holds < 2^16 item slots)
        if (K >= 15 && (uint64_t)G2 * cap2 * 64 < 65536 && !ctx->quad_hist_unpacked)
            LAUNCH(ctx, "quad_hist", (quad_hist_kernel<K, TableSink, true>), dim3(512, NB1), dim3(1024), (const uint32_t *)pool2, (const uint32_t *)nrounds2,
                   G2, (uint32_t)cap2, table_h, stage);
        else
            LAUNCH(ctx, "quad_hist", (quad_hist_kernel<K, TableSink, false>), dim3(512, NB1), dim3(1024), (const uint32_t *)pool2, (const uint32_t *)nrounds2,
                   G2, (uint32_t)cap2, table_h, stage);
    });
#undef KPAL_QUAD2_LAUNCH
    // ---- arm the finalisation.  The staged forms are added to the table by quad2_finalize_kernel -- LATER: kpal_count_balance fuses Profile.balance into
    // that pass; anything else that needs the table (the next piece or feed, kpal_count_finish / _table, kpal_sync) flushes it
    // first (quad2_finalize(ctx, false)).
    ctx->fin.arm(stage, fresh, s, nseg, seg, seg_h);
    if (fresh) ctx->table_zero_pending = false;   // the finalisation writes every entry
    return KPAL_OK;
}

// The table as every consumer other than a FRESH finalisation expects it: zeroed if nothing has been counted into it yet, the
// staged forms of the last two-level quad piece added.
int table_ready(kpal_ctx *ctx)
{
    if (ctx->table_zero_pending) {
        HIPCHK(hipMemsetAsync(ctx->table.p, 0, ctx->bins * sizeof(int64_t), ctx->stream));
        ctx->table_zero_pending = false;
    }
    return quad2_finalize(ctx, false);
}

// A pending FRESH piece: did every bypassing count fit its list segment?  (One word; the host waits for the piece's kernels --
// it would soon anyway: the finalisation is launched from the host.)  If not -- a heavily skewed piece; the lists are sized for
// the usual few hundred entries per workgroup -- the classic way after all: zero the table, count the piece AGAIN with atomic
// adds for what bypasses the records.  That re-reads the fed buffer, so kpal_count_feed_device calls this before it returns: the
// caller's buffer is free again when the feed call is back, as with every other pipeline.
int quad2_resolve_fresh(kpal_ctx *ctx)
{
    if (!ctx->fin.needs_resolve()) return KPAL_OK;
    uint32_t overflow = 0;
    const uint32_t *word = (const uint32_t *)ctx->direct_meta.p + ctx->fin.nseg;
    HIPCHK(hipMemcpyAsync(&overflow, word, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->fin.resolve();
    if (overflow) {
        ++ctx->stat_fresh_reruns;
        ctx->fin.clear();
        HIPCHK(hipMemsetAsync(ctx->table.p, 0, ctx->bins * sizeof(int64_t), ctx->stream));
        const int rc = launch_partition2_quads(ctx, ctx->fin.span, false);   // (classic: armed again, not fresh)
        if (rc != KPAL_OK) return rc == kQuadsUseChunked || rc == kSplitBatch ? set_err(KPAL_E_HIP, "two-level quad pipeline: cannot repeat a piece") : rc;
    }
    return KPAL_OK;
}

// Adds the staged forms of the last two-level quad piece to the count table (and balances the table in the same pass).
int quad2_finalize(kpal_ctx *ctx, bool balance)
{
    if (!ctx->fin.pending) return KPAL_OK;
    CHK(quad2_resolve_fresh(ctx));
    const bool fresh = ctx->fin.take();
    const quad2_stage_t *stage = (const quad2_stage_t *)ctx->fin.stage;
    unsigned long long *table = (unsigned long long *)ctx->table.p;
    if (ctx->k == 12) {   // the one-level pipeline's staged forms (kpal_quads.hip): never FRESH (its table is zeroed by kpal_count_begin)
        if (balance) LAUNCH(ctx, "quad2_finalize_balanced", (quad2_finalize_kernel<12, true, false>), dim3(Quad2Index<12>::kSets), dim3(1024), stage, table);
        else LAUNCH(ctx, "quad2_finalize", (quad2_finalize_kernel<12, false, false>), dim3(Quad2Index<12>::kSets), dim3(1024), stage, table);
        return KPAL_OK;
    }
    DISPATCH_K_13_16(ctx->k, {
        if (balance && fresh)
            LAUNCH(ctx, "quad2_finalize_balanced", (quad2_finalize_kernel<K, true, true>), dim3(Quad2Index<K>::kSets), dim3(1024), stage, table);
        else if (balance)
            LAUNCH(ctx, "quad2_finalize_balanced", (quad2_finalize_kernel<K, true, false>), dim3(Quad2Index<K>::kSets), dim3(1024), stage, table);
        else if (fresh)
            LAUNCH(ctx, "quad2_finalize", (quad2_finalize_kernel<K, false, true>), dim3(Quad2Index<K>::kSets), dim3(1024), stage, table);
        else
            LAUNCH(ctx, "quad2_finalize", (quad2_finalize_kernel<K, false, false>), dim3(Quad2Index<K>::kSets), dim3(1024), stage, table);
        if (fresh)
            LAUNCH(ctx, "quad2_apply_list", (quad2_apply_list_kernel<K>), dim3(ctx->fin.nseg - 1 + kQuad2ListTailBlocks), dim3(256),
                   (const unsigned long long *)ctx->direct_list.p, (const uint32_t *)ctx->direct_meta.p, ctx->fin.seg, ctx->fin.nseg - 1,
                   ctx->fin.seg_hist, balance ? 1u : 0u, table);
    });
    return KPAL_OK;
}
