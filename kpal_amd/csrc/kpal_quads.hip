// kpal_quads.hip -- launcher of the quad record pipeline, k = 8..12 (quad_kernels.hpp): the sample of the row loads, one
// scatter launch, one histogram launch.  What they are launched with is decided in quad_plan.hpp.
#include "kpal_host.hpp"

#include "quad_kernels.hpp"

// The metadata of both quad pipelines (one buffer: rounds per scatter workgroup, error + statistics words, sample counters);
// the error word is cleared when it is first handed out (kpal_count_begin clears it from then on).
int quad_meta(kpal_ctx *ctx, QuadMeta *out)
{
    CHK(ensure(ctx, ctx->quad_meta, ((size_t)ctx->num_cu + 4 + 2048 + 512) * sizeof(uint32_t)));
    out->nrounds = (uint32_t *)ctx->quad_meta.p;
    out->error = out->nrounds + ctx->num_cu;
    out->load = out->error + 4;
    if (!ctx->quad_error_word) {
        HIPCHK(hipMemsetAsync(out->error, 0, 4 * sizeof(uint32_t), ctx->stream));
        ctx->quad_error_word = out->error;
    }
    return KPAL_OK;
}

// Tile size of a quad scatter from the row loads of a ~1/64 sample of the feed (quad_sample_kernel; quad_plan.hpp says what
// they mean): the largest candidate (wave-steps per wave per tile) whose expected steady-state backlog stays well inside the
// spill list.  Returns kQuadsUseChunked (AUTO only) when a few rows hold more than 1.5 % of all items.  `fine`: the two-level
// path also takes the sorted loads of the 512 fine rows.
int quad_choose_steps(kpal_ctx *ctx, const Span &s, uint32_t *load, int buckets, int slots, const int *candidates, size_t n_candidates,
                      int *steps_out, std::vector<double> *fine)
{
    const int extra = fine ? kQuadFineRows : 0;
    const QuadSampleGrid g = quad_sample_grid((s.nchunks + 63) / 64);
    HIPCHK(hipMemsetAsync(load, 0, (size_t)(buckets + extra + 1) * sizeof(uint32_t), ctx->stream));   // (+ 1: the items of repeat lanes)
    DISPATCH_K_8_16(ctx->k, LAUNCH(ctx, "quad_sample", (quad_sample_kernel<K>), dim3(g.groups), dim3(512), s, g.stride, g.sample_steps, load));
    std::vector<uint32_t> h((size_t)(buckets + extra + 1));
    HIPCHK(hipMemcpyAsync(h.data(), load, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    QuadVerdict v = quad_sample_verdict(h.data(), buckets, fine ? h.data() + buckets : nullptr, h[(size_t)(buckets + extra)], g.sampled_steps,
                                        ctx->strategy == KPAL_STRATEGY_AUTO);
    if (ctx->quad_verbose)
        fprintf(stderr, "[kpal quad] sample: %.2f %% of the items are the excess of the 32 fullest rows, %.0f %% of it in three rows\n",
                v.hot_percent, v.top3_percent);
    if (v.use_chunked) return kQuadsUseChunked;
    ctx->tiles.hot_rows = v.hot_rows;
    const QuadWalk w = quad_walk_level1(v.loads, slots, candidates, n_candidates, v.budget);
    if (ctx->quad_verbose)
        for (size_t ci = 0; ci < w.tried; ++ci)
            fprintf(stderr, "[kpal quad] sample: %d steps per wave -> expected backlog %.0f items (fullest row %.1f of %d)\n", candidates[ci],
                    w.backlog[ci], v.loads.back() * kQuadWaves * candidates[ci], slots);
    *steps_out = w.steps;
    if (fine) *fine = std::move(v.fine);
    return KPAL_OK;
}

// Partition of quads into aligned records, k = 8..12 (quad_kernels.hpp): one workgroup per CU scatters,
// one workgroup per bucket histograms.  pool[bucket][workgroup][round] holds one record per flush round.
int launch_partition_quads(kpal_ctx *ctx, const Span &s)
{
    const uint64_t total_steps = (s.nchunks + 63) / 64;
    if (total_steps == 0) return KPAL_OK;
    const int buckets = ctx->k == 12 ? QuadCfg<12>::kBuckets : 512;                                     // ROWS of the scatter
    const int slots = ctx->k == 12 ? QuadCfg<12>::kItems : kQuadRowWords / buckets;                     // items a row holds
    QuadMeta meta;
    CHK(quad_meta(ctx, &meta));
    uint32_t *nrounds = meta.nrounds, *error = meta.error;
    // ---- plan: the tile size.  A tile of 16 waves x STEPS wave-steps brings ~0.119 x 16 x STEPS items per 16-slot row at k = 12 when
    // the k-mers are uniform (7 steps: 13.3 of 16, records 83 % full, ~3 % of the items spill to the list); the row loads of a
    // 1/64 sample say what THIS input brings.  The largest STEPS whose expected overflow per round stays well inside the
    // spill list is used (KPAL_QUAD_STEPS forces one: A/B timing, tests).  16 waves = four per SIMD with 128 registers each
    // (8 record vectors + 7 prefetched chunks live): measured 3 % faster than 8 waves x 13 steps and the records are fuller.
    static const int candidates[] = {8, 7, 6, 4, 3, 2, 1};
    constexpr size_t n_candidates = sizeof(candidates) / sizeof(candidates[0]);
    const size_t feed_bytes = (size_t)(s.hi - s.emit_from);
    int steps = quad_forced_steps(ctx->quad_steps_forced, candidates, n_candidates);
    if (!steps && ctx->tiles.hit(feed_bytes, 1)) steps = ctx->tiles.steps1;
    const bool sampled = !steps;
    if (sampled) {
        CHK(quad_choose_steps(ctx, s, meta.load, buckets, slots, candidates, n_candidates, &steps));
        ctx->tiles.store(steps, 0, feed_bytes);
    }
    const QuadTile tile = quad1_tile(steps, sampled, ctx->tiles.hot_rows, ctx->quad_steps_forced, ctx->quad_repeat_forced);
    steps = tile.steps;
    const bool repeat = tile.repeat;
    if (tile.counted) ++ctx->stat_repeat_pieces;
    ctx->plan_strategy = KPAL_STRATEGY_PARTITION_QUADS;
    ctx->plan_steps1 = steps;
    ctx->plan_steps2 = 0;
    // ---- check
    const Quad1Geometry geo = quad1_geometry(total_steps, steps, ctx->quad_cus());
    if (geo.too_large) return set_err(KPAL_E_INVALID, "quad partition: batch too large");
    if (geo.pool_bytes > ctx->quad_pool_max && s.nchunks > 64) return kSplitBatch;   // (heavily skewed 16 GiB piece: small tiles)
    const uint32_t G = geo.G;
    const uint64_t tpb = geo.tpb;
    // ---- buffers
    CHK(ensure(ctx, ctx->keys, geo.pool_bytes));
    uint32_t *pool = (uint32_t *)ctx->keys.p;
    const TableOnly table = {(unsigned long long *)ctx->table.p};   // counts that bypass the records: atomics into the (zeroed) table
    // k = 12: every table entry receives FOUR adds from the histogram stage (one per form, from four different workgroups): 67 M
    // global atomics per piece, 0.25 ms of the 3.7 ms histogram (A/B `hist_nomerge`) -- and Profile.balance then reads and writes the
    // table once more.  As on the two-level path the forms are STAGED instead (8-bit counts, 64 MiB; quad2_index.hpp with the
    // 11-bit bucket read as coarse : fine) and quad2_finalize_kernel gathers the four of every entry -- and balances in the same
    // pass when kpal_count_balance asks (the pending finalisation: kpal_quads2.hip).  A form count >= 256 goes to the table
    // directly; the mean per form is bytes / (4 x 4^12), so pieces whose mean could pass 240 (16 GB of unbroken sequence) keep the
    // atomic merge.  KPAL_K12_STAGED=0: the atomic merge everywhere (A/B, tests).
    uint32_t *stage = nullptr;
    if (ctx->k == 12 && ctx->k12_staged && (double)feed_bytes <= 240.0 * 4.0 * (double)ctx->bins) {
        CHK(ensure(ctx, ctx->residuals, (size_t)ctx->bins * 4 * sizeof(quad2_stage_t)));
        stage = (uint32_t *)ctx->residuals.p;
    }
    // ---- launch
    // (input chunks are requested S steps ahead; at k <= 11 with eight steps that ring costs the registers the kernel does not have --
    // 12 spilled, and a kernel that uses scratch memory at all ran ~10 % slower in same-box comparisons -- so four steps ahead there;
    // k = 12 fits its 128 registers either way and a four-step ring changed nothing: 7.44 vs 7.40 ms)
    // REPEAT: the instantiation that sends the repeat lanes of low-complexity sequence straight to the hot-item table (quad_kernels.hpp);
    // taken when the sample shows hot rows (KPAL_QUAD_REPEAT=0 / 1 forces one: A/B, tests).  Its call site costs registers: a
    // four-step input ring in the 8-step tile (and no such instantiation of the 7-step tile: it would spill).
#define KPAL_QUAD_LAUNCH(S)                                                                                                  \
    do {                                                                                                                     \
        if (repeat)                                                                                                          \
            LAUNCH(ctx, "quad_scatter", (quad_scatter_kernel<K, 16, S, (S == 8 ? 4 : S), TableOnly, (S != 7)>), dim3(G), dim3(1024), s, tpb, pool, (uint32_t)tpb, \
                   nrounds, error, table);                                                                                   \
        else                                                                                                                 \
            LAUNCH(ctx, "quad_scatter", (quad_scatter_kernel<K, 16, S, (S == 8 && K != 12 ? 4 : S), TableOnly, false>), dim3(G), dim3(1024), s, tpb, pool,    \
                   (uint32_t)tpb, nrounds, error, table);                                                                    \
    } while (0)
    DISPATCH_K_8_12(ctx->k, {
        switch (steps) {
        case 8: KPAL_QUAD_LAUNCH(8); break;
        case 7: KPAL_QUAD_LAUNCH(7); break;
        case 4: KPAL_QUAD_LAUNCH(4); break;
        case 3: KPAL_QUAD_LAUNCH(3); break;
        case 2: KPAL_QUAD_LAUNCH(2); break;
        case 1: KPAL_QUAD_LAUNCH(1); break;
        default: KPAL_QUAD_LAUNCH(6); break;
        }
        LAUNCH(ctx, "quad_hist", (quad_hist_kernel<K>), dim3(QuadCfg<K>::kHistBuckets), dim3(1024), (const uint32_t *)pool,
               (const uint32_t *)nrounds, G, (uint32_t)tpb, table, stage);
    });
#undef KPAL_QUAD_LAUNCH
    // ---- arm the finalisation
    if (stage) ctx->fin.arm(stage);   // added to the table (and balanced) by quad2_finalize_kernel<12, ...> when something needs the table
    if (ctx->quad_verbose) {   // diagnostics: tile size chosen, tiles abandoned to the direct path
        uint32_t st[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(st, error, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        fprintf(stderr, "[kpal quad] k=%d steps/wave/tile=%d tiles=%llu workgroups=%u hot-table entries used so far=%u\n", ctx->k, steps,
                (unsigned long long)geo.tiles, G, st[1]);
    }
    return KPAL_OK;
}

