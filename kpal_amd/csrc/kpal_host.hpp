// kpal_host.hpp -- host side shared by the translation units of libkpal_hip.so: errors, the context,
// workspace buffers, per-kernel HIP-event timing, the launch / dispatch macros and the few host functions
// one unit calls in another.  (kpal_ctx.hip: context + profiling API; kpal_count.hip: counting front end and the
// round-1 pipelines; kpal_text.hip: FASTA and FASTQ ingest; kpal_records.hip: one profile per record / per sliding window;
// kpal_quads.hip / kpal_quads2.hip: the quad record pipelines, planned by quad_plan.hpp; kpal_vec.hip: one vector -- balance,
// split, summaries, merge, shrink; kpal_sets.hip: the summaries and the strand balance of a whole set of vectors, planned by
// stat_plan.hpp, and the strand balance of one vector, which is a set of one; kpal_spectrum.hip: the count-of-counts spectrum of
// every vector of a set, planned by spectrum_plan.hpp; kpal_transform.hip: the balance, the shrink and the pool of a whole set of
// vectors, planned by transform_plan.hpp; kpal_pool_groups.hip: the pool of a set by label, planned by pool_groups_plan.hpp --
// these five share table_host.hpp on top of this header: the argument checks, the upload of host tables, the shrink launch;
// kpal_multi.hip: multi-GPU entry points over RCCL.  The five units that serve distances
// share dist_host.hpp on top of this header -- kpal_pair.hip: the distance of one pair, plain and with options; kpal_cross.hip:
// the distances of sets of profiles, triangle and rectangle, plain, with options and with dynamic smoothing, planned by
// matrix_plan.hpp and smooth_plan.hpp; kpal_paired.hip: the distances of the linked pairs of two sets, planned by
// pair_set_plan.hpp; kpal_paired_smooth.hip: those with dynamic smoothing and the smoothed tables of the pairs, planned by
// pair_smooth_plan.hpp; kpal_nearest.hip: the nearest n of a rectangle, tiled by nearest_plan.hpp.)
#pragma once
#include "../../include/kpal_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "kpal_device.hpp"
#include "host_pool.hpp"
#include "quad_plan.hpp"
#include "matrix_plan.hpp"
#include "fastq_mask.hpp"
#include "record_scan.hpp"

#define KPAL_API extern "C" __attribute__((visibility("default")))

using namespace kpal;

// ----------------------------------------------------------------------------------------------
// errors
// ----------------------------------------------------------------------------------------------
int set_err(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIPCHK(expr)                                                                               \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return set_err(e_ == hipErrorOutOfMemory ? KPAL_E_NOMEM : KPAL_E_HIP, "%s failed: %s (%s:%d)", \
                           #expr, hipGetErrorString(e_), __FILE__, __LINE__);                      \
    } while (0)

#define CHK(expr)              \
    do {                       \
        int rc_ = (expr);      \
        if (rc_ != KPAL_OK) return rc_; \
    } while (0)


// ----------------------------------------------------------------------------------------------
// context
// ----------------------------------------------------------------------------------------------
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

struct ProfRec {
    int name;
    hipEvent_t a, b;
};

// The staged forms of the last quad piece that have not been added to the table yet (quad2_finalize; armed by
// launch_partition_quads at k = 12 and by launch_partition2_quads).  FRESH (kpal_quads2.hip): kpal_count_begin leaves the table
// of a k >= 13 count UNZEROED (kpal_ctx::table_zero_pending) -- the first piece, if it is a whole device feed on the two-level
// quad pipeline, lets its finalisation WRITE the table instead of adding to it, and keeps the few counts that bypass the
// records in lists until then.  Every other consumer of the table materialises the zeros first (table_ready).
//   idle --arm--> pending [fresh: --resolve--> resolved (lists fit) | --clear--> idle, the piece armed again classically]
//   pending --take--> idle (the finalisation is launched);  kpal_count_begin: clear (staged forms of an abandoned count)
struct QuadFinalize {
    bool pending = false;
    const void *stage = nullptr;
    bool fresh = false;
    bool resolved = false;        // the overflow word of the pending FRESH piece has been read (quad2_resolve_fresh)
    Span span = {};               // the piece of a FRESH finalisation (re-run classically if a list overflowed)
    uint32_t nseg = 0;            // list segments of that piece
    uint32_t seg = 16384;         // ... entries of each (sixteen times kpal_ctx::direct_seg for a feed with hot rows)
    uint32_t seg_hist = 16384;    // ... and of the last one (histogram stage, shared)

    void arm(const void *stage_, bool fresh_ = false, const Span &span_ = {}, uint32_t nseg_ = 0, uint32_t seg_ = 0, uint32_t seg_hist_ = 0)
    {
        pending = true;
        stage = stage_;
        fresh = fresh_;
        resolved = false;
        if (fresh_) {
            span = span_;
            nseg = nseg_;
            seg = seg_;
            seg_hist = seg_hist_;
        }
    }
    bool needs_resolve() const { return pending && fresh && !resolved; }
    void resolve() { resolved = true; }
    bool take()   // -> whether the finalisation that is launched now is a FRESH one
    {
        const bool was_fresh = fresh;
        pending = fresh = false;
        return was_fresh;
    }
    void clear() { pending = fresh = false; }
};

// The open by-record scan of a file (kpal_fasta_records_file_*): the range and the unfinished record carried between pieces
// (record_scan.hpp) and, when the scan is one of FASTQ reads (kpal_fastq_records_file_open), its mask and the records its
// pieces have indexed so far.
struct RecordFileScan {
    RecordScan scan;
    bool fastq = false;
    FqMask mask = {-1, 33};
    uint64_t records = 0;
};

// The roles of kpal_ctx::scratch that the distance units rely on: the table at that member.
enum { kScratchUpload = 0, kScratchBalanced = 2, kScratchTotals = 3 };

struct kpal_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;
    int num_cu = 256;
    int numa_node = -1;                      // NUMA node of the host the GPU is attached to (-1: unknown): staging buffers and copy threads go there
    // counting state
    int k = 0;
    int strategy = KPAL_STRATEGY_AUTO;
    bool counting = false;
    DevBuf table;  // int64[4^k]
    uint64_t bins = 0;
    size_t batch_bytes = (size_t)1 << 30;
    bool batch_bytes_set = false;            // KPAL_BATCH_BYTES given (else the chunked path uses its own maximum)
    uint64_t split_above = 0xFFFFFFFFull;   // two-level path: largest coarse bucket one batch may hold (32-bit offsets)
    size_t quad_pool_max = (size_t)30 << 30; // quad pipelines: largest record pool of one piece (a record store is a scalar base
                                             // + a 32-bit per-thread offset that spans 1/8 of the pool); larger pieces are halved
    // partition workspace
    DevBuf keys, cntmat, offs, bucket_start, slice_start;
    DevBuf chunk_meta, chunk_table, chunk_ovf, chunk_sorted;   // chunked one-level path
    DevBuf quad_meta, quad_meta2;            // quad path: rounds per workgroup, error word; level-2 rounds (k >= 13)
    uint32_t *quad_error_word = nullptr;
    bool chunk_error_armed = false;
    int quad_steps_forced = 0, quad_steps2_forced = 0;   // KPAL_QUAD_STEPS / KPAL_QUAD_STEPS2 at context creation (tests, A/B): tile sizes of the quad scatters
    int quad_workgroups_max = 0;             // KPAL_QUAD_WORKGROUPS (tests): the quad plans are made for this many CUs (0: the device's) -- few
                                             // scatter workgroups write long runs, the shapes the histogram's run stream is tested on
    int quad_cus() const { return quad_workgroups_max > 0 && quad_workgroups_max < num_cu ? quad_workgroups_max : num_cu; }
    bool k12_staged = true;                  // KPAL_K12_STAGED=0: the k = 12 histogram merges into the table with atomics (A/B, tests)
    bool quad_verbose = false;               // KPAL_QUAD_VERBOSE
    int quad_repeat_forced = -1;             // KPAL_QUAD_REPEAT=0 / 1: the scatter instantiation without / with the repeat lanes' shortcut (-1: by the sample)
    // what the last piece of the last feed took (kpal_count_last_plan): strategy, wave-steps per wave and tile of level 1 / level 2
    int plan_strategy = 0, plan_steps1 = 0, plan_steps2 = 0;
    // kpal_count_stats: pieces by pipeline and the FRESH pieces / re-runs, since the context was created
    uint64_t stat_fresh_pieces = 0, stat_fresh_reruns = 0, stat_quad_pieces = 0, stat_chunked_pieces = 0, stat_split_pieces = 0, stat_repeat_pieces = 0;
    QuadTileCache tiles;                     // tile sizes and verdict of the last sample of this count (kpal_count_begin clears them)
    QuadFinalize fin;                        // the pending finalisation of the last quad piece
    bool table_zero_pending = false;         // the table of this k >= 13 count has not been zeroed yet (FRESH: QuadFinalize)
    bool fresh_feed = false;                 // set by kpal_count_feed_device around count_device_range: a whole device feed
    DevBuf direct_list, direct_meta;         // TableSink segments ((index << 32) | count entries); per-segment counts + overflow word
    uint32_t direct_seg = 16384;             // entries per segment (KPAL_DIRECT_SEG: tests force the overflow path)
    bool direct_seg_forced = false;          // ... then the histogram stage's segment is as small
    bool quad_hist_unpacked = false;         // KPAL_HIST_PACKED=0: the 128 KiB histogram at every k (A/B, tests)
    int level2_mode = 2;                     // level 2 of the two-level path (KPAL_LEVEL2): 0 count + exact offsets, 1 chunked per-tile runs, 2 chunked aligned lines (default)
    alignas(16) unsigned char chunk_pool_sent[96] = {};   // (ChunkPool) what the device copy of the pool descriptor holds
    void *chunk_pool_dev = nullptr;
    uint32_t chunk_meta_y = 0;               // coarse-bucket count the meta layout was cleared for
    uint32_t *chunk_error_word = nullptr;
    DevBuf residuals, cnt1, offs1, start1;  // two-level path (k = 13..16)
    // FASTA ingest (kpal_text.hip): raw text and flattened stream of two chunks in flight, scan metadata, the flattened tail of
    // the previous chunk (the k-1 bytes the next one's first windows begin in), the chunks' flattened sizes in pinned host memory
    DevBuf fa_raw[2], fa_flat[2], fa_meta[2], fa_tail;
    // record index of the text of the last kpal_fasta_records_begin / kpal_fastq_records_begin (from_fasta_by_record, from_fastq_by_record): raw text, flattened stream, scan metadata,
    // record starts in the flattened stream (R + 1) and header offsets in the raw text (R) on the device and on the host
    DevBuf rec_raw, rec_flat, rec_meta, rec_starts, rec_hdr;
    std::vector<uint64_t> rec_starts_host, rec_hdr_host;
    uint64_t rec_n = 0, rec_nf = 0;
    // ... over a file the library reads itself (kpal_fasta_records_file_*)
    RecordFileScan rec_scan;
    // ... cut into sliding windows (kpal_fasta_windows_*): first window and first tile of every record (R + 1 values each; on
    // the device one behind the other) for the (window, step) last asked for -- a new record index clears them -- and the
    // tile tables of the call in flight
    DevBuf win_index, win_tiles;
    std::vector<uint64_t> win_first_host, win_tile_host;
    uint64_t win_window = 0, win_step = 0;
    uint64_t *fa_nflat_host = nullptr;
    // FASTQ ingest (kpal_text.hip): raw text (carried rest of the chunk before + the chunk) and flattened stream of two chunks,
    // scan metadata and newline positions of the chunk being tokenised, its status words on the device and in pinned host memory
    DevBuf fq_raw[2], fq_flat[2], fq_meta, fq_pos, fq_status;
    unsigned long long *fq_status_host = nullptr;
    hipEvent_t fq_ev = nullptr;
    // ... and the record a count's last FASTQ feed left unfinished (count_end_text ends it), with that feed's mask options
    std::vector<uint8_t> fq_carry;
    uint64_t fq_records = 0;                 // records of this count finished so far (error messages name record fq_records + r + 1)
    FqMask fq_mask = {-1, 33};
    bool fq_open = false;                    // a FASTQ feed happened since kpal_count_begin or the last end of the text: count_end_text ends it
    std::vector<void *> host_allocs;         // kpal_host_alloc buffers still owned by callers (released with the context at the latest)
    size_t fa_chunk = kStage;                // text bytes per chunk (KPAL_FASTA_CHUNK: tests put the seams everywhere)
    // host-feed staging
    static constexpr size_t kStage = (size_t)64 << 20;
    static constexpr size_t kStagePad = 64;
    void *pinned[2] = {nullptr, nullptr};
    DevBuf dstage[2];
    hipEvent_t ev_copied[2] = {nullptr, nullptr};
    hipEvent_t ev_done[2] = {nullptr, nullptr};
    bool stage_used[2] = {false, false};
    // Scratch for vector ops.  kpal_vec, kpal_sets, kpal_records, kpal_spectrum and kpal_multi use scratch[0..3] within one function;
    // the host entries of the table units fill them through table_host.hpp alone (upload_vector; for_uploaded_chunks: scratch[0]).
    // The distance units (dist_host.hpp) hold a buffer ACROSS calls into functions that take workspace themselves, by these roles.
    // ensure() frees a buffer that must grow: a callee that grew one its caller still points into would leave that pointer
    // dangling, so only the functions of the last column may ensure() a buffer, and nothing called while a pointer is held does.
    //   buffer (kScratch*) filled by                                  held across                                  ensured by
    //   scratch[Upload]    the host entries: upload_rectangle,        the whole device entry the host entry ends   those host entries alone (one pair: the
    //                      kpal_distance_matrix, upload_pair          in                                           right vector in scratch[Upload + 1])
    //   scratch[Balanced]  the device entries, before their cores:    the cores, the pair pipeline (balanced =     those device entries alone (one plain pair:
    //                      balance_sets, balanced_pair_chunk, the     true), smooth_set_pyramids, every tile of    the right copy in scratch[Balanced + 1],
    //                      tile loop of kpal_cross_nearest_device     a nearest call                               which takes no totals)
    //   scratch[Totals]    the launch functions: totals (cross_       the launches that follow in the same core    those launch functions alone; reduce_partials
    //                      option_launch, paired_chunk), pyramid      and its finish_partials; the roots as        and finish_partials never touch scratch
    //                      roots (smooth_set_pyramids), the word of   SmoothPyramids::totals until the pair or
    //                      a reciprocal form, the Gram block list     rectangle passes are reduced
    //   partials           the kernels of every launch function       cross_*_launch leave them to their caller,   the launch functions (and the cores before
    //                                                                 up to its finish_partials / reduce_partials  smooth_set_pyramids, which takes none)
    //   result             reduce_partials                            the finish kernels of a nearest tile;        finish_partials, reduce_to_result,
    //                                                                 gram_euclidean until its download            gram_euclidean
    //   opt_l, opt_r       profile_distance_pair, kpal_dynamic_smooth nothing outside those two functions          those two functions
    //   opt_levels         launch_smooth (one pair; held nowhere),    the passes over the pyramids, as             those two functions
    //                      smooth_set_pyramids                        SmoothPyramids::sums / codes
    //   opt_profiles       kpal_profile_distance_matrix's upload      the device entry it ends in                  that host entry alone
    //   near_dist, _best   kpal_cross_nearest_device                  every tile of the call                       that entry alone, before its first tile
    DevBuf scratch[4];
    DevBuf partials, result;
    // the (value, number) pairs of the last kpal_distribution_set / _set_device, table after table (kpal_spectrum.hip): what
    // kpal_distribution_fetch hands out
    std::vector<int64_t> spec_values;
    std::vector<uint64_t> spec_numbers;
    bool spec_pending = false;
    DevBuf opt_l, opt_r, opt_levels, opt_profiles;   // ProfileDistance option pipeline
    DevBuf near_dist, near_best;             // kpal_nearest.hip: the finished distances of one tile (and the word of the Gram test behind them); the n best of a band's rows
    // the canonical tile pairs of the LDS-tiled balance kernels for the k they were last built for (kpal_vec.hip: canon_tiles)
    DevBuf canon;
    std::vector<uint32_t> canon_host;
    int canon_k = 0;
    // multi-GPU (kpal_multi.hip): RCCL communicator, the stream the pipelined reduce runs on, two side buffers for it
    void *comm = nullptr;                    // ncclComm_t
    int comm_rank = 0, comm_world = 1;
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_table_copied = nullptr;
    hipEvent_t ev_side_free[2] = {nullptr, nullptr};
    bool side_used[2] = {false, false};
    DevBuf side[2];
    int side_turn = 0;
    void *merged = nullptr;                  // where the last merged table lies (the count table or a side buffer)
    uint64_t merged_bins = 0;                // ... and how many bins it has (kpal_count_begin with another k discards it)
    uint64_t merged_first = 0;               // ... and which bin its first one is (bin-range merge: a rank holds its range only)
    DevBuf xsend, xrecv;                     // the packed blocks of the mirror exchange (kpal_comm_reduce_scatter_table)
    // profiling
    bool prof = false;
    std::vector<std::string> prof_names;
    std::vector<double> prof_ms;
    std::vector<uint64_t> prof_launches;
    std::vector<ProfRec> prof_pending;
    std::vector<hipEvent_t> ev_pool;
    uint64_t prof_dropped = 0;               // launches whose timing events could not be recorded
};


int ensure(kpal_ctx *ctx, DevBuf &b, size_t bytes);
int prof_name_id(kpal_ctx *ctx, const char *name);
hipEvent_t prof_event(kpal_ctx *ctx);
int prof_collect(kpal_ctx *ctx);

struct ProfScope {
    kpal_ctx *ctx;
    ProfRec rec;
    bool on;
    ProfScope(kpal_ctx *c, const char *name) : ctx(c), on(c->prof)
    {
        if (on) {
            rec.name = prof_name_id(c, name);
            rec.a = prof_event(c);
            rec.b = prof_event(c);
            // a launch that cannot be timed is still launched: the pair is dropped, the failure is counted
            if (!rec.a || !rec.b || hipEventRecord(rec.a, c->stream) != hipSuccess) drop();
        }
    }
    void drop()
    {
        on = false;
        ++ctx->prof_dropped;
        if (rec.a) ctx->ev_pool.push_back(rec.a);
        if (rec.b) ctx->ev_pool.push_back(rec.b);
    }
    ~ProfScope()
    {
        if (on) {
            if (hipEventRecord(rec.b, ctx->stream) == hipSuccess) ctx->prof_pending.push_back(rec);
            else drop();
        }
    }
};

#define LAUNCH(ctx, name, kernel, grid, block, ...)                                       \
    do {                                                                                  \
        {                                                                                 \
            ProfScope ps_(ctx, name);                                                     \
            hipLaunchKernelGGL(kernel, grid, block, 0, (ctx)->stream, __VA_ARGS__);       \
        }                                                                                 \
        HIPCHK(hipGetLastError());                                                        \
    } while (0)

#define CASE_K(N, ...)           \
    case N: {                    \
        constexpr int K = N;     \
        __VA_ARGS__;             \
    } break;

#define DISPATCH_K_1_16(k, ...)                                                                            \
    switch (k) {                                                                                            \
        CASE_K(1, __VA_ARGS__) CASE_K(2, __VA_ARGS__) CASE_K(3, __VA_ARGS__) CASE_K(4, __VA_ARGS__) CASE_K(5, __VA_ARGS__) CASE_K(6, __VA_ARGS__)     \
        CASE_K(7, __VA_ARGS__) CASE_K(8, __VA_ARGS__) CASE_K(9, __VA_ARGS__) CASE_K(10, __VA_ARGS__) CASE_K(11, __VA_ARGS__) CASE_K(12, __VA_ARGS__) \
        CASE_K(13, __VA_ARGS__) CASE_K(14, __VA_ARGS__) CASE_K(15, __VA_ARGS__) CASE_K(16, __VA_ARGS__)                                 \
    default:                                                                                                \
        return set_err(KPAL_E_INVALID, "k=%d out of range 1..%d", k, KPAL_MAX_K);                           \
    }

#define DISPATCH_K_1_7(k, ...)                                                                         \
    switch (k) {                                                                                        \
        CASE_K(1, __VA_ARGS__) CASE_K(2, __VA_ARGS__) CASE_K(3, __VA_ARGS__) CASE_K(4, __VA_ARGS__) CASE_K(5, __VA_ARGS__) CASE_K(6, __VA_ARGS__) \
        CASE_K(7, __VA_ARGS__)                                                                                 \
    default:                                                                                            \
        return set_err(KPAL_E_INVALID, "LDS-direct strategy needs k <= 7 (k=%d)", k);                   \
    }

#define DISPATCH_K_13_16(k, ...)                                                                   \
    switch (k) {                                                                                   \
        CASE_K(13, __VA_ARGS__) CASE_K(14, __VA_ARGS__) CASE_K(15, __VA_ARGS__) CASE_K(16, __VA_ARGS__) \
    default:                                                                                       \
        return set_err(KPAL_E_INVALID, "two-level partition strategy needs 13 <= k <= 16 (k=%d)", k); \
    }

#define DISPATCH_K_12_16(k, ...)                                                                   \
    switch (k) {                                                                                   \
        CASE_K(12, __VA_ARGS__) CASE_K(13, __VA_ARGS__) CASE_K(14, __VA_ARGS__) CASE_K(15, __VA_ARGS__) CASE_K(16, __VA_ARGS__) \
    default:                                                                                       \
        return set_err(KPAL_E_INVALID, "staged quad histograms need 12 <= k <= 16 (k=%d)", k);     \
    }

#define DISPATCH_K_8_16(k, ...)                                                                   \
    switch (k) {                                                                                   \
        CASE_K(8, __VA_ARGS__) CASE_K(9, __VA_ARGS__) CASE_K(10, __VA_ARGS__) CASE_K(11, __VA_ARGS__) CASE_K(12, __VA_ARGS__)         \
        CASE_K(13, __VA_ARGS__) CASE_K(14, __VA_ARGS__) CASE_K(15, __VA_ARGS__) CASE_K(16, __VA_ARGS__)                               \
    default:                                                                                       \
        return set_err(KPAL_E_INVALID, "quad partition needs 8 <= k <= 16 (k=%d)", k);             \
    }

#define DISPATCH_K_8_12(k, ...)                                                                   \
    switch (k) {                                                                                   \
        CASE_K(8, __VA_ARGS__) CASE_K(9, __VA_ARGS__) CASE_K(10, __VA_ARGS__) CASE_K(11, __VA_ARGS__) CASE_K(12, __VA_ARGS__)         \
    default:                                                                                       \
        return set_err(KPAL_E_INVALID, "partition strategy needs 8 <= k <= 12 (k=%d)", k);         \
    }

#define CTX_ENTER(ctx)                                            \
    if (!(ctx)) return set_err(KPAL_E_INVALID, "ctx is NULL");    \
    HIPCHK(hipSetDevice((ctx)->device))


inline unsigned stream_grid(kpal_ctx *ctx, uint64_t n_items, unsigned block = 256)
{
    const uint64_t want = (n_items + block - 1) / block;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)ctx->num_cu * 8));
}

// ----------------------------------------------------------------------------------------------
// host functions shared between the units
// ----------------------------------------------------------------------------------------------
constexpr int kQuadsUseChunked = 2;   // launch_partition*_quads (AUTO): the sample shows a feed for the round-1 pipeline
constexpr int kSplitBatch = 1;        // launch_partition2 / launch_partition*_quads: the caller halves the piece
int launch_partition_quads(kpal_ctx *ctx, const Span &s);                 // kpal_quads.hip
int launch_partition2_quads(kpal_ctx *ctx, const Span &s, bool fresh = false);   // kpal_quads2.hip
struct QuadMeta {   // kpal_ctx::quad_meta
    uint32_t *nrounds;   // rounds per (level-1) scatter workgroup
    uint32_t *error;     // the error word and the three statistics words behind it
    uint32_t *load;      // the counters of the row-load sample
};
int quad_meta(kpal_ctx *ctx, QuadMeta *out);                              // kpal_quads.hip: that buffer exists, the error word is armed
int quad_choose_steps(kpal_ctx *ctx, const Span &s, uint32_t *load, int buckets, int slots, const int *candidates, size_t n_candidates,
                      int *steps_out, std::vector<double> *fine = nullptr);   // kpal_quads.hip: sample a piece; ctx->tiles.hot_rows and the level-1 size (or kQuadsUseChunked)
int quad2_finalize(kpal_ctx *ctx, bool balance);                          // kpal_quads2.hip: no-op unless a finalisation is pending
int quad2_resolve_fresh(kpal_ctx *ctx);                                   // kpal_quads2.hip: a FRESH piece whose lists overflowed is counted again (the fed buffer is read)
Span make_span(const uint8_t *addr, size_t n, size_t halo);               // kpal_count.hip: the k-mers ending in [addr, addr + n), `halo` readable bytes of the same feed left of addr
int count_device_range(kpal_ctx *ctx, const uint8_t *addr, size_t n, size_t halo, int strategy = -1, size_t batch_bytes = 0);   // kpal_count.hip: a device range into the running count (strategy / batch_bytes: its own re-counts only)
int ensure_pinned(kpal_ctx *ctx);                                         // kpal_count.hip: the two pinned staging buffers exist
int pinned_wait(kpal_ctx *ctx, int slot);                                 // kpal_count.hip: before ctx->pinned[slot] is written
int pinned_h2d(kpal_ctx *ctx, int slot, void *dst, const void *src, size_t n);   // kpal_count.hip: the DMA out of ctx->pinned[slot]
void staged_memcpy(void *dst, const void *src, size_t n);                 // kpal_count.hip: host copy into a staging buffer on several cores
int fa_flatten(kpal_ctx *ctx, const uint8_t *raw, uint64_t m, int state, int tail, uint8_t *flat, void *meta, uint64_t **offs_out,
               void **rest = nullptr);                                    // kpal_text.hip: the FASTA flattening of raw[0, m) into flat
int open_text_range(const char *path, uint64_t begin, uint64_t end, FaSource &src);   // kpal_text.hip: a byte range of a regular file, opened for sequential reading
// kpal_text.hip: the FASTQ tokeniser (fastq_kernels.hpp is compiled there alone), for the count path and the record index
int fq_mask_options(const kpal_fastq_options *opt, FqMask &m);           // the mask of a FASTQ call, checked (min_quality -1: none)
int fq_tokenise(kpal_ctx *ctx, const uint8_t *raw, uint64_t n, bool fin, FqMask m, uint8_t *flat);   // one FASTQ chunk on the device -> flat stream, newline positions (fq_pos), status words
int fq_tokenise_wait(kpal_ctx *ctx, uint64_t records, const unsigned long long **status);   // the status words of that chunk on the host; a malformed record is the error
int fq_title_offsets(kpal_ctx *ctx, uint64_t R, uint64_t *dev_title);    // where the title lines of the R records that chunk finishes begin (device, queued)
int fq_chunk_too_long(uint64_t records);                                  // kpal_text.hip: the error of a FASTQ chunk of 4 GiB
void fq_reset(kpal_ctx *ctx);                                             // kpal_text.hip: the unfinished FASTQ record of a count is dropped
int count_end_text(kpal_ctx *ctx);                                        // kpal_text.hip: an open FASTQ text is ended (its carried record counted, or the count abandoned)
int table_ready(kpal_ctx *ctx);                                           // kpal_quads2.hip: zeros materialised, pending finalisation done: the table is the table
int launch_balance(kpal_ctx *ctx, int k, const int64_t *in, int64_t *out);   // kpal_vec.hip
int canon_tiles(kpal_ctx *ctx, int k, int per_cu, const uint32_t **list, uint32_t *count, unsigned *grid);   // kpal_vec.hip: the canonical tile pairs of the LDS-tiled balance family (k >= 6), the grid for per_cu workgroups on a CU
int balance_set_launch(kpal_ctx *ctx, int k, size_t n_tables, const int64_t *dev_in, int64_t *dev_out);   // kpal_transform.hip: the one launch behind kpal_balance_set_device (nothing checked)
int distance_matrix_core(kpal_ctx *ctx, int P, uint64_t n, const int64_t *prof, int metric, double *out_lower, bool allreduce,
                         int tiled = -1);   // kpal_cross.hip (tiled: -1 decided from n; 0 / 1 agreed between the ranks)
int reduce_partials(kpal_ctx *ctx, const Partial *partials, uint32_t nq, uint32_t nblocks, Partial *out);   // kpal_vec.hip: nq groups of nblocks device partials added in a fixed order
int finish_partials(kpal_ctx *ctx, uint32_t nq, uint32_t nblocks, std::vector<Partial> &out, bool allreduce = false);   // kpal_vec.hip: reduce nq groups of nblocks partials, fetch them
double finish_value(int metric, const Partial &p, int64_t *aux);         // kpal_vec.hip: the distance of one reduced partial of a plain metric (aux: its count / wrapping dot)
int comm_allreduce_partials(kpal_ctx *ctx, Partial *dev_partials, size_t count);   // kpal_multi.hip: partials added over the ranks, in place
