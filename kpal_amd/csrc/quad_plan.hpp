// quad_plan.hpp -- what the host decides before it launches a quad record pipeline (kpal_quads.hip, k = 8..12; kpal_quads2.hip,
// k = 13..16): the grid of the row-load sample and its verdict, the tile sizes from the queue model, the tile sizes kept for the
// next feeds of a count, and the geometry of the launches (tiles, workgroups, record pools).  No GPU in it: the two launchers and
// a CPU program (tests/test_quad_plan_host.py) read the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

namespace kpal {

constexpr int kQuadRowWords = 32768;          // 128 KiB of rows (quad_kernels.hpp: the LDS of a scatter workgroup)
constexpr int kQuadPackedRecordBytes = 192;   // a level-2 record: 64 items of 23 bits (quad_kernels.hpp: quad_pack3)
constexpr double kQuadBacklogMax = 1500.0;    // expected steady-state backlog a tile size may bring (spill list: 2048 entries)
constexpr int kQuadWaves = 16;                // waves of a scatter workgroup, level 1 and level 2
constexpr int kQuadHotRows = 32;              // rows the queue model leaves to the hot-item table
constexpr int kQuadFineRows = 512;            // rows of level 2

// Expected number of items in the spill list of a workgroup in the steady state.  A row is a queue: Poisson(mu) items
// arrive per round, `slots` leave with the record, the rest is carried to the next round.  The single-round overflow
// E[max(X - slots, 0)] underestimates the backlog of a well-filled row (carried items arrive again: at 83 % fill of a
// 16-slot row the backlog is twice the overflow, at 95 % six times; a row whose load exceeds its slots grows without
// bound until the list is full and the slow direct path takes over -- measured 2x slower on AT-rich input with tiles
// chosen by the single-round figure).  backlog = overflow x r(fill, slots), r tabulated from a simulation of the queue
// (tools/diag/spill_queue.py).
inline double quad_expected_backlog(const std::vector<double> &mu, int slots)
{
    static const double rho_grid[10] = {0.5, 0.6, 0.7, 0.75, 0.8, 0.85, 0.9, 0.925, 0.95, 0.975};
    static const double ratio[4][10] = {
        {1.02, 1.08, 1.25, 1.43, 1.70, 2.19, 3.21, 4.24, 6.34, 12.7},   // 16 slots
        {1.00, 1.01, 1.08, 1.17, 1.33, 1.65, 2.34, 3.05, 4.52, 8.9},    // 32
        {1.00, 1.00, 1.01, 1.04, 1.12, 1.30, 1.75, 2.24, 3.25, 6.35},   // 64
        {1.00, 1.00, 1.00, 1.02, 1.02, 1.10, 1.36, 1.68, 2.37, 4.55}};  // 128
    const int ti = slots <= 24 ? 0 : (slots <= 32 ? 1 : (slots <= 64 ? 2 : 3));   // (20 slots: the 16-slot row of the table, on the safe side)
    double total = 0.0;
    // mu is sorted: rows whose load lies within 1 % of each other are evaluated once, at their mid-point (this runs
    // on the host inside every large feed: 2048 Poisson tails per candidate cost 0.6 ms of a 12 ms step)
    for (size_t at = 0; at < mu.size();) {
        size_t end = at + 1;
        while (end < mu.size() && mu[end] <= mu[at] * 1.01) ++end;
        const double m = 0.5 * (mu[at] + mu[end - 1]), weight = (double)(end - at);
        at = end;
        if (m <= 0.0) continue;
        const double rho = m / slots;
        if (rho >= 0.995) {   // the row cannot keep up
            total += 1e6 * weight;
            continue;
        }
        // E[max(X - c, 0)] = sum_{x > c} (x - c) p(x); p by recurrence from p(0) = exp(-m)
        double p = std::exp(-m), acc = 0.0;
        const int upto = (int)(m + 12.0 * std::sqrt(m) + 40.0);
        for (int x = 1; x <= upto; ++x) {
            p *= m / x;
            if (x > slots) acc += (x - slots) * p;
        }
        double r = 1.0;
        if (rho >= rho_grid[9]) {
            r = ratio[ti][9];
            acc = std::max(acc * r, m / (2.0 * (slots - m)));   // heavy traffic
            r = 1.0;
        } else if (rho > rho_grid[0]) {
            int j = 0;
            while (rho > rho_grid[j + 1]) ++j;
            const double f = (rho - rho_grid[j]) / (rho_grid[j + 1] - rho_grid[j]);
            r = ratio[ti][j] + f * (ratio[ti][j + 1] - ratio[ti][j]);
        }
        total += acc * r * weight;
    }
    return total;
}

// The grid of quad_sample_kernel over a piece of total_steps wave-steps: `groups` workgroups of eight waves, `stride` wave-steps
// apart, each wave reading sample_steps of them -- about 1/64 of the piece, 32 KiB per workgroup, at most 1024 workgroups.
struct QuadSampleGrid {
    uint32_t groups;
    uint64_t stride;
    uint32_t sample_steps;    // per wave
    uint64_t sampled_steps;   // wave-steps the row loads are divided by
};

inline QuadSampleGrid quad_sample_grid(uint64_t total_steps)
{
    QuadSampleGrid g;
    g.sample_steps = 4;
    const uint64_t want = std::max<uint64_t>(1, total_steps / (64ull * 8 * g.sample_steps));
    g.groups = (uint32_t)std::min<uint64_t>(want, 1024);
    g.stride = std::max<uint64_t>(8 * g.sample_steps, total_steps / g.groups);
    g.sampled_steps = std::min<uint64_t>((uint64_t)g.groups * 8 * g.sample_steps, total_steps);
    return g;
}

// What a sample says about its feed.
struct QuadVerdict {
    std::vector<double> loads;   // items per row per wave-step, sorted, without the 32 fullest rows
    std::vector<double> fine;    // ... per fine row of level 2, sorted (all 512; empty on one level)
    bool use_chunked;            // AUTO: the feed goes to the round-1 pipeline
    double budget;               // backlog the level-1 tile may bring
    bool hot_rows;               // the scatter takes its REPEAT instantiation
    double hot_percent;          // the excess of the 32 fullest rows over the median row, in % of all items
    double top3_percent;         // ... and how much of that excess sits in the three fullest rows
};

// rows: the `buckets` row loads of the sample; fine: the 512 fine-row loads of the two-level sample, or null; repeat_items: the
// items of repeat lanes (they are not in the row loads: the scatter sends them past the rows); sampled_steps >= 1.
inline QuadVerdict quad_sample_verdict(const uint32_t *rows, int buckets, const uint32_t *fine, uint32_t repeat_items, uint64_t sampled_steps,
                                       bool is_auto)
{
    QuadVerdict v;
    const double steps = (double)sampled_steps;
    std::vector<double> &per_step = v.loads;
    per_step.resize((size_t)buckets);
    for (int b = 0; b < buckets; ++b) per_step[b] = rows[b] / steps;
    if (fine) {
        v.fine.resize(kQuadFineRows);
        for (int b = 0; b < kQuadFineRows; ++b) v.fine[b] = fine[b] / steps;
        std::sort(v.fine.begin(), v.fine.end());
    }
    std::sort(per_step.begin(), per_step.end());
    // the 32 fullest rows are left out: a handful of very hot rows (poly-A, an adapter shared by every read) cannot be
    // helped by smaller tiles -- their items are counted in the workgroup's hot-item table instead.
    // When those hot rows hold more than 1.5 % of all items (reads that share an adapter / primer prefix, several
    // per cent of low-complexity reads) the slow path of the scatter would run in nearly every placement step --
    // measured 20-50x slower on a 20..40-base prefix shared by all reads.  The round-1 pipelines take such a feed
    // in their stride (their buckets simply own more chunks), so AUTO hands the feed over; an explicitly chosen quad
    // strategy stays (tests, A/B).
    double all = 0.0, hot = 0.0;
    const double median = per_step[(size_t)buckets / 2];
    for (int b = 0; b < buckets; ++b) all += per_step[b];
    for (int b = buckets - kQuadHotRows; b < buckets; ++b) hot += std::max(0.0, per_step[b] - median);
    // ... unless nearly all of that excess sits in one to three rows (a homopolymer run, a two-letter repeat): then a
    // wave's hot items are all the same, one ballot round counts them into the workgroup's hot-item table, and the
    // quad path is the faster one (homopolymer feed: 520 vs 230 Gbases/s).  A shared prefix spreads over a dozen rows.
    double top3 = 0.0;
    for (int b = buckets - 3; b < buckets; ++b) top3 += std::max(0.0, per_step[b] - median);
    const bool concentrated = top3 >= 0.8 * hot;
    v.hot_percent = all > 0.0 ? 100.0 * hot / all : 0.0;
    v.top3_percent = hot > 0.0 ? 100.0 * top3 / hot : 0.0;
    v.use_chunked = is_auto && all > 0.0 && hot > 0.015 * all && !concentrated;
    // hot rows fill the spill list first (their excess is carried every round before it is counted directly): the
    // ordinary rows then get a quarter of the list (k = 13, 2 % low-complexity reads: level 1 0.55 instead of 2.9 ms)
    const bool hot_excess = all > 0.0 && hot > 0.003 * all;
    v.budget = hot_excess ? kQuadBacklogMax / 4 : kQuadBacklogMax;
    // the scatter takes its REPEAT instantiation when the sample holds repeat lanes or hot rows of another kind
    const double repeats = repeat_items / steps;
    v.hot_rows = hot_excess || repeats > 0.001 * (all + repeats);
    per_step.resize((size_t)buckets - kQuadHotRows);
    return v;
}

// Level-1 tile size (wave-steps per wave per tile): the first of `candidates` (largest first) whose expected backlog over the
// sorted `loads` stays within `budget`, else the last.  backlog[i] is the figure of candidates[i] for the `tried` that were evaluated.
constexpr size_t kQuadMaxCandidates = 8;
struct QuadWalk {
    int steps;
    size_t tried;
    double backlog[kQuadMaxCandidates];
};

inline QuadWalk quad_walk_level1(const std::vector<double> &loads, int slots, const int *candidates, size_t n_candidates, double budget)
{
    QuadWalk w = {candidates[n_candidates - 1], 0, {}};
    std::vector<double> mu(loads.size());
    for (size_t ci = 0; ci < n_candidates && ci < kQuadMaxCandidates; ++ci) {
        const int c = candidates[ci];
        for (size_t b = 0; b < mu.size(); ++b) mu[b] = loads[b] * kQuadWaves * c;
        w.backlog[ci] = quad_expected_backlog(mu, slots);
        w.tried = ci + 1;
        if (w.backlog[ci] <= budget) {
            w.steps = c;
            break;
        }
    }
    return w;
}

// Level-2 tile size: 16 waves x steps2 KiB of level-1 records.  A wave-step of records holds 256 item slots, filled to
// f1 = (items of a level-1 tile) / 32768; a fine row (512 rows of 64 slots) receives its share of them.  Same queue
// model as level 1 (the 32 fullest fine rows are left to the spill list and the hot-item table), always the full budget.
// `fine`: QuadVerdict::fine.
constexpr int kQuadCandidates2[] = {8, 7, 6, 4, 3, 2};

inline int quad_walk_level2(const std::vector<double> &fine, int steps1)
{
    double all = 0.0;
    for (double v : fine) all += v;
    const double f1 = std::min(1.0, all * 16.0 * steps1 / (double)kQuadRowWords);
    std::vector<double> mu(fine.size() > (size_t)kQuadHotRows ? fine.size() - kQuadHotRows : 0);
    for (int c : kQuadCandidates2) {
        for (size_t b = 0; b < mu.size(); ++b) mu[b] = all > 0.0 ? fine[b] / all * (256.0 * f1) * kQuadWaves * c : 0.0;
        if (quad_expected_backlog(mu, 64) <= kQuadBacklogMax) return c;
    }
    return 2;
}

// `forced` if it is one of the candidates, else 0 (KPAL_QUAD_STEPS / KPAL_QUAD_STEPS2: any other number forces nothing).
inline int quad_forced_steps(int forced, const int *candidates, size_t n_candidates)
{
    for (size_t i = 0; i < n_candidates; ++i)
        if (candidates[i] == forced) return forced;
    return 0;
}

// The tile sizes chosen from the sample of an earlier feed of this count: a file streamed in many feeds is sampled once per
// 16 feeds of about the same size, not once per feed (the sample costs a D2H copy + a host synchronisation).
// kpal_count_begin clears it, and k is fixed until then: a one-level count stores level 1 only, a two-level count both.
struct QuadTileCache {
    int steps1 = 0, steps2 = 0;
    uint32_t uses = 0;
    size_t bytes = 0;
    bool hot_rows = false;   // the verdict of the last sample of this count (also of one whose piece was then split or refused)

    // a feed of feed_bytes takes the kept sizes (and uses them up once): kept for every level, used less than 16 times, the
    // feed at most twice and at least half the sampled one
    bool hit(size_t feed_bytes, int levels)
    {
        if (!steps1 || (levels == 2 && !steps2) || uses >= 16 || feed_bytes > 2 * bytes || 2 * feed_bytes < bytes) return false;
        ++uses;
        return true;
    }
    void store(int s1, int s2, size_t feed_bytes)
    {
        steps1 = s1;
        steps2 = s2;
        uses = 0;
        bytes = feed_bytes;
    }
    void clear() { *this = QuadTileCache(); }
};

// The scatter of a piece: its tile size and whether it is the REPEAT instantiation (repeat lanes go straight to the hot-item table).
struct QuadTile {
    int steps;
    bool repeat;
    bool counted;   // the piece counts as a REPEAT piece in kpal_count_stats
};

// One level.  `steps` is the forced, kept or sampled size; `sampled`: it comes from a sample taken for this piece; hot_rows:
// QuadTileCache::hot_rows; steps_forced / repeat_forced: KPAL_QUAD_STEPS (0: none) and KPAL_QUAD_REPEAT (-1: none) as given.
//   * A forced size takes no sample, so REPEAT is on (the instantiation that knows repeats) unless KPAL_QUAD_REPEAT says
//     otherwise -- and so it is for a kept size while KPAL_QUAD_STEPS holds a number that is no candidate.
//   * There is no REPEAT instantiation of the 7-step tile (it would spill registers): REPEAT takes six steps, unless
//     KPAL_QUAD_STEPS is set -- then seven steps run without the shortcut.
//   * A piece counts as REPEAT when `repeat && steps != 7`.
inline QuadTile quad1_tile(int steps, bool sampled, bool hot_rows, int steps_forced, int repeat_forced)
{
    bool repeat = (sampled || !steps_forced) ? hot_rows : true;
    if (repeat_forced >= 0) repeat = repeat_forced != 0;
    if (repeat && steps == 7 && !steps_forced) steps = 6;
    return {steps, repeat, repeat && steps != 7};
}

// Two levels, level 1.  forced1: quad_forced_steps of {8, 7, 6, 3}; chosen: the kept or sampled size.
//   * A forced size still samples when nothing is kept: steps2 needs the sample.
//   * REPEAT is the LAST sample's verdict (hot_rows), also when the sizes were kept, unless KPAL_QUAD_REPEAT is set.
//   * Seven steps stay seven: their scatter runs without the shortcut (and the piece does not count as REPEAT), level 2 with it.
inline QuadTile quad2_tile1(int forced1, int chosen, bool hot_rows, int repeat_forced)
{
    const int steps1 = forced1 ? forced1 : chosen;
    const bool repeat1 = repeat_forced >= 0 ? repeat_forced != 0 : hot_rows;
    return {steps1, repeat1, repeat1 && steps1 != 7};
}

// One level: `tiles` of 16 x steps wave-steps over G workgroups (one per CU), tpb tiles (= flush rounds) each; every round
// writes all rows, 128 KiB per workgroup.  too_large: tpb does not fit the 24 bits the kernel has for it.
struct Quad1Geometry {
    bool too_large;
    uint64_t tiles;
    uint32_t G;
    uint64_t tpb;
    size_t pool_bytes;
};

inline Quad1Geometry quad1_geometry(uint64_t total_steps, int steps, int num_cu)
{
    Quad1Geometry g = {};
    const uint64_t tile_steps = (uint64_t)kQuadWaves * steps;
    g.tiles = (total_steps + tile_steps - 1) / tile_steps;
    g.G = (uint32_t)std::min<uint64_t>((uint64_t)num_cu, g.tiles);
    g.tpb = (g.tiles + g.G - 1) / g.G;
    g.too_large = g.tpb > 0xFFFFFFull;
    g.pool_bytes = (size_t)kQuadRowWords * 4 * g.G * g.tpb;
    return g;
}

// Two levels: the rows of level 1 are NB1 coarse buckets x REP replicas, 256 rows of S1 = 128 slots (1024 of 32 at k = 16).
struct Quad2Rows {
    uint32_t NB1, REP, S1;
};

inline Quad2Rows quad2_rows(int k)
{
    Quad2Rows r;
    r.NB1 = 1u << (2 * k - 22);
    r.REP = r.NB1 >= 256 ? 1u : 256u / r.NB1;
    r.S1 = (uint32_t)kQuadRowWords / (r.NB1 * r.REP);
    return r;
}

// Two levels, level 1: tiles1 tiles of 16 x steps1 wave-steps over
// G1 <= 256 workgroups, tpb1 each.  cap1 is the capacity (stride) of a workgroup's run of records per row: tpb1 + 1 (the tail
// round of what the last tile carried over), rounded up so that a unit of level 2 is a whole number of KiB -- a wave-step of
// quad2_scatter_kernel then never straddles two units.  too_large: tpb1 does not fit 16 bits.
struct Quad2Level1 {
    bool too_large;
    uint32_t NB1, REP, S1;
    uint64_t tiles1;
    uint32_t G1;
    uint64_t tpb1, cap1;
    size_t pool1_bytes;
};

inline Quad2Level1 quad2_level1(int k, uint64_t total_steps, int steps1, int num_cu)
{
    Quad2Level1 g = {};
    const Quad2Rows r = quad2_rows(k);
    g.NB1 = r.NB1;
    g.REP = r.REP;
    g.S1 = r.S1;
    const uint64_t tile_steps = (uint64_t)kQuadWaves * steps1;
    g.tiles1 = (total_steps + tile_steps - 1) / tile_steps;
    g.G1 = (uint32_t)std::min<uint64_t>((uint64_t)std::min(num_cu, 256), g.tiles1);
    g.tpb1 = (g.tiles1 + g.G1 - 1) / g.G1;
    g.too_large = g.tpb1 > 0xFFFFull;
    const uint64_t per_kib = 1024 / (g.S1 * 4);   // records per KiB: 2 (8 at k = 16)
    g.cap1 = (g.tpb1 + 1 + per_kib - 1) / per_kib * per_kib;
    g.pool1_bytes = (size_t)kQuadRowWords * 4 * g.G1 * g.cap1;
    return g;
}

// Two levels, level 2: ~4 workgroups per CU in total; workgroup (g2, c) takes `upw` of the REP x G1 units (unit_cap bytes each) of
// coarse bucket c in tiles2 tiles of 16 x steps2 KiB, cap2 rounds (its tiles + the tail round); its records are 64 items packed
// into 192 bytes.  nseg: the list segments of a FRESH piece, one per scatter workgroup (level 1: G1, level 2: G2 x NB1) and one
// shared by the histogram stage.  too_large: a workgroup's input does not fit a 32-bit offset (whatever steps2 is).
struct Quad2Level2 {
    bool too_large;
    uint32_t units, G2, upw;
    uint64_t unit_cap, tiles2, cap2;
    size_t pool2_bytes;
    uint32_t nseg;
};

inline Quad2Level2 quad2_level2(const Quad2Level1 &l1, int steps2, int num_cu)
{
    Quad2Level2 g = {};
    g.units = l1.REP * l1.G1;
    g.G2 = std::max<uint32_t>(1, std::min<uint32_t>(g.units, (uint32_t)num_cu * 4 / l1.NB1));
    g.upw = (g.units + g.G2 - 1) / g.G2;
    g.G2 = (g.units + g.upw - 1) / g.upw;
    g.unit_cap = l1.cap1 * l1.S1 * 4;
    g.too_large = (uint64_t)g.upw * g.unit_cap >= (1ull << 32);
    const uint64_t tile2_bytes = (uint64_t)kQuadWaves * steps2 * 1024;
    g.tiles2 = ((uint64_t)g.upw * g.unit_cap + tile2_bytes - 1) / tile2_bytes;
    g.cap2 = g.tiles2 + 1;
    g.pool2_bytes = (size_t)kQuadFineRows * kQuadPackedRecordBytes * l1.NB1 * g.G2 * g.cap2;
    g.nseg = l1.G1 + g.G2 * l1.NB1 + 1;
    return g;
}

}  // namespace kpal
