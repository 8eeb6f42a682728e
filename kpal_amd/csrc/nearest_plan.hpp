// nearest_plan.hpp -- what the host decides before it takes the nearest n right profiles of every left profile
// (kpal_cross_nearest[_device], kpal_nearest.hip): the order of the candidates, which family of rectangle kernels an option set
// takes, and the tiles a Q x R rectangle is cut into so that every tile passes the 32-bit limit of the partials
// (partials_too_many) and keeps its workspace within a budget.  No GPU in it: kpal_nearest.hip, the selection kernel
// (nearest_kernels.hpp: the order) and a CPU program (tests/test_nearest_plan_host.py) read the same definitions.
#pragma once
#include "matrix_plan.hpp"

namespace kpal {

// ---- the order ------------------------------------------------------------------------------------------------------------
// One candidate of a left profile: its distance and the GLOBAL index of the right profile (index < 0: no candidate).
struct NearestCand {
    double dist;
    int64_t index;
};

// a precedes b: the row order of kdistlib.nearest -- np.argsort(kind='stable'): ascending distance, equal distances (+0 and
// -0 are equal) by the lower index, NaN behind every number, NaNs among themselves by index.
KPAL_MATRIX_HD bool nearest_before(const NearestCand &a, const NearestCand &b)
{
    if (a.dist < b.dist) return true;
    if (b.dist < a.dist) return false;
    const bool a_nan = a.dist != a.dist, b_nan = b.dist != b.dist;
    if (a_nan != b_nan) return b_nan;
    return a.index < b.index;
}

// ... with "no candidate" behind every candidate.
KPAL_MATRIX_HD bool nearest_better(const NearestCand &a, const NearestCand &b)
{
    if (a.index < 0) return false;
    return b.index < 0 || nearest_before(a, b);
}

// The best n of `have` candidates in order (best) and `count` new ones, on the host: what the selection kernel does for one
// row of one tile, for the option sets whose tiles are computed into a host buffer (dynamic smoothing).  Returns how many of
// best[0, n) are candidates afterwards.
inline int nearest_merge_host(NearestCand *best, int have, int n, const double *dist, int64_t count, int64_t first_index)
{
    std::vector<NearestCand> all(best, best + have);
    all.reserve((size_t)have + (size_t)count);
    for (int64_t r = 0; r < count; ++r) all.push_back(NearestCand{dist[r], first_index + r});
    const size_t keep = std::min<size_t>((size_t)n, all.size());
    std::partial_sort(all.begin(), all.begin() + keep, all.end(), nearest_before);
    std::copy(all.begin(), all.begin() + keep, best);
    return (int)keep;
}

// ---- which kernels --------------------------------------------------------------------------------------------------------
// The family of an option set and the (s, m) groups it keeps per slot of a pair in the partials.
enum NearestRoute {
    kNearestPlain = 0,    // 'prod' / 'sum': cross_pairs, one group per slot
    kNearestGram = 1,     // plain euclidean: the Gram layout when the tile is staged, else (or when it is inexact) cross_pairs
    kNearestOption = 2,   // positive / scale / cosine: option_nacc_max groups per slot
    kNearestSmooth = 3,   // dynamic smoothing: the existing cores into a host buffer of one tile (2 * option_nacc groups)
};
struct NearestKind {
    int route;
    uint32_t groups_per_slot;
};
inline NearestKind nearest_kind(const kpal_distance_options *opt)
{
    if (opt->do_smooth) return NearestKind{kNearestSmooth, option_nacc(opt->metric) * 2u};
    if (options_plain(opt)) return NearestKind{opt->metric == KPAL_EUCLIDEAN ? kNearestGram : kNearestPlain, 1u};
    return NearestKind{kNearestOption, option_nacc_max(opt->metric, opt->do_scale != 0, opt->do_positive != 0)};
}

// ---- tiles ----------------------------------------------------------------------------------------------------------------
// Workspace of one tile unless the caller says otherwise.  The partials of a staged tile are 128 bytes per pair (8 workgroup
// partials of 16 bytes), its reduced results 16 and its finished distances 8: 4 GiB hold some 28 million pairs, about 10 ms of
// the rectangle kernel at k = 6 and more at every larger k, against which the fixed dozen launches and the one small download
// of a tile no longer count; and 4 GiB next to two resident sets of up to 32 GiB each (kdistlib.CROSS_MAX_BYTES) leave most of
// the 288 GB of an MI355X to the caller.  (The entries without tiles allow up to 32 GiB of partials, their 32-bit limit.)
constexpr uint64_t kNearestBudgetBytes = 4ULL << 30;

// What one tile of tq x tr profiles needs: whether every pass it may take passes partials_too_many, and the bytes of its
// partials, its reduced results, the totals of a scaled option set and its tq x tr finished distances.
struct NearestCost {
    bool indexable;
    uint64_t bytes;
};
inline NearestCost nearest_tile_cost(uint64_t bins, int num_cu, const NearestKind &kind, int tq, int tr)
{
    const CrossSets c = {nullptr, nullptr, tq, tr, bins, 0};
    const bool staged = cross_staged(tq, tr, bins);
    const CrossGrid g = cross_grid(num_cu, c, staged);
    const uint64_t nprof = (uint64_t)tq + (uint64_t)tr;
    uint64_t groups = g.slots * kind.groups_per_slot;
    bool indexable = !partials_too_many(groups, g.gx);
    uint64_t partials = groups * g.gx, results = groups, extra = 0;
    if (kind.route == kNearestGram && staged) {
        const uint64_t nblocks = (uint64_t)((tq + 63) / 64) * (uint64_t)((tr + 63) / 64);
        const uint64_t gram_groups = nblocks * 4096 + nprof;
        indexable = indexable && nblocks <= 0x7fffffffu / 4096u;
        if (indexable) {
            const uint32_t gx = cross_gram_gx(num_cu, (uint32_t)nblocks, bins);
            indexable = !partials_too_many(gram_groups, gx);
            partials = std::max(partials, gram_groups * gx);
        }
        results = std::max(results, gram_groups);
    }
    if (kind.route == kNearestOption || kind.route == kNearestSmooth) {
        partials = std::max(partials, nprof * option_totals_gx(num_cu, (uint32_t)nprof, bins));
        extra = std::max<uint64_t>(g.slots * 2, nprof);   // the totals (of the pairs, for positive + scale)
    }
    return NearestCost{indexable, (partials + results + extra) * sizeof(Partial) + (uint64_t)tq * (uint64_t)tr * sizeof(double)};
}

struct NearestTile {
    int q0, q1, r0, r1;   // left profiles [q0, q1) against right profiles [r0, r1)
};
struct NearestPlan {
    int tile_q, tile_r;               // the sides of every tile but the ragged last ones of a band / of the bands
    std::vector<NearestTile> tiles;   // band after band (ascending q0), within a band in ascending r0
};

// Half of a tile side, in whole 64-profile blocks while the side is longer than two of them.
inline int nearest_half(int side)
{
    const int half = (side + 1) / 2;
    return side > 128 ? (half + 63) / 64 * 64 : half;
}

// The tiles of a Q x R rectangle of profiles of `bins` bins: one grid of tile_q x tile_r tiles (the last of a band and the
// last band ragged) that covers every pair exactly once.  tile_q / tile_r > 0: the caller's caps -- they only shrink tiles.
// A tile that does not pass is cut in its left side while that is the longer one or longer than 1024 profiles (a band keeps
// its running best on the device, so a long right side means fewer selections), else in its right side.  A budget that not
// even one pair fits gives tiles of one pair.
inline NearestPlan nearest_plan(uint64_t bins, int num_cu, const NearestKind &kind, int Q, int R, uint64_t budget, int tile_q = 0, int tile_r = 0)
{
    int tq = tile_q > 0 ? std::min(Q, tile_q) : Q, tr = tile_r > 0 ? std::min(R, tile_r) : R;
    auto passes = [&](int a, int b) {
        const NearestCost cost = nearest_tile_cost(bins, num_cu, kind, a, b);
        return cost.indexable && cost.bytes <= budget;
    };
    auto fits = [&]() {   // the four shapes the grid has: whole tiles, the ragged ends, the corner
        const int lq = Q - (Q - 1) / tq * tq, lr = R - (R - 1) / tr * tr;
        return passes(tq, tr) && passes(lq, tr) && passes(tq, lr) && passes(lq, lr);
    };
    while (!fits() && (tq > 1 || tr > 1)) {
        if (tq > 1 && (tq > 1024 || tq >= tr || tr == 1)) tq = nearest_half(tq);
        else tr = nearest_half(tr);
    }
    NearestPlan plan = {tq, tr, {}};
    for (int64_t q0 = 0; q0 < Q; q0 += tq)
        for (int64_t r0 = 0; r0 < R; r0 += tr)
            plan.tiles.push_back(NearestTile{(int)q0, (int)std::min<int64_t>(Q, q0 + tq), (int)r0, (int)std::min<int64_t>(R, r0 + tr)});
    return plan;
}

}  // namespace kpal
