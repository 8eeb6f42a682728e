// pair_smooth_kernels.hpp -- dynamic smoothing (kdistlib.py:53-124) over the LINKED pairs of two sets of profiles, gfx950
// (kpal_paired_smooth_distance[_device], kpal_paired_smooth_device; planned by pair_smooth_plan.hpp, launched by
// kpal_paired_smooth.hip).  Every distinct table of a chunk has its pyramid of node sums and node codes already
// (smooth_set_level_kernel, smooth_set_codes_kernel; layout: smooth_plan.hpp).  On the model of pair_set_kernels.hpp:
//   pair_smooth_kernel        the distance of every pair: SmoothAcc's arithmetic (smooth_set_kernels.hpp) stated per element --
//                             a BIN i is live iff its height-0 node i >> 2 has code 0 on BOTH sides; a live bin gives
//                             opt_term(x_i, y_i), a dead one the (0, 0) term (nothing when unscaled; scaled, the reference
//                             scales the zeros and 0 * a non-finite factor is its NaN).  A pyramid ELEMENT e is live iff
//                             max(code_left, code_right) == 1 and gives the term of the two node sums; a dead node, the
//                             padding included, gives nothing.  The factors: cross_opt_scale on the two roots (smoothing
//                             conserves totals).  Items, units, grid and partial layout: pair_smooth_plan.hpp.
//   pair_smooth_apply_kernel  the smoothed tables of every pair, both sides: a live bin keeps its count; the first bin of the
//                             live node (h, i >> 2(h+1)) -- at most one h -- gets that node's sum; every other bin 0.
// A lane streams both tables with 16-byte loads, kPairSetUnroll per table in flight; pair, slice and the bases are uniform and
// the walk is scalar arithmetic.  CODES are a byte per four bins and a byte per node: beside a 16-byte load of two bins goes
// one byte per side (both bins lie in one height-0 node), beside a 16-byte load of two node sums one 16-bit word per side --
// never a code per bin.  The inputs and the pyramids are not written.
#pragma once
#include "option_term.hpp"
#include "pair_smooth_plan.hpp"
#include "pair_set_kernels.hpp"

namespace kpal {

struct PairSmoothArgs {
    const int64_t *left, *right;   // the first tables of the two sides (16-byte aligned)
    const int64_t *sums;           // the pyramids: node sums, `stride` a profile
    const uint8_t *codes;          // ... and node codes
    const Partial *totals;         // .m: the root of pyramid t = np.sum of its table
    uint64_t bins, stride;         // 4^k, smooth_stride(k)
    uint32_t n_pairs, bin_slices, slices, units;
    uint32_t lbase, rbase;         // the pyramids of pair p: lbase + p and rbase + p
    int k, down;
};

template <int MODE, bool SCALED>
struct PairSmoothAcc {
    static constexpr int NACC = MODE == 3 ? 3 : 1;
    double s[NACC];
    unsigned long long m[NACC];
    double ls, rs;

    __device__ __forceinline__ void begin(const PairSmoothArgs &a, uint32_t pair)
    {
#pragma unroll
        for (int n = 0; n < NACC; ++n) {
            s[n] = 0.0;
            m[n] = 0ULL;
        }
        ls = 1.0;
        rs = 1.0;
        if constexpr (SCALED) cross_opt_scale((int64_t)a.totals[a.lbase + pair].m, (int64_t)a.totals[a.rbase + pair].m, a.down != 0, ls, rs);
    }
    __device__ __forceinline__ void term(int64_t xi, int64_t yi)
    {
        constexpr int n1 = NACC > 1 ? 1 : 0, n2 = NACC - 1;
        opt_term<MODE, SCALED>(xi, yi, ls, rs, s[0], s[n1], s[n2], m[0], m[n1], m[n2]);
    }
    // two bins of one height-0 node, its code on either side
    __device__ __forceinline__ void bins(const longlong2 &x, const longlong2 &y, uint32_t cx, uint32_t cy)
    {
        const bool live = (cx | cy) == 0;   // (unscaled, the (0, 0) term of a dead bin adds nothing)
        term(live ? x.x : 0, live ? y.x : 0);
        term(live ? x.y : 0, live ? y.y : 0);
    }
    // two node sums, their two codes on either side in a 16-bit word
    __device__ __forceinline__ void nodes(const longlong2 &x, const longlong2 &y, uint32_t cx, uint32_t cy)
    {
        if (max(cx & 0xffu, cy & 0xffu) == 1u) term(x.x, y.x);
        if (max(cx >> 8, cy >> 8) == 1u) term(x.y, y.y);
    }
};

// T lanes (lane t of them) stream nvec 16-byte vectors of two tables from `left` / `right` on, with the codes that belong to
// them from cl / cr on.  BINS: vector v is bins 2v, 2v + 1 and its code the byte v >> 1; else vector v is elements 2v, 2v + 1
// and its codes the 16-bit word v.  Whole rounds of kPairSetUnroll loads per table, then the rest a load at a time.
template <int T, bool BINS, class Acc>
__device__ __forceinline__ void pair_smooth_stream(const int64_t *__restrict__ left, const int64_t *__restrict__ right,
                                                   const uint8_t *__restrict__ cl, const uint8_t *__restrict__ cr, uint32_t nvec, uint32_t t,
                                                   Acc &acc)
{
    constexpr uint32_t U = kPairSetUnroll;
    auto code = [](const uint8_t *c, uint32_t v) -> uint32_t {
        if constexpr (BINS) return c[v >> 1];
        else return *reinterpret_cast<const uint16_t *>(c + 2 * (size_t)v);
    };
    uint32_t v = 0;
    for (; v + U * T <= nvec; v += U * T) {
        const uint64_t at = pair_set_uniform(2 * (uint64_t)v);
        const uint64_t cat = pair_set_uniform(BINS ? (uint64_t)(v >> 1) : 2 * (uint64_t)v);
        const char *lr = reinterpret_cast<const char *>(left + at), *rr = reinterpret_cast<const char *>(right + at);
        const uint8_t *lc = cl + cat, *rc = cr + cat;
        longlong2 x[U], y[U];
        uint32_t cx[U], cy[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            x[u] = *reinterpret_cast<const longlong2 *>(lr + (u * T + t) * 16u);
            y[u] = *reinterpret_cast<const longlong2 *>(rr + (u * T + t) * 16u);
            cx[u] = code(lc, u * T + t);   // (v is a multiple of 2 T: the byte of vector v + w is byte (v >> 1) + (w >> 1))
            cy[u] = code(rc, u * T + t);
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            if constexpr (BINS) acc.bins(x[u], y[u], cx[u], cy[u]);
            else acc.nodes(x[u], y[u], cx[u], cy[u]);
        }
    }
    for (; v < nvec; v += T) {
        if (v + t < nvec) {
            const longlong2 x = *reinterpret_cast<const longlong2 *>(left + 2 * (size_t)(v + t));
            const longlong2 y = *reinterpret_cast<const longlong2 *>(right + 2 * (size_t)(v + t));
            const uint32_t cx = code(cl, v + t), cy = code(cr, v + t);
            if constexpr (BINS) acc.bins(x, y, cx, cy);
            else acc.nodes(x, y, cx, cy);
        }
    }
}

// The bin slice `slice` of pair `pair` (WAVE: the whole table), by T lanes.
template <int T, class Acc>
__device__ __forceinline__ void pair_smooth_bins(const PairSmoothArgs &a, uint32_t pair, uint32_t slice, uint32_t t, Acc &acc)
{
    const uint64_t first = pair_set_slice_begin(slice), end = pair_set_slice_end(a.bins, slice);
    const uint64_t at = pair_set_uniform((uint64_t)pair * a.bins + first);
    // bins / 4 height-0 nodes open a pyramid (k = 1: the root alone)
    const uint64_t lc = pair_set_uniform((uint64_t)(a.lbase + pair) * a.stride + first / 4), rc = pair_set_uniform((uint64_t)(a.rbase + pair) * a.stride + first / 4);
    pair_smooth_stream<T, true>(a.left + at, a.right + at, a.codes + lc, a.codes + rc, (uint32_t)((end - first) / 2), t, acc);
}

// The node slice `node_slice` of the two pyramids of pair `pair`, by T lanes.
template <int T, class Acc>
__device__ __forceinline__ void pair_smooth_nodes(const PairSmoothArgs &a, uint32_t pair, uint32_t node_slice, uint32_t t, Acc &acc)
{
    const uint64_t first = pair_smooth_node_begin(node_slice);
    const uint64_t end = (first + kPairSmoothSliceNodes) < a.stride ? first + kPairSmoothSliceNodes : a.stride;   // pair_smooth_node_end
    const uint64_t l = pair_set_uniform((uint64_t)(a.lbase + pair) * a.stride + first), r = pair_set_uniform((uint64_t)(a.rbase + pair) * a.stride + first);
    pair_smooth_stream<T, false>(a.sums + l, a.sums + r, a.codes + l, a.codes + r, (uint32_t)((end - first) / 2), t, acc);   // (the stride is even)
}

// MODE 0 .. 3: KPAL_PAIRWISE_PROD .. KPAL_COSINE
template <int MODE, bool SCALED, bool WAVE>
__global__ __launch_bounds__(kPairSetThreads) void pair_smooth_kernel(const PairSmoothArgs a, Partial *__restrict__ partials)
{
    using Acc = PairSmoothAcc<MODE, SCALED>;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (uint32_t unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
        uint32_t pair, slice;
        if constexpr (WAVE) {
            pair = unit * (uint32_t)kPairSetWaves + wave;
            slice = 0;
            if (pair >= a.n_pairs) break;   // the ragged last unit (no barrier in this form)
        } else {
            pair = unit / a.slices;
            slice = unit - pair * a.slices;
        }
        Acc acc;
        acc.begin(a, pair);
        if constexpr (WAVE) {
            pair_smooth_bins<64>(a, pair, 0, lane, acc);
            pair_smooth_nodes<64>(a, pair, 0, lane, acc);
        } else if (slice < a.bin_slices) {   // (uniform)
            pair_smooth_bins<kPairSetThreads>(a, pair, slice, threadIdx.x, acc);
        } else {
            pair_smooth_nodes<kPairSetThreads>(a, pair, slice - a.bin_slices, threadIdx.x, acc);
        }
#pragma unroll
        for (int n = 0; n < Acc::NACC; ++n) {
            const uint64_t at = pair_set_partial((uint64_t)n, a.n_pairs, a.slices, pair, slice);
            if constexpr (WAVE) {
                const Partial p = pair_set_wave_reduce(Partial{acc.s[n], acc.m[n]});
                if (lane == 0) partials[at] = p;
            } else {
                const Partial p = block_reduce(Partial{acc.s[n], acc.m[n]});
                if (threadIdx.x == 0) partials[at] = p;
            }
        }
    }
}

// What bins 2v, 2v + 1 of a smoothed table of a pair hold, given the counts x: `dead` -- the height-0 node above them is not
// code 0 on both sides.  Only a bin that is a multiple of four can be the first bin of a node: bin 2v for even v.
__device__ __forceinline__ longlong2 pair_smooth_value(const PairSmoothArgs &a, const longlong2 &x, bool dead, uint64_t bin, const int64_t *__restrict__ sums,
                                                       const uint8_t *__restrict__ lc, const uint8_t *__restrict__ rc)
{
    if (!dead) return x;
    longlong2 o;
    o.x = 0;
    o.y = 0;
    if (bin & 3) return o;
    uint64_t node = bin >> 2, off = 0;
    for (int h = 0; h < a.k; ++h) {   // node (h, bin >> 2(h+1)) while bin is its first bin
        if (max(lc[off + node], rc[off + node]) == 1) {
            o.x = sums[off + node];
            break;
        }
        if (node & 3) break;
        off += smooth_level_nodes(a.k, h);
        node >>= 2;
    }
    return o;
}

// Units: those of the bins (pair_set_units); a unit is a bin slice of a pair (WAVE: four pairs, a table a wave).
template <bool WAVE>
__global__ __launch_bounds__(kPairSetThreads) void pair_smooth_apply_kernel(const PairSmoothArgs a, int64_t *__restrict__ out_left, int64_t *__restrict__ out_right)
{
    constexpr uint32_t T = WAVE ? 64 : kPairSetThreads;
    const uint32_t t = WAVE ? (threadIdx.x & 63) : threadIdx.x;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (uint32_t unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
        uint32_t pair, slice;
        if constexpr (WAVE) {
            pair = unit * (uint32_t)kPairSetWaves + wave;
            slice = 0;
            if (pair >= a.n_pairs) break;
        } else {
            pair = unit / a.bin_slices;
            slice = unit - pair * a.bin_slices;
        }
        const uint64_t first = pair_set_slice_begin(slice), end = pair_set_slice_end(a.bins, slice);
        const uint32_t nvec = (uint32_t)((end - first) / 2);
        const uint64_t at = pair_set_uniform((uint64_t)pair * a.bins + first);
        const uint64_t lp = pair_set_uniform((uint64_t)(a.lbase + pair) * a.stride), rp = pair_set_uniform((uint64_t)(a.rbase + pair) * a.stride);
        const uint8_t *lc = a.codes + lp, *rc = a.codes + rp;
        for (uint32_t v = t; v < nvec; v += T) {
            const uint64_t bin = first + 2 * (uint64_t)v;
            const longlong2 x = *reinterpret_cast<const longlong2 *>(a.left + at + 2 * (size_t)v);
            const longlong2 y = *reinterpret_cast<const longlong2 *>(a.right + at + 2 * (size_t)v);
            const bool dead = (lc[bin >> 2] | rc[bin >> 2]) != 0;
            *reinterpret_cast<longlong2 *>(out_left + at + 2 * (size_t)v) = pair_smooth_value(a, x, dead, bin, a.sums + lp, lc, rc);
            *reinterpret_cast<longlong2 *>(out_right + at + 2 * (size_t)v) = pair_smooth_value(a, y, dead, bin, a.sums + rp, lc, rc);
        }
    }
}

}  // namespace kpal
