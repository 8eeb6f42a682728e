// pair_set_kernels.hpp -- the distances of the LINKED pairs of two sets of profiles (pair p: left table p against right table p)
// for every built-in ProfileDistance without dynamic smoothing, gfx950 (kpal_paired_distance[_device]; planned by
// pair_set_plan.hpp, launched by kpal_paired.hip).  The work is the flat list of items (pair, slice of kPairSetSliceBins bins);
// persistent workgroups take it in units, round robin:
//   SLICE form (a table of more than kPairSetWaveMaxBins bins)  a unit is one item, streamed by the four waves of a workgroup
//   WAVE form                                                  a unit is four pairs, one whole table each per wave: no LDS and
//                                                              no barrier, the last unit may have fewer than four
// Either way a lane streams both tables with 16-byte loads, kPairSetUnroll per table in flight; pair, slice and the two table
// bases are uniform (blockIdx, readfirstlane of the wave number): the walk through a slice is scalar arithmetic, and a round of
// loads costs one 64-bit vector add per table (the lane's address + the round's scalar offset, the loads 1 KiB or 4 KiB apart
// by immediate offsets).  One
// Partial per accumulator and item goes to (a * N + pair) * slices + slice; reduce_partials adds a pair's slices in slice order.
// The arithmetic of a bin is option_term.hpp's, which the rectangle kernels share.  Plain 'prod' / 'sum' / euclidean are the
// same kernel with no option set.
//   scale   pair_set_totals_kernel first: the two int64 totals of every pair (masked under positive), same items, same
//           reduction; the metric pass derives the pair's factors from the reduced totals (cross_opt_scale).
// No table is materialised and the inputs are never written.
#pragma once
#include "option_term.hpp"
#include "pair_set_plan.hpp"

namespace kpal {

struct PairSetArgs {
    const int64_t *left, *right;   // the first tables of the two sides (16-byte aligned)
    uint64_t bins;                 // 4^k
    uint32_t n_pairs, slices, units;
    int down;                      // metrics.scale_down
    const Partial *totals;         // SCALED: the reduced totals (.m), left of pair p at p, right at n_pairs + p
};

// The accumulators of one pair in one lane.
template <int MODE, bool SCALED, bool POSITIVE>
struct PairAcc {
    static constexpr int NACC = MODE == 3 ? 3 : MODE == kOptTotals ? 2 : 1;
    double s[NACC];
    unsigned long long m[NACC];
    double ls, rs;

    __device__ __forceinline__ void begin(const PairSetArgs &a, uint32_t pair)
    {
#pragma unroll
        for (int n = 0; n < NACC; ++n) {
            s[n] = 0.0;
            m[n] = 0ULL;
        }
        ls = 1.0;
        rs = 1.0;
        if constexpr (SCALED) cross_opt_scale((int64_t)a.totals[pair].m, (int64_t)a.totals[a.n_pairs + pair].m, a.down != 0, ls, rs);
    }
    __device__ __forceinline__ void bin(int64_t xi, int64_t yi)
    {
        constexpr int n1 = NACC > 1 ? 1 : 0, n2 = NACC - 1;
        opt_mask<POSITIVE>(xi, yi);
        opt_term<MODE, SCALED>(xi, yi, ls, rs, s[0], s[n1], s[n2], m[0], m[n1], m[n2]);
    }
    __device__ __forceinline__ void add(const longlong2 &x, const longlong2 &y)
    {
        bin(x.x, y.x);
        bin(x.y, y.y);
    }
};

// An offset every lane of the wave holds alike, said explicitly: the loop's address arithmetic stays on the scalar unit.
__device__ __forceinline__ uint64_t pair_set_uniform(uint64_t a)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// T lanes (lane t of them) stream the nvec bin pairs from entry `first` on of the tables at left / right: whole rounds of
// kPairSetUnroll loads per table, then the rest (tables below one round: k <= 4 in the wave form) a load at a time, nothing
// read past nvec.
template <int T, class Acc>
__device__ __forceinline__ void pair_set_stream(const int64_t *__restrict__ left, const int64_t *__restrict__ right, uint64_t first,
                                                uint32_t nvec, uint32_t t, Acc &acc)
{
    constexpr uint32_t U = kPairSetUnroll;
    uint32_t v = 0;
    for (; v + U * T <= nvec; v += U * T) {
        const uint64_t at = pair_set_uniform(first + 2 * (uint64_t)v);
        const char *lr = reinterpret_cast<const char *>(left + at), *rr = reinterpret_cast<const char *>(right + at);
        longlong2 x[U], y[U];
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) {
            x[u] = *reinterpret_cast<const longlong2 *>(lr + (u * T + t) * 16u);   // (a 32-bit byte offset: below 16 KiB)
            y[u] = *reinterpret_cast<const longlong2 *>(rr + (u * T + t) * 16u);
        }
#pragma unroll
        for (uint32_t u = 0; u < U; ++u) acc.add(x[u], y[u]);
    }
    for (; v < nvec; v += T) {
        const uint64_t at = pair_set_uniform(first + 2 * (uint64_t)v);
        const char *lr = reinterpret_cast<const char *>(left + at), *rr = reinterpret_cast<const char *>(right + at);
        if (v + t < nvec) acc.add(*reinterpret_cast<const longlong2 *>(lr + t * 16u), *reinterpret_cast<const longlong2 *>(rr + t * 16u));
    }
}

__device__ __forceinline__ Partial pair_set_wave_reduce(Partial p)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        p.s += __shfl_down(p.s, d);
        p.m += __shfl_down(p.m, d);
    }
    return p;   // valid in lane 0
}

template <int MODE, bool SCALED, bool POSITIVE, bool WAVE>
__device__ __forceinline__ void pair_set_body(const PairSetArgs &a, Partial *__restrict__ partials)
{
    using Acc = PairAcc<MODE, SCALED, POSITIVE>;
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (uniform: the table bases stay scalar)
    for (uint32_t unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
        uint32_t pair, slice;
        if constexpr (WAVE) {
            pair = unit * (uint32_t)kPairSetWaves + wave;
            slice = 0;
            if (pair >= a.n_pairs) break;   // the ragged last unit (this form has no barrier a wave could be missed at)
        } else {
            pair = unit / a.slices;
            slice = unit - pair * a.slices;
        }
        const uint64_t first = pair_set_slice_begin(slice), end = pair_set_slice_end(a.bins, slice);
        const uint32_t nvec = (uint32_t)((end - first) / 2);   // 4^k is even: 16 bytes are two bins of one table
        const uint64_t at = (uint64_t)pair * a.bins + first;   // the slice's first entry in both sets
        Acc acc;
        acc.begin(a, pair);
        if constexpr (WAVE) pair_set_stream<64>(a.left, a.right, at, nvec, lane, acc);
        else pair_set_stream<kPairSetThreads>(a.left, a.right, at, nvec, threadIdx.x, acc);
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

// MODE 0 .. 3: KPAL_PAIRWISE_PROD .. KPAL_COSINE
template <int MODE, bool SCALED, bool POSITIVE, bool WAVE>
__global__ __launch_bounds__(kPairSetThreads) void pair_set_kernel(const PairSetArgs a, Partial *__restrict__ partials)
{
    pair_set_body<MODE, SCALED, POSITIVE, WAVE>(a, partials);
}

// np.sum of the two tables of every pair (wrapping int64), under POSITIVE of the bins where both counts are non-zero:
// accumulator 0 the left total, 1 the right one.
template <bool POSITIVE, bool WAVE>
__global__ __launch_bounds__(kPairSetThreads) void pair_set_totals_kernel(const PairSetArgs a, Partial *__restrict__ partials)
{
    pair_set_body<kOptTotals, false, POSITIVE, WAVE>(a, partials);
}

}  // namespace kpal
