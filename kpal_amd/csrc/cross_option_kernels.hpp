// cross_option_kernels.hpp -- the Q x R rectangle (and the lower triangle of a set against itself) for every built-in
// ProfileDistance that is NOT plain: any mix of positive, scale (+- down) and the metrics prod / sum / euclidean / cosine
// (kpal_cross_profile_distance[_device], kpal_profile_distance_matrix_device).  Dynamic smoothing is not here: these entries
// keep one pair pipeline per pair (kpal_cross.hip loops it); a node's collapse decision is an OR of one flag per partner, and
// smooth_set_kernels.hpp runs the smoothed rectangle from per-profile pyramids with this file's arithmetic (SmoothAcc).
//
// The arithmetic of a term is option_distance_kernel<METRIC, SCALED>'s (option_kernels.hpp), term for term: wrapping int64
// when unscaled, float64 `count * scale` when scaled, IEEE division in the multiset terms.  What is new is that the steps
// that depend on the partner never materialise a table:
//   positive   a bin counts for a pair only where BOTH counts are non-zero (positive_kernel's identity): a mask in registers
//   scale      the pair's two factors are derived on the device from reduced int64 totals (metrics.get_scale / scale_down as
//              profile_distance_pair evaluates them): per profile (cross_option_totals_kernel, Q + R totals in one pass) or,
//              with positive, per pair from a first rectangle pass (MODE kOptTotals: sum x [y != 0] and sum y [x != 0])
// OptAcc is an accumulator of cross_kernels.hpp's two skeletons, cross_tile_kernel (a side of at most four profiles, or k < 6)
// and cross_super_kernel; addressing, tile numbers and the partial layout are theirs.
// Accumulators: multiset (sum of terms, terms); euclidean (float sum | int64 dot); cosine l.r, l.l, r.r (float | int64 each);
// kOptTotals: the two masked totals (int64).
#pragma once
#include "cross_kernels.hpp"
#include "option_term.hpp"   // kOptTotals, cross_opt_scale, the mask and the term of a bin

namespace kpal {

template <int MODE, bool SCALED, bool POSITIVE>
struct OptAcc {
    static constexpr int NACC = MODE == 3 ? 3 : MODE == kOptTotals ? 2 : 1;
    static constexpr bool RCP = false;
    static constexpr bool CODES = false;
    using Opt = CrossOpt;
    double s[NACC][4][4];
    unsigned long long m[NACC][4][4];
    double ls[4][4], rs[4][4];

    // tile (ti, tj) with number t: zero the accumulators, derive the pairs' factors
    __device__ __forceinline__ void begin(const CrossOpt &o, int ti, int tj, uint32_t t)
    {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
#pragma unroll
                for (int n = 0; n < NACC; ++n) {
                    s[n][a][b] = 0.0;
                    m[n][a][b] = 0ULL;
                }
                ls[a][b] = 1.0;
                rs[a][b] = 1.0;
                if constexpr (SCALED) {
                    int64_t tl, tr;
                    if constexpr (POSITIVE) {
                        const uint32_t slot = t * 16u + (uint32_t)(a * 4 + b);
                        tl = (int64_t)o.totals[slot].m;
                        tr = (int64_t)o.totals[o.slots + slot].m;
                    } else {
                        tl = (int64_t)o.totals[min(ti * 4 + a, o.c.Q - 1)].m;
                        tr = (int64_t)o.totals[o.roff + (uint32_t)min(tj * 4 + b, o.c.R - 1)].m;
                    }
                    cross_opt_scale(tl, tr, o.down != 0, ls[a][b], rs[a][b]);
                }
            }
    }

    // one bin of the four rows and four columns
    __device__ __forceinline__ void add(const int64_t (&x)[4], const int64_t (&y)[4])
    {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                int64_t xi = x[a], yi = y[b];
                opt_mask<POSITIVE || MODE == kOptTotals>(xi, yi);
                term(a, b, xi, yi);
            }
    }
    // the term of pair (a, b) for the counts (xi, yi) that are left of a bin
    __device__ __forceinline__ void term(int a, int b, int64_t xi, int64_t yi)
    {
        constexpr int n1 = NACC > 1 ? 1 : 0, n2 = NACC - 1;   // (the accumulators a MODE lacks: one it has, untouched)
        opt_term<MODE, SCALED>(xi, yi, ls[a][b], rs[a][b], s[0][a][b], s[n1][a][b], s[n2][a][b], m[0][a][b], m[n1][a][b], m[n2][a][b]);
    }
    __device__ __forceinline__ void finish() {}
    __device__ __forceinline__ Partial partial(int n, int a, int b) const { return Partial{s[n][a][b], m[n][a][b]}; }
};

// np.sum of every profile (wrapping int64): blockIdx.x = profile * gx + slice, profiles 0 .. Q-1 left, Q .. nprof-1 right
// (nprof = Q when the right set is the left one).  Partials: profile * gx + slice, .m = the partial total.
__global__ __launch_bounds__(256) void cross_option_totals_kernel(const CrossSets c, uint32_t gx, Partial *__restrict__ partials)
{
    const uint32_t p = blockIdx.x / gx, slice = blockIdx.x % gx;
    const int64_t *v = p < (uint32_t)c.Q ? c.left + (uint64_t)p * c.n : c.right + (uint64_t)(p - (uint32_t)c.Q) * c.n;
    Partial acc = {0.0, 0ULL};
    for (uint64_t i = (uint64_t)slice * blockDim.x + threadIdx.x; i < c.n; i += (uint64_t)gx * blockDim.x) acc.m += (uint64_t)v[i];
    acc = block_reduce(acc);
    if (threadIdx.x == 0) partials[(uint64_t)p * gx + slice] = acc;
}

}  // namespace kpal
