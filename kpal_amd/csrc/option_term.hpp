// option_term.hpp -- the arithmetic of ONE bin of ONE pair under a built-in ProfileDistance, as the set kernels share it: the
// rectangle and the triangle (cross_option_kernels.hpp: OptAcc) and the linked pairs of two sets (pair_set_kernels.hpp).  It is
// option_distance_kernel<METRIC, SCALED>'s (option_kernels.hpp), term for term: wrapping int64 when unscaled, float64
// `count * scale` when scaled, IEEE division in the multiset terms; positive is a both-non-zero mask in registers
// (positive_kernel's identity).  No kernel lives here.
#pragma once
#include "matrix_common.hpp"

namespace kpal {

constexpr int kOptTotals = 4;   // MODE of the masked-totals pass (0 .. 3: KPAL_PAIRWISE_PROD .. KPAL_COSINE)

// metrics.get_scale (metrics.py:49-72: int64 totals, true division) and metrics.scale_down (metrics.py:75-86), evaluated
// as profile_distance_pair does on the host.
__device__ __forceinline__ void cross_opt_scale(int64_t tl, int64_t tr, bool down, double &ls, double &rs)
{
    ls = 1.0;
    rs = 1.0;
    if (tl < tr) ls = (double)tr / (double)tl;
    else rs = (double)tl / (double)tr;
    if (down) {
        const double top = ls > rs ? ls : rs;
        ls /= top;
        rs /= top;
    }
}

// positive (and the masked totals): a bin counts for a pair only where BOTH counts are non-zero
template <bool MASKED>
__device__ __forceinline__ void opt_mask(int64_t &xi, int64_t &yi)
{
    if constexpr (MASKED) {
        const bool both = xi != 0 && yi != 0;
        xi = both ? xi : 0;
        yi = both ? yi : 0;
    }
}

// The term of one pair for the counts (xi, yi) that are left of a bin, added to the pair's accumulators: (s0, m0) alone but for
// the cosine (s0 / m0 the dot, s1 / m1 and s2 / m2 the squared norms) and kOptTotals (m0, m1 the two totals).  The accumulators
// a MODE does not have may be passed as any of those it has: they are not touched.
template <int MODE, bool SCALED>
__device__ __forceinline__ void opt_term(int64_t xi, int64_t yi, double ls, double rs, double &s0, double &s1, double &s2,
                                         unsigned long long &m0, unsigned long long &m1, unsigned long long &m2)
{
    if constexpr (MODE == kOptTotals) {
        m0 += (uint64_t)xi;
        m1 += (uint64_t)yi;
    } else if constexpr (SCALED) {
        const double xd = (double)xi * ls, yd = (double)yi * rs;
        if constexpr (MODE <= 1) {
            if (xd != 0.0 || yd != 0.0) {
                s0 += MODE == 0 ? pw_prod(xd, yd) : pw_sum(xd, yd);
                m0 += 1;
            }
        } else if constexpr (MODE == 2) {
            const double d = xd - yd;
            s0 += d * d;
        } else {
            s0 += xd * yd;
            s1 += xd * xd;
            s2 += yd * yd;
        }
    } else {
        if constexpr (MODE <= 1) {
            if (xi != 0 || yi != 0) {
                s0 += MODE == 0 ? pw_prod(xi, yi) : pw_sum(xi, yi);
                m0 += 1;
            }
        } else if constexpr (MODE == 2) {
            const uint64_t d = (uint64_t)xi - (uint64_t)yi;
            m0 += d * d;
        } else {
            m0 += (uint64_t)xi * (uint64_t)yi;
            m1 += (uint64_t)xi * (uint64_t)xi;
            m2 += (uint64_t)yi * (uint64_t)yi;
        }
    }
}

}  // namespace kpal
