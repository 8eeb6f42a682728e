// smooth_set_kernels.hpp -- dynamic smoothing (kdistlib.py:53-124) over the Q x R rectangle, or the lower triangle, of two
// SETS of profiles in a fixed number of launches (kpal_cross_smooth_distance_device, kpal_smooth_distance_matrix_device).
// smooth_plan.hpp has the decomposition and the layout: the collapse test of a node is an OR of one flag per partner, so
// every profile gets its pyramid of node sums and node codes ONCE --
//   smooth_set_level_kernel   one height of every profile of both sets: the wrapping sums of the four children and the
//                             node's own flag, summarise4(quarters) <= threshold (the pair pipeline's summarise4: tie for tie)
//   smooth_set_codes_kernel   flags -> codes: a node walks its <= k - 1 ancestors, as smooth_apply_kernel walks them per bin;
//                             the padding behind the root becomes dead (sum 0, code 2); the root is the profile's np.sum
//                             (smoothing conserves totals), written as the total get_scale wants
// -- and a pair's distance is OptAcc's term arithmetic (cross_option_kernels.hpp) over the LIVE elements, max(code_left,
// code_right) == 1, of two passes of the same rectangle skeleton (cross_kernels.hpp): over the bins, whose code follows from
// their bottom node's, and over the pyramids.  SmoothAcc is that accumulator.
//   A dead BIN still gives its (0, 0) term: the reference scales the zeros of the smoothed tables, and 0 * (a factor that is
// not finite) is the NaN it returns then.  A dead NODE is no bin of the reference's tables and gives nothing.  (A live node
// stands for its first bin, which is dead: the reference has a zero bin exactly when some bin is dead here.)
#pragma once
#include "cross_option_kernels.hpp"
#include "smooth_summary.hpp"
#include "smooth_plan.hpp"

namespace kpal {

// The pyramids of the nprof profiles of c (left 0 .. Q-1, then right; nprof = Q when the right set is the left one).
struct SmoothSet {
    CrossSets c;
    uint32_t nprof;
    int k;
    uint64_t stride;   // smooth_stride(k): elements from one profile's pyramid to the next
    int64_t *sums;
    uint8_t *codes, *flags;
    Partial *totals;   // .m = np.sum of profile p
};

// blockIdx.x = profile * per + part; the parts stride over the nodes of height h.
__global__ __launch_bounds__(256) void smooth_set_level_kernel(const SmoothSet s, int h, uint32_t per, int summary, double threshold)
{
    const uint32_t p = blockIdx.x / per, part = blockIdx.x % per;
    const uint64_t nodes = smooth_level_nodes(s.k, h), at = (uint64_t)p * s.stride + smooth_level_offset(s.k, h);
    const int64_t *child;
    if (h == 0) child = p < (uint32_t)s.c.Q ? s.c.left + (uint64_t)p * s.c.n : s.c.right + (uint64_t)(p - (uint32_t)s.c.Q) * s.c.n;
    else child = s.sums + (uint64_t)p * s.stride + smooth_level_offset(s.k, h - 1);
    for (uint64_t j = (uint64_t)part * blockDim.x + threadIdx.x; j < nodes; j += (uint64_t)per * blockDim.x) {
        const longlong2 *pc = reinterpret_cast<const longlong2 *>(child + 4 * j);
        const longlong2 a0 = pc[0], a1 = pc[1];
        const int64_t q[4] = {a0.x, a0.y, a1.x, a1.y};
        s.sums[at + j] = (int64_t)((uint64_t)q[0] + (uint64_t)q[1] + (uint64_t)q[2] + (uint64_t)q[3]);
        s.flags[at + j] = summarise4(q, summary) <= threshold ? 1 : 0;
    }
}

// blockIdx.x = profile * per + part; the parts stride over the `stride` elements of a pyramid.
__global__ __launch_bounds__(256) void smooth_set_codes_kernel(const SmoothSet s, uint32_t per)
{
    const uint32_t p = blockIdx.x / per, part = blockIdx.x % per;
    const uint64_t base = (uint64_t)p * s.stride;
    for (uint64_t e = (uint64_t)part * blockDim.x + threadIdx.x; e < s.stride; e += (uint64_t)per * blockDim.x) {
        const SmoothElement el = smooth_element(s.k, e);
        if (el.height == kSmoothPadding) {
            s.sums[base + e] = 0;
            s.codes[base + e] = 2;
            continue;
        }
        bool above = false;
        uint64_t node = el.node;
        for (int h = el.height + 1; h < s.k; ++h) {
            node >>= 2;
            above |= s.flags[base + smooth_level_offset(s.k, h) + node] != 0;
        }
        s.codes[base + e] = above ? 2 : s.flags[base + e];
        if (el.height == s.k - 1) s.totals[p] = Partial{0.0, (unsigned long long)s.sums[base + e]};
    }
}

// OptAcc<MODE, SCALED, false> over the live elements of a pass.
template <int MODE, bool SCALED>
struct SmoothAcc {
    static constexpr int NACC = MODE == 3 ? 3 : 1;
    static constexpr bool RCP = false;
    static constexpr bool CODES = true;
    using Opt = CrossCodeOpt;
    OptAcc<MODE, SCALED, false> t;
    bool dead_terms;   // the elements are bins: a dead one is a (0, 0) term

    __device__ __forceinline__ void begin(const CrossCodeOpt &o, int ti, int tj, uint32_t tile)
    {
        t.begin(o, ti, tj, tile);
        dead_terms = o.cshift != 0;
    }
    __device__ __forceinline__ void add(const int64_t (&x)[4], const int64_t (&y)[4], const uint8_t (&cx)[4], const uint8_t (&cy)[4])
    {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const bool live = max(cx[a], cy[b]) == 1;
                if constexpr (SCALED) {
                    if (!live && !dead_terms) continue;   // (unscaled: a (0, 0) term adds nothing to any accumulator)
                }
                t.term(a, b, live ? x[a] : 0, live ? y[b] : 0);
            }
    }
    __device__ __forceinline__ void finish() {}
    __device__ __forceinline__ Partial partial(int n, int a, int b) const { return t.partial(n, a, b); }
};

}  // namespace kpal
