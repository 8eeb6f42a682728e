// cross_option_kernels.hpp -- the Q x R rectangle (and the lower triangle of a set against itself) for every built-in
// ProfileDistance that is NOT plain: any mix of positive, scale (+- down) and the metrics prod / sum / euclidean / cosine
// (kpal_cross_profile_distance[_device], kpal_profile_distance_matrix_device).  Dynamic smoothing is not here: a node's
// collapse decision depends on both partners, so smoothed tables exist per pair only (kpal_cross.hip loops the pair pipeline).
//
// The arithmetic of a term is option_distance_kernel<METRIC, SCALED>'s (option_kernels.hpp), term for term: wrapping int64
// when unscaled, float64 `count * scale` when scaled, IEEE division in the multiset terms.  What is new is that the steps
// that depend on the partner never materialise a table:
//   positive   a bin counts for a pair only where BOTH counts are non-zero (positive_kernel's identity): a mask in registers
//   scale      the pair's two factors are derived on the device from reduced int64 totals (metrics.get_scale / scale_down as
//              profile_distance_pair evaluates them): per profile (cross_option_totals_kernel, Q + R totals in one pass) or,
//              with positive, per pair from a first rectangle pass (MODE kOptTotals: sum x [y != 0] and sum y [x != 0])
// Two forms with cross_kernels.hpp's addressing: cross_option_tile_kernel (4 x 4 register tiles from global memory: a side of
// at most four profiles, or k < 6) and cross_option_super_kernel (16 x 16 super-tiles, 64 bins of 16 + 16 rows per stage,
// cross_block's XCD-aware grid).  With `tri` the left and the right set are the same P profiles and only the tiles on or below
// the diagonal exist: tile (ti, tj), tj <= ti, has number ti (ti + 1) / 2 + tj, a super-tile likewise.
// Partials: accumulator a of pair (row x, column y) of tile t lies at ((a * slots + t * 16 + x * 4 + y) * ngroups + group),
// slots = 16 * tiles; reduce_partials_kernel adds the groups in a fixed order.  Accumulators: multiset (sum of terms, terms);
// euclidean (float sum | int64 dot); cosine l.r, l.l, r.r (float | int64 each); kOptTotals: the two masked totals (int64).
#pragma once
#include "cross_kernels.hpp"

namespace kpal {

constexpr int kOptTotals = 4;   // MODE of the masked-totals pass (0 .. 3: KPAL_PAIRWISE_PROD .. KPAL_COSINE)

struct CrossOpt {
    CrossSets c;
    int tri;                 // the set against itself (c.left == c.right, c.Q == c.R): tiles on or below the diagonal
    int down;                // metrics.scale_down
    const Partial *totals;   // SCALED: reduced totals (.m), per profile (left 0 .. Q-1, right from `roff`) or per pair slot
    uint32_t roff;
    uint32_t slots;
};

// Number t of a tile -> (ti, tj): row-major over `side` columns, or the lower triangle's ti (ti + 1) / 2 + tj.
__device__ __forceinline__ void cross_opt_tile(uint32_t t, int side, bool tri, int &ti, int &tj)
{
    if (!tri) {
        ti = (int)(t / (uint32_t)side);
        tj = (int)(t % (uint32_t)side);
        return;
    }
    uint32_t i = (uint32_t)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((i + 1u) * (i + 2u) / 2u <= t) ++i;
    while (i * (i + 1u) / 2u > t) --i;
    ti = (int)i;
    tj = (int)(t - i * (i + 1u) / 2u);
}

__device__ __forceinline__ uint32_t cross_opt_tile_number(int ti, int tj, int side, bool tri)
{
    return tri ? (uint32_t)ti * ((uint32_t)ti + 1u) / 2u + (uint32_t)tj : (uint32_t)ti * (uint32_t)side + (uint32_t)tj;
}

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

template <int MODE, bool SCALED, bool POSITIVE>
struct OptAcc {
    static constexpr int NACC = MODE == 3 ? 3 : MODE == kOptTotals ? 2 : 1;
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
                if constexpr (POSITIVE || MODE == kOptTotals) {
                    const bool both = xi != 0 && yi != 0;
                    xi = both ? xi : 0;
                    yi = both ? yi : 0;
                }
                if constexpr (MODE == kOptTotals) {
                    m[0][a][b] += (uint64_t)xi;
                    m[1][a][b] += (uint64_t)yi;
                } else if constexpr (SCALED) {
                    const double xd = (double)xi * ls[a][b], yd = (double)yi * rs[a][b];
                    if constexpr (MODE <= 1) {
                        if (xd != 0.0 || yd != 0.0) {
                            s[0][a][b] += MODE == 0 ? pw_prod(xd, yd) : pw_sum(xd, yd);
                            m[0][a][b] += 1;
                        }
                    } else if constexpr (MODE == 2) {
                        const double d = xd - yd;
                        s[0][a][b] += d * d;
                    } else {
                        s[0][a][b] += xd * yd;
                        s[1][a][b] += xd * xd;
                        s[2][a][b] += yd * yd;
                    }
                } else {
                    if constexpr (MODE <= 1) {
                        if (xi != 0 || yi != 0) {
                            s[0][a][b] += MODE == 0 ? pw_prod(xi, yi) : pw_sum(xi, yi);
                            m[0][a][b] += 1;
                        }
                    } else if constexpr (MODE == 2) {
                        const uint64_t d = (uint64_t)xi - (uint64_t)yi;
                        m[0][a][b] += d * d;
                    } else {
                        m[0][a][b] += (uint64_t)xi * (uint64_t)yi;
                        m[1][a][b] += (uint64_t)xi * (uint64_t)xi;
                        m[2][a][b] += (uint64_t)yi * (uint64_t)yi;
                    }
                }
            }
    }
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

// cross_tile_kernel's form: blockIdx.x = tile * gx + slice, the slices stride over the bins.
template <int MODE, bool SCALED, bool POSITIVE>
__global__ __launch_bounds__(256) void cross_option_tile_kernel(const CrossOpt o, uint32_t gx, Partial *__restrict__ partials)
{
    using Acc = OptAcc<MODE, SCALED, POSITIVE>;
    const CrossSets &c = o.c;
    const int sideR = (c.R + 3) / 4;
    const uint32_t tile = blockIdx.x / gx, slice = blockIdx.x % gx;
    int tq, tr;
    cross_opt_tile(tile, sideR, o.tri != 0, tq, tr);
    Acc acc;
    acc.begin(o, tq, tr, tile);
    const int64_t *rowp[4];
    const int64_t *colp[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        rowp[a] = c.left + (uint64_t)min(tq * 4 + a, c.Q - 1) * c.n;
        colp[a] = c.right + (uint64_t)min(tr * 4 + a, c.R - 1) * c.n;
    }
    for (uint64_t i = (uint64_t)slice * blockDim.x + threadIdx.x; i < c.n; i += (uint64_t)gx * blockDim.x) {
        int64_t x[4], y[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            x[a] = rowp[a][i];
            y[a] = colp[a][i];
        }
        acc.add(x, y);
    }
#pragma unroll
    for (int n = 0; n < Acc::NACC; ++n)
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                Partial p = {acc.s[n][a][b], acc.m[n][a][b]};
                p = block_reduce(p);
                if (threadIdx.x == 0) partials[((uint64_t)n * o.slots + (uint64_t)tile * 16u + (uint64_t)(a * 4 + b)) * gx + slice] = p;
            }
}

// cross_super_kernel's form: linear block id (cgrp * nsuper + s) * 8 + x -> super-tile s, bin-group cgrp * 8 + x (cross_block);
// sixteen 16-lane groups with one 4 x 4 register tile each; a group whose tile lies outside the rectangle, or above the
// diagonal of a triangle, only helps with the staging.
template <int MODE, bool SCALED, bool POSITIVE>
__global__ __launch_bounds__(256) void cross_option_super_kernel(const CrossOpt o, uint32_t nsuper, int superR, Partial *__restrict__ partials)
{
    using Acc = OptAcc<MODE, SCALED, POSITIVE>;
    __shared__ int64_t stage[2][32][kSuperRow];
    const CrossSets &c = o.c;
    const bool tri = o.tri != 0;
    const uint32_t lin = blockIdx.x, sidx = (lin >> 3) % nsuper, group = ((lin >> 3) / nsuper) * 8u + (lin & 7u), ngroups = gridDim.x / nsuper;
    int si, sj;
    cross_opt_tile(sidx, superR, tri, si, sj);
    const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
    const int ti = si * 4 + (g >> 2), tj = sj * 4 + (g & 3);
    const int sideQ = (c.Q + 3) / 4, sideR = (c.R + 3) / 4;
    const bool mine = ti < sideQ && tj < sideR && (!tri || tj <= ti);
    const uint32_t tile = mine ? cross_opt_tile_number(ti, tj, sideR, tri) : 0u;
    Acc acc;
    acc.begin(o, mine ? ti : 0, mine ? tj : 0, tile);
    // loader: value q of thread t is bin (t & 63) of staged row 4 q + (t >> 6): a wave reads one 512-byte run
    const int lrow = threadIdx.x >> 6, lcol = threadIdx.x & 63;
    const int64_t *src[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) src[q] = cross_row(c, si, sj, 4 * q + lrow) + lcol;
    const uint64_t chunks = c.n / kSuperBins;
    int64_t next[8];
    uint64_t ch = group;
    if (ch < chunks) {
#pragma unroll
        for (int q = 0; q < 8; ++q) stage[0][4 * q + lrow][lcol] = src[q][ch * kSuperBins];
    }
    __syncthreads();
    int cur = 0;
    for (; ch < chunks; ch += ngroups) {
        const bool more = ch + ngroups < chunks;       // block-uniform
        if (more) {
#pragma unroll
            for (int q = 0; q < 8; ++q) next[q] = src[q][(ch + ngroups) * kSuperBins];
        }
        if (mine) {
#pragma unroll 1
            for (int u = 0; u < kSuperBins / 16; ++u) {
                int64_t x[4], y[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    x[a] = stage[cur][4 * (g >> 2) + a][16 * u + l];
                    y[a] = stage[cur][16 + 4 * (g & 3) + a][16 * u + l];
                }
                acc.add(x, y);
            }
        }
        if (more) {
#pragma unroll
            for (int q = 0; q < 8; ++q) stage[cur ^ 1][4 * q + lrow][lcol] = next[q];
        }
        __syncthreads();
        cur ^= 1;
    }
    // per-group reduction over its 16 lanes (fixed order), lane 0 of the group writes
#pragma unroll
    for (int n = 0; n < Acc::NACC; ++n)
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                double ps = acc.s[n][a][b];
                unsigned long long pm = acc.m[n][a][b];
#pragma unroll
                for (int d = 8; d >= 1; d >>= 1) {
                    ps += __shfl_down(ps, d, 16);
                    pm += __shfl_down(pm, d, 16);
                }
                if (mine && l == 0)
                    partials[((uint64_t)n * o.slots + (uint64_t)tile * 16u + (uint64_t)(a * 4 + b)) * ngroups + group] = Partial{ps, pm};
            }
}

}  // namespace kpal
