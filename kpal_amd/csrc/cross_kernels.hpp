// cross_kernels.hpp -- the Q x R rectangle of distances between two SETS of profiles (kpal_cross_distance[_device]).
// The triangle kernels of vec_kernels.hpp take one base pointer and walk a list of lower-triangle tiles; these take a
// left set (rows) and a right set (columns) in separate allocations and cover every tile of the rectangle, so no pair
// inside one set is ever evaluated.  The arithmetic is the triangle's (matrix_accumulate, matrix_accumulate_prod_rcp,
// rcp_counts, the byte-counter term counts); only the addressing, the masks and the partial layout are new.
//   cross_tile_kernel    4 x 4 register tiles straight from global memory: few queries (Q <= 4 or R <= 4: the long side
//                        streams past once, the short side's bins stay in the caches) and k < 6
//   cross_super_kernel   16 x 16 super-tiles staged through LDS, any values (the fallback of the two below, and euclidean
//                        where the Gram form does not apply)
//   cross_recip_kernel<0> multiset 'prod' as a difference of reciprocals, counts in [0, 2^16)   (matrix_rdiff_kernel's form)
//   cross_recip_kernel<1> multiset 'sum' with the reciprocal of the denominator from a table     (matrix_rsum_kernel's form)
//   cross_gram_kernel    euclidean from A . B^T on the fp64 matrix cores plus the norms of cross_norm_kernel, exact while
//                        every |x|^2 < 2^53
// Partials of the first four: slot ((i / 4) * sideR + j / 4) * 16 + (i % 4) * 4 + j % 4 of pair (left i, right j), sideR =
// ceil(R / 4), `ngroups` workgroup partials per slot -- reduced in a fixed order by reduce_partials_kernel.  Rows past the
// end of a set are masked (their address is clamped to the last profile, their results are never written).
#pragma once
#include "vec_kernels.hpp"
#include "gram_kernels.hpp"

namespace kpal {

struct CrossSets {
    const int64_t *left;    // Q x n
    const int64_t *right;   // R x n
    int Q, R;
    uint64_t n;
};

__device__ __forceinline__ uint64_t cross_slot(int sideR, int i, int j)
{
    return ((uint64_t)(i >> 2) * (uint64_t)sideR + (uint64_t)(j >> 2)) * 16u + (uint64_t)((i & 3) * 4 + (j & 3));
}

// Staged row r of super-tile (si, sj): rows 0..15 are left profiles, 16..31 right ones.
__device__ __forceinline__ const int64_t *cross_row(const CrossSets &c, int si, int sj, int r)
{
    return r < 16 ? c.left + (uint64_t)min(si * 16 + r, c.Q - 1) * c.n : c.right + (uint64_t)min(sj * 16 + (r - 16), c.R - 1) * c.n;
}

// The 1-D grid of the staged kernels, cut like matrix_rdiff_kernel's: the `nsuper` workgroups that stage the SAME bins are
// neighbours on ONE XCD (the left rows of a bin range are then read from HBM once per XCD and hit its L2 afterwards).
// Linear id L = (c * nsuper + s) * 8 + x  ->  super-tile s, bin-group c * 8 + x; the host launches nsuper * a multiple of 8.
struct CrossBlock {
    int si, sj;
    uint32_t group, ngroups;
};
__device__ __forceinline__ CrossBlock cross_block(uint32_t nsuper, int superR)
{
    const uint32_t lin = blockIdx.x, xcd = lin & 7u, sidx = (lin >> 3) % nsuper, cgrp = (lin >> 3) / nsuper;
    return CrossBlock{(int)(sidx / (uint32_t)superR), (int)(sidx % (uint32_t)superR), cgrp * 8u + xcd, gridDim.x / nsuper};
}

// blockIdx.x = tile * gx + slice: tile (tq, tr) of 4 x 4 pairs, the slices stride over the bins.
template <int METRIC>
__global__ __launch_bounds__(256) void cross_tile_kernel(const CrossSets c, uint32_t gx, Partial *__restrict__ partials)
{
    constexpr int TILE = 4;
    const int sideR = (c.R + TILE - 1) / TILE;
    const uint32_t tile = blockIdx.x / gx, slice = blockIdx.x % gx;
    const int tq = (int)(tile / (uint32_t)sideR), tr = (int)(tile % (uint32_t)sideR);
    double s[TILE][TILE];
    unsigned long long m[TILE][TILE];
    uint32_t mf[TILE][TILE];
#pragma unroll
    for (int a = 0; a < TILE; ++a)
#pragma unroll
        for (int b = 0; b < TILE; ++b) {
            s[a][b] = 0.0;
            m[a][b] = 0ULL;
            mf[a][b] = 0u;
        }
    TermBytes<TILE> tb = {{0u, 0u, 0u, 0u}, 0u};
    const int64_t *rowp[TILE];
    const int64_t *colp[TILE];
#pragma unroll
    for (int a = 0; a < TILE; ++a) {
        rowp[a] = c.left + (uint64_t)min(tq * TILE + a, c.Q - 1) * c.n;
        colp[a] = c.right + (uint64_t)min(tr * TILE + a, c.R - 1) * c.n;
    }
    for (uint64_t i = (uint64_t)slice * blockDim.x + threadIdx.x; i < c.n; i += (uint64_t)gx * blockDim.x) {
        int64_t x[TILE], y[TILE];
#pragma unroll
        for (int a = 0; a < TILE; ++a) {
            x[a] = rowp[a][i];
            y[a] = colp[a][i];
        }
        matrix_accumulate<METRIC, TILE>(x, y, s, m, mf, tb);
    }
    term_bytes_flush(tb, mf);
#pragma unroll
    for (int a = 0; a < TILE; ++a)
#pragma unroll
        for (int b = 0; b < TILE; ++b) {
            Partial p = {s[a][b], METRIC != 2 ? (unsigned long long)mf[a][b] : m[a][b]};
            p = block_reduce(p);
            if (threadIdx.x == 0) partials[((uint64_t)tile * TILE * TILE + a * TILE + b) * gx + slice] = p;
        }
}

// matrix_super_kernel over a rectangle: 64 bins of 16 left and 16 right profiles per stage, the next stage's loads in
// flight during the arithmetic, sixteen 16-lane groups with one 4 x 4 register tile each.
template <int METRIC>
__global__ __launch_bounds__(256) void cross_super_kernel(const CrossSets c, uint32_t nsuper, int superR, Partial *__restrict__ partials)
{
    constexpr int TILE = 4;
    constexpr bool RCP = METRIC == 0;              // 'prod': reciprocals 1 / (x + 1) staged next to the values
    __shared__ int64_t stage[2][32][kSuperRow];
    __shared__ double rstage[RCP ? 2 : 1][RCP ? 32 : 1][RCP ? kSuperRow : 1];
    auto put = [&](int buf, int row, int col, int64_t v) {
        stage[buf][row][col] = v;
        if constexpr (RCP) rstage[buf][row][col] = rcp_counts((double)(uint32_t)v + 1.0);   // (unused when v >= 2^31)
    };
    const CrossBlock blk = cross_block(nsuper, superR);
    const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
    const int ti = blk.si * 4 + (g >> 2), tj = blk.sj * 4 + (g & 3);
    const int sideQ = (c.Q + TILE - 1) / TILE, sideR = (c.R + TILE - 1) / TILE;
    const bool mine = ti < sideQ && tj < sideR;        // this group's 4 x 4 tile is part of the rectangle
    double s[TILE][TILE];
    unsigned long long m[TILE][TILE];
    uint32_t mf[TILE][TILE];
#pragma unroll
    for (int a = 0; a < TILE; ++a)
#pragma unroll
        for (int b = 0; b < TILE; ++b) {
            s[a][b] = 0.0;
            m[a][b] = 0ULL;
            mf[a][b] = 0u;
        }
    TermBytes<TILE> tb = {{0u, 0u, 0u, 0u}, 0u};
    // loader: value q of thread t is bin (t & 63) of staged row 4 q + (t >> 6): a wave reads one 512-byte run
    const int lrow = threadIdx.x >> 6, lcol = threadIdx.x & 63;
    const int64_t *src[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) src[q] = cross_row(c, blk.si, blk.sj, 4 * q + lrow) + lcol;
    const uint64_t chunks = c.n / kSuperBins;
    int64_t next[8];
    uint64_t ch = blk.group;
    if (ch < chunks) {
#pragma unroll
        for (int q = 0; q < 8; ++q) put(0, 4 * q + lrow, lcol, src[q][ch * kSuperBins]);
    }
    __syncthreads();
    int cur = 0;
    for (; ch < chunks; ch += blk.ngroups) {
        const bool more = ch + blk.ngroups < chunks;   // block-uniform
        if (more) {
#pragma unroll
            for (int q = 0; q < 8; ++q) next[q] = src[q][(ch + blk.ngroups) * kSuperBins];
        }
        if (mine) {
#pragma unroll 1
            for (int u = 0; u < kSuperBins / 16; ++u) {
                int64_t x[TILE], y[TILE];
#pragma unroll
                for (int a = 0; a < TILE; ++a) {
                    x[a] = stage[cur][4 * (g >> 2) + a][16 * u + l];
                    y[a] = stage[cur][16 + 4 * (g & 3) + a][16 * u + l];
                }
                if constexpr (RCP) {
                    double rx[TILE], ry[TILE];
#pragma unroll
                    for (int a = 0; a < TILE; ++a) {
                        rx[a] = rstage[cur][4 * (g >> 2) + a][16 * u + l];
                        ry[a] = rstage[cur][16 + 4 * (g & 3) + a][16 * u + l];
                    }
                    matrix_accumulate_prod_rcp<TILE>(x, y, rx, ry, s, m, mf, tb);
                } else {
                    matrix_accumulate<METRIC, TILE>(x, y, s, m, mf, tb);
                }
            }
        }
        if (more) {
#pragma unroll
            for (int q = 0; q < 8; ++q) put(cur ^ 1, 4 * q + lrow, lcol, next[q]);
        }
        __syncthreads();
        cur ^= 1;
    }
    term_bytes_flush(tb, mf);
    // per-group reduction over its 16 lanes (fixed order), lane 0 of the group writes
#pragma unroll
    for (int a = 0; a < TILE; ++a)
#pragma unroll
        for (int b = 0; b < TILE; ++b) {
            double ps = s[a][b];
            unsigned long long pm = METRIC != 2 ? (unsigned long long)mf[a][b] : m[a][b];
#pragma unroll
            for (int d = 8; d >= 1; d >>= 1) {
                ps += __shfl_down(ps, d, 16);
                pm += __shfl_down(pm, d, 16);
            }
            if (mine && l == 0)
                partials[(((uint64_t)ti * sideR + tj) * TILE * TILE + a * TILE + b) * blk.ngroups + blk.group] = Partial{ps, pm};
        }
}

// The zero mask of a staged row from the loader's two ballots (matrix_rdiff_kernel): bit c = bin 2c, bit 32 + c = bin 2c + 1.
__device__ __forceinline__ unsigned long long cross_zero_mask(const longlong2 &v, int lhalf)
{
    const unsigned long long z0 = __builtin_amdgcn_ballot_w64(v.x == 0), z1 = __builtin_amdgcn_ballot_w64(v.y == 0);
    return lhalf ? ((z0 >> 32) | (z1 & 0xFFFFFFFF00000000ull)) : ((z0 & 0xFFFFFFFFull) | (z1 << 32));
}

// FORM 0: multiset 'prod' as | 1/(y + 1) - 1/(x + 1) | over staged reciprocals (matrix_rdiff_kernel: accuracy, table and
// the kRdiffMaxCount limit are argued there).  FORM 1: multiset 'sum' as |x - y| * T[x + y] over staged 32-bit counts
// (matrix_rsum_kernel).  Same loader (16-byte loads, two rows per wave), zero masks and popcounts for the term counts.  A count
// outside the form's range raises *big and the caller reruns cross_super_kernel; the partials must be zeroed before the
// launch (.s and .m of a slot come from different threads).
template <int FORM>
__global__ __launch_bounds__(256) void cross_recip_kernel(const CrossSets c, uint32_t nsuper, int superR, Partial *__restrict__ partials,
                                                          uint32_t *__restrict__ big)
{
    constexpr int TILE = 4;
    constexpr int kTable = FORM == 0 ? kRdiffTable : kRsumTable;
    __shared__ __attribute__((aligned(16))) double rstage[FORM == 0 ? 2 : 1][FORM == 0 ? 32 : 1][FORM == 0 ? kRdiffRow : 2];
    __shared__ __attribute__((aligned(16))) uint32_t cstage[FORM == 1 ? 2 : 1][FORM == 1 ? 32 : 1][FORM == 1 ? kSuperBins : 4];
    __shared__ unsigned long long zmask[2][32];
    __shared__ double rtable[kTable];
    for (int i = threadIdx.x; i < kTable; i += 256) rtable[i] = rcp_counts((double)i + 1.0);
    const CrossBlock blk = cross_block(nsuper, superR);
    const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
    const int ti = blk.si * 4 + (g >> 2), tj = blk.sj * 4 + (g & 3);
    const int sideQ = (c.Q + TILE - 1) / TILE, sideR = (c.R + TILE - 1) / TILE;
    const bool mine = ti < sideQ && tj < sideR;
    double s[TILE][TILE];
#pragma unroll
    for (int a = 0; a < TILE; ++a)
#pragma unroll
        for (int b = 0; b < TILE; ++b) s[a][b] = 0.0;
    uint32_t both_zero = 0;                            // pair (row threadIdx.x >> 4, column threadIdx.x & 15) of the super-tile
    bool saw_big = false;
    const int lrow = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lhalf = (threadIdx.x >> 5) & 1, lcol = threadIdx.x & 31;
    const int64_t *src[4][2];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int h = 0; h < 2; ++h) src[q][h] = cross_row(c, blk.si, blk.sj, 8 * q + 2 * lrow + h);   // (uniform)
    __syncthreads();                                   // the table
    auto put = [&](int buf, int q, const longlong2 &v) {
        const int row = 8 * q + 2 * lrow + lhalf;
        if constexpr (FORM == 0) {
            const bool all_small = __all((unsigned long long)v.x < (unsigned long long)kTable && (unsigned long long)v.y < (unsigned long long)kTable);   // wave-uniform
            auto recip = [&](int64_t w) -> double {
                if (all_small) return rtable[(uint32_t)w];
                saw_big |= (unsigned long long)w >= kRdiffMaxCount;
                return (unsigned long long)w < (unsigned long long)kTable ? rtable[(uint32_t)w & (kTable - 1)] : rcp_counts((double)(uint32_t)w + 1.0);
            };
            double2 r;
            r.x = recip(v.x);
            r.y = recip(v.y);
            *reinterpret_cast<double2 *>(&rstage[buf][row][2 * lcol]) = r;
        } else {
            saw_big |= (unsigned long long)v.x >= (unsigned long long)(kTable / 2) || (unsigned long long)v.y >= (unsigned long long)(kTable / 2);   // (x + y must stay inside the table)
            // (masked: a larger count only ever costs a rerun, never an out-of-range read)
            *reinterpret_cast<uint2 *>(&cstage[buf][row][2 * lcol]) =
                make_uint2((uint32_t)v.x & (uint32_t)(kTable / 2 - 1), (uint32_t)v.y & (uint32_t)(kTable / 2 - 1));
        }
        const unsigned long long z = cross_zero_mask(v, lhalf);
        if (lcol == 0) zmask[buf][row] = z;
    };
    const uint64_t chunks = c.n / kSuperBins;
    auto request = [&](longlong2 (&dst)[4], uint64_t chunk) {
        if (chunk < chunks) {                          // block-uniform
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t *p = lhalf ? src[q][1] : src[q][0];
                dst[q] = *reinterpret_cast<const longlong2 *>(p + chunk * kSuperBins + 2 * lcol);
            }
        }
    };
    auto compute = [&](int cur) {
        both_zero += (uint32_t)__popcll(zmask[cur][threadIdx.x >> 4] & zmask[cur][16 + (threadIdx.x & 15)]);
        if (!mine) return;
        if constexpr (FORM == 0) {
            // lane l takes the bin pairs (2l, 2l+1) and (32 + 2l, 32 + 2l + 1): 16-byte LDS reads
#pragma unroll
            for (int u = 0; u < kSuperBins / 32; ++u) {
                double2 rx[TILE], ry[TILE];
#pragma unroll
                for (int a = 0; a < TILE; ++a) {
                    rx[a] = *reinterpret_cast<const double2 *>(&rstage[cur][4 * (g >> 2) + a][32 * u + 2 * l]);
                    ry[a] = *reinterpret_cast<const double2 *>(&rstage[cur][16 + 4 * (g & 3) + a][32 * u + 2 * l]);
                }
#pragma unroll
                for (int a = 0; a < TILE; ++a)
#pragma unroll
                    for (int b = 0; b < TILE; ++b) {
                        s[a][b] += fabs(rx[a].x - ry[b].x);
                        s[a][b] += fabs(rx[a].y - ry[b].y);
                    }
            }
        } else {
            // lane l takes the bins 4l .. 4l+3 of every row: one 16-byte LDS read per row
            uint4 cx[TILE], cy[TILE];
#pragma unroll
            for (int a = 0; a < TILE; ++a) {
                cx[a] = *reinterpret_cast<const uint4 *>(&cstage[cur][4 * (g >> 2) + a][4 * l]);
                cy[a] = *reinterpret_cast<const uint4 *>(&cstage[cur][16 + 4 * (g & 3) + a][4 * l]);
            }
            const char *tab = reinterpret_cast<const char *>(rtable);
#pragma unroll
            for (int a = 0; a < TILE; ++a)
#pragma unroll
                for (int b = 0; b < TILE; ++b) {
                    // one pair (four terms) at a time keeps the register count at four waves per SIMD (matrix_rsum_kernel)
                    asm volatile("" : "+v"(cy[b].x), "+v"(cy[b].y), "+v"(cy[b].z), "+v"(cy[b].w));
                    const uint32_t x[4] = {cx[a].x, cx[a].y, cx[a].z, cx[a].w}, y[4] = {cy[b].x, cy[b].y, cy[b].z, cy[b].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        uint32_t d;
                        asm("v_sad_u32 %0, %1, %2, 0" : "=v"(d) : "v"(x[e]), "v"(y[e]));   // |x - y|
                        const double r = *reinterpret_cast<const double *>(tab + ((x[e] + y[e]) << 3));
                        s[a][b] = fma((double)d, r, s[a][b]);
                    }
                }
        }
    };
    longlong2 next[4];
    uint64_t ch = blk.group;
    uint64_t stages = 0;
    request(next, ch);
    if (ch < chunks) {
#pragma unroll
        for (int q = 0; q < 4; ++q) put(0, q, next[q]);
    }
    __syncthreads();
    int cur = 0;
    const uint64_t my_stages = blk.group < chunks ? (chunks - blk.group + blk.ngroups - 1) / blk.ngroups : 1;
    for (; ch < chunks; ch += blk.ngroups, ++stages) {
        const bool more = ch + blk.ngroups < chunks;   // block-uniform
        if ((stages & 15u) == 0) matrix_stage_priority(stages, my_stages);
        request(next, ch + blk.ngroups);
        compute(cur);
        if (more) {
#pragma unroll
            for (int q = 0; q < 4; ++q) put(cur ^ 1, q, next[q]);
        }
        __syncthreads();
        cur ^= 1;
    }
    if (saw_big) atomicOr(big, 1u);
    // sums: per-group reduction over its 16 lanes (fixed order), lane 0 of the group writes .s
#pragma unroll
    for (int a = 0; a < TILE; ++a)
#pragma unroll
        for (int b = 0; b < TILE; ++b) {
            double ps = s[a][b];
#pragma unroll
            for (int d = 8; d >= 1; d >>= 1) ps += __shfl_down(ps, d, 16);
            if (mine && l == 0)
                partials[(((uint64_t)ti * sideR + tj) * TILE * TILE + a * TILE + b) * blk.ngroups + blk.group].s = ps;
        }
    // term counts: thread (i, j) of the super-tile writes .m = bins seen - bins where both are zero
    {
        const int i = blk.si * 16 + (int)(threadIdx.x >> 4), j = blk.sj * 16 + (int)(threadIdx.x & 15);
        if ((i >> 2) < sideQ && (j >> 2) < sideR) partials[cross_slot(sideR, i, j) * blk.ngroups + blk.group].m = stages * kSuperBins - both_zero;
    }
}

// |x|^2 of every profile of both sets in fp64: blockIdx.x = profile * gx + slice (profiles 0..Q-1 left, Q.. right).  Every
// partial sum of the non-negative squares is an integer, so a total below 2^53 was formed without a rounding -- and since
// rounding is monotone, a true total of 2^53 or more is never reported below it.
__global__ __launch_bounds__(256) void cross_norm_kernel(const CrossSets c, uint32_t gx, Partial *__restrict__ partials)
{
    const uint32_t p = blockIdx.x / gx, slice = blockIdx.x % gx;
    const int64_t *v = p < (uint32_t)c.Q ? c.left + (uint64_t)p * c.n : c.right + (uint64_t)(p - (uint32_t)c.Q) * c.n;
    Partial acc = {0.0, 0ULL};
    for (uint64_t i = (uint64_t)slice * blockDim.x + threadIdx.x; i < c.n; i += (uint64_t)gx * blockDim.x) {
        const double x = (double)v[i];
        acc.s += x * x;
    }
    acc = block_reduce(acc);
    if (threadIdx.x == 0) partials[(uint64_t)p * gx + slice] = acc;
}

// gram_mfma_kernel's off-diagonal block over two sets: 64 left x 64 right profiles per workgroup, A . B^T accumulated by
// mfma_f64_16x16x4f64 from LDS-staged fp64 copies of the counts.  blockIdx.x = block * gx + slice, block = I * blocksR + J.
// Partials: ((block * 16 + gi * 4 + gj) * 256 + row * 16 + col) * gx + slice, .s = the partial dot product.
__global__ __launch_bounds__(256) void cross_gram_kernel(const CrossSets c, uint32_t gx, int blocksR, Partial *__restrict__ partials)
{
    __shared__ double stage[2][128][kGramRow];
    const uint32_t block = blockIdx.x / gx, slice = blockIdx.x % gx;
    const int I = (int)(block / (uint32_t)blocksR), J = (int)(block % (uint32_t)blocksR);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // loader: value q of thread t is bin (t & 63) of staged row 4 q + (t >> 6): a wave reads one 512-byte run
    const int lrow = threadIdx.x >> 6, lcol = threadIdx.x & 63;
    auto load_slab = [&](uint64_t ch, int64_t (&v)[32]) {
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int pl = I * 64 + 4 * q + lrow, pr = J * 64 + 4 * q + lrow;
            v[q] = pl < c.Q ? c.left[(uint64_t)pl * c.n + ch * kGramBins + lcol] : 0;
            v[16 + q] = pr < c.R ? c.right[(uint64_t)pr * c.n + ch * kGramBins + lcol] : 0;
        }
    };
    auto store_slab = [&](int buf, const int64_t (&v)[32]) {
#pragma unroll
        for (int sidx = 0; sidx < 2; ++sidx)
#pragma unroll
            for (int q = 0; q < 16; ++q) stage[buf][sidx * 64 + 4 * q + lrow][lcol] = (double)v[sidx * 16 + q];
    };
    gram_v4f64 acc[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) acc[t] = gram_v4f64{0.0, 0.0, 0.0, 0.0};
    const uint64_t slabs = c.n / kGramBins;
    uint64_t ch = slice;
    int64_t next[32];
    if (ch < slabs) {
        load_slab(ch, next);
        store_slab(0, next);
    }
    __syncthreads();
    int cur = 0;
    for (; ch < slabs; ch += gx) {
        const bool more = ch + gx < slabs;             // block-uniform
        if (more) load_slab(ch + gx, next);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int q = wave + 4 * u;
            double a[4], b[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                a[g] = stage[cur][16 * g + (lane & 15)][4 * q + (lane >> 4)];
                b[g] = stage[cur][64 + 16 * g + (lane & 15)][4 * q + (lane >> 4)];
            }
#pragma unroll
            for (int gi = 0; gi < 4; ++gi)
#pragma unroll
                for (int gj = 0; gj < 4; ++gj) acc[gi * 4 + gj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[gi], b[gj], acc[gi * 4 + gj], 0, 0, 0);
        }
        if (more) store_slab(cur ^ 1, next);
        __syncthreads();
        cur ^= 1;
    }
    // sum the four waves' accumulators (fixed order) and write this workgroup's partial block
    double *red = &stage[0][0][0];                     // 4 x 256 doubles
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave * 256 + ((lane >> 4) + 4 * r) * 16 + (lane & 15)] = acc[t][r];
        __syncthreads();
        const int e = threadIdx.x;                     // element row * 16 + col of the tile
        const double sum = ((red[e] + red[256 + e]) + red[512 + e]) + red[768 + e];
        partials[(((uint64_t)block * 16 + t) * 256 + e) * gx + slice] = Partial{sum, 0ULL};
    }
}

}  // namespace kpal
