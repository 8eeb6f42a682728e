// cross_kernels.hpp -- every pair (left i, right j) of two SETS of profiles: the Q x R rectangle of kpal_cross_distance[_device]
// and, with CrossSets::tri, the lower triangle of one set against itself (kdistlib.distance_matrix, kpal/kdistlib.py:179-186:
// kpal_distance_matrix[_device]).  One set of kernels serves both -- the triangle is a set crossed with itself of which only
// the tiles on or below the diagonal exist -- and both kinds of arithmetic: the plain metrics (PlainAcc below) and every
// ProfileDistance with options (OptAcc, cross_option_kernels.hpp) are accumulators plugged into the same two skeletons.
//   cross_tile_kernel     4 x 4 register tiles straight from global memory: few profiles on a side (the long side streams
//                         past once, the short side's bins stay in the caches) and k < 6
//   cross_super_kernel    16 x 16 super-tiles staged through LDS, any values (the fallback of the two below, and euclidean
//                         where the Gram form does not apply)
//   cross_recip_kernel<0> multiset 'prod' as a difference of reciprocals, counts in [0, 2^16)
//   cross_recip_kernel<1> multiset 'sum' with the reciprocal of the denominator from a table
//   cross_gram_kernel     euclidean from A . B^T on the fp64 matrix cores plus the norms of cross_norm_kernel, exact while
//                         every |x|^2 < 2^53 (rectangle only; the triangle's is gram_kernels.hpp)
// Tiles: tile (ti, tj) of 4 x 4 pairs has number ti * sideR + tj, sideR = ceil(R / 4), or -- tri, tj <= ti -- ti (ti + 1) / 2 + tj;
// super-tiles of 16 x 16 pairs likewise.  The number is computed from the block id: no list of tiles is uploaded.
// Partials of the first four: accumulator a of pair (i, j) lies at (a * slots + cross_slot(i, j)) * ngroups + group, slots =
// 16 * tiles, `ngroups` workgroup partials per slot -- reduced in a fixed order by reduce_partials_kernel.  Rows past the end
// of a set are masked (their address is clamped to the last profile, their results are never written); so are, in a
// triangle, the tiles above the diagonal.
#pragma once
#include "matrix_common.hpp"
#include "gram_kernels.hpp"

namespace kpal {

// What a kernel of the two skeletons is launched with; the plain accumulators read `c` alone.
struct CrossOpt {
    CrossSets c;
    int down;                // metrics.scale_down
    const Partial *totals;   // SCALED: reduced totals (.m), per profile (left 0 .. Q-1, right from `roff`) or per pair slot
    uint32_t roff;
    uint32_t slots;          // 16 * tiles: the stride between the accumulators of one pair
};
// ... of an accumulator with CODES (SmoothAcc, smooth_set_kernels.hpp): one code per node beside the values, profile p's at
// codes + p * cstride.  cshift 0: the elements ARE the nodes; 2: the elements are bins, whose code follows from bottom node
// (bin >> 2)'s.  An accumulator names what its kernels are launched with (Opt), so the others' arguments stay what they were.
struct CrossCodeOpt : CrossOpt {
    const uint8_t *lcodes, *rcodes;
    uint64_t cstride;
    int cshift;
};

// The code of element i of a profile whose node codes lie at `codes` (CrossCodeOpt::cshift).
__device__ __forceinline__ uint8_t cross_code(const uint8_t *codes, uint64_t i, int shift)
{
    const uint8_t c = codes[i >> shift];
    return shift ? (uint8_t)(c ? 2 : 1) : c;
}

constexpr int kCodeRow = 80;   // bytes of a staged row of codes: rows four apart lie 16 banks apart for the groups' 4-byte reads

// Number t of a tile (or super-tile) -> (ti, tj): row-major over `side` columns, or the lower triangle's ti (ti + 1) / 2 + tj.
__device__ __forceinline__ void cross_tile(uint32_t t, int side, bool tri, int &ti, int &tj)
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

// (the other way, cross_tile_number, and cross_slot, the slot of a pair: matrix_plan.hpp -- the host finds the pairs with them)

// Staged row r of super-tile (si, sj): rows 0..15 are left profiles, 16..31 right ones.
__device__ __forceinline__ const int64_t *cross_row(const CrossSets &c, int si, int sj, int r)
{
    return r < 16 ? c.left + (uint64_t)min(si * 16 + r, c.Q - 1) * c.n : c.right + (uint64_t)min(sj * 16 + (r - 16), c.R - 1) * c.n;
}

// The 1-D grid of the staged kernels.  Every profile is staged by several super-tiles (64 profiles in a triangle: 10
// super-tiles x 32 rows = 5 x the profiles' bytes, 43 GB at k = 12 -- more than the arithmetic takes).  Workgroups are
// dispatched round-robin over the 8 XCDs, each with its own L2: the grid is cut so that the `nsuper` workgroups that stage the
// SAME bins are neighbours on ONE XCD -- linear id L = (c * nsuper + s) * 8 + x  ->  super-tile s, bin-group c * 8 + x -- and the
// second to tenth reader of a line hits that L2.  The host launches nsuper * a multiple of 8 workgroups.
struct CrossBlock {
    int si, sj;
    uint32_t group, ngroups;
};
__device__ __forceinline__ CrossBlock cross_block(const CrossSets &c, uint32_t nsuper, int superR)
{
    const uint32_t lin = blockIdx.x, xcd = lin & 7u, sidx = (lin >> 3) % nsuper, cgrp = (lin >> 3) / nsuper;
    CrossBlock blk = {0, 0, cgrp * 8u + xcd, gridDim.x / nsuper};
    cross_tile(sidx, superR, c.tri != 0, blk.si, blk.sj);
    return blk;
}

// The tile of group g (16 lanes, one 4 x 4 register tile) of a staged workgroup: (4 si + g / 4, 4 sj + g % 4).  A group whose
// tile lies outside the rectangle, or above the diagonal of a triangle, only helps with the staging.
struct CrossGroup {
    int ti, tj, sideR;
    bool mine;
};
__device__ __forceinline__ CrossGroup cross_group(const CrossSets &c, const CrossBlock &blk, int g)
{
    const int ti = blk.si * 4 + (g >> 2), tj = blk.sj * 4 + (g & 3);
    const int sideQ = (c.Q + 3) / 4, sideR = (c.R + 3) / 4;
    return CrossGroup{ti, tj, sideR, ti < sideQ && tj < sideR && (!c.tri || tj <= ti)};
}

// The plain metrics (0 / 1: multiset prod / sum, metrics.py:121-123; 2: euclidean as a wrapping int64 dot, metrics.py:135,46)
// as an accumulator of the two skeletons.  An accumulator says how many (s, m) pairs it writes per pair of profiles (NACC),
// whether the staged skeleton should stage the reciprocals 1 / (x + 1) beside the values (RCP: 'prod' then takes
// matrix_accumulate_prod_rcp), whether it takes a code per value as well (CODES: add(x, y, cx, cy)), and what a pair's
// (s, m) is once the bins are through.
template <int METRIC>
struct PlainAcc {
    static constexpr int NACC = 1;
    static constexpr bool RCP = METRIC == 0;
    static constexpr bool CODES = false;
    using Opt = CrossOpt;
    double s[4][4];
    unsigned long long m[4][4];   // the euclidean dots
    uint32_t mf[4][4];            // multiset: number of terms (a thread sees fewer than 2^32 bins)
    TermBytes<4> tb;

    __device__ __forceinline__ void begin(const CrossOpt &, int, int, uint32_t)
    {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                s[a][b] = 0.0;
                m[a][b] = 0ULL;
                mf[a][b] = 0u;
            }
            tb.packed[a] = 0u;
        }
        tb.bins = 0u;
    }
    __device__ __forceinline__ void add(const int64_t (&x)[4], const int64_t (&y)[4]) { matrix_accumulate<METRIC, 4>(x, y, s, m, mf, tb); }
    __device__ __forceinline__ void add(const int64_t (&x)[4], const int64_t (&y)[4], const double (&rx)[4], const double (&ry)[4])
    {
        matrix_accumulate_prod_rcp<4>(x, y, rx, ry, s, m, mf, tb);
    }
    __device__ __forceinline__ void finish() { term_bytes_flush(tb, mf); }
    __device__ __forceinline__ Partial partial(int, int a, int b) const
    {
        return Partial{s[a][b], METRIC != 2 ? (unsigned long long)mf[a][b] : m[a][b]};
    }
};

// blockIdx.x = tile * gx + slice: tile (tq, tr) of 4 x 4 pairs, the slices stride over the bins.  Each thread streams one
// bin at a time of the four row and four column profiles (coalesced 512-byte wave loads per profile).
template <class Acc>
__global__ __launch_bounds__(256) void cross_tile_kernel(const typename Acc::Opt o, uint32_t gx, Partial *__restrict__ partials)
{
    const CrossSets &c = o.c;
    const int sideR = (c.R + 3) / 4;
    const uint32_t tile = blockIdx.x / gx, slice = blockIdx.x % gx;
    int tq, tr;
    cross_tile(tile, sideR, c.tri != 0, tq, tr);
    Acc acc;
    acc.begin(o, tq, tr, tile);
    const int64_t *rowp[4];
    const int64_t *colp[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        rowp[a] = c.left + (uint64_t)min(tq * 4 + a, c.Q - 1) * c.n;
        colp[a] = c.right + (uint64_t)min(tr * 4 + a, c.R - 1) * c.n;
    }
    const uint8_t *rowc[Acc::CODES ? 4 : 1];
    const uint8_t *colc[Acc::CODES ? 4 : 1];
    if constexpr (Acc::CODES) {
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            rowc[a] = o.lcodes + (uint64_t)min(tq * 4 + a, c.Q - 1) * o.cstride;
            colc[a] = o.rcodes + (uint64_t)min(tr * 4 + a, c.R - 1) * o.cstride;
        }
    }
    for (uint64_t i = (uint64_t)slice * blockDim.x + threadIdx.x; i < c.n; i += (uint64_t)gx * blockDim.x) {
        int64_t x[4], y[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            x[a] = rowp[a][i];
            y[a] = colp[a][i];
        }
        if constexpr (Acc::CODES) {
            uint8_t cx[4], cy[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                cx[a] = cross_code(rowc[a], i, o.cshift);
                cy[a] = cross_code(colc[a], i, o.cshift);
            }
            acc.add(x, y, cx, cy);
        } else {
            acc.add(x, y);
        }
    }
    acc.finish();
#pragma unroll
    for (int n = 0; n < Acc::NACC; ++n)
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const Partial p = block_reduce(acc.partial(n, a, b));
                if (threadIdx.x == 0) partials[((uint64_t)n * o.slots + (uint64_t)tile * 16u + (uint64_t)(a * 4 + b)) * gx + slice] = p;
            }
}

// 16 x 16 SUPER-tiles staged through LDS (k >= 6): a workgroup loads 64 bins of its 16 row and 16 column profiles once
// (512-byte runs, the next stage's loads in flight during the arithmetic) and its 16 groups of 16 lanes compute the sixteen
// 4 x 4 register tiles from LDS -- a quarter of the global loads per term of cross_tile_kernel, whose 146 GB of (cached)
// loads bound the euclidean matrix of 64 profiles at k = 12 and nearly bound the multiset one.  Rows are padded to 68 bins
// so that the column rows of the two groups of a half-wave (4 rows apart) sit 32 banks apart for ds_read_b64.  Grid:
// cross_block; bin-group g takes the chunks g, g + ngroups, ...
template <class Acc>
__global__ __launch_bounds__(256) void cross_super_kernel(const typename Acc::Opt o, uint32_t nsuper, int superR, Partial *__restrict__ partials)
{
    constexpr bool RCP = Acc::RCP;                 // 'prod': reciprocals 1 / (x + 1) staged next to the values
    __shared__ int64_t stage[2][32][kSuperRow];
    __shared__ double rstage[RCP ? 2 : 1][RCP ? 32 : 1][RCP ? kSuperRow : 1];
    auto put = [&](int buf, int row, int col, int64_t v) {
        stage[buf][row][col] = v;
        if constexpr (RCP) rstage[buf][row][col] = rcp_counts((double)(uint32_t)v + 1.0);   // (unused when v >= 2^31)
    };
    // CODES: the code of bin 16 u + l of a row is byte u of its word l -- a lane reads the codes of its four bins at once
    constexpr bool CODES = Acc::CODES;
    __shared__ __attribute__((aligned(4))) uint8_t cstage[CODES ? 2 : 1][CODES ? 32 : 1][CODES ? kCodeRow : 4];
    auto put_code = [&](int buf, int row, int col, uint8_t v) { cstage[buf][row][4 * (col & 15) + (col >> 4)] = v; };
    const CrossSets &c = o.c;
    const CrossBlock blk = cross_block(c, nsuper, superR);
    const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
    const CrossGroup grp = cross_group(c, blk, g);
    const bool mine = grp.mine;
    const uint32_t tile = mine ? cross_tile_number(grp.ti, grp.tj, grp.sideR, c.tri != 0) : 0u;
    Acc acc;
    acc.begin(o, mine ? grp.ti : 0, mine ? grp.tj : 0, tile);
    // loader: value q of thread t is bin (t & 63) of staged row 4 q + (t >> 6): a wave reads one 512-byte run
    const int lrow = threadIdx.x >> 6, lcol = threadIdx.x & 63;
    const int64_t *src[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) src[q] = cross_row(c, blk.si, blk.sj, 4 * q + lrow) + lcol;
    const uint8_t *csrc[CODES ? 8 : 1];
    if constexpr (CODES) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int r = 4 * q + lrow;
            csrc[q] = r < 16 ? o.lcodes + (uint64_t)min(blk.si * 16 + r, c.Q - 1) * o.cstride
                             : o.rcodes + (uint64_t)min(blk.sj * 16 + (r - 16), c.R - 1) * o.cstride;
        }
    }
    const uint64_t chunks = c.n / kSuperBins;
    int64_t next[8];
    uint8_t nextc[CODES ? 8 : 1];
    uint64_t ch = blk.group;
    if (ch < chunks) {
#pragma unroll
        for (int q = 0; q < 8; ++q) put(0, 4 * q + lrow, lcol, src[q][ch * kSuperBins]);
        if constexpr (CODES) {
#pragma unroll
            for (int q = 0; q < 8; ++q) put_code(0, 4 * q + lrow, lcol, cross_code(csrc[q], ch * kSuperBins + lcol, o.cshift));
        }
    }
    __syncthreads();
    int cur = 0;
    for (; ch < chunks; ch += blk.ngroups) {
        const bool more = ch + blk.ngroups < chunks;   // block-uniform
        if (more) {
#pragma unroll
            for (int q = 0; q < 8; ++q) next[q] = src[q][(ch + blk.ngroups) * kSuperBins];
            if constexpr (CODES) {
#pragma unroll
                for (int q = 0; q < 8; ++q) nextc[q] = cross_code(csrc[q], (ch + blk.ngroups) * kSuperBins + lcol, o.cshift);
            }
        }
        if (mine) {
            uint32_t wx[CODES ? 4 : 1], wy[CODES ? 4 : 1];
            if constexpr (CODES) {
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    wx[a] = *reinterpret_cast<const uint32_t *>(&cstage[cur][4 * (g >> 2) + a][4 * l]);
                    wy[a] = *reinterpret_cast<const uint32_t *>(&cstage[cur][16 + 4 * (g & 3) + a][4 * l]);
                }
            }
#pragma unroll 1   // (unrolled 2 / 4 times: 21.3 / 20.4 ms against 19.9 for 64 profiles at k = 12)
            for (int u = 0; u < kSuperBins / 16; ++u) {
                int64_t x[4], y[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    x[a] = stage[cur][4 * (g >> 2) + a][16 * u + l];
                    y[a] = stage[cur][16 + 4 * (g & 3) + a][16 * u + l];
                }
                if constexpr (RCP) {
                    double rx[4], ry[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        rx[a] = rstage[cur][4 * (g >> 2) + a][16 * u + l];
                        ry[a] = rstage[cur][16 + 4 * (g & 3) + a][16 * u + l];
                    }
                    acc.add(x, y, rx, ry);
                } else if constexpr (CODES) {
                    uint8_t cx[4], cy[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        cx[a] = (uint8_t)(wx[a] >> (8 * u));
                        cy[a] = (uint8_t)(wy[a] >> (8 * u));
                    }
                    acc.add(x, y, cx, cy);
                } else {
                    acc.add(x, y);
                }
            }
        }
        if (more) {
#pragma unroll
            for (int q = 0; q < 8; ++q) put(cur ^ 1, 4 * q + lrow, lcol, next[q]);
            if constexpr (CODES) {
#pragma unroll
                for (int q = 0; q < 8; ++q) put_code(cur ^ 1, 4 * q + lrow, lcol, nextc[q]);
            }
        }
        __syncthreads();
        cur ^= 1;
    }
    acc.finish();
    // per-group reduction over its 16 lanes (fixed order), lane 0 of the group writes
#pragma unroll
    for (int n = 0; n < Acc::NACC; ++n)
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                Partial p = acc.partial(n, a, b);
#pragma unroll
                for (int d = 8; d >= 1; d >>= 1) {
                    p.s += __shfl_down(p.s, d, 16);
                    p.m += __shfl_down(p.m, d, 16);
                }
                if (mine && l == 0) partials[((uint64_t)n * o.slots + (uint64_t)tile * 16u + (uint64_t)(a * 4 + b)) * blk.ngroups + blk.group] = p;
            }
}


// The zero mask of a staged row from the loader's two ballots: bit c = bin 2c, bit 32 + c = bin 2c + 1 (the same permutation
// of the bins in every row).
__device__ __forceinline__ unsigned long long cross_zero_mask(const longlong2 &v, int lhalf)
{
    const unsigned long long z0 = __builtin_amdgcn_ballot_w64(v.x == 0), z1 = __builtin_amdgcn_ballot_w64(v.y == 0);
    return lhalf ? ((z0 >> 32) | (z1 & 0xFFFFFFFF00000000ull)) : ((z0 & 0xFFFFFFFFull) | (z1 << 32));
}

// The two reciprocal forms of the multiset metrics over staged super-tiles (cross_super_kernel's structure, cross_block's grid).
//
// FORM 0: the 'prod' pairwise function (the default of kpal distance / matrix; metrics.py:101-123, 159-162) as a difference
// of reciprocals:
//        |x - y| / ((x + 1)(y + 1))  =  |(x + 1) - (y + 1)| / ((x + 1)(y + 1))  =  | 1/(y + 1) - 1/(x + 1) |.
// With r = 1 / (count + 1) staged instead of the counts a term is ONE subtraction and ONE add of an absolute value -- two
// fp64 instructions (cross_super_kernel with PlainAcc<0>: three, plus the conversions; the plain division: ~12) -- and the
// number of terms (bins where x != 0 or y != 0) leaves the fp64 loop entirely: the loader's waves read 64 bins of one profile
// at a time, so ONE ballot gives that row's zero mask, and the bins where BOTH profiles are zero are popcount(mask_i & mask_j),
// two v_bcnt per pair and stage, accumulated by thread (i, j) of the 16 x 16 super-tile.
//   Accuracy: r is within 1 ulp of 1 / (x + 1) (rcp_counts), so a term's error is at most 2^-52 (r_x + r_y) against a term
// of at least r_x r_y (x != y: |x - y| >= 1): relative 2^-52 (x + y + 2) -- below 2.9e-11 while both counts are below 2^16
// (kRdiffMaxCount; at 2^20 the bound would be 4.7e-10, half the contract with nothing left for the accumulation),
// and every term being non-negative that bounds the relative error of the sum as well; the contract for fp64 results is
// 1e-9 (typical: 1e-15; the cancellation-dominated worst case -- all counts just below the limit, differing by 1 -- is
// tests/test_gpu_vec.py::test_matrix_rdiff_worst_case).  A count >= 2^16 (or negative) anywhere raises *big and the caller
// reruns the pair-of-counts kernel, cross_super_kernel.
//   Reciprocals of counts below 512 come from a table in LDS (one ds_read_b64 instead of v_rcp_f64 + four fused
// multiply-adds per staged value -- the loader would cost 60 % of the arithmetic otherwise); larger counts are computed.
//
// FORM 1: the 'sum' pairwise function, |x - y| / (x + y + 1): no difference form as for 'prod', but the denominator is a
// small integer -- its reciprocal comes from a table in LDS, R[s] = 1 / (s + 1) for s = x + y < kRsumTable, and a term is
// v_sad_u32 (|x - y|), v_add_lshl_u32 (the table offset), one ds_read_b64, a conversion and one fused multiply-add
// (cross_super_kernel with PlainAcc<1>: the two conversions, the sum and a ~10-instruction division).  Profiles of one sample
// have counts within a narrow range, so the 64 lanes of a table read touch a few dozen consecutive entries: few bank
// conflicts.  The staged values are the counts themselves as 32-bit integers (16 KiB instead of 32).
//   A count >= kRsumTable / 2 anywhere raises *big and the caller reruns cross_super_kernel (an inline second path for such
// stages cost the kernel its occupancy: 200 registers).
//   Accuracy: R within 1 ulp, |x - y| exact: a term within 1.5 ulp of the correctly rounded quotient the reference computes.
//
// Both: the same loader, zero masks and popcounts for the term counts, and partial layout.  The partials must be zeroed
// before the launch (.s and .m of a slot come from different threads).
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
    const CrossBlock blk = cross_block(c, nsuper, superR);
    const int g = threadIdx.x >> 4, l = threadIdx.x & 15;
    const CrossGroup grp = cross_group(c, blk, g);
    const bool mine = grp.mine;
    double s[TILE][TILE];
#pragma unroll
    for (int a = 0; a < TILE; ++a)
#pragma unroll
        for (int b = 0; b < TILE; ++b) s[a][b] = 0.0;
    uint32_t both_zero = 0;                            // pair (row threadIdx.x >> 4, column threadIdx.x & 15) of the super-tile
    bool saw_big = false;
    // loader: values 2 q', 2 q' + 1 of thread t are the bins 2 (t & 31), 2 (t & 31) + 1 of staged row 8 q' + (t >> 5): a wave reads
    // two 512-byte runs with 16-byte loads (as 8-byte loads the 43 GB of staged reads moved at 0.6 of the rate: MI355X_MICROARCH.md).
    // The row addresses of a wave's two halves are scalar; a lane selects its half's.
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
            // lane l takes the bin pairs (2l, 2l+1) and (32 + 2l, 32 + 2l + 1): 16-byte LDS reads (ds_read_b128 moves 256 B/clk per
            // CU; the ds_read2_b64 the 8-byte form compiled to, half of that -- and the LDS, not the fp64 pipe, set the pace)
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
                    // one pair (four terms) at a time: everything a term needs before its table read depends only on the staged counts,
                    // and with the offsets and differences of all 64 terms computed up front the kernel needed 190 registers (two
                    // waves per SIMD); the other three waves of the SIMD cover the latency of the four reads
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
    // the values of the next stage are requested before this stage's arithmetic and staged after it.  (Requesting TWO stages
    // ahead -- a stage's arithmetic takes ~0.3 us, a load 1-2 us -- needs 16 more registers than four waves per SIMD leave:
    // the compiler parked the prefetched values in scratch memory and the kernel was slower.  Round 4 tried the register-free
    // way to that depth: the raw counts by LDS-DMA (global_load_lds_dwordx4, inline assembly so that hipcc does not drain it
    // before every LDS read) into a three-slot ring, converted to reciprocals in place one iteration later, one raw s_barrier
    // per stage, 52 KiB of LDS = three workgroups per CU -- correct, and 8.4 ms against this kernel's 6.0: the DMA pieces cost
    // 100-185 cycles of issue each (MI355X_MICROARCH.md) -- four per wave and stage, as much as the stage's 136 fp64
    // instructions -- and the in-place pass adds a third to the LDS traffic, which already runs level with the fp64 pipe.)
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
                partials[((uint64_t)cross_tile_number(grp.ti, grp.tj, grp.sideR, c.tri != 0) * 16u + (uint64_t)(a * TILE + b)) * blk.ngroups + blk.group].s = ps;
        }
    // term counts: thread (i, j) of the super-tile writes .m = bins seen - bins where both are zero
    {
        const int i = blk.si * 16 + (int)(threadIdx.x >> 4), j = blk.sj * 16 + (int)(threadIdx.x & 15);
        const int sideQ = (c.Q + 3) / 4;
        if ((i >> 2) < sideQ && (j >> 2) < grp.sideR && (!c.tri || (j >> 2) <= (i >> 2)))
            partials[cross_slot(c, grp.sideR, i, j) * blk.ngroups + blk.group].m = stages * kSuperBins - both_zero;
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