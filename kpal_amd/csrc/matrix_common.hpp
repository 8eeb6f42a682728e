// matrix_common.hpp -- what the tiled distance kernels share (gfx950): the pairwise terms, the (sum, count) partial and its
// fixed-order block reduction, the short divisions, the 4 x 4 register-tile accumulation with its byte-counter term
// counts, and the geometry / table constants of the LDS-staged forms.  Used by vec_kernels.hpp (pair kernels),
// matrix_all_kernels.hpp (every profile staged once), cross_kernels.hpp (tiles and super-tiles of a rectangle or a
// triangle) and gram_kernels.hpp.  No kernel lives here.
#pragma once
#include "kpal_device.hpp"
#include "matrix_plan.hpp"   // CrossSets, Partial, the index functions the host shares, kSuperBins

namespace kpal {

// ---- pairwise functions, kpal/metrics.py:159-162, int64 wrap-around like NumPy -------------
__device__ __forceinline__ int64_t wrap_abs_diff(int64_t x, int64_t y)
{
    const uint64_t d = (uint64_t)x - (uint64_t)y;
    return (int64_t)d < 0 ? (int64_t)(0ULL - d) : (int64_t)d;
}
__device__ __forceinline__ double pw_prod(int64_t x, int64_t y)
{
    const int64_t den = (int64_t)(((uint64_t)x + 1ULL) * ((uint64_t)y + 1ULL));
    return (double)wrap_abs_diff(x, y) / (double)den;
}
__device__ __forceinline__ double pw_sum(int64_t x, int64_t y)
{
    const int64_t den = (int64_t)((uint64_t)x + (uint64_t)y + 1ULL);
    return (double)wrap_abs_diff(x, y) / (double)den;
}
__device__ __forceinline__ double pw_prod(double x, double y) { return fabs(x - y) / ((x + 1.0) * (y + 1.0)); }
__device__ __forceinline__ double pw_sum(double x, double y) { return fabs(x - y) / (x + y + 1.0); }

__device__ __forceinline__ Partial block_reduce(Partial p)
{
    __shared__ double sh_s[16];
    __shared__ unsigned long long sh_m[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        p.s += __shfl_down(p.s, d);
        p.m += __shfl_down(p.m, d);
    }
    __syncthreads();
    if (lane == 0) {
        sh_s[wave] = p.s;
        sh_m[wave] = p.m;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nw = (blockDim.x + 63) >> 6;
        for (int w = 1; w < nw; ++w) {
            p.s += sh_s[w];
            p.m += sh_m[w];
        }
    }
    return p;  // valid in thread 0
}

// num / den for den in [1, 2^63) and num >= 0 (the float path of the matrix kernel: counts < 2^31, so no
// zero, infinite, NaN or denormal operands and no scaling): v_rcp_f64, one Newton step on the reciprocal,
// the product, and one residual correction of the quotient -- the correction multiplies the error of the
// quotient by the error of the reciprocal, so the result is within 1 ulp of the correctly rounded quotient
// whenever v_rcp_f64 is good to 14 bits.  6 full-rate instructions instead of the ~13 of the IEEE
// division sequence (v_div_scale x2, two Newton steps, v_div_fmas, v_div_fixup), 29.0 -> 21.4 ms for the
// 64-profile k=12 matrix with register tiles.  The parity contract for fp64 results is 1e-9 relative.
// KPAL_MATRIX_DIV: 0 = IEEE division, 1 = two Newton steps without the correction, 2 = two steps with it.
#ifndef KPAL_MATRIX_DIV
#define KPAL_MATRIX_DIV 3
#endif
__device__ __forceinline__ double div_counts(double num, double den)
{
#if KPAL_MATRIX_DIV == 0
    return num / den;
#else
    double r = __builtin_amdgcn_rcp(den);   // (an fp32 v_rcp_f32 seed is as exact and not faster: the reciprocal is not the limit)
    r = __builtin_fma(__builtin_fma(-den, r, 1.0), r, r);
#if KPAL_MATRIX_DIV != 3
    r = __builtin_fma(__builtin_fma(-den, r, 1.0), r, r);
#endif
    const double q = num * r;
#if KPAL_MATRIX_DIV == 1
    return q;
#else
    return __builtin_fma(__builtin_fma(-den, q, num), r, q);
#endif
#endif
}

// 1 / d for d in [1, 2^32]: v_rcp_f64 and two Newton steps (within 1 ulp; no zero, infinite, NaN or denormal operand)
__device__ __forceinline__ double rcp_counts(double d)
{
    double r = __builtin_amdgcn_rcp(d);
    r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
    return __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
}

// ---- TILE x TILE register tiles -----------------------------------------------------------------
// A thread takes one bin at a time of TILE row profiles and TILE column profiles and accumulates TILE^2 (sum, m) pairs
// in registers (cross_tile_kernel: from global memory; cross_super_kernel: from LDS).
// The TILE x TILE terms of one bin: row values x[], column values y[]; s = fp64 sums, mf = number of
// multiset terms, m = exact int64 dots (euclidean).
// Term counts of the float path: per row a one word of four byte counters (column b in byte b) of the bins in
// which x[a] or y[b] is non-zero -- 19 instead of 48 instructions per bin for the 16 counts; the bytes are
// added to the 32-bit totals every 255 bins.
template <int TILE>
struct TermBytes {
    uint32_t packed[TILE];
    uint32_t bins;
};

template <int TILE>
__device__ __forceinline__ void term_bytes_flush(TermBytes<TILE> &tb, uint32_t (&mf)[TILE][TILE])
{
    static_assert(TILE == 4, "four byte counters per word");
#pragma unroll
    for (int a = 0; a < TILE; ++a) {
#pragma unroll
        for (int b = 0; b < TILE; ++b) mf[a][b] += (tb.packed[a] >> (8 * b)) & 255u;
        tb.packed[a] = 0u;
    }
    tb.bins = 0u;
}

template <int METRIC, int TILE>
__device__ __forceinline__ void matrix_accumulate(const int64_t (&x)[TILE], const int64_t (&y)[TILE], double (&s)[TILE][TILE],
                                                  unsigned long long (&m)[TILE][TILE], uint32_t (&mf)[TILE][TILE],
                                                  TermBytes<TILE> &tb)
{
    if constexpr (METRIC != 2) {
        // Counts below 2^31 (any real profile): |x-y|, (x+1)(y+1) and x+y+1 are exact in float64 or
        // round exactly like the int64 value NumPy converts, so the terms are bit-identical to the
        // int64 formulation -- with 8 cheap 32-bit conversions per bin instead of 32 64-bit ones.
        uint64_t any = 0;
#pragma unroll
        for (int a = 0; a < TILE; ++a) any |= (uint64_t)x[a] | (uint64_t)y[a];
        if (__all((any >> 31) == 0)) {   // wave-uniform
            double xd[TILE], yd[TILE];
#pragma unroll
            for (int a = 0; a < TILE; ++a) {
                xd[a] = (double)(uint32_t)x[a];
                yd[a] = (double)(uint32_t)y[a];
            }
            // branch-free: a pair of zeros contributes |0 - 0| / 1 = +0.0 to the sum and nothing to the count, so
            // the 16 division chains of a bin are independent straight-line code that the scheduler interleaves
#pragma unroll
            for (int a = 0; a < TILE; ++a)
#pragma unroll
                for (int b = 0; b < TILE; ++b) {
                    const double num = fabs(xd[a] - yd[b]);
                    const double den = METRIC == 0 ? (xd[a] + 1.0) * (yd[b] + 1.0) : xd[a] + yd[b] + 1.0;
                    s[a][b] += div_counts(num, den);
                }
            uint32_t ynz = 0u;   // byte b = 1 iff y[b] != 0
#pragma unroll
            for (int b = 0; b < TILE; ++b) ynz |= min((uint32_t)y[b], 1u) << (8 * b);
#pragma unroll
            for (int a = 0; a < TILE; ++a) tb.packed[a] += (uint32_t)x[a] != 0u ? 0x01010101u : ynz;
            if (++tb.bins == 255u) term_bytes_flush(tb, mf);   // wave-uniform
            return;
        }
    }
#pragma unroll
    for (int a = 0; a < TILE; ++a)
#pragma unroll
        for (int b = 0; b < TILE; ++b) {
            if constexpr (METRIC == 2) {
                const uint64_t d = (uint64_t)x[a] - (uint64_t)y[b];
                m[a][b] += d * d;
            } else {
                if (x[a] != 0 || y[b] != 0) {
                    s[a][b] += METRIC == 0 ? pw_prod(x[a], y[b]) : pw_sum(x[a], y[b]);
                    mf[a][b] += 1u;
                }
            }
        }
}

// Multiset 'prod' terms with the reciprocals 1 / (x + 1) of the staged values precomputed ONCE per value by the
// loader of cross_super_kernel instead of one division per pair: |x - y| / ((x + 1)(y + 1)) = |x - y| * rx * ry --
// a subtraction, a multiplication and a fused multiply-add per term (3 fp64 issue slots instead of ~12).  Each
// factor is within 1 ulp, so a term is within ~2 ulp of the reference's quotient and the sum of the non-negative
// terms within ~5e-16 relative -- the contract for fp64 results is 1e-9 (metrics.py:101-123).  Counts >= 2^31
// anywhere in the wave's values take the int64 formulation (matrix_accumulate), like before.
template <int TILE>
__device__ __forceinline__ void matrix_accumulate_prod_rcp(const int64_t (&x)[TILE], const int64_t (&y)[TILE],
                                                           const double (&rx)[TILE], const double (&ry)[TILE],
                                                           double (&s)[TILE][TILE], unsigned long long (&m)[TILE][TILE],
                                                           uint32_t (&mf)[TILE][TILE], TermBytes<TILE> &tb)
{
    uint64_t any = 0;
#pragma unroll
    for (int a = 0; a < TILE; ++a) any |= (uint64_t)x[a] | (uint64_t)y[a];
    if (!__all((any >> 31) == 0)) {   // wave-uniform
        matrix_accumulate<0, TILE>(x, y, s, m, mf, tb);
        return;
    }
    double xd[TILE], yd[TILE];
#pragma unroll
    for (int a = 0; a < TILE; ++a) {
        xd[a] = (double)(uint32_t)x[a];
        yd[a] = (double)(uint32_t)y[a];
    }
#pragma unroll
    for (int a = 0; a < TILE; ++a)
#pragma unroll
        for (int b = 0; b < TILE; ++b) s[a][b] = __builtin_fma(fabs(xd[a] - yd[b]) * rx[a], ry[b], s[a][b]);
    uint32_t ynz = 0u;   // byte b = 1 iff y[b] != 0
#pragma unroll
    for (int b = 0; b < TILE; ++b) ynz |= min((uint32_t)y[b], 1u) << (8 * b);
#pragma unroll
    for (int a = 0; a < TILE; ++a) tb.packed[a] += (uint32_t)x[a] != 0u ? 0x01010101u : ynz;
    if (++tb.bins == 255u) term_bytes_flush(tb, mf);   // wave-uniform
}

// Geometry of a staged super-tile (cross_super_kernel, cross_recip_kernel): kSuperBins = 64 bins per stage, rows padded to 68 bins.
constexpr int kSuperRow = 68;

// Wave priority by progress (quad_kernels.hpp: quad_tile_priority): the workgroups of the staged matrix kernels run a few thousand
// stages each, four to a CU, and the arbiter's oldest-first order let them finish one after the other -- the last one of a CU
// alone.  A workgroup's priority falls with the share of its stages it has done.
__device__ __forceinline__ void matrix_stage_priority(uint64_t done, uint64_t total)
{
#if !defined(KPAL_MATRIX_NO_PRIO)   // A/B builds
    switch ((uint32_t)(done * 4u / total)) {     // (block-uniform scalars)
    case 0: __builtin_amdgcn_s_setprio(3); break;
    case 1: __builtin_amdgcn_s_setprio(2); break;
    case 2: __builtin_amdgcn_s_setprio(1); break;
    default: __builtin_amdgcn_s_setprio(0); break;
    }
#endif
}

// Limits and tables of the reciprocal forms (cross_recip_kernel argues them; matrix_all_kernels.hpp shares them).
constexpr unsigned long long kRdiffMaxCount = 1ull << 16;   // counts the difference form is accurate for (cross_recip_kernel)
constexpr int kRdiffTable = 512;    // reciprocals 1 / (c + 1) of counts c < 512 (4 KiB: four workgroups per CU)
constexpr int kRdiffRow = 64;       // staged row: 64 bins, unpadded -- with 16-byte reads a 16-lane group covers all 64 banks, and
                                    // rows a multiple of 8 doubles apart keep the lanes of two groups that share a read pass apart
constexpr int kRsumTable = 2048;   // reciprocals 1 / (s + 1) of the sums s = x + y < 2048 ('sum': both counts below 1024)

}  // namespace kpal
