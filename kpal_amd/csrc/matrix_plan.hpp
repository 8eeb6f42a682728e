// matrix_plan.hpp -- what the host decides about the distances of SETS of profiles before it launches anything, and the
// arithmetic it finishes them with: which kernel family a triangle or a rectangle takes, the grids, where the partial of a
// pair lies, the "too many for one call" limit, the distance of reduced partials.  No GPU in it: kpal_cross.hip, kpal_pair.hip,
// kpal_multi.hip, the kernels (the structs and the index functions) and a CPU program (tests/test_matrix_plan_host.py) read
// the same definitions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/kpal_hip.h"

#if defined(__HIPCC__)
#define KPAL_MATRIX_HD __host__ __device__ __forceinline__
#else
#define KPAL_MATRIX_HD inline
#endif

namespace kpal {

// Two sets of profiles whose pairs (left i, right j) are wanted (cross_kernels.hpp).  tri: a set against ITSELF -- left ==
// right, Q == R -- and only the pairs on or below the diagonal: the lower triangle of kdistlib.distance_matrix.
struct CrossSets {
    const int64_t *left;    // Q x n
    const int64_t *right;   // R x n
    int Q, R;
    uint64_t n;
    int tri;
};

struct Partial {
    double s;            // sum of pairwise terms
    unsigned long long m;  // multiset: bins with l!=0 or r!=0; euclidean: wrapping int64 dot
};

constexpr int kSuperBins = 64;      // bins per stage of a staged super-tile (cross_super_kernel, cross_recip_kernel)
constexpr int kGramBins = 64;       // bins per slab of the Gram kernels (gram_kernels.hpp, cross_gram_kernel)

// ---- which kernels --------------------------------------------------------------------------------------------------------
// (whole profiles: k >= 6) the LDS-staged kernels of a triangle take 64 bins at a time
inline bool matrix_tiled(uint64_t n) { return n >= 4096 && n % 64 == 0; }

// The LDS-staged kernels of a rectangle take 64 bins at a time (k >= 6) and pay when both sides fill more than one register
// tile; with at most four profiles on a side the register-tile kernel already reads the long side once.
inline bool cross_staged(int Q, int R, uint64_t n) { return n >= 4096 && Q > 4 && R > 4; }

// Options that ask for nothing but a plain metric (and perhaps the balance): the plain entries serve them.
inline bool options_plain(const kpal_distance_options *opt)
{
    return !opt->do_positive && !opt->do_smooth && !opt->do_scale && opt->metric <= KPAL_EUCLIDEAN;
}

// KPAL_MATRIX_MFMA / _SUPER / _ALL / _RDIFF (each on unless set to 0; A/B timing, cross-checks): 0 forces the int64 kernels
// instead of the Gram form, the register tiles instead of the staged ones, the super-tile kernels instead of the *_all ones,
// the pair-of-counts kernel instead of the reciprocal forms.
struct MatrixSwitches {
    bool mfma, super_, all, rdiff;
};

// The way of a triangle of P profiles of n bins, in the order distance_matrix_core goes through it.  tiled_agreed: 0 when the
// ranks of a bin-range matrix agreed NOT to take the staged kernels (kpal_comm_distance_matrix_device); anything else: by n.
struct MatrixRoute {
    bool gram;       // euclidean with enough profiles and bins: the fp64 Gram matrix first (exact while every |x|^2 < 2^53)
    bool all;        // multiset of 17..64 profiles: every profile staged once per bin range (matrix_all_kernels.hpp) ...
    bool all_wide;   // ... in its form for P > 32
    bool staged;     // else cross_pairs: LDS-staged 16 x 16 super-tiles (or 4 x 4 register tiles)
    bool recip;      // ... 'prod' / 'sum' in their reciprocal forms before the pair-of-counts kernel
};
inline MatrixRoute matrix_route(int P, uint64_t n, int metric, int tiled_agreed, const MatrixSwitches &sw)
{
    const bool tiled = matrix_tiled(n) && tiled_agreed != 0;
    MatrixRoute r = {};
    r.gram = metric == KPAL_EUCLIDEAN && sw.mfma && P > 8 && tiled;
    r.staged = sw.super_ && P > 8 && tiled;
    r.all = r.staged && sw.all && sw.rdiff && metric <= KPAL_PAIRWISE_SUM && P > 16 && P <= 64;
    r.all_wide = r.all && P > 32;
    r.recip = r.staged && sw.rdiff && metric != KPAL_EUCLIDEAN;
    return r;
}

// ---- grids ----------------------------------------------------------------------------------------------------------------
// Partials are indexed with 32 bits: `groups` reduced values of gx workgroup partials each are too many for one call.
inline bool partials_too_many(uint64_t groups, uint32_t gx) { return groups > 0x7fffffffu / gx; }

// Tiles, slots and the grid of one pass of cross_tile_kernel / cross_super_kernel (or cross_recip_kernel) over c.
struct CrossGrid {
    int sideR, superR;
    uint32_t units;   // what the grid counts: super-tiles (staged) or 4 x 4 tiles
    uint32_t gx;      // workgroups per unit = partials per slot
    uint64_t slots;   // 16 * tiles
};
inline CrossGrid cross_grid(int num_cu, const CrossSets &c, bool staged)
{
    const int sideQ = (c.Q + 3) / 4, sideR = (c.R + 3) / 4, superQ = (c.Q + 15) / 16, superR = (c.R + 15) / 16;
    const uint64_t ntiles = c.tri ? (uint64_t)sideQ * (sideQ + 1) / 2 : (uint64_t)sideQ * sideR;
    const uint64_t nsuper = c.tri ? (uint64_t)superQ * (superQ + 1) / 2 : (uint64_t)superQ * superR;
    uint32_t gx;
    if (staged) {
        gx = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(c.n / kSuperBins, std::max<uint64_t>(1, (uint64_t)num_cu * 8 / nsuper)));
        gx = std::max(8u, gx / 8u * 8u);   // (cross_block deals bin-groups to the 8 XCDs; n / 64 >= 64 for k >= 6)
    } else {
        gx = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((c.n + 255) / 256, std::max<uint64_t>(1, (uint64_t)num_cu * 16 / ntiles)));
    }
    return CrossGrid{sideR, superR, (uint32_t)(staged ? nsuper : ntiles), gx, ntiles * 16};
}

// The Gram matrix of a triangle (gram_mfma_kernel): the blocks (I, J), J <= I, of 64 x 64 profiles -- the diagonal ones in
// order of I, then the others in order of (I, J) -- and the workgroups per block: diagonal blocks two 68 KiB workgroups per
// CU; off-diagonal ones (P > 64) one.
struct GramBlock {
    int I, J;
};
struct GramPlan {
    std::vector<GramBlock> blocks;
    uint32_t nd, no;       // diagonal, off-diagonal blocks
    unsigned gx_d, gx_o;
};
inline GramPlan gram_plan(int num_cu, int P, uint64_t n)
{
    const int nb = (P + 63) / 64;
    GramPlan g = {};
    for (int I = 0; I < nb; ++I) g.blocks.push_back(GramBlock{I, I});
    for (int I = 0; I < nb; ++I)
        for (int J = 0; J < I; ++J) g.blocks.push_back(GramBlock{I, J});
    g.nd = (uint32_t)nb;
    g.no = (uint32_t)g.blocks.size() - g.nd;
    const uint64_t slabs = n / kGramBins;
    g.gx_d = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(slabs, (uint64_t)num_cu * 2 / g.nd));
    g.gx_o = g.no ? (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(slabs, (uint64_t)num_cu / g.no)) : 0u;
    return g;
}
// ... of a rectangle (cross_gram_kernel): one 132 KiB workgroup per CU over the nblocks blocks of 64 x 64 profiles
inline uint32_t cross_gram_gx(int num_cu, uint32_t nblocks, uint64_t n)
{
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n / kGramBins, (uint64_t)num_cu / nblocks));
}

// Workgroups of a *_all kernel: four 256-thread ones per CU, or one of its wide (P > 32) form.
inline unsigned matrix_all_gx(int num_cu, uint64_t n, bool wide)
{
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(n / 128, (uint64_t)num_cu * (wide ? 1 : 4)));
}

// Workgroups per profile of the totals pass of a scaled option set (cross_option_totals_kernel).
inline uint32_t option_totals_gx(int num_cu, uint32_t nprof, uint64_t n)
{
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, std::max<uint64_t>(1, (uint64_t)num_cu * 8 / nprof)));
}

// (s, m) accumulators per pair of an option set: of its metric, and of the widest of its passes (the masked totals take two).
inline uint32_t option_nacc(int metric) { return metric == KPAL_COSINE ? 3 : 1; }
inline uint32_t option_nacc_max(int metric, bool scaled, bool positive) { return std::max(option_nacc(metric), scaled && positive ? 2u : 1u); }

// ---- where a pair lies ----------------------------------------------------------------------------------------------------
// Tile (ti, tj) of 4 x 4 pairs (or super-tile of 16 x 16): row-major over `side` columns, or the lower triangle's ti (ti + 1) / 2 + tj.
KPAL_MATRIX_HD uint32_t cross_tile_number(int ti, int tj, int side, bool tri)
{
    return tri ? (uint32_t)ti * ((uint32_t)ti + 1u) / 2u + (uint32_t)tj : (uint32_t)ti * (uint32_t)side + (uint32_t)tj;
}

// Slot of pair (i, j) among the 16 * tiles of one accumulator.
KPAL_MATRIX_HD uint64_t cross_slot(const CrossSets &c, int sideR, int i, int j)
{
    return (uint64_t)cross_tile_number(i >> 2, j >> 2, sideR, c.tri != 0) * 16u + (uint64_t)((i & 3) * 4 + (j & 3));
}

// Pair (i, j), j < i, in the lower triangle of kdistlib.distance_matrix.
inline size_t triangle_index(int i, int j) { return (size_t)i * (i - 1) / 2 + j; }

// Dot product of profiles i and j in the reduced result of the Gram kernels: block `blk` of 64 x 64 profiles holds 16 tiles of
// 16 x 16.  Triangle (i >= j): GramPlan's order; rectangle: the blocks row-major over blocksR.
KPAL_MATRIX_HD size_t gram_entry(size_t blk, int i, int j)
{
    return (blk * 16 + (size_t)((i % 64) / 16 * 4 + (j % 64) / 16)) * 256 + (size_t)((i % 16) * 16 + (j % 16));
}
inline size_t gram_index(const GramPlan &g, int i, int j)
{
    const int I = i / 64, J = j / 64;
    return gram_entry(I == J ? (size_t)I : g.nd + (size_t)I * (I - 1) / 2 + J, i, j);
}
KPAL_MATRIX_HD size_t cross_gram_index(int blocksR, int q, int r) { return gram_entry((size_t)(q / 64) * blocksR + (size_t)(r / 64), q, r); }

// ---- finishing ------------------------------------------------------------------------------------------------------------
// (host and device: the build keeps -ffp-contract=off, and the fp64 divide and square root are correctly rounded on both, so a
// kernel that finishes a pair -- nearest_kernels.hpp -- gives the bits of the host loops)
// The distance from the reduced accumulators of a pair: p0 alone, but for the cosine similarity (p0 the dot, p1 / p2 the
// squared norms).  scaled: the sums were formed in fp64 (.s); else the euclidean and cosine ones are wrapping int64 (.m).
KPAL_MATRIX_HD double finish_distance(int metric, bool scaled, const Partial &p0, const Partial &p1, const Partial &p2)
{
    if (metric <= KPAL_PAIRWISE_SUM) return p0.s / (double)(p0.m + 1ULL);   // metrics.py:123
    if (metric == KPAL_EUCLIDEAN) return scaled ? std::sqrt(p0.s) : std::sqrt((double)(int64_t)p0.m);   // metrics.py:135,46
    // metrics.py:147: dot(l, r) / (|l| * |r|)
    if (scaled) return p0.s / (std::sqrt(p1.s) * std::sqrt(p2.s));
    return (double)(int64_t)p0.m / (std::sqrt((double)(int64_t)p1.m) * std::sqrt((double)(int64_t)p2.m));
}

// Euclidean from the fp64 Gram matrix, valid while every |x|^2 < 2^53 (gram_kernels.hpp): *exact says whether these two are.
KPAL_MATRIX_HD bool gram_exact(double norm) { return norm < 9007199254740992.0; }   // 2^53
KPAL_MATRIX_HD double gram_distance(double norm_i, double norm_j, double dot, bool *exact)
{
    *exact = gram_exact(norm_i) && gram_exact(norm_j);
    if (!*exact) return 0.0;
    // exact integers below 2^53 each: the int64 expression is the reference's sum of squared differences
    const int64_t d2 = (int64_t)norm_i + (int64_t)norm_j - 2 * (int64_t)dot;
    return std::sqrt((double)d2);   // metrics.py:46: np.sqrt(np.dot(v, v))
}

// The factors that scale two profiles of totals tl and tr to each other: metrics.get_scale, metrics.py:49-72 (int64 totals,
// true division), and with `down` metrics.scale_down, metrics.py:75-86.
inline void scale_factors(int64_t tl, int64_t tr, bool down, double *ls, double *rs)
{
    *ls = *rs = 1.0;
    if (tl < tr) *ls = (double)tr / (double)tl;
    else *rs = (double)tl / (double)tr;
    if (down) {
        // Python's max(left, right) keeps `left` unless right > left; this keeps `rs` unless ls > rs.  The operand kept
        // differs only when a factor is NaN (totals 0 == 0), and then every metric is NaN whichever it is: the G13 cases
        // totals_k1_vboth_zero, totals_k2_vboth_zero and totals_k4_vboth_zero (tests/golden/option_edges.json) pin NaN
        // with and without `down`.
        const double top = *ls > *rs ? *ls : *rs;
        *ls /= top;
        *rs /= top;
    }
}

}  // namespace kpal
