// pool_groups_kernels.hpp -- the pool (sum) of the tables of a set BY LABEL (gfx950), planned by pool_groups_plan.hpp: for every
// group the sum of its member tables, read where they lie through the inverted index the host uploads.  An HBM-bandwidth
// kernel; integer sums wrap.  One unit includes this header (kpal_pool_groups.hip).
#pragma once
#include "kpal_device.hpp"
#include "pool_groups_plan.hpp"

namespace kpal {

// U rows of one item in flight: sx, sy += the column pair at `col` of the rows members[i] .. members[i + U - 1] (LISTED; else of
// the rows i .. i + U - 1).  The indices are fetched before the first row is asked for, so that one wait covers them.
template <bool VEC, bool LISTED, int U>
__device__ __forceinline__ void pool_groups_step(const int64_t *__restrict__ col, uint64_t bins, const uint32_t *__restrict__ members, uint32_t i, bool two,
                                                 uint64_t &sx, uint64_t &sy)
{
    uint64_t x[U], y[U], t[U];
#pragma unroll
    for (int u = 0; u < U; ++u) t[u] = LISTED ? members[i + u] : i + u;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int64_t *src = col + t[u] * bins;
        if constexpr (VEC) {
            const longlong2 v = *reinterpret_cast<const longlong2 *>(src);
            x[u] = (uint64_t)v.x;
            y[u] = (uint64_t)v.y;
        } else {
            x[u] = (uint64_t)src[0];
            y[u] = two ? (uint64_t)src[1] : 0ULL;
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        sx += x[u];
        sy += y[u];
    }
}

// pool_set_kernel (transform_set_kernels.hpp) with the slice of consecutive tables widened to an ITEM: the members
// members[begin[item]] .. members[begin[item + 1] - 1] of the table list (LISTED; else the rows begin[item] .. begin[item + 1] - 1
// themselves -- the partial rows of a group in the second pass).  row `item` of `out` (+)= their sum.  An item
// takes 2^lane_shift threads, one 16-byte column pair each, and walks its list kPoolUnroll tables at a time; a workgroup takes
// kPoolThreads >> lane_shift items (one unless a table has fewer than kPoolThreads column pairs), blockIdx.y strides over the
// workgroups of items.  VEC: bins is even and both ranges are 16-byte aligned -- one 16-byte load per table; else two 8-byte
// ones, and the last pair of an odd row is a single column.  WAVE: an item has 64 threads at least, so the item -- and with it
// the bounds of its list and every member index -- is the same for a whole wave: it is taken through readfirstlane, the index
// costs scalar loads and scalar address arithmetic.  The second pass (not LISTED) has as many workgroups with work as there are
// cut groups, and a long group's partial rows are one chain of dependent steps: it keeps kPoolGroupsFinalUnroll rows in flight
// while that many are left (measured: 228 rows of k = 6 took 27 us four at a time).  An item with an empty list writes zeros, or
// with `accumulate` nothing.
template <bool VEC, bool WAVE, bool LISTED>
__global__ __launch_bounds__(kPoolThreads) void pool_groups_kernel(const int64_t *__restrict__ tables, uint64_t bins, const uint32_t *__restrict__ members,
                                                                   const uint32_t *__restrict__ begin, uint32_t n_items, int lane_shift, int accumulate,
                                                                   int64_t *__restrict__ out)
{
    const uint32_t lanes = 1u << lane_shift, per = (uint32_t)kPoolThreads >> lane_shift;
    const uint64_t p = ((uint64_t)blockIdx.x << lane_shift) + (threadIdx.x & (lanes - 1));
    if (p >= pool_column_pairs(bins)) return;
    const uint64_t j = 2 * p;
    const bool two = j + 1 < bins;
    const uint32_t item_workgroups = n_items / per + (n_items % per != 0 ? 1 : 0);
    for (uint32_t w = blockIdx.y; w < item_workgroups; w += gridDim.y) {
        uint32_t item = w * per + (threadIdx.x >> lane_shift);
        if constexpr (WAVE) item = (uint32_t)__builtin_amdgcn_readfirstlane((int)item);
        if (item >= n_items) continue;
        const uint32_t b = begin[item], e = begin[item + 1];
        if (b == e && accumulate) continue;
        int64_t *row = out + (uint64_t)item * bins;
        uint64_t sx = 0, sy = 0;
        if (accumulate) {
            sx = (uint64_t)row[j];
            if (two) sy = (uint64_t)row[j + 1];
        }
        const int64_t *col = tables + j;
        uint32_t i = b;
        if constexpr (!LISTED)
            for (; i + kPoolGroupsFinalUnroll <= e; i += kPoolGroupsFinalUnroll) pool_groups_step<VEC, LISTED, kPoolGroupsFinalUnroll>(col, bins, members, i, two, sx, sy);
        for (; i + kPoolUnroll <= e; i += kPoolUnroll) pool_groups_step<VEC, LISTED, kPoolUnroll>(col, bins, members, i, two, sx, sy);
        for (; i < e; ++i) pool_groups_step<VEC, LISTED, 1>(col, bins, members, i, two, sx, sy);
        if constexpr (VEC) {
            longlong2 v;
            v.x = (long long)sx;
            v.y = (long long)sy;
            *reinterpret_cast<longlong2 *>(row + j) = v;
        } else {
            row[j] = (int64_t)sx;
            if (two) row[j + 1] = (int64_t)sy;
        }
    }
}

}  // namespace kpal
