// transform_set_kernels.hpp -- kernels that make new tables out of a whole SET of 4^k int64 count tables lying one behind the
// other (gfx950), planned by transform_plan.hpp:
//   balance of every table    Profile.balance            kpal/klib.py:285-298
//   pool (sum) of all tables  Profile.merge with sum     kpal/klib.py:269-283, folded over the set
// (The shrink of a set is the flat shrink of its entries: stat_kernels.hpp.)  All are HBM-bandwidth kernels; integer sums wrap.
// One unit includes this header (kpal_transform.hip).
#pragma once
#include "kpal_device.hpp"
#include "transform_plan.hpp"

namespace kpal {

// ---- balance, k <= 5 ------------------------------------------------------------------------------------------------------------
// One flat index over n_tables x 4^k bins: table = i >> 2k, bin = the low bits.  The owner of bin < rc(bin) reads both ends and
// writes both; bin == rc(bin) doubles (klib.py:290-298).  Every entry is written once, by the only thread that reads it: in ==
// out is as legal as two disjoint ranges.
static __global__ __launch_bounds__(256) void balance_set_kernel(const int64_t *in, int64_t *out, int k, uint64_t total)
{
    const uint64_t mask = (1ULL << (2 * k)) - 1ULL;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t bin = i & mask, r = revcomp(bin, k);
        if (bin < r) {
            const uint64_t j = i - bin + r;
            const uint64_t v = (uint64_t)in[i] + (uint64_t)in[j];
            out[i] = (int64_t)v;
            out[j] = (int64_t)v;
        } else if (bin == r) {
            out[i] = (int64_t)((uint64_t)in[i] * 2ULL);
        }
    }
}

// ---- balance, k >= 6 ------------------------------------------------------------------------------------------------------------
// balance_tiled_kernel (vec_kernels.hpp) with the work list widened from "canonical pair c" to "(table t, canonical pair c)":
// item = t * ncanon + c < items, taken round robin by persistent workgroups (grid: balance_set_workgroups), the next item's eight
// values per thread requested before the current pair is exchanged through LDS and written.  (t, c) are stepped, not divided:
// the grid is (dt, dc) items wide.  A workgroup owns the tile pair (M, rc(M)) of ITS table: it reads both 64 x 64 tiles as 64
// runs of 512 B, keeps them in LDS (rows padded to 65: the transposed read spreads over the banks) and writes out[i] = in[i] +
// in[rc(i)] for both.  in == out is allowed: all reads of an item precede its barrier, items are disjoint, and the item whose
// loads are in flight is another tile pair.  Within a table the pairs keep the page-aware order of canon_tiles (k >= 13).
static __global__ __launch_bounds__(kBalanceSetThreads) __attribute__((amdgpu_waves_per_eu(8))) void balance_tiled_set_kernel(
    const int64_t *in, int64_t *out, int k, const uint32_t *__restrict__ canon, uint32_t ncanon, uint64_t items)
{
    constexpr int T = 3, S = 64;
    __shared__ unsigned long long A[S][S + 1];
    __shared__ unsigned long long B[S][S + 1];
    const int md = k - 2 * T;
    const uint64_t rowstride = 1ULL << (2 * (k - T));
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rl = (int)revcomp((uint64_t)lane, T);
    const unsigned long long *uin = reinterpret_cast<const unsigned long long *>(in);
    unsigned long long *uout = reinterpret_cast<unsigned long long *>(out);
    auto fetch = [&](uint64_t t, uint64_t M, unsigned long long (&a)[4], unsigned long long (&b)[4]) {
        const uint64_t Mr = md > 0 ? revcomp(M, md) : 0;
        const unsigned long long *tab = uin + (t << (2 * k));
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint64_t row = (uint64_t)(w + 16 * q) * rowstride;
            a[q] = tab[row + M * S + lane];
            b[q] = tab[row + Mr * S + lane];
        }
    };
    // the step of one round, as (tables, pairs)
    const uint64_t dt = gridDim.x / ncanon;
    const uint32_t dc = gridDim.x % ncanon;
    uint64_t item = blockIdx.x, t = blockIdx.x / ncanon;
    uint32_t c = blockIdx.x % ncanon;
    unsigned long long a[4], b[4], na[4], nb[4];
    if (item < items) fetch(t, canon[c], a, b);
    while (item < items) {
        const uint64_t M = canon[c];
        const uint64_t itemn = item + gridDim.x;
        uint64_t tn = t + dt;
        uint32_t cn = c + dc;
        if (cn >= ncanon) {
            cn -= ncanon;
            ++tn;
        }
        if (itemn < items) fetch(tn, canon[cn], na, nb);
        const uint64_t Mr = md > 0 ? revcomp(M, md) : 0;
        const bool self = M == Mr;
        unsigned long long *tab = uout + (t << (2 * k));
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            A[w + 16 * q][lane] = a[q];
            B[w + 16 * q][lane] = b[q];   // self: B == A
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int rh = (int)revcomp((uint64_t)(w + 16 * q), T);
            const uint64_t row = (uint64_t)(w + 16 * q) * rowstride;
            tab[row + M * S + lane] = a[q] + B[rl][rh];
            if (!self) tab[row + Mr * S + lane] = b[q] + A[rl][rh];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            a[q] = na[q];
            b[q] = nb[q];
        }
        item = itemn;
        t = tn;
        c = cn;
    }
}

// ---- pool -----------------------------------------------------------------------------------------------------------------------
// out[j] (+)= the sum over the tables of slice blockIdx.y of tables[t][j], int64 wrap.  Thread (blockIdx.x, threadIdx.x) owns the
// column pair (2p, 2p + 1) and walks its slice kPoolUnroll tables at a time.  VEC: bins is even and both ranges are 16-byte
// aligned -- one 16-byte load per table; else two 8-byte ones, and the last pair of an odd row is a single column.  Row s of
// `out` (out + s * bins) takes slice s: with one slice that is the result itself (accumulate: onto what lies there), with more
// the rows are partials that a second launch of this kernel -- one slice over `slices` tables -- adds up.
template <bool VEC>
__global__ __launch_bounds__(kPoolThreads) void pool_set_kernel(const int64_t *__restrict__ tables, uint64_t n_tables, uint64_t bins, uint32_t slices,
                                                                int accumulate, int64_t *__restrict__ out)
{
    const uint64_t p = (uint64_t)blockIdx.x * kPoolThreads + threadIdx.x;
    if (p >= pool_column_pairs(bins)) return;
    const uint64_t j = 2 * p;
    const bool two = j + 1 < bins;
    const uint64_t t0 = pool_slice_begin(n_tables, slices, blockIdx.y), t1 = pool_slice_end(n_tables, slices, blockIdx.y);
    int64_t *row = out + (uint64_t)blockIdx.y * bins;
    uint64_t sx = 0, sy = 0;
    if (accumulate) {
        sx = (uint64_t)row[j];
        if (two) sy = (uint64_t)row[j + 1];
    }
    const int64_t *src = tables + t0 * bins + j;
    uint64_t t = t0;
    for (; t + kPoolUnroll <= t1; t += kPoolUnroll) {
        uint64_t x[kPoolUnroll], y[kPoolUnroll];
#pragma unroll
        for (int u = 0; u < kPoolUnroll; ++u) {
            if constexpr (VEC) {
                const longlong2 v = *reinterpret_cast<const longlong2 *>(src + (uint64_t)u * bins);
                x[u] = (uint64_t)v.x;
                y[u] = (uint64_t)v.y;
            } else {
                x[u] = (uint64_t)src[(uint64_t)u * bins];
                y[u] = two ? (uint64_t)src[(uint64_t)u * bins + 1] : 0ULL;
            }
        }
#pragma unroll
        for (int u = 0; u < kPoolUnroll; ++u) {
            sx += x[u];
            sy += y[u];
        }
        src += (uint64_t)kPoolUnroll * bins;
    }
    for (; t < t1; ++t) {
        if constexpr (VEC) {
            const longlong2 v = *reinterpret_cast<const longlong2 *>(src);
            sx += (uint64_t)v.x;
            sy += (uint64_t)v.y;
        } else {
            sx += (uint64_t)src[0];
            if (two) sy += (uint64_t)src[1];
        }
        src += bins;
    }
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

}  // namespace kpal
