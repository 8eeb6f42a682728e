// nearest_kernels.hpp -- the nearest n right profiles of every left profile of a tile (kpal_cross_nearest[_device],
// kpal_nearest.hip; tiles and the order: nearest_plan.hpp).  Two steps behind the rectangle kernels and their reduction:
//   finish   the reduced partials of a tile -> its Qt x Rt distances, row-major, with matrix_plan.hpp's finish_distance /
//            gram_distance -- the definitions the host loops of kpal_cross.hip use; fp64 divide and square root are correctly
//            rounded here and there and nothing is contracted, so the doubles are the same
//   select   one workgroup per left profile merges the row's Rt distances into the n best it has so far
// Both are a fixed number of launches whatever Qt and Rt are.
#pragma once
#include "kpal_device.hpp"
#include "nearest_plan.hpp"

namespace kpal {

constexpr int kNearestThreads = 256;
constexpr int kNearestPer = 8;   // candidates a thread holds in registers per chunk of a row
static_assert(KPAL_NEAREST_MAX <= kNearestThreads && KPAL_NEAREST_MAX <= 64, "one thread per kept candidate; one wave reads the old list");

// The slot layouts of cross_pairs (nacc = 1, unscaled) and of cross_option_launch: accumulator a of pair (q, r) at
// a * slots + cross_slot(c, sideR, q, r).
__global__ __launch_bounds__(256) void nearest_finish_slots_kernel(const Partial *__restrict__ res, CrossSets c, int sideR, uint64_t slots,
                                                                   uint32_t nacc, int metric, int scaled, double *__restrict__ out)
{
    const uint64_t pairs = (uint64_t)c.Q * (uint64_t)c.R;
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < pairs; p += (uint64_t)gridDim.x * 256) {
        const int q = (int)(p / (uint64_t)c.R), r = (int)(p % (uint64_t)c.R);
        const uint64_t slot = cross_slot(c, sideR, q, r);
        out[p] = finish_distance(metric, scaled != 0, res[slot], res[(uint64_t)(nacc / 2) * slots + slot], res[(uint64_t)(nacc - 1) * slots + slot]);
    }
}

// The Gram layout: the dot of (q, r) at cross_gram_index, the Q + R norms from `dots` on.  *inexact is set (it was cleared
// before) when a norm is not below 2^53: the host then takes the int64 kernels for this tile, as cross_core does.
__global__ __launch_bounds__(256) void nearest_finish_gram_kernel(const Partial *__restrict__ res, int Q, int R, int blocksR, uint64_t dots,
                                                                  double *__restrict__ out, uint32_t *__restrict__ inexact)
{
    const uint64_t pairs = (uint64_t)Q * (uint64_t)R;
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x; p < pairs; p += (uint64_t)gridDim.x * 256) {
        const int q = (int)(p / (uint64_t)R), r = (int)(p % (uint64_t)R);
        bool exact;
        out[p] = gram_distance(res[dots + (uint64_t)q].s, res[dots + (uint64_t)Q + (uint64_t)r].s, res[cross_gram_index(blocksR, q, r)].s, &exact);
        if (!exact) *inexact = 1u;
    }
}

// Row blockIdx.x of a tile: dist[row * Rt + r] is the distance to right profile first + r.  best_d / best_i (n per row) hold
// `have` candidates in order and hold min(n, have + Rt) afterwards, NaN / -1 behind them.  The row is walked in chunks of
// 256 * kNearestPer candidates that stay in registers; per chunk, round j takes the first candidate BEHIND the one round
// j - 1 took (nearest_before; the keys of a row are distinct, their indices are) among the chunk and the old list: a minimum
// per thread, per wave by shuffles, over the four waves through LDS -- one barrier per round.
__global__ __launch_bounds__(kNearestThreads) void nearest_select_kernel(const double *__restrict__ dist, uint32_t Rt, int64_t first, int n, int have,
                                                                         double *__restrict__ best_d, int64_t *__restrict__ best_i)
{
    __shared__ double list_d[2][KPAL_NEAREST_MAX];
    __shared__ int64_t list_i[2][KPAL_NEAREST_MAX];
    __shared__ double wave_d[2][kNearestThreads / 64];
    __shared__ int64_t wave_i[2][kNearestThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t row = blockIdx.x;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (tid < have) {
        list_d[0][tid] = best_d[row * (uint64_t)n + tid];
        list_i[0][tid] = best_i[row * (uint64_t)n + tid];
    }
    __syncthreads();
    const double *drow = dist + row * (uint64_t)Rt;
    int cur = 0, count = have;
    for (uint32_t c0 = 0; c0 < Rt; c0 += kNearestThreads * kNearestPer) {
        NearestCand mine[kNearestPer];
#pragma unroll
        for (int i = 0; i < kNearestPer; ++i) {
            const uint32_t r = c0 + (uint32_t)(i * kNearestThreads + tid);
            mine[i] = r < Rt ? NearestCand{drow[r], first + (int64_t)r} : NearestCand{nan, -1};
        }
        const NearestCand old = tid < count ? NearestCand{list_d[cur][tid], list_i[cur][tid]} : NearestCand{nan, -1};
        const uint32_t chunk = Rt - c0 < (uint32_t)(kNearestThreads * kNearestPer) ? Rt - c0 : (uint32_t)(kNearestThreads * kNearestPer);
        int want = (uint32_t)(n - count) < chunk ? n : count + (int)chunk;   // min(n, count + chunk)
        NearestCand prev = {nan, -1};
        int j = 0;
        for (; j < want; ++j) {
            NearestCand b = {nan, -1};
            if (old.index >= 0 && (prev.index < 0 || nearest_before(prev, old))) b = old;
#pragma unroll
            for (int i = 0; i < kNearestPer; ++i)
                if (mine[i].index >= 0 && (prev.index < 0 || nearest_before(prev, mine[i])) && nearest_better(mine[i], b)) b = mine[i];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const NearestCand o = {__shfl_xor(b.dist, off), (int64_t)__shfl_xor((long long)b.index, off)};
                if (nearest_better(o, b)) b = o;
            }
            if (lane == 0) {
                wave_d[j & 1][wave] = b.dist;
                wave_i[j & 1][wave] = b.index;
            }
            __syncthreads();
            b = NearestCand{wave_d[j & 1][0], wave_i[j & 1][0]};
#pragma unroll
            for (int w = 1; w < kNearestThreads / 64; ++w) {
                const NearestCand o = {wave_d[j & 1][w], wave_i[j & 1][w]};
                if (nearest_better(o, b)) b = o;
            }
            if (b.index < 0) break;   // (the same b in every thread) fewer distinct keys than candidates: the list ends here
            if (tid == 0) {
                list_d[cur ^ 1][j] = b.dist;
                list_i[cur ^ 1][j] = b.index;
            }
            prev = b;
        }
        __syncthreads();
        cur ^= 1;
        count = j;
    }
    if (tid < n) {
        best_d[row * (uint64_t)n + tid] = tid < count ? list_d[cur][tid] : nan;
        best_i[row * (uint64_t)n + tid] = tid < count ? list_i[cur][tid] : -1;
    }
}

}  // namespace kpal
