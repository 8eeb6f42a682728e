// spectrum_kernels.hpp -- the count-of-counts spectrum (metrics.distribution, kpal/metrics.py:22-33) of ALL tables of a set at
// once, without a sort (gfx950).  Table t of a pass is at tables + t * bins; the plan (window, LDS bins, scratch) is
// spectrum_plan.hpp's.  The streaming kernels run on the grid of stat_set_kernels.hpp, slices x tables, a slice of 8192 bins per
// workgroup of 256 threads; the window kernels on window slices x tables.
//
//   (T1 stats_set_kernel          min and max per slice: the partials of the summaries, stat_set_kernels.hpp)
//   P1  spectrum_range_kernel     a table's slices combined: its smallest key and (largest - smallest); the widest of the pass
//   P2  spectrum_hist_kernel      window counters: LDS-private for the first spectrum_lds_bins(W), global atomics for the rest,
//                                 flushed once per workgroup; entries past the window are COUNTED per table
//   P3  spectrum_nonzero_kernel   non-zero window counters per window slice
//   P4  spectrum_scan_kernel      exclusive scan of those over slices and tables: one workgroup, chunk after chunk with a carry
//   P5  spectrum_compact_kernel   (value, number) of the non-zero counters, ascending, at the scanned offsets
//   P6  spectrum_overflow_kernel  only if P2 counted any: (key, table) of the entries past the window, appended with one cursor
//                                 bump per wave; tables that have none are skipped by their workgroups
//
// K-mer tables are runs of few values (zeros are more than 99 % of a k = 12 table of a read), so 64 lanes on one LDS address
// is the common case: a wave counts the value of its first lane that is still waiting with a ballot and a popcount and adds it
// ONCE, kSpectrumPeels times at most (one: more rounds were timed and cost more than the colliding atomics they save,
// docs/NOTEBOOK.md); the lanes left over add one each.  All counters of a window and all numbers are 64-bit:
// a value may fill a k = 16 table.  P2 reads 8 bytes per bin; LDS 16 KiB + 16 B (P2), 32 B (P3, P5), 128 B (P4).
#pragma once
#include "stat_kernels.hpp"
#include "stat_plan.hpp"
#include "spectrum_plan.hpp"

namespace kpal {

static_assert(sizeof(SpectrumRange) == kSpectrumRangeBytes && sizeof(SpectrumOverflow) == kSpectrumOverflowBytes,
              "spectrum_plan.hpp sizes the scratch of a range and of an overflow entry");
static_assert(kSpectrumWindowSlice == (uint64_t)kStatSetThreads * kSpectrumCompactPerThread, "a thread of the compaction takes its run of counters");
static_assert(kStatSliceBins <= 0xFFFFFFFFull, "the LDS counters of a slice are 32-bit");

__device__ __forceinline__ uint64_t spectrum_readlane(uint64_t v, int lane)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}

// One workgroup per table (min and max do not care in which order they are taken: a k = 15 table has 131 072 slices).
// widest: the largest `wide` of the pass (the host chooses the window from it).
static __global__ __launch_bounds__(kStatSetThreads) void spectrum_range_kernel(const StatPartial *__restrict__ partial, uint32_t slices,
                                                                               SpectrumRange *__restrict__ range,
                                                                               unsigned long long *__restrict__ widest)
{
    __shared__ int64_t wmn[kStatSetThreads / 64], wmx[kStatSetThreads / 64];
    const StatPartial *src = partial + (uint64_t)blockIdx.x * slices;
    int64_t mn = INT64_MAX, mx = INT64_MIN;
    for (uint32_t s = threadIdx.x; s < slices; s += kStatSetThreads) {
        mn = src[s].mn < mn ? src[s].mn : mn;
        mx = src[s].mx > mx ? src[s].mx : mx;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int64_t on = (int64_t)shfl_down_u64((uint64_t)mn, d), ox = (int64_t)shfl_down_u64((uint64_t)mx, d);
        mn = on < mn ? on : mn;
        mx = ox > mx ? ox : mx;
    }
    if ((threadIdx.x & 63) == 0) {
        wmn[threadIdx.x >> 6] = mn;
        wmx[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kStatSetThreads / 64; ++w) {
            mn = wmn[w] < mn ? wmn[w] : mn;
            mx = wmx[w] > mx ? wmx[w] : mx;
        }
        SpectrumRange r;
        r.kmin = spectrum_key(mn);
        r.wide = spectrum_key(mx) - r.kmin;
        range[blockIdx.x] = r;
        atomicMax(widest, (unsigned long long)r.wide);
    }
}

// n entries at window offset `off` of this workgroup's table: LDS, the global window, or past it.
__device__ __forceinline__ void spectrum_add(uint32_t *h, unsigned long long *win, uint32_t lds, uint64_t window, uint64_t off, uint32_t n,
                                             uint32_t &over)
{
    if (off < lds) atomicAdd(&h[(uint32_t)off], n);
    else if (off < window) atomicAdd(&win[off], (unsigned long long)n);
    else over += n;
}

static __global__ __launch_bounds__(kStatSetThreads) void spectrum_hist_kernel(const int64_t *__restrict__ tables, uint64_t bins,
                                                                              const SpectrumRange *__restrict__ range, uint64_t window,
                                                                              unsigned long long *__restrict__ windows,
                                                                              unsigned long long *__restrict__ overflow)
{
    __shared__ uint32_t h[kSpectrumLdsBins];
    __shared__ uint32_t wover[kStatSetThreads / 64];
    const int64_t *x = tables + (uint64_t)blockIdx.y * bins;
    unsigned long long *win = windows + (uint64_t)blockIdx.y * window;
    const uint64_t kmin = range[blockIdx.y].kmin;
    const uint32_t lds = spectrum_lds_bins(window);
    const int lane = threadIdx.x & 63;
    for (uint32_t i = threadIdx.x; i < lds; i += kStatSetThreads) h[i] = 0;
    __syncthreads();
    const uint64_t begin = stat_slice_begin(blockIdx.x), end = stat_slice_end(bins, blockIdx.x);
    const uint32_t rounds = (uint32_t)((end - begin + kStatSetThreads - 1) / kStatSetThreads);   // every lane runs every round: the ballots need whole waves
    uint32_t over = 0;
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint64_t i = begin + (uint64_t)r * kStatSetThreads + threadIdx.x;
        bool waiting = i < end;
        const uint64_t off = waiting ? spectrum_offset(spectrum_key(x[i]), kmin) : 0;
        uint64_t todo = __builtin_amdgcn_ballot_w64(waiting);
        for (int peel = 0; peel < kSpectrumPeels && todo != 0; ++peel) {
            const int lead = __ffsll((unsigned long long)todo) - 1;
            const uint64_t hot = spectrum_readlane(off, lead);
            const uint64_t same = __builtin_amdgcn_ballot_w64(waiting && off == hot);
            if (lane == lead) spectrum_add(h, win, lds, window, hot, (uint32_t)__popcll(same), over);
            waiting = waiting && off != hot;
            todo &= ~same;
        }
        if (waiting) spectrum_add(h, win, lds, window, off, 1u, over);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) over += __shfl_down(over, d);
    if (lane == 0) wover[threadIdx.x >> 6] = over;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < lds; i += kStatSetThreads)
        if (h[i]) atomicAdd(&win[i], (unsigned long long)h[i]);
    if (threadIdx.x == 0) {
        for (int w = 1; w < kStatSetThreads / 64; ++w) over += wover[w];
        if (over) atomicAdd(&overflow[blockIdx.y], (unsigned long long)over);
    }
}

// nz[t * gridDim.x + s] = non-zero counters of window slice s of table t.
static __global__ __launch_bounds__(kStatSetThreads) void spectrum_nonzero_kernel(const unsigned long long *__restrict__ windows, uint64_t window,
                                                                                 unsigned long long *__restrict__ nz)
{
    __shared__ uint32_t wsum[kStatSetThreads / 64];
    const unsigned long long *win = windows + (uint64_t)blockIdx.y * window;
    const uint64_t first = (uint64_t)blockIdx.x * kSpectrumWindowSlice + (uint64_t)threadIdx.x * kSpectrumCompactPerThread;
    uint32_t n = 0;
#pragma unroll
    for (int j = 0; j < kSpectrumCompactPerThread; ++j)
        if (first + j < window && win[first + j] != 0) ++n;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_down(n, d);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kStatSetThreads / 64; ++w) n += wsum[w];
        nz[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = n;
    }
}

// In place: nz[i] = nz[0] + ... + nz[i - 1] for i < m, nz[m] = the sum of all.  ONE workgroup; it takes kSpectrumScanThreads
// entries at a time and carries their sum into the next chunk, so any number of tables is one launch.
static __global__ __launch_bounds__(kSpectrumScanThreads) void spectrum_scan_kernel(unsigned long long *__restrict__ nz, uint64_t m)
{
    __shared__ unsigned long long wsum[kSpectrumScanThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long carry = 0;
    for (uint64_t base = 0; base < m; base += kSpectrumScanThreads) {
        const uint64_t i = base + threadIdx.x;
        const unsigned long long mine = i < m ? nz[i] : 0;
        unsigned long long incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned long long o = ((unsigned long long)__shfl_up((uint32_t)(incl >> 32), d) << 32) | __shfl_up((uint32_t)incl, d);
            if (lane >= d) incl += o;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        unsigned long long before = carry, chunk = 0;
        for (int w = 0; w < kSpectrumScanThreads / 64; ++w) {
            if (w < wave) before += wsum[w];
            chunk += wsum[w];
        }
        if (i < m) nz[i] = before + incl - mine;
        carry += chunk;
        __syncthreads();
    }
    if (threadIdx.x == 0) nz[m] = carry;
}

// The non-zero counters of window slice blockIdx.x of table blockIdx.y as (value, number), ascending, from where the scan put them.
static __global__ __launch_bounds__(kStatSetThreads) void spectrum_compact_kernel(const unsigned long long *__restrict__ windows, uint64_t window,
                                                                                 const SpectrumRange *__restrict__ range,
                                                                                 const unsigned long long *__restrict__ scanned,
                                                                                 int64_t *__restrict__ values, unsigned long long *__restrict__ numbers)
{
    __shared__ uint32_t wsum[kStatSetThreads / 64];
    const unsigned long long *win = windows + (uint64_t)blockIdx.y * window;
    const uint64_t kmin = range[blockIdx.y].kmin;
    const uint64_t first = (uint64_t)blockIdx.x * kSpectrumWindowSlice + (uint64_t)threadIdx.x * kSpectrumCompactPerThread;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long c[kSpectrumCompactPerThread];
    uint32_t n = 0;
#pragma unroll
    for (int j = 0; j < kSpectrumCompactPerThread; ++j) {
        c[j] = first + j < window ? win[first + j] : 0;
        n += c[j] != 0;
    }
    uint32_t incl = n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint64_t at = scanned[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] + incl - n;
    for (int w = 0; w < wave; ++w) at += wsum[w];
#pragma unroll
    for (int j = 0; j < kSpectrumCompactPerThread; ++j) {
        if (c[j] != 0) {
            values[at] = spectrum_value(kmin + first + j);
            numbers[at] = c[j];
            ++at;
        }
    }
}

// (key, table) of every entry past its table's window, in no particular order: cursor[0] counts them, entries from `capacity`
// on are not written (the host sized the list by the counts of P2).
static __global__ __launch_bounds__(kStatSetThreads) void spectrum_overflow_kernel(const int64_t *__restrict__ tables, uint64_t bins,
                                                                                  const SpectrumRange *__restrict__ range, uint64_t window,
                                                                                  const unsigned long long *__restrict__ overflow,
                                                                                  unsigned long long *__restrict__ cursor,
                                                                                  SpectrumOverflow *__restrict__ list, uint64_t capacity)
{
    if (overflow[blockIdx.y] == 0) return;   // (the whole workgroup)
    const int64_t *x = tables + (uint64_t)blockIdx.y * bins;
    const uint64_t kmin = range[blockIdx.y].kmin;
    const int lane = threadIdx.x & 63;
    const uint64_t begin = stat_slice_begin(blockIdx.x), end = stat_slice_end(bins, blockIdx.x);
    const uint32_t rounds = (uint32_t)((end - begin + kStatSetThreads - 1) / kStatSetThreads);
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint64_t i = begin + (uint64_t)r * kStatSetThreads + threadIdx.x;
        uint64_t key = 0;
        bool out = false;
        if (i < end) {
            key = spectrum_key(x[i]);
            out = !spectrum_in_window(key, kmin, window);
        }
        const uint64_t mask = __builtin_amdgcn_ballot_w64(out);
        if (mask == 0) continue;
        const int lead = __ffsll((unsigned long long)mask) - 1;
        unsigned long long base = 0;
        if (lane == lead) base = atomicAdd(cursor, (unsigned long long)__popcll(mask));
        base = spectrum_readlane(base, lead);
        if (out) {
            const uint64_t at = base + (uint64_t)__popcll(mask & ((1ULL << lane) - 1ULL));
            if (at < capacity) {
                SpectrumOverflow e;
                e.key = key;
                e.table = blockIdx.y;
                list[at] = e;
            }
        }
    }
}

}  // namespace kpal
