// stat_set_kernels.hpp -- the summaries (Profile.total / non_zero / mean / median / std, kpal/klib.py:193-225) and the strand
// balance (kmer.get_balance, kpal/kmer.py:243-245) of ALL profiles of a set at once (gfx950).  Profile p of a pass is the table at
// tables + p * bins.  The streaming kernels run on a grid of slices x profiles (stat_plan.hpp: a slice is 8192 bins, one
// workgroup of 256 threads; its number depends on `bins` alone), the small ones on one wave or one workgroup per profile.
//
//   T1  stats_set_kernel         a StatPartial per slice: 128-bit sum, non-zero count, min, max (stats_kernel's arithmetic)
//   T2  stats_set_final_kernel   a profile's slices combined in slice order; total, non_zero, min, max, mean; the select state
//   T3  var_set_kernel           sum of ((double)x - mean)^2 per slice: per lane, wave tree, workgroup (stats_var_kernel's)
//   T4  var_set_final_kernel     slices in a fixed order; std = sqrt(ss / bins)
//   T5  select_hist_set_kernel   one 8-bit digit of every profile's radix select: LDS histogram, integer atomics into hist[p]
//   T6  select_pick_set_kernel   the digit that holds rank (bins - 1) / 2, per profile; extends its prefix; clears hist[p]
//   T7  select_next_set_kernel   the smallest key above the lower middle one, where the upper middle one is another value
//   T8  median_set_kernel        median = ((double)v0 + (double)v1) / 2
//   B1  strand_balance_set_kernel<PW>         k < 6: fused split + multiset, a (sum, count) partial per 256 bins
//   B2  strand_balance_tiled_set_kernel<PW>   k >= 6: the same over 64 x 64 LDS tiles, a partial per tile
//
// B1 and B2 are the only strand balance kernels: kpal_strand_balance runs them on a set of one table.  (The summaries of one
// table still have kernels of their own, stat_kernels.hpp: at k = 15 the set pass on one table is slower, docs/NOTEBOOK.md.)
//
// A profile whose smallest and largest key agree in a byte (and in every byte above it) has the same digit there in every
// entry: T5 and T6 leave it alone at that byte (StatSetState::top) -- the digit is the smallest key's, which the prefix starts
// as.  So a constant table costs no select pass, and a table of small counts next to one with 10^12 in it costs its own bytes.
// 8 bytes of HBM traffic per bin and pass; LDS: 1 KiB (T5), 2 KiB (T6), 160 B or less elsewhere.
#pragma once
#include "stat_kernels.hpp"
#include "stat_plan.hpp"
#include "matrix_common.hpp"

namespace kpal {

static_assert(sizeof(StatPartial) == kStatPartialBytes, "stat_plan.hpp sizes the scratch of a StatPartial");
static_assert(kStatSetThreads == kStatThreads, "the set kernels reduce a workgroup as the single-profile kernels do");

constexpr uint32_t kStatErrRank = 1;   // select_pick_set_kernel: no digit holds the rank
constexpr uint32_t kStatErrNext = 2;   // median_set_kernel: no key above the lower middle one

static __global__ __launch_bounds__(kStatSetThreads) void stats_set_kernel(const int64_t *__restrict__ tables, uint64_t bins,
                                                                          StatPartial *__restrict__ partial)
{
    __shared__ StatPartial wsum[kStatSetThreads / 64];
    const int64_t *x = tables + (uint64_t)blockIdx.y * bins;
    const uint64_t end = stat_slice_end(bins, blockIdx.x);
    StatPartial p = {0, 0, 0, INT64_MAX, INT64_MIN};
    for (uint64_t i = stat_slice_begin(blockIdx.x) + threadIdx.x; i < end; i += kStatSetThreads) {
        const int64_t v = x[i];
        const uint64_t lo = p.sum_lo + (uint64_t)v;
        p.sum_hi += (v >> 63) + (lo < p.sum_lo ? 1 : 0);   // sign extension of v plus the carry
        p.sum_lo = lo;
        p.non_zero += v != 0;
        p.mn = v < p.mn ? v : p.mn;
        p.mx = v > p.mx ? v : p.mx;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const StatPartial o = stat_shfl_down(p, d);
        stat_combine(p, o);
    }
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = p;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kStatSetThreads / 64; ++w) stat_combine(p, wsum[w]);
        partial[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = p;
    }
}

// One wave per profile.  top_max: the highest StatSetState::top of the pass (the host runs that many digits).
static __global__ __launch_bounds__(64) void stats_set_final_kernel(const StatPartial *__restrict__ partial, uint32_t slices, uint64_t bins,
                                                                   StatSetState *__restrict__ state, kpal_profile_stats *__restrict__ out,
                                                                   int *__restrict__ top_max)
{
    const StatPartial *src = partial + (uint64_t)blockIdx.x * slices;
    StatPartial p = {0, 0, 0, INT64_MAX, INT64_MIN};
    for (uint32_t s = threadIdx.x; s < slices; s += 64) stat_combine(p, src[s]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const StatPartial o = stat_shfl_down(p, d);
        stat_combine(p, o);
    }
    if (threadIdx.x == 0) {
        kpal_profile_stats r;
        r.total = (int64_t)p.sum_lo;
        r.non_zero = (int64_t)p.non_zero;
        r.min = p.mn;
        r.max = p.mx;
        r.mean = stat_mean(p.sum_lo, p.sum_hi, bins);
        r.median = 0.0;
        r.std = 0.0;
        out[blockIdx.x] = r;
        StatSetState st;
        st.prefix = select_key(p.mn);
        st.below = 0;
        st.equal = bins;
        st.next = UINT64_MAX;
        st.mean = r.mean;
        st.top = stat_top_byte(select_key(p.mn), select_key(p.mx));
        st.reserved = 0;
        state[blockIdx.x] = st;
        if (st.top >= 0) atomicMax(top_max, st.top);
    }
}

static __global__ __launch_bounds__(kStatSetThreads) void var_set_kernel(const int64_t *__restrict__ tables, uint64_t bins,
                                                                        const StatSetState *__restrict__ state, double *__restrict__ partial)
{
    __shared__ double wsum[kStatSetThreads / 64];
    const int64_t *x = tables + (uint64_t)blockIdx.y * bins;
    const double mean = state[blockIdx.y].mean;
    const uint64_t end = stat_slice_end(bins, blockIdx.x);
    double s = 0.0;
    for (uint64_t i = stat_slice_begin(blockIdx.x) + threadIdx.x; i < end; i += kStatSetThreads) {
        const double d = (double)x[i] - mean;
        s += d * d;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kStatSetThreads / 64; ++w) s += wsum[w];
        partial[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

// One wave per profile: lane l adds slices l, l + 64, ... in that order, then the wave's tree.
static __global__ __launch_bounds__(64) void var_set_final_kernel(const double *__restrict__ partial, uint32_t slices, uint64_t bins,
                                                                 kpal_profile_stats *__restrict__ out)
{
    const double *src = partial + (uint64_t)blockIdx.x * slices;
    double s = 0.0;
    for (uint32_t i = threadIdx.x; i < slices; i += 64) s += src[i];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d);
    if (threadIdx.x == 0) out[blockIdx.x].std = sqrt(s / (double)bins);
}

// hist[p][d] += entries of the slice whose key has the digits chosen so far above byte `byte` and digit d there.  Counts
// concentrate in one digit: the wave counts the digit of its first lane with a ballot, only the other lanes use an LDS atomic
// each (select_hist_kernel).
static __global__ __launch_bounds__(kStatSetThreads) void select_hist_set_kernel(const int64_t *__restrict__ tables, uint64_t bins,
                                                                                const StatSetState *__restrict__ state, int byte,
                                                                                unsigned long long *__restrict__ hist)
{
    __shared__ uint32_t h[kStatHistBins];
    if (byte > state[blockIdx.y].top) return;   // (the whole workgroup: every entry has the smallest key's digit here)
    const int64_t *x = tables + (uint64_t)blockIdx.y * bins;
    const uint64_t mask = stat_mask_above(byte), prefix = state[blockIdx.y].prefix & mask;
    const int shift = 8 * byte;
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t begin = stat_slice_begin(blockIdx.x), end = stat_slice_end(bins, blockIdx.x);
    const uint32_t rounds = (uint32_t)((end - begin + kStatSetThreads - 1) / kStatSetThreads);   // every lane runs every round: the ballots need whole waves
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint64_t i = begin + (uint64_t)r * kStatSetThreads + threadIdx.x;
        uint32_t d = 0xFFFFFFFFu;
        if (i < end) {
            const uint64_t key = select_key(x[i]);
            if ((key & mask) == prefix) d = (uint32_t)(key >> shift) & 255u;
        }
        const uint32_t hot = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
        const bool eq = d == hot && d != 0xFFFFFFFFu;
        const uint32_t same = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(eq));
        if (same && (threadIdx.x & 63) == 0) atomicAdd(&h[hot], same);
        if (!eq && d != 0xFFFFFFFFu) atomicAdd(&h[d], 1u);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&hist[(uint64_t)blockIdx.y * kStatHistBins + threadIdx.x], (unsigned long long)h[threadIdx.x]);
}

// One workgroup per profile: the digit d with below + hist[0 .. d-1] <= rank < below + hist[0 .. d]; hist[p] is zero afterwards.
static __global__ __launch_bounds__(kStatHistBins) void select_pick_set_kernel(StatSetState *__restrict__ state, unsigned long long *__restrict__ hist,
                                                                              uint64_t bins, int byte, uint32_t *__restrict__ error)
{
    __shared__ unsigned long long h[kStatHistBins];
    if (byte > state[blockIdx.x].top) return;
    unsigned long long *mine = hist + (uint64_t)blockIdx.x * kStatHistBins;
    h[threadIdx.x] = mine[threadIdx.x];
    mine[threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x == 0) {
        StatSetState st = state[blockIdx.x];
        const uint64_t rank = (bins - 1) / 2;
        uint64_t acc = st.below;
        int d = 0;
        for (; d < (int)kStatHistBins; ++d) {
            if (rank < acc + h[d]) break;
            acc += h[d];
        }
        if (d == (int)kStatHistBins) {
            atomicOr(error, kStatErrRank);
            return;
        }
        st.below = acc;
        st.equal = h[d];
        st.prefix = (st.prefix & ~(255ULL << (8 * byte))) | ((uint64_t)d << (8 * byte));
        state[blockIdx.x] = st;
    }
}

// state[p].next = the smallest key above state[p].prefix (the lower middle key), for the profiles whose upper middle entry,
// rank bins / 2, is not among the entries equal to it.
static __global__ __launch_bounds__(kStatSetThreads) void select_next_set_kernel(const int64_t *__restrict__ tables, uint64_t bins,
                                                                                StatSetState *__restrict__ state)
{
    __shared__ uint64_t wmin[kStatSetThreads / 64];
    const uint64_t key0 = state[blockIdx.y].prefix;
    if (bins / 2 < state[blockIdx.y].below + state[blockIdx.y].equal) return;
    const int64_t *x = tables + (uint64_t)blockIdx.y * bins;
    const uint64_t end = stat_slice_end(bins, blockIdx.x);
    uint64_t m = UINT64_MAX;
    for (uint64_t i = stat_slice_begin(blockIdx.x) + threadIdx.x; i < end; i += kStatSetThreads) {
        const uint64_t key = select_key(x[i]);
        if (key > key0 && key < m) m = key;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t o = shfl_down_u64(m, d);
        m = o < m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kStatSetThreads / 64; ++w) m = wmin[w] < m ? wmin[w] : m;
        if (m != UINT64_MAX) atomicMin((unsigned long long *)&state[blockIdx.y].next, (unsigned long long)m);
    }
}

// np.median: the mean of the two middle elements.
static __global__ __launch_bounds__(256) void median_set_kernel(const StatSetState *__restrict__ state, uint64_t bins, uint32_t count,
                                                               kpal_profile_stats *__restrict__ out, uint32_t *__restrict__ error)
{
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    if (p >= count) return;
    const StatSetState st = state[p];
    const int64_t v0 = (int64_t)(st.prefix ^ 0x8000000000000000ULL);
    int64_t v1 = v0;
    if (bins / 2 >= st.below + st.equal) {
        if (st.next == UINT64_MAX) atomicOr(error, kStatErrNext);
        v1 = (int64_t)(st.next ^ 0x8000000000000000ULL);
    }
    out[p].median = ((double)v0 + (double)v1) / 2.0;
}

// ---- strand balance: multiset(*split()) fused, the profile from blockIdx.y.  A single profile (kpal_strand_balance) is a set of
// one: these are the only strand balance kernels. ----
// k < 6: the workgroups of blockIdx.x stride through the n bins of the profile.
template <int PW>
__global__ __launch_bounds__(256) void strand_balance_set_kernel(const int64_t *__restrict__ tables, int k, uint64_t n,
                                                                 Partial *__restrict__ partials)
{
    const int64_t *c = tables + (uint64_t)blockIdx.y * n;
    Partial p = {0.0, 0ULL};
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = revcomp(i, k);
        if (i > r) continue;
        int64_t f, v;
        if (i < r) {
            f = (int64_t)((uint64_t)c[i] * 2ULL);
            v = (int64_t)((uint64_t)c[r] * 2ULL);
        } else {
            f = v = c[i];
        }
        if (f != 0 || v != 0) {
            p.s += PW == 0 ? pw_prod(f, v) : pw_sum(f, v);
            p.m += 1;
        }
    }
    p = block_reduce(p);
    if (threadIdx.x == 0) partials[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = p;
}

// k >= 6: kmer.get_balance score (kpal/kmer.py:243-245) with the split halves never materialised: every
// unordered pair {i, rc(i)} is visited once -- from the tile of the smaller M, or, inside a
// self-paired tile, from its smaller index (palindromes contribute f = r = c[i], klib.py:322-323).
// Tile M = blockIdx.x.
template <int PW>
__global__ __launch_bounds__(1024) void strand_balance_tiled_set_kernel(const int64_t *__restrict__ tables, int k,
                                                                        Partial *__restrict__ partials)
{
    __shared__ unsigned long long A[64][65], B[64][65];
    constexpr int T = 3, S = 64;
    const int64_t *c = tables + ((uint64_t)blockIdx.y << (2 * k));
    const int md = k - 2 * T;
    const uint64_t M = blockIdx.x;
    const uint64_t Mr = md > 0 ? revcomp(M, md) : 0;
    Partial p = {0.0, 0ULL};
    if (M <= Mr) {
        const bool self = M == Mr;
        const uint64_t rowstride = 1ULL << (2 * (k - T));
        const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
        const unsigned long long *uc = reinterpret_cast<const unsigned long long *>(c);
        for (int h = w; h < S; h += 16) {
            A[h][lane] = uc[(uint64_t)h * rowstride + M * S + lane];
            if (!self) B[h][lane] = uc[(uint64_t)h * rowstride + Mr * S + lane];
        }
        __syncthreads();
        const int rl = (int)revcomp((uint64_t)lane, T);
        for (int h = w; h < S; h += 16) {
            const int rh = (int)revcomp((uint64_t)h, T);
            const unsigned long long mine = A[h][lane];
            const unsigned long long other = self ? A[rl][rh] : B[rl][rh];
            int64_t f, v;
            bool take = true;
            if (self) {
                const int i_loc = h * S + lane, r_loc = rl * S + rh;   // order inside the tile == global order
                take = i_loc <= r_loc;
                if (i_loc == r_loc) {
                    f = v = (int64_t)mine;
                } else {
                    f = (int64_t)(mine * 2ULL);
                    v = (int64_t)(other * 2ULL);
                }
            } else {
                f = (int64_t)(mine * 2ULL);
                v = (int64_t)(other * 2ULL);
            }
            if (take && (f != 0 || v != 0)) {
                p.s += PW == 0 ? pw_prod(f, v) : pw_sum(f, v);
                p.m += 1;
            }
        }
    }
    p = block_reduce(p);
    if (threadIdx.x == 0) partials[(uint64_t)blockIdx.y * gridDim.x + blockIdx.x] = p;
}

}  // namespace kpal
