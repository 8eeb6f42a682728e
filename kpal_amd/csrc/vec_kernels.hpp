// vec_kernels.hpp -- streaming kernels over 4^k int64 count vectors (gfx950).
//   balance            Profile.balance            kpal/klib.py:285-298
//   split              Profile.split              kpal/klib.py:300-327
//   pair distance      metrics.multiset/euclidean kpal/metrics.py:101-135
// All are HBM-bandwidth kernels.  (The distance matrix, kdistlib.distance_matrix, is fp64-VALU bound and lives in
// cross_kernels.hpp -- the triangle is a set crossed with itself -- and matrix_all_kernels.hpp; what those share with the
// pair kernels here is matrix_common.hpp.  The strand balance, kmer.get_balance, of one profile or of a set: stat_set_kernels.hpp.)
// fp64 sums are reduced in a FIXED order (per-thread serial, wave shuffle tree, block tree,
// then a single-workgroup pass over the per-block partials) so results are run-to-run
// reproducible; they agree with NumPy's pairwise summation to ~1e-15 relative.
// Two units include this header (kpal_vec.hip; kpal_pair.hip for the pair kernels): the kernels that are no templates are static.
#pragma once
#include "matrix_common.hpp"

namespace kpal {

// ---- balance ------------------------------------------------------------------------------
// out[i] = in[i] + in[rc(i)] (i == rc(i) gives 2*in[i], klib.py:297-298).  Out of place.
static __global__ __launch_bounds__(256) void balance_oop_kernel(const int64_t *__restrict__ in, int64_t *__restrict__ out,
                                                          int k, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = (int64_t)((uint64_t)in[i] + (uint64_t)in[revcomp(i, k)]);
}

// In place: the thread owning i < rc(i) updates both ends of the pair (klib.py:290-296).
static __global__ __launch_bounds__(256) void balance_inplace_kernel(int64_t *__restrict__ c, int k, uint64_t n)
{
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = revcomp(i, k);
        if (i < r) {
            const uint64_t v = (uint64_t)c[i] + (uint64_t)c[r];
            c[i] = (int64_t)v;
            c[r] = (int64_t)v;
        } else if (i == r) {
            c[i] = (int64_t)((uint64_t)c[i] * 2ULL);
        }
    }
}

// LDS-tiled balance for k >= 6.  Write i = (H, M, L) with H / L the top / bottom three digits
// and M the k-6 middle digits; then rc(i) = (rc(L), rc(M), rc(H)): the 64x64 tile {(H, M, L)} maps
// onto the tile of rc(M), transposed and with rows/columns permuted by the 3-digit reverse
// complement.  One workgroup owns the tile pair (M, rc(M)), M <= rc(M): it reads both tiles as 64
// runs of 512 B, keeps them in LDS (rows padded to 65 to spread banks on the transposed read),
// and writes out[i] = in[i] + in[rc(i)] for both tiles -- 16 B of HBM traffic per bin instead of
// scattered 8-byte partner accesses.  in == out is allowed (all reads precede the barrier).
// The tile pairs come from a LIST (canon[c] = M of the c-th canonical pair, built by the host: kpal_vec.hip, canon_tiles) and the
// persistent workgroups take them round robin -- every workgroup gets the same number of pairs to within one.  (Striding through
// M itself and skipping the non-canonical ones left the work badly spread: a workgroup's M share their low digits, and those
// decide whether M <= rc(M) for nearly all of them -- a quarter of the workgroups had eight pairs, a quarter none.)
static __global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8))) void balance_tiled_kernel(const int64_t *in, int64_t *out, int k,
                                                                                                     const uint32_t *__restrict__ canon, uint32_t ncanon)
{
    constexpr int T = 3, S = 64;
    __shared__ unsigned long long A[S][S + 1];
    __shared__ unsigned long long B[S][S + 1];
    const int md = k - 2 * T;
    const uint64_t nM = 1ULL << (2 * md);
    const uint64_t rowstride = 1ULL << (2 * (k - T));
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int rl = (int)revcomp((uint64_t)lane, T);
    const unsigned long long *uin = reinterpret_cast<const unsigned long long *>(in);
    unsigned long long *uout = reinterpret_cast<unsigned long long *>(out);
    // persistent workgroups over the canonical tile pairs (M <= rc(M)); the next pair's eight values
    // per thread are loaded before the current pair is exchanged through LDS and written back.
    // The ORDER of the list (k >= 13) is page-aware: see canon_tiles.
    (void)nM;
    auto fetch = [&](uint64_t M, unsigned long long (&a)[4], unsigned long long (&b)[4]) {
        const uint64_t Mr = md > 0 ? revcomp(M, md) : 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint64_t row = (uint64_t)(w + 16 * q) * rowstride;
            a[q] = uin[row + M * S + lane];
            b[q] = uin[row + Mr * S + lane];
        }
    };
    unsigned long long a[4], b[4], na[4], nb[4];
    uint32_t seq = blockIdx.x;
    if (seq < ncanon) fetch(canon[seq], a, b);
    while (seq < ncanon) {
        const uint64_t M = canon[seq];
        const uint32_t seqn = seq + gridDim.x;
        if (seqn < ncanon) fetch(canon[seqn], na, nb);
        const uint64_t Mr = md > 0 ? revcomp(M, md) : 0;
        const bool self = M == Mr;
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
            uout[row + M * S + lane] = a[q] + B[rl][rh];
            if (!self) uout[row + Mr * S + lane] = b[q] + A[rl][rh];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            a[q] = na[q];
            b[q] = nb[q];
        }
        seq = seqn;
    }
}

// ---- split --------------------------------------------------------------------------------
// Order-preserving compaction of i <= rc(i).  Pass 1 counts canonical indices per block-sized
// segment; the host scans the (small) count array; pass 2 writes.
constexpr int kSplitSeg = 4096;  // indices per block

static __global__ __launch_bounds__(256) void split_count_kernel(int k, uint64_t n, uint32_t *__restrict__ seg_count)
{
    const uint64_t base = (uint64_t)blockIdx.x * kSplitSeg;
    uint32_t c = 0;
    for (int t = threadIdx.x; t < kSplitSeg; t += blockDim.x) {
        const uint64_t i = base + t;
        if (i < n && i <= revcomp(i, k)) ++c;
    }
    __shared__ uint32_t sh[4];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_down(c, d);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) seg_count[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}

static __global__ __launch_bounds__(256) void split_write_kernel(const int64_t *__restrict__ c, int k, uint64_t n,
                                                          const uint64_t *__restrict__ seg_offset,
                                                          int64_t *__restrict__ fwd, int64_t *__restrict__ rev)
{
    __shared__ uint32_t wave_tot[4];
    const uint64_t base = (uint64_t)blockIdx.x * kSplitSeg;
    uint64_t out = seg_offset[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t0 = 0; t0 < kSplitSeg; t0 += 256) {
        const uint64_t i = base + t0 + threadIdx.x;
        uint64_t r = 0;
        bool keep = false;
        if (i < n) {
            r = revcomp(i, k);
            keep = i <= r;
        }
        const unsigned long long bal = __ballot(keep);
        const uint32_t before = __popcll(bal & ((1ULL << lane) - 1ULL));
        if (lane == 0) wave_tot[wave] = __popcll(bal);
        __syncthreads();
        uint32_t wbase = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (w < wave) wbase += wave_tot[w];
            tot += wave_tot[w];
        }
        if (keep) {
            const uint64_t o = out + wbase + before;
            if (i < r) {
                fwd[o] = (int64_t)((uint64_t)c[i] * 2ULL);   // klib.py:319-320
                rev[o] = (int64_t)((uint64_t)c[r] * 2ULL);
            } else {
                fwd[o] = c[i];                               // klib.py:322-323
                rev[o] = c[i];
            }
        }
        out += tot;
        __syncthreads();
    }
}

// ---- pair distance --------------------------------------------------------------------------
// METRIC 0/1: multiset prod/sum (metrics.py:121-123); 2: euclidean (int64 dot, metrics.py:135,46).
template <int METRIC, typename T>
__global__ __launch_bounds__(256) void pair_distance_kernel(const T *__restrict__ l, const T *__restrict__ r,
                                                            uint64_t n, Partial *__restrict__ partials)
{
    Partial p = {0.0, 0ULL};
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    // two elements per 16-byte load
    const uint64_t n2 = n >> 1;
    using V2 = typename std::conditional<std::is_same<T, double>::value, double2, longlong2>::type;
    const V2 *l2 = reinterpret_cast<const V2 *>(l);
    const V2 *r2 = reinterpret_cast<const V2 *>(r);
    auto term = [&](T x, T y) {
        if constexpr (METRIC == 2) {
            const uint64_t d = (uint64_t)x - (uint64_t)y;
            p.m += d * d;
        } else {
            if (x != 0 || y != 0) {
                p.s += METRIC == 0 ? pw_prod(x, y) : pw_sum(x, y);
                p.m += 1;
            }
        }
    };
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += stride) {
        const V2 a = l2[i], b = r2[i];
        term((T)a.x, (T)b.x);
        term((T)a.y, (T)b.y);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) term(l[n - 1], r[n - 1]);
    p = block_reduce(p);
    if (threadIdx.x == 0) partials[blockIdx.x] = p;
}

// ---- fused balance + distance, fused split + multiset (k >= 6) ----------------------------------
// Same tiling as balance_tiled_kernel: the workgroup of tile pair (M, rc(M)) forms the balanced
// values x = l[i] + l[rc(i)], y = r[i] + r[rc(i)] on the fly (kpal/kdistlib.py:139-141) and
// reduces the metric over the 2 x 4096 bins of the pair -- 16 B of HBM traffic per bin, no balanced
// copies.  The two LDS tiles (66 KiB: two workgroups per CU) are used twice: first for the left
// profile, whose balanced values stay in registers (8 per thread), then for the right profile,
// whose global loads are already in flight while the left one is transposed.
// PREFETCH: persistent workgroups, the next pair's values requested before the current pair is worked on -- ~120 registers, so
// ONE 1024-thread workgroup per CU (the launcher sizes the grid for that).  Without (KPAL_PDB_PREFETCH=0, A/B only): one pair at
// a time; forced into 64 registers for two workgroups per CU it spills and ran at half the rate (k = 12: 0.126 vs 0.059 ms).
template <int METRIC, bool PREFETCH>
__device__ __forceinline__ void pair_distance_balanced_body(const int64_t *__restrict__ l, const int64_t *__restrict__ r, int k,
                                                            const uint32_t *__restrict__ canon, uint32_t ncanon,
                                                            Partial *__restrict__ partials, unsigned long long (*A)[65], unsigned long long (*B)[65])
{
    constexpr int T = 3, S = 64;
    const int md = k - 2 * T;
    const uint64_t nM = 1ULL << (2 * md);
    const uint64_t rowstride = 1ULL << (2 * (k - T));
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (wave-uniform: row addresses are scalar)
    const int rl = (int)revcomp((uint64_t)lane, T);
    const unsigned long long *ul = reinterpret_cast<const unsigned long long *>(l);
    const unsigned long long *ur = reinterpret_cast<const unsigned long long *>(r);
    Partial p = {0.0, 0ULL};
    // persistent workgroups over the list of canonical tile pairs (M <= rc(M): balance_tiled_kernel), round robin; the next
    // pair's 16 values per thread are loaded before the current pair is transposed and reduced
    (void)nM;
    auto fetch = [&](uint64_t M, unsigned long long (&la)[4], unsigned long long (&lb)[4], unsigned long long (&ra)[4],
                     unsigned long long (&rb)[4]) {
        // (everything but the lane is wave-uniform: said explicitly, the loads take a scalar base + the lane's offset)
        const uint64_t Mu = (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)M);
        const uint64_t Mr = md > 0 ? (uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)revcomp(Mu, md)) : 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint64_t row = (uint64_t)(w + 16 * q) * rowstride;
            const unsigned long long *pla = ul + (row + Mu * S), *plb = ul + (row + Mr * S);
            const unsigned long long *pra = ur + (row + Mu * S), *prb = ur + (row + Mr * S);
            la[q] = pla[lane];
            lb[q] = plb[lane];
            ra[q] = pra[lane];
            rb[q] = prb[lane];
        }
    };
    auto term = [&](unsigned long long xu, unsigned long long yu) {
        const int64_t x = (int64_t)xu, y = (int64_t)yu;
        if constexpr (METRIC == 2) {
            const uint64_t d = (uint64_t)x - (uint64_t)y;
            p.m += d * d;
        } else {
            if (x != 0 || y != 0) {
                p.s += METRIC == 0 ? pw_prod(x, y) : pw_sum(x, y);
                p.m += 1;
            }
        }
    };
    unsigned long long la[4], lb[4], ra[4], rb[4], nla[4], nlb[4], nra[4], nrb[4];
    uint32_t seq = blockIdx.x;
    if (PREFETCH && seq < ncanon) fetch(canon[seq], la, lb, ra, rb);
    while (seq < ncanon) {
        const uint64_t M = canon[seq];
        const uint32_t seqn = seq + gridDim.x;
        if constexpr (PREFETCH) {
            if (seqn < ncanon) fetch(canon[seqn], nla, nlb, nra, nrb);
        } else {
            fetch(M, la, lb, ra, rb);
        }
        const bool self = md == 0 || M == revcomp(M, md);
        auto exchange = [&](unsigned long long (&a)[4], unsigned long long (&b)[4]) {
            // a/b: this thread's bins of tile M / rc(M); on return each holds bin + bin[rc]
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                A[w + 16 * q][lane] = a[q];
                B[w + 16 * q][lane] = b[q];   // self: B == A
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int rh = (int)revcomp((uint64_t)(w + 16 * q), T);
                a[q] += B[rl][rh];
                b[q] += A[rl][rh];
            }
            __syncthreads();
        };
        exchange(la, lb);
        exchange(ra, rb);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            term(la[q], ra[q]);
            if constexpr (!PREFETCH) __builtin_amdgcn_sched_barrier(0);   // (64 registers: one division's temporaries at a time)
            if (!self) term(lb[q], rb[q]);
            if constexpr (!PREFETCH) __builtin_amdgcn_sched_barrier(0);
        }
        if constexpr (PREFETCH) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                la[q] = nla[q];
                lb[q] = nlb[q];
                ra[q] = nra[q];
                rb[q] = nrb[q];
            }
        }
        seq = seqn;
    }
    p = block_reduce(p);
    if (threadIdx.x == 0) partials[blockIdx.x] = p;
}

template <int METRIC>
__global__ __launch_bounds__(1024) void pair_distance_balanced_kernel(const int64_t *__restrict__ l, const int64_t *__restrict__ r, int k,
                                                                      const uint32_t *__restrict__ canon, uint32_t ncanon,
                                                                      Partial *__restrict__ partials)
{
    __shared__ unsigned long long A[64][65], B[64][65];
    pair_distance_balanced_body<METRIC, true>(l, r, k, canon, ncanon, partials, A, B);
}

// Final fixed-order reduction of per-block partials: out[q] = sum over blocks of partials[q*nblocks + b].
static __global__ __launch_bounds__(256) void reduce_partials_kernel(const Partial *__restrict__ partials, uint32_t nblocks,
                                                              Partial *__restrict__ out)
{
    const Partial *src = partials + (uint64_t)blockIdx.x * nblocks;
    Partial p = {0.0, 0ULL};
    for (uint32_t b = threadIdx.x; b < nblocks; b += blockDim.x) {
        p.s += src[b].s;
        p.m += src[b].m;
    }
    p = block_reduce(p);
    if (threadIdx.x == 0) out[blockIdx.x] = p;
}

}  // namespace kpal
