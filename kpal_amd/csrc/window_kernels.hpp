// window_kernels.hpp -- one profile per sliding window of each FASTA record (Profile.from_fasta_by_window; gfx950).
//
// Every window restates Profile.from_sequences (kpal/klib.py:135-170) on the bases [j S, min(j S + W, L)) of its record.
// The cost per base does not grow with the overlap m = W / S (window_index.hpp has the arithmetic):
//   1. window_tiles    : the record is cut into tiles of S bases, a k-mer belongs to the tile its FIRST base lies in;
//                        one 4^k int64 table per tile;
//   2. window_slide    : window j = sum of tiles j .. j + m - 1, a running sum along the tiles (skipped for m = 1: the
//                        tiles are written straight to the caller's windows);
//   3. window_trim     : a window that ends before its record does gives back the at most k - 1 k-mers that begin in its
//                        last k - 1 bases and run past its end.
// The stream is the flattened text of kpal_fasta_records_begin: record r = one '\n' at starts[r], then its bases.
#pragma once
#include "kpal_device.hpp"
#include "window_index.hpp"

namespace kpal {

// the geometry one launch needs: windows [first, first + n) of the piece and their tiles [tile0, tile1)
struct WinGeom {
    const uint64_t *starts;         // R + 1: separator of record r in the stream; starts[R] = stream length
    const uint64_t *first_window;   // R + 1
    const uint64_t *first_tile;     // R + 1
    uint64_t R, W, S;
    uint64_t first, n;
    uint64_t tile0, tile1;
};

// mask (bit 15 - j for the k-mer ENDING at byte p0 + j) of the ends that lie in [e_lo, e_hi)
__device__ __forceinline__ uint32_t win_end_mask(uint64_t p0, uint64_t e_lo, uint64_t e_hi)
{
    // the chunk's bytes [p0, p0 + 16) cut with [e_lo, e_hi); compared as positions before anything is subtracted (a lane
    // behind the tile has p0 > e_hi)
    const uint64_t lo = max(e_lo, p0), hi = min(e_hi, p0 + 16);
    if (lo >= hi) return 0u;
    const uint32_t a = (uint32_t)(lo - p0), b = (uint32_t)(hi - p0);   // 0 <= a < b <= 16
    return (0xFFFFu >> a) & ~(0xFFFFu >> b);
}

// ------------------------------------------------------------------------------------------
// 1a. Tile tables, k <= 7: the tile's histogram lives in LDS (u32 bins, one ds_add per k-mer, as count_lds_direct;
// REP bank-interleaved replicas for the tiny tables), and is stored as the tile's dense int64 table with plain vector
// stores: no global atomics, the destination is not zeroed first.  A workgroup of WAVES waves holds TPW histograms and
// WAVES / TPW waves walk one tile (TPW = 4, one wave per tile, for the tiles of a compositional scan: 500 bases are
// half a wave-step; TPW = 1 with eight waves for long tiles and for k = 7, whose histogram is 64 KiB).  A tile holds
// fewer than 2^32 k-mers (the host sends longer steps to the atomic kernel).
// ------------------------------------------------------------------------------------------
template <int K>
struct WinTileCfg {
    static constexpr int kBins = 1 << (2 * K);
    static constexpr int kRep = kBins >= 1024 ? 1 : (1024 / kBins > 16 ? 16 : 1024 / kBins);
    static constexpr int kSmallTpw = K <= 6 ? 4 : 1;   // histograms per 256-thread workgroup for short tiles
};

template <int K, int TPW, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void window_tiles_lds_kernel(Span s, WinGeom g, unsigned long long *__restrict__ tiles)
{
    constexpr int BINS = WinTileCfg<K>::kBins;
    constexpr int REP = WinTileCfg<K>::kRep;
    constexpr int GROUP = WAVES / TPW;             // waves per tile
    __shared__ uint32_t h[TPW * BINS * REP];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int slot = wave / GROUP, member = wave % GROUP;
    const int rep = lane % REP;
    uint32_t *hist = h + slot * (BINS * REP);
    const uint64_t ntiles = g.tile1 - g.tile0;
    const uint64_t ngroups = (ntiles + TPW - 1) / TPW;
    for (uint64_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
        for (int i = threadIdx.x; i < TPW * BINS * REP; i += WAVES * 64) h[i] = 0;
        __syncthreads();
        const uint64_t local = grp * TPW + slot;   // tile of this wave, relative to tile0
        const bool live = local < ntiles;
        if (live) {
            const uint64_t T = g.tile0 + local;
            const uint64_t r = win_find(g.first_tile, g.R, T);
            const uint64_t rec_end = g.starts[r + 1];
            const uint64_t a = g.starts[r] + 1 + (T - g.first_tile[r]) * g.S;   // first base of the tile
            const uint64_t b = min(a + g.S, rec_end);
            // k-mers that BEGIN in [a, b) END in [a + K - 1, b + K - 1); none ends at or behind the record's end
            const uint64_t e_lo = a + (K - 1), e_hi = min(b + (K - 1), rec_end);
            if (e_lo < e_hi) {
                const uint64_t c_lo = e_lo / 16, c_hi = (e_hi + 15) / 16;
                const uint64_t steps = (c_hi - c_lo + 63) / 64;
                const uint64_t per = (steps + GROUP - 1) / GROUP;
                const uint64_t st0 = member * per, st1 = min(st0 + per, steps);
                if (st0 < st1) {
                    Chunk carry = load_chunk(s, (int64_t)(c_lo + st0 * 64) - 1);
                    for (uint64_t st = st0; st < st1; ++st) {
                        const uint64_t c0 = c_lo + st * 64;
                        uint64_t window;
                        uint32_t mask;
                        if (interior_range(s, c0, c0 + 64)) wave_step<K, false>(s, (int64_t)(c0 + lane), carry, window, mask);
                        else wave_step<K, true>(s, (int64_t)(c0 + lane), carry, window, mask);
                        mask &= win_end_mask((c0 + lane) * 16, e_lo, e_hi);
                        // branch-free: a k-mer that must not be counted adds 0 to whatever bin its bits name
#pragma unroll
                        for (int j = 0; j < 16; ++j) atomicAdd(&hist[kmer_at<K>(window, j) * REP + rep], (mask >> (15 - j)) & 1u);
                    }
                }
            }
        }
        __syncthreads();
        if (live) {
            unsigned long long *dst = tiles + local * BINS;
            for (int bin = member * 64 + lane; bin < BINS; bin += GROUP * 64) {
                unsigned long long v = 0;
#pragma unroll
                for (int q = 0; q < REP; ++q) v += hist[bin * REP + q];
                dst[bin] = v;
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// 1b. Tile tables, any k (the k >= 8 path): one global atomic per k-mer into the (zeroed) table of its tile, in the style
// of count_records_kernel -- the atomic count does not depend on m.  The fed span is the bytes the tiles' k-mers lie in;
// `origin` is the stream position of its first byte.  The record is searched once per lane, the tile follows from the
// position and the record's start.
// ------------------------------------------------------------------------------------------
template <int K>
__global__ __launch_bounds__(256) void window_tiles_atomic_kernel(Span s, uint64_t steps_per_wave, uint64_t origin, WinGeom g,
                                                                  unsigned long long *__restrict__ tiles)
{
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t step0 = wave * steps_per_wave;
    const uint64_t total_steps = (s.nchunks + 63) / 64;
    if (step0 >= total_steps) return;
    const uint64_t step1 = min(step0 + steps_per_wave, total_steps);
    Chunk carry = load_chunk(s, (int64_t)(step0 * 64) - 1);
    for (uint64_t st = step0; st < step1; ++st) {
        uint64_t window;
        uint32_t mask;
        if (interior_range(s, st * 64, st * 64 + 64)) wave_step<K, false>(s, (int64_t)(st * 64 + lane), carry, window, mask);
        else wave_step<K, true>(s, (int64_t)(st * 64 + lane), carry, window, mask);
        if (mask == 0) continue;
        const uint64_t p0 = (st * 64 + lane) * 16;
        // a counted k-mer ends at or behind s.lo + K - 1: its first byte p is in the span, at stream position origin + (p - s.lo)
        uint64_t r = 0, next_start = 0, T = 0, tile_end = 0;   // record, the next record's separator, tile, one past the tile's last base
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (!(mask & (1u << (15 - j)))) continue;
            const uint64_t p = origin + (p0 + j - (K - 1) - s.lo);   // first base of the k-mer (positions ascend with j)
            if (p >= next_start) {
                r = win_find(g.starts, g.R, p);
                next_start = g.starts[r + 1];
                tile_end = 0;
            }
            if (p >= tile_end) {
                const uint64_t base = g.starts[r] + 1;
                const uint64_t t = (p - base) / g.S;
                T = g.first_tile[r] + t;
                tile_end = base + (t + 1) * g.S;
            }
            if (T >= g.tile0 && T < g.tile1) atomicAdd(&tiles[((T - g.tile0) << (2 * K)) + kmer_at<K>(window, j)], 1ULL);
        }
    }
}

// ------------------------------------------------------------------------------------------
// 2. The running sum along the tiles: out[w][bin] = sum of tile[t][bin] over the tiles of window w.  One thread owns one
// bin of a SEGMENT of consecutive windows: it derives the segment's first sum from its m tiles and then adds the tile
// that comes in and takes off the one that goes out (a new record starts a new sum).  Lanes run along the bins: loads
// and stores are coalesced; the segments give one long record at k = 4 (256 bins) thousands of threads.
// ------------------------------------------------------------------------------------------
constexpr int kWinSlideThreads = 256;

__global__ __launch_bounds__(kWinSlideThreads) void window_slide_kernel(WinGeom g, uint64_t bins, uint64_t segment, uint64_t n_segments,
                                                                       const unsigned long long *__restrict__ tiles,
                                                                       unsigned long long *__restrict__ out)
{
    // bins < 256: a workgroup holds 256 / bins segments; else bins / 256 workgroups share a segment
    uint64_t seg, bin;
    if (bins < kWinSlideThreads) {
        seg = (uint64_t)blockIdx.x * (kWinSlideThreads / bins) + threadIdx.x / bins;
        bin = threadIdx.x % bins;
    } else {
        const uint64_t per_seg = bins / kWinSlideThreads;
        seg = blockIdx.x / per_seg;
        bin = (blockIdx.x % per_seg) * kWinSlideThreads + threadIdx.x;
    }
    if (seg >= n_segments) return;
    const uint64_t m = g.W / g.S;
    const uint64_t w0 = g.first + seg * segment, w1 = min(w0 + segment, g.first + g.n);
    uint64_t r = win_find(g.first_window, g.R, w0);
    uint64_t j = w0 - g.first_window[r];
    uint64_t next_first = g.first_window[r + 1];
    uint64_t nt = win_tiles(win_record_bases(g.starts, r), g.S);
    // tile t of record r is row first_tile[r] + t - tile0 of the buffer; rows before it (a range that begins inside a
    // record) are never read: a window of the range begins at or behind tile0
    int64_t row0 = (int64_t)g.first_tile[r] - (int64_t)g.tile0;
    unsigned long long sum = 0;
    bool fresh = true;
    for (uint64_t w = w0; w < w1; ++w, ++j) {
        if (w >= next_first) {   // the next record that has windows
            do ++r; while (g.first_window[r + 1] <= w);
            j = 0;
            next_first = g.first_window[r + 1];
            nt = win_tiles(win_record_bases(g.starts, r), g.S);
            row0 = (int64_t)g.first_tile[r] - (int64_t)g.tile0;
            fresh = true;
        }
        if (fresh) {
            sum = 0;
            const uint64_t t1 = min(j + m, nt);
            for (uint64_t t = j; t < t1; ++t) sum += tiles[(uint64_t)(row0 + (int64_t)t) * bins + bin];
            fresh = false;
        } else {
            sum -= tiles[(uint64_t)(row0 + (int64_t)(j - 1)) * bins + bin];
            if (j + m - 1 < nt) sum += tiles[(uint64_t)(row0 + (int64_t)(j + m - 1)) * bins + bin];
        }
        out[(w - g.first) * bins + bin] = sum;
    }
}

// ------------------------------------------------------------------------------------------
// 3. The trim: one thread per window.  A window that ends at base e before its record does gives back the k-mers that
// begin in [e - k + 1, e): they END in [e, e + k - 1), and each is re-encoded from the stream with its validity (the
// reference's rolling window, kpal/klib.py:157-168).  At most k - 1 subtractions per window, plain loads and stores (two
// of them may name the same bin: one thread does them in turn).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void window_trim_kernel(WinGeom g, int k, const uint8_t *__restrict__ flat, unsigned long long *__restrict__ out)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.n) return;
    const uint64_t w = g.first + i;
    const uint64_t r = win_find(g.first_window, g.R, w);
    const uint64_t j = w - g.first_window[r];
    const uint64_t L = win_record_bases(g.starts, r);
    if (!win_trimmed(j, L, g.W, g.S)) return;
    const uint64_t e = j * g.S + g.W;
    const uint8_t *seq = flat + g.starts[r] + 1;
    const uint64_t q1 = min(e + (uint64_t)(k - 1), L);   // one past the last byte a straddling k-mer may end at
    const uint64_t kmask = k >= 32 ? ~0ULL : ((1ULL << (2 * k)) - 1ULL);
    unsigned long long *table = out + (i << (2 * k));
    uint64_t kmer = 0;
    int run = 0;   // valid bytes in a row
    for (uint64_t q = e - (uint64_t)(k - 1); q < q1; ++q) {
        const uint8_t c = seq[q];
        const uint8_t u = c & 0xDF;
        if (u == 'A' || u == 'C' || u == 'G' || u == 'T') {
            kmer = ((kmer << 2) | (uint64_t)(((c >> 1) ^ (c >> 2)) & 3)) & kmask;
            ++run;
        } else {
            run = 0;
        }
        if (q >= e && run >= k) table[kmer] -= 1;
    }
}

}  // namespace kpal
