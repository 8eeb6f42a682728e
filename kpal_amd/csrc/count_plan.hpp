// count_plan.hpp -- what the counting front end decides on the host before it launches anything: the pipeline of a piece
// (the AUTO rule), the size of a piece, the grid of a wave-per-range launch.  No GPU in it: kpal_count.hip /
// kpal_records.hip and a CPU program (tests/test_count_plan_host.py) read the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/kpal_hip.h"

namespace kpal {

// The concrete strategy of a count of k-mers of length k for the requested one (AUTO: by k alone).  A strategy that does
// not serve this k is one of the error codes; the caller has the messages.
constexpr int kPlanNeedsLdsK = -1;      // LDS-direct needs k <= 7
constexpr int kPlanNeedsOneLevelK = -2; // the one-level partitions need 8 <= k <= 12
constexpr int kPlanNeedsTwoLevelK = -3; // the two-level partitions need 13 <= k <= 16

inline int plan_resolve(int requested, int k)
{
    int s = requested;
    if (s == KPAL_STRATEGY_AUTO)
        s = k <= 7 ? KPAL_STRATEGY_LDS_DIRECT : (k <= 12 ? KPAL_STRATEGY_PARTITION_QUADS : KPAL_STRATEGY_PARTITION2_QUADS);
    if (s == KPAL_STRATEGY_LDS_DIRECT && k > 7) return kPlanNeedsLdsK;
    if ((s == KPAL_STRATEGY_PARTITION || s == KPAL_STRATEGY_PARTITION_CHUNKED || s == KPAL_STRATEGY_PARTITION_QUADS) && (k < 8 || k > 12))
        return kPlanNeedsOneLevelK;
    if ((s == KPAL_STRATEGY_PARTITION2 || s == KPAL_STRATEGY_PARTITION2_QUADS) && (k < 13 || k > 16)) return kPlanNeedsTwoLevelK;
    return s;
}

// The strategy of one piece of n bytes: `resolved` is plan_resolve's answer, `is_auto` whether AUTO was asked for (an explicit
// strategy is never rewritten), `fresh_candidate` whether the piece may be a FRESH one (the table still unzeroed, a whole
// device feed, nothing of the feed to its left).
inline int plan_strategy(int resolved, bool is_auto, int k, size_t n, bool fresh_candidate)
{
    if (!is_auto) return resolved;
    // tiny feeds (single records, short reads lists): the partition pipelines cost a fixed
    // 0.1 - 0.5 ms (launches, one merge of the whole table); a quarter million atomics do not
    if (k >= 8 && n <= ((size_t)1 << 18)) return KPAL_STRATEGY_GLOBAL_ATOMIC;
    // the quad pipeline pays a fixed histogram stage (one 128 KiB workgroup per bucket): medium feeds take the chunked one
    if (resolved == KPAL_STRATEGY_PARTITION_QUADS && n < ((size_t)32 << 20)) return KPAL_STRATEGY_PARTITION_CHUNKED;
    // The two-level quad pipeline pays per FEED for the whole table -- its forms are staged (4 bytes per entry) and the finalisation
    // reads them and the table and writes the table -- where the round-1 two-level pipeline adds into the table with atomics and
    // pays for the table once per count (memset, Profile.balance).  Measured at the end of round 4 (same box, count + balance,
    // 68 MB .. 15 GB of reads): a feed that is the FIRST piece of a count and a whole device buffer (FRESH: no memset, the table
    // not read, the balance fused) is faster through the quads at every size from 64 MiB up -- k = 15: 4.7 vs 9.5 ms on 68 MB, 8.6
    // vs 23.7 on 4.2 GB; k = 16: 19.3 vs 30.5 and 24.2 vs 54.6, and 34.9 vs 92.8 ms on the 15.1 GB of BASELINE's reads, which the
    // earlier rule (feed >= 4 bytes per table entry, from round-2 timings of both pipelines) still sent to the old pipeline --
    // except that a count that is never balanced loses ~7 % below an eighth of a byte per entry (k = 16).  Any other feed (a later
    // piece, a piece of a host feed, a FASTA chunk) takes the quads once it holds about three bytes per table entry (the per-feed
    // crossover computed from the same timings: 2.8 B per entry at k = 15, 1.5 at k = 16).
    if (resolved == KPAL_STRATEGY_PARTITION2_QUADS) {
        const uint64_t bins = 1ULL << (2 * k);
        const size_t need = fresh_candidate ? (size_t)(bins / 8) : (size_t)(bins * 3);
        const size_t floor64 = (size_t)64 << 20;
        if (n < (need > floor64 ? need : floor64)) return KPAL_STRATEGY_PARTITION2;
    }
    return resolved;
}

// The constants of the kernel headers that bound a piece (partition_kernels.hpp, chunk_kernels.hpp): the caller fills them in.
struct PlanLimits {
    uint64_t chunk_id_bits;             // kChunkIdBits
    uint64_t chunk_keys;                // kChunkKeys
    uint64_t num_buckets;               // kNumBuckets
    uint64_t steps_per_block_quantum;   // kStepsPerBlockQuantum
};

// Bytes per piece of a feed of n bytes on `strategy`: a multiple of 16, at least 16.  A strategy without a bound of its own
// (global atomics) takes the n bytes, rounded like every other piece.
inline size_t plan_piece_bytes(int strategy, int k, size_t n, int num_cu, size_t batch_bytes, bool batch_bytes_set, const PlanLimits &lim)
{
    const size_t cap16 = (size_t)16 << 30;
    size_t piece = n;
    if (strategy == KPAL_STRATEGY_PARTITION) piece = batch_bytes;
    else if (strategy == KPAL_STRATEGY_PARTITION_CHUNKED) {
        // as large as the 20-bit chunk ids allow (G workgroups x R chunks each < 2^20, R = steps/4 + 1088 in
        // launch_partition_chunked): every piece ends with a merge of the whole table and four launches.
        // 1.86 GiB on 256 CUs; KPAL_BATCH_BYTES lowers it.
        const uint64_t G = (uint64_t)num_cu * 2;
        const uint64_t r_max = ((1ull << lim.chunk_id_bits) - 1) / G;
        const uint64_t fixed = 2 * lim.num_buckets + 64;
        uint64_t spb_max = r_max > fixed + 64 ? (r_max - fixed) * (lim.chunk_keys / 1024) : 64;
        spb_max = spb_max > 3 * lim.steps_per_block_quantum ? spb_max - 2 * lim.steps_per_block_quantum : spb_max;   // margin: the halo may add a step
        spb_max = spb_max / lim.steps_per_block_quantum * lim.steps_per_block_quantum;
        const size_t cap = (size_t)(spb_max * G * 1024);
        piece = batch_bytes_set && batch_bytes < cap ? batch_bytes : cap;
    }
    else if (strategy == KPAL_STRATEGY_PARTITION_QUADS) {
        // the record pool takes 4/3 of the input bytes (up to 8 x that for heavily skewed input, whose tiles are
        // smaller): pieces of up to 16 GiB (KPAL_BATCH_BYTES lowers it)
        piece = batch_bytes_set && batch_bytes < cap16 ? batch_bytes : cap16;
    }
    else if (strategy == KPAL_STRATEGY_PARTITION2_QUADS) {
        // two record pools of ~4/3 of the input bytes each: pieces of up to 16 GiB
        piece = batch_bytes_set && batch_bytes * 16 < cap16 ? batch_bytes * 16 : cap16;
    }
    else if (strategy == KPAL_STRATEGY_PARTITION2) {
        // every batch ends with a read-modify-write of the whole 4^k table (0.5 - 32 GiB): few, large
        // batches.  In-bucket offsets are 32-bit: below 2^32 keys per batch always safe (k = 13 has
        // only four coarse buckets); larger batches are checked per coarse bucket and halved if needed.
        const size_t cap13 = (size_t)0xF0000000u;
        piece = k == 13 ? (batch_bytes * 4 < cap13 ? batch_bytes * 4 : cap13) : (batch_bytes * 16 < cap16 ? batch_bytes * 16 : cap16);
    }
    else if (strategy == KPAL_STRATEGY_LDS_DIRECT) piece = (size_t)1 << 31;
    piece &= ~(size_t)15;
    if (piece == 0) piece = 16;
    return piece;
}

// A launch in which every wave takes a contiguous range of wave-steps: as many waves as fill the device once
// (blocks_per_cu workgroups of waves_per_block waves on each CU), each taking spw steps.
struct WaveGrid {
    uint64_t spw;    // steps per wave (>= 1)
    unsigned grid;   // workgroups
};

inline WaveGrid wave_grid(uint64_t steps, int num_cu, int blocks_per_cu, int waves_per_block)
{
    const uint64_t max_waves = (uint64_t)num_cu * blocks_per_cu * waves_per_block;
    const uint64_t spw = steps > max_waves ? (steps + max_waves - 1) / max_waves : 1;
    const uint64_t waves = (steps + spw - 1) / spw;
    return {spw, (unsigned)((waves + waves_per_block - 1) / waves_per_block)};
}

}  // namespace kpal
