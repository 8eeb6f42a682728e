// smooth_plan.hpp -- what the host decides about dynamic smoothing over whole SETS of profiles before it launches anything
// (kpal_cross_smooth_distance_device, kpal_smooth_distance_matrix_device; the kernels: smooth_set_kernels.hpp).  No GPU in it:
// kpal_cross.hip, the kernels (the layout functions) and a CPU program (tests/test_smooth_plan_host.py) read the same definitions.
//
// The reference collapses node (start, length) iff min(f(left quarter sums), f(right quarter sums)) <= threshold
// (kdistlib.py:99-100), which is f(left quarters) <= t OR f(right quarters) <= t: each side's flag depends on that profile
// alone.  So every profile gets, once, its PYRAMID: the wrapping int64 sum of every node of every level, and one code per node --
//   1  the node is flagged and no strict ancestor is      2  a strict ancestor is flagged      0  otherwise
// (a bin: 2 if any node above it is flagged, else 1 -- a function of its bottom node's code, never stored).  For a pair, over
// "all bins + all nodes", element e is LIVE iff max(code_left(e), code_right(e)) == 1, and the reference's smoothed pair is
// the live bins with their counts and the live nodes with their sums (in the node's first bin), zero everywhere else.
//
// Layout of one profile's pyramid: HEIGHT h = 0 .. k-1 has 4^(k-1-h) nodes (height 0: the nodes of four bins; height k-1: the
// root), bottom first, so that the four children of a node are 32-byte aligned; padded with dead elements (sum 0, code 2) to
// a multiple of kSuperBins, which both rectangle skeletons can walk.
#pragma once
#include "matrix_plan.hpp"

namespace kpal {

// Pyramids of one call: as many bytes as kdistlib.cross_distances keeps of right-side tables at a time (CROSS_MAX_BYTES),
// the largest workspace a rectangle is sized for elsewhere.  Never a query of free memory: the route is a function of the call.
constexpr uint64_t kSmoothBudgetBytes = 32ULL << 30;

constexpr int kSmoothPadding = -1;   // SmoothElement::height of an element behind the root

KPAL_MATRIX_HD uint64_t smooth_level_nodes(int k, int h) { return 1ULL << (2 * (k - 1 - h)); }
// 4^(k-1) + ... + 4^(k-h)
KPAL_MATRIX_HD uint64_t smooth_level_offset(int k, int h) { return ((1ULL << (2 * k)) - (1ULL << (2 * (k - h)))) / 3; }
KPAL_MATRIX_HD uint64_t smooth_nodes(int k) { return ((1ULL << (2 * k)) - 1) / 3; }
KPAL_MATRIX_HD uint64_t smooth_stride(int k)
{
    return (smooth_nodes(k) + (uint64_t)kSuperBins - 1) / (uint64_t)kSuperBins * (uint64_t)kSuperBins;
}

struct SmoothElement {
    int height;      // kSmoothPadding: no node
    uint64_t node;   // 0 .. 4^(k-1-height) - 1
};
KPAL_MATRIX_HD SmoothElement smooth_element(int k, uint64_t e)
{
    for (int h = 0; h < k; ++h) {
        const uint64_t nodes = smooth_level_nodes(k, h);
        if (e < nodes) return SmoothElement{h, e};
        e -= nodes;
    }
    return SmoothElement{kSmoothPadding, e};
}

// Scratch of nprof pyramids: the sums (int64), the codes and the nodes' own flags (a byte each), one array behind the other.
constexpr uint64_t kSmoothElementBytes = 8 + 1 + 1;
inline uint64_t smooth_scratch_bytes(int k, uint64_t nprof) { return nprof * smooth_stride(k) * kSmoothElementBytes; }

// Whether a smoothed rectangle of Q x R profiles (a triangle: R = 0) runs as a fixed number of launches.  With do_positive
// the masks come before the smoothing and a node's sums depend on the partner; pyramids past the budget do not fit: both keep
// one pair pipeline per pair.
inline bool smooth_batched(int k, int Q, int R, bool do_positive, uint64_t budget_bytes)
{
    return !do_positive && smooth_scratch_bytes(k, (uint64_t)Q + (uint64_t)R) <= budget_bytes;
}

}  // namespace kpal
