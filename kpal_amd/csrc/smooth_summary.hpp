// smooth_summary.hpp -- the summary function of the dynamic-smoothing test (kdistlib.py:99-100), ONE definition for the pair
// pipeline (option_kernels.hpp) and for the pyramids of whole sets (smooth_set_kernels.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kpal {

constexpr int kSummaryMin = 0, kSummaryAverage = 1, kSummaryMedian = 2;

// Summary of four int64 quarter sums as NumPy evaluates it on an int64 array of length 4:
// np.min -> the integer; np.mean -> float64 sum of the converted values / 4; np.median -> mean of
// the two middle values.  Returned as double for the comparison with the threshold.
__device__ __forceinline__ double summarise4(const int64_t (&q)[4], int summary)
{
    if (summary == kSummaryMin) return (double)min(min(q[0], q[1]), min(q[2], q[3]));
    if (summary == kSummaryAverage) return ((((double)q[0] + (double)q[1]) + (double)q[2]) + (double)q[3]) / 4.0;
    // median: sort four values with a 5-comparator network, average the middle two
    int64_t a = min(q[0], q[1]), b = max(q[0], q[1]), c = min(q[2], q[3]), d = max(q[2], q[3]);
    const int64_t lo = max(a, c), hi = min(b, d);   // the two middle values are {max of mins, min of maxes}
    return ((double)min(lo, hi) + (double)max(lo, hi)) / 2.0;
}

}  // namespace kpal
