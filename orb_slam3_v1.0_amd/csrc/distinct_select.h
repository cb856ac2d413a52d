// distinct_select.h -- the selection arithmetic of MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:397-411), once, for
// kernels_distinct.hip (descriptors the host gathered) and kernels_covis_refresh.hip (descriptors the resident graph indexes): the
// position of the median in a sorted row, the search for the element at that position without sorting, and the packed minimum.
// No HIP here: tests/cpp/*.cpp may include this text as host C++.
#pragma once
#include <cstddef>

#include "host_device.h"

namespace orbfe {

// vDists[0.5 * (N - 1)] (:404): the index is the double truncated towards zero; N >= 1
ORBFE_HD inline int distinct_median_position(int N) { return (int)(size_t)(0.5 * (double)(N - 1)); }

// The element at position k of the sorted row = the smallest v with #{j : dist(i, j) <= v} >= k + 1.  Distances lie in 0..256, so nine
// steps over the VALUE find it; countLE(v) recounts the row (the zero self-distance included) instead of materialising it.
template <class CountLE>
ORBFE_HD inline int distinct_kth_distance(int k, CountLE countLE)
{
    int vlo = 0, vhi = 256;
    while (vlo < vhi) {
        const int mid = (vlo + vhi) >> 1;
        if (countLE(mid) >= k + 1) vhi = mid;
        else vlo = mid + 1;
    }
    return vlo;
}

// the representative is the minimum of (median, tie): the strict "<" of :406 keeps the first minimum of the iteration order, which is
// the row index for gathered descriptors ...
constexpr int kDistinctIndexBits = 20;
ORBFE_HD inline unsigned int distinct_pack(int median, int index) { return ((unsigned int)median << kDistinctIndexBits) | (unsigned int)index; }
// ... and the observer's mn_id for the resident graph (SPEC DECISION S26), then its position in the observation list so that a graph
// with two key frames of one mn_id still has one answer: 9 + 31 + 12 bits
ORBFE_HD inline unsigned long long distinct_pack_observer(int median, int mnId, int position)
{
    return ((unsigned long long)(unsigned int)median << 44) | ((unsigned long long)((unsigned int)mnId & 0x7fffffffu) << 12) |
           (unsigned long long)((unsigned int)position & 0xfffu);
}
constexpr unsigned long long kDistinctNoObserver = ~0ull;

}  // namespace orbfe
