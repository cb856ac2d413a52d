// covis_refresh_check.h -- what the S26 setters decide on the host before the device is touched, and the layout of their staged blocks.
// Host-pure: no HIP header, only staging.h and the C ABI's keypoint, so the validation and the layout are exercised without a GPU and
// under sanitizers (tests/cpp/point_refresh.cpp).  Every function returns true when the arguments are in order; nothing is written.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/orbfe.h"
#include "staging.h"

namespace orbfe {

struct RefreshDims {
    int kfCap, kfStride, obsStride, cap, nLevels;
};

inline bool refresh_features_ok(const RefreshDims& D, int slot, int n, const orbfe_keypoint* kp, const uint8_t* desc, bool hostArrays)
{
    if (slot < 0 || slot >= D.kfCap || n < 0 || n > D.kfStride || (n > 0 && (!kp || !desc))) return false;
    if (hostArrays)   // the device form clamps the octaves instead
        for (int i = 0; i < n; i++)
            if (kp[i].octave < 0 || kp[i].octave >= D.nLevels) return false;
    return true;
}

inline bool refresh_centres_ok(const RefreshDims& D, int n, const int* slots, const float* twc)
{
    if (n < 0 || (n > 0 && (!slots || !twc))) return false;
    std::vector<char> seen((size_t)D.kfCap, 0);
    for (int i = 0; i < n; i++) {
        if (slots[i] < 0 || slots[i] >= D.kfCap || seen[(size_t)slots[i]]) return false;
        seen[(size_t)slots[i]] = 1;
        for (int c = 0; c < 3; c++)
            if (!std::isfinite(twc[3 * (size_t)i + c])) return false;
    }
    return true;
}

inline bool refresh_ids_distinct(int n, const int* ids)
{
    std::vector<int> sorted(ids, ids + n);
    std::sort(sorted.begin(), sorted.end());
    return std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end();
}

// the CSR block of both observation setters; featIdx is looked at only when `indexed`
inline bool refresh_observations_ok(const RefreshDims& D, int n, const int* ids, const int* off, const int* kfSlots, const int* featIdx,
                                    bool indexed)
{
    if (n < 0 || (n > 0 && (!ids || !off))) return false;
    if (n == 0) return true;
    if (off[0] < 0) return false;
    for (int i = 0; i < n; i++)
        if (ids[i] < 0 || ids[i] >= D.cap || off[i + 1] < off[i] || off[i + 1] - off[i] > D.obsStride) return false;
    if (!refresh_ids_distinct(n, ids)) return false;
    const int total = off[n];
    if (total > off[0] && (!kfSlots || (indexed && !featIdx))) return false;
    for (int k = off[0]; k < total; k++)
        if (kfSlots[k] < 0 || kfSlots[k] >= D.kfCap || (indexed && (featIdx[k] < -1 || featIdx[k] >= D.kfStride))) return false;
    return true;
}

inline bool refresh_refs_ok(const RefreshDims& D, int n, const int* ids, const int* refSlots)
{
    if (n < 0 || (n > 0 && (!ids || !refSlots))) return false;
    for (int i = 0; i < n; i++)
        if (ids[i] < 0 || ids[i] >= D.cap || refSlots[i] < -1 || refSlots[i] >= D.kfCap) return false;
    return n == 0 || refresh_ids_distinct(n, ids);
}

// ---- the staged blocks: taken in this order, all inputs ----
struct FeaturesStage {
    Block<orbfe_keypoint> kp;
    Block<uint8_t> desc;
    FeaturesStage(Staging& st, int n) : kp(st.in<orbfe_keypoint>((size_t)std::max(n, 1))), desc(st.in<uint8_t>((size_t)std::max(n, 1) * ORBFE_DESC_BYTES)) {}
    void fill(const Staging& st, int n, const orbfe_keypoint* k, const uint8_t* d) const
    {
        st.put(kp, k, (size_t)n);
        st.put(desc, d, (size_t)n * ORBFE_DESC_BYTES);
    }
};

struct ObservationsStage {
    Block<int> ids, off, slots, idx;
    int total;
    ObservationsStage(Staging& st, int n, const int* off_, bool indexed)
        : ids(st.in<int>((size_t)n)), off(st.in<int>((size_t)n + 1)), slots(st.in<int>((size_t)std::max(off_[n], 1))),
          idx(st.in<int>(indexed ? (size_t)std::max(off_[n], 1) : 0)), total(off_[n])
    {
    }
    void fill(const Staging& st, const int* ids_, const int* off_, const int* kfSlots, const int* featIdx) const
    {
        st.put(ids, ids_);
        st.put(off, off_);
        st.put(slots, kfSlots, (size_t)total);
        if (idx.n) st.put(idx, featIdx, (size_t)total);
    }
};

// the list and the six result rows of orbfe_covis_refresh_points
struct RefreshStage {
    Block<int> ids, status;
    Block<float> minD, maxD;
    Block<int> slot, index, median;
    RefreshStage(Staging& st, int n)
        : ids(st.in<int>((size_t)n)), status(st.out<int>((size_t)n)), minD(st.out<float>((size_t)n)), maxD(st.out<float>((size_t)n)),
          slot(st.out<int>((size_t)n)), index(st.out<int>((size_t)n)), median(st.out<int>((size_t)n))
    {
    }
};

}  // namespace orbfe
