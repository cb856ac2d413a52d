// covis_refresh.h -- the refresh state of the resident covisibility graph and the host entry points of kernels_covis_refresh.hip
// (MapPoint::UpdateDepth and MapPoint::ComputeDistinctiveDescriptors, SPEC DECISION S26).
#pragma once
#include <string>

#include "local_map.h"

namespace orbfe {

constexpr int kRefreshMaxLevels = ORBFE_REFRESH_MAX_LEVELS;
constexpr int kRefreshThreads = 256;                 // both refresh kernels
constexpr int kRefreshWaves = kRefreshThreads / 64;  // points per block on the wave path
constexpr int kRefreshWaveObs = 64;                  // observers the wave path takes: one per lane
constexpr int kRefreshRestBlocks = 256;              // the rest path's grid: a block per listed point, this many at a time

// what orbfe_covis_enable_refresh adds; nLevels == 0 until then.  Every index stored here was checked on the host when it was set
// or is clamped by the kernel that writes it; the kernels that read test them again.
struct CovisRefresh {
    int nLevels;
    uint8_t* desc;    // [kfCap][kfStride][32]
    uint8_t* octave;  // [kfCap][kfStride]
    int* nFeat;       // [kfCap]: the count of the last set_features, 0 before
    float* centre;    // [kfCap][3]
    int* obsIdx;      // [cap][obsStride], parallel to CovisTables::obs; -1 = leftIndex == -1
    int* refKf;       // [cap]: mpRefKF as a slot, -1 = none
    float* sf;        // [kRefreshMaxLevels]
    // scratch of the call: [2 counters | restCap entries].  The wave launch of a call appends to counter `parity` and puts the other one
    // back to zero; the next call uses the other one, so no launch is spent on a reset.
    int* rest;
    int restCap;
    int parity;
};

struct RefreshOut {
    int* status;
    float *minDistance, *maxDistance;
    int *bestSlot, *bestIndex, *bestMedian;
};

int covis_set_features_launch(hipStream_t s, const CovisTables& T, const CovisRefresh& R, int slot, int n, const orbfe_keypoint* dKp,
                              const uint8_t* dDesc, std::string& err);
int covis_scatter_centres_launch(hipStream_t s, const CovisTables& T, const CovisRefresh& R, int n, const int* dSlots, const float* dTwc,
                                 std::string& err);
// dIdx == nullptr: every index of the named points becomes -1 (the setter without indices)
int covis_scatter_indices_launch(hipStream_t s, const CovisTables& T, const CovisRefresh& R, int n, const int* dIds, const int* dOff,
                                 const int* dIdx, std::string& err);
int covis_scatter_ref_launch(hipStream_t s, const CovisTables& T, const CovisRefresh& R, int n, const int* dIds, const int* dRef,
                             std::string& err);
int covis_index_added_launch(hipStream_t s, const CovisTables& T, const CovisRefresh& R, int slot, int nFeatures, const int* dPointIds,
                             const int* dAdded, std::string& err);
// two launches; R.rest holds at least n entries and R.parity names the counter at zero
int covis_refresh_launch(hipStream_t s, const CovisTables& T, const CovisRefresh& R, orbfe_world_point* mapPts, uint8_t* mapDesc, int n,
                         const int* dIds, const int* dSelect, int selectValue, int what, const RefreshOut& out, std::string& err);

}  // namespace orbfe
