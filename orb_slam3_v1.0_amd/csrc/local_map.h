// local_map.h -- the resident covisibility graph (orbfe_covis) and the host entry points of kernels_local_map.hip
// (Tracking::UpdateLocalMap, SPEC DECISION S24).
#pragma once
#include <string>

#include "orbfe_internal.h"

namespace orbfe {

constexpr int kPointsThreads = ORBFE_LOCAL_MAP_BLOCK;            // the points kernel: one chunk of the walk per step
constexpr int kVoteThreads = 256;                                // the votes kernel
constexpr int kVoteTableKeys = ORBFE_LOCAL_MAP_VOTE_TABLE;  // distinct key frames the LDS table takes before the call switches to HBM counters
constexpr int kVoteTableSlots = 2 * kVoteTableKeys;         // open addressing at half load
constexpr int kLocalKfMax = ORBFE_LOCAL_KF_MAX;
constexpr int kCovisMaxKf = 1 << 18;                        // the list's membership bitmap is kf_capacity bits of LDS (32 KiB here)
constexpr int kCovisMaxKfStride = 1 << 20;                  // 288 * 2^20 walk positions stay below 2^31
constexpr int kCovisMaxShort = 4096;                        // obs_stride, child_stride
constexpr size_t kCovisMaxStamps = (size_t)1 << 28;         // batch * capacity words of first-occurrence stamps
constexpr unsigned kStampRest = 0xffffffffu;                // a stamp nobody holds; bit 31 cleared = the point voted in this frame

// the scalars of one key frame (32 bytes)
struct CovisKf {
    int mnId, bad, parent, prev, nFeatures, nCovisible, nChildren, pad;
};

// the tables in HBM; every index stored in them was checked on the host when it was set
struct CovisTables {
    int kfCap, kfStride, obsStride, childStride, cap;
    CovisKf* kf;      // [kfCap]
    int* covisible;   // [kfCap][ORBFE_COVIS_MAX_COVISIBLE]
    int* children;    // [kfCap][childStride]
    int* kfPoints;    // [kfCap][kfStride]
    int* obsCount;    // [cap]
    int* obs;         // [cap][obsStride]
};

// one record of orbfe_covis_set_keyframes in the staged block (ints); the lists follow at their offsets (in ints from the block's start)
struct CovisStagedKf {
    int slot, mnId, bad, parent, prev, nFeatures /* -1: keep */, nCovisible, nChildren, oPoints, oCovisible, oChildren, pad;
};

int local_map_check(const orbfe_local_map_params* P, std::string& err);
int covis_init_launch(hipStream_t s, const CovisTables& T, std::string& err);
int covis_scatter_keyframes_launch(hipStream_t s, const CovisTables& T, int n, const int* dBlock, std::string& err);
int covis_scatter_observations_launch(hipStream_t s, const CovisTables& T, int n, const int* dIds, const int* dOff, const int* dSlots,
                                      std::string& err);
// stamps: [batch][cap] words at kStampRest; counters: [batch][kfCap] zeros -- both left as found
int local_map_launch(hipStream_t s, const orbfe_local_map_params* P, int batch, int voteStride, const CovisTables& T,
                     const orbfe_world_point* mapPts, int M, const orbfe_local_map_io* io, unsigned* stamps, int* counters, std::string& err);
int frame_points_launch(hipStream_t s, int batch, int kpStride, int M, int mapCap, const orbfe_world_point* mapPts, const int* dIds,
                        const int* dMatch, const uint8_t* dOutlier, const int* dN, int* dOut, std::string& err);

}  // namespace orbfe
