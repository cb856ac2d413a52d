// covis_update.h -- the connection rows of the resident covisibility graph and the host entry points of kernels_covis_update.hip
// (KeyFrame::UpdateConnections and the graph part of LocalMapping::ProcessNewKeyFrame, SPEC DECISION S25).
#pragma once
#include <string>

#include "local_map.h"

namespace orbfe {

constexpr int kCovisMaxConnStride = ORBFE_COVIS_MAX_CONN_STRIDE;
constexpr int kCovisMaxMinWeight = 1 << 20;
constexpr int kUpdateThreads = 256;  // the counting and the selection block
constexpr int kApplyBlocks = 128;    // the reciprocal step's grid: one wave per connected neighbour, this many at a time
constexpr int kAddThreads = 1024;    // the one block of add_keyframe

// mConnectedKeyFrameWeights per key-frame slot, and the hand-over between the launches of one key frame
struct CovisConn {
    int connStride;
    int* slots;    // [kfCap][connStride]
    int* weights;  // [kfCap][connStride]
    int* count;    // [kfCap]
    // work: [kWorkHead ints | slot, weight, mn_id of every counted key frame: 3 x connStride]
    int* work;
};
constexpr int kWorkHead = 8;  // nCounted, refuse (the writing launch returns on it), nConnected

int covis_update_check(const orbfe_covis_update_params* P, std::string& err);
int covis_conn_init_launch(hipStream_t s, const CovisTables& T, const CovisConn& C, std::string& err);
int covis_scatter_connections_launch(hipStream_t s, const CovisTables& T, const CovisConn& C, int n, const int* dSlots, const int* dOff,
                                     const int* dConn, const int* dWeights, std::string& err);
// counters: [kfCap + 1] zeros, left as found.  The outputs of key frame k of a call lie at dSlots + k * connStride, ...
int covis_update_launch(hipStream_t s, const CovisTables& T, const CovisConn& C, const orbfe_world_point* mapPts, int minWeight, int slot,
                        int flag, int* dSlots, int* dWeights, int* dCount, int* dStatus, int* counters, std::string& err);
// stamps: [cap] words at kStampRest, left as found.  conn may be null (connections not enabled)
int covis_add_keyframe_launch(hipStream_t s, const CovisTables& T, const CovisConn* conn, const orbfe_world_point* mapPts, const CovisKf& rec,
                              int slot, const int* dPointIds, int* dAdded, int* dStatus, unsigned* stamps, std::string& err);

}  // namespace orbfe
