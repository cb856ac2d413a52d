// orbfe_host.cpp -- host orchestration + C ABI (include/orbfe.h) of the MI355X ORB front-end.
//
// Mirrors the host side of the reference extractor (src/ORBextractor.cc): constructor tables
// (:82-149), AllocatePyramid (:587-605), ComputePyramid (:607-623), ComputeKeyPointsOctTree
// (:433-541) and extractFeatures (:543-585) -- but as ONE ordered chain of asynchronous kernel
// launches on one HIP stream, with no host synchronisation between stages (the reference syncs
// >= 8 times per level) and no per-frame allocation.
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <condition_variable>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "launch.h"
#include "fast_common.h"
#include "match.h"
#include "match_common.h"
#include "match_proj.h"
#include "keyframe.h"
#include "local_map.h"
#include "covis_update.h"
#include "covis_refresh.h"
#include "covis_refresh_check.h"
#include "marginalize.h"
#include "poseimu_math.h"
#include "prep.h"
#include "vocab.h"

using namespace orbfe;

namespace {

constexpr int kEventSets = 128;

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

const char* kStageNames[ORBFE_NUM_STAGES] = {"pyramid_resize", "fast_nms_blur",
                                             "quadtree", "orient_brief", "total"};

// the staging of one per-frame chain: a device input and a device result block, each with a pinned mirror
// (chain_blocks_alloc / chain_blocks_free)
struct ChainBlocks {
    uint8_t *dIn = nullptr, *hIn = nullptr, *dOut = nullptr, *hOut = nullptr;
};

// The captured graphs of one chain.  Keys are compared as bytes: a key is zeroed with memset before it is filled, so that
// padding compares equal.  Bounded: a caller cycling through more keys than `bound` drops everything and starts afresh.
template <class Key>
struct GraphCache {
    struct Entry {
        Key key;
        hipGraphExec_t exec;
    };
    std::vector<Entry> entries;
    hipGraphExec_t find(const Key& key) const
    {
        for (const Entry& e : entries)
            if (memcmp(&e.key, &key, sizeof key) == 0) return e.exec;
        return nullptr;
    }
    void insert(const Key& key, hipGraphExec_t exec, size_t bound)
    {
        if (entries.size() >= bound) drop();
        entries.push_back({key, exec});
    }
    void drop()
    {
        for (Entry& e : entries)
            if (e.exec) (void)hipGraphExecDestroy(e.exec);
        entries.clear();
    }
};

}  // namespace

struct orbfe_map;
struct orbfe_stream;
struct orbfe_covis;

struct orbfe_handle {
    orbfe_params prm{};
    int device = 0;
    int nLevels = 0;
    double scaleFactorD = 0.0;  // the reference stores scaleFactor as double (ORBextractor.h:108)
    float sf[kMaxLevels]{}, inv[kMaxLevels]{}, sig2[kMaxLevels]{}, invSig2[kMaxLevels]{};
    PipelineDesc P{};
    PipelineDesc* dP = nullptr;
    int maxBatch = 1;
    int maxNodeCap = 0;

    uint8_t* ws = nullptr;          // pyramid + blurred pyramid, all frames
    size_t wsBytes = 0;
    uint32_t* dCand = nullptr;      // [level][frame][candCap]
    uint16_t* dNodeOf = nullptr;
    size_t candWordsPerBatch = 0;
    uint32_t* dCounters = nullptr;  // [frame][level][kCntWords]
    uint32_t* dLvlKp = nullptr;     // [frame][kpCapFrame]
    uint16_t* dTileRows = nullptr;  // [frame][FAST tile][32] pre-NMS corner counts per tile row: low pass | high pass << 8
    uint8_t* dQtScratch = nullptr;  // node tables of the large-N quadtree variant, [level][frame] slabs
    uint32_t* dTabs = nullptr;      // resize tables
    uint32_t* dTileInfo = nullptr;  // FAST tile -> (level, tile column, tile row)
    bool pyrFits[kMaxLevels]{};     // level is produced by the row-streaming pyramid kernel (else: the table-driven tile kernel)
    bool fusedFits[kMaxLevels]{};   // large launches: level is written by the FAST launch of the level below it
    int fusedMinFrames = kFusedPyramidMinFrames;  // launches of at least this many frames take the fused level build (0: none)
    bool fusedSplitOnly = false;    // liborbfe_diag.so: one FAST launch per level behind the pyramid launches (what do the launches cost?)
    float* dSf = nullptr;           // mvScaleFactor on the device (batched matcher)

    // staging for the host-pointer API
    uint8_t* dIn = nullptr;
    int dInPitch = 0;
    uint8_t* hIn = nullptr;         // pinned
    // results of the host-pointer API: ONE device block [n | status | per-level | keypoints | descriptors] with a
    // pinned mirror of the same layout, so a full batch comes back in a single D2H copy
    uint8_t* dOutBlock = nullptr;
    uint8_t* hOutBlock = nullptr;   // pinned
    size_t outBlockBytes = 0, offStatus = 0, offPer = 0, offKp = 0, offDesc = 0;
    orbfe_keypoint* dKp = nullptr;
    uint8_t* dDesc = nullptr;
    int* dN = nullptr;
    int* dStatus = nullptr;
    int* dPer = nullptr;
    orbfe_keypoint* hKp = nullptr;
    uint8_t* hDesc = nullptr;
    int* hN = nullptr;
    int* hStatus = nullptr;
    int* hPer = nullptr;
    // the whole host-API call (H2D, kernel chain, D2H) as a captured hipGraph per batch size (latency path)
    std::map<int, hipGraphExec_t> graphs;
    bool useGraph = true;
    int graphCaptures = 0, captureFailures = 0;  // orbfe_debug_graph_stats (totals since create / the last orbfe_set_graph_capture(1))
    int captureFailStreak = 0;                   // CONSECUTIVE failed captures: a successful one resets it

    hipStream_t stream = nullptr;
    bool timing = false;
    hipEvent_t ev[kEventSets][ORBFE_NUM_STAGES]{};
    int evHead = 0, evCount = 0;

    // last call (for the pyramid / candidate getters)
    const uint8_t* lastGray = nullptr;
    size_t lastStride = 0;
    int lastPitch = 0, lastBatch = 0;

    MatchScratch match;

    // orbfe_track_frame: the fused per-frame chain.  Its captured graphs hold the addresses of these blocks and of this
    // matcher arena, so nothing else uses them and a regrow drops every graph.
    struct TrackKey {
        int Mb, inPitch, gridCols, gridRows, farPoints;
        float minX, minY, invW, invH, th, nnRatio, thFar;
        const void* map;  // null: explicit points in the block; else the resident map the ids refer to (its addresses are in the graph)
    };
    MatchScratch trackMatch;
    // in:  [image | frustum | points (Mb) | descriptors (Mb)]
    // out: [n, status, n_matches | per-level | keypoints | descriptors | match | map-point records (Mb) | xr (Mb)]
    ChainBlocks trk;
    int trkCapM = 0;
    GraphCache<TrackKey> trackGraphs;
    // orbfe_track_reference_keyframe: extract -> vocabulary descent -> SearchByBoW against a resident key frame.  The key
    // frame is named by a record inside the input block, so a graph depends only on what is in RefKey.
    struct RefKey {
        int inPitch, levelsup, checkOri;
        float nnRatio;
        unsigned long long vocabSerial;
    };
    // in:  [image | key-frame record | key-frame flags (refCapFlags)]
    // out: [n, status, n_matches | per-level | keypoints | descriptors | match | (word, node) | leaf | bins]
    ChainBlocks ref;
    int refCapFlags = 0;
    GraphCache<RefKey> refGraphs;
    // orbfe_track_initialization: extract -> SearchForInitialization(resident initial frame, frame).  A graph holds the
    // addresses of the initial frame it was captured for (named by its serial) and of these blocks.
    struct IniKey {
        int inPitch, gridCols, gridRows, window, checkOri;
        float minX, minY, invW, invH, nnRatio;
        unsigned long long frameSerial;
    };
    // in:  [image]
    // out: [n, status, n_matches | per-level | keypoints | descriptors | matches12 (iniCapN1)] + matcher scratch
    ChainBlocks ini;
    int iniCapN1 = -1;
    size_t iniScratchBytes = 0;
    GraphCache<IniKey> iniGraphs;
    // orbfe_track_frame_inertial: extract -> the inertial TrackLocalMap chain with batch == 1 (plain launches, no graph)
    // in:  [image | times | bias | state1 | key-frame record | frame record | prior | samples | ids]
    // out: [n, status | per-level | keypoints | descriptors | the chain's outputs]
    ChainBlocks tin;
    size_t tinInBytes = 0, tinOutBytes = 0;
    std::mutex mu;
    std::string err;
    // objects that keep a pointer to this handle: orbfe_destroy releases their device memory and orphans them (h = null), so
    // that destroying them afterwards -- a binding's finalisers run in any order -- only frees the empty shell
    std::vector<orbfe_map*> maps;
    std::vector<orbfe_stream*> rings;
    std::vector<orbfe_covis*> covis;

    // Cross-stream ordering of the scratch the handle owns: an event recorded behind the last enqueue that used the
    // extraction scratch (pyramid, candidates, counters, level keypoints) / the matcher arena, and the stream it ran on.
    // The next enqueue on a different stream waits for it first; the getters wait for it on the host.
    hipEvent_t evExtract = nullptr, evMatch = nullptr;
    hipStream_t extractStream = nullptr, matchStream = nullptr;
    bool extractUsed = false, matchUsed = false;
};

namespace {

int fail_hip(orbfe_handle* h, hipError_t e, const char* what, int line)
{
    char buf[256];
    snprintf(buf, sizeof buf, "%s failed at orbfe_host.cpp:%d: %s", what, line, hipGetErrorString(e));
    if (h) h->err = buf;
    return ORBFE_ERR_HIP;
}

#define HIPCHK(h, call)                                                   \
    do {                                                                  \
        hipError_t e_ = (call);                                           \
        if (e_ != hipSuccess) return fail_hip((h), e_, #call, __LINE__);  \
    } while (0)

// scratch hand-over between streams (see the handle): call with h->mu held
int scratch_acquire(orbfe_handle* h, bool used, hipStream_t last, hipEvent_t ev, hipStream_t s)
{
    if (used && last != s) HIPCHK(h, hipStreamWaitEvent(s, ev, 0));
    return ORBFE_OK;
}

int extract_scratch_release(orbfe_handle* h, hipStream_t s)
{
    HIPCHK(h, hipEventRecord(h->evExtract, s));
    h->extractStream = s;
    h->extractUsed = true;
    return ORBFE_OK;
}

// RAII pair around a matcher launch: waits for the arena's previous user on another stream, records behind this one
struct MatchScope {
    orbfe_handle* h;
    hipStream_t s;
    int rc;
    MatchScope(orbfe_handle* h_, hipStream_t s_) : h(h_), s(s_), rc(scratch_acquire(h_, h_->matchUsed, h_->matchStream, h_->evMatch, s_)) {}
    ~MatchScope()
    {
        if (hipEventRecord(h->evMatch, s) == hipSuccess) {
            h->matchStream = s;
            h->matchUsed = true;
        }
    }
};

// What an entry point does once its arguments stand, with h->mu held: the device, the stream (null: the handle's), the scratch
// hand-over, then run(s, err); a failure's text, empty or not, becomes the handle's last error.
template <class Run>
int match_call_locked(orbfe_handle* h, hipStream_t s, Run run)
{
    HIPCHK(h, hipSetDevice(h->device));
    if (!s) s = h->stream;
    MatchScope scope_(h, s);
    if (scope_.rc != ORBFE_OK) return scope_.rc;
    std::string err;
    const int rc = run(s, err);
    if (rc != ORBFE_OK) h->err = err;
    return rc;
}

template <class Run>
int match_call(orbfe_handle* h, hipStream_t s, Run run)
{
    std::lock_guard<std::mutex> lk(h->mu);
    return match_call_locked(h, s, run);
}

// A refusal in front of the lock that may carry text (h may be null).  The sites do not agree on a refusal without text, and each keeps
// its rule: the solvers' *_batch_device (S14, S19, S20) replace the last error with the empty string (kReplace), the S22 / S23 calls
// keep the older text (kKeep); so do the matchers, which return such refusals without coming here.
enum RefuseText { kKeep, kReplace };
int refuse(orbfe_handle* h, int rc, const std::string& err, RefuseText empty)
{
    if (h && (empty == kReplace || !err.empty())) {
        std::lock_guard<std::mutex> lk(h->mu);
        h->err = err;
    }
    return rc;
}

int cv_round_f(float v) { return (int)lrintf(v); }

// resize tables of SPEC DECISION S1: entry = x1 | (Q11 weight << 16)
void fill_resize_table(std::vector<uint32_t>& t, size_t off, int srcN, int dstN)
{
    for (int x = 0; x < dstN; x++) {
        const int64_t sx = (int64_t)x * srcN;
        const int x1 = (int)(sx / dstN);
        const int fx = (int)(sx % dstN);
        const int wx = (int)(((int64_t)fx * 2048 + dstN / 2) / dstN);
        t[off + x] = (uint32_t)x1 | ((uint32_t)wx << 16);
    }
    // the kernel evaluates whole groups of four: pad with the last entry (its results are never stored)
    for (size_t x = (size_t)dstN; x < align_up((size_t)dstN, 4); x++) t[off + x] = t[off + dstN - 1];
}

// The caller holds h->mu (or is the handle's destruction), nothing that uses the blocks is in flight, and the graphs that
// hold their addresses have been dropped.
void chain_blocks_free(orbfe_handle* h, ChainBlocks& b)
{
    // the getters read level 0 of the last call through lastGray: forget a frame that lives in the block that goes away
    // (they refuse frame >= lastBatch), whatever becomes of the call that is regrowing it
    if (b.dIn && h->lastGray == b.dIn) {
        h->lastGray = nullptr;
        h->lastStride = 0;
        h->lastPitch = h->lastBatch = 0;
    }
    if (b.dIn) (void)hipFree(b.dIn);
    if (b.dOut) (void)hipFree(b.dOut);
    if (b.hIn) (void)hipHostFree(b.hIn);
    if (b.hOut) (void)hipHostFree(b.hOut);
    b = ChainBlocks{};
}

// replaces the blocks by new ones of these sizes (only part of the result block is ever downloaded: hostOutBytes <= devOutBytes)
int chain_blocks_alloc(orbfe_handle* h, ChainBlocks& b, size_t inBytes, size_t devOutBytes, size_t hostOutBytes, const char* who)
{
    chain_blocks_free(h, b);
    if (hipMalloc(&b.dIn, inBytes) != hipSuccess || hipMalloc(&b.dOut, devOutBytes) != hipSuccess ||
        hipHostMalloc(&b.hIn, inBytes) != hipSuccess || hipHostMalloc(&b.hOut, hostOutBytes) != hipSuccess) {
        (void)hipGetLastError();
        chain_blocks_free(h, b);
        h->err = std::string(who) + ": allocation of the staging blocks failed";
        return ORBFE_ERR_OUT_OF_MEMORY;
    }
    return ORBFE_OK;
}

void orphan_children(orbfe_handle* h);  // defined behind orbfe_map / orbfe_stream

void destroy_impl(orbfe_handle* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    orphan_children(h);
    for (auto& set : h->ev)
        for (auto& e : set)
            if (e) (void)hipEventDestroy(e);
    if (h->evExtract) (void)hipEventDestroy(h->evExtract);
    if (h->evMatch) (void)hipEventDestroy(h->evMatch);
    h->match.busy = nullptr;
    match_scratch_free(h->match);
    h->trackGraphs.drop();
    match_scratch_free(h->trackMatch);
    h->refGraphs.drop();
    h->iniGraphs.drop();
    for (ChainBlocks* b : {&h->ini, &h->ref, &h->trk, &h->tin}) chain_blocks_free(h, *b);
    for (auto& g : h->graphs)
        if (g.second) (void)hipGraphExecDestroy(g.second);
    void* dptrs[] = {h->dP, h->ws, h->dCand, h->dNodeOf, h->dCounters, h->dLvlKp, h->dTileRows, h->dQtScratch, h->dTabs,
                     h->dTileInfo, h->dSf, h->dIn, h->dOutBlock};
    for (void* p : dptrs)
        if (p) (void)hipFree(p);
    void* hptrs[] = {h->hIn, h->hOutBlock};
    for (void* p : hptrs)
        if (p) (void)hipHostFree(p);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

}  // namespace

extern "C" {

const char* orbfe_version(void) { return "orbfe 0.1 (gfx950, HIP)"; }

const char* orbfe_status_string(int s)
{
    switch (s) {
    case ORBFE_OK: return "ok";
    case ORBFE_ERR_INVALID_ARG: return "invalid argument";
    case ORBFE_ERR_UNSUPPORTED: return "unsupported configuration";
    case ORBFE_ERR_NO_DEVICE: return "no usable gfx950 device";
    case ORBFE_ERR_HIP: return "HIP runtime error";
    case ORBFE_ERR_OUT_OF_MEMORY: return "out of memory";
    case ORBFE_ERR_INTERNAL: return "internal device-side guard tripped";
    case ORBFE_ERR_BUSY: return "every slot of the stream ring is in flight";
    default: return "unknown status";
    }
}

const char* orbfe_last_error(const orbfe_handle* h) { return h ? h->err.c_str() : ""; }
const char* orbfe_stage_name(int s) { return (s >= 0 && s < ORBFE_NUM_STAGES) ? kStageNames[s] : ""; }

int orbfe_create(const orbfe_params* p, orbfe_handle** out)
{
    if (!p || !out) return ORBFE_ERR_INVALID_ARG;
    *out = nullptr;
    if (p->n_levels < 1 || p->n_levels > kMaxLevels || p->image_width < 16 || p->image_height < 16 ||
        p->n_features < 0 || p->n_fast_features < 1 || p->max_batch < 1 || !(p->scale_factor > 1.0f))
        return ORBFE_ERR_INVALID_ARG;
    // one fused FAST pass serves both thresholds only when iniThFAST >= minThFAST >= 1
    if (p->min_th_fast < 1 || p->ini_th_fast < p->min_th_fast || p->ini_th_fast > 254)
        return ORBFE_ERR_UNSUPPORTED;
    if (p->image_width > (int)kCoordMask || p->image_height > (int)kCoordMask) return ORBFE_ERR_UNSUPPORTED;

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || p->device_id < 0 || p->device_id >= ndev)
        return ORBFE_ERR_NO_DEVICE;
    if (hipSetDevice(p->device_id) != hipSuccess) return ORBFE_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, p->device_id) != hipSuccess) return ORBFE_ERR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return ORBFE_ERR_NO_DEVICE;  // code object is gfx950 only

    orbfe_handle* h = new (std::nothrow) orbfe_handle();
    if (!h) return ORBFE_ERR_OUT_OF_MEMORY;
    h->prm = *p;
    h->device = p->device_id;
    h->nLevels = p->n_levels;
    h->maxBatch = p->max_batch;
    const int nL = p->n_levels;

    // ---- scale tables, src/ORBextractor.cc:92-108 ----
    h->scaleFactorD = p->scale_factor;
    h->sf[0] = 1.0f;
    h->sig2[0] = 1.0f;
    for (int i = 1; i < nL; i++) {
        h->sf[i] = (float)(h->sf[i - 1] * h->scaleFactorD);
        h->sig2[i] = h->sf[i] * h->sf[i];
    }
    for (int i = 0; i < nL; i++) {
        h->inv[i] = 1.0f / h->sf[i];
        h->invSig2[i] = 1.0f / h->sig2[i];
    }
    // ---- features per level, :112-124 ----
    int fpl[kMaxLevels];
    {
        const float factor = (float)(1.0f / h->scaleFactorD);
        float nDesired = (float)p->n_features * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nL));
        int sum = 0;
        for (int l = 0; l < nL - 1; l++) {
            fpl[l] = cv_round_f(nDesired);
            sum += fpl[l];
            nDesired *= factor;
        }
        fpl[nL - 1] = std::max(p->n_features - sum, 0);
    }

    // ---- level geometry (AllocatePyramid :587-605) + workspace layout ----
    PipelineDesc& P = h->P;
    memset(&P, 0, sizeof P);
    P.nLevels = nL;
    P.nFast = p->n_fast_features;
    P.iniTh = p->ini_th_fast;
    P.minTh = p->min_th_fast;
    size_t wsOff = 0, candOff = 0, tabOff = 0;
    int tileBase = 0, kpBase = 0;
    const size_t B = (size_t)p->max_batch;
    int status = ORBFE_OK;
    for (int l = 0; l < nL; l++) {
        LevelDesc& L = P.lv[l];
        if (l == 0) {
            L.w = p->image_width;
            L.h = p->image_height;
        } else {
            L.w = cv_round_f(h->inv[l] * (float)p->image_width);
            L.h = cv_round_f(h->inv[l] * (float)p->image_height);
        }
        if (L.w < 16 || L.h < 16) { status = ORBFE_ERR_UNSUPPORTED; break; }
        L.pitch = (int)align_up((size_t)L.w, kPitchAlign);
        L.nFeatures = fpl[l];
        L.nIni = (int)roundf((float)L.w / (float)L.h);  // :231
        if (L.nIni < 1) { status = ORBFE_ERR_UNSUPPORTED; break; }  // the reference divides by zero here
        L.hX = (float)L.w / (float)L.nIni;                // :233
        L.nodeCap = std::max(L.nFeatures + 3, 4 * L.nIni);
        L.candCap = ((L.w + 1) / 2) * ((L.h + 1) / 2);
        fast_tiles_for(L.w, L.h, &L.tilesX, &L.tilesY);
        L.tileBase = tileBase;
        tileBase += L.tilesX * L.tilesY;
        L.kpBase = kpBase;
        kpBase += L.nodeCap;
        L.invScale = h->inv[l];
        L.scaledPatch = (int)(kPatch * h->inv[l]);         // :511
        const size_t frameBytes = align_up((size_t)L.pitch * L.h, 256);
        L.imgFrameStride = frameBytes;
        L.blurFrameStride = frameBytes;
        if (l > 0) {
            L.imgOff = wsOff;
            wsOff += frameBytes * B;
        }
        L.blurOff = wsOff;
        wsOff += frameBytes * B;
        L.candOff = candOff;
        candOff += (size_t)L.candCap * B;
        tabOff = align_up(tabOff, 4);  // uint4 table loads in resize_kernel
        L.xtabOff = tabOff;
        tabOff += align_up((size_t)L.w, 4);
        L.ytabOff = tabOff;
        tabOff += align_up((size_t)L.h, 4);
        tabOff = align_up(tabOff, 4);
        L.ownOff = (uint32_t)tabOff;  // ownership tables of the fused level build (filled below)
        tabOff += (size_t)L.tilesX + L.tilesY + 2;
        h->maxNodeCap = std::max(h->maxNodeCap, L.nodeCap);
    }
    if (status == ORBFE_OK && quadtree_node_capacity(h->maxNodeCap) == 0) status = ORBFE_ERR_UNSUPPORTED;  // > 65535 nodes/level
    if (status != ORBFE_OK) {
        delete h;
        return status;
    }
    P.kpCapFrame = kpBase;
    P.totalTiles = tileBase;
    for (int l = 0; l < 8; l++) P.tileBaseTab[l] = l < nL ? P.lv[l].tileBase : 0x7fffffff;
    h->wsBytes = wsOff;
    h->candWordsPerBatch = candOff;

    std::vector<uint32_t> tabs(tabOff ? tabOff : 1, 0);
    for (int l = 1; l < nL; l++) {
        fill_resize_table(tabs, P.lv[l].xtabOff, P.lv[l - 1].w, P.lv[l].w);
        fill_resize_table(tabs, P.lv[l].ytabOff, P.lv[l - 1].h, P.lv[l].h);
    }

    for (int l = 1; l < nL; l++)
        if (pyramid_level_fits(tabs.data() + P.lv[l].xtabOff, tabs.data() + P.lv[l].ytabOff, P.lv[l - 1].w, P.lv[l - 1].h, P.lv[l].w,
                               P.lv[l].h))
            h->pyrFits[l] = true;
    // the fused build takes the levels the row-streaming kernel takes (no clamped far tap) whose tiles own at most 64 columns
    for (int l = 1; l < nL; l++)
        h->fusedFits[l] = fast_next_level_fits(tabs.data() + P.lv[l].xtabOff, tabs.data() + P.lv[l].ytabOff, P.lv[l - 1].w, P.lv[l - 1].h,
                                               P.lv[l].w, P.lv[l].h, tabs.data() + P.lv[l - 1].ownOff) && h->pyrFits[l];

#define CREATE_CHK(call)                                                  \
    do {                                                                  \
        hipError_t e_ = (call);                                           \
        if (e_ != hipSuccess) {                                           \
            int rc_ = e_ == hipErrorOutOfMemory ? ORBFE_ERR_OUT_OF_MEMORY : ORBFE_ERR_HIP; \
            destroy_impl(h);                                              \
            return rc_;                                                   \
        }                                                                 \
    } while (0)

    CREATE_CHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    CREATE_CHK(hipMalloc(&h->dP, sizeof(PipelineDesc)));
    CREATE_CHK(hipMalloc(&h->ws, h->wsBytes + 256));  // + slack: the pyramid kernel's 12-byte row windows may end past a level's last row
    CREATE_CHK(hipMalloc(&h->dCand, candOff * sizeof(uint32_t)));
    CREATE_CHK(hipMalloc(&h->dNodeOf, candOff * sizeof(uint16_t)));
    CREATE_CHK(hipMalloc(&h->dCounters, B * nL * kCntWords * sizeof(uint32_t)));
    CREATE_CHK(hipMalloc(&h->dLvlKp, B * (size_t)P.kpCapFrame * sizeof(uint32_t)));
    CREATE_CHK(hipMalloc(&h->dTileRows, B * (size_t)P.totalTiles * 32 * sizeof(uint16_t)));
    if (quadtree_scratch_bytes_per_block(h->maxNodeCap))
        CREATE_CHK(hipMalloc(&h->dQtScratch, quadtree_scratch_bytes_per_block(h->maxNodeCap) * B * nL));
    CREATE_CHK(hipMalloc(&h->dTabs, tabs.size() * sizeof(uint32_t)));
    {
        std::vector<uint32_t> info((size_t)P.totalTiles);
        for (int l = 0; l < nL; l++)
            for (int ty = 0; ty < P.lv[l].tilesY; ty++)
                for (int tx = 0; tx < P.lv[l].tilesX; tx++) info[P.lv[l].tileBase + ty * P.lv[l].tilesX + tx] = fast_tile_info(l, tx, ty);
        CREATE_CHK(hipMalloc(&h->dTileInfo, info.size() * sizeof(uint32_t)));
        CREATE_CHK(copy_sync(h->dTileInfo, info.data(), info.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    }
    CREATE_CHK(hipMalloc(&h->dSf, kMaxLevels * sizeof(float)));
    CREATE_CHK(copy_sync(h->dSf, h->sf, kMaxLevels * sizeof(float), hipMemcpyHostToDevice, h->stream));
    CREATE_CHK(copy_sync(h->dP, &P, sizeof P, hipMemcpyHostToDevice, h->stream));
    CREATE_CHK(copy_sync(h->dTabs, tabs.data(), tabs.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));

    // staging for the host-pointer entry points
    h->dInPitch = (int)align_up((size_t)p->image_width, kPitchAlign);
    const size_t inFrame = (size_t)h->dInPitch * p->image_height;
    const size_t cap = (size_t)P.kpCapFrame;
    CREATE_CHK(hipMalloc(&h->dIn, inFrame * B));
    CREATE_CHK(hipHostMalloc(&h->hIn, inFrame * B));
    {
        size_t off = 0;
        auto take = [&](size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; };
        take(B * sizeof(int));  // n at offset 0
        h->offStatus = take(B * sizeof(int));
        h->offPer = take(B * nL * sizeof(int));
        h->offKp = take(B * cap * sizeof(orbfe_keypoint));
        h->offDesc = take(B * cap * ORBFE_DESC_BYTES);
        h->outBlockBytes = off;
    }
    CREATE_CHK(hipMalloc(&h->dOutBlock, h->outBlockBytes));
    CREATE_CHK(hipHostMalloc(&h->hOutBlock, h->outBlockBytes));
    h->dN = reinterpret_cast<int*>(h->dOutBlock);
    h->dStatus = reinterpret_cast<int*>(h->dOutBlock + h->offStatus);
    h->dPer = reinterpret_cast<int*>(h->dOutBlock + h->offPer);
    h->dKp = reinterpret_cast<orbfe_keypoint*>(h->dOutBlock + h->offKp);
    h->dDesc = h->dOutBlock + h->offDesc;
    h->hN = reinterpret_cast<int*>(h->hOutBlock);
    h->hStatus = reinterpret_cast<int*>(h->hOutBlock + h->offStatus);
    h->hPer = reinterpret_cast<int*>(h->hOutBlock + h->offPer);
    h->hKp = reinterpret_cast<orbfe_keypoint*>(h->hOutBlock + h->offKp);
    h->hDesc = h->hOutBlock + h->offDesc;
#ifdef ORBFE_DIAG
    h->useGraph = getenv("ORBFE_NO_GRAPH") == nullptr;  // liborbfe_diag.so only: plain launches, e.g. under a debugger
    // liborbfe_diag.so only: ORBFE_FUSED_PYRAMID=1 forces the fused level build on every launch, =0 never takes it, =2 keeps
    // the pyramid launches and only splits FAST into one launch per level (timing experiment)
    if (const char* e = getenv("ORBFE_FUSED_PYRAMID")) {
        h->fusedMinFrames = atoi(e) ? 1 : 0;
        h->fusedSplitOnly = atoi(e) == 2;
    }
#endif
    CREATE_CHK(hipEventCreateWithFlags(&h->evExtract, hipEventDisableTiming));
    CREATE_CHK(hipEventCreateWithFlags(&h->evMatch, hipEventDisableTiming));
    h->match.busy = h->evMatch;  // the arena is not regrown while a launch still uses it
    for (auto& set : h->ev)
        for (auto& e : set) CREATE_CHK(hipEventCreate(&e));
#undef CREATE_CHK
    *out = h;
    return ORBFE_OK;
}

void orbfe_destroy(orbfe_handle* h) { destroy_impl(h); }

int orbfe_get_levels(const orbfe_handle* h) { return h ? h->nLevels : 0; }
float orbfe_get_scale_factor(const orbfe_handle* h) { return h ? (float)h->scaleFactorD : 0.f; }

int orbfe_get_scale_tables(const orbfe_handle* h, float* sf, float* inv, float* s2, float* is2)
{
    if (!h) return ORBFE_ERR_INVALID_ARG;
    for (int i = 0; i < h->nLevels; i++) {
        if (sf) sf[i] = h->sf[i];
        if (inv) inv[i] = h->inv[i];
        if (s2) s2[i] = h->sig2[i];
        if (is2) is2[i] = h->invSig2[i];
    }
    return ORBFE_OK;
}

int orbfe_get_level_info(const orbfe_handle* h, int* fpl, int* lw, int* lh)
{
    if (!h) return ORBFE_ERR_INVALID_ARG;
    for (int i = 0; i < h->nLevels; i++) {
        if (fpl) fpl[i] = h->P.lv[i].nFeatures;
        if (lw) lw[i] = h->P.lv[i].w;
        if (lh) lh[i] = h->P.lv[i].h;
    }
    return ORBFE_OK;
}

int orbfe_max_keypoints(const orbfe_handle* h) { return h ? h->P.kpCapFrame : 0; }

int orbfe_set_stage_timing(orbfe_handle* h, int enabled)
{
    if (!h) return ORBFE_ERR_INVALID_ARG;
    h->timing = enabled != 0;
    h->evHead = h->evCount = 0;
    return ORBFE_OK;
}

int orbfe_get_stage_ms(orbfe_handle* h, float ms[ORBFE_NUM_STAGES], int* n_calls)
{
    if (!h || !ms || !n_calls) return ORBFE_ERR_INVALID_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    for (int s = 0; s < ORBFE_NUM_STAGES; s++) ms[s] = 0.f;
    const int n = h->evCount < kEventSets ? h->evCount : kEventSets;
    for (int i = 0; i < n; i++) {
        hipEvent_t* e = h->ev[i];
        HIPCHK(h, hipEventSynchronize(e[ORBFE_NUM_STAGES - 1]));
        for (int s = 0; s + 1 < ORBFE_NUM_STAGES; s++) {
            float t = 0.f;
            HIPCHK(h, hipEventElapsedTime(&t, e[s], e[s + 1]));
            ms[s] += t;
        }
        float t = 0.f;
        HIPCHK(h, hipEventElapsedTime(&t, e[0], e[ORBFE_NUM_STAGES - 1]));
        ms[ORBFE_NUM_STAGES - 1] += t;
    }
    *n_calls = n;
    return ORBFE_OK;
}

static int extract_chain(orbfe_handle* h, const uint8_t* d_gray, size_t frame_stride, int pitch, int batch,
                         orbfe_keypoint* d_kp, uint8_t* d_desc, int* d_n, int* d_per, int* d_status, void* stream_);

int orbfe_extract_batch_device(orbfe_handle* h, const uint8_t* d_gray, size_t frame_stride, int pitch,
                               int batch, orbfe_keypoint* d_kp, uint8_t* d_desc, int* d_n, int* d_per,
                               void* stream_)
{
    if (!h) return ORBFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    return extract_chain(h, d_gray, frame_stride, pitch, batch, d_kp, d_desc, d_n, d_per, nullptr, stream_);
}

}  // extern "C"

static int extract_chain(orbfe_handle* h, const uint8_t* d_gray, size_t frame_stride, int pitch, int batch,
                         orbfe_keypoint* d_kp, uint8_t* d_desc, int* d_n, int* d_per, int* d_status, void* stream_)
{
    if (!h || !d_gray || !d_kp || !d_desc || !d_n) return ORBFE_ERR_INVALID_ARG;
    if (batch < 1 || batch > h->maxBatch || pitch < h->prm.image_width || pitch >= (1 << 24)) return ORBFE_ERR_INVALID_ARG;
    const int aligned4 = ((reinterpret_cast<uintptr_t>(d_gray) | (uintptr_t)pitch | (uintptr_t)frame_stride) & 3u) == 0;
    // frame extent the kernels read (orbfe.h, input contract): whole dwords on the aligned path
    const size_t rowEnd = aligned4 ? (size_t)((h->prm.image_width + 3) & ~3) : (size_t)h->prm.image_width;
    if (batch > 1 && frame_stride < (size_t)pitch * (h->prm.image_height - 1) + rowEnd) return ORBFE_ERR_INVALID_ARG;
    // the kernels address a frame with 32-bit byte offsets and send dropped lanes to offset 0x7ffffff0 of a buffer
    // descriptor: a frame must end below that (480 rows at an 8 MiB pitch would wrap the row offsets)
    if ((size_t)pitch * (h->prm.image_height - 1) + (size_t)((h->prm.image_width + 3) & ~3) >= (size_t)0x7ffffff0u)
        return ORBFE_ERR_INVALID_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = stream_ ? (hipStream_t)stream_ : h->stream;
    // while the chain is being captured into a hipGraph the hand-over events stay outside it: the replay path waits
    // and records around hipGraphLaunch
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &capturing) != hipSuccess) (void)hipGetLastError();
    if (capturing == hipStreamCaptureStatusNone) {
        const int rc = scratch_acquire(h, h->extractUsed, h->extractStream, h->evExtract, s);
        if (rc != ORBFE_OK) return rc;
    }
    const PipelineDesc& P = h->P;
    const int nL = P.nLevels;
    hipEvent_t* ev = nullptr;
    if (h->timing) {
        ev = h->ev[h->evHead];
        h->evHead = (h->evHead + 1) % kEventSets;
        h->evCount++;
    }
    // fused level build: no pyramid launches, one FAST launch per level that also writes the next level (kernels_fast.hip)
    const bool fused = h->fusedMinFrames > 0 && batch >= h->fusedMinFrames && nL > 1;
    const bool chainPyr = !fused && (long long)batch * nL <= 64 && !ev && nL > 1;  // one to eight frames: see below
    if (!chainPyr) HIPCHK(h, hipMemsetAsync(h->dCounters, 0, (size_t)batch * nL * kCntWords * sizeof(uint32_t), s));
    if (ev) HIPCHK(h, hipEventRecord(ev[0], s));
    // ComputePyramid (:607-623): level l from the UNBLURRED level l-1
    // (one to eight frames: two or three levels per launch -- a dependent launch costs more than the small levels' work)
    for (int l = 1; chainPyr && l < nL;) {
        const int left = nL - l;
        const int depth = left >= 5 ? 2 : std::min(left, 3);  // 7 levels to build: 2 + 2 + 3
        launch_pyramid_chain(s, batch, h->dP, P, l - 1, depth, d_gray, frame_stride, pitch, h->ws, h->dTabs,
                             l == 1 ? h->dCounters : nullptr, nL * kCntWords);  // the first launch clears the level counters
        l += depth;
    }
    auto pyramid_level = [&](int l) {
        const LevelDesc& S = P.lv[l - 1];
        const LevelDesc& D = P.lv[l];
        if (h->pyrFits[l] && (l > 1 || aligned4)) {
            launch_pyramid_level(s, batch, h->dP, l, D.w, D.h, d_gray, frame_stride, pitch, h->ws, h->dTabs);
            return;
        }
        const uint8_t* src = l == 1 ? d_gray : h->ws + S.imgOff;
        const size_t sstride = l == 1 ? frame_stride : S.imgFrameStride;
        const int spitch = l == 1 ? pitch : S.pitch;
        launch_resize(s, batch, src, sstride, S.w, S.h, spitch, l == 1 ? aligned4 : 1, h->ws + D.imgOff, D.imgFrameStride, D.w, D.h,
                      D.pitch, h->dTabs + D.xtabOff, h->dTabs + D.ytabOff);
    };
    for (int l = chainPyr || (fused && !h->fusedSplitOnly) ? nL : 1; l < nL; l++) pyramid_level(l);
    if (ev) HIPCHK(h, hipEventRecord(ev[1], s));  // fused: nothing in front of it, the FAST stage covers the level build
    if (fused) {
        for (int l = 0; l < nL; l++) {
            const bool build = l + 1 < nL && h->fusedFits[l + 1] && !h->fusedSplitOnly;
            launch_fast_blur(s, batch, P.lv[l].tileBase, P.lv[l].tilesX * P.lv[l].tilesY, build, h->dP, h->dTileInfo, h->dTabs, d_gray,
                             frame_stride, pitch, aligned4, h->ws, h->dCand, h->dCounters, h->dTileRows);
            if (l + 1 < nL && !build && !h->fusedSplitOnly) pyramid_level(l + 1);  // a level the tiles cannot build: its own launch, from level l
        }
    } else {
        launch_fast_blur(s, batch, 0, P.totalTiles, false, h->dP, h->dTileInfo, h->dTabs, d_gray, frame_stride, pitch, aligned4, h->ws,
                         h->dCand, h->dCounters, h->dTileRows);
    }
    if (ev) HIPCHK(h, hipEventRecord(ev[2], s));
    launch_quadtree(s, batch, nL, h->maxNodeCap, h->dP, h->dCand, h->dNodeOf, h->dCounters, h->dLvlKp, d_gray, frame_stride,
                    pitch, h->ws, h->dTileRows, h->dQtScratch);
    if (ev) HIPCHK(h, hipEventRecord(ev[3], s));
    int kpBase[kMaxLevels];
    for (int l = 0; l < nL; l++) kpBase[l] = P.lv[l].kpBase;
    launch_orient_brief(s, batch, P.kpCapFrame, h->dP, d_gray, frame_stride, pitch, h->ws, h->dCounters, h->dLvlKp,
                        d_kp, d_desc, d_n, d_per, d_status, kpBase, nL);
    if (ev) HIPCHK(h, hipEventRecord(ev[4], s));
    HIPCHK(h, hipGetLastError());
    h->lastGray = d_gray;
    h->lastStride = frame_stride;
    h->lastPitch = pitch;
    h->lastBatch = batch;
    if (capturing == hipStreamCaptureStatusNone) return extract_scratch_release(h, s);
    return ORBFE_OK;
}

extern "C" {

static int check_device_flags(orbfe_handle* h, int batch)
{
    // caller has synchronised the stream; hStatus holds the OR of the per-level guard flags of every frame
    for (int b = 0; b < batch; b++)
        if (h->hStatus[b]) {
            char buf[128];
            snprintf(buf, sizeof buf, "device guard flags 0x%x at frame %d", (unsigned)h->hStatus[b], b);
            h->err = buf;
            return ORBFE_ERR_INTERNAL;
        }
    return ORBFE_OK;
}

// kernel chain on the frames already sent to dIn, D2H of the result block (one copy for a full batch)
static int extract_host_enqueue(orbfe_handle* h, int batch, int inPitch, hipStream_t s)
{
    const int nL = h->nLevels;
    const size_t inFrame = (size_t)h->dInPitch * h->prm.image_height;
    const size_t cap = (size_t)h->P.kpCapFrame;
    const int rc = extract_chain(h, h->dIn, inFrame, inPitch, batch, h->dKp, h->dDesc, h->dN, h->dPer, h->dStatus, s);
    if (rc != ORBFE_OK) return rc;
    if (batch == h->maxBatch) {
        HIPCHK(h, hipMemcpyAsync(h->hOutBlock, h->dOutBlock, h->outBlockBytes, hipMemcpyDeviceToHost, s));
    } else {
        HIPCHK(h, hipMemcpyAsync(h->hN, h->dN, batch * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipMemcpyAsync(h->hStatus, h->dStatus, batch * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipMemcpyAsync(h->hPer, h->dPer, (size_t)batch * nL * sizeof(int), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipMemcpyAsync(h->hKp, h->dKp, batch * cap * sizeof(orbfe_keypoint), hipMemcpyDeviceToHost, s));
        HIPCHK(h, hipMemcpyAsync(h->hDesc, h->dDesc, batch * cap * ORBFE_DESC_BYTES, hipMemcpyDeviceToHost, s));
    }
    return ORBFE_OK;
}

}  // extern "C"

namespace {

// Graphs are captured on a THROW-AWAY stream, never on the handle's (or a caller's) own.  On this runtime (ROCm 7.2) a
// NULL-stream operation of any other thread of the process -- a plain hipMemcpy of the application -- that meets a capture in
// flight fails with hipErrorStreamCaptureImplicit AND leaves the capturing stream unusable for good, whatever the capture mode
// and although the stream is non-blocking (tools/probes/capture_invalidate.cpp): every later call on it returns
// hipErrorStreamCaptureInvalidated.  With a throw-away stream such an encounter costs the call that was capturing its graph,
// not the handle: the stream is destroyed, the call runs on plain launches, a later call captures again.  Only a handle
// whose captures fail eight times IN A ROW stops trying (a success resets the count).  (The library itself makes no NULL-stream call: copy_sync / memset_sync.)
struct CaptureStream {
    hipStream_t s = nullptr;
    bool capturing = false;
    bool begin()
    {
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
            s = nullptr;
            (void)hipGetLastError();
            return false;
        }
        if (hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        capturing = true;
        return true;
    }
    // the captured graph, or null if the capture did not survive
    hipGraph_t end()
    {
        hipGraph_t g = nullptr;
        if (capturing) {
            capturing = false;
            if (hipStreamEndCapture(s, &g) != hipSuccess) {
                (void)hipGetLastError();
                if (g) (void)hipGraphDestroy(g);
                g = nullptr;
            }
        }
        return g;
    }
    ~CaptureStream()
    {
        if (capturing) {
            hipGraph_t g = end();
            if (g) (void)hipGraphDestroy(g);
        }
        if (s) (void)hipStreamDestroy(s);
        (void)hipGetLastError();
    }
};

void graph_capture_failed(orbfe_handle* h)
{
    (void)hipGetLastError();
    h->captureFailures++;
    if (++h->captureFailStreak >= 8) h->useGraph = false;  // eight in a row: this handle's captures keep failing
}

void graph_capture_succeeded(orbfe_handle* h)
{
    h->graphCaptures++;
    h->captureFailStreak = 0;  // an occasional foreign NULL-stream call over a long run never adds up to the limit
}

// One capture attempt: enqueue(stream) -> status, captured on a throw-away stream and instantiated.  Null when any step
// failed; the caller then runs the same enqueue on plain launches, which returns the real error if the enqueue itself is
// what failed.
template <class Enqueue>
hipGraphExec_t capture_graph(orbfe_handle* h, Enqueue& enqueue)
{
    int rc;
    hipGraph_t graph = nullptr;
    {
        CaptureStream cs;
        rc = cs.begin() ? enqueue(cs.s) : ORBFE_ERR_HIP;
        graph = cs.end();
    }
    hipGraphExec_t exec = nullptr;
    if (rc == ORBFE_OK && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) exec = nullptr;
    if (graph) (void)hipGraphDestroy(graph);
    if (exec)
        graph_capture_succeeded(h);
    else
        graph_capture_failed(h);
    return exec;
}

// Replay on s.  While a chain is captured the hand-over events stay outside the graph (extract_chain), so the wait and
// the record go around the launch here, and so does what extract_chain records for the pyramid / candidate getters.
int launch_graph(orbfe_handle* h, hipGraphExec_t exec, hipStream_t s, const uint8_t* dGray, size_t stride, int pitch, int batch)
{
    int rc = scratch_acquire(h, h->extractUsed, h->extractStream, h->evExtract, s);
    if (rc != ORBFE_OK) return rc;
    HIPCHK(h, hipGraphLaunch(exec, s));
    rc = extract_scratch_release(h, s);
    if (rc != ORBFE_OK) return rc;
    h->lastGray = dGray;
    h->lastStride = stride;
    h->lastPitch = pitch;
    h->lastBatch = batch;
    return ORBFE_OK;
}

// extract_host_enqueue, replayed from a hipGraph when possible: every pointer behind the upload is owned by the
// handle, so the enqueue sequence (the kernels of extract_chain, result copy) is captured once per (batch, input pitch) and
// replayed with a single hipGraphLaunch
int extract_enqueue_replay(orbfe_handle* h, int batch, int inPitch, hipStream_t s)
{
    auto enqueue = [&](hipStream_t q) { return extract_host_enqueue(h, batch, inPitch, q); };
    hipGraphExec_t exec = nullptr;
    if (h->useGraph && !h->timing && batch < 4096) {  // batch <= 4095 frames per call in graph mode, else plain launches
        const int gkey = batch | (inPitch << 12);
        const auto it = h->graphs.find(gkey);
        if (it != h->graphs.end())
            exec = it->second;
        else if ((exec = capture_graph(h, enqueue)))
            h->graphs[gkey] = exec;
    }
    if (!exec) return enqueue(s);
    return launch_graph(h, exec, s, h->dIn, (size_t)h->dInPitch * h->prm.image_height, inPitch, batch);
}

// Single-frame upload into blk.dIn, with [smallBegin, smallEnd) of blk.hIn -- what the chain staged behind the frame, or
// nothing -- going up too.  Pinned sources (the reference hands over cv::cuda::HostMem, include/ORBextractor.h:62) with a
// dword-aligned pitch that fits the staging rows are copied by the DMA engine straight from the caller's buffer, followed
// by the small range; everything else goes through the pinned mirror, where frame and small range are ONE copy.
// *inPitch: the pitch of the frame as it lies in blk.dIn.
int upload_frame(orbfe_handle* h, const ChainBlocks& blk, const uint8_t* gray, int pitch, size_t smallBegin, size_t smallEnd,
                 hipStream_t s, int* inPitch)
{
    const int W = h->prm.image_width, H = h->prm.image_height;
    const bool keepPitch = pitch <= h->dInPitch && (pitch & 3) == 0;  // level 0 is read with an arbitrary dword-aligned pitch
    bool direct = keepPitch && (reinterpret_cast<uintptr_t>(gray) & 3u) == 0;
    if (direct) {
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, gray) != hipSuccess || attr.type != hipMemoryTypeHost) {
            (void)hipGetLastError();
            direct = false;
        }
    }
    *inPitch = keepPitch ? pitch : h->dInPitch;
    const size_t frameBytes = (size_t)*inPitch * (H - 1) + (size_t)W;
    if (direct) {
        HIPCHK(h, hipMemcpyAsync(blk.dIn, gray, frameBytes, hipMemcpyHostToDevice, s));
        if (smallEnd > smallBegin)
            HIPCHK(h, hipMemcpyAsync(blk.dIn + smallBegin, blk.hIn + smallBegin, smallEnd - smallBegin, hipMemcpyHostToDevice, s));
        return ORBFE_OK;
    }
    if (keepPitch)  // the frame is one contiguous copy
        memcpy(blk.hIn, gray, frameBytes);
    else
        for (int y = 0; y < H; y++) memcpy(blk.hIn + (size_t)y * *inPitch, gray + (size_t)y * pitch, (size_t)W);
    HIPCHK(h, hipMemcpyAsync(blk.dIn, blk.hIn, smallEnd > smallBegin ? smallEnd : frameBytes, hipMemcpyHostToDevice, s));
    return ORBFE_OK;
}

// What every chain does behind its upload: replay the graph of `key` -- capturing it first if need be -- or, with graphs
// off or after a failed capture, run the same enqueue(stream) -> status on plain launches; wait; check the guard word of
// the downloaded head [n, status, n_matches].
template <class Key, class Enqueue>
int chain_submit(orbfe_handle* h, GraphCache<Key>& cache, size_t bound, const Key& key, const ChainBlocks& blk, size_t inFrame,
                 int inPitch, hipStream_t s, Enqueue enqueue, const char* who)
{
    hipGraphExec_t exec = nullptr;
    if (h->useGraph && !h->timing) {
        exec = cache.find(key);
        if (!exec && (exec = capture_graph(h, enqueue))) cache.insert(key, exec, bound);
    }
    const int rc = exec ? launch_graph(h, exec, s, blk.dIn, inFrame, inPitch, 1) : enqueue(s);
    if (rc != ORBFE_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(s));
    const int status = reinterpret_cast<const int*>(blk.hOut)[1];
    if (status) {
        char buf[112];
        snprintf(buf, sizeof buf, "device guard flags 0x%x in %s", (unsigned)status, who);
        h->err = buf;
        return ORBFE_ERR_INTERNAL;
    }
    return ORBFE_OK;
}

// What every chain's blocks begin with: the frame in the input block; [n, status, n_matches] at 0 of the result block,
// then the per-level counts, the keypoints and the descriptors.  A chain's layout continues behind them with take256().
struct ChainPrefix {
    size_t inFrame, oPer, oKp, oDesc;
};

size_t take256(size_t& off, size_t bytes)
{
    const size_t o = off;
    off = align_up(off + bytes, 256);
    return o;
}

// -> the offset at which the chain's own part of the result block starts
size_t chain_prefix_layout(const orbfe_handle* h, ChainPrefix& L)
{
    const size_t cap = (size_t)h->P.kpCapFrame;
    L.inFrame = align_up((size_t)h->dInPitch * h->prm.image_height, 256);
    size_t off = 256;
    L.oPer = take256(off, (size_t)h->nLevels * sizeof(int));
    L.oKp = take256(off, cap * sizeof(orbfe_keypoint));
    L.oDesc = take256(off, cap * ORBFE_DESC_BYTES);
    return off;
}

// hand-over of that prefix out of the pinned result block; -> n
int chain_prefix_copy_out(const orbfe_handle* h, const uint8_t* hOut, const ChainPrefix& L, orbfe_keypoint* kp_out, uint8_t* desc_out,
                          int* n_out, int* per_level)
{
    const int n = reinterpret_cast<const int*>(hOut)[0];
    *n_out = n;
    memcpy(kp_out, hOut + L.oKp, (size_t)n * sizeof(orbfe_keypoint));
    memcpy(desc_out, hOut + L.oDesc, (size_t)n * ORBFE_DESC_BYTES);
    if (per_level) memcpy(per_level, hOut + L.oPer, (size_t)h->nLevels * sizeof(int));
    return n;
}

}  // namespace

extern "C" {

int orbfe_extract_batch(orbfe_handle* h, const uint8_t* const* grays, int pitch, int batch, orbfe_keypoint* kp_out,
                        uint8_t* desc_out, int* n_out, int* per_level)
{
    if (!h || !grays || !kp_out || !desc_out || !n_out) return ORBFE_ERR_INVALID_ARG;
    if (batch < 1 || batch > h->maxBatch || pitch < h->prm.image_width) return ORBFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    const int W = h->prm.image_width, H = h->prm.image_height, nL = h->nLevels;
    const size_t inFrame = (size_t)h->dInPitch * H;
    hipStream_t s = h->stream;
    // Upload.  Pinned sources (the reference hands over cv::cuda::HostMem, include/ORBextractor.h:62) with a
    // dword-aligned pitch that fits the device staging rows are copied by the DMA engine straight from the caller's
    // buffer, keeping the caller's pitch (level 0 is read with an arbitrary pitch anyway); everything else is
    // re-pitched through the handle's pinned staging block first.
    bool direct = pitch <= h->dInPitch && (pitch & 3) == 0;
    for (int b = 0; b < batch; b++) {
        if (!grays[b]) return ORBFE_ERR_INVALID_ARG;
        if (direct) {
            hipPointerAttribute_t attr;
            if ((reinterpret_cast<uintptr_t>(grays[b]) & 3u) != 0 || hipPointerGetAttributes(&attr, grays[b]) != hipSuccess ||
                attr.type != hipMemoryTypeHost) {
                (void)hipGetLastError();
                direct = false;
            }
        }
    }
    const int inPitch = direct ? pitch : h->dInPitch;
    if (direct) {
        const size_t bytes = (size_t)pitch * (H - 1) + (size_t)W;
        for (int b = 0; b < batch; b++)
            HIPCHK(h, hipMemcpyAsync(h->dIn + b * inFrame, grays[b], bytes, hipMemcpyHostToDevice, s));
    } else {
        for (int b = 0; b < batch; b++)
            for (int y = 0; y < H; y++)
                memcpy(h->hIn + b * inFrame + (size_t)y * h->dInPitch, grays[b] + (size_t)y * pitch, (size_t)W);
        HIPCHK(h, hipMemcpyAsync(h->dIn, h->hIn, inFrame * batch, hipMemcpyHostToDevice, s));
    }
    int rc = extract_enqueue_replay(h, batch, inPitch, s);
    if (rc != ORBFE_OK) return rc;
    HIPCHK(h, hipStreamSynchronize(s));
    rc = check_device_flags(h, batch);
    if (rc != ORBFE_OK) return rc;
    const size_t cap = (size_t)h->P.kpCapFrame;
    for (int b = 0; b < batch; b++) {
        const int n = h->hN[b];
        n_out[b] = n;
        memcpy(kp_out + b * cap, h->hKp + b * cap, (size_t)n * sizeof(orbfe_keypoint));
        memcpy(desc_out + b * cap * ORBFE_DESC_BYTES, h->hDesc + b * cap * ORBFE_DESC_BYTES, (size_t)n * ORBFE_DESC_BYTES);
        if (per_level) memcpy(per_level + (size_t)b * nL, h->hPer + (size_t)b * nL, nL * sizeof(int));
    }
    return ORBFE_OK;
}

int orbfe_extract(orbfe_handle* h, const uint8_t* gray, int pitch, orbfe_keypoint* kp_out, uint8_t* desc_out,
                  int* n_out, int* per_level)
{
    const uint8_t* one[1] = {gray};
    return orbfe_extract_batch(h, one, pitch, 1, kp_out, desc_out, n_out, per_level);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// orbfe_track_frame: extract -> isInFrustum -> SearchByProjection as one captured hipGraph (orbfe.h)
// ---------------------------------------------------------------------------------------------
struct orbfe_map {  // map points resident in HBM (orbfe_map_*, further down)
    orbfe_handle* h = nullptr;
    int cap = 0;
    orbfe_world_point* dPts = nullptr;
    uint8_t* dDesc = nullptr;
};

struct orbfe_covis {  // the covisibility graph resident in HBM (orbfe_covis_*, SPEC DECISION S24, further down)
    orbfe_handle* h = nullptr;
    const orbfe_map* map = nullptr;  // null once the map is destroyed: every later call is refused
    CovisTables T{};
    // per-call scratch, kept here because it has to be found as it was left: first-occurrence stamps [scratchBatch][cap] at rest,
    // vote counters [scratchBatch][kfCap + 1] at zero
    unsigned* dStamps = nullptr;
    int* dCounters = nullptr;
    int scratchBatch = 0;
    CovisConn C{};  // the connection rows (SPEC DECISION S25): connStride == 0 until orbfe_covis_enable_connections
    CovisRefresh R{};  // the refresh state (SPEC DECISION S26): nLevels == 0 until orbfe_covis_enable_refresh
};

// the caller holds h->mu (or is the handle's destruction); the handle's stream is idle
static void covis_free(orbfe_covis* g)
{
    void* ptrs[] = {g->T.kf, g->T.covisible, g->T.children, g->T.kfPoints, g->T.obsCount, g->T.obs, g->dStamps, g->dCounters,
                    g->C.slots, g->C.weights, g->C.count, g->C.work,
                    g->R.desc, g->R.octave, g->R.nFeat, g->R.centre, g->R.obsIdx, g->R.refKf, g->R.sf, g->R.rest};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    g->C = CovisConn{};
    g->R = CovisRefresh{};
    g->T.kf = nullptr;
    g->T.covisible = g->T.children = g->T.kfPoints = g->T.obsCount = g->T.obs = nullptr;
    g->dStamps = nullptr;
    g->dCounters = nullptr;
    g->scratchBatch = 0;
}
static void covis_orphan(orbfe_covis* g)
{
    covis_free(g);
    g->h = nullptr;
    g->map = nullptr;
}
static void covis_detach_map(orbfe_handle* h, const orbfe_map* m)
{
    for (orbfe_covis* g : h->covis)
        if (g->map == m) g->map = nullptr;
}

namespace {

// map points per graph: rounded up so that a local map that grows by a few points replays the same graph; the padding
// records are "bad" (isInFrustum leaves them out of view, SearchByProjection skips them), so results do not change
int track_bucket(int M)
{
    int g = 256;
    while (g * 8 <= M) g <<= 1;  // <= 8 buckets per octave
    return std::max(g, (M + g - 1) / g * g);
}

struct TrackLayout : ChainPrefix {
    size_t oFr, oPts, oMpDesc, inBytes;  // input block
    size_t oMatch, oMps, oXr, outBytes;  // result block
};

TrackLayout track_layout(const orbfe_handle* h, int Mb)
{
    TrackLayout L{};
    size_t off = chain_prefix_layout(h, L);
    L.oFr = L.inFrame;
    L.oPts = L.oFr + align_up(sizeof(orbfe_frustum), 256);
    L.oMpDesc = L.oPts + (size_t)Mb * sizeof(orbfe_world_point);
    L.inBytes = L.oMpDesc + (size_t)Mb * ORBFE_DESC_BYTES;
    L.oMatch = take256(off, (size_t)h->P.kpCapFrame * sizeof(int));
    L.oMps = take256(off, (size_t)Mb * sizeof(orbfe_map_point));
    L.oXr = take256(off, (size_t)Mb * sizeof(float));
    L.outBytes = off;
    return L;
}

// (re)allocate the blocks for Mb map points; the caller holds h->mu and nothing of this path is in flight
int track_reserve(orbfe_handle* h, int Mb)
{
    if (Mb <= h->trkCapM) return ORBFE_OK;
    h->trackGraphs.drop();
    h->trkCapM = 0;
    const int capM = Mb + Mb / 2;  // head-room: a growing local map does not reallocate (and re-capture) at every bucket
    const TrackLayout L = track_layout(h, capM);
    const int rc = chain_blocks_alloc(h, h->trk, L.inBytes, L.outBytes, L.outBytes, "orbfe_track_frame");
    if (rc == ORBFE_OK) h->trkCapM = capM;
    return rc;
}

// the device side of one call, enqueued on s (directly, or under stream capture): extraction chain on the uploaded
// frame, projection of the uploaded map points with the uploaded frustum, SearchByProjection on the fresh keypoints,
// download of the result block
int track_enqueue(orbfe_handle* h, const TrackLayout& L, int Mb, int inPitch, proj::ProjArgs& A, const orbfe_map* map, hipStream_t s)
{
    int* dHead = reinterpret_cast<int*>(h->trk.dOut);  // [n, status, n_matches]
    int rc = extract_chain(h, h->trk.dIn, L.inFrame, inPitch, 1, reinterpret_cast<orbfe_keypoint*>(h->trk.dOut + L.oKp),
                           h->trk.dOut + L.oDesc, dHead, reinterpret_cast<int*>(h->trk.dOut + L.oPer), dHead + 1, s);
    if (rc != ORBFE_OK) return rc;
    std::string err;
    const orbfe_frustum* dF = reinterpret_cast<const orbfe_frustum*>(h->trk.dIn + L.oFr);
    orbfe_map_point* dMps = reinterpret_cast<orbfe_map_point*>(h->trk.dOut + L.oMps);
    float* dXr = reinterpret_cast<float*>(h->trk.dOut + L.oXr);
    if (map)  // the block carries ids (at the points' offset): gather record + descriptor from the resident map, then project
        rc = frustum_gather_launch(s, 1, dF, reinterpret_cast<const int*>(h->trk.dIn + L.oPts), Mb, map->cap, map->dPts, map->dDesc, dMps,
                                   h->trk.dIn + L.oMpDesc, dXr, err);
    else
        rc = frustum_launch_dev(s, dF, Mb, reinterpret_cast<const orbfe_world_point*>(h->trk.dIn + L.oPts), dMps, dXr, err);
    if (rc == ORBFE_OK) rc = proj::proj_launch(s, A, err);
    if (rc != ORBFE_OK) {
        h->err = err;
        return rc;
    }
    HIPCHK(h, hipMemcpyAsync(h->trk.hOut, h->trk.dOut, L.outBytes, hipMemcpyDeviceToHost, s));
    return ORBFE_OK;
}

}  // namespace

static int track_frame_impl(orbfe_handle* h, const uint8_t* gray, int pitch, const orbfe_frustum* frustum,
                            const orbfe_track_params* tp, int M, const orbfe_world_point* points, const uint8_t* mp_desc,
                            const orbfe_map* map, const int* ids, orbfe_keypoint* kp_out, uint8_t* desc_out, int* n_out, int* per_level,
                            orbfe_map_point* mp_out, float* proj_xr_out, int* match_out, int* n_matches)
{
    if (!h || !gray || !tp || !kp_out || !desc_out || !n_out || !match_out || !n_matches || M < 0) return ORBFE_ERR_INVALID_ARG;
    if (map ? (map->h != h || (M > 0 && !ids)) : (M > 0 && (!points || !mp_desc))) return ORBFE_ERR_INVALID_ARG;
    if (pitch < h->prm.image_width || pitch >= (1 << 24)) return ORBFE_ERR_INVALID_ARG;
    const int rc0 = frustum_validate(frustum);
    if (rc0 != ORBFE_OK) return rc0;
    std::lock_guard<std::mutex> lk(h->mu);
    if (tp->struct_size != (int)sizeof(orbfe_track_params)) {
        h->err = "orbfe_track_params.struct_size does not match this library (rebuild the caller against include/orbfe.h)";
        return ORBFE_ERR_INVALID_ARG;
    }
    if (tp->grid_cols < 1 || tp->grid_rows < 1 || frustum->n_levels > h->nLevels) return ORBFE_ERR_INVALID_ARG;
    if (h->P.kpCapFrame >= (1 << 20) || tp->grid_cols > 65535 || tp->grid_rows > 32767 ||
        (long long)tp->grid_cols * tp->grid_rows > proj::kMaxCells || M > (1 << 24))
        return ORBFE_ERR_UNSUPPORTED;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const int nL = h->nLevels;
    const int cap = h->P.kpCapFrame;
    const int Mb = track_bucket(M);
    int rc = track_reserve(h, Mb);
    if (rc != ORBFE_OK) return rc;
    const TrackLayout L = track_layout(h, Mb);

    // ---- matcher arguments; the arena is sized here, outside any capture ----
    proj::ProjArgs A{};
    A.B = 1; A.M = Mb; A.kpStride = cap;
    A.g = proj::GridDesc{tp->grid_cols, tp->grid_rows, tp->min_x, tp->min_y, tp->grid_inv_w, tp->grid_inv_h};
    A.th = tp->th; A.thFar = tp->th_far_points; A.nnRatio = tp->nn_ratio; A.farPoints = tp->far_points; A.bFactor = tp->th != 1.0;
    A.kp = reinterpret_cast<const orbfe_keypoint*>(h->trk.dOut + L.oKp);
    A.desc = h->trk.dOut + L.oDesc;
    A.nKp = reinterpret_cast<const int*>(h->trk.dOut);
    A.mps = reinterpret_cast<const orbfe_map_point*>(h->trk.dOut + L.oMps);
    A.mpDesc = h->trk.dIn + L.oMpDesc;
    A.initObs = nullptr;
    A.scaleFactors = h->dSf; A.nLevels = nL;
    A.matchOut = reinterpret_cast<int*>(h->trk.dOut + L.oMatch);
    A.nMatches = reinterpret_cast<int*>(h->trk.dOut) + 2;
    {
        std::string err;
        void* before = h->trackMatch.d;
        rc = proj::proj_setup(h->trackMatch, A, Carver(), 64, err);
        if (rc != ORBFE_OK) {
            h->err = err;
            return rc;
        }
        if (before && h->trackMatch.d != before) h->trackGraphs.drop();  // the arena moved: graphs hold its old address
    }

    // ---- stage the small block: [frustum | points | descriptors] with the padding records marked bad, or -- resident map --
    //      [frustum | ids] with the padding ids outside the map (the gather kernel turns those into bad records) ----
    memcpy(h->trk.hIn + L.oFr, frustum, sizeof(orbfe_frustum));
    size_t smallEnd;  // end of what has to go up behind the frame
    if (map) {
        int* hid = reinterpret_cast<int*>(h->trk.hIn + L.oPts);
        if (M) memcpy(hid, ids, (size_t)M * sizeof(int));
        for (int i = M; i < Mb; i++) hid[i] = 0x7fffffff;
        smallEnd = L.oPts + (size_t)Mb * sizeof(int);
    } else {
        if (M) memcpy(h->trk.hIn + L.oPts, points, (size_t)M * sizeof(orbfe_world_point));
        orbfe_world_point pad{};
        pad.bad = 1;
        pad.skip = 1;
        orbfe_world_point* hp = reinterpret_cast<orbfe_world_point*>(h->trk.hIn + L.oPts);
        for (int i = M; i < Mb; i++) hp[i] = pad;
        if (M) memcpy(h->trk.hIn + L.oMpDesc, mp_desc, (size_t)M * ORBFE_DESC_BYTES);
        if (Mb > M) memset(h->trk.hIn + L.oMpDesc + (size_t)M * ORBFE_DESC_BYTES, 0, (size_t)(Mb - M) * ORBFE_DESC_BYTES);
        smallEnd = L.inBytes;
    }

    // ---- upload: the frame with the small block behind it ----
    int inPitch;
    rc = upload_frame(h, h->trk, gray, pitch, L.oFr, smallEnd, s, &inPitch);
    if (rc != ORBFE_OK) return rc;

    // ---- kernels + download: the graph of this (bucket, pitch, parameters) ----
    orbfe_handle::TrackKey key;
    memset(&key, 0, sizeof key);
    key.Mb = Mb; key.inPitch = inPitch; key.gridCols = tp->grid_cols; key.gridRows = tp->grid_rows; key.farPoints = tp->far_points;
    key.minX = tp->min_x; key.minY = tp->min_y; key.invW = tp->grid_inv_w; key.invH = tp->grid_inv_h; key.th = tp->th;
    key.nnRatio = tp->nn_ratio; key.thFar = tp->th_far_points; key.map = map;
    rc = chain_submit(h, h->trackGraphs, 64, key, h->trk, L.inFrame, inPitch, s,
                      [&](hipStream_t q) { return track_enqueue(h, L, Mb, inPitch, A, map, q); }, "orbfe_track_frame");
    if (rc != ORBFE_OK) return rc;

    // ---- hand over ----
    const int n = chain_prefix_copy_out(h, h->trk.hOut, L, kp_out, desc_out, n_out, per_level);
    *n_matches = n > 0 ? reinterpret_cast<const int*>(h->trk.hOut)[2] : 0;
    memcpy(match_out, h->trk.hOut + L.oMatch, (size_t)n * sizeof(int));
    if (mp_out && M) memcpy(mp_out, h->trk.hOut + L.oMps, (size_t)M * sizeof(orbfe_map_point));
    if (proj_xr_out && M) memcpy(proj_xr_out, h->trk.hOut + L.oXr, (size_t)M * sizeof(float));
    return ORBFE_OK;
}

extern "C" int orbfe_track_frame(orbfe_handle* h, const uint8_t* gray, int pitch, const orbfe_frustum* frustum,
                                 const orbfe_track_params* tp, int M, const orbfe_world_point* points, const uint8_t* mp_desc,
                                 orbfe_keypoint* kp_out, uint8_t* desc_out, int* n_out, int* per_level, orbfe_map_point* mp_out,
                                 float* proj_xr_out, int* match_out, int* n_matches)
{
    return track_frame_impl(h, gray, pitch, frustum, tp, M, points, mp_desc, nullptr, nullptr, kp_out, desc_out, n_out, per_level, mp_out,
                            proj_xr_out, match_out, n_matches);
}

extern "C" int orbfe_track_frame_map(orbfe_handle* h, const uint8_t* gray, int pitch, const orbfe_frustum* frustum,
                                     const orbfe_track_params* tp, const orbfe_map* map, int M, const int* ids, orbfe_keypoint* kp_out,
                                     uint8_t* desc_out, int* n_out, int* per_level, orbfe_map_point* mp_out, float* proj_xr_out,
                                     int* match_out, int* n_matches)
{
    if (!map) return ORBFE_ERR_INVALID_ARG;
    return track_frame_impl(h, gray, pitch, frustum, tp, M, nullptr, nullptr, map, ids, kp_out, desc_out, n_out, per_level, mp_out,
                            proj_xr_out, match_out, n_matches);
}

// ---------------------------------------------------------------------------------------------
// Pipelined host-pointer extraction (orbfe.h: orbfe_stream_*)
// ---------------------------------------------------------------------------------------------
namespace {

// a few persistent workers for the row-by-row re-pitch of pageable frames into pinned memory (one thread moves
// ~8 GB/s of 752-byte rows: a third of what the PCIe link takes)
class RowCopyPool {
public:
    explicit RowCopyPool(int n)
    {
        for (int i = 0; i < n; i++) workers_.emplace_back([this] { loop(); });
    }
    ~RowCopyPool()
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : workers_) t.join();
    }
    // run fn(i) for i in [0, n) on the workers and the caller; returns when all are done
    void parallel_for(int n, const std::function<void(int)>& fn)
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            fn_ = &fn;
            next_ = 0;
            end_ = n;
            pending_ = n;
        }
        cv_.notify_all();
        run_some();
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [this] { return pending_ == 0; });
        fn_ = nullptr;
    }

private:
    void run_some()
    {
        for (;;) {
            int i;
            const std::function<void(int)>* fn;
            {
                std::lock_guard<std::mutex> lk(mu_);
                if (!fn_ || next_ >= end_) return;
                i = next_++;
                fn = fn_;
            }
            (*fn)(i);
            std::lock_guard<std::mutex> lk(mu_);
            if (--pending_ == 0) done_.notify_all();
        }
    }
    void loop()
    {
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [this] { return stop_ || (fn_ && next_ < end_); });
                if (stop_) return;
            }
            run_some();
        }
    }
    std::vector<std::thread> workers_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    const std::function<void(int)>* fn_ = nullptr;
    int next_ = 0, end_ = 0, pending_ = 0;
    bool stop_ = false;
};

struct StreamSlot {
    uint8_t* hIn = nullptr;   // pinned, slotFrames x inFrame
    uint8_t* dIn = nullptr;
    uint8_t* dOut = nullptr;  // [n | status | per-level | keypoints | descriptors], the handle's block layout
    uint8_t* hOut = nullptr;  // pinned mirror
    // extract-and-match submissions (orbfe_stream_enable_track): per frame frustum + map-point ids up, matches down
    uint8_t* hTrkIn = nullptr;   // pinned [frusta (slotFrames) | ids (slotFrames x maxPoints)]
    uint8_t* dTrkIn = nullptr;
    uint8_t* dTrkWork = nullptr; // [map-point records | gathered descriptors]
    uint8_t* dTrkOut = nullptr;  // [n_matches (slotFrames) | match (slotFrames x cap)]
    uint8_t* hTrkOut = nullptr;  // pinned mirror
    hipEvent_t evIn = nullptr, evDone = nullptr, evOut = nullptr;
    int n = 0;
    bool track = false;
};

}  // namespace

struct orbfe_stream {
    orbfe_handle* h = nullptr;
    int nSlots = 0, slotFrames = 0;
    size_t inFrame = 0, outBytes = 0, offStatus = 0, offPer = 0, offKp = 0, offDesc = 0;
    hipStream_t sIn = nullptr, sOut = nullptr;  // upload / download; the kernels run on the handle's stream
    std::vector<StreamSlot> slots;
    // one producer (submit) and one consumer (collect) may run concurrently: a slot belongs to its submission from the
    // moment `submitted` passes it until `collected` does
    std::atomic<unsigned long long> submitted{0}, collected{0};
    RowCopyPool* pool = nullptr;
    std::mutex poolMu;  // RowCopyPool::parallel_for is not re-entrant: the two sides take turns
    // extract-and-match
    orbfe_map* map = nullptr;
    int maxPoints = 0;
    size_t trkInBytes = 0, offIds = 0, trkWorkBytes = 0, offGatherDesc = 0, trkOutBytes = 0, offMatch = 0;
};

extern "C" {

}  // extern "C"

// everything a ring owns except the struct itself; the handle is still alive
static void stream_release(orbfe_stream* st)
{
    orbfe_handle* h = st->h;
    (void)hipSetDevice(h->device);
    if (st->sIn) (void)hipStreamSynchronize(st->sIn);
    (void)hipStreamSynchronize(h->stream);
    if (st->sOut) (void)hipStreamSynchronize(st->sOut);
    for (auto& sl : st->slots) {
        if (sl.hIn) (void)hipHostFree(sl.hIn);
        if (sl.dIn) (void)hipFree(sl.dIn);
        if (sl.dOut) (void)hipFree(sl.dOut);
        if (sl.hOut) (void)hipHostFree(sl.hOut);
        if (sl.hTrkIn) (void)hipHostFree(sl.hTrkIn);
        if (sl.dTrkIn) (void)hipFree(sl.dTrkIn);
        if (sl.dTrkWork) (void)hipFree(sl.dTrkWork);
        if (sl.dTrkOut) (void)hipFree(sl.dTrkOut);
        if (sl.hTrkOut) (void)hipHostFree(sl.hTrkOut);
        for (hipEvent_t e : {sl.evIn, sl.evDone, sl.evOut})
            if (e) (void)hipEventDestroy(e);
    }
    st->slots.clear();
    if (st->sIn) (void)hipStreamDestroy(st->sIn);
    if (st->sOut) (void)hipStreamDestroy(st->sOut);
    st->sIn = st->sOut = nullptr;
    delete st->pool;
    st->pool = nullptr;
    st->map = nullptr;
}

extern "C" {

void orbfe_stream_destroy(orbfe_stream* st)
{
    if (!st) return;
    if (st->h) {  // (null: the handle went first and released the ring's memory, orphan_children)
        orbfe_handle* h = st->h;
        {
            std::lock_guard<std::mutex> lk(h->mu);
            for (size_t i = 0; i < h->rings.size(); i++)
                if (h->rings[i] == st) h->rings.erase(h->rings.begin() + (long)i--);
        }
        stream_release(st);
    }
    delete st;
}

int orbfe_stream_create(orbfe_handle* h, int slots, int slot_frames, orbfe_stream** out)
{
    return orbfe_stream_create_copy_threads(h, slots, slot_frames, 0, out);
}

}  // extern "C"

int orbfe_stream_create_copy_threads(orbfe_handle* h, int slots, int slot_frames, int copy_threads, orbfe_stream** out)
{
    if (!h || !out || slots < 2 || slots > 64 || slot_frames < 1 || slot_frames > h->maxBatch) return ORBFE_ERR_INVALID_ARG;
    *out = nullptr;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    orbfe_stream* st = new (std::nothrow) orbfe_stream();
    if (!st) return ORBFE_ERR_OUT_OF_MEMORY;
    st->h = h;
    st->nSlots = slots;
    st->slotFrames = slot_frames;
    st->inFrame = (size_t)h->dInPitch * h->prm.image_height;
    const size_t B = (size_t)slot_frames, cap = (size_t)h->P.kpCapFrame;
    {
        size_t off = 0;
        auto take = [&](size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; };
        take(B * sizeof(int));
        st->offStatus = take(B * sizeof(int));
        st->offPer = take(B * h->nLevels * sizeof(int));
        st->offKp = take(B * cap * sizeof(orbfe_keypoint));
        st->offDesc = take(B * cap * ORBFE_DESC_BYTES);
        st->outBytes = off;
    }
    st->slots.resize((size_t)slots);
    bool ok = hipStreamCreateWithFlags(&st->sIn, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&st->sOut, hipStreamNonBlocking) == hipSuccess;
    for (auto& sl : st->slots) {
        ok = ok && hipHostMalloc(&sl.hIn, st->inFrame * B) == hipSuccess && hipMalloc(&sl.dIn, st->inFrame * B) == hipSuccess &&
             hipMalloc(&sl.dOut, st->outBytes) == hipSuccess && hipHostMalloc(&sl.hOut, st->outBytes) == hipSuccess &&
             hipEventCreateWithFlags(&sl.evIn, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&sl.evDone, hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&sl.evOut, hipEventDisableTiming) == hipSuccess;
    }
    if (!ok) {
        (void)hipGetLastError();
        h->err = "orbfe_stream_create: allocation failed";
        stream_release(st);  // (not yet registered with the handle; h->mu is held)
        delete st;
        return ORBFE_ERR_OUT_OF_MEMORY;
    }
    const unsigned hw = std::thread::hardware_concurrency();
    st->pool = new RowCopyPool(copy_threads > 0 ? copy_threads : (int)std::min<unsigned>(7u, hw > 2 ? hw / 2 : 1));
    h->rings.push_back(st);
    *out = st;
    return ORBFE_OK;
}

// the slots' extract-and-match blocks and the map of orbfe_stream_enable_track: the ring is idle and serves plain submissions
// again, and a later enable_track starts from empty slots
void orbfe_stream_release_track(orbfe_stream* st)
{
    if (!st || !st->h) return;
    orbfe_handle* h = st->h;
    std::lock_guard<std::mutex> lk(h->mu);
    (void)hipSetDevice(h->device);
    for (auto& sl : st->slots) {
        if (sl.hTrkIn) (void)hipHostFree(sl.hTrkIn);
        if (sl.dTrkIn) (void)hipFree(sl.dTrkIn);
        if (sl.dTrkWork) (void)hipFree(sl.dTrkWork);
        if (sl.dTrkOut) (void)hipFree(sl.dTrkOut);
        if (sl.hTrkOut) (void)hipHostFree(sl.hTrkOut);
        sl.hTrkIn = sl.dTrkIn = sl.dTrkWork = sl.dTrkOut = sl.hTrkOut = nullptr;
    }
    st->map = nullptr;
    st->maxPoints = 0;
}

// waits for everything the ring has in flight (errors ignored) and drops it uncollected
void orbfe_stream_drain(orbfe_stream* st)
{
    if (!st || !st->h) return;
    orbfe_handle* h = st->h;
    (void)hipSetDevice(h->device);
    for (hipStream_t s : {st->sIn, h->stream, st->sOut})
        if (s) (void)hipStreamSynchronize(s);
    (void)hipGetLastError();
    st->collected.store(st->submitted.load(std::memory_order_acquire), std::memory_order_release);
}

extern "C" {

int orbfe_stream_in_flight(const orbfe_stream* st)
{
    return st ? (int)(st->submitted.load(std::memory_order_acquire) - st->collected.load(std::memory_order_acquire)) : 0;
}

// the common submission: upload, extraction chain, optionally projection + SearchByProjection of the slot's frames, download
static int stream_submit_impl(orbfe_stream* st, const uint8_t* const* grays, int pitch, int n, const orbfe_track_params* tp,
                              const orbfe_frustum* frusta, int nPoints, const int* ids)
{
    if (!st || !st->h || !grays || n < 1 || n > st->slotFrames) return ORBFE_ERR_INVALID_ARG;
    orbfe_handle* h = st->h;
    if (pitch < h->prm.image_width) return ORBFE_ERR_INVALID_ARG;
    const bool track = tp != nullptr;
    if (track) {
        if (!st->map || !frusta || nPoints < 0 || nPoints > st->maxPoints || (nPoints > 0 && !ids)) return ORBFE_ERR_INVALID_ARG;
        if (tp->struct_size != (int)sizeof(orbfe_track_params) || tp->grid_cols < 1 || tp->grid_rows < 1) return ORBFE_ERR_INVALID_ARG;
        for (int b = 0; b < n; b++) {
            const int rcf = frustum_validate(&frusta[b]);
            if (rcf != ORBFE_OK) return rcf;
            if (frusta[b].n_levels > h->nLevels) return ORBFE_ERR_INVALID_ARG;
        }
    }
    const unsigned long long seq = st->submitted.load(std::memory_order_relaxed);
    if (seq - st->collected.load(std::memory_order_acquire) >= (unsigned long long)st->nSlots) return ORBFE_ERR_BUSY;
    StreamSlot& sl = st->slots[seq % st->nSlots];
    const int W = h->prm.image_width, H = h->prm.image_height;
    // (the slot was collected: its previous upload, kernels and download have completed -- evOut was waited for)
    bool direct = pitch <= h->dInPitch && (pitch & 3) == 0;
    for (int b = 0; b < n; b++) {
        if (!grays[b]) return ORBFE_ERR_INVALID_ARG;
        if (direct) {
            hipPointerAttribute_t attr;
            if ((reinterpret_cast<uintptr_t>(grays[b]) & 3u) != 0 || hipPointerGetAttributes(&attr, grays[b]) != hipSuccess ||
                attr.type != hipMemoryTypeHost) {
                (void)hipGetLastError();
                direct = false;
            }
        }
    }
    int stagedPitch = h->dInPitch;
    size_t frameStride = st->inFrame;
    if (!direct) {
        // pageable sources go through the slot's pinned staging block on a pool of copy threads -- BEFORE the handle is
        // locked: a consumer thread's collect may need the handle meanwhile.  A dword-aligned source pitch is kept (the
        // kernels read it as it is), so a band of rows is ONE contiguous copy; other pitches are re-pitched row by row.
        const bool keep = (pitch & 3) == 0 && pitch <= h->dInPitch;
        const int dp = keep ? pitch : h->dInPitch;
        const size_t inFrame = st->inFrame;
        uint8_t* hIn = sl.hIn;
        const int bands = 4;  // row bands per frame so that a handful of frames still spreads over the pool
        std::lock_guard<std::mutex> pk(st->poolMu);
        st->pool->parallel_for(n * bands, [&](int job) {
            const int b = job / bands, band = job - b * bands;
            const int y0 = H * band / bands, y1 = H * (band + 1) / bands;
            if (keep) {
                const size_t bytes = (size_t)(y1 - y0 - 1) * pitch + (size_t)W;
                memcpy(hIn + b * inFrame + (size_t)y0 * dp, grays[b] + (size_t)y0 * pitch, bytes);
            } else {
                for (int y = y0; y < y1; y++) memcpy(hIn + b * inFrame + (size_t)y * dp, grays[b] + (size_t)y * pitch, (size_t)W);
            }
        });
        stagedPitch = dp;
    }
    if (track) {  // [frusta | ids] of the slot into its pinned block
        memcpy(sl.hTrkIn, frusta, (size_t)n * sizeof(orbfe_frustum));
        if (nPoints) memcpy(sl.hTrkIn + st->offIds, ids, (size_t)n * nPoints * sizeof(int));
    }
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    if (direct) {
        // pinned sources: DMA straight from the caller's memory.  Frames that sit at a constant distance (a packed
        // [n][H][pitch] block is the usual case) go as ONE copy and keep that distance on the device.
        const size_t bytes = (size_t)pitch * (H - 1) + (size_t)((W + 3) & ~3);
        bool block = n > 1 && grays[1] > grays[0];
        const size_t dist = block ? (size_t)(grays[1] - grays[0]) : 0;
        for (int b = 2; b < n && block; b++) block = grays[b] == grays[b - 1] + dist;
        block = block && (dist & 3) == 0 && dist >= bytes && dist * (size_t)(n - 1) + bytes <= st->inFrame * (size_t)st->slotFrames;
        if (block) {
            frameStride = dist;
            HIPCHK(h, hipMemcpyAsync(sl.dIn, grays[0], dist * (size_t)(n - 1) + bytes, hipMemcpyHostToDevice, st->sIn));
        } else {
            for (int b = 0; b < n; b++)
                HIPCHK(h, hipMemcpyAsync(sl.dIn + b * st->inFrame, grays[b], std::min(bytes, st->inFrame), hipMemcpyHostToDevice, st->sIn));
        }
    } else {
        HIPCHK(h, hipMemcpyAsync(sl.dIn, sl.hIn, st->inFrame * (size_t)n, hipMemcpyHostToDevice, st->sIn));
    }
    if (track) {
        HIPCHK(h, hipMemcpyAsync(sl.dTrkIn, sl.hTrkIn, (size_t)n * sizeof(orbfe_frustum), hipMemcpyHostToDevice, st->sIn));
        if (nPoints)
            HIPCHK(h, hipMemcpyAsync(sl.dTrkIn + st->offIds, sl.hTrkIn + st->offIds, (size_t)n * nPoints * sizeof(int), hipMemcpyHostToDevice,
                                     st->sIn));
    }
    HIPCHK(h, hipEventRecord(sl.evIn, st->sIn));
    // kernels on the handle's stream, behind the upload
    HIPCHK(h, hipStreamWaitEvent(h->stream, sl.evIn, 0));
    const int inPitch = direct ? pitch : stagedPitch;
    orbfe_keypoint* dKp = reinterpret_cast<orbfe_keypoint*>(sl.dOut + st->offKp);
    const int rc = extract_chain(h, sl.dIn, frameStride, inPitch, n, dKp, sl.dOut + st->offDesc, reinterpret_cast<int*>(sl.dOut),
                                 reinterpret_cast<int*>(sl.dOut + st->offPer), reinterpret_cast<int*>(sl.dOut + st->offStatus), h->stream);
    if (rc != ORBFE_OK) return rc;
    if (track) {
        std::string err;
        orbfe_map_point* dMps = reinterpret_cast<orbfe_map_point*>(sl.dTrkWork);
        uint8_t* dMpDesc = sl.dTrkWork + st->offGatherDesc;
        int rcm = frustum_gather_launch(h->stream, n, reinterpret_cast<const orbfe_frustum*>(sl.dTrkIn),
                                        reinterpret_cast<const int*>(sl.dTrkIn + st->offIds), nPoints, st->map->cap, st->map->dPts,
                                        st->map->dDesc, dMps, dMpDesc, nullptr, err);
        if (rcm == ORBFE_OK) {
            MatchScope scope_(h, h->stream);
            rcm = scope_.rc;
            if (rcm == ORBFE_OK)
                rcm = match_projection_batch_device(h->match, h->stream, n, dKp, sl.dOut + st->offDesc, reinterpret_cast<const int*>(sl.dOut),
                                                    h->P.kpCapFrame, tp->grid_cols, tp->grid_rows, tp->min_x, tp->min_y, tp->grid_inv_w,
                                                    tp->grid_inv_h, h->dSf, h->nLevels, nPoints, dMps, dMpDesc, nullptr, tp->th, tp->far_points,
                                                    tp->th_far_points, tp->nn_ratio, reinterpret_cast<int*>(sl.dTrkOut + st->offMatch),
                                                    reinterpret_cast<int*>(sl.dTrkOut), err);
        }
        if (rcm != ORBFE_OK) {
            h->err = err;
            return rcm;
        }
    }
    HIPCHK(h, hipEventRecord(sl.evDone, h->stream));
    // download behind the kernels: the whole block for a full slot (one copy), the used parts otherwise
    HIPCHK(h, hipStreamWaitEvent(st->sOut, sl.evDone, 0));
    if (n == st->slotFrames) {
        HIPCHK(h, hipMemcpyAsync(sl.hOut, sl.dOut, st->outBytes, hipMemcpyDeviceToHost, st->sOut));
    } else {
        const size_t cap = (size_t)h->P.kpCapFrame;
        HIPCHK(h, hipMemcpyAsync(sl.hOut, sl.dOut, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st->sOut));
        HIPCHK(h, hipMemcpyAsync(sl.hOut + st->offStatus, sl.dOut + st->offStatus, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st->sOut));
        HIPCHK(h, hipMemcpyAsync(sl.hOut + st->offPer, sl.dOut + st->offPer, (size_t)n * h->nLevels * sizeof(int), hipMemcpyDeviceToHost, st->sOut));
        HIPCHK(h, hipMemcpyAsync(sl.hOut + st->offKp, sl.dOut + st->offKp, (size_t)n * cap * sizeof(orbfe_keypoint), hipMemcpyDeviceToHost, st->sOut));
        HIPCHK(h, hipMemcpyAsync(sl.hOut + st->offDesc, sl.dOut + st->offDesc, (size_t)n * cap * ORBFE_DESC_BYTES, hipMemcpyDeviceToHost, st->sOut));
    }
    if (track) {
        const size_t cap = (size_t)h->P.kpCapFrame;
        if (n == st->slotFrames) {
            HIPCHK(h, hipMemcpyAsync(sl.hTrkOut, sl.dTrkOut, st->trkOutBytes, hipMemcpyDeviceToHost, st->sOut));
        } else {
            HIPCHK(h, hipMemcpyAsync(sl.hTrkOut, sl.dTrkOut, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st->sOut));
            HIPCHK(h, hipMemcpyAsync(sl.hTrkOut + st->offMatch, sl.dTrkOut + st->offMatch, (size_t)n * cap * sizeof(int), hipMemcpyDeviceToHost,
                                     st->sOut));
        }
    }
    HIPCHK(h, hipEventRecord(sl.evOut, st->sOut));
    sl.n = n;
    sl.track = track;
    st->submitted.store(seq + 1, std::memory_order_release);
    return ORBFE_OK;
}

int orbfe_stream_submit(orbfe_stream* st, const uint8_t* const* grays, int pitch, int n)
{
    return stream_submit_impl(st, grays, pitch, n, nullptr, nullptr, 0, nullptr);
}

int orbfe_stream_submit_track(orbfe_stream* st, const uint8_t* const* grays, int pitch, int n, const orbfe_track_params* tp,
                              const orbfe_frustum* frusta, int n_points, const int* ids)
{
    if (!tp) return ORBFE_ERR_INVALID_ARG;
    return stream_submit_impl(st, grays, pitch, n, tp, frusta, n_points, ids);
}

int orbfe_stream_enable_track(orbfe_stream* st, orbfe_map* map, int max_points)
{
    if (!st || !st->h || !map || map->h != st->h || max_points < 1 || max_points > (1 << 24)) return ORBFE_ERR_INVALID_ARG;
    if (st->map || st->slots[0].dTrkIn || st->submitted.load() != st->collected.load()) return ORBFE_ERR_INVALID_ARG;  // once, on an idle ring
    orbfe_handle* h = st->h;
    if (h->P.kpCapFrame >= (1 << 20)) return ORBFE_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    const size_t F = (size_t)st->slotFrames, M = (size_t)max_points, cap = (size_t)h->P.kpCapFrame;
    st->offIds = align_up(F * sizeof(orbfe_frustum), 256);
    st->trkInBytes = st->offIds + F * M * sizeof(int);
    st->offGatherDesc = align_up(F * M * sizeof(orbfe_map_point), 256);
    st->trkWorkBytes = st->offGatherDesc + F * M * ORBFE_DESC_BYTES;
    st->offMatch = align_up(F * sizeof(int), 256);
    st->trkOutBytes = st->offMatch + F * cap * sizeof(int);
    bool ok = true;
    for (auto& sl : st->slots)
        ok = ok && hipHostMalloc(&sl.hTrkIn, st->trkInBytes) == hipSuccess && hipMalloc(&sl.dTrkIn, st->trkInBytes) == hipSuccess &&
             hipMalloc(&sl.dTrkWork, st->trkWorkBytes) == hipSuccess && hipMalloc(&sl.dTrkOut, st->trkOutBytes) == hipSuccess &&
             hipHostMalloc(&sl.hTrkOut, st->trkOutBytes) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        // give back what was allocated: the ring stays usable for plain submissions, and a retry starts from empty slots
        for (auto& sl : st->slots) {
            if (sl.hTrkIn) (void)hipHostFree(sl.hTrkIn);
            if (sl.dTrkIn) (void)hipFree(sl.dTrkIn);
            if (sl.dTrkWork) (void)hipFree(sl.dTrkWork);
            if (sl.dTrkOut) (void)hipFree(sl.dTrkOut);
            if (sl.hTrkOut) (void)hipHostFree(sl.hTrkOut);
            sl.hTrkIn = sl.dTrkIn = sl.dTrkWork = sl.dTrkOut = sl.hTrkOut = nullptr;
        }
        h->err = "orbfe_stream_enable_track: allocation failed";
        return ORBFE_ERR_OUT_OF_MEMORY;
    }
    st->map = map;
    st->maxPoints = max_points;
    return ORBFE_OK;
}

// waits for the oldest submission and checks its guard flags; *slot_out stays in flight until the caller bumps `collected`
static int stream_wait_oldest(orbfe_stream* st, StreamSlot** slot_out)
{
    if (!st || !st->h) return ORBFE_ERR_INVALID_ARG;
    const unsigned long long seq = st->collected.load(std::memory_order_relaxed);
    if (st->submitted.load(std::memory_order_acquire) == seq) return ORBFE_ERR_INVALID_ARG;
    orbfe_handle* h = st->h;
    StreamSlot& sl = st->slots[seq % st->nSlots];
    HIPCHK(h, hipSetDevice(h->device));
    {
        const hipError_t e = hipEventSynchronize(sl.evOut);  // (no handle lock: a producer may be submitting right now)
        if (e != hipSuccess) {
            std::lock_guard<std::mutex> lk(h->mu);
            return fail_hip(h, e, "hipEventSynchronize(slot)", __LINE__);
        }
    }
    *slot_out = &sl;
    const int* status = reinterpret_cast<const int*>(sl.hOut + st->offStatus);
    for (int b = 0; b < sl.n; b++)
        if (status[b]) {
            char buf[128];
            snprintf(buf, sizeof buf, "device guard flags 0x%x at frame %d of the collected submission", (unsigned)status[b], b);
            std::lock_guard<std::mutex> lk(h->mu);
            h->err = buf;
            st->collected.store(seq + 1, std::memory_order_release);
            return ORBFE_ERR_INTERNAL;
        }
    return ORBFE_OK;
}

int orbfe_stream_collect_view(orbfe_stream* st, const orbfe_keypoint** kp, const uint8_t** desc, const int** n,
                              const int** per_level, int* n_frames)
{
    StreamSlot* sl = nullptr;
    const int rc = stream_wait_oldest(st, &sl);
    if (rc != ORBFE_OK) return rc;
    if (kp) *kp = reinterpret_cast<const orbfe_keypoint*>(sl->hOut + st->offKp);
    if (desc) *desc = sl->hOut + st->offDesc;
    if (n) *n = reinterpret_cast<const int*>(sl->hOut);
    if (per_level) *per_level = reinterpret_cast<const int*>(sl->hOut + st->offPer);
    if (n_frames) *n_frames = sl->n;
    st->collected.fetch_add(1, std::memory_order_release);
    return ORBFE_OK;
}

static int stream_collect_impl(orbfe_stream* st, orbfe_keypoint* kp_out, uint8_t* desc_out, int* n_out, int* per_level, int* match_out,
                               int* n_matches, int* n_frames, bool wantTrack)
{
    if (!st || !kp_out || !desc_out || !n_out || (wantTrack && (!match_out || !n_matches))) return ORBFE_ERR_INVALID_ARG;
    StreamSlot* sl = nullptr;
    const int rc = stream_wait_oldest(st, &sl);
    if (rc != ORBFE_OK) return rc;
    orbfe_handle* h = st->h;
    if (wantTrack && !sl->track) {  // the oldest submission carried no map points: leave it in flight for orbfe_stream_collect
        std::lock_guard<std::mutex> lk(h->mu);
        h->err = "orbfe_stream_collect_track: the oldest submission was made with orbfe_stream_submit";
        return ORBFE_ERR_INVALID_ARG;
    }
    const size_t cap = (size_t)h->P.kpCapFrame;
    const int nL = h->nLevels;
    const int* hn = reinterpret_cast<const int*>(sl->hOut);
    const orbfe_keypoint* hkp = reinterpret_cast<const orbfe_keypoint*>(sl->hOut + st->offKp);
    const uint8_t* hdesc = sl->hOut + st->offDesc;
    const int* hper = reinterpret_cast<const int*>(sl->hOut + st->offPer);
    const int* hnm = wantTrack ? reinterpret_cast<const int*>(sl->hTrkOut) : nullptr;
    const int* hmatch = wantTrack ? reinterpret_cast<const int*>(sl->hTrkOut + st->offMatch) : nullptr;
    const int nfr = sl->n;
    {
        std::lock_guard<std::mutex> pk(st->poolMu);
        st->pool->parallel_for(nfr, [&](int b) {
            const int k = hn[b];
            n_out[b] = k;
            memcpy(kp_out + b * cap, hkp + b * cap, (size_t)k * sizeof(orbfe_keypoint));
            memcpy(desc_out + b * cap * ORBFE_DESC_BYTES, hdesc + b * cap * ORBFE_DESC_BYTES, (size_t)k * ORBFE_DESC_BYTES);
            if (per_level) memcpy(per_level + (size_t)b * nL, hper + (size_t)b * nL, nL * sizeof(int));
            if (wantTrack) {
                n_matches[b] = k > 0 ? hnm[b] : 0;
                memcpy(match_out + b * cap, hmatch + b * cap, (size_t)k * sizeof(int));
            }
        });
    }
    if (n_frames) *n_frames = nfr;
    st->collected.fetch_add(1, std::memory_order_release);
    return ORBFE_OK;
}

int orbfe_stream_collect(orbfe_stream* st, orbfe_keypoint* kp_out, uint8_t* desc_out, int* n_out, int* per_level, int* n_frames)
{
    return stream_collect_impl(st, kp_out, desc_out, n_out, per_level, nullptr, nullptr, n_frames, false);
}

int orbfe_stream_collect_track(orbfe_stream* st, orbfe_keypoint* kp_out, uint8_t* desc_out, int* n_out, int* per_level, int* match_out,
                               int* n_matches, int* n_frames)
{
    return stream_collect_impl(st, kp_out, desc_out, n_out, per_level, match_out, n_matches, n_frames, true);
}

// ---------------------------------------------------------------------------------------------
// Map points resident in HBM (orbfe.h: orbfe_map_*)
// ---------------------------------------------------------------------------------------------
int orbfe_map_create(orbfe_handle* h, int capacity, orbfe_map** out)
{
    if (!h || !out || capacity < 1 || capacity > (1 << 26)) return ORBFE_ERR_INVALID_ARG;
    *out = nullptr;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    orbfe_map* m = new (std::nothrow) orbfe_map();
    if (!m) return ORBFE_ERR_OUT_OF_MEMORY;
    m->h = h;
    m->cap = capacity;
    if (hipMalloc(&m->dPts, (size_t)capacity * sizeof(orbfe_world_point)) != hipSuccess ||
        hipMalloc(&m->dDesc, (size_t)capacity * ORBFE_DESC_BYTES) != hipSuccess) {
        (void)hipGetLastError();
        if (m->dPts) (void)hipFree(m->dPts);
        delete m;
        h->err = "orbfe_map_create: allocation failed";
        return ORBFE_ERR_OUT_OF_MEMORY;
    }
    // an entry that was never written is a bad point: skipped by isInFrustum and by the matcher
    std::vector<orbfe_world_point> init((size_t)std::min(capacity, 1 << 16));
    for (auto& p : init) { p = orbfe_world_point{}; p.bad = 1; }
    for (size_t o = 0; o < (size_t)capacity; o += init.size())
        if (copy_sync(m->dPts + o, init.data(), std::min(init.size(), (size_t)capacity - o) * sizeof(orbfe_world_point),
                      hipMemcpyHostToDevice, h->stream) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(m->dPts);
            (void)hipFree(m->dDesc);
            delete m;
            return ORBFE_ERR_HIP;
        }
    (void)memset_sync(m->dDesc, 0, (size_t)capacity * ORBFE_DESC_BYTES, h->stream);
    h->maps.push_back(m);
    *out = m;
    return ORBFE_OK;
}

// the map's device memory and every reference to it; the caller holds m->h->mu (or is the handle's destruction)
static void map_release(orbfe_map* m)
{
    orbfe_handle* h = m->h;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    h->trackGraphs.drop();  // graphs of orbfe_track_frame_map hold this map's addresses
    for (orbfe_stream* st : h->rings)
        if (st->map == m) {  // a ring that was given this map: its later track submissions are refused, not served from freed memory
            st->map = nullptr;
            st->maxPoints = 0;
        }
    covis_detach_map(h, m);  // a graph over this map's ids: its later calls are refused
    if (m->dPts) (void)hipFree(m->dPts);
    if (m->dDesc) (void)hipFree(m->dDesc);
    m->dPts = nullptr;
    m->dDesc = nullptr;
}

void orbfe_map_destroy(orbfe_map* m)
{
    if (!m) return;
    if (m->h) {  // (null: the handle went first, orphan_children)
        std::lock_guard<std::mutex> lk(m->h->mu);
        for (size_t i = 0; i < m->h->maps.size(); i++)
            if (m->h->maps[i] == m) m->h->maps.erase(m->h->maps.begin() + (long)i--);
        map_release(m);
    }
    delete m;
}

int orbfe_map_update(orbfe_handle* h, orbfe_map* m, int n, const int* ids, const orbfe_world_point* points, const uint8_t* desc)
{
    if (!h || !m || m->h != h || n < 0 || (n > 0 && (!ids || !points || !desc))) return ORBFE_ERR_INVALID_ARG;
    for (int i = 0; i < n; i++)
        if (ids[i] < 0 || ids[i] >= m->cap) return ORBFE_ERR_INVALID_ARG;
    if (n == 0) return ORBFE_OK;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    // staged through the matcher's grow-only arenas: [ids | points | descriptors]; on the handle's stream, i.e. behind
    // every submission made so far (their kernels run there) and in front of every later one
    Carver c;
    const size_t oIds = c.take((size_t)n * sizeof(int));
    const size_t oPts = c.take((size_t)n * sizeof(orbfe_world_point));
    const size_t oDesc = c.take((size_t)n * ORBFE_DESC_BYTES);
    std::string err;
    MatchScope scope_(h, h->stream);
    if (scope_.rc != ORBFE_OK) return scope_.rc;
    int rc = ensure(h->match, c.off, c.off, err);
    if (rc != ORBFE_OK) {
        h->err = err;
        return rc;
    }
    uint8_t* hp = static_cast<uint8_t*>(h->match.hpin);
    uint8_t* dp = static_cast<uint8_t*>(h->match.d);
    memcpy(hp + oIds, ids, (size_t)n * sizeof(int));
    memcpy(hp + oPts, points, (size_t)n * sizeof(orbfe_world_point));
    memcpy(hp + oDesc, desc, (size_t)n * ORBFE_DESC_BYTES);
    HIPCHK(h, hipMemcpyAsync(dp, hp, c.off, hipMemcpyHostToDevice, h->stream));
    rc = map_scatter_launch(h->stream, n, reinterpret_cast<const int*>(dp + oIds), reinterpret_cast<const orbfe_world_point*>(dp + oPts),
                            dp + oDesc, m->cap, m->dPts, m->dDesc, err);
    if (rc != ORBFE_OK) {
        h->err = err;
        return rc;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ORBFE_OK;
}

}  // extern "C"

namespace {
// orbfe_destroy with maps / rings still alive: release their memory now (the device context of the handle is still
// current) and cut the back pointers; their own destroy calls then only delete the shells
void orphan_children(orbfe_handle* h)
{
    for (orbfe_stream* st : h->rings) {
        stream_release(st);
        st->h = nullptr;
    }
    h->rings.clear();
    for (orbfe_covis* g : h->covis) covis_orphan(g);
    h->covis.clear();
    for (orbfe_map* m : h->maps) {
        map_release(m);
        m->h = nullptr;
    }
    h->maps.clear();
}
}  // namespace

extern "C" {

int orbfe_get_pyramid_level(orbfe_handle* h, int frame, int level, int blurred, uint8_t* out, int out_pitch)
{
    if (!h || !out || level < 0 || level >= h->nLevels || frame < 0) return ORBFE_ERR_INVALID_ARG;
    const LevelDesc& L = h->P.lv[level];
    if (out_pitch < L.w) return ORBFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (frame >= h->lastBatch) return ORBFE_ERR_INVALID_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (h->extractUsed) HIPCHK(h, hipEventSynchronize(h->evExtract));  // the last call, whatever stream it ran on
    const uint8_t* src;
    size_t spitch;
    if (blurred) {
        src = h->ws + L.blurOff + (size_t)frame * L.blurFrameStride;
        spitch = L.pitch;
    } else if (level == 0) {
        src = h->lastGray + (size_t)frame * h->lastStride;
        spitch = h->lastPitch;
    } else {
        src = h->ws + L.imgOff + (size_t)frame * L.imgFrameStride;
        spitch = L.pitch;
    }
    HIPCHK(h, hipMemcpy2D(out, out_pitch, src, spitch, L.w, L.h, hipMemcpyDeviceToHost));
    return ORBFE_OK;
}

int orbfe_debug_get_candidates(orbfe_handle* h, int frame, int level, uint32_t* packed, int cap, int* n_out,
                               int counters[4])
{
    if (!h || !n_out || level < 0 || level >= h->nLevels || frame < 0) return ORBFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (frame >= h->lastBatch) return ORBFE_ERR_INVALID_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (h->extractUsed) HIPCHK(h, hipEventSynchronize(h->evExtract));
    uint32_t c[kCntWords];
    HIPCHK(h, copy_sync(c, h->dCounters + ((size_t)frame * h->nLevels + level) * kCntWords, sizeof c, hipMemcpyDeviceToHost, h->stream));
    const LevelDesc& L = h->P.lv[level];
    int n = (int)std::min<uint32_t>(c[kCntCand], (uint32_t)L.candCap);
    if (counters) {
        counters[0] = (int)c[kCntCand];
        counters[1] = (int)c[kCntHigh];
        counters[2] = (int)c[kCntPreLow];
        counters[3] = (int)c[kCntPreHigh];
    }
    const int m = std::min(n, cap);
    if (packed && m > 0)
        HIPCHK(h, copy_sync(packed, h->dCand + L.candOff + (size_t)frame * L.candCap, (size_t)m * sizeof(uint32_t),
                            hipMemcpyDeviceToHost, h->stream));
    *n_out = m;
    return ORBFE_OK;
}

int orbfe_set_graph_capture(orbfe_handle* h, int enable)
{
    if (!h) return ORBFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    h->useGraph = enable != 0;
    if (enable) h->captureFailures = h->captureFailStreak = 0;
    return ORBFE_OK;
}

int orbfe_set_stream_priority(orbfe_handle* h, int high)
{
    if (!h) return ORBFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    int least = 0, greatest = 0;
    HIPCHK(h, hipDeviceGetStreamPriorityRange(&least, &greatest));  // numerically lower = higher priority
    hipStream_t ns = nullptr;
    HIPCHK(h, hipStreamCreateWithPriority(&ns, hipStreamNonBlocking, high ? greatest : least));
    // the handle must be idle: everything it enqueued has finished before the stream goes away
    if (hipStreamSynchronize(h->stream) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamDestroy(ns);
        return ORBFE_ERR_HIP;
    }
    (void)hipStreamDestroy(h->stream);
    h->stream = ns;
    h->extractUsed = h->matchUsed = false;  // the hand-over events belonged to work that is complete
    h->extractStream = h->matchStream = nullptr;
    return ORBFE_OK;
}

int orbfe_debug_clock_probe(orbfe_handle* h, int spin_us, unsigned long long* d_out, void* stream)
{
    if (!h || !d_out || spin_us < 1 || spin_us > 100000) return ORBFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    launch_clock_probe(stream ? static_cast<hipStream_t>(stream) : h->stream, d_out, (unsigned)spin_us * 100u);
    HIPCHK(h, hipGetLastError());
    return ORBFE_OK;
}

int orbfe_debug_graph_stats(orbfe_handle* h, int* captured, int* failed)
{
    if (!h) return ORBFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (captured) *captured = h->graphCaptures;
    if (failed) *failed = h->captureFailures;
    return ORBFE_OK;
}

int orbfe_get_device_status(orbfe_handle* h, unsigned* flags_out)
{
    if (!h) return ORBFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    unsigned flags = 0;
    if (h->extractUsed && h->lastBatch > 0) {
        HIPCHK(h, hipEventSynchronize(h->evExtract));
        std::vector<uint32_t> c((size_t)h->lastBatch * h->nLevels * kCntWords);
        HIPCHK(h, copy_sync(c.data(), h->dCounters, c.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        for (size_t i = 0; i < (size_t)h->lastBatch * h->nLevels; i++) flags |= c[i * kCntWords + kCntStatus];
    }
    if (flags_out) *flags_out = flags;
    if (flags) {
        char buf[96];
        snprintf(buf, sizeof buf, "device guard flags 0x%x in the last extract call", flags);
        h->err = buf;
        return ORBFE_ERR_INTERNAL;
    }
    return ORBFE_OK;
}

int orbfe_hamming(const uint8_t* a, const uint8_t* b)
{
    // ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1375-1391): popcount of the 256-bit XOR
    int d = 0;
    for (int i = 0; i < 4; i++) {
        uint64_t x, y;
        memcpy(&x, a + 8 * i, 8);
        memcpy(&y, b + 8 * i, 8);
        d += __builtin_popcountll(x ^ y);
    }
    return d;
}

int orbfe_match_projection(orbfe_handle* h, const orbfe_frame_view* F, int M, const orbfe_map_point* mps,
                           const uint8_t* mp_desc, const int* init_obs, float th, int far_points, float th_far,
                           float nn_ratio, int* match_out, int* n_matches)
{
    if (!h || !F || !match_out || !n_matches || M < 0 || F->n < 0) return ORBFE_ERR_INVALID_ARG;
    if ((M > 0 && (!mps || !mp_desc)) || (F->n > 0 && (!F->kp || !F->desc)) || !F->scale_factors) return ORBFE_ERR_INVALID_ARG;
    return match_call(h, nullptr, [&](hipStream_t s, std::string& err) {
        return match_projection_run(h->match, s, F, M, mps, mp_desc, init_obs, th, far_points, th_far, nn_ratio, match_out, n_matches,
                                    err);
    });
}

int orbfe_match_projection_batch_device(orbfe_handle* h, int batch, const orbfe_keypoint* d_kp, const uint8_t* d_desc,
                                        const int* d_n, int kp_stride, int grid_cols, int grid_rows, float min_x,
                                        float min_y, float inv_w, float inv_h, int M, const orbfe_map_point* d_mps,
                                        const uint8_t* d_mp_desc, const int* d_init_obs, float th, int far_points,
                                        float th_far, float nn_ratio, int* d_match_out, int* d_n_matches, void* stream_)
{
    if (!h || !d_kp || !d_desc || !d_n || !d_match_out || !d_n_matches || batch < 1 || M < 0 || kp_stride < 1 ||
        grid_cols < 1 || grid_rows < 1)
        return ORBFE_ERR_INVALID_ARG;
    if (M > 0 && (!d_mps || !d_mp_desc)) return ORBFE_ERR_INVALID_ARG;
    return match_call(h, (hipStream_t)stream_, [&](hipStream_t s, std::string& err) {
        return match_projection_batch_device(h->match, s, batch, d_kp, d_desc, d_n, kp_stride, grid_cols, grid_rows, min_x, min_y, inv_w,
                                             inv_h, h->dSf, h->nLevels, M, d_mps, d_mp_desc, d_init_obs, th, far_points, th_far, nn_ratio,
                                             d_match_out, d_n_matches, err);
    });
}

int orbfe_match_initialization(orbfe_handle* h, const orbfe_frame_view* F1, const orbfe_frame_view* F2, int window_size,
                               float nn_ratio, int check_orientation, int* matches12_out, int* n_matches)
{
    if (!h || !F1 || !F2 || !matches12_out || !n_matches || F1->n < 0 || F2->n < 0 || window_size < 0)
        return ORBFE_ERR_INVALID_ARG;
    if ((F1->n > 0 && (!F1->kp || !F1->desc)) || (F2->n > 0 && (!F2->kp || !F2->desc)) || F2->grid_cols < 1 || F2->grid_rows < 1)
        return ORBFE_ERR_INVALID_ARG;
    return match_call(h, nullptr, [&](hipStream_t s, std::string& err) {
        return match_initialization_run(h->match, s, F1, F2, window_size, nn_ratio, check_orientation, matches12_out, n_matches, err);
    });
}

int orbfe_project_map_points_device(orbfe_handle* h, const orbfe_frustum* frustum, int n, const orbfe_world_point* d_points,
                                    orbfe_map_point* d_out, float* d_proj_xr, void* stream)
{
    if (!h || n < 0 || (n > 0 && (!d_points || !d_out))) return ORBFE_ERR_INVALID_ARG;
    const int rc0 = frustum_validate(frustum);
    if (rc0 != ORBFE_OK) return rc0;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    std::string err;
    const int rc = frustum_launch(stream ? static_cast<hipStream_t>(stream) : h->stream, frustum, n, d_points, d_out, d_proj_xr, err);
    if (rc != ORBFE_OK) h->err = err;
    return rc;
}

int orbfe_project_map_points(orbfe_handle* h, const orbfe_frustum* frustum, int n, const orbfe_world_point* points,
                             orbfe_map_point* out, float* proj_xr)
{
    if (!h || n < 0 || (n > 0 && (!points || !out))) return ORBFE_ERR_INVALID_ARG;
    const int rc0 = frustum_validate(frustum);
    if (rc0 != ORBFE_OK) return rc0;
    if (n == 0) return ORBFE_OK;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    // staging through the matcher's grow-only arenas: [points | out | xr] on both sides
    const size_t bIn = (size_t)n * sizeof(orbfe_world_point), bOut = (size_t)n * sizeof(orbfe_map_point), bXr = (size_t)n * sizeof(float);
    std::string err;
    MatchScope scope_(h, h->stream);
    if (scope_.rc != ORBFE_OK) return scope_.rc;
    int rc = ensure(h->match, bIn + bOut + bXr + 256, bIn + bOut + bXr + 256, err);
    if (rc != ORBFE_OK) {
        h->err = err;
        return rc;
    }
    uint8_t* dp = static_cast<uint8_t*>(h->match.d);
    uint8_t* hp = static_cast<uint8_t*>(h->match.hpin);
    memcpy(hp, points, bIn);
    HIPCHK(h, hipMemcpyAsync(dp, hp, bIn, hipMemcpyHostToDevice, h->stream));
    rc = frustum_launch(h->stream, frustum, n, reinterpret_cast<const orbfe_world_point*>(dp),
                        reinterpret_cast<orbfe_map_point*>(dp + bIn), reinterpret_cast<float*>(dp + bIn + bOut), err);
    if (rc != ORBFE_OK) {
        h->err = err;
        return rc;
    }
    HIPCHK(h, hipMemcpyAsync(hp + bIn, dp + bIn, bOut + bXr, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    memcpy(out, hp + bIn, bOut);
    if (proj_xr) memcpy(proj_xr, hp + bIn + bOut, bXr);
    return ORBFE_OK;
}

int orbfe_fuse_search(orbfe_handle* h, const orbfe_frame_view* KF, const float* inv_level_sigma2, const float* u_right,
                      const orbfe_frustum* frustum, float th, int M, const orbfe_world_point* points, const uint8_t* mp_desc,
                      int* best_idx_out, int* best_dist_out)
{
    if (!h || !KF || !inv_level_sigma2 || M < 0 || KF->n < 0 || (KF->n > 0 && (!KF->kp || !KF->desc || !KF->scale_factors)) ||
        (M > 0 && (!points || !mp_desc || !best_idx_out || !best_dist_out)))
        return ORBFE_ERR_INVALID_ARG;
    const int rc0 = frustum_validate(frustum);
    if (rc0 != ORBFE_OK) return rc0;
    return match_call(h, nullptr, [&](hipStream_t s, std::string& err) {
        return fuse_search_run(h->match, s, KF, inv_level_sigma2, u_right, frustum, th, M, points, mp_desc, 1, -1, best_idx_out,
                               best_dist_out, err);
    });
}

int orbfe_fuse_search_right(orbfe_handle* h, const orbfe_frame_view* KF, int n_right, const float* inv_level_sigma2,
                            const float* u_right, const orbfe_frustum* frustum, float th, int M, const orbfe_world_point* points,
                            const uint8_t* mp_desc, int* best_idx_out, int* best_dist_out)
{
    if (!h || !KF || !inv_level_sigma2 || M < 0 || KF->n < 0 || n_right < 0 ||
        (KF->n > 0 && (!KF->kp || !KF->desc || !KF->scale_factors)) ||
        (M > 0 && (!points || !mp_desc || !best_idx_out || !best_dist_out)))
        return ORBFE_ERR_INVALID_ARG;
    const int rc0 = frustum_validate(frustum);
    if (rc0 != ORBFE_OK) return rc0;
    return match_call(h, nullptr, [&](hipStream_t s, std::string& err) {
        return fuse_search_run(h->match, s, KF, inv_level_sigma2, u_right, frustum, th, M, points, mp_desc, 1, n_right, best_idx_out,
                               best_dist_out, err);
    });
}

static bool view_args_bad(const orbfe_frame_view* V)
{
    return !V || V->n < 0 || (V->n > 0 && (!V->kp || !V->desc || !V->scale_factors));
}

int orbfe_fuse_search_sim3(orbfe_handle* h, const orbfe_frame_view* KF, const orbfe_frustum* frustum, float th, int M,
                           const orbfe_world_point* points, const uint8_t* mp_desc, int* best_idx_out, int* best_dist_out)
{
    if (!h || view_args_bad(KF) || M < 0 || (M > 0 && (!points || !mp_desc || !best_idx_out || !best_dist_out)))
        return ORBFE_ERR_INVALID_ARG;
    const int rc0 = frustum_validate(frustum);
    if (rc0 != ORBFE_OK) return rc0;
    return match_call(h, nullptr, [&](hipStream_t s, std::string& err) {
        return fuse_search_run(h->match, s, KF, nullptr, nullptr, frustum, th, M, points, mp_desc, 0, -1, best_idx_out, best_dist_out,
                               err);
    });
}

static bool sim3_view_bad(const orbfe_sim3_view* D)
{
    return !D || D->n_levels < 1 || !(D->log_scale_factor > 0.0f);
}

int orbfe_search_by_sim3(orbfe_handle* h, const orbfe_frame_view* KF1, const orbfe_frame_view* KF2,
                         const orbfe_sim3_view* dir12, const orbfe_sim3_view* dir21, const orbfe_world_point* mp1,
                         const uint8_t* mp_desc1, const orbfe_world_point* mp2, const uint8_t* mp_desc2, float th,
                         int* match12_out, int* n_found)
{
    if (!h || view_args_bad(KF1) || view_args_bad(KF2) || sim3_view_bad(dir12) || sim3_view_bad(dir21) || !n_found ||
        (KF1->n > 0 && (!mp1 || !mp_desc1 || !match12_out)) || (KF2->n > 0 && (!mp2 || !mp_desc2)))
        return ORBFE_ERR_INVALID_ARG;
    return match_call(h, nullptr, [&](hipStream_t s, std::string& err) {
        return search_by_sim3_run(h->match, s, KF1, KF2, dir12, dir21, mp1, mp_desc1, mp2, mp_desc2, th, match12_out, n_found, err);
    });
}

int orbfe_match_projection_keyframe(orbfe_handle* h, const orbfe_frame_view* frame, const orbfe_frustum* frustum,
                                    int n_points, const orbfe_world_point* points, const uint8_t* mp_desc,
                                    const float* kf_angle, const uint8_t* frame_has_mp, float th, int check_orientation,
                                    int* match_out, int* n_matches)
{
    if (!h || view_args_bad(frame) || n_points < 0 || !n_matches || (frame->n > 0 && !match_out) ||
        (n_points > 0 && (!points || !mp_desc || (check_orientation && !kf_angle))))
        return ORBFE_ERR_INVALID_ARG;
    const int rc0 = frustum_validate(frustum);
    if (rc0 != ORBFE_OK) return rc0;
    return match_call(h, nullptr, [&](hipStream_t s, std::string& err) {
        return match_projection_kf_run(h->match, s, frame, frustum, n_points, points, mp_desc, kf_angle, frame_has_mp, th,
                                       check_orientation, match_out, n_matches, err);
    });
}

int orbfe_match_triangulation(orbfe_handle* h, int n_groups, const int* kf1_off, const int* kf1_idx, const int* kf2_off,
                              const int* kf2_idx, int n1, const orbfe_keypoint* kp1, const uint8_t* desc1,
                              const uint8_t* has_mp1, const uint8_t* stereo1, int n2, const orbfe_keypoint* kp2,
                              const uint8_t* desc2, const uint8_t* has_mp2, const uint8_t* stereo2,
                              const float* scale_factors2, int n_levels2, const orbfe_tri_params* params,
                              int* matches12_out, int* n_matches)
{
    if (!h || !params || !n_matches || n_groups < 0 || n1 < 0 || n2 < 0 || n_levels2 < 1 || !scale_factors2 ||
        (n_groups > 0 && (!kf1_off || !kf2_off)) || (n1 > 0 && (!kp1 || !desc1 || !has_mp1 || !matches12_out)) ||
        (n2 > 0 && (!kp2 || !desc2 || !has_mp2)))
        return ORBFE_ERR_INVALID_ARG;
    if (n_groups > 0 && ((kf1_off[n_groups] > 0 && !kf1_idx) || (kf2_off[n_groups] > 0 && !kf2_idx))) return ORBFE_ERR_INVALID_ARG;
    if (params->struct_size != (int)sizeof(orbfe_tri_params)) {  // a caller built against another layout of the block
        std::lock_guard<std::mutex> lk(h->mu);
        h->err = "orbfe_tri_params.struct_size does not match this library (rebuild the caller against include/orbfe.h)";
        return ORBFE_ERR_INVALID_ARG;
    }
    return match_call(h, nullptr, [&](hipStream_t s, std::string& err) {
        return match_triangulation_run(h->match, s, n_groups, kf1_off, kf1_idx, kf2_off, kf2_idx, n1, kp1, desc1, has_mp1, stereo1, n2, kp2,
                                       desc2, has_mp2, stereo2, scale_factors2, n_levels2, params, matches12_out, n_matches, err);
    });
}

struct orbfe_keyframe {
    orbfe::KeyFrameDev* k;
    int device;
    const orbfe_handle* owner;  // the handle it was created from (the new-point entry points refuse any other)
};

int orbfe_keyframe_create(orbfe_handle* h, int n, const orbfe_keypoint* kp, const uint8_t* desc, const int* node_id,
                          const uint8_t* stereo, const float* scale_factors, int n_levels, orbfe_keyframe** out)
{
    if (!h || !out) return ORBFE_ERR_INVALID_ARG;
    *out = nullptr;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    std::string err;
    orbfe::KeyFrameDev* k = nullptr;
    const int rc = keyframe_create(n, kp, desc, node_id, stereo, scale_factors, n_levels, h->stream, &k, err);
    if (rc != ORBFE_OK) {
        h->err = err;
        return rc;
    }
    *out = new orbfe_keyframe{k, h->device, h};
    return ORBFE_OK;
}

void orbfe_keyframe_destroy(orbfe_keyframe* kf)
{
    if (!kf) return;
    (void)hipSetDevice(kf->device);
    keyframe_destroy(kf->k);
    delete kf;
}

int orbfe_keyframe_size(const orbfe_keyframe* kf) { return kf ? kf->k->n : 0; }

int orbfe_keyframe_set_grid(orbfe_handle* h, orbfe_keyframe* kf, int grid_cols, int grid_rows, float min_x, float min_y,
                            float grid_inv_w, float grid_inv_h, const float* inv_level_sigma2, const float* u_right)
{
    if (!h || !kf || kf->device != h->device || !inv_level_sigma2 || grid_cols < 1 || grid_rows < 1) return ORBFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    std::string err;
    const int rc = keyframe_set_grid(kf->k, h->stream, grid_cols, grid_rows, min_x, min_y, grid_inv_w, grid_inv_h, inv_level_sigma2,
                                     u_right, err);
    if (rc != ORBFE_OK) h->err = err;
    return rc;
}

int orbfe_fuse_search_keyframe(orbfe_handle* h, const orbfe_keyframe* kf, const orbfe_map* map, int M, const int* ids,
                               const orbfe_frustum* frustum, float th, int* best_idx_out, int* best_dist_out)
{
    if (!h || !kf || !map || kf->device != h->device || map->h != h || M < 0 || (M > 0 && (!ids || !best_idx_out || !best_dist_out)))
        return ORBFE_ERR_INVALID_ARG;
    const int rc0 = frustum_validate(frustum);
    if (rc0 != ORBFE_OK) return rc0;
    // the scope also orders the call behind an orbfe_map_update of another stream's making
    return match_call(h, nullptr, [&](hipStream_t s, std::string& err) {
        return fuse_search_keyframe_run(h->match, s, kf->k, map->cap, map->dPts, map->dDesc, M, ids, frustum, th, best_idx_out,
                                        best_dist_out, err);
    });
}

int orbfe_fuse_search_keyframes(orbfe_handle* h, int K, const orbfe_keyframe* const* kfs, const orbfe_frustum* frusta,
                                const orbfe_map* map, int M, const int* ids, const uint8_t* skip, float th, int* best_idx_out,
                                int* best_dist_out, int cand_cap, int* cand_idx_out, int* cand_count_out)
{
    if (!h || !map || map->h != h || K < 0 || K > 4096 || M < 0 || cand_cap < 0 || cand_cap > 16) return ORBFE_ERR_INVALID_ARG;
    if (K > 0 && (!kfs || !frusta)) return ORBFE_ERR_INVALID_ARG;
    if (K > 0 && M > 0 && (!ids || !best_idx_out || !best_dist_out || (cand_cap > 0 && (!cand_idx_out || !cand_count_out))))
        return ORBFE_ERR_INVALID_ARG;
    std::vector<const orbfe::KeyFrameDev*> kd((size_t)K);
    for (int k = 0; k < K; k++) {
        if (!kfs[k] || kfs[k]->device != h->device) return ORBFE_ERR_INVALID_ARG;
        const int rc0 = frustum_validate(&frusta[k]);
        if (rc0 != ORBFE_OK) return rc0;
        kd[(size_t)k] = kfs[k]->k;
    }
    std::lock_guard<std::mutex> lk(h->mu);
    for (int k = 0; k < K; k++) {  // the single call's checks for every target, before anything is enqueued
        if (!kd[(size_t)k]->hasGrid) {
            h->err = "orbfe_fuse_search_keyframes: target " + std::to_string(k) + " has no grid (orbfe_keyframe_set_grid)";
            return ORBFE_ERR_INVALID_ARG;
        }
        if (kd[(size_t)k]->n > 0 && M > 0 && frusta[k].n_levels > kd[(size_t)k]->nLevels) return ORBFE_ERR_INVALID_ARG;
    }
    if (K == 0 || M == 0) return ORBFE_OK;
    // the scope also orders the call behind an orbfe_map_update of another stream's making
    return match_call_locked(h, nullptr, [&](hipStream_t s, std::string& err) {
        return fuse_search_keyframes_run(h->match, s, K, kd.data(), frusta, map->cap, map->dPts, map->dDesc, M, ids, skip, th, best_idx_out,
                                         best_dist_out, cand_cap, cand_idx_out, cand_count_out, err);
    });
}

int orbfe_fuse_select(const int* cand_idx, int cand_count, int cand_cap, const uint8_t* kf_desc, int n_kf, const uint8_t* mp_desc,
                      int* best_idx, int* best_dist)
{
    if (!best_idx || !best_dist || cand_count < 0 || cand_cap < 0 || cand_cap > 16 || n_kf < 0 || !mp_desc) return ORBFE_ERR_INVALID_ARG;
    if (cand_count > 0 && cand_count <= cand_cap && (!cand_idx || !kf_desc)) return ORBFE_ERR_INVALID_ARG;
    return fuse_select_host(cand_idx, cand_count, cand_cap, kf_desc, n_kf, mp_desc, best_idx, best_dist);
}

int orbfe_match_triangulation_batch(orbfe_handle* h, const orbfe_keyframe* kf1, const uint8_t* has_mp1, int K,
                                    const orbfe_keyframe* const* kf2, const uint8_t* const* has_mp2,
                                    const orbfe_tri_params* params, int* raw_match12, uint8_t* raw_bin)
{
    if (!h || !kf1 || K < 0 || K > 4096 || (K > 0 && (!kf2 || !has_mp2 || !params)) ||
        (kf1->k->n > 0 && K > 0 && (!has_mp1 || !raw_match12 || !raw_bin)))
        return ORBFE_ERR_INVALID_ARG;
    std::vector<const orbfe::KeyFrameDev*> k2((size_t)K);
    for (int k = 0; k < K; k++) {
        if (!kf2[k] || kf2[k]->device != h->device) return ORBFE_ERR_INVALID_ARG;
        k2[(size_t)k] = kf2[k]->k;
    }
    if (kf1->device != h->device) return ORBFE_ERR_INVALID_ARG;
    return match_call(h, nullptr, [&](hipStream_t s, std::string& err) {
        return match_triangulation_batch_run(h->match, s, kf1->k, has_mp1, K, k2.data(), has_mp2, params, raw_match12, raw_bin, err);
    });
}

int orbfe_create_new_points_batch(orbfe_handle* h, const orbfe_keyframe* kf1, const uint8_t* has_mp1, int K,
                                  const orbfe_keyframe* const* kf2, const uint8_t* const* has_mp2,
                                  const orbfe_tri_params* tri_params, const orbfe_newpoint_params* np_params, int* raw_match12,
                                  uint8_t* raw_bin, float* x3d_out, uint8_t* verdict_out)
{
    if (!h || !kf1 || K < 0 || K > 4096 || (K > 0 && (!kf2 || !has_mp2 || !tri_params || !np_params)) ||
        (kf1->k->n > 0 && K > 0 && (!has_mp1 || !raw_match12 || !raw_bin || !x3d_out || !verdict_out)))
        return ORBFE_ERR_INVALID_ARG;
    std::vector<const orbfe::KeyFrameDev*> k2((size_t)K);
    for (int k = 0; k < K; k++) {
        if (!kf2[k] || kf2[k]->device != h->device || kf2[k]->owner != h) return ORBFE_ERR_INVALID_ARG;
        if (np_params[k].struct_size != (int)sizeof(orbfe_newpoint_params)) return ORBFE_ERR_INVALID_ARG;
        k2[(size_t)k] = kf2[k]->k;
    }
    if (kf1->device != h->device || kf1->owner != h) return ORBFE_ERR_INVALID_ARG;
    return match_call(h, nullptr, [&](hipStream_t s, std::string& err) {
        return match_triangulation_batch_run(h->match, s, kf1->k, has_mp1, K, k2.data(), has_mp2, tri_params, raw_match12, raw_bin, err,
                                             np_params, x3d_out, verdict_out);
    });
}

int orbfe_triangulate_pairs(orbfe_handle* h, const orbfe_keyframe* kf1, const orbfe_keyframe* kf2,
                            const orbfe_newpoint_params* np_params, int n_pairs, const int* idx1, const int* idx2, float* x3d_out,
                            uint8_t* verdict_out)
{
    if (!h || !kf1 || !kf2 || !np_params || n_pairs < 0 || (n_pairs > 0 && (!idx1 || !idx2 || !x3d_out || !verdict_out)))
        return ORBFE_ERR_INVALID_ARG;
    if (np_params->struct_size != (int)sizeof(orbfe_newpoint_params)) return ORBFE_ERR_INVALID_ARG;
    if (kf1->device != h->device || kf2->device != h->device || kf1->owner != h || kf2->owner != h) return ORBFE_ERR_INVALID_ARG;
    return match_call(h, nullptr, [&](hipStream_t s, std::string& err) {
        return triangulate_pairs_run(h->match, s, kf1->k, kf2->k, np_params, n_pairs, idx1, idx2, x3d_out, verdict_out, err);
    });
}

int orbfe_two_view_reconstruct(orbfe_handle* h, const orbfe_two_view_params* p, int n1, const orbfe_keypoint* kp1, int n2,
                               const orbfe_keypoint* kp2, const int* matches12, const int* sets, int* reconstructed, float* R21,
                               float* t21, float* p3d, uint8_t* triangulated, orbfe_two_view_info* info)
{
    if (!h || !p || n1 < 0 || n2 < 0 || !reconstructed || !R21 || !t21 || (n1 > 0 && (!kp1 || !matches12 || !p3d || !triangulated)) ||
        (n2 > 0 && !kp2))
        return ORBFE_ERR_INVALID_ARG;
    return match_call(h, nullptr, [&](hipStream_t s, std::string& err) {
        return two_view_run(h->match, s, p, n1, kp1, n2, kp2, matches12, sets, reconstructed, R21, t21, p3d, triangulated, info, err);
    });
}

int orbfe_mlpnp_plan(const orbfe_mlpnp_params* p, int N, int* min_inliers, int* max_its, int* total_iterations)
{
    if (!p || !min_inliers || !max_its || !total_iterations) return ORBFE_ERR_INVALID_ARG;
    return mlpnp_plan(p, N, min_inliers, max_its, total_iterations);
}

int orbfe_mlpnp_ransac(orbfe_handle* h, const orbfe_mlpnp_params* p, int n, const orbfe_keypoint* kp, const int* mp_index, int n_points,
                       const float* points, const int* sets, int n_sets, int* solved, float* Tcw, uint8_t* inliers, int* n_inliers,
                       int* no_more, orbfe_mlpnp_info* info)
{
    if (!h || !p || n < 0 || n_points < 0 || n_sets < 0 || !solved || !Tcw || !n_inliers || !no_more ||
        (n > 0 && (!kp || !mp_index || !inliers)) || (n_points > 0 && !points))
        return ORBFE_ERR_INVALID_ARG;
    return match_call(h, nullptr, [&](hipStream_t s, std::string& err) {
        return mlpnp_run(h->match, s, p, h->sig2, h->nLevels, n, kp, mp_index, n_points, points, sets, n_sets, solved, Tcw, inliers,
                         n_inliers, no_more, info, err);
    });
}

int orbfe_pose_optimization(orbfe_handle* h, const orbfe_pose_opt_params* p, int n, const orbfe_keypoint* kp, const int* mp_index,
                            int n_points, const float* points, const float* Rcw, const float* tcw, float* Tcw_out, uint8_t* outlier_out,
                            int* n_inliers, orbfe_pose_opt_info* info)
{
    if (!p) return ORBFE_ERR_INVALID_ARG;
    std::string err;
    int rc = pose_opt_check(p, info, err);  // struct sizes, unsupported branches and ranges need no handle
    if (rc == ORBFE_OK && (!h || n < 0 || n_points < 0 || !Rcw || !tcw || !Tcw_out || !n_inliers ||
                           (n > 0 && (!kp || !mp_index || !outlier_out)) || (n_points > 0 && !points)))
        return ORBFE_ERR_INVALID_ARG;
    if (!h) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    std::vector<int> first;
    // the other refusals and the return for fewer than 3 matches (:949) read the handle's level count only: the device is not touched
    if (rc == ORBFE_OK) rc = pose_opt_begin(p, h->nLevels, n, kp, mp_index, n_points, Rcw, tcw, Tcw_out, outlier_out, n_inliers, info, first, err);
    if (rc != ORBFE_OK) {
        h->err = err;
        return rc;
    }
    if (first.size() < 3) return ORBFE_OK;
    return match_call_locked(h, nullptr, [&](hipStream_t s, std::string& e) {
        return pose_opt_run(h->match, s, p, h->invSig2, h->nLevels, n, kp, mp_index, points, Rcw, tcw, first, Tcw_out, outlier_out, n_inliers,
                            info, e);
    });
}

int orbfe_pose_optimization_batch_device(orbfe_handle* h, const orbfe_pose_opt_params* p, int batch, const orbfe_keypoint* d_kp,
                                         const int* d_n, int kp_stride, const int* d_match, int n_map_points,
                                         const orbfe_world_point* d_points, int point_stride_frames, const float* d_pose_in,
                                         float* d_pose_out, uint8_t* d_outlier, int* d_n_inliers, void* stream_)
{
    if (!p) return ORBFE_ERR_INVALID_ARG;
    std::string err;
    const int crc = pose_opt_check(p, nullptr, err);
    if (crc != ORBFE_OK) return refuse(h, crc, err, kReplace);
    if (!h || batch < 1 || !d_kp || !d_n || kp_stride < 1 || !d_match || n_map_points < 0 || (n_map_points > 0 && !d_points) ||
        point_stride_frames < 0 || !d_pose_in || !d_pose_out || !d_outlier || !d_n_inliers)
        return ORBFE_ERR_INVALID_ARG;
    return match_call(h, (hipStream_t)stream_, [&](hipStream_t s, std::string& e) {
        return pose_opt_batch_device(h->match, s, p, h->invSig2, h->nLevels, batch, d_kp, d_n, kp_stride, d_match, n_map_points, d_points,
                                     point_stride_frames, d_pose_in, d_pose_out, d_outlier, d_n_inliers, e);
    });
}

// the inertial solvers' state as they read it, in[kImuStateIn], and as they write it, out[kImuState]
static void pack_imu_state(float* in, const float* Rcw, const float* tcw, const float* Rwb, const float* twb, const float* v, const float* bg,
                           const float* ba)
{
    memcpy(in, Rcw, 9 * sizeof(float));
    memcpy(in + 9, tcw, 3 * sizeof(float));
    memcpy(in + 12, Rwb, 9 * sizeof(float));
    memcpy(in + 21, twb, 3 * sizeof(float));
    memcpy(in + 24, v, 3 * sizeof(float));
    memcpy(in + 27, bg, 3 * sizeof(float));
    memcpy(in + 30, ba, 3 * sizeof(float));
}

static void unpack_imu_state(const float* out, float* Rwb, float* twb, float* v, float* bg, float* ba)
{
    memcpy(Rwb, out, 9 * sizeof(float));
    memcpy(twb, out + 9, 3 * sizeof(float));
    memcpy(v, out + 12, 3 * sizeof(float));
    memcpy(bg, out + 15, 3 * sizeof(float));
    memcpy(ba, out + 18, 3 * sizeof(float));
}

int orbfe_pose_inertial_optimization_last_keyframe(orbfe_handle* h, const orbfe_pose_inertial_params* p, const orbfe_imu_link* link,
                                                   int n, const orbfe_keypoint* kp, const int* mp_index, int n_points,
                                                   const float* points, const float* track_depth, const float* Rcw, const float* tcw,
                                                   const float* Rwb, const float* twb, const float* v, const float* bg, const float* ba,
                                                   float* Rwb_out, float* twb_out, float* v_out, float* bg_out, float* ba_out,
                                                   double* H_out, uint8_t* outlier_out, int* n_inliers, orbfe_pose_inertial_info* info)
{
    if (!p) return ORBFE_ERR_INVALID_ARG;
    std::string err;
    int rc = pose_imu_check(p, link, info, err);  // struct sizes, unsupported branches and ranges need no handle
    if (rc == ORBFE_OK && (!h || !link || n < 0 || n_points < 0 || !Rcw || !tcw || !Rwb || !twb || !v || !bg || !ba || !Rwb_out ||
                           !twb_out || !v_out || !bg_out || !ba_out || !H_out || !n_inliers ||
                           (n > 0 && (!kp || !mp_index || !outlier_out)) || (n_points > 0 && (!points || !track_depth))))
        return ORBFE_ERR_INVALID_ARG;
    if (!h) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    std::vector<int> first;
    // the other refusals read the handle's level count only: the device is not touched
    if (rc == ORBFE_OK) rc = pose_imu_begin(p, link, h->nLevels, n, kp, mp_index, n_points, info, first, err);
    if (rc != ORBFE_OK) {
        h->err = err;
        return rc;
    }
    return match_call_locked(h, nullptr, [&](hipStream_t s, std::string& e) {
        float in[kImuStateIn], out[kImuState];
        pack_imu_state(in, Rcw, tcw, Rwb, twb, v, bg, ba);
        const int r = pose_imu_run(h->match, s, p, link, h->invSig2, h->nLevels, n, kp, mp_index, points, track_depth, in, first, out, H_out,
                                   outlier_out, n_inliers, info, e);
        if (r == ORBFE_OK) unpack_imu_state(out, Rwb_out, twb_out, v_out, bg_out, ba_out);
        return r;
    });
}

int orbfe_pose_inertial_optimization_batch_device(orbfe_handle* h, const orbfe_pose_inertial_params* p, int batch,
                                                  const orbfe_imu_link* d_links, const orbfe_keypoint* d_kp, const int* d_n,
                                                  int kp_stride, const int* d_match, int n_map_points,
                                                  const orbfe_world_point* d_points, int point_stride_frames,
                                                  const float* d_track_depth, const float* d_state_in, float* d_state_out,
                                                  double* d_H_out, uint8_t* d_outlier, int* d_n_inliers, void* stream_)
{
    if (!p) return ORBFE_ERR_INVALID_ARG;
    std::string err;
    const int crc = pose_imu_check(p, nullptr, nullptr, err);
    if (crc != ORBFE_OK) return refuse(h, crc, err, kReplace);
    if (!h || batch < 1 || !d_links || !d_kp || !d_n || kp_stride < 1 || !d_match || n_map_points < 0 ||
        (n_map_points > 0 && (!d_points || !d_track_depth)) || point_stride_frames < 0 || !d_state_in || !d_state_out || !d_H_out ||
        !d_outlier || !d_n_inliers)
        return ORBFE_ERR_INVALID_ARG;
    return match_call(h, (hipStream_t)stream_, [&](hipStream_t s, std::string& e) {
        return pose_imu_batch_device(h->match, s, p, h->invSig2, h->nLevels, batch, d_links, d_kp, d_n, kp_stride, d_match, n_map_points,
                                     d_points, point_stride_frames, d_track_depth, d_state_in, d_state_out, d_H_out, d_outlier, d_n_inliers, e);
    });
}

int orbfe_pose_inertial_optimization_last_frame(orbfe_handle* h, const orbfe_pose_inertial_prev_params* p,
                                                const orbfe_imu_link_free* link, const orbfe_pose_imu_prior* prior, int n,
                                                const orbfe_keypoint* kp, const int* mp_index, int n_points, const float* points,
                                                const float* track_depth, const float* Rcw, const float* tcw, const float* Rwb,
                                                const float* twb, const float* v, const float* bg, const float* ba, float* Rwb_out,
                                                float* twb_out, float* v_out, float* bg_out, float* ba_out, double* H30_out,
                                                double* Hprior_out, uint8_t* outlier_out, int* n_inliers, int* accepted,
                                                orbfe_pose_inertial_prev_info* info)
{
    if (!p) return ORBFE_ERR_INVALID_ARG;
    std::string err;
    int rc = pose_prev_check(p, link, prior, info, err);  // struct sizes, unsupported branches and ranges need no handle
    if (rc == ORBFE_OK && (!h || !link || !prior || n < 0 || n_points < 0 || !Rcw || !tcw || !Rwb || !twb || !v || !bg || !ba || !Rwb_out ||
                           !twb_out || !v_out || !bg_out || !ba_out || !H30_out || !n_inliers || !accepted ||
                           (n > 0 && (!kp || !mp_index || !outlier_out)) || (n_points > 0 && (!points || !track_depth))))
        return ORBFE_ERR_INVALID_ARG;
    if (!h) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    std::vector<int> first;
    // the other refusals read the handle's level count only: the device is not touched
    if (rc == ORBFE_OK) rc = pose_prev_begin(p, link, prior, h->nLevels, n, kp, mp_index, n_points, info, first, err);
    if (rc != ORBFE_OK) {
        h->err = err;
        return rc;
    }
    return match_call_locked(h, nullptr, [&](hipStream_t s, std::string& e) {
        float in[kImuStateIn], out[kImuState];
        pack_imu_state(in, Rcw, tcw, Rwb, twb, v, bg, ba);
        const int r = pose_prev_run(h->match, s, p, link, prior, h->invSig2, h->nLevels, n, kp, mp_index, points, track_depth, in, first, out,
                                    H30_out, Hprior_out, outlier_out, n_inliers, accepted, info, e);
        if (r == ORBFE_OK) unpack_imu_state(out, Rwb_out, twb_out, v_out, bg_out, ba_out);
        return r;
    });
}

int orbfe_pose_inertial_optimization_last_frame_batch_device(orbfe_handle* h, const orbfe_pose_inertial_prev_params* p, int batch,
                                                             const orbfe_imu_link_free* d_links, const orbfe_pose_imu_prior* d_priors,
                                                             const orbfe_keypoint* d_kp, const int* d_n, int kp_stride,
                                                             const int* d_match, int n_map_points, const orbfe_world_point* d_points,
                                                             int point_stride_frames, const float* d_track_depth,
                                                             const float* d_state_in, float* d_state_out, double* d_H30_out,
                                                             double* d_Hprior_out, uint8_t* d_outlier, int* d_n_inliers,
                                                             int* d_accepted, void* stream_)
{
    if (!p) return ORBFE_ERR_INVALID_ARG;
    std::string err;
    const int crc = pose_prev_check(p, nullptr, nullptr, nullptr, err);
    if (crc != ORBFE_OK) return refuse(h, crc, err, kReplace);
    if (!h || batch < 1 || !d_links || !d_priors || !d_kp || !d_n || kp_stride < 1 || !d_match || n_map_points < 0 ||
        (n_map_points > 0 && (!d_points || !d_track_depth)) || point_stride_frames < 0 || !d_state_in || !d_state_out || !d_H30_out ||
        !d_outlier || !d_n_inliers || !d_accepted)
        return ORBFE_ERR_INVALID_ARG;
    return match_call(h, (hipStream_t)stream_, [&](hipStream_t s, std::string& e) {
        return pose_prev_batch_device(h->match, s, p, h->invSig2, h->nLevels, batch, d_links, d_priors, d_kp, d_n, kp_stride, d_match,
                                      n_map_points, d_points, point_stride_frames, d_track_depth, d_state_in, d_state_out, d_H30_out,
                                      d_Hprior_out, d_outlier, d_n_inliers, d_accepted, e);
    });
}

int orbfe_marginalize_pose_imu(const double* H, double* Hp)
{
    if (!H || !Hp) return ORBFE_ERR_INVALID_ARG;
    orbfe::SeqExec X;
    orbfe::MargWork W;
    orbfe::marginalize_run(X, W, H, Hp);
    return ORBFE_OK;
}

int orbfe_imu_preintegrate_frame(orbfe_handle* h, const orbfe_imu_noise* noise, int n_samples, const orbfe_imu_sample* samples,
                                 double t_prev, double t_cur, const float* frame_bias, orbfe_imu_preint* kf, orbfe_imu_preint* frame,
                                 orbfe_imu_step* steps_out, int* n_steps)
{
    if (!noise || !kf || !frame || !n_steps || !frame_bias || n_samples < 0 || (n_samples > 0 && !samples)) return ORBFE_ERR_INVALID_ARG;
    std::string err;
    // *frame is written whole when there is a step; its size field is checked all the same: it says what the caller compiled against
    const int crc = imu_check(noise, nullptr, kf, frame, err);
    if (crc != ORBFE_OK) return refuse(h, crc, err, kKeep);
    if (!h) return ORBFE_ERR_INVALID_ARG;
    if (n_samples < 2) {   // (:235-238)
        *n_steps = 0;
        return ORBFE_OK;
    }
    return match_call(h, nullptr, [&](hipStream_t s, std::string& e) {
        return imu_preintegrate_run(h->match, s, noise, n_samples, samples, t_prev, t_cur, frame_bias, kf, frame, steps_out, n_steps, e);
    });
}

int orbfe_imu_reintegrate(orbfe_handle* h, const orbfe_imu_noise* noise, const float* bias, int n_steps, const orbfe_imu_step* steps,
                          orbfe_imu_preint* out)
{
    if (!noise || !bias || !out || n_steps < 0 || (n_steps > 0 && !steps)) return ORBFE_ERR_INVALID_ARG;
    std::string err;
    const int crc = imu_check(noise, nullptr, nullptr, nullptr, err);
    if (crc != ORBFE_OK) return refuse(h, crc, err, kKeep);
    if (!h) return ORBFE_ERR_INVALID_ARG;
    return match_call(h, nullptr, [&](hipStream_t s, std::string& e) { return imu_reintegrate_run(h->match, s, noise, bias, n_steps, steps, out, e); });
}

int orbfe_imu_predict(orbfe_handle* h, const orbfe_imu_predict_params* p, const float* state1, const orbfe_imu_preint* kf,
                      const orbfe_imu_preint* frame, float* state_out, void* link_out, int* info_ok)
{
    if (!p || !state1 || !kf || !state_out || !link_out || !info_ok) return ORBFE_ERR_INVALID_ARG;
    std::string err;
    const int crc = imu_check(nullptr, p, kf, frame, err);
    if (crc != ORBFE_OK) return refuse(h, crc, err, kKeep);
    if (!h || (p->which == ORBFE_IMU_FROM_FRAME && !frame)) return ORBFE_ERR_INVALID_ARG;
    return match_call(h, nullptr, [&](hipStream_t s, std::string& e) { return imu_predict_run(h->match, s, p, state1, kf, frame, state_out, link_out, info_ok, e); });
}

int orbfe_imu_frame_batch_device(orbfe_handle* h, const orbfe_imu_noise* noise, const orbfe_imu_predict_params* p, int batch,
                                 const orbfe_imu_sample* d_samples, const int* sample_off, const double* d_t_prev, const double* d_t_cur,
                                 const float* d_frame_bias, const float* d_state1, orbfe_imu_preint* d_kf, orbfe_imu_preint* d_frame,
                                 orbfe_imu_step* d_steps_out, float* d_state_in, void* d_links, int* d_info_ok, void* stream_)
{
    if (!noise || !p) return ORBFE_ERR_INVALID_ARG;
    std::string err;
    const int crc = imu_check(noise, p, nullptr, nullptr, err);
    if (crc != ORBFE_OK) return refuse(h, crc, err, kKeep);
    if (imu_check_offsets(batch, sample_off) != ORBFE_OK) return ORBFE_ERR_INVALID_ARG;
    if (!h || !d_samples || !d_t_prev || !d_t_cur || !d_frame_bias || !d_state1 || !d_kf || !d_frame || !d_state_in || !d_links || !d_info_ok)
        return ORBFE_ERR_INVALID_ARG;
    return match_call(h, (hipStream_t)stream_, [&](hipStream_t s, std::string& e) {
        return imu_frame_batch_device(h->match, s, noise, p, batch, d_samples, sample_off, d_t_prev, d_t_cur, d_frame_bias, d_state1, d_kf, d_frame,
                                      d_steps_out, d_state_in, d_links, d_info_ok, e);
    });
}

int orbfe_imu_reintegrate_batch_device(orbfe_handle* h, const orbfe_imu_noise* noise, int batch, const orbfe_imu_step* d_steps,
                                       const int* step_off, const float* d_bias, orbfe_imu_preint* d_out, void* stream_)
{
    if (!noise) return ORBFE_ERR_INVALID_ARG;
    std::string err;
    const int crc = imu_check(noise, nullptr, nullptr, nullptr, err);
    if (crc != ORBFE_OK) return refuse(h, crc, err, kKeep);
    if (imu_check_offsets(batch, step_off) != ORBFE_OK) return ORBFE_ERR_INVALID_ARG;
    if (!h || !d_steps || !d_bias || !d_out) return ORBFE_ERR_INVALID_ARG;
    return match_call(h, (hipStream_t)stream_, [&](hipStream_t s, std::string& e) {
        return imu_reintegrate_batch_device(h->match, s, noise, batch, d_steps, step_off, d_bias, d_out, e);
    });
}

// ---- Tracking::UpdateLocalMap from a resident covisibility graph (SPEC DECISION S24) ----

int orbfe_covis_create(orbfe_handle* h, const orbfe_map* map, int kf_capacity, int kf_stride, int obs_stride, int child_stride,
                       orbfe_covis** out)
{
    if (!h || !out || !map || map->h != h || kf_capacity < 1 || kf_capacity > kCovisMaxKf || kf_stride < 1 || kf_stride > kCovisMaxKfStride ||
        obs_stride < 1 || obs_stride > kCovisMaxShort || child_stride < 1 || child_stride > kCovisMaxShort)
        return ORBFE_ERR_INVALID_ARG;
    *out = nullptr;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    orbfe_covis* g = new (std::nothrow) orbfe_covis();
    if (!g) return ORBFE_ERR_OUT_OF_MEMORY;
    g->h = h;
    g->map = map;
    CovisTables& T = g->T;
    T.kfCap = kf_capacity;
    T.kfStride = kf_stride;
    T.obsStride = obs_stride;
    T.childStride = child_stride;
    T.cap = map->cap;
    const size_t K = (size_t)kf_capacity, C = (size_t)map->cap;
    if (hipMalloc(&T.kf, K * sizeof(CovisKf)) != hipSuccess || hipMalloc(&T.covisible, K * ORBFE_COVIS_MAX_COVISIBLE * sizeof(int)) != hipSuccess ||
        hipMalloc(&T.children, K * child_stride * sizeof(int)) != hipSuccess || hipMalloc(&T.kfPoints, K * kf_stride * sizeof(int)) != hipSuccess ||
        hipMalloc(&T.obsCount, C * sizeof(int)) != hipSuccess || hipMalloc(&T.obs, C * obs_stride * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        covis_free(g);
        delete g;
        h->err = "orbfe_covis_create: allocation failed";
        return ORBFE_ERR_OUT_OF_MEMORY;
    }
    std::string err;
    int rc = covis_init_launch(h->stream, T, err);
    if (rc == ORBFE_OK && hipStreamSynchronize(h->stream) != hipSuccess) {
        err = "orbfe_covis_create: hipStreamSynchronize failed";
        rc = ORBFE_ERR_HIP;
    }
    if (rc != ORBFE_OK) {
        (void)hipGetLastError();
        covis_free(g);
        delete g;
        h->err = err;
        return rc;
    }
    h->covis.push_back(g);
    *out = g;
    return ORBFE_OK;
}

void orbfe_covis_destroy(orbfe_covis* g)
{
    if (!g) return;
    if (g->h) {  // (null: the handle went first, orphan_children)
        orbfe_handle* h = g->h;
        std::lock_guard<std::mutex> lk(h->mu);
        for (size_t i = 0; i < h->covis.size(); i++)
            if (h->covis[i] == g) h->covis.erase(h->covis.begin() + (long)i--);
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
        if (h->matchUsed) (void)hipEventSynchronize(h->evMatch);  // a call on another stream
        covis_free(g);
    }
    delete g;
}

}  // extern "C"

// the inputs of st filled, `bytes` of them up, run() behind them, synchronised: what the two setters share; the caller holds nothing
template <class Fill, class Run>
static int covis_staged_call(orbfe_handle* h, Staging& st, size_t bytes, Fill fill, Run run)
{
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    std::string err;
    MatchScope scope_(h, h->stream);
    if (scope_.rc != ORBFE_OK) return scope_.rc;
    int rc = reserve(h->match, st, err);
    if (rc != ORBFE_OK) {
        h->err = err;
        return rc;
    }
    fill();
    HIPCHK(h, hipMemcpyAsync(st.dp, st.hp, bytes, hipMemcpyHostToDevice, h->stream));
    rc = run(err);
    if (rc != ORBFE_OK) {
        h->err = err;
        return rc;
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return ORBFE_OK;
}

extern "C" {

int orbfe_covis_set_keyframes(orbfe_handle* h, orbfe_covis* g, int n, const orbfe_covis_keyframe* recs)
{
    if (!h || !g || g->h != h || !g->map || n < 0 || (n > 0 && !recs)) return ORBFE_ERR_INVALID_ARG;
    const CovisTables& T = g->T;
    auto slot_or_none = [&](int s) { return s >= -1 && s < T.kfCap; };
    std::vector<char> seen((size_t)T.kfCap, 0);
    size_t ints = (size_t)n * (sizeof(CovisStagedKf) / sizeof(int));
    for (int i = 0; i < n; i++) {
        const orbfe_covis_keyframe& r = recs[i];
        if (r.struct_size != (int)sizeof(orbfe_covis_keyframe)) {
            std::lock_guard<std::mutex> lk(h->mu);
            h->err = "orbfe_covis_keyframe.struct_size does not match this library (rebuild the caller against include/orbfe.h)";
            return ORBFE_ERR_INVALID_ARG;
        }
        if (r.slot < 0 || r.slot >= T.kfCap || seen[(size_t)r.slot] || r.mn_id < 0 || !slot_or_none(r.parent) || !slot_or_none(r.prev) ||
            r.n_covisible < 0 || r.n_covisible > ORBFE_COVIS_MAX_COVISIBLE || r.n_children < 0 || r.n_children > T.childStride ||
            (r.n_covisible > 0 && !r.covisible) || (r.n_children > 0 && !r.children) ||
            (r.point_ids && (r.n_features < 0 || r.n_features > T.kfStride)))
            return ORBFE_ERR_INVALID_ARG;
        seen[(size_t)r.slot] = 1;
        for (int j = 0; j < r.n_covisible; j++)
            if (!slot_or_none(r.covisible[j])) return ORBFE_ERR_INVALID_ARG;
        for (int j = 0; j < r.n_children; j++)
            if (!slot_or_none(r.children[j])) return ORBFE_ERR_INVALID_ARG;
        ints += (size_t)(r.point_ids ? r.n_features : 0) + (size_t)r.n_covisible + (size_t)r.n_children;
    }
    if (n == 0) return ORBFE_OK;
    if (ints > (size_t)0x7fffffff) return ORBFE_ERR_INVALID_ARG;  // offsets are ints: split the call
    Staging stg;
    const auto bBlk = stg.in<int>(ints);  // [n records | their lists]: the records hold offsets in ints from the start of the block
    return covis_staged_call(
        h, stg, bBlk.bytes(),
        [&]() {
            int* blk = stg.host(bBlk);
            CovisStagedKf* st = reinterpret_cast<CovisStagedKf*>(blk);  // the head of the block seen as records
            size_t at = (size_t)n * (sizeof(CovisStagedKf) / sizeof(int));
            for (int i = 0; i < n; i++) {
                const orbfe_covis_keyframe& r = recs[i];
                const int nf = r.point_ids ? r.n_features : -1;
                st[i] = CovisStagedKf{r.slot, r.mn_id, r.bad != 0, r.parent, r.prev, nf, r.n_covisible, r.n_children, 0, 0, 0, 0};
                st[i].oPoints = (int)at;
                if (nf > 0) memcpy(blk + at, r.point_ids, (size_t)nf * sizeof(int));
                at += (size_t)std::max(nf, 0);
                st[i].oCovisible = (int)at;
                if (r.n_covisible > 0) memcpy(blk + at, r.covisible, (size_t)r.n_covisible * sizeof(int));
                at += (size_t)r.n_covisible;
                st[i].oChildren = (int)at;
                if (r.n_children > 0) memcpy(blk + at, r.children, (size_t)r.n_children * sizeof(int));
                at += (size_t)r.n_children;
            }
        },
        [&](std::string& err) { return covis_scatter_keyframes_launch(h->stream, T, n, stg.dev(bBlk), err); });
}

}  // extern "C"

// both observation setters; feat_idx: null for the form without indices, which on a graph with refresh state writes -1 (S26)
static int covis_set_observations(orbfe_handle* h, orbfe_covis* g, int n, const int* ids, const int* off, const int* kf_slots,
                                  const int* feat_idx, bool indexed)
{
    if (!h || !g || g->h != h || !g->map || n < 0 || (n > 0 && (!ids || !off))) return ORBFE_ERR_INVALID_ARG;
    if (indexed && g->R.nLevels == 0) return ORBFE_ERR_INVALID_ARG;
    const CovisTables& T = g->T;
    if (!refresh_observations_ok(RefreshDims{T.kfCap, T.kfStride, T.obsStride, T.cap, g->R.nLevels}, n, ids, off, kf_slots, feat_idx, indexed))
        return ORBFE_ERR_INVALID_ARG;
    if (n == 0) return ORBFE_OK;
    Staging st;
    const ObservationsStage B(st, n, off, indexed);
    const auto bIds = B.ids, bOff = B.off, bSlots = B.slots, bIdx = B.idx;
    return covis_staged_call(
        h, st, st.inBytes, [&]() { B.fill(st, ids, off, kf_slots, feat_idx); },
        [&](std::string& err) {
            const int rc = covis_scatter_observations_launch(h->stream, T, n, st.dev(bIds), st.dev(bOff), st.dev(bSlots), err);
            if (rc != ORBFE_OK || g->R.nLevels == 0) return rc;
            return covis_scatter_indices_launch(h->stream, T, g->R, n, st.dev(bIds), st.dev(bOff), indexed ? st.dev(bIdx) : nullptr, err);
        });
}

extern "C" {

int orbfe_covis_set_observations(orbfe_handle* h, orbfe_covis* g, int n, const int* ids, const int* off, const int* kf_slots)
{
    return covis_set_observations(h, g, n, ids, off, kf_slots, nullptr, false);
}

// what the arguments alone decide, for both per-frame calls: no handle is looked at
static int local_map_refuse(const orbfe_local_map_params* p, int batch, int vote_stride, const orbfe_covis* g, int M, std::string& err)
{
    if (!p) return ORBFE_ERR_INVALID_ARG;
    const int crc = local_map_check(p, err);
    if (crc != ORBFE_OK) return crc;
    if (batch < 1 || vote_stride < 1 || M < 1 || !g) return ORBFE_ERR_INVALID_ARG;
    return ORBFE_OK;
}

// the scratch for `batch` frames, left at rest; the caller holds h->mu.  Grows only: a call allocates when its batch is the largest so far.
static int covis_scratch(orbfe_handle* h, orbfe_covis* g, int batch, hipStream_t s, std::string& err)
{
    if (batch <= g->scratchBatch) return ORBFE_OK;
    const size_t stamps = (size_t)batch * g->T.cap, counters = (size_t)batch * ((size_t)g->T.kfCap + 1);
    if (stamps > kCovisMaxStamps) {
        err = "orbfe_update_local_map: batch x map capacity exceeds the 2^28 first-occurrence stamps of one call";
        return ORBFE_ERR_OUT_OF_MEMORY;
    }
    // the blocks in use may still be read by a call in flight on another stream: hipFree waits for the device
    if (g->dStamps) (void)hipFree(g->dStamps);
    if (g->dCounters) (void)hipFree(g->dCounters);
    g->dStamps = nullptr;
    g->dCounters = nullptr;
    g->scratchBatch = 0;
    if (hipMalloc(&g->dStamps, stamps * sizeof(unsigned)) != hipSuccess || hipMalloc(&g->dCounters, counters * sizeof(int)) != hipSuccess) {
        (void)hipGetLastError();
        if (g->dStamps) (void)hipFree(g->dStamps);
        g->dStamps = nullptr;
        err = "orbfe_update_local_map: allocation of the per-frame scratch failed";
        return ORBFE_ERR_OUT_OF_MEMORY;
    }
    MCHK(hipMemsetAsync(g->dStamps, 0xff, stamps * sizeof(unsigned), s));
    MCHK(hipMemsetAsync(g->dCounters, 0, counters * sizeof(int), s));
    g->scratchBatch = batch;
    return ORBFE_OK;
}

int orbfe_update_local_map_batch_device(orbfe_handle* h, const orbfe_local_map_params* p, int batch, int vote_stride, orbfe_covis* g,
                                        int n_points, const orbfe_local_map_io* io, void* stream_)
{
    std::string err;
    int crc = local_map_refuse(p, batch, vote_stride, g, n_points, err);
    if (crc == ORBFE_OK && !io) crc = ORBFE_ERR_INVALID_ARG;
    if (crc == ORBFE_OK && io->struct_size != (int)sizeof(orbfe_local_map_io)) {
        err = "orbfe_local_map_io.struct_size does not match this library (rebuild the caller against include/orbfe.h)";
        crc = ORBFE_ERR_INVALID_ARG;
    }
    if (crc != ORBFE_OK) return refuse(h, crc, err, kKeep);
    if (!io->d_vote_ids || !io->d_n_votes || (p->inertial != 0 && !io->d_last_kf) || !io->d_ids_out || !io->d_n_local_points ||
        !io->d_local_kfs || !io->d_n_local_kfs)
        return ORBFE_ERR_INVALID_ARG;
    if (!h || g->h != h || !g->map) return ORBFE_ERR_INVALID_ARG;
    return match_call(h, (hipStream_t)stream_, [&](hipStream_t s, std::string& e) -> int {
        const int rc = covis_scratch(h, g, batch, s, e);
        if (rc != ORBFE_OK) return rc;
        return local_map_launch(s, p, batch, vote_stride, g->T, g->map->dPts, n_points, io, g->dStamps, g->dCounters, e);
    });
}

int orbfe_update_local_map(orbfe_handle* h, const orbfe_local_map_params* p, int n_votes, const int* vote_ids, int last_kf, orbfe_covis* g,
                           int n_points, int* ids_out, int* n_local_points, int* local_kfs, int* n_local_kfs, int* vote_ids_out)
{
    std::string err;
    const int crc = local_map_refuse(p, 1, 1, g, n_points, err);
    if (crc != ORBFE_OK) return refuse(h, crc, err, kKeep);
    if (n_votes < 0 || (n_votes > 0 && !vote_ids) || !ids_out || !n_local_points || !local_kfs || !n_local_kfs) return ORBFE_ERR_INVALID_ARG;
    if (!h || g->h != h || !g->map) return ORBFE_ERR_INVALID_ARG;
    const int stride = std::max(n_votes, 1), M = n_points;
    // in:  [vote ids | n_votes, last_kf]      out: [ids (M) | n_local_points, n_local_kfs | local_kfs | vote ids out]
    Staging st;
    const auto bVotes = st.in<int>(stride);
    const auto bScal = st.in<int>(2);   // n_votes, last_kf
    const auto bIds = st.out<int>(M);
    const auto bCounts = st.out<int>(2);   // n_local_points, n_local_kfs
    const auto bKfs = st.out<int>(ORBFE_LOCAL_KF_MAX);
    const auto bVotesOut = st.out<int>(stride);
    return match_call(h, nullptr, [&](hipStream_t s, std::string& e) -> int {
        int rc = reserve(h->match, st, e);
        if (rc != ORBFE_OK) return rc;
        rc = covis_scratch(h, g, 1, s, e);
        if (rc != ORBFE_OK) return rc;
        st.put(bVotes, vote_ids, n_votes);
        const int scal[2] = {n_votes, last_kf};
        st.put(bScal, scal);
        if ((rc = upload(st, s, e)) != ORBFE_OK) return rc;
        orbfe_local_map_io io{};
        io.struct_size = (int)sizeof io;
        io.d_vote_ids = st.dev(bVotes);
        io.d_n_votes = st.dev(bScal);
        io.d_last_kf = io.d_n_votes + 1;
        io.d_ids_out = st.dev(bIds);
        io.d_n_local_points = st.dev(bCounts);
        io.d_n_local_kfs = io.d_n_local_points + 1;
        io.d_local_kfs = st.dev(bKfs);
        io.d_vote_ids_out = st.dev(bVotesOut);
        rc = local_map_launch(s, p, 1, stride, g->T, g->map->dPts, M, &io, g->dStamps, g->dCounters, e);
        if (rc != ORBFE_OK) return rc;
        if ((rc = download(st, s, e)) != ORBFE_OK) return rc;
        st.get(bIds, ids_out);
        *n_local_points = st.res(bCounts)[0];
        *n_local_kfs = st.res(bCounts)[1];
        st.get(bKfs, local_kfs);
        st.get(bVotesOut, vote_ids_out, n_votes);
        return ORBFE_OK;
    });
}

int orbfe_frame_points_batch_device(orbfe_handle* h, const orbfe_map* map, int batch, int kp_stride, int n_points, const int* d_ids,
                                    const int* d_match, const uint8_t* d_outlier, const int* d_n, int* d_out, void* stream_)
{
    if (!map || batch < 1 || kp_stride < 1 || kp_stride > kPoseMaxKp || n_points < 1 || !d_ids || !d_match || !d_outlier || !d_n || !d_out)
        return ORBFE_ERR_INVALID_ARG;
    if (!h || map->h != h) return ORBFE_ERR_INVALID_ARG;
    return match_call(h, (hipStream_t)stream_, [&](hipStream_t s, std::string& e) {
        return frame_points_launch(s, batch, kp_stride, n_points, map->cap, map->dPts, d_ids, d_match, d_outlier, d_n, d_out, e);
    });
}

// ---- maintaining the resident graph: KeyFrame::UpdateConnections and the graph part of ProcessNewKeyFrame (SPEC DECISION S25) ----

int orbfe_covis_enable_connections(orbfe_handle* h, orbfe_covis* g, int conn_stride)
{
    if (!h || !g || g->h != h || !g->map || conn_stride < 1 || conn_stride > kCovisMaxConnStride) return ORBFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (g->C.connStride != 0) {
        h->err = "orbfe_covis_enable_connections: the graph has its connection rows already";
        return ORBFE_ERR_INVALID_ARG;
    }
    HIPCHK(h, hipSetDevice(h->device));
    CovisConn C{};
    C.connStride = conn_stride;
    const size_t rows = (size_t)g->T.kfCap * conn_stride * sizeof(int);
    std::string err;
    int rc = ORBFE_OK;
    if (hipMalloc(&C.slots, rows) != hipSuccess || hipMalloc(&C.weights, rows) != hipSuccess ||
        hipMalloc(&C.count, (size_t)g->T.kfCap * sizeof(int)) != hipSuccess ||
        hipMalloc(&C.work, ((size_t)kWorkHead + 3 * (size_t)conn_stride) * sizeof(int)) != hipSuccess) {
        err = "orbfe_covis_enable_connections: allocation failed";
        rc = ORBFE_ERR_OUT_OF_MEMORY;
    }
    if (rc == ORBFE_OK) rc = covis_conn_init_launch(h->stream, g->T, C, err);
    if (rc == ORBFE_OK && hipStreamSynchronize(h->stream) != hipSuccess) {
        err = "orbfe_covis_enable_connections: hipStreamSynchronize failed";
        rc = ORBFE_ERR_HIP;
    }
    if (rc != ORBFE_OK) {
        (void)hipGetLastError();
        void* ptrs[] = {C.slots, C.weights, C.count, C.work};
        for (void* p : ptrs)
            if (p) (void)hipFree(p);
        h->err = err;
        return rc;
    }
    g->C = C;
    return ORBFE_OK;
}

int orbfe_covis_set_connections(orbfe_handle* h, orbfe_covis* g, int n, const int* slots, const int* off, const int* conn_slots,
                                const int* weights)
{
    if (!h || !g || g->h != h || !g->map || g->C.connStride == 0 || n < 0 || (n > 0 && (!slots || !off))) return ORBFE_ERR_INVALID_ARG;
    if (n == 0) return ORBFE_OK;
    const CovisTables& T = g->T;
    if (off[0] < 0) return ORBFE_ERR_INVALID_ARG;
    std::vector<char> seen((size_t)T.kfCap, 0);
    for (int i = 0; i < n; i++) {
        if (slots[i] < 0 || slots[i] >= T.kfCap || seen[(size_t)slots[i]] || off[i + 1] < off[i] || off[i + 1] - off[i] > g->C.connStride)
            return ORBFE_ERR_INVALID_ARG;
        seen[(size_t)slots[i]] = 1;
    }
    const int total = off[n];
    if (total > off[0] && (!conn_slots || !weights)) return ORBFE_ERR_INVALID_ARG;
    for (int k = off[0]; k < total; k++)
        if (conn_slots[k] < 0 || conn_slots[k] >= T.kfCap || weights[k] < 0) return ORBFE_ERR_INVALID_ARG;
    Staging st;
    const auto bSlots = st.in<int>(n);
    const auto bOff = st.in<int>((size_t)n + 1);
    const auto bConn = st.in<int>(std::max(total, 1));
    const auto bW = st.in<int>(std::max(total, 1));
    return covis_staged_call(
        h, st, st.inBytes,
        [&]() {
            st.put(bSlots, slots);
            st.put(bOff, off);
            st.put(bConn, conn_slots, total);
            st.put(bW, weights, total);
        },
        [&](std::string& err) {
            return covis_scatter_connections_launch(h->stream, T, g->C, n, st.dev(bSlots), st.dev(bOff), st.dev(bConn), st.dev(bW), err);
        });
}

int orbfe_covis_get_keyframe(orbfe_handle* h, orbfe_covis* g, int slot, orbfe_covis_keyframe* rec, int* covisible, int* children,
                             int* conn_slots, int* conn_weights, int* n_conn)
{
    if (!h || !g || g->h != h || !g->map || !rec || !covisible || !children || slot < 0 || slot >= g->T.kfCap) return ORBFE_ERR_INVALID_ARG;
    if (rec->struct_size != (int)sizeof(orbfe_covis_keyframe)) {
        std::lock_guard<std::mutex> lk(h->mu);
        h->err = "orbfe_covis_keyframe.struct_size does not match this library (rebuild the caller against include/orbfe.h)";
        return ORBFE_ERR_INVALID_ARG;
    }
    const bool wantConn = conn_slots || conn_weights || n_conn;
    if (wantConn && g->C.connStride == 0) return ORBFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    const CovisTables& T = g->T;
    hipStream_t s = h->stream;
    CovisKf k{};
    const size_t S = (size_t)g->C.connStride;
    HIPCHK(h, hipMemcpyAsync(&k, T.kf + slot, sizeof k, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(covisible, T.covisible + (size_t)slot * ORBFE_COVIS_MAX_COVISIBLE, ORBFE_COVIS_MAX_COVISIBLE * sizeof(int),
                             hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(children, T.children + (size_t)slot * T.childStride, (size_t)T.childStride * sizeof(int), hipMemcpyDeviceToHost, s));
    if (conn_slots) HIPCHK(h, hipMemcpyAsync(conn_slots, g->C.slots + (size_t)slot * S, S * sizeof(int), hipMemcpyDeviceToHost, s));
    if (conn_weights) HIPCHK(h, hipMemcpyAsync(conn_weights, g->C.weights + (size_t)slot * S, S * sizeof(int), hipMemcpyDeviceToHost, s));
    if (n_conn) HIPCHK(h, hipMemcpyAsync(n_conn, g->C.count + slot, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    rec->slot = slot;
    rec->mn_id = k.mnId;
    rec->bad = k.bad;
    rec->parent = k.parent;
    rec->prev = k.prev;
    rec->n_features = k.nFeatures;
    rec->n_covisible = k.nCovisible;
    rec->n_children = k.nChildren;
    rec->reserved = 0;
    rec->point_ids = rec->covisible = rec->children = nullptr;
    return ORBFE_OK;
}

// what the arguments alone decide, for both forms: no handle is looked at
static int covis_update_refuse(const orbfe_covis_update_params* p, const orbfe_covis* g, std::string& err)
{
    if (!p) return ORBFE_ERR_INVALID_ARG;
    const int crc = covis_update_check(p, err);
    if (crc != ORBFE_OK) return crc;
    if (!g) return ORBFE_ERR_INVALID_ARG;
    return ORBFE_OK;
}

int orbfe_covis_update_connections_device(orbfe_handle* h, const orbfe_covis_update_params* p, orbfe_covis* g, int n, const int* slots,
                                          const int* flags, const orbfe_covis_update_io* io, void* stream_)
{
    std::string err;
    int crc = covis_update_refuse(p, g, err);
    if (crc == ORBFE_OK && !io) crc = ORBFE_ERR_INVALID_ARG;
    if (crc == ORBFE_OK && io->struct_size != (int)sizeof(orbfe_covis_update_io)) {
        err = "orbfe_covis_update_io.struct_size does not match this library (rebuild the caller against include/orbfe.h)";
        crc = ORBFE_ERR_INVALID_ARG;
    }
    if (crc != ORBFE_OK) return refuse(h, crc, err, kKeep);
    if (n < 1 || !slots || !flags || !io->d_slots || !io->d_weights || !io->d_count || !io->d_status) return ORBFE_ERR_INVALID_ARG;
    if (!h || g->h != h || !g->map || g->C.connStride == 0) return ORBFE_ERR_INVALID_ARG;
    for (int k = 0; k < n; k++)
        if (slots[k] < 0 || slots[k] >= g->T.kfCap) return ORBFE_ERR_INVALID_ARG;
    return match_call(h, (hipStream_t)stream_, [&](hipStream_t s, std::string& e) -> int {
        int rc = covis_scratch(h, g, 1, s, e);
        for (int k = 0; k < n && rc == ORBFE_OK; k++)
            rc = covis_update_launch(s, g->T, g->C, g->map->dPts, p->min_weight, slots[k], flags[k], io->d_slots + (size_t)k * g->C.connStride,
                                     io->d_weights + (size_t)k * g->C.connStride, io->d_count + k, io->d_status + k, g->dCounters, e);
        return rc;
    });
}

int orbfe_covis_update_connections(orbfe_handle* h, const orbfe_covis_update_params* p, orbfe_covis* g, int slot, int flag,
                                   int* ordered_slots, int* ordered_weights, int* count, int* status)
{
    std::string err;
    const int crc = covis_update_refuse(p, g, err);
    if (crc != ORBFE_OK) return refuse(h, crc, err, kKeep);
    if (!ordered_slots || !ordered_weights || !count || !status) return ORBFE_ERR_INVALID_ARG;
    if (!h || g->h != h || !g->map || g->C.connStride == 0 || slot < 0 || slot >= g->T.kfCap) return ORBFE_ERR_INVALID_ARG;
    const size_t S = (size_t)g->C.connStride;
    Staging st;
    const auto bSlots = st.out<int>(S);
    const auto bWeights = st.out<int>(S);
    const auto bScal = st.out<int>(2);  // count, status
    const int rc = match_call(h, nullptr, [&](hipStream_t s, std::string& e) -> int {
        int r = reserve(h->match, st, e);
        if (r != ORBFE_OK) return r;
        if ((r = covis_scratch(h, g, 1, s, e)) != ORBFE_OK) return r;
        r = covis_update_launch(s, g->T, g->C, g->map->dPts, p->min_weight, slot, flag, st.dev(bSlots), st.dev(bWeights), st.dev(bScal),
                                st.dev(bScal) + 1, g->dCounters, e);
        if (r != ORBFE_OK) return r;
        if ((r = download(st, s, e)) != ORBFE_OK) return r;
        st.get(bSlots, ordered_slots);
        st.get(bWeights, ordered_weights);
        *count = st.res(bScal)[0];
        *status = st.res(bScal)[1];
        if (*status == ORBFE_COVIS_STATUS_REFUSED) {
            e = "orbfe_covis_update_connections: a connection row or a children row is full; the graph was left as it was";
            return ORBFE_ERR_OUT_OF_MEMORY;
        }
        return ORBFE_OK;
    });
    return rc;
}

// what both forms of add_keyframe refuse, in the header's order; k: the record the kernel writes
static int covis_add_refuse(orbfe_handle* h, const orbfe_covis* g, const orbfe_covis_keyframe* rec, int n_features, CovisKf& k)
{
    if (!rec || !g || n_features < 0) return ORBFE_ERR_INVALID_ARG;
    if (rec->struct_size != (int)sizeof(orbfe_covis_keyframe)) {
        return refuse(h, ORBFE_ERR_INVALID_ARG,
                      "orbfe_covis_keyframe.struct_size does not match this library (rebuild the caller against include/orbfe.h)", kKeep);
    }
    if (!h || g->h != h || !g->map) return ORBFE_ERR_INVALID_ARG;
    const CovisTables& T = g->T;
    auto slot_or_none = [&](int s) { return s >= -1 && s < T.kfCap; };
    if (rec->slot < 0 || rec->slot >= T.kfCap || rec->mn_id < 0 || !slot_or_none(rec->parent) || !slot_or_none(rec->prev) ||
        n_features > T.kfStride)
        return ORBFE_ERR_INVALID_ARG;
    k = CovisKf{};
    k.mnId = rec->mn_id;
    k.bad = rec->bad != 0;
    k.parent = rec->parent;
    k.prev = rec->prev;
    k.nFeatures = n_features;
    return ORBFE_OK;
}

int orbfe_covis_add_keyframe(orbfe_handle* h, orbfe_covis* g, const orbfe_covis_keyframe* rec, int* added, int* status)
{
    if (!rec || !status || (rec->n_features > 0 && (!rec->point_ids || !added))) return ORBFE_ERR_INVALID_ARG;
    CovisKf k{};
    const int crc = covis_add_refuse(h, g, rec, rec->n_features, k);
    if (crc != ORBFE_OK) return crc;
    const int n = rec->n_features;
    Staging st;
    const auto bIds = st.in<int>(std::max(n, 1));
    const auto bAdded = st.out<int>(std::max(n, 1));
    const auto bStatus = st.out<int>(1);
    return match_call(h, nullptr, [&](hipStream_t s, std::string& e) -> int {
        int rc = reserve(h->match, st, e);
        if (rc != ORBFE_OK) return rc;
        if ((rc = covis_scratch(h, g, 1, s, e)) != ORBFE_OK) return rc;
        st.put(bIds, rec->point_ids, n);
        if ((rc = upload(st, s, e)) != ORBFE_OK) return rc;
        rc = covis_add_keyframe_launch(s, g->T, g->C.connStride ? &g->C : nullptr, g->map->dPts, k, rec->slot, st.dev(bIds), st.dev(bAdded),
                                       st.dev(bStatus), g->dStamps, e);
        if (rc != ORBFE_OK) return rc;
        if (g->R.nLevels && (rc = covis_index_added_launch(s, g->T, g->R, rec->slot, n, st.dev(bIds), st.dev(bAdded), e)) != ORBFE_OK) return rc;
        if ((rc = download(st, s, e)) != ORBFE_OK) return rc;
        st.get(bAdded, added, n);
        *status = st.res(bStatus)[0];
        if (*status == ORBFE_COVIS_STATUS_REFUSED) {
            e = "orbfe_covis_add_keyframe: an observation list is full; the graph was left as it was";
            return ORBFE_ERR_OUT_OF_MEMORY;
        }
        return ORBFE_OK;
    });
}

int orbfe_covis_add_keyframe_device(orbfe_handle* h, orbfe_covis* g, const orbfe_covis_keyframe* rec, const int* d_point_ids, int n_features,
                                    int* d_added, int* d_status, void* stream_)
{
    if (!d_point_ids || !d_added || !d_status) return ORBFE_ERR_INVALID_ARG;
    CovisKf k{};
    const int crc = covis_add_refuse(h, g, rec, n_features, k);
    if (crc != ORBFE_OK) return crc;
    const CovisTables& T = g->T;
    return match_call(h, (hipStream_t)stream_, [&](hipStream_t s, std::string& e) -> int {
        int rc = covis_scratch(h, g, 1, s, e);
        if (rc != ORBFE_OK) return rc;
        rc = covis_add_keyframe_launch(s, T, g->C.connStride ? &g->C : nullptr, g->map->dPts, k, rec->slot, d_point_ids, d_added, d_status,
                                       g->dStamps, e);
        if (rc != ORBFE_OK || g->R.nLevels == 0) return rc;
        return covis_index_added_launch(s, T, g->R, rec->slot, n_features, d_point_ids, d_added, e);
    });
}

// ---- refreshing map points from the resident graph: UpdateDepth and ComputeDistinctiveDescriptors (SPEC DECISION S26) ----

int orbfe_covis_enable_refresh(orbfe_handle* h, orbfe_covis* g, int n_levels, const float* scale_factors)
{
    if (!h || !g || g->h != h || !g->map || !scale_factors || n_levels < 1 || n_levels > kRefreshMaxLevels) return ORBFE_ERR_INVALID_ARG;
    const CovisTables& T = g->T;
    const size_t rowsKf = (size_t)T.kfCap * T.kfStride;
    if (rowsKf >= ((size_t)1 << 31)) return ORBFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (g->R.nLevels != 0) {
        h->err = "orbfe_covis_enable_refresh: the graph has its refresh state already";
        return ORBFE_ERR_INVALID_ARG;
    }
    HIPCHK(h, hipSetDevice(h->device));
    CovisRefresh R{};
    R.nLevels = n_levels;
    const size_t rowsObs = (size_t)T.cap * T.obsStride;
    float sf[kRefreshMaxLevels] = {};
    memcpy(sf, scale_factors, (size_t)n_levels * sizeof(float));
    std::string err;
    int rc = ORBFE_OK;
    hipStream_t s = h->stream;
    if (hipMalloc(&R.desc, rowsKf * ORBFE_DESC_BYTES) != hipSuccess || hipMalloc(&R.octave, rowsKf) != hipSuccess ||
        hipMalloc(&R.nFeat, (size_t)T.kfCap * sizeof(int)) != hipSuccess || hipMalloc(&R.centre, (size_t)T.kfCap * 3 * sizeof(float)) != hipSuccess ||
        hipMalloc(&R.obsIdx, rowsObs * sizeof(int)) != hipSuccess || hipMalloc(&R.refKf, (size_t)T.cap * sizeof(int)) != hipSuccess ||
        hipMalloc(&R.sf, sizeof sf) != hipSuccess) {
        err = "orbfe_covis_enable_refresh: allocation failed";
        rc = ORBFE_ERR_OUT_OF_MEMORY;
    }
    // all rows empty: no features, indices and reference slots -1 (every byte 0xff)
    if (rc == ORBFE_OK &&
        (hipMemsetAsync(R.desc, 0, rowsKf * ORBFE_DESC_BYTES, s) != hipSuccess || hipMemsetAsync(R.octave, 0, rowsKf, s) != hipSuccess ||
         hipMemsetAsync(R.nFeat, 0, (size_t)T.kfCap * sizeof(int), s) != hipSuccess ||
         hipMemsetAsync(R.centre, 0, (size_t)T.kfCap * 3 * sizeof(float), s) != hipSuccess ||
         hipMemsetAsync(R.obsIdx, 0xff, rowsObs * sizeof(int), s) != hipSuccess ||
         hipMemsetAsync(R.refKf, 0xff, (size_t)T.cap * sizeof(int), s) != hipSuccess ||
         copy_sync(R.sf, sf, sizeof sf, hipMemcpyHostToDevice, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)) {
        err = "orbfe_covis_enable_refresh: initialising the rows failed";
        rc = ORBFE_ERR_HIP;
    }
    if (rc != ORBFE_OK) {
        (void)hipGetLastError();
        void* ptrs[] = {R.desc, R.octave, R.nFeat, R.centre, R.obsIdx, R.refKf, R.sf};
        for (void* p : ptrs)
            if (p) (void)hipFree(p);
        h->err = err;
        return rc;
    }
    g->R = R;
    return ORBFE_OK;
}

// what every refresh setter refuses first
static bool covis_no_refresh(const orbfe_handle* h, const orbfe_covis* g) { return !h || !g || g->h != h || !g->map || g->R.nLevels == 0; }
static RefreshDims covis_dims(const orbfe_covis* g) { return RefreshDims{g->T.kfCap, g->T.kfStride, g->T.obsStride, g->T.cap, g->R.nLevels}; }

int orbfe_covis_set_features(orbfe_handle* h, orbfe_covis* g, int slot, int n, const orbfe_keypoint* kp, const uint8_t* desc)
{
    if (covis_no_refresh(h, g) || !refresh_features_ok(covis_dims(g), slot, n, kp, desc, true)) return ORBFE_ERR_INVALID_ARG;
    Staging st;
    const FeaturesStage B(st, n);
    return covis_staged_call(
        h, st, st.inBytes, [&]() { B.fill(st, n, kp, desc); },
        [&](std::string& err) { return covis_set_features_launch(h->stream, g->T, g->R, slot, n, st.dev(B.kp), st.dev(B.desc), err); });
}

int orbfe_covis_set_features_device(orbfe_handle* h, orbfe_covis* g, int slot, const orbfe_keypoint* d_kp, const uint8_t* d_desc, int n,
                                    void* stream_)
{
    if (covis_no_refresh(h, g) || !refresh_features_ok(covis_dims(g), slot, n, d_kp, d_desc, false)) return ORBFE_ERR_INVALID_ARG;
    return match_call(h, (hipStream_t)stream_, [&](hipStream_t s, std::string& e) -> int {
        return covis_set_features_launch(s, g->T, g->R, slot, n, d_kp, d_desc, e);
    });
}

int orbfe_covis_set_centres(orbfe_handle* h, orbfe_covis* g, int n, const int* slots, const float* twc)
{
    if (covis_no_refresh(h, g) || !refresh_centres_ok(covis_dims(g), n, slots, twc)) return ORBFE_ERR_INVALID_ARG;
    if (n == 0) return ORBFE_OK;
    Staging st;
    const auto bSlots = st.in<int>(n);
    const auto bTwc = st.in<float>((size_t)n * 3);
    return covis_staged_call(
        h, st, st.inBytes,
        [&]() {
            st.put(bSlots, slots);
            st.put(bTwc, twc);
        },
        [&](std::string& err) { return covis_scatter_centres_launch(h->stream, g->T, g->R, n, st.dev(bSlots), st.dev(bTwc), err); });
}

int orbfe_covis_set_observations_indexed(orbfe_handle* h, orbfe_covis* g, int n, const int* ids, const int* off, const int* kf_slots,
                                         const int* feat_idx)
{
    return covis_set_observations(h, g, n, ids, off, kf_slots, feat_idx, true);
}

int orbfe_covis_set_ref_keyframes(orbfe_handle* h, orbfe_covis* g, int n, const int* ids, const int* ref_slots)
{
    if (covis_no_refresh(h, g) || !refresh_refs_ok(covis_dims(g), n, ids, ref_slots)) return ORBFE_ERR_INVALID_ARG;
    if (n == 0) return ORBFE_OK;
    Staging st;
    const auto bIds = st.in<int>(n);
    const auto bRef = st.in<int>(n);
    return covis_staged_call(
        h, st, st.inBytes,
        [&]() {
            st.put(bIds, ids);
            st.put(bRef, ref_slots);
        },
        [&](std::string& err) { return covis_scatter_ref_launch(h->stream, g->T, g->R, n, st.dev(bIds), st.dev(bRef), err); });
}

int orbfe_covis_get_point(orbfe_handle* h, orbfe_covis* g, int id, int* n_obs, int* kf_slots, int* feat_idx, int* ref_slot,
                          orbfe_world_point* point, uint8_t* desc)
{
    if (covis_no_refresh(h, g) || !n_obs || !kf_slots || !feat_idx || !ref_slot || id < 0 || id >= g->T.cap) return ORBFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    const CovisTables& T = g->T;
    hipStream_t s = h->stream;
    const size_t S = (size_t)T.obsStride;
    HIPCHK(h, hipMemcpyAsync(n_obs, T.obsCount + id, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(kf_slots, T.obs + (size_t)id * S, S * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(feat_idx, g->R.obsIdx + (size_t)id * S, S * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(ref_slot, g->R.refKf + id, sizeof(int), hipMemcpyDeviceToHost, s));
    if (point) HIPCHK(h, hipMemcpyAsync(point, g->map->dPts + id, sizeof *point, hipMemcpyDeviceToHost, s));
    if (desc) HIPCHK(h, hipMemcpyAsync(desc, g->map->dDesc + (size_t)id * ORBFE_DESC_BYTES, ORBFE_DESC_BYTES, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    return ORBFE_OK;
}

// the rest list for a call of n entries; the caller holds h->mu.  Grows only, both counters at zero when it does.
static int covis_refresh_scratch(orbfe_covis* g, int n, hipStream_t s, std::string& err)
{
    CovisRefresh& R = g->R;
    if (n > R.restCap) {
        // the block in use may still be read by a call in flight on another stream: hipFree waits for the device
        if (R.rest) (void)hipFree(R.rest);
        R.rest = nullptr;
        R.restCap = 0;
        if (hipMalloc(&R.rest, ((size_t)n + 2) * sizeof(int)) != hipSuccess) {
            (void)hipGetLastError();
            R.rest = nullptr;
            err = "orbfe_covis_refresh_points: allocation of the rest list failed";
            return ORBFE_ERR_OUT_OF_MEMORY;
        }
        MCHK(hipMemsetAsync(R.rest, 0, 2 * sizeof(int), s));
        R.restCap = n;
        R.parity = 0;
    }
    return ORBFE_OK;
}

// what the arguments alone decide, for both forms
static int covis_refresh_refuse(const orbfe_handle* h, const orbfe_covis* g, int n, const void* ids, int what)
{
    if (covis_no_refresh(h, g) || !ids || n < 1 || what < 1 || what > 3) return ORBFE_ERR_INVALID_ARG;
    return ORBFE_OK;
}

// the two launches of one call; the caller holds h->mu inside a call scope
static int covis_refresh_run(orbfe_covis* g, hipStream_t s, int n, const int* dIds, const int* dSelect, int selectValue, int what,
                             const RefreshOut& out, std::string& e)
{
    int rc = covis_refresh_scratch(g, n, s, e);
    if (rc != ORBFE_OK) return rc;
    rc = covis_refresh_launch(s, g->T, g->R, g->map->dPts, g->map->dDesc, n, dIds, dSelect, selectValue, what, out, e);
    g->R.parity ^= 1;
    return rc;
}

int orbfe_covis_refresh_points_device(orbfe_handle* h, orbfe_covis* g, int n, const int* d_ids, const int* d_select, int select_value,
                                      int what, const orbfe_refresh_io* io, void* stream_)
{
    if (!io) return ORBFE_ERR_INVALID_ARG;
    if (io->struct_size != (int)sizeof(orbfe_refresh_io))
        return refuse(h, ORBFE_ERR_INVALID_ARG,
                      "orbfe_refresh_io.struct_size does not match this library (rebuild the caller against include/orbfe.h)", kKeep);
    const int crc = covis_refresh_refuse(h, g, n, d_ids, what);
    if (crc != ORBFE_OK) return crc;
    const RefreshOut out{io->d_status, io->d_min_distance, io->d_max_distance, io->d_best_slot, io->d_best_index, io->d_best_median};
    return match_call(h, (hipStream_t)stream_, [&](hipStream_t s, std::string& e) -> int {
        return covis_refresh_run(g, s, n, d_ids, d_select, select_value, what, out, e);
    });
}

int orbfe_covis_refresh_points(orbfe_handle* h, orbfe_covis* g, int n, const int* ids, int what, int* status, float* min_distance,
                               float* max_distance, int* best_slot, int* best_index, int* best_median)
{
    const int crc = covis_refresh_refuse(h, g, n, ids, what);
    if (crc != ORBFE_OK) return crc;
    Staging st;
    const RefreshStage B(st, n);
    const auto bIds = B.ids, bStatus = B.status, bSlot = B.slot, bIndex = B.index, bMedian = B.median;
    const auto bMin = B.minD, bMax = B.maxD;
    return match_call(h, nullptr, [&](hipStream_t s, std::string& e) -> int {
        int rc = reserve(h->match, st, e);
        if (rc != ORBFE_OK) return rc;
        st.put(bIds, ids);
        if ((rc = upload(st, s, e)) != ORBFE_OK) return rc;
        const RefreshOut out{st.dev(bStatus), st.dev(bMin), st.dev(bMax), st.dev(bSlot), st.dev(bIndex), st.dev(bMedian)};
        if ((rc = covis_refresh_run(g, s, n, st.dev(bIds), nullptr, 0, what, out, e)) != ORBFE_OK) return rc;
        if ((rc = download(st, s, e)) != ORBFE_OK) return rc;
        st.get(bStatus, status);
        st.get(bMin, min_distance);
        st.get(bMax, max_distance);
        st.get(bSlot, best_slot);
        st.get(bIndex, best_index);
        st.get(bMedian, best_median);
        return ORBFE_OK;
    });
}

// ---- Tracking::TrackLocalMap with the IMU, batched and resident (SPEC DECISION S23) ----

// what the arguments alone decide, for both entry points: nothing is dereferenced but the two blocks, no handle is looked at
static int track_inertial_refuse(const orbfe_track_inertial_params* p, int batch, int kp_stride, const orbfe_map* map, int M,
                                 const orbfe_track_inertial_io* io, std::string& err)
{
    if (!p || !io) return ORBFE_ERR_INVALID_ARG;
    const int crc = track_inertial_check(p, err);
    if (crc != ORBFE_OK) return crc;
    if (io->struct_size != (int)sizeof(orbfe_track_inertial_io)) {
        err = "orbfe_track_inertial_io.struct_size does not match this library (rebuild the caller against include/orbfe.h)";
        return ORBFE_ERR_INVALID_ARG;
    }
    if (imu_check_offsets(batch, io->sample_off) != ORBFE_OK) return ORBFE_ERR_INVALID_ARG;
    if (M < 0 || kp_stride < 1 || kp_stride > kPoseMaxKp || !map) return ORBFE_ERR_INVALID_ARG;
    const bool fromFrame = p->predict.which == ORBFE_IMU_FROM_FRAME;
    if (!io->d_samples || !io->d_t_prev || !io->d_t_cur || !io->d_frame_bias || !io->d_state1 || !io->d_kf || !io->d_frame || !io->d_kp ||
        !io->d_desc || !io->d_n || !io->d_state_in || !io->d_info_ok || !io->d_match_out || !io->d_n_matches || !io->d_state_out ||
        !io->d_H_out || !io->d_outlier || !io->d_n_inliers || !io->d_accepted || !io->d_matches_inliers || !io->d_tracked ||
        !io->d_Tcw_out || (fromFrame && !io->d_priors) || (M > 0 && (!io->d_ids || !io->d_mp_out || !io->d_found)))
        return ORBFE_ERR_INVALID_ARG;
    return ORBFE_OK;
}

int orbfe_track_inertial_batch_device(orbfe_handle* h, const orbfe_track_inertial_params* p, int batch, int kp_stride, const orbfe_map* map,
                                      int n_points, const orbfe_track_inertial_io* io, void* stream_)
{
    std::string err;
    const int crc = track_inertial_refuse(p, batch, kp_stride, map, n_points, io, err);
    if (crc != ORBFE_OK) return refuse(h, crc, err, kKeep);
    if (!h) return ORBFE_ERR_INVALID_ARG;
    if (map->h != h || p->frustum.n_levels > h->nLevels || n_points > (1 << 24)) return ORBFE_ERR_INVALID_ARG;
    return match_call(h, (hipStream_t)stream_, [&](hipStream_t s, std::string& e) {
        return track_inertial_batch_device(h->match, s, p, h->dSf, h->invSig2, h->nLevels, batch, kp_stride, map->cap, map->dPts, map->dDesc,
                                           n_points, io, nullptr, e);
    });
}

int orbfe_track_frame_inertial(orbfe_handle* h, const orbfe_track_inertial_params* p, const uint8_t* gray, int pitch, int n_samples,
                               const orbfe_imu_sample* samples, double t_prev, double t_cur, const float* frame_bias, const float* state1,
                               orbfe_imu_preint* kf, orbfe_imu_preint* frame, const orbfe_map* map, int M, const int* ids,
                               const orbfe_pose_imu_prior* prior, orbfe_keypoint* kp_out, uint8_t* desc_out, int* n_out, int* per_level,
                               orbfe_track_inertial_result* res)
{
    if (!p || !res) return ORBFE_ERR_INVALID_ARG;
    std::string err;
    int crc = track_inertial_check(p, err);
    if (crc == ORBFE_OK) crc = imu_check(nullptr, nullptr, kf, frame, err);
    if (crc == ORBFE_OK && res->struct_size != (int)sizeof(orbfe_track_inertial_result)) {
        err = "orbfe_track_inertial_result.struct_size does not match this library (rebuild the caller against include/orbfe.h)";
        crc = ORBFE_ERR_INVALID_ARG;
    }
    if (crc != ORBFE_OK) return refuse(h, crc, err, kKeep);
    const bool fromFrame = p->predict.which == ORBFE_IMU_FROM_FRAME;
    if (fromFrame && prior && prior->struct_size != (int)sizeof(orbfe_pose_imu_prior)) return ORBFE_ERR_INVALID_ARG;
    if (!gray || n_samples < 0 || (n_samples > 0 && !samples) || !frame_bias || !state1 || !kf || !frame || !map || M < 0 ||
        (M > 0 && (!ids || !res->mp_out || !res->found)) || (fromFrame && !prior) || !kp_out || !desc_out || !n_out || !res->state_in ||
        !res->match_out || !res->state_out || !res->H_out || !res->outlier)
        return ORBFE_ERR_INVALID_ARG;
    if (!h) return ORBFE_ERR_INVALID_ARG;
    if (map->h != h || p->frustum.n_levels > h->nLevels || M > (1 << 24) || pitch < h->prm.image_width || pitch >= (1 << 24))
        return ORBFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    const int cap = h->P.kpCapFrame, nL = h->nLevels;
    if (cap > kPoseMaxKp) return ORBFE_ERR_UNSUPPORTED;  // the pose kernels' bound on kp_stride
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;

    // ---- layout ----
    const size_t linkBytes = fromFrame ? sizeof(orbfe_imu_link_free) : sizeof(orbfe_imu_link);
    const size_t hBytes = (fromFrame ? 900 : 225) * sizeof(double);
    const int Mp = std::max(M, 1), nS = std::max(n_samples, 1);
    ChainPrefix L{};
    size_t out = chain_prefix_layout(h, L);
    size_t in = L.inFrame;
    const size_t iTimes = take256(in, 2 * sizeof(double));
    const size_t iBias = take256(in, 6 * sizeof(float));
    const size_t iState1 = take256(in, kImuState * sizeof(float));
    const size_t iKf = take256(in, sizeof(orbfe_imu_preint));
    const size_t iFrame = take256(in, sizeof(orbfe_imu_preint));
    const size_t iPrior = take256(in, sizeof(orbfe_pose_imu_prior));
    const size_t iSamples = take256(in, (size_t)nS * sizeof(orbfe_imu_sample));
    const size_t iIds = take256(in, (size_t)Mp * sizeof(int));
    // the records come back too: they sit in the input block on the device and are copied into the result block behind the chain
    const size_t oKf = take256(out, sizeof(orbfe_imu_preint));
    const size_t oFrame = take256(out, sizeof(orbfe_imu_preint));
    const size_t oSteps = take256(out, (size_t)nS * sizeof(orbfe_imu_step));
    const size_t oStateIn = take256(out, kImuStateIn * sizeof(float));
    const size_t oLink = take256(out, linkBytes);
    const size_t oInts = take256(out, 8 * sizeof(int));  // info_ok, n_matches, n_inliers, accepted, matches_inliers, tracked
    const size_t oMps = take256(out, (size_t)Mp * sizeof(orbfe_map_point));
    const size_t oMatch = take256(out, (size_t)cap * sizeof(int));
    const size_t oStateOut = take256(out, kImuState * sizeof(float));
    const size_t oH = take256(out, hBytes);
    const size_t oHp = take256(out, 225 * sizeof(double));
    const size_t oOutlier = take256(out, (size_t)cap);
    const size_t oFound = take256(out, (size_t)Mp);
    const size_t oTcw = take256(out, 12 * sizeof(float));
    if (in > h->tinInBytes || out > h->tinOutBytes) {
        HIPCHK(h, hipStreamSynchronize(s));
        h->tinInBytes = h->tinOutBytes = 0;
        const size_t wantIn = in + in / 4, wantOut = out + out / 4;
        const int rc = chain_blocks_alloc(h, h->tin, wantIn, wantOut, wantOut, "orbfe_track_frame_inertial");
        if (rc != ORBFE_OK) return rc;
        h->tinInBytes = wantIn;
        h->tinOutBytes = wantOut;
    }
    uint8_t *hi = h->tin.hIn, *di = h->tin.dIn, *dout = h->tin.dOut, *ho = h->tin.hOut;

    // ---- stage and upload: the frame with the small block behind it ----
    const double times[2] = {t_prev, t_cur};
    memcpy(hi + iTimes, times, sizeof times);
    memcpy(hi + iBias, frame_bias, 6 * sizeof(float));
    memcpy(hi + iState1, state1, kImuState * sizeof(float));
    memcpy(hi + iKf, kf, sizeof(orbfe_imu_preint));
    memcpy(hi + iFrame, frame, sizeof(orbfe_imu_preint));
    if (fromFrame) memcpy(hi + iPrior, prior, sizeof(orbfe_pose_imu_prior));
    if (n_samples > 0) memcpy(hi + iSamples, samples, (size_t)n_samples * sizeof(orbfe_imu_sample));
    if (M > 0) memcpy(hi + iIds, ids, (size_t)M * sizeof(int));
    int inPitch;
    int rc = upload_frame(h, h->tin, gray, pitch, iTimes, in, s, &inPitch);
    if (rc != ORBFE_OK) return rc;

    // ---- extraction, then the chain with batch == 1 ----
    int* dHead = reinterpret_cast<int*>(dout);  // [n, status]
    rc = extract_chain(h, di, L.inFrame, inPitch, 1, reinterpret_cast<orbfe_keypoint*>(dout + L.oKp), dout + L.oDesc, dHead,
                       reinterpret_cast<int*>(dout + L.oPer), dHead + 1, s);
    if (rc != ORBFE_OK) return rc;
    const int off[2] = {0, n_samples};
    int* dInts = reinterpret_cast<int*>(dout + oInts);
    orbfe_track_inertial_io io{};
    io.struct_size = (int)sizeof io;
    io.d_samples = reinterpret_cast<const orbfe_imu_sample*>(di + iSamples);
    io.sample_off = off;
    io.d_t_prev = reinterpret_cast<const double*>(di + iTimes);
    io.d_t_cur = io.d_t_prev + 1;
    io.d_frame_bias = reinterpret_cast<const float*>(di + iBias);
    io.d_state1 = reinterpret_cast<const float*>(di + iState1);
    io.d_kf = reinterpret_cast<orbfe_imu_preint*>(di + iKf);
    io.d_frame = reinterpret_cast<orbfe_imu_preint*>(di + iFrame);
    io.d_steps_out = reinterpret_cast<orbfe_imu_step*>(dout + oSteps);
    io.d_kp = reinterpret_cast<const orbfe_keypoint*>(dout + L.oKp);
    io.d_desc = dout + L.oDesc;
    io.d_n = dHead;
    io.d_ids = reinterpret_cast<const int*>(di + iIds);
    io.d_priors = fromFrame ? reinterpret_cast<const orbfe_pose_imu_prior*>(di + iPrior) : nullptr;
    io.d_state_in = reinterpret_cast<float*>(dout + oStateIn);
    io.d_info_ok = dInts;
    io.d_mp_out = reinterpret_cast<orbfe_map_point*>(dout + oMps);
    io.d_match_out = reinterpret_cast<int*>(dout + oMatch);
    io.d_n_matches = dInts + 1;
    io.d_state_out = reinterpret_cast<float*>(dout + oStateOut);
    io.d_H_out = reinterpret_cast<double*>(dout + oH);
    io.d_Hprior_out = fromFrame && res->Hprior_out ? reinterpret_cast<double*>(dout + oHp) : nullptr;
    io.d_outlier = dout + oOutlier;
    io.d_n_inliers = dInts + 2;
    io.d_accepted = dInts + 3;
    io.d_found = dout + oFound;
    io.d_matches_inliers = dInts + 4;
    io.d_tracked = dInts + 5;
    io.d_Tcw_out = reinterpret_cast<float*>(dout + oTcw);
    {
        MatchScope scope_(h, s);
        if (scope_.rc != ORBFE_OK) return scope_.rc;
        void* dLinks = nullptr;
        rc = track_inertial_batch_device(h->match, s, p, h->dSf, h->invSig2, nL, 1, cap, map->cap, map->dPts, map->dDesc, M, &io, &dLinks, err);
        if (rc != ORBFE_OK) {
            h->err = err;
            return rc;
        }
        // the records and the link join the result block, so that ONE copy brings everything back
        HIPCHK(h, hipMemcpyAsync(dout + oKf, di + iKf, sizeof(orbfe_imu_preint), hipMemcpyDeviceToDevice, s));
        HIPCHK(h, hipMemcpyAsync(dout + oFrame, di + iFrame, sizeof(orbfe_imu_preint), hipMemcpyDeviceToDevice, s));
        HIPCHK(h, hipMemcpyAsync(dout + oLink, dLinks, linkBytes, hipMemcpyDeviceToDevice, s));
        HIPCHK(h, hipMemcpyAsync(ho, dout, out, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(h, hipStreamSynchronize(s));
    const int status = reinterpret_cast<const int*>(ho)[1];
    if (status) {
        char buf[112];
        snprintf(buf, sizeof buf, "device guard flags 0x%x in orbfe_track_frame_inertial", (unsigned)status);
        h->err = buf;
        return ORBFE_ERR_INTERNAL;
    }

    // ---- hand over ----
    const int n = chain_prefix_copy_out(h, ho, L, kp_out, desc_out, n_out, per_level);
    const int nSteps = n_samples < 2 ? 0 : n_samples - 1;
    memcpy(kf, ho + oKf, sizeof(orbfe_imu_preint));
    memcpy(frame, ho + oFrame, sizeof(orbfe_imu_preint));
    res->n_steps = nSteps;
    if (res->steps_out && nSteps) memcpy(res->steps_out, ho + oSteps, (size_t)nSteps * sizeof(orbfe_imu_step));
    memcpy(res->state_in, ho + oStateIn, kImuStateIn * sizeof(float));
    if (res->link_out) memcpy(res->link_out, ho + oLink, linkBytes);
    const int* ints = reinterpret_cast<const int*>(ho + oInts);
    res->info_ok = ints[0];
    res->n_matches = ints[1];
    res->n_inliers = ints[2];
    res->accepted = ints[3];
    res->matches_inliers = ints[4];
    res->tracked = ints[5];
    if (M > 0) {
        memcpy(res->mp_out, ho + oMps, (size_t)M * sizeof(orbfe_map_point));
        memcpy(res->found, ho + oFound, (size_t)M);
    }
    memcpy(res->match_out, ho + oMatch, (size_t)n * sizeof(int));
    memcpy(res->state_out, ho + oStateOut, kImuState * sizeof(float));
    memcpy(res->H_out, ho + oH, hBytes);
    if (io.d_Hprior_out) memcpy(res->Hprior_out, ho + oHp, 225 * sizeof(double));
    memcpy(res->outlier, ho + oOutlier, (size_t)n);
    memcpy(res->Tcw, ho + oTcw, 12 * sizeof(float));
    return ORBFE_OK;
}

int orbfe_initial_bundle_adjustment(orbfe_handle* h, const orbfe_initial_ba_params* p, int n1, const orbfe_keypoint* kp1, int n2,
                                    const orbfe_keypoint* kp2, const int* matches12, const float* points, const float* Rcw1,
                                    const float* tcw1, const float* Rcw2, const float* tcw2, float* Tcw2_out, float* points_out,
                                    orbfe_initial_ba_info* info)
{
    if (!p) return ORBFE_ERR_INVALID_ARG;
    std::string err;
    int rc = initial_ba_check(p, info, err);  // struct sizes, unsupported branches and ranges need no handle
    if (rc == ORBFE_OK && (!h || n1 < 0 || n2 < 0 || !Rcw1 || !tcw1 || !Rcw2 || !tcw2 || !Tcw2_out ||
                           (n1 > 0 && (!kp1 || !matches12 || !points || !points_out)) || (n2 > 0 && !kp2)))
        return ORBFE_ERR_INVALID_ARG;
    if (!h) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    std::vector<int> first;
    // the other refusals and the return for no match at all read the handle's level count only: the device is not touched
    if (rc == ORBFE_OK) rc = initial_ba_begin(p, h->nLevels, n1, kp1, n2, kp2, matches12, points, Rcw2, tcw2, Tcw2_out, points_out, info, first, err);
    if (rc != ORBFE_OK) {
        h->err = err;
        return rc;
    }
    if (first.empty()) return ORBFE_OK;
    return match_call_locked(h, nullptr, [&](hipStream_t s, std::string& e) {
        return initial_ba_run_host(h->match, s, p, h->invSig2, kp1, kp2, matches12, points, Rcw1, tcw1, Rcw2, tcw2, first, Tcw2_out, points_out,
                                   info, e);
    });
}

int orbfe_triangulation_select(int n1, const int* raw_match12, const uint8_t* raw_bin, const uint8_t* has_mp1_now,
                               int check_orientation, int* matches12_out, int* n_matches)
{
    if (n1 < 0 || !n_matches || (n1 > 0 && (!raw_match12 || !raw_bin || !has_mp1_now || !matches12_out))) return ORBFE_ERR_INVALID_ARG;
    int hist[ORBFE_HISTO_LENGTH] = {0};
    int n = 0;
    for (int i = 0; i < n1; i++) {
        int m = has_mp1_now[i] ? -1 : raw_match12[i];  // src/ORBmatcher.cc:506-509
        if (m >= 0) {
            if (check_orientation && raw_bin[i] >= ORBFE_HISTO_LENGTH) return ORBFE_ERR_INVALID_ARG;
            n++;
            if (check_orientation) hist[raw_bin[i]]++;
        }
        matches12_out[i] = m;
    }
    if (check_orientation) {  // :633-661
        int ind1, ind2, ind3;
        three_maxima(hist, ind1, ind2, ind3);
        for (int i = 0; i < n1; i++)
            if (matches12_out[i] >= 0) {
                const int b = raw_bin[i];
                if (b != ind1 && b != ind2 && b != ind3) {
                    matches12_out[i] = -1;
                    n--;
                }
            }
    }
    *n_matches = n;
    return ORBFE_OK;
}

int orbfe_distinctive_descriptors(orbfe_handle* h, int n_sets, const int* set_off, const uint8_t* desc, int* best_idx_out,
                                  int* best_median_out)
{
    if (!h || n_sets < 0 || (n_sets > 0 && (!set_off || !best_idx_out || set_off[0] != 0)) ||
        (n_sets > 0 && set_off[n_sets] > 0 && !desc))
        return ORBFE_ERR_INVALID_ARG;
    return match_call(h, nullptr, [&](hipStream_t s, std::string& err) {
        return distinctive_run(h->match, s, n_sets, set_off, desc, best_idx_out, best_median_out, err);
    });
}

// ---------------------------------------------------------------------------------------------
// Node-side image preparation (image_grabber.hpp:96-110): kernels_prep.hip
// ---------------------------------------------------------------------------------------------
struct orbfe_prep {
    int device = 0;
    int srcW = 0, srcH = 0, dstW = 0, dstH = 0;
    float* dMap1 = nullptr;
    float* dMap2 = nullptr;
    uint8_t* dSrc = nullptr;   // srcH x srcPitch, BGR
    uint8_t* hSrc = nullptr;   // pinned staging for pageable sources
    int srcPitch = 0;
    uint8_t* dGray = nullptr;  // dstH x grayPitch
    uint8_t* hGray = nullptr;  // pinned
    int grayPitch = 0;
};

void orbfe_prep_destroy(orbfe_prep* p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    if (p->dMap1) (void)hipFree(p->dMap1);
    if (p->dMap2) (void)hipFree(p->dMap2);
    if (p->dSrc) (void)hipFree(p->dSrc);
    if (p->dGray) (void)hipFree(p->dGray);
    if (p->hSrc) (void)hipHostFree(p->hSrc);
    if (p->hGray) (void)hipHostFree(p->hGray);
    delete p;
}

int orbfe_prep_create(orbfe_handle* h, int src_w, int src_h, const float* map1, const float* map2, int dst_w, int dst_h,
                      orbfe_prep** out)
{
    if (!h || !map1 || !map2 || !out || src_w < 2 || src_h < 2 || dst_w < 1 || dst_h < 1 || src_w > 16384 || src_h > 16384 ||
        dst_w > 16384 || dst_h > 16384)
        return ORBFE_ERR_INVALID_ARG;
    *out = nullptr;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    orbfe_prep* p = new (std::nothrow) orbfe_prep();
    if (!p) return ORBFE_ERR_OUT_OF_MEMORY;
    p->device = h->device;
    p->srcW = src_w; p->srcH = src_h; p->dstW = dst_w; p->dstH = dst_h;
    p->srcPitch = (int)align_up((size_t)src_w * 3, 256);
    p->grayPitch = (int)align_up((size_t)dst_w, 256);
    const size_t mapBytes = (size_t)src_w * src_h * sizeof(float);
    bool ok = hipMalloc(&p->dMap1, mapBytes) == hipSuccess && hipMalloc(&p->dMap2, mapBytes) == hipSuccess &&
              hipMalloc(&p->dSrc, (size_t)p->srcPitch * src_h) == hipSuccess &&
              hipHostMalloc(&p->hSrc, (size_t)p->srcPitch * src_h) == hipSuccess &&
              hipMalloc(&p->dGray, (size_t)p->grayPitch * dst_h) == hipSuccess &&
              hipHostMalloc(&p->hGray, (size_t)p->grayPitch * dst_h) == hipSuccess;
    ok = ok && copy_sync(p->dMap1, map1, mapBytes, hipMemcpyHostToDevice, h->stream) == hipSuccess &&
         copy_sync(p->dMap2, map2, mapBytes, hipMemcpyHostToDevice, h->stream) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        orbfe_prep_destroy(p);
        h->err = "orbfe_prep_create: allocation or map upload failed";
        return ORBFE_ERR_OUT_OF_MEMORY;
    }
    *out = p;
    return ORBFE_OK;
}

static orbfe::PrepArgs prep_args(const orbfe_prep* p, const uint8_t* dSrc, int srcPitch, uint8_t* dDst, int dstPitch)
{
    orbfe::PrepArgs P{};
    P.src = dSrc; P.srcPitch = srcPitch; P.srcFrameStride = 0;
    P.srcW = p->srcW; P.srcH = p->srcH;
    P.map1 = p->dMap1; P.map2 = p->dMap2;
    P.dst = dDst; P.dstPitch = dstPitch; P.dstFrameStride = 0;
    P.dstW = p->dstW; P.dstH = p->dstH;
    P.fx = orbfe::prep_scale(p->srcW, p->dstW);
    P.fy = orbfe::prep_scale(p->srcH, p->dstH);
    return P;
}

// BGR frame -> p->dSrc on stream s (pinned sources go straight through the DMA engine with their own pitch)
static int prep_upload(orbfe_handle* h, orbfe_prep* p, const uint8_t* bgr, int pitch, hipStream_t s, int* devPitch)
{
    const size_t rowBytes = (size_t)p->srcW * 3;
    hipPointerAttribute_t attr;
    const bool pinned = pitch <= p->srcPitch && hipPointerGetAttributes(&attr, bgr) == hipSuccess && attr.type == hipMemoryTypeHost;
    if (!pinned) (void)hipGetLastError();
    if (pinned) {
        HIPCHK(h, hipMemcpyAsync(p->dSrc, bgr, (size_t)pitch * (p->srcH - 1) + rowBytes, hipMemcpyHostToDevice, s));
        *devPitch = pitch;
    } else {
        for (int y = 0; y < p->srcH; y++) memcpy(p->hSrc + (size_t)y * p->srcPitch, bgr + (size_t)y * pitch, rowBytes);
        HIPCHK(h, hipMemcpyAsync(p->dSrc, p->hSrc, (size_t)p->srcPitch * p->srcH, hipMemcpyHostToDevice, s));
        *devPitch = p->srcPitch;
    }
    return ORBFE_OK;
}

int orbfe_prepare_image_device(orbfe_handle* h, orbfe_prep* p, const uint8_t* d_bgr, int pitch, uint8_t* d_gray, int gray_pitch,
                               void* stream)
{
    if (!h || !p || !d_bgr || !d_gray || pitch < p->srcW * 3 || gray_pitch < p->dstW) return ORBFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    orbfe::prep_launch(s, prep_args(p, d_bgr, pitch, d_gray, gray_pitch), 1);
    HIPCHK(h, hipGetLastError());
    return ORBFE_OK;
}

int orbfe_prepare_image(orbfe_handle* h, orbfe_prep* p, const uint8_t* bgr, int pitch, uint8_t* gray_out, int gray_pitch)
{
    if (!h || !p || !bgr || !gray_out || pitch < p->srcW * 3 || gray_pitch < p->dstW) return ORBFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int devPitch = 0;
    const int rc = prep_upload(h, p, bgr, pitch, s, &devPitch);
    if (rc != ORBFE_OK) return rc;
    orbfe::prep_launch(s, prep_args(p, p->dSrc, devPitch, p->dGray, p->grayPitch), 1);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(p->hGray, p->dGray, (size_t)p->grayPitch * p->dstH, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    for (int y = 0; y < p->dstH; y++) memcpy(gray_out + (size_t)y * gray_pitch, p->hGray + (size_t)y * p->grayPitch, (size_t)p->dstW);
    return ORBFE_OK;
}

int orbfe_prepare_and_extract(orbfe_handle* h, orbfe_prep* p, const uint8_t* bgr, int pitch, orbfe_keypoint* kp_out,
                              uint8_t* desc_out, int* n_out, int* per_level, uint8_t* gray_out, int gray_pitch)
{
    if (!h || !p || !bgr || !kp_out || !desc_out || !n_out || pitch < p->srcW * 3 || (gray_out && gray_pitch < p->dstW))
        return ORBFE_ERR_INVALID_ARG;
    if (p->dstW != h->prm.image_width || p->dstH != h->prm.image_height) return ORBFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int devPitch = 0;
    int rc = prep_upload(h, p, bgr, pitch, s, &devPitch);
    if (rc != ORBFE_OK) return rc;
    // the grey frame is written straight into the extractor's level-0 input rows: no host round trip in between
    orbfe::prep_launch(s, prep_args(p, p->dSrc, devPitch, h->dIn, h->dInPitch), 1);
    HIPCHK(h, hipGetLastError());
    rc = extract_enqueue_replay(h, 1, h->dInPitch, s);
    if (rc != ORBFE_OK) return rc;
    if (gray_out)
        HIPCHK(h, hipMemcpy2DAsync(p->hGray, p->grayPitch, h->dIn, h->dInPitch, p->dstW, p->dstH, hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    rc = check_device_flags(h, 1);
    if (rc != ORBFE_OK) return rc;
    const int n = h->hN[0];
    n_out[0] = n;
    memcpy(kp_out, h->hKp, (size_t)n * sizeof(orbfe_keypoint));
    memcpy(desc_out, h->hDesc, (size_t)n * ORBFE_DESC_BYTES);
    if (per_level) memcpy(per_level, h->hPer, h->nLevels * sizeof(int));
    if (gray_out)
        for (int y = 0; y < p->dstH; y++) memcpy(gray_out + (size_t)y * gray_pitch, p->hGray + (size_t)y * p->grayPitch, (size_t)p->dstW);
    return ORBFE_OK;
}

struct orbfe_vocab {
    orbfe::Vocab* v;
    int device;
    unsigned long long serial;  // names the vocabulary in graph keys (an address could be reused after a destroy)
};
static std::atomic<unsigned long long> g_vocabSerial{1};

int orbfe_vocab_create(orbfe_handle* h, int n_nodes, const int* child_off, const int* child_idx, const uint8_t* node_desc,
                       const int* word_id, const double* weight, int L, orbfe_vocab** out)
{
    if (!h || !child_off || !child_idx || !node_desc || !word_id || !weight || !out || n_nodes < 2 || L < 1)
        return ORBFE_ERR_INVALID_ARG;
    *out = nullptr;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    std::string err;
    orbfe::Vocab* v = nullptr;
    const int rc = vocab_create(n_nodes, child_off, child_idx, node_desc, word_id, weight, L, h->stream, &v, err);
    if (rc != ORBFE_OK) {
        h->err = err;
        return rc;
    }
    *out = new orbfe_vocab{v, h->device, g_vocabSerial.fetch_add(1)};
    return ORBFE_OK;
}

void orbfe_vocab_destroy(orbfe_vocab* v)
{
    if (!v) return;
    (void)hipSetDevice(v->device);
    vocab_destroy(v->v);
    delete v;
}

int orbfe_bow_transform(orbfe_handle* h, orbfe_vocab* v, const uint8_t* desc, int n, int levelsup, int* word_id_out,
                        int* node_id_out, double* weight_out)
{
    if (!h || !v || n < 0 || (n > 0 && (!desc || !word_id_out || !node_id_out))) return ORBFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    std::string err;
    const int rc = vocab_transform(v->v, h->stream, desc, n, levelsup, word_id_out, node_id_out, weight_out, err);
    if (rc != ORBFE_OK) h->err = err;
    return rc;
}

int orbfe_match_bow_rig(orbfe_handle* h, int G, const int* kf_off, const int* kf_idx, const int* f_off, const int* f_idx,
                        int n_kf, const uint8_t* kf_desc, const float* kf_angle, const uint8_t* kf_has_mp, int n_f,
                        const uint8_t* f_desc, const float* f_angle, int n_left, float nn_ratio, int check_orientation,
                        int* match_out, int* n_matches)
{
    if (!h || !match_out || !n_matches || G < 0 || n_kf < 0 || n_f < 0 || n_left < -1 || n_left > n_f) return ORBFE_ERR_INVALID_ARG;
    if (G > 0 && (!kf_off || !kf_idx || !f_off || !f_idx || !kf_desc || !f_desc || !kf_has_mp)) return ORBFE_ERR_INVALID_ARG;
    if (check_orientation && G > 0 && (!kf_angle || !f_angle)) return ORBFE_ERR_INVALID_ARG;
    return match_call(h, nullptr, [&](hipStream_t s, std::string& err) {
        return match_bow_run(h->match, s, G, kf_off, kf_idx, f_off, f_idx, n_kf, kf_desc, kf_angle, kf_has_mp, n_f, f_desc, f_angle, n_left,
                             nn_ratio, check_orientation, match_out, n_matches, err);
    });
}

int orbfe_match_bow(orbfe_handle* h, int G, const int* kf_off, const int* kf_idx, const int* f_off, const int* f_idx,
                    int n_kf, const uint8_t* kf_desc, const float* kf_angle, const uint8_t* kf_has_mp, int n_f,
                    const uint8_t* f_desc, const float* f_angle, float nn_ratio, int check_orientation, int* match_out,
                    int* n_matches)
{
    return orbfe_match_bow_rig(h, G, kf_off, kf_idx, f_off, f_idx, n_kf, kf_desc, kf_angle, kf_has_mp, n_f, f_desc, f_angle, -1,
                               nn_ratio, check_orientation, match_out, n_matches);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// orbfe_track_reference_keyframe: extract -> vocabulary descent -> SearchByBoW(resident key frame) as one captured hipGraph
// ---------------------------------------------------------------------------------------------
namespace {

struct RefLayout : ChainPrefix {
    size_t oRef, oFlags, inBytes;
    size_t oMatch, oBow, oLeaf, outBytes /* what is downloaded */, oBin, oGrp, oFIdx, oFCnt, oFOff, devBytes;
};

RefLayout ref_layout(const orbfe_handle* h, int capFlags)
{
    RefLayout L{};
    const size_t cap = (size_t)h->P.kpCapFrame;
    size_t off = chain_prefix_layout(h, L);
    L.oRef = L.inFrame;
    L.oFlags = L.oRef + align_up(sizeof(BowKfRef), 256);
    L.inBytes = L.oFlags + align_up((size_t)capFlags, 256);
    L.oMatch = take256(off, cap * sizeof(int));
    L.oBow = take256(off, cap * 2 * sizeof(int));
    L.oLeaf = take256(off, cap * sizeof(int));
    L.outBytes = off;
    L.oBin = take256(off, cap * sizeof(int));
    // the per-node frame lists of frames above 7168 features (bow_track_launch): a key frame has at most capFlags nodes
    L.oGrp = take256(off, cap * sizeof(int));
    L.oFIdx = take256(off, cap * sizeof(int));
    L.oFCnt = take256(off, (size_t)capFlags * sizeof(int));
    L.oFOff = take256(off, ((size_t)capFlags + 1) * sizeof(int));
    L.devBytes = off;
    return L;
}

int ref_reserve(orbfe_handle* h, int nFlags)
{
    if (h->ref.dIn && nFlags <= h->refCapFlags) return ORBFE_OK;
    h->refGraphs.drop();
    h->refCapFlags = 0;
    const int capFlags = std::max(4096, nFlags + nFlags / 2);
    const RefLayout L = ref_layout(h, capFlags);
    const int rc = chain_blocks_alloc(h, h->ref, L.inBytes, L.devBytes, L.outBytes, "orbfe_track_reference_keyframe");
    if (rc == ORBFE_OK) h->refCapFlags = capFlags;
    return rc;
}

// the device side of one call, enqueued on s (directly, or under stream capture)
int ref_enqueue(orbfe_handle* h, const RefLayout& L, int inPitch, const orbfe::Vocab* v, int levelsup, float nnRatio, int checkOri,
                hipStream_t s)
{
    const int cap = h->P.kpCapFrame;
    int* dHead = reinterpret_cast<int*>(h->ref.dOut);  // [n, status, n_matches]
    orbfe_keypoint* dKp = reinterpret_cast<orbfe_keypoint*>(h->ref.dOut + L.oKp);
    int rc = extract_chain(h, h->ref.dIn, L.inFrame, inPitch, 1, dKp, h->ref.dOut + L.oDesc, dHead, reinterpret_cast<int*>(h->ref.dOut + L.oPer),
                           dHead + 1, s);
    if (rc != ORBFE_OK) return rc;
    std::string err;
    int* dBow = reinterpret_cast<int*>(h->ref.dOut + L.oBow);
    rc = vocab_transform_launch_dev(v, s, h->ref.dOut + L.oDesc, dHead, cap, levelsup, dBow, reinterpret_cast<int*>(h->ref.dOut + L.oLeaf),
                                    reinterpret_cast<int*>(h->ref.dOut + L.oMatch), err);
    if (rc == ORBFE_OK) {
        BowTrackArgs A{};
        A.ref = reinterpret_cast<const BowKfRef*>(h->ref.dIn + L.oRef);
        A.kfHasMP = h->ref.dIn + L.oFlags;
        A.fKp = dKp;
        A.fDesc = h->ref.dOut + L.oDesc;
        A.fBow = dBow;
        A.fLeaf = reinterpret_cast<const int*>(h->ref.dOut + L.oLeaf);
        A.weight = v->dWeight;
        A.nF = dHead;
        A.cap = cap;
        A.nnRatio = nnRatio;
        A.checkOrientation = checkOri;
        A.matchOut = reinterpret_cast<int*>(h->ref.dOut + L.oMatch);
        A.binOf = reinterpret_cast<int*>(h->ref.dOut + L.oBin);
        A.nMatches = dHead + 2;
        A.fGrp = reinterpret_cast<int*>(h->ref.dOut + L.oGrp);
        A.fIdx = reinterpret_cast<int*>(h->ref.dOut + L.oFIdx);
        A.fCnt = reinterpret_cast<int*>(h->ref.dOut + L.oFCnt);
        A.fOff = reinterpret_cast<int*>(h->ref.dOut + L.oFOff);
        A.capGroups = h->refCapFlags;
        rc = bow_track_launch(s, A, err);
    }
    if (rc != ORBFE_OK) {
        h->err = err;
        return rc;
    }
    HIPCHK(h, hipMemcpyAsync(h->ref.hOut, h->ref.dOut, L.outBytes, hipMemcpyDeviceToHost, s));
    return ORBFE_OK;
}

}  // namespace

extern "C" int orbfe_track_reference_keyframe(orbfe_handle* h, const uint8_t* gray, int pitch, const orbfe_vocab* vocab, int levelsup,
                                              const orbfe_keyframe* kf, const uint8_t* kf_has_mp, float nn_ratio,
                                              int check_orientation, orbfe_keypoint* kp_out, uint8_t* desc_out, int* n_out,
                                              int* per_level, int* word_id_out, int* node_id_out, double* weight_out,
                                              int* match_out, int* n_matches)
{
    if (!h || !gray || !vocab || !kf || !kp_out || !desc_out || !n_out || !word_id_out || !node_id_out || !match_out || !n_matches)
        return ORBFE_ERR_INVALID_ARG;
    if (pitch < h->prm.image_width || pitch >= (1 << 24)) return ORBFE_ERR_INVALID_ARG;
    if (vocab->device != h->device || kf->device != h->device) return ORBFE_ERR_INVALID_ARG;
    const KeyFrameDev* K = kf->k;
    if (K->n > 0 && !kf_has_mp) return ORBFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->P.kpCapFrame >= (1 << 20)) return ORBFE_ERR_UNSUPPORTED;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int rc = ref_reserve(h, K->n);
    if (rc != ORBFE_OK) return rc;
    const RefLayout L = ref_layout(h, h->refCapFlags);

    // ---- the small block: which key frame (addresses of its resident arrays) + its flags as they stand now ----
    BowKfRef R{K->desc, K->kp, K->order, K->nodeList, K->nodeOff, K->G, K->n};
    memcpy(h->ref.hIn + L.oRef, &R, sizeof R);
    if (K->n) memcpy(h->ref.hIn + L.oFlags, kf_has_mp, (size_t)K->n);
    const size_t smallEnd = L.oFlags + (size_t)K->n;

    // ---- upload: the frame with the small block behind it ----
    int inPitch;
    rc = upload_frame(h, h->ref, gray, pitch, L.oRef, smallEnd, s, &inPitch);
    if (rc != ORBFE_OK) return rc;

    // ---- kernels + download: the graph of this (pitch, vocabulary, parameters) ----
    orbfe_handle::RefKey key;
    memset(&key, 0, sizeof key);
    key.inPitch = inPitch; key.levelsup = levelsup; key.checkOri = check_orientation; key.nnRatio = nn_ratio;
    key.vocabSerial = vocab->serial;
    rc = chain_submit(h, h->refGraphs, 16, key, h->ref, L.inFrame, inPitch, s,
                      [&](hipStream_t q) { return ref_enqueue(h, L, inPitch, vocab->v, levelsup, nn_ratio, check_orientation, q); },
                      "orbfe_track_reference_keyframe");
    if (rc != ORBFE_OK) return rc;

    // ---- hand over ----
    const int n = chain_prefix_copy_out(h, h->ref.hOut, L, kp_out, desc_out, n_out, per_level);
    *n_matches = n > 0 ? reinterpret_cast<const int*>(h->ref.hOut)[2] : 0;
    memcpy(match_out, h->ref.hOut + L.oMatch, (size_t)n * sizeof(int));
    const int* bow = reinterpret_cast<const int*>(h->ref.hOut + L.oBow);
    const int* leaf = reinterpret_cast<const int*>(h->ref.hOut + L.oLeaf);
    for (int i = 0; i < n; i++) {
        word_id_out[i] = bow[2 * i];
        node_id_out[i] = bow[2 * i + 1];
        if (weight_out) weight_out[i] = vocab->v->hWeight[(size_t)leaf[i]];  // m_nodes[final_id].weight, TemplatedVocabulary.h:1268
    }
    return ORBFE_OK;
}


// ---------------------------------------------------------------------------------------------
// orbfe_track_initialization: extract -> SearchForInitialization(resident initial frame, frame) as one captured hipGraph
// ---------------------------------------------------------------------------------------------
struct orbfe_init_frame {
    int device;
    unsigned long long serial;  // names the frame in graph keys (an address could be reused after a destroy)
    int n, n0;                  // keypoints, level-0 keypoints (the only ones SearchForInitialization walks, ORBmatcher.cc:346-347)
    void* block;
    const orbfe_keypoint* kp;
    const uint8_t* desc;
    const int* list0;           // level-0 keypoints in index order
};
static std::atomic<unsigned long long> g_initFrameSerial{1};

extern "C" int orbfe_init_frame_create(orbfe_handle* h, int n, const orbfe_keypoint* kp, const uint8_t* desc, orbfe_init_frame** out)
{
    if (!h || !out || n < 0 || (n > 0 && (!kp || !desc))) return ORBFE_ERR_INVALID_ARG;
    *out = nullptr;
    if (n >= (1 << 20)) return ORBFE_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(h->mu);
    HIPCHK(h, hipSetDevice(h->device));
    std::vector<int> list0;
    for (int i = 0; i < n; i++)
        if (kp[i].octave <= 0) list0.push_back(i);  // level1 > 0 -> continue (:346-347)
    Carver c;
    const size_t oKp = c.take((size_t)std::max(n, 1) * sizeof(orbfe_keypoint));
    const size_t oDesc = c.take((size_t)std::max(n, 1) * ORBFE_DESC_BYTES);
    const size_t oList = c.take((size_t)std::max(n, 1) * sizeof(int));  // n entries: the sequential matcher kernel rebuilds the list in place
    std::vector<uint8_t> img(c.off, 0);
    if (n) {
        memcpy(&img[oKp], kp, (size_t)n * sizeof(orbfe_keypoint));
        memcpy(&img[oDesc], desc, (size_t)n * ORBFE_DESC_BYTES);
    }
    if (!list0.empty()) memcpy(&img[oList], list0.data(), list0.size() * sizeof(int));
    void* block = nullptr;
    if (hipMalloc(&block, c.off) != hipSuccess) {
        (void)hipGetLastError();
        h->err = "orbfe_init_frame_create: allocation failed";
        return ORBFE_ERR_OUT_OF_MEMORY;
    }
    if (copy_sync(block, img.data(), c.off, hipMemcpyHostToDevice, h->stream) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(block);
        h->err = "orbfe_init_frame_create: upload failed";
        return ORBFE_ERR_HIP;
    }
    uint8_t* b = static_cast<uint8_t*>(block);
    *out = new orbfe_init_frame{h->device, g_initFrameSerial.fetch_add(1), n, (int)list0.size(), block,
                                reinterpret_cast<const orbfe_keypoint*>(b + oKp), b + oDesc, reinterpret_cast<const int*>(b + oList)};
    return ORBFE_OK;
}

extern "C" void orbfe_init_frame_destroy(orbfe_init_frame* f)
{
    if (!f) return;
    (void)hipSetDevice(f->device);
    (void)hipDeviceSynchronize();  // (a replay that reads the block may still be running on some handle's stream)
    if (f->block) (void)hipFree(f->block);
    delete f;
}

extern "C" int orbfe_init_frame_size(const orbfe_init_frame* f) { return f ? f->n : 0; }

namespace {

struct IniLayout : ChainPrefix {
    size_t inBytes;
    size_t oMatch, outBytes /* what is downloaded */, oScratch, devBytes;
};

IniLayout ini_layout(const orbfe_handle* h, int capN1, size_t scratchBytes)
{
    IniLayout L{};
    size_t off = chain_prefix_layout(h, L);
    L.inBytes = L.inFrame;
    L.oMatch = take256(off, (size_t)std::max(capN1, 1) * sizeof(int));
    L.outBytes = off;
    L.oScratch = take256(off, scratchBytes);
    L.devBytes = off;
    return L;
}

int ini_reserve(orbfe_handle* h, int n1, size_t scratchBytes)
{
    if (h->ini.dIn && n1 <= h->iniCapN1 && scratchBytes <= h->iniScratchBytes) return ORBFE_OK;
    h->iniGraphs.drop();
    h->iniCapN1 = -1;
    h->iniScratchBytes = 0;
    const int capN1 = std::max(n1 + n1 / 2, h->P.kpCapFrame);  // the initial frame is a frame of this extractor: <= kpCapFrame keypoints
    const size_t capScratch = std::max(scratchBytes + scratchBytes / 2, init_track_scratch_bytes(capN1, std::min(capN1, 1024), h->P.kpCapFrame));
    const IniLayout L = ini_layout(h, capN1, capScratch);
    const int rc = chain_blocks_alloc(h, h->ini, L.inBytes, L.devBytes, L.outBytes, "orbfe_track_initialization");
    if (rc != ORBFE_OK) return rc;
    h->iniCapN1 = capN1;
    h->iniScratchBytes = capScratch;
    return ORBFE_OK;
}

// the device side of one call, enqueued on s (directly, or under stream capture)
int ini_enqueue(orbfe_handle* h, const IniLayout& L, int inPitch, const orbfe_init_frame* f1, const orbfe_track_params* tp, int window,
                float nnRatio, int checkOri, hipStream_t s)
{
    const int cap = h->P.kpCapFrame;
    int* dHead = reinterpret_cast<int*>(h->ini.dOut);  // [n, status, n_matches]
    orbfe_keypoint* dKp = reinterpret_cast<orbfe_keypoint*>(h->ini.dOut + L.oKp);
    int rc = extract_chain(h, h->ini.dIn, L.inFrame, inPitch, 1, dKp, h->ini.dOut + L.oDesc, dHead, reinterpret_cast<int*>(h->ini.dOut + L.oPer),
                           dHead + 1, s);
    if (rc != ORBFE_OK) return rc;
    std::string err;
    rc = init_track_launch(s, f1->n, f1->n0, f1->kp, f1->desc, f1->list0, dKp, h->ini.dOut + L.oDesc, dHead, cap, tp->grid_cols, tp->grid_rows,
                           tp->min_x, tp->min_y, tp->grid_inv_w, tp->grid_inv_h, window, nnRatio, checkOri,
                           reinterpret_cast<int*>(h->ini.dOut + L.oMatch), dHead + 2, h->ini.dOut + L.oScratch, err);
    if (rc != ORBFE_OK) {
        h->err = err;
        return rc;
    }
    // [head | per-level | keypoints | descriptors | matches12 of THIS initial frame]: the block is laid out for iniCapN1 entries,
    // the copy stops behind the n1 that exist
    HIPCHK(h, hipMemcpyAsync(h->ini.hOut, h->ini.dOut, L.oMatch + (size_t)std::max(f1->n, 1) * sizeof(int), hipMemcpyDeviceToHost, s));
    return ORBFE_OK;
}

}  // namespace

extern "C" int orbfe_track_initialization(orbfe_handle* h, const uint8_t* gray, int pitch, const orbfe_init_frame* f1,
                                          const orbfe_track_params* tp, int window_size, float nn_ratio, int check_orientation,
                                          orbfe_keypoint* kp_out, uint8_t* desc_out, int* n_out, int* per_level, int* matches12_out,
                                          int* n_matches)
{
    if (!h || !gray || !f1 || !tp || !kp_out || !desc_out || !n_out || !n_matches || window_size < 0 || (f1->n > 0 && !matches12_out))
        return ORBFE_ERR_INVALID_ARG;
    if (pitch < h->prm.image_width || pitch >= (1 << 24) || f1->device != h->device) return ORBFE_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(h->mu);
    if (tp->struct_size != (int)sizeof(orbfe_track_params)) {
        h->err = "orbfe_track_params.struct_size does not match this library (rebuild the caller against include/orbfe.h)";
        return ORBFE_ERR_INVALID_ARG;
    }
    if (tp->grid_cols < 1 || tp->grid_rows < 1) return ORBFE_ERR_INVALID_ARG;
    if (h->P.kpCapFrame >= (1 << 20) || tp->grid_cols > 65535 || tp->grid_rows > 32767) return ORBFE_ERR_UNSUPPORTED;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    int rc = ini_reserve(h, f1->n, init_track_scratch_bytes(f1->n, f1->n0, h->P.kpCapFrame));
    if (rc != ORBFE_OK) return rc;
    const IniLayout L = ini_layout(h, h->iniCapN1, h->iniScratchBytes);

    // ---- upload: the frame alone ----
    int inPitch;
    rc = upload_frame(h, h->ini, gray, pitch, 0, 0, s, &inPitch);
    if (rc != ORBFE_OK) return rc;

    // ---- kernels + download: the graph of this (initial frame, pitch, parameters) ----
    orbfe_handle::IniKey key;
    memset(&key, 0, sizeof key);
    key.inPitch = inPitch; key.gridCols = tp->grid_cols; key.gridRows = tp->grid_rows; key.window = window_size;
    key.checkOri = check_orientation; key.minX = tp->min_x; key.minY = tp->min_y; key.invW = tp->grid_inv_w; key.invH = tp->grid_inv_h;
    key.nnRatio = nn_ratio; key.frameSerial = f1->serial;
    rc = chain_submit(h, h->iniGraphs, 8, key, h->ini, L.inFrame, inPitch, s,  // initial frames come and go (:569-602)
                      [&](hipStream_t q) { return ini_enqueue(h, L, inPitch, f1, tp, window_size, nn_ratio, check_orientation, q); },
                      "orbfe_track_initialization");
    if (rc != ORBFE_OK) return rc;

    // ---- hand over ----
    const int n = chain_prefix_copy_out(h, h->ini.hOut, L, kp_out, desc_out, n_out, per_level);
    if (n > 0 && f1->n > 0) {
        *n_matches = reinterpret_cast<const int*>(h->ini.hOut)[2];
        memcpy(matches12_out, h->ini.hOut + L.oMatch, (size_t)f1->n * sizeof(int));
    } else {  // the reference returns early on either empty frame (vnMatches12 all -1)
        *n_matches = 0;
        for (int i = 0; i < f1->n; i++) matches12_out[i] = -1;
    }
    return ORBFE_OK;
}
