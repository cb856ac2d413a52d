// The first loop of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:819-824) the way a binding drives it: mock MapPoint /
// KeyFrame types whose Replace really hands over observations and recomputes the survivor's descriptor (host median scan,
// src/MapPoint.cc:343-416), include/orbfe_adaptor.hpp's NeighbourFuseBatch against the loop of K ResidentFuse::Fuse calls with
// the ResidentMap updated between them, on two copies of one scene.  Both must end with identical graphs: bad flags,
// observations, descriptors, the key frames' slots, nFused per target.  Prints the timing line of the whole replay.
//   usage: fuse_neighbors <scene.bin> <fobs_lo> <fobs_hi> <inkf> [reps] [cand_cap]      (scene.bin: see tests/test_fuse_neighbors_cpp.py)
#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <random>
#include <set>

#include "orbfe_adaptor.hpp"

using namespace ORB_SLAM3;
using Desc = std::array<uint8_t, 32>;

struct KeyFrame;
struct ByIndex {  // key frames in the order of the loop, not of their addresses: the two worlds must iterate alike
    bool operator()(const KeyFrame* a, const KeyFrame* b) const;
};

struct MapPoint : std::enable_shared_from_this<MapPoint> {
    int id = -1;
    float pos[3] = {0, 0, 0};
    float mfMinDistance = 0, mfMaxDistance = 0;
    bool bad = false;
    Desc desc{};
    std::vector<Desc> extra;             // descriptors of observations outside the K targets
    std::map<KeyFrame*, int, ByIndex> obs;       // observations in the targets
    std::set<KeyFrame*, ByIndex> in;            // IsInKeyFrame
    std::array<float, 3> GetWorldPos() const { return {pos[0], pos[1], pos[2]}; }
    bool isBad() const { return bad; }
    int Observations() const { return (int)(extra.size() + obs.size()); }
    bool IsInKeyFrame(const std::shared_ptr<KeyFrame>& kf) const { return in.count(kf.get()) != 0; }
    void AddObservation(const std::shared_ptr<KeyFrame>& kf, int idx) { AddObservation(kf.get(), idx); }
    void AddObservation(KeyFrame* kf, int idx)
    {
        obs[kf] = idx;
        in.insert(kf);
    }
    void Replace(const std::shared_ptr<MapPoint>& other);
    void ComputeDistinctiveDescriptors();
};

struct KeyFrame {
    int N = 0, index = -1;
    std::shared_ptr<std::vector<KeyPoint>> mvKeysUn;
    std::vector<uint8_t> mDescriptors;
    std::map<unsigned, std::vector<unsigned>> mFeatVec;
    std::vector<std::shared_ptr<MapPoint>> mvpMapPoints;
    std::vector<float> mvuRight, mvScaleFactors, mvInvLevelSigma2;
    int mnGridCols = 64, mnGridRows = 48;
    float mnMinX = 0, mnMinY = 0, mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
    std::shared_ptr<MapPoint> GetMapPoint(size_t i) const { return mvpMapPoints[i]; }
    void AddMapPoint(const std::shared_ptr<MapPoint>& mp, size_t i) { mvpMapPoints[i] = mp; }
};

bool ByIndex::operator()(const KeyFrame* a, const KeyFrame* b) const { return a->index < b->index; }

void MapPoint::ComputeDistinctiveDescriptors()
{
    std::vector<Desc> v(extra);
    for (const auto& o : obs) {
        Desc d;
        std::memcpy(d.data(), &o.first->mDescriptors[(size_t)o.second * 32], 32);
        v.push_back(d);
    }
    if (v.empty()) return;
    const size_t n = v.size();
    int bestMedian = 1 << 30;
    size_t best = 0;
    std::vector<int> dist(n);
    for (size_t i = 0; i < n; i++) {
        for (size_t j = 0; j < n; j++) dist[j] = orbfe_hamming(v[i].data(), v[j].data());
        std::sort(dist.begin(), dist.end());
        const int median = dist[(size_t)(0.5 * (double)(n - 1))];
        if (median < bestMedian) {
            bestMedian = median;
            best = i;
        }
    }
    desc = v[best];
}

void MapPoint::Replace(const std::shared_ptr<MapPoint>& other)  // src/MapPoint.cc:262-314
{
    if (other.get() == this) return;
    bad = true;
    auto self = shared_from_this();
    for (const auto& o : obs) {
        KeyFrame* kf = o.first;
        if (!other->in.count(kf)) {
            kf->mvpMapPoints[(size_t)o.second] = other;  // ReplaceMapPointMatch
            other->AddObservation(kf, o.second);
        } else if (kf->mvpMapPoints[(size_t)o.second] == self) {
            kf->mvpMapPoints[(size_t)o.second] = nullptr;  // EraseMapPointMatch
        }
    }
    for (KeyFrame* kf : in) other->in.insert(kf);
    for (const Desc& d : extra) other->extra.push_back(d);
    obs.clear();
    extra.clear();
    other->ComputeDistinctiveDescriptors();  // :311
}

struct Scene {
    int K = 0, M = 0, L = 0;
    std::vector<float> sf, is2;
    orbfe_frustum fr{};
    std::vector<orbfe_world_point> pts;
    std::vector<uint8_t> mpd;
    std::vector<int> n;
    std::vector<std::vector<KeyPoint>> kp;
    std::vector<std::vector<uint8_t>> desc;
};

static bool read_scene(const char* path, Scene& s)
{
    std::ifstream f(path, std::ios::binary);
    int hdr[3];
    if (!f.read(reinterpret_cast<char*>(hdr), sizeof hdr)) return false;
    s.K = hdr[0]; s.M = hdr[1]; s.L = hdr[2];
    if (s.K < 0 || s.M < 0 || s.L < 1 || s.L > ORBFE_MAX_LEVELS) return false;
    s.sf.resize((size_t)s.L);
    s.is2.resize((size_t)s.L);
    f.read(reinterpret_cast<char*>(s.sf.data()), s.L * 4);
    f.read(reinterpret_cast<char*>(s.is2.data()), s.L * 4);
    f.read(reinterpret_cast<char*>(&s.fr), sizeof s.fr);
    s.pts.resize((size_t)s.M);
    s.mpd.resize((size_t)s.M * 32);
    f.read(reinterpret_cast<char*>(s.pts.data()), (std::streamsize)(s.pts.size() * sizeof(orbfe_world_point)));
    f.read(reinterpret_cast<char*>(s.mpd.data()), (std::streamsize)s.mpd.size());
    for (int k = 0; k < s.K; k++) {
        int n = 0;
        f.read(reinterpret_cast<char*>(&n), 4);
        if (!f || n < 0) return false;
        s.n.push_back(n);
        s.kp.emplace_back((size_t)n);
        s.desc.emplace_back((size_t)n * 32);
        f.read(reinterpret_cast<char*>(s.kp.back().data()), (std::streamsize)((size_t)n * sizeof(KeyPoint)));
        f.read(reinterpret_cast<char*>(s.desc.back().data()), (std::streamsize)((size_t)n * 32));
    }
    return (bool)f;
}

static Desc flipped(const uint8_t* d, int bits, std::mt19937& rng)
{
    Desc o;
    std::memcpy(o.data(), d, 32);
    for (int b = 0; b < bits; b++) {
        const unsigned p = rng() % 256;
        o[p >> 3] ^= (uint8_t)(1u << (p & 7));
    }
    return o;
}

struct World {
    std::vector<std::shared_ptr<KeyFrame>> kfs;
    std::vector<std::shared_ptr<MapPoint>> mps;   // vpMapPointMatches
    std::vector<std::shared_ptr<MapPoint>> all;   // + the targets' own points, by id
};

// the graph at the start of the loop: half of every target's features carry a point of the target's own (fobsLo..fobsHi-1
// observations), a share `inkf` of our points is already observed in each target
static World build(const Scene& s, int fobsLo, int fobsHi, double inkf, unsigned seed)
{
    World w;
    std::mt19937 rng(seed);
    auto uni = [&] { return (double)(rng() >> 8) / (double)(1u << 24); };
    for (int i = 0; i < s.M; i++) {
        auto p = std::make_shared<MapPoint>();
        p->id = (int)w.all.size();
        std::memcpy(p->pos, &s.pts[(size_t)i].x, 12);
        p->mfMinDistance = s.pts[(size_t)i].min_distance;
        p->mfMaxDistance = s.pts[(size_t)i].max_distance;
        p->bad = s.pts[(size_t)i].bad != 0;
        std::memcpy(p->desc.data(), &s.mpd[(size_t)i * 32], 32);
        const int ne = 2 + (int)(rng() % 3);
        for (int e = 0; e < ne; e++) p->extra.push_back(flipped(p->desc.data(), (int)(rng() % 8), rng));
        w.mps.push_back(p);
        w.all.push_back(p);
    }
    for (int k = 0; k < s.K; k++) {
        auto kf = std::make_shared<KeyFrame>();
        kf->index = k;
        kf->N = s.n[(size_t)k];
        kf->mvKeysUn = std::make_shared<std::vector<KeyPoint>>(s.kp[(size_t)k]);
        kf->mDescriptors = s.desc[(size_t)k];
        kf->mvuRight.assign((size_t)kf->N, -1.0f);
        kf->mvScaleFactors = s.sf;
        kf->mvInvLevelSigma2 = s.is2;
        kf->mfGridElementWidthInv = 64.0f / (s.fr.max_x - s.fr.min_x);
        kf->mfGridElementHeightInv = 48.0f / (s.fr.max_y - s.fr.min_y);
        kf->mnMinX = s.fr.min_x;
        kf->mnMinY = s.fr.min_y;
        kf->mvpMapPoints.resize((size_t)kf->N);
        for (int f = 0; f < kf->N; f++) {
            if (uni() >= 0.5) continue;
            auto q = std::make_shared<MapPoint>();
            q->id = (int)w.all.size();
            const uint8_t* d = &kf->mDescriptors[(size_t)f * 32];
            std::memcpy(q->desc.data(), d, 32);
            const int ne = fobsLo + (int)(rng() % (unsigned)std::max(fobsHi - fobsLo, 1)) - 1;  // + the observation in this target
            for (int e = 0; e < ne; e++) q->extra.push_back(flipped(d, (int)(rng() % 8), rng));
            q->AddObservation(kf.get(), f);
            kf->mvpMapPoints[(size_t)f] = q;
            w.all.push_back(q);
        }
        for (int i = 0; i < s.M; i++)
            if (uni() < inkf) w.mps[(size_t)i]->in.insert(kf.get());
        w.kfs.push_back(kf);
    }
    return w;
}

// everything the loop can change, as comparable records
static std::vector<int> snapshot(const World& w, const std::vector<int>& nFused)
{
    std::vector<int> out(nFused);
    for (const auto& p : w.all) {
        out.push_back(p->bad);
        out.push_back(p->Observations());
        for (int b = 0; b < 32; b += 4) {
            int v;
            std::memcpy(&v, &p->desc[(size_t)b], 4);
            out.push_back(v);
        }
        for (const auto& kf : w.kfs) out.push_back(p->in.count(kf.get()) ? 1 : 0);
        for (const auto& o : p->obs) {
            out.push_back(o.first->index);
            out.push_back(o.second);
        }
    }
    for (const auto& kf : w.kfs)
        for (const auto& q : kf->mvpMapPoints) out.push_back(q ? q->id : -1);
    return out;
}

static double now_us()
{
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char** argv)
{
    if (argc < 5) { std::printf("%s\n", orbfe_version()); return 0; }
    Scene s;
    if (!read_scene(argv[1], s)) return 2;
    const int fobsLo = atoi(argv[2]), fobsHi = atoi(argv[3]);
    const double inkf = atof(argv[4]);
    const int reps = argc > 5 ? atoi(argv[5]) : 5;
    const int candCap = argc > 6 ? atoi(argv[6]) : 4;
    const float th = 10.0f;
    orbfe_params p = {1000, 40000, 1.2f, 8, 20, 7, 752, 480, 0, 1};
    orbfe_handle* h = nullptr;
    if (orbfe_create(&p, &h) != ORBFE_OK) { std::puts("orbfe_create failed"); return 3; }
    int same = 1, fused = 0, submissions = 0, selects = 0, overflows = 0;
    size_t aboveCap = 0;
    std::vector<double> tSeq, tBatch;
    {
        auto descOfKF = [](const std::shared_ptr<KeyFrame>& kf) { return kf->mDescriptors.data(); };
        auto descOfMP = [](const std::shared_ptr<MapPoint>& mp) { return mp->desc.data(); };
        const World w0 = build(s, fobsLo, fobsHi, inkf, 7);
        std::vector<std::unique_ptr<ResidentKeyFrame>> own;
        std::vector<const ResidentKeyFrame*> res;
        for (const auto& kf : w0.kfs) {  // the key frames' own arrays never change: one resident copy serves every world
            own.emplace_back(new ResidentKeyFrame(h, kf, descOfKF));
            own.back()->SetGrid(h, kf);
            res.push_back(own.back().get());
        }
        std::vector<int> ids((size_t)s.M);
        for (int i = 0; i < s.M; i++) ids[(size_t)i] = i;
        const std::vector<orbfe_frustum> frusta((size_t)s.K, s.fr);
        ResidentMap map(h, std::max(s.M, 1));
        for (int r = 0; r < reps; r++) {
            // ---- K sequential calls, the ResidentMap updated between them ----
            World a = build(s, fobsLo, fobsHi, inkf, 7);
            map.Update(a.mps, ids, descOfMP);
            std::vector<int> nA;
            {
                std::vector<Desc> pushed;
                std::vector<uint8_t> pushedBad;
                for (const auto& q : a.mps) {
                    pushed.push_back(q->desc);
                    pushedBad.push_back(q->bad);
                }
                const double t0 = now_us();
                for (int k = 0; k < s.K; k++) {
                    nA.push_back(ResidentFuse::Fuse(h, a.kfs[(size_t)k], *res[(size_t)k], map, a.mps, ids, th, s.fr));
                    std::vector<std::shared_ptr<MapPoint>> ch;  // what the edits changed reaches the map before the next call
                    std::vector<int> chIds;
                    for (int i = 0; i < s.M; i++) {
                        const auto& q = a.mps[(size_t)i];
                        if (q->desc != pushed[(size_t)i] || (uint8_t)q->bad != pushedBad[(size_t)i]) {
                            ch.push_back(q);
                            chIds.push_back(i);
                            pushed[(size_t)i] = q->desc;
                            pushedBad[(size_t)i] = q->bad;
                        }
                    }
                    if (!ch.empty()) map.Update(ch, chIds, descOfMP);
                }
                tSeq.push_back(now_us() - t0);
            }
            // ---- one submission + replay ----
            World b = build(s, fobsLo, fobsHi, inkf, 7);
            map.Update(b.mps, ids, descOfMP);
            std::vector<int> nB;
            {
                std::vector<Desc> start;
                std::vector<uint8_t> startBad;
                for (const auto& q : b.mps) {
                    start.push_back(q->desc);
                    startBad.push_back(q->bad);
                }
                const double t0 = now_us();
                NeighbourFuseBatch batch(h, b.kfs, res, frusta, map, b.mps, ids, th, descOfKF, descOfMP, candCap);
                for (int k = 0; k < s.K; k++) nB.push_back(batch.Fuse(k, b.kfs[(size_t)k], b.mps, descOfMP));
                std::vector<std::shared_ptr<MapPoint>> ch;  // the map catches up once, after the loop
                std::vector<int> chIds;
                for (int i = 0; i < s.M; i++) {
                    const auto& q = b.mps[(size_t)i];
                    if (q->desc != start[(size_t)i] || (uint8_t)q->bad != startBad[(size_t)i]) {
                        ch.push_back(q);
                        chIds.push_back(i);
                    }
                }
                if (!ch.empty()) map.Update(ch, chIds, descOfMP);
                tBatch.push_back(now_us() - t0);
                submissions = batch.Submissions();
                selects = batch.HostSelects();
                overflows = batch.Overflows();
                aboveCap = batch.PairsAboveCap();
            }
            if (snapshot(a, nA) != snapshot(b, nB)) same = 0;
            fused = 0;
            for (int v : nB) fused += v;
        }
    }
    // the host scan alone: `selects` calls on a 4-entry list
    double selectUs = 0.0;
    if (s.K > 0 && s.n[0] >= 4) {
        const int cand[4] = {0, 1, 2, 3};
        int bi = 0, bd = 0, acc = 0;
        const int loops = 200000;
        const double t0 = now_us();
        for (int i = 0; i < loops; i++) {
            orbfe_fuse_select(cand, 1 + (i & 3), 4, s.desc[0].data(), s.n[0], &s.mpd[(size_t)(i % std::max(s.M, 1)) * 32], &bi, &bd);
            acc += bd;
        }
        selectUs = (now_us() - t0) / loops;
        if (acc == -1) std::puts("");
    }
    std::sort(tSeq.begin(), tSeq.end());
    std::sort(tBatch.begin(), tBatch.end());
    std::printf("fuse_neighbors K=%d M=%d fused=%d same=%d submissions=%d host_selects=%d overflows=%d pairs_above_cap=%zu\n", s.K, s.M,
                fused, same, submissions, selects, overflows, aboveCap);
    std::printf("fuse_neighbors_latency_us sequential_loop=%.1f batch_replay=%.1f reps=%d select_us_per_call=%.4f select_us_total=%.1f\n",
                tSeq.empty() ? 0.0 : tSeq[tSeq.size() / 2], tBatch.empty() ? 0.0 : tBatch[tBatch.size() / 2], reps, selectUs,
                selectUs * selects);
    orbfe_destroy(h);
    return same ? 0 : 1;
}
