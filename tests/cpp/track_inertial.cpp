// track_inertial.cpp -- include/orbfe_adaptor.hpp's InertialFrameTracker over CONSECUTIVE frames (SPEC DECISION S23), from a plain C++
// program: ResidentMap, ImuPreintegrator::Fresh and InertialFrameTracker::Track frame by frame, the caller's side of the hand-over
// written as INTEGRATION.md ("Between frames") tells a caller to:
//   key-frame kind  <=>  mbMapUpdated || !tracker.HasPrior();  its start state is the key frame's, else the last frame's
//   the last frame's state afterwards: Result::state -- unless the frame ran against the last frame and was not accepted, then
//   Result::predicted + 12 (pose and velocity of PredictStateIMU, the bias it copied); lastFrameBias = that state's bias
//   a new key frame: its state is the last frame's, tracker.ResetFromLastKF(imu.Fresh(its bias))
// The prior is passed on raw (Prior() is not touched).  tests/test_track_inertial_cpp.py writes the sequence and compares every
// field of every Result, the two records, HasPrior() and Prior() with the chain of restatements, byte for byte.
//   track_inertial.bin                    -> the library's version string
//   track_inertial.bin scene.bin out.bin  -> the sequence
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "orbfe_adaptor.hpp"

namespace {

template <class T>
void rd(std::ifstream& f, T* p, size_t n) { f.read(reinterpret_cast<char*>(p), (std::streamsize)(n * sizeof(T))); }
template <class T>
void wr(std::ofstream& f, const T* p, size_t n) { f.write(reinterpret_cast<const char*>(p), (std::streamsize)(n * sizeof(T))); }

// what ResidentMap::Update reads from a MapPoint
struct MapPoint {
    orbfe_world_point p;
    const uint8_t* desc;
    const float* GetWorldPos() const { return &p.x; }
    float mfMinDistance, mfMaxDistance;
    bool isBad() const { return p.bad != 0; }
    int Observations() const { return p.observations; }
};

struct FrameIn {
    std::vector<uint8_t> image;
    std::vector<orbfe_imu_sample> samples;
    double tPrev, tCur;
    std::vector<int> ids;
    int mapUpdated, fresh;
};

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 3) {
        std::printf("%s\n", orbfe_version());
        return 0;
    }
    std::ifstream f(argv[1], std::ios::binary);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    // the extractor (nFeatures nFastFeatures nLevels iniThFAST minThFAST W H, then scaleFactor), the sizes, the orbfe_track_inertial_params block
    int ei[7], K = 0, M = 0, capacity = 0, parBytes = 0;
    float scaleFactor = 0.0f;
    rd(f, ei, 7);
    rd(f, &scaleFactor, 1);
    rd(f, &K, 1);
    rd(f, &M, 1);
    rd(f, &capacity, 1);
    rd(f, &parBytes, 1);
    orbfe_track_inertial_params par;
    if (!f || parBytes != (int)sizeof par) { std::fprintf(stderr, "parameter block of %d bytes, expected %d\n", parBytes, (int)sizeof par); return 2; }
    rd(f, &par, 1);
    float stateKF[21], stateLast[21];
    orbfe_imu_preint kf0;
    rd(f, stateKF, 21);
    rd(f, stateLast, 21);
    rd(f, &kf0, 1);
    if (!f || K < 1 || M < 0 || capacity < 1 || kf0.struct_size != (int)sizeof kf0) { std::fprintf(stderr, "bad scene header\n"); return 2; }
    // the map
    std::vector<orbfe_world_point> pts((size_t)capacity);
    std::vector<uint8_t> desc((size_t)capacity * 32);
    rd(f, pts.data(), pts.size());
    rd(f, desc.data(), desc.size());
    const int W = ei[5], H = ei[6];
    std::vector<FrameIn> frames((size_t)K);
    for (FrameIn& fr : frames) {
        int nS = 0;
        fr.image.resize((size_t)W * H);
        rd(f, fr.image.data(), fr.image.size());
        rd(f, &nS, 1);
        if (!f || nS < 0 || nS > 100000) { std::fprintf(stderr, "bad frame\n"); return 2; }
        fr.samples.resize((size_t)nS);
        rd(f, fr.samples.data(), fr.samples.size());
        rd(f, &fr.tPrev, 1);
        rd(f, &fr.tCur, 1);
        fr.ids.resize((size_t)M);
        rd(f, fr.ids.data(), fr.ids.size());
        rd(f, &fr.mapUpdated, 1);
        rd(f, &fr.fresh, 1);
    }
    if (!f) { std::fprintf(stderr, "short scene file\n"); return 2; }

    ORB_SLAM3::ORBextractor ex(ei[0], ei[1], scaleFactor, ei[2], ei[3], ei[4], W, H);
    ORB_SLAM3::ResidentMap map(ex.handle(), capacity);
    {
        std::vector<MapPoint> store((size_t)capacity);
        std::vector<const MapPoint*> vp((size_t)capacity);
        std::vector<int> ids((size_t)capacity);
        for (int i = 0; i < capacity; i++) {
            store[(size_t)i] = MapPoint{pts[(size_t)i], &desc[(size_t)i * 32], pts[(size_t)i].min_distance, pts[(size_t)i].max_distance};
            vp[(size_t)i] = &store[(size_t)i];
            ids[(size_t)i] = i;
        }
        map.Update(vp, ids, [](const MapPoint* p) { return p->desc; });
    }
    std::array<float, 6> cov, walk;
    for (int i = 0; i < 6; i++) {
        cov[(size_t)i] = par.noise.cov[i];
        walk[(size_t)i] = par.noise.cov_walk[i];
    }
    ORB_SLAM3::ImuPreintegrator imu(ex, cov, walk, par.predict.gravity, par.predict.Rcb, par.predict.tcb, par.predict.tbc);
    ORB_SLAM3::InertialFrameTracker tracker(ex, par);
    tracker.ResetFromLastKF(kf0);

    std::ofstream o(argv[2], std::ios::binary);
    for (int k = 0; k < K; k++) {
        const FrameIn& fr = frames[(size_t)k];
        if (fr.fresh) {   // the last frame became a key frame
            std::memcpy(stateKF, stateLast, sizeof stateKF);
            tracker.ResetFromLastKF(imu.Fresh(stateLast + 15));
        }
        const bool keyFrameKind = fr.mapUpdated || !tracker.HasPrior();
        float lastFrameBias[6];
        std::memcpy(lastFrameBias, stateLast + 15, sizeof lastFrameBias);
        const ORB_SLAM3::InertialFrameTracker::Result r =
            tracker.Track(ORB_SLAM3::GrayImageView{fr.image.data(), W}, fr.samples, fr.tPrev, fr.tCur, lastFrameBias,
                          keyFrameKind ? stateKF : stateLast, fr.mapUpdated != 0, map, fr.ids);
        if (!keyFrameKind && !r.accepted) std::memcpy(stateLast, r.predicted + 12, sizeof stateLast);
        else std::memcpy(stateLast, r.state, sizeof stateLast);

        const int head[10] = {keyFrameKind ? 0 : 1, r.n, (int)r.steps.size(), r.nMatches, r.nInliers, r.matchesInliers, r.accepted ? 1 : 0,
                              r.tracked ? 1 : 0, r.infoOk ? 1 : 0, tracker.HasPrior() ? 1 : 0};
        wr(o, head, 10);
        wr(o, reinterpret_cast<const orbfe_keypoint*>(r.keys.data()), r.keys.size());
        wr(o, r.descriptors.data(), r.descriptors.size());
        wr(o, r.steps.data(), r.steps.size());
        wr(o, r.predicted, 33);
        wr(o, r.state, 21);
        wr(o, r.Tcw, 12);
        wr(o, r.points.data(), r.points.size());
        wr(o, r.match.data(), r.match.size());
        wr(o, r.outlier.data(), r.outlier.size());
        wr(o, r.found.data(), r.found.size());
        wr(o, &tracker.FromLastKF(), 1);
        wr(o, &tracker.FromLastFrame(), 1);
        wr(o, &tracker.Prior(), 1);
        std::printf("frame %d: %s n=%d matches=%d inliers=%d accepted=%d tracked=%d has_prior=%d\n", k, keyFrameKind ? "last key frame" : "last frame",
                    r.n, r.nMatches, r.nInliers, r.accepted ? 1 : 0, r.tracked ? 1 : 0, tracker.HasPrior() ? 1 : 0);
    }
    return o ? 0 : 2;
}
