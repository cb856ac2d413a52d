// local_map.cpp -- Tracking::UpdateLocalMap (src/Tracking.cc:1119-1324, SPEC DECISION S24) three ways on one scene file:
//   local_map.bin                          prints the library's version (the build-and-link test)
//   local_map.bin host  scene.bin out.bin  a plain C++ restatement on the flat arrays, no GPU: it has to equal tests/local_map_ref.py,
//                                          and it is the one-core yardstick of tests/tools/local_map_latency.py
//   local_map.bin time  scene.bin reps     that restatement timed: nanoseconds per frame, best of `reps` passes over the frames
//   local_map.bin gpu   scene.bin out.bin  include/orbfe_adaptor.hpp's ResidentCovisibility + LocalMapUpdater over mock KeyFrame /
//                                          MapPoint objects built from the scene (needs the GPU)
// The yardstick is friendlier to the CPU than the reference's own walk: flat arrays instead of shared_ptr graphs, std::map
// observations and mutexes; it allocates nothing per frame.
// Scene file (int32): kf_capacity capacity kf_stride obs_stride child_stride n_frames M max_local_kf n_covisible n_temporal inertial
// mark | per slot: set mn_id bad parent prev nf nc nch, points, covisibles, children | point_bad[capacity] | per point: n, slots |
// per frame: n_votes last_kf votes.   Output (int32) per frame: n_kfs n_points kfs[288] ids[M] n_votes votes_out.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
#include <tuple>
#include <vector>

#include "orbfe_adaptor.hpp"

namespace {

struct Kf {
    int set, mnId, bad, parent, prev;
    std::vector<int> points, covisible, children;
};
struct Frame {
    int lastKf;
    std::vector<int> votes;
};
struct Scene {
    int kfCap, cap, kfStride, obsStride, childStride, nFrames, M;
    orbfe_local_map_params p;
    std::vector<Kf> kf;
    std::vector<int> pointBad;
    std::vector<std::vector<int>> obs;
    std::vector<Frame> frames;
};
struct Result {
    int nKfs, nPoints;
    std::vector<int> kfs, ids, votes;
};

Scene load(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    std::vector<int> w;
    int buf[4096];
    size_t got;
    while ((got = fread(buf, sizeof(int), 4096, f)) > 0) w.insert(w.end(), buf, buf + got);
    fclose(f);
    size_t at = 0;
    auto take = [&]() { return w.at(at++); };
    auto list = [&](int n) { std::vector<int> v(w.begin() + (long)at, w.begin() + (long)at + n); at += (size_t)n; return v; };
    Scene s;
    s.kfCap = take(); s.cap = take(); s.kfStride = take(); s.obsStride = take(); s.childStride = take(); s.nFrames = take(); s.M = take();
    s.p = orbfe_local_map_params{(int)sizeof(orbfe_local_map_params), 0, 0, 0, 0, 0};
    s.p.max_local_kf = take(); s.p.n_covisible = take(); s.p.n_temporal = take(); s.p.inertial = take(); s.p.mark_voters_seen = take();
    s.kf.resize((size_t)s.kfCap);
    for (Kf& k : s.kf) {
        k.set = take(); k.mnId = take(); k.bad = take(); k.parent = take(); k.prev = take();
        const int nf = take(), nc = take(), nch = take();
        k.points = list(nf); k.covisible = list(nc); k.children = list(nch);
    }
    s.pointBad = list(s.cap);
    s.obs.resize((size_t)s.cap);
    for (auto& o : s.obs) o = list(take());
    s.frames.resize((size_t)s.nFrames);
    for (Frame& fr : s.frames) {
        const int n = take();
        fr.lastKf = take();
        fr.votes = list(n);
    }
    if (at != w.size()) { fprintf(stderr, "scene file: %zu words left\n", w.size() - at); exit(2); }
    return s;
}

void save(const char* path, const std::vector<Result>& out)
{
    FILE* f = fopen(path, "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
    for (const Result& r : out) {
        const int head[2] = {r.nKfs, r.nPoints}, n = (int)r.votes.size();
        fwrite(head, sizeof(int), 2, f);
        fwrite(r.kfs.data(), sizeof(int), r.kfs.size(), f);
        fwrite(r.ids.data(), sizeof(int), r.ids.size(), f);
        fwrite(&n, sizeof(int), 1, f);
        fwrite(r.votes.data(), sizeof(int), r.votes.size(), f);
    }
    fclose(f);
}

// S24 on the flat arrays.  The scratch lives across frames and is put back after each: nothing is allocated or cleared per frame.
class HostLocalMap {
public:
    explicit HostLocalMap(const Scene& s) : s_(s), count_((size_t)s.kfCap, 0), listed_((size_t)s.kfCap, 0), seen_((size_t)s.cap, 0), voted_((size_t)s.cap, 0)
    {
        touched_.reserve((size_t)s.kfCap);
        local_.reserve(ORBFE_LOCAL_KF_MAX);
    }
    void run(const Frame& fr, Result& r)
    {
        const Scene& s = s_;
        const orbfe_local_map_params& p = s.p;
        auto inKfs = [&](int k) { return k >= 0 && k < s.kfCap; };
        // 1. votes
        r.votes = fr.votes;
        touched_.clear();
        for (size_t i = 0; i < fr.votes.size(); i++) {
            const int id = fr.votes[i];
            if (id < 0 || id >= s.cap) continue;
            if (s.pointBad[(size_t)id]) { r.votes[i] = -1; continue; }
            voted_[(size_t)id] = 1;
            for (int k : s.obs[(size_t)id])
                if (count_[(size_t)k]++ == 0) touched_.push_back(k);
        }
        // 2. ranking: count descending, equal counts in ascending mn_id (S24), 3. the first nKFs, a bad one uses its place
        std::sort(touched_.begin(), touched_.end(), [&](int a, int b) {
            if (count_[(size_t)a] != count_[(size_t)b]) return count_[(size_t)a] > count_[(size_t)b];
            if (s.kf[(size_t)a].mnId != s.kf[(size_t)b].mnId) return s.kf[(size_t)a].mnId < s.kf[(size_t)b].mnId;
            return a < b;
        });
        local_.clear();
        auto append = [&](int k) { local_.push_back(k); listed_[(size_t)k] = 1; };
        const size_t nKFs = std::min((size_t)p.max_local_kf, touched_.size());
        for (size_t i = 0; i < nKFs; i++)
            if (!s.kf[(size_t)touched_[i]].bad) append(touched_[i]);
        // 4. expansion over the first phase
        const size_t nFirst = local_.size();
        for (size_t i = 0; i < nFirst; i++) {
            const Kf& k = s.kf[(size_t)local_[i]];
            const size_t nc = std::min(k.covisible.size(), (size_t)std::min(p.n_covisible, ORBFE_COVIS_MAX_COVISIBLE));
            for (size_t j = 0; j < nc; j++) {
                const int c = k.covisible[j];
                if (inKfs(c) && !s.kf[(size_t)c].bad && !listed_[(size_t)c]) { append(c); break; }
            }
            for (int c : k.children)
                if (inKfs(c) && !s.kf[(size_t)c].bad && !listed_[(size_t)c]) { append(c); break; }
            if (inKfs(k.parent) && !listed_[(size_t)k.parent]) { append(k.parent); break; }
        }
        // 5. temporal key frames
        if (p.inertial) {
            int t = fr.lastKf;
            for (int i = 0; i < p.n_temporal; i++) {
                if (!inKfs(t)) break;
                if (!listed_[(size_t)t]) { append(t); t = s.kf[(size_t)t].prev; }
            }
        }
        // 6. points: the list in reverse, slots ascending, first occurrence
        r.ids.assign((size_t)s.M, ORBFE_NO_POINT);
        int n = 0;
        for (size_t i = local_.size(); i-- > 0;)
            for (int id : s.kf[(size_t)local_[i]].points) {
                if (id < 0 || id >= s.cap || seen_[(size_t)id] || s.pointBad[(size_t)id]) continue;
                seen_[(size_t)id] = 1;
                if (n < s.M) r.ids[(size_t)n] = (p.mark_voters_seen && voted_[(size_t)id]) ? ~id : id;
                n++;
            }
        r.nPoints = n;
        r.nKfs = (int)local_.size();
        r.kfs.assign(ORBFE_LOCAL_KF_MAX, -1);
        std::copy(local_.begin(), local_.end(), r.kfs.begin());
        // put the scratch back: proportional to what was touched
        for (int k : touched_) count_[(size_t)k] = 0;
        for (int k : local_) {
            listed_[(size_t)k] = 0;
            for (int id : s.kf[(size_t)k].points)
                if (id >= 0 && id < s.cap) seen_[(size_t)id] = 0;
        }
        for (int id : fr.votes)
            if (id >= 0 && id < s.cap) voted_[(size_t)id] = 0;
    }

private:
    const Scene& s_;
    std::vector<int> count_, touched_, local_;
    std::vector<char> listed_, seen_, voted_;
};

// ---- the adaptor over mock objects with the members it reads ----
struct MockKF;
struct MockMP {
    int id = -1;
    bool bad = false;
    std::map<MockKF*, std::tuple<int, int>> obs;
    bool isBad() const { return bad; }
    const std::map<MockKF*, std::tuple<int, int>>& GetObservations() const { return obs; }
};
struct MockKF {
    long unsigned int mnId = 0;
    int slot = -1;
    bool bad = false;
    MockKF* parent = nullptr;
    MockKF* mPrevKF = nullptr;
    std::vector<MockMP*> mps;
    std::vector<MockKF*> ordered;
    std::set<MockKF*> childs;
    bool isBad() const { return bad; }
    MockKF* GetParent() const { return parent; }
    std::vector<MockMP*> GetMapPointMatches() const { return mps; }
    std::vector<MockKF*> GetBestCovisibilityKeyFrames(int N) const
    {
        return (int)ordered.size() < N ? ordered : std::vector<MockKF*>(ordered.begin(), ordered.begin() + N);
    }
    std::set<MockKF*> GetChilds() const { return childs; }
};

int run_gpu(const Scene& s, const char* outPath)
{
    orbfe_params prm{};
    prm.n_features = 1000; prm.n_fast_features = 40000; prm.scale_factor = 1.2f; prm.n_levels = 8; prm.ini_th_fast = 20; prm.min_th_fast = 7;
    prm.image_width = 752; prm.image_height = 480; prm.max_batch = 1;
    orbfe_handle* h = nullptr;
    if (orbfe_create(&prm, &h) != ORBFE_OK) { fprintf(stderr, "orbfe_create failed\n"); return 1; }
    int rc = 0;
    {
        ORB_SLAM3::ResidentMap map(h, s.cap);
        std::vector<orbfe_world_point> pts((size_t)s.cap);
        std::vector<int> all((size_t)s.cap);
        std::vector<uint8_t> desc((size_t)s.cap * 32, 0);
        for (int i = 0; i < s.cap; i++) {
            all[(size_t)i] = i;
            pts[(size_t)i] = orbfe_world_point{0, 0, 0, 1, 2, s.pointBad[(size_t)i], (int)s.obs[(size_t)i].size(), 0};
        }
        if (orbfe_map_update(h, const_cast<orbfe_map*>(map.get()), s.cap, all.data(), pts.data(), desc.data()) != ORBFE_OK) return 1;

        std::vector<MockMP> mp((size_t)s.cap);
        std::vector<MockKF> kf((size_t)s.kfCap);
        auto kfAt = [&](int k) { return k >= 0 && k < s.kfCap ? &kf[(size_t)k] : nullptr; };
        auto mpAt = [&](int id) { return id >= 0 && id < s.cap ? &mp[(size_t)id] : nullptr; };
        for (int i = 0; i < s.cap; i++) {
            mp[(size_t)i].id = i;
            mp[(size_t)i].bad = s.pointBad[(size_t)i] != 0;
            for (int k : s.obs[(size_t)i]) mp[(size_t)i].obs[&kf[(size_t)k]] = std::make_tuple(0, -1);
        }
        std::vector<MockKF*> setKfs;
        for (int k = 0; k < s.kfCap; k++) {
            const Kf& src = s.kf[(size_t)k];
            MockKF& d = kf[(size_t)k];
            d.slot = k; d.mnId = (long unsigned)src.mnId; d.bad = src.bad != 0; d.parent = kfAt(src.parent); d.mPrevKF = kfAt(src.prev);
            for (int id : src.points) d.mps.push_back(mpAt(id));
            for (int c : src.covisible) d.ordered.push_back(kfAt(c));
            for (int c : src.children) d.childs.insert(kfAt(c));
            if (src.set) setKfs.push_back(&d);
        }
        auto slotOf = [](const MockKF* p) { return p->slot; };
        auto idOf = [](const MockMP* p) { return p->id; };
        ORB_SLAM3::ResidentCovisibility graph(h, map, s.kfCap, s.kfStride, s.obsStride, s.childStride);
        graph.UpdateKeyFrames(setKfs, slotOf, idOf);
        std::vector<MockMP*> observed;
        for (MockMP& p : mp)
            if (!p.obs.empty()) observed.push_back(&p);
        graph.UpdateObservations(observed, idOf, slotOf);
        ORB_SLAM3::LocalMapUpdater updater(h, graph, s.M, s.p.max_local_kf, s.p.n_covisible, s.p.n_temporal);
        std::vector<Result> out;
        for (const Frame& fr : s.frames) {
            std::vector<MockMP*> voters;
            for (int id : fr.votes) voters.push_back(mpAt(id));
            std::vector<MockKF*> localKfs;
            std::vector<MockMP*> localMps;
            updater.Update(voters, kfAt(fr.lastKf), s.p.inertial != 0, s.p.mark_voters_seen != 0, idOf, slotOf, kfAt, mpAt, localKfs, localMps);
            Result r;
            r.nKfs = (int)localKfs.size();
            r.nPoints = updater.LocalPointCount();
            r.kfs.assign(ORBFE_LOCAL_KF_MAX, -1);
            for (size_t i = 0; i < localKfs.size(); i++) r.kfs[i] = localKfs[i]->slot;
            r.ids = updater.Ids();
            for (size_t i = 0; i < localMps.size(); i++)   // mvpLocalMapPoints names the same points as the id row
                if (localMps[i]->id != (r.ids[i] < 0 ? ~r.ids[i] : r.ids[i])) rc = 3;
            for (MockMP* v : voters) r.votes.push_back(v ? v->id : -1);
            out.push_back(r);
        }
        save(outPath, out);
    }
    orbfe_destroy(h);
    return rc;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 4) {
        printf("%s\n", orbfe_version());
        return 0;
    }
    const std::string mode = argv[1];
    const Scene s = load(argv[2]);
    if (mode == "gpu") return run_gpu(s, argv[3]);
    HostLocalMap host(s);
    std::vector<Result> out((size_t)s.nFrames);
    if (mode == "host") {
        for (int f = 0; f < s.nFrames; f++) host.run(s.frames[(size_t)f], out[(size_t)f]);
        save(argv[3], out);
        return 0;
    }
    if (mode == "time") {
        const int reps = atoi(argv[3]);
        double best = 1e30;
        long long check = 0;
        for (int rep = 0; rep < reps; rep++) {
            const auto t0 = std::chrono::steady_clock::now();
            for (int f = 0; f < s.nFrames; f++) host.run(s.frames[(size_t)f], out[(size_t)f]);
            const double ns = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / s.nFrames;
            best = std::min(best, ns);
            check += out[0].nPoints;
        }
        printf("{\"host_ns_per_frame\": %.1f, \"frames\": %d, \"reps\": %d, \"check\": %lld}\n", best, s.nFrames, reps, check);
        return 0;
    }
    fprintf(stderr, "unknown mode %s\n", mode.c_str());
    return 2;
}
