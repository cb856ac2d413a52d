// covis_update.cpp -- KeyFrame::UpdateConnections and the graph part of LocalMapping::ProcessNewKeyFrame (SPEC DECISION S25) on one
// scene file:
//   covis_update.bin                           prints the library's version (the build-and-link test)
//   covis_update.bin host  scene.bin out.bin   a plain C++ restatement on flat arrays, no GPU: it has to equal tests/covis_update_ref.py
//   covis_update.bin gpu   scene.bin out.bin   include/orbfe_adaptor.hpp's ResidentCovisibility::EnableConnections / AddKeyFrame /
//                                              UpdateConnections over mock KeyFrame / MapPoint objects (needs the GPU); the final
//                                              key frames are read back with orbfe_covis_get_keyframe
//   covis_update.bin push  scene.bin reps      the path before S25, timed (needs the GPU): the restatement computes the scene's
//                                              operations on the host and pushes every key frame and point it touched through
//                                              orbfe_covis_set_keyframes + orbfe_covis_set_observations; median microseconds per pass
// Scene file (int32): kf_capacity capacity kf_stride obs_stride child_stride conn_stride n_ops | per slot: set mn_id bad parent prev nf
// nc nch nconn, points, covisibles, children, (slot, weight) pairs | point_bad[capacity] | per point: n, slots | per operation:
// 0 slot mn_id bad parent prev n ids  (add)  or  1 n min_weight slots flags  (update).
// Output (int32): per add: n added[n] status; per updated key frame: count status slots[conn_stride] weights[conn_stride]; then per
// slot: mn_id bad parent prev nf nc covisibles nch children nconn pairs (ascending slot); then has_obs and, if 1, per point: n, slots.
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
    int set = 0, mnId = 0, bad = 1, parent = -1, prev = -1;
    std::vector<int> points, covisible, children;
    std::map<int, int> conn;
};
struct Op {
    int kind = 0, slot = 0, mnId = 0, bad = 0, parent = -1, prev = -1, minWeight = 50;
    std::vector<int> ids, slots, flags;
};
struct Scene {
    int kfCap, cap, kfStride, obsStride, childStride, connStride;
    std::vector<Kf> kf;
    std::vector<int> pointBad;
    std::vector<std::vector<int>> obs;
    std::vector<Op> ops;
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
    s.kfCap = take(); s.cap = take(); s.kfStride = take(); s.obsStride = take(); s.childStride = take(); s.connStride = take();
    const int nOps = take();
    s.kf.resize((size_t)s.kfCap);
    for (Kf& k : s.kf) {
        k.set = take(); k.mnId = take(); k.bad = take(); k.parent = take(); k.prev = take();
        const int nf = take(), nc = take(), nch = take(), nconn = take();
        k.points = list(nf); k.covisible = list(nc); k.children = list(nch);
        for (int i = 0; i < nconn; i++) { const int q = take(); k.conn[q] = take(); }
    }
    s.pointBad = list(s.cap);
    s.obs.resize((size_t)s.cap);
    for (auto& o : s.obs) o = list(take());
    s.ops.resize((size_t)nOps);
    for (Op& op : s.ops) {
        op.kind = take();
        if (op.kind == 0) {
            op.slot = take(); op.mnId = take(); op.bad = take(); op.parent = take(); op.prev = take();
            op.ids = list(take());
        } else {
            const int n = take();
            op.minWeight = take();
            op.slots = list(n); op.flags = list(n);
        }
    }
    if (at != w.size()) { fprintf(stderr, "scene file: %zu words left\n", w.size() - at); exit(2); }
    return s;
}

// ---- S25 on the flat arrays ----
// the order of mvpOrderedConnectedKeyFrames: weight descending, equal weights in descending mn_id, then descending slot
void order(const Scene& s, std::vector<std::pair<int, int>>& v)
{
    std::sort(v.begin(), v.end(), [&](const std::pair<int, int>& a, const std::pair<int, int>& b) {
        if (a.second != b.second) return a.second > b.second;
        if (s.kf[(size_t)a.first].mnId != s.kf[(size_t)b.first].mnId) return s.kf[(size_t)a.first].mnId > s.kf[(size_t)b.first].mnId;
        return a.first > b.first;
    });
}

void best_covisibles(Scene& s, int q)
{
    std::vector<std::pair<int, int>> v;
    for (const auto& e : s.kf[(size_t)q].conn)
        if (!s.kf[(size_t)e.first].bad) v.push_back(e);
    order(s, v);
    Kf& k = s.kf[(size_t)q];
    k.covisible.clear();
    for (size_t i = 0; i < v.size() && i < ORBFE_COVIS_MAX_COVISIBLE; i++) k.covisible.push_back(v[i].first);
}

// `touchedPts`: the points whose observation lists grew
int add_keyframe(Scene& s, const Op& op, std::vector<int>& added, std::vector<int>* touchedPts = nullptr)
{
    const size_t n = op.ids.size();
    added.assign(n, 0);
    std::vector<int> appends;
    std::set<int> seen;
    for (size_t i = 0; i < n; i++) {
        const int p = op.ids[i];
        if (p < 0 || p >= s.cap || s.pointBad[(size_t)p]) continue;
        const bool first = seen.insert(p).second;
        const auto& o = s.obs[(size_t)p];
        if (first && std::find(o.begin(), o.end(), op.slot) == o.end()) {
            appends.push_back(p);
            added[i] = 1;
        } else
            added[i] = 2;
    }
    for (int p : appends)
        if ((int)s.obs[(size_t)p].size() >= s.obsStride) {
            added.assign(n, 0);
            return ORBFE_COVIS_STATUS_REFUSED;
        }
    Kf& k = s.kf[(size_t)op.slot];
    k = Kf();
    k.set = 1; k.mnId = op.mnId; k.bad = op.bad; k.parent = op.parent; k.prev = op.prev;
    k.points = op.ids;
    for (int p : appends) s.obs[(size_t)p].push_back(op.slot);
    if (touchedPts) *touchedPts = appends;
    return ORBFE_COVIS_STATUS_OK;
}

// `touchedKfs`: the key frames whose record, head or children changed
int update_connections(Scene& s, int slot, int flag, int th, std::vector<int>& oSlots, std::vector<int>& oWeights, int& count,
                       std::vector<int>* touchedKfs = nullptr)
{
    oSlots.assign((size_t)s.connStride, -1);
    oWeights.assign((size_t)s.connStride, 0);
    count = 0;
    std::map<int, int> counter;
    for (int p : s.kf[(size_t)slot].points) {
        if (p < 0 || p >= s.cap || s.pointBad[(size_t)p]) continue;
        for (int o : s.obs[(size_t)p])
            if (o != slot && o >= 0 && o < s.kfCap && !s.kf[(size_t)o].bad) counter[o]++;
    }
    if (counter.empty()) return ORBFE_COVIS_STATUS_NO_COUNTS;
    int nmax = 0, kfmax = -1;
    std::vector<std::pair<int, int>> connected;
    for (const auto& e : counter) {
        if (kfmax < 0 || e.second > nmax || (e.second == nmax && s.kf[(size_t)e.first].mnId < s.kf[(size_t)kfmax].mnId)) {
            nmax = e.second;
            kfmax = e.first;
        }
        if (e.second >= th) connected.push_back(e);
    }
    if (connected.empty()) connected.emplace_back(kfmax, nmax);
    order(s, connected);
    const int par = connected[0].first;
    bool refused = (int)counter.size() > s.connStride;
    for (const auto& e : connected) {
        const auto& row = s.kf[(size_t)e.first].conn;
        refused = refused || (!row.count(slot) && (int)row.size() >= s.connStride);
    }
    const auto& kids = s.kf[(size_t)par].children;
    const bool isChild = std::find(kids.begin(), kids.end(), slot) != kids.end();
    refused = refused || ((flag & 1) && !isChild && (int)kids.size() >= s.childStride);
    if (refused) return ORBFE_COVIS_STATUS_REFUSED;
    for (const auto& e : connected) {
        auto& row = s.kf[(size_t)e.first].conn;
        const auto it = row.find(slot);
        if (it != row.end() && it->second == e.second) continue;
        row[slot] = e.second;
        best_covisibles(s, e.first);
        if (touchedKfs) touchedKfs->push_back(e.first);
    }
    Kf& k = s.kf[(size_t)slot];
    k.conn = counter;
    k.covisible.clear();
    for (size_t i = 0; i < connected.size() && i < ORBFE_COVIS_MAX_COVISIBLE; i++) k.covisible.push_back(connected[i].first);
    if (flag & 1) {
        k.parent = par;
        if (!isChild) s.kf[(size_t)par].children.push_back(slot);
        if (touchedKfs) touchedKfs->push_back(par);
    }
    if (touchedKfs) touchedKfs->push_back(slot);
    count = (int)connected.size();
    for (int i = 0; i < count; i++) {
        oSlots[(size_t)i] = connected[(size_t)i].first;
        oWeights[(size_t)i] = connected[(size_t)i].second;
    }
    return ORBFE_COVIS_STATUS_OK;
}

struct Out {
    std::vector<int> w;
    void put(int v) { w.push_back(v); }
    void put(const std::vector<int>& v) { w.insert(w.end(), v.begin(), v.end()); }
    void save(const char* path) const
    {
        FILE* f = fopen(path, "wb");
        if (!f) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
        fwrite(w.data(), sizeof(int), w.size(), f);
        fclose(f);
    }
};

void put_kf(Out& out, const Kf& k)
{
    out.put(k.mnId); out.put(k.bad); out.put(k.parent); out.put(k.prev); out.put((int)k.points.size());
    out.put((int)k.covisible.size()); out.put(k.covisible);
    out.put((int)k.children.size()); out.put(k.children);
    out.put((int)k.conn.size());
    for (const auto& e : k.conn) { out.put(e.first); out.put(e.second); }
}

int run_host(Scene s, const char* outPath)
{
    Out out;
    std::vector<int> a, b;
    for (const Op& op : s.ops) {
        if (op.kind == 0) {
            const int st = add_keyframe(s, op, a);
            out.put((int)a.size()); out.put(a); out.put(st);
        } else
            for (size_t i = 0; i < op.slots.size(); i++) {
                int count = 0;
                const int st = update_connections(s, op.slots[i], op.flags[i], op.minWeight, a, b, count);
                out.put(count); out.put(st); out.put(a); out.put(b);
            }
    }
    for (int k = 0; k < s.kfCap; k++) {
        Kf kf = s.kf[(size_t)k];
        if (!kf.set) { kf.mnId = k; kf.bad = 1; }
        put_kf(out, kf);
    }
    out.put(1);
    for (const auto& o : s.obs) { out.put((int)o.size()); out.put(o); }
    out.save(outPath);
    return 0;
}

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

orbfe_handle* create_handle()
{
    orbfe_params prm{};
    prm.n_features = 1000; prm.n_fast_features = 40000; prm.scale_factor = 1.2f; prm.n_levels = 8; prm.ini_th_fast = 20; prm.min_th_fast = 7;
    prm.image_width = 752; prm.image_height = 480; prm.max_batch = 1;
    orbfe_handle* h = nullptr;
    if (orbfe_create(&prm, &h) != ORBFE_OK) { fprintf(stderr, "orbfe_create failed\n"); exit(1); }
    return h;
}

void upload_points(orbfe_handle* h, const ORB_SLAM3::ResidentMap& map, const Scene& s)
{
    std::vector<orbfe_world_point> pts((size_t)s.cap);
    std::vector<int> all((size_t)s.cap);
    std::vector<uint8_t> desc((size_t)s.cap * 32, 0);
    for (int i = 0; i < s.cap; i++) {
        all[(size_t)i] = i;
        pts[(size_t)i] = orbfe_world_point{0, 0, 0, 1, 2, s.pointBad[(size_t)i], (int)s.obs[(size_t)i].size(), 0};
    }
    if (orbfe_map_update(h, const_cast<orbfe_map*>(map.get()), s.cap, all.data(), pts.data(), desc.data()) != ORBFE_OK) exit(1);
}

void import_connections(orbfe_handle* h, orbfe_covis* g, const Scene& s)
{
    std::vector<int> slots, off(1, 0), conn, w;
    for (int k = 0; k < s.kfCap; k++) {
        if (s.kf[(size_t)k].conn.empty()) continue;
        slots.push_back(k);
        for (const auto& e : s.kf[(size_t)k].conn) { conn.push_back(e.first); w.push_back(e.second); }
        off.push_back((int)conn.size());
    }
    if (orbfe_covis_set_connections(h, g, (int)slots.size(), slots.data(), off.data(), conn.data(), w.data()) != ORBFE_OK) exit(1);
}

int run_gpu(const Scene& s, const char* outPath)
{
    orbfe_handle* h = create_handle();
    {
        ORB_SLAM3::ResidentMap map(h, s.cap);
        upload_points(h, map, s);
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
        graph.EnableConnections(s.connStride);
        import_connections(h, graph.get(), s);

        Out out;
        for (const Op& op : s.ops) {
            if (op.kind == 0) {
                MockKF& d = kf[(size_t)op.slot];
                d.slot = op.slot; d.mnId = (long unsigned)op.mnId; d.bad = op.bad != 0; d.parent = kfAt(op.parent); d.mPrevKF = kfAt(op.prev);
                d.mps.clear();
                for (int id : op.ids) d.mps.push_back(mpAt(id));
                std::vector<int> added = graph.AddKeyFrame(&d, op.slot, slotOf, idOf);
                // a feature slot that names an id outside the map is a null pointer to the adaptor: the same "no point"
                out.put((int)added.size()); out.put(added); out.put(ORBFE_COVIS_STATUS_OK);
            } else
                for (size_t i = 0; i < op.slots.size(); i++) {
                    std::vector<int> sl, w;
                    const bool ok = graph.UpdateConnections(kfAt(op.slots[i]), slotOf, (op.flags[i] & 1) != 0, sl, w, op.minWeight);
                    out.put((int)sl.size()); out.put(ok ? ORBFE_COVIS_STATUS_OK : ORBFE_COVIS_STATUS_NO_COUNTS);
                    sl.resize((size_t)s.connStride, -1);
                    w.resize((size_t)s.connStride, 0);
                    out.put(sl); out.put(w);
                }
        }
        std::vector<int> cov(ORBFE_COVIS_MAX_COVISIBLE), kids((size_t)s.childStride), cs((size_t)s.connStride), cw((size_t)s.connStride);
        for (int k = 0; k < s.kfCap; k++) {
            orbfe_covis_keyframe r{};
            r.struct_size = (int)sizeof r;
            int nconn = 0;
            if (orbfe_covis_get_keyframe(h, graph.get(), k, &r, cov.data(), kids.data(), cs.data(), cw.data(), &nconn) != ORBFE_OK) return 1;
            Kf got;
            got.mnId = r.mn_id; got.bad = r.bad; got.parent = r.parent; got.prev = r.prev;
            got.points.resize((size_t)r.n_features);
            got.covisible.assign(cov.begin(), cov.begin() + r.n_covisible);
            got.children.assign(kids.begin(), kids.begin() + r.n_children);
            for (int i = 0; i < nconn; i++) got.conn[cs[(size_t)i]] = cw[(size_t)i];
            put_kf(out, got);
        }
        out.put(0);
        out.save(outPath);
    }
    orbfe_destroy(h);
    return 0;
}

// ---- the path before S25, timed: the host computes, then pushes what it touched ----
int run_push(const Scene& s0, int reps)
{
    orbfe_handle* h = create_handle();
    std::vector<double> us;
    int touchedKfs = 0, touchedPts = 0;
    {
        ORB_SLAM3::ResidentMap map(h, s0.cap);
        upload_points(h, map, s0);
        orbfe_covis* g = nullptr;
        if (orbfe_covis_create(h, map.get(), s0.kfCap, s0.kfStride, s0.obsStride, s0.childStride, &g) != ORBFE_OK) return 1;
        for (int rep = 0; rep < reps + 3; rep++) {
            Scene s = s0;  // (not timed)
            const auto t0 = std::chrono::steady_clock::now();
            std::vector<int> a, b, kfs, pts;
            for (const Op& op : s.ops) {
                if (op.kind == 0) {
                    add_keyframe(s, op, a, &pts);
                    kfs.push_back(op.slot);
                } else
                    for (size_t i = 0; i < op.slots.size(); i++) {
                        int count = 0;
                        update_connections(s, op.slots[i], op.flags[i], op.minWeight, a, b, count, &kfs);
                    }
            }
            std::sort(kfs.begin(), kfs.end());
            kfs.erase(std::unique(kfs.begin(), kfs.end()), kfs.end());
            std::vector<orbfe_covis_keyframe> recs(kfs.size());
            for (size_t i = 0; i < kfs.size(); i++) {
                const Kf& k = s.kf[(size_t)kfs[i]];
                orbfe_covis_keyframe r{};
                r.struct_size = (int)sizeof r;
                r.slot = kfs[i]; r.mn_id = k.mnId; r.bad = k.bad; r.parent = k.parent; r.prev = k.prev;
                r.n_features = (int)k.points.size(); r.n_covisible = (int)k.covisible.size(); r.n_children = (int)k.children.size();
                const bool isNew = std::any_of(s.ops.begin(), s.ops.end(), [&](const Op& op) { return op.kind == 0 && op.slot == kfs[i]; });
                r.point_ids = isNew ? k.points.data() : nullptr;   // only the new key frame's feature list goes up
                r.covisible = k.covisible.data(); r.children = k.children.data();
                recs[i] = r;
            }
            if (orbfe_covis_set_keyframes(h, g, (int)recs.size(), recs.data()) != ORBFE_OK) return 1;
            std::vector<int> off(1, 0), flat;
            for (int p : pts) {
                flat.insert(flat.end(), s.obs[(size_t)p].begin(), s.obs[(size_t)p].end());
                off.push_back((int)flat.size());
            }
            if (orbfe_covis_set_observations(h, g, (int)pts.size(), pts.data(), off.data(), flat.data()) != ORBFE_OK) return 1;
            const double t = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
            if (rep >= 3) us.push_back(t);
            touchedKfs = (int)kfs.size();
            touchedPts = (int)pts.size();
        }
        orbfe_covis_destroy(g);
    }
    orbfe_destroy(h);
    std::sort(us.begin(), us.end());
    printf("{\"push_us_median\": %.1f, \"push_us_min\": %.1f, \"reps\": %d, \"touched_kfs\": %d, \"touched_points\": %d}\n", us[us.size() / 2],
           us[0], reps, touchedKfs, touchedPts);
    return 0;
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
    if (mode == "host") return run_host(s, argv[3]);
    if (mode == "gpu") return run_gpu(s, argv[3]);
    if (mode == "push") return run_push(s, atoi(argv[3]));
    fprintf(stderr, "unknown mode %s\n", mode.c_str());
    return 2;
}
