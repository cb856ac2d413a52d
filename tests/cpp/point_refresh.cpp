// point_refresh.cpp -- MapPoint::UpdateDepth and MapPoint::ComputeDistinctiveDescriptors (SPEC DECISION S26) on one scene file:
//   point_refresh.bin                           prints the library's version (the build-and-link test)
//   point_refresh.bin host  scene.bin out.bin   a plain C++ restatement on flat arrays, no GPU, with the arithmetic of csrc/spec_math.h
//                                               and csrc/distinct_select.h: it has to equal tests/point_refresh_ref.py
//   point_refresh.bin gpu   scene.bin out.bin   include/orbfe_adaptor.hpp's ResidentCovisibility::EnableRefresh / SetFeatures /
//                                               SetCentres / SetObservations / SetReferenceKeyFrames / RefreshPoints over mock
//                                               KeyFrame / MapPoint objects (needs the GPU); the map records are read back with
//                                               orbfe_covis_get_point
// Scene file (int32 words, floats as their bit patterns): kf_capacity capacity kf_stride obs_stride n_levels n_ids what |
// sf[n_levels] | per slot: set mn_id bad n_feat, octave[n_feat], descriptors (8 words each), centre[3] | per point: bad ref n_obs,
// slots, indices, pos[3], min max, descriptor (8 words) | ids[n_ids].
// Output (int32 words): per entry: status min max slot index median; then per point: min max descriptor (8 words).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <tuple>
#include <vector>

#include "distinct_select.h"
#include "orbfe_adaptor.hpp"
#include "spec_math.h"

namespace {

struct Kf {
    int set = 0, mnId = 0, bad = 1;
    std::vector<int> octave;
    std::vector<uint8_t> desc;
    float centre[3] = {0, 0, 0};
};
struct Pt {
    int bad = 0, ref = -1;
    std::vector<int> slots, idx;
    float pos[3] = {0, 0, 0}, minD = 0, maxD = 0;
    uint8_t desc[32] = {};
};
struct Scene {
    int kfCap, cap, kfStride, obsStride, nLevels, what;
    std::vector<float> sf;
    std::vector<Kf> kf;
    std::vector<Pt> pt;
    std::vector<int> ids;
};

float as_float(int w) { float f; memcpy(&f, &w, 4); return f; }
int as_int(float f) { int w; memcpy(&w, &f, 4); return w; }

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
    auto bytes = [&](uint8_t* dst, int words) { memcpy(dst, w.data() + at, (size_t)words * 4); at += (size_t)words; };
    Scene s;
    s.kfCap = take(); s.cap = take(); s.kfStride = take(); s.obsStride = take(); s.nLevels = take();
    const int nIds = take();
    s.what = take();
    for (int i = 0; i < s.nLevels; i++) s.sf.push_back(as_float(take()));
    s.kf.resize((size_t)s.kfCap);
    for (Kf& k : s.kf) {
        k.set = take(); k.mnId = take(); k.bad = take();
        const int nf = take();
        k.octave = list(nf);
        k.desc.resize((size_t)nf * 32);
        bytes(k.desc.data(), nf * 8);
        for (float& c : k.centre) c = as_float(take());
    }
    s.pt.resize((size_t)s.cap);
    for (Pt& p : s.pt) {
        p.bad = take(); p.ref = take();
        const int n = take();
        p.slots = list(n); p.idx = list(n);
        for (float& c : p.pos) c = as_float(take());
        p.minD = as_float(take()); p.maxD = as_float(take());
        bytes(p.desc, 8);
    }
    s.ids = list(nIds);
    if (at != w.size()) { fprintf(stderr, "scene file: %zu words left\n", w.size() - at); exit(2); }
    return s;
}

struct Out {
    std::vector<int> w;
    void put(int v) { w.push_back(v); }
    void put(float v) { w.push_back(as_int(v)); }
    void desc(const uint8_t* d) { int v[8]; memcpy(v, d, 32); w.insert(w.end(), v, v + 8); }
    void save(const char* path) const
    {
        FILE* f = fopen(path, "wb");
        if (!f || fwrite(w.data(), sizeof(int), w.size(), f) != w.size()) { fprintf(stderr, "cannot write %s\n", path); exit(2); }
        fclose(f);
    }
};

// ---- S26 on the flat arrays ----
int hamming(const uint8_t* a, const uint8_t* b)
{
    int d = 0;
    for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

bool names_feature(const Scene& s, int slot, int idx) { return slot >= 0 && slot < s.kfCap && idx >= 0 && idx < (int)s.kf[(size_t)slot].octave.size(); }

struct Entry {
    int status = 0, slot = -1, index = -1, median = -1;
    float minD = 0, maxD = 0;
};

Entry refresh_point(Scene& s, int id, int what)
{
    Entry e;
    if (id < 0 || id >= s.cap) return e;
    Pt& p = s.pt[(size_t)id];
    if (p.bad || p.slots.empty()) return e;                    // :352, :357, :448, :455
    if (what & 1) {
        const int r = p.ref;
        const auto at = std::find(p.slots.begin(), p.slots.end(), r);
        const int idx = at == p.slots.end() ? 0 : p.idx[(size_t)(at - p.slots.begin())];   // :461 default-constructs (0, 0)
        if (names_feature(s, r, idx)) {                        // elsewhere the reference is undefined: nothing written
            const Kf& k = s.kf[(size_t)r];
            const float dist = orbfe::spec_point_distance(p.pos[0], p.pos[1], p.pos[2], k.centre[0], k.centre[1], k.centre[2]);
            orbfe::spec_update_depth(dist, s.sf[(size_t)k.octave[(size_t)idx]], s.sf[(size_t)s.nLevels - 1], p.minD, p.maxD);
            e.minD = p.minD;
            e.maxD = p.maxD;
            e.status |= 1;
        }
    }
    if (what & 2) {
        std::vector<int> got;                                  // positions in the list
        for (size_t j = 0; j < p.slots.size(); j++)
            if (names_feature(s, p.slots[j], p.idx[j]) && !s.kf[(size_t)p.slots[j]].bad) got.push_back((int)j);   // :366, :370
        const int N = (int)got.size();
        if (N > 0) {
            auto desc = [&](int j) { return s.kf[(size_t)p.slots[(size_t)j]].desc.data() + (size_t)p.idx[(size_t)j] * 32; };
            const int k = orbfe::distinct_median_position(N);
            unsigned long long best = orbfe::kDistinctNoObserver;
            for (int i : got) {
                const int median = orbfe::distinct_kth_distance(k, [&](int v) {
                    int c = 0;
                    for (int j : got) c += hamming(desc(i), desc(j)) <= v;
                    return c;
                });
                best = std::min(best, orbfe::distinct_pack_observer(median, s.kf[(size_t)p.slots[(size_t)i]].mnId, i));
            }
            const int win = (int)(best & 0xfffu);
            memcpy(p.desc, desc(win), 32);
            e.slot = p.slots[(size_t)win];
            e.index = p.idx[(size_t)win];
            e.median = (int)(best >> 44);
            e.status |= 2;
        }
    }
    return e;
}

void put_entry(Out& out, const Entry& e)
{
    out.put(e.status); out.put(e.minD); out.put(e.maxD); out.put(e.slot); out.put(e.index); out.put(e.median);
}

int run_host(Scene s, const char* outPath)
{
    Out out;
    for (int id : s.ids) put_entry(out, refresh_point(s, id, s.what));
    for (const Pt& p : s.pt) { out.put(p.minD); out.put(p.maxD); out.desc(p.desc); }
    out.save(outPath);
    return 0;
}

// ---- the adaptor over mock objects with the members it reads ----
struct MockKF;
struct MockMP {
    int id = -1;
    MockKF* ref = nullptr;
    std::map<MockKF*, std::tuple<int, int>> obs;
    const std::map<MockKF*, std::tuple<int, int>>& GetObservations() const { return obs; }
    MockKF* GetReferenceKeyFrame() const { return ref; }
};
struct MockKF {
    long unsigned int mnId = 0;
    int slot = -1;
    bool bad = false;
    MockKF* mPrevKF = nullptr;
    bool isBad() const { return bad; }
    MockKF* GetParent() const { return nullptr; }
    std::vector<MockMP*> GetMapPointMatches() const { return {}; }
    std::vector<MockKF*> GetBestCovisibilityKeyFrames(int) const { return {}; }
    std::set<MockKF*> GetChilds() const { return {}; }
};

int run_gpu(const Scene& s, const char* outPath)
{
    orbfe_params prm{};
    prm.n_features = 1000; prm.n_fast_features = 40000; prm.scale_factor = 1.2f; prm.n_levels = 8; prm.ini_th_fast = 20; prm.min_th_fast = 7;
    prm.image_width = 752; prm.image_height = 480; prm.max_batch = 1;
    orbfe_handle* h = nullptr;
    if (orbfe_create(&prm, &h) != ORBFE_OK) { fprintf(stderr, "orbfe_create failed\n"); return 1; }
    {
        ORB_SLAM3::ResidentMap map(h, s.cap);
        std::vector<orbfe_world_point> pts((size_t)s.cap);
        std::vector<int> all((size_t)s.cap);
        std::vector<uint8_t> desc((size_t)s.cap * 32);
        for (int i = 0; i < s.cap; i++) {
            const Pt& p = s.pt[(size_t)i];
            all[(size_t)i] = i;
            pts[(size_t)i] = orbfe_world_point{p.pos[0], p.pos[1], p.pos[2], p.minD, p.maxD, p.bad, (int)p.slots.size(), 0};
            memcpy(desc.data() + (size_t)i * 32, p.desc, 32);
        }
        if (orbfe_map_update(h, const_cast<orbfe_map*>(map.get()), s.cap, all.data(), pts.data(), desc.data()) != ORBFE_OK) return 1;
        std::vector<MockKF> kf((size_t)s.kfCap);
        std::vector<MockMP> mp((size_t)s.cap);
        std::vector<MockKF*> setKfs;
        std::vector<int> slots;
        std::vector<float> twc;
        for (int k = 0; k < s.kfCap; k++) {
            kf[(size_t)k].mnId = (long unsigned int)s.kf[(size_t)k].mnId;
            kf[(size_t)k].slot = k;
            kf[(size_t)k].bad = s.kf[(size_t)k].bad != 0;
            if (s.kf[(size_t)k].set) setKfs.push_back(&kf[(size_t)k]);
            slots.push_back(k);
            twc.insert(twc.end(), s.kf[(size_t)k].centre, s.kf[(size_t)k].centre + 3);
        }
        std::vector<MockMP*> mps;
        for (int i = 0; i < s.cap; i++) {
            const Pt& p = s.pt[(size_t)i];
            mp[(size_t)i].id = i;
            mp[(size_t)i].ref = p.ref >= 0 && p.ref < s.kfCap ? &kf[(size_t)p.ref] : nullptr;
            for (size_t j = 0; j < p.slots.size(); j++) mp[(size_t)i].obs[&kf[(size_t)p.slots[j]]] = std::make_tuple(p.idx[j], -1);
            mps.push_back(&mp[(size_t)i]);
        }
        auto slotOf = [](const MockKF* k) { return k->slot; };
        auto idOf = [](const MockMP* m) { return m->id; };
        ORB_SLAM3::ResidentCovisibility cv(h, map, s.kfCap, s.kfStride, s.obsStride, 4);
        cv.UpdateKeyFrames(setKfs, slotOf, idOf);
        cv.EnableRefresh(s.sf);
        for (int k = 0; k < s.kfCap; k++)
            if (!s.kf[(size_t)k].octave.empty()) cv.SetFeatures(k, s.kf[(size_t)k].octave, s.kf[(size_t)k].desc);
        cv.SetCentres(slots, twc);
        cv.SetObservations(mps, idOf, slotOf);
        cv.SetReferenceKeyFrames(mps, idOf, slotOf);
        const auto r = cv.RefreshPoints(s.ids, s.what);
        Out out;
        for (size_t e = 0; e < s.ids.size(); e++) {
            out.put(r.status[e]); out.put(r.minDistance[e]); out.put(r.maxDistance[e]);
            out.put(r.bestSlot[e]); out.put(r.bestIndex[e]); out.put(r.bestMedian[e]);
        }
        std::vector<int> a((size_t)s.obsStride), b((size_t)s.obsStride);
        for (int i = 0; i < s.cap; i++) {
            int n = 0, ref = 0;
            orbfe_world_point rec{};
            uint8_t d[32];
            if (orbfe_covis_get_point(h, cv.get(), i, &n, a.data(), b.data(), &ref, &rec, d) != ORBFE_OK) return 1;
            out.put(rec.min_distance); out.put(rec.max_distance); out.desc(d);
        }
        out.save(outPath);
    }
    orbfe_destroy(h);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc == 1) {
        printf("%s\n", orbfe_version());
        return 0;
    }
    if (argc != 4) { fprintf(stderr, "usage: point_refresh.bin [host|gpu scene.bin out.bin]\n"); return 2; }
    const std::string mode = argv[1];
    const Scene s = load(argv[2]);
    try {
        if (mode == "host") return run_host(s, argv[3]);
        if (mode == "gpu") return run_gpu(s, argv[3]);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 2;
}
