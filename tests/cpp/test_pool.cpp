// The multi-device pool (orbfe_pool_*) from a plain C++ program through the adaptor's FramePool: extraction and
// extract-and-match of a set of host frames sharded over the members, compared byte for byte with orbfe_extract_batch and
// orbfe_track_frame_map on one plain handle of the same program.  Inputs come from files written by tests/test_pool_gpu.py.
//   usage: test_pool <W> <H> <n_frames> <frames.raw> <map.bin> <n_map> <frusta.bin> <ids.bin> <n_points> <devices, e.g. 0,0>
//   without arguments: the host-only checks (shard arithmetic, argument refusals) and the library version
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "orbfe_adaptor.hpp"

static std::vector<uint8_t> slurp(const char* p)
{
    std::ifstream f(p, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

static int host_only()
{
    int lo = 0, hi = 0, prev = 0;
    for (int k = 0; k < 3; k++) {  // 7 frames over 3 members: [0, 3) [3, 6) [6, 7)
        if (orbfe_shard_range(7, k, 3, &lo, &hi) != ORBFE_OK || lo != prev) return 1;
        prev = hi;
    }
    if (prev != 7 || orbfe_shard_range(7, 3, 3, &lo, &hi) != ORBFE_ERR_INVALID_ARG) return 1;
    orbfe_params p = {600, 24000, 1.2f, 6, 20, 7, 376, 240, 0, 16};
    const int dev[2] = {0, 0};
    orbfe_pool* pool = nullptr;
    if (orbfe_pool_create(&p, dev, 2, 1, 8, &pool) != ORBFE_ERR_INVALID_ARG || pool) return 1;  // one slot
    if (orbfe_pool_extract(nullptr, nullptr, 376, 1, nullptr, nullptr, nullptr, nullptr) != ORBFE_ERR_INVALID_ARG) return 1;
    orbfe_pool_destroy(nullptr);
    std::printf("%s host_only=1\n", orbfe_version());
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 11) return host_only();
    const int W = atoi(argv[1]), H = atoi(argv[2]), N = atoi(argv[3]), nMap = atoi(argv[6]), M = atoi(argv[9]);
    const auto img = slurp(argv[4]);
    const auto wraw = slurp(argv[5]);  // nMap x (orbfe_world_point + 32 descriptor bytes)
    const auto fraw = slurp(argv[7]);
    const auto iraw = slurp(argv[8]);
    if (img.size() < (size_t)N * W * H || wraw.size() < (size_t)nMap * 64 || fraw.size() < (size_t)N * sizeof(orbfe_frustum) ||
        iraw.size() < (size_t)N * M * sizeof(int))
        return 2;
    std::vector<int> devices;
    for (const char* s = argv[10]; *s;) {
        devices.push_back((int)strtol(s, const_cast<char**>(&s), 10));
        if (*s == ',') s++;
    }
    std::vector<orbfe_frustum> frusta((size_t)N);
    std::memcpy(frusta.data(), fraw.data(), frusta.size() * sizeof(orbfe_frustum));
    std::vector<int> ids((size_t)N * M);
    std::memcpy(ids.data(), iraw.data(), ids.size() * sizeof(int));
    std::vector<orbfe_world_point> pts((size_t)nMap);
    std::vector<uint8_t> mpd((size_t)nMap * 32);
    std::vector<int> mapIds((size_t)nMap);
    for (int i = 0; i < nMap; i++) {
        std::memcpy(&pts[(size_t)i], wraw.data() + (size_t)i * 64, 32);
        std::memcpy(&mpd[(size_t)i * 32], wraw.data() + (size_t)i * 64 + 32, 32);
        mapIds[(size_t)i] = i;
    }
    const int maxBatch = 16;
    orbfe_params p = {600, 24000, 1.2f, 6, 20, 7, W, H, 0, maxBatch};
    orbfe_track_params tp = ORBFE_TRACK_PARAMS_INIT;
    tp.grid_cols = 32;
    tp.grid_rows = 20;
    tp.grid_inv_w = 32.0f / (float)W;
    tp.grid_inv_h = 20.0f / (float)H;
    tp.th = 20.0f;
    tp.nn_ratio = 0.85f;

    std::vector<ORB_SLAM3::GrayImageView> views((size_t)N);
    std::vector<const uint8_t*> ptrs((size_t)N);
    for (int i = 0; i < N; i++) {
        ptrs[(size_t)i] = img.data() + (size_t)i * W * H;
        views[(size_t)i] = ORB_SLAM3::GrayImageView{ptrs[(size_t)i], W};
    }
    try {
        ORB_SLAM3::FramePool pool(p, devices, 3, 8);
        const size_t cap = (size_t)pool.Cap();
        const int nL = pool.Levels();
        std::vector<orbfe_keypoint> kp;
        std::vector<uint8_t> desc;
        std::vector<int> n, per, match, nm;
        pool.Extract(views, kp, desc, n, &per);

        // the same frames on one plain handle, max_batch at a time
        orbfe_handle* h = nullptr;
        if (orbfe_create(&p, &h) != ORBFE_OK) { std::puts("orbfe_create failed"); return 3; }
        std::vector<orbfe_keypoint> kp1(cap * maxBatch);
        std::vector<uint8_t> desc1(cap * maxBatch * 32);
        std::vector<int> n1(maxBatch), per1((size_t)maxBatch * nL), match1(cap);
        int sameExtract = 1;
        for (int lo = 0; lo < N; lo += maxBatch) {
            const int b = std::min(maxBatch, N - lo);
            if (orbfe_extract_batch(h, ptrs.data() + lo, W, b, kp1.data(), desc1.data(), n1.data(), per1.data()) != ORBFE_OK) return 4;
            for (int j = 0; j < b; j++) {
                const size_t i = (size_t)(lo + j);
                sameExtract &= n[i] == n1[(size_t)j] && std::memcmp(&kp[i * cap], &kp1[j * cap], (size_t)n1[(size_t)j] * sizeof(orbfe_keypoint)) == 0 &&
                               std::memcmp(&desc[i * cap * 32], &desc1[j * cap * 32], (size_t)n1[(size_t)j] * 32) == 0 &&
                               std::memcmp(&per[i * nL], &per1[(size_t)j * nL], (size_t)nL * sizeof(int)) == 0;
            }
        }

        pool.EnableTrack(nMap + 100, M);
        pool.MapUpdate(mapIds, pts, mpd);
        pool.Track(views, tp, frusta, M, ids, kp, desc, n, match, nm, &per);
        orbfe_map* map = nullptr;
        if (orbfe_map_create(h, nMap + 100, &map) != ORBFE_OK ||
            orbfe_map_update(h, map, nMap, mapIds.data(), pts.data(), mpd.data()) != ORBFE_OK)
            return 5;
        int sameTrack = 1;
        std::string counts;
        for (int i = 0; i < N; i++) {
            int k1 = 0, m1 = 0;
            if (orbfe_track_frame_map(h, ptrs[(size_t)i], W, &frusta[(size_t)i], &tp, map, M, ids.data() + (size_t)i * M, kp1.data(), desc1.data(), &k1,
                                      per1.data(), nullptr, nullptr, match1.data(), &m1) != ORBFE_OK)
                return 6;
            const size_t o = (size_t)i * cap;
            sameTrack &= n[(size_t)i] == k1 && nm[(size_t)i] == m1 && std::memcmp(&kp[o], kp1.data(), (size_t)k1 * sizeof(orbfe_keypoint)) == 0 &&
                         std::memcmp(&desc[o * 32], desc1.data(), (size_t)k1 * 32) == 0 &&
                         std::memcmp(&match[o], match1.data(), (size_t)k1 * sizeof(int)) == 0 &&
                         std::memcmp(&per[(size_t)i * nL], per1.data(), (size_t)nL * sizeof(int)) == 0;
            counts += (i ? "," : "") + std::to_string(m1);
        }
        std::string frames;
        for (int k = 0; k < pool.Size(); k++) frames += (k ? "," : "") + std::to_string(pool.MemberFrames(k));
        std::printf("pool_cpp members=%d member_frames=%s extract_same=%d track_same=%d matches=%s rc=0\n", pool.Size(), frames.c_str(),
                    sameExtract, sameTrack, counts.c_str());
        orbfe_map_destroy(map);
        orbfe_destroy(h);
    } catch (const std::exception& e) {
        std::printf("exception: %s\n", e.what());
        return 7;
    }
    return 0;
}
