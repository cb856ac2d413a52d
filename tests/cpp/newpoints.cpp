// The neighbour loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:453-725) the way a binding drives it: light mock
// KeyFrame types, include/orbfe_adaptor.hpp's NewMapPointsBatch, pKF1->AddMapPoint between the neighbours.  Writes the created
// points for tests/test_newpoints_cpp.py and times, on the same inputs,
//   (a) orbfe_match_triangulation_batch, (b) orbfe_create_new_points_batch (three alternations, median of `reps` calls each),
//   (c) the geometry of SPEC DECISION S11 as a single-thread host loop (Pinhole cameras; this file, -O2) over the matches the
//       K orbfe_triangulation_select calls return -- what the mapping thread computes itself when it only has (a).
// The host loop's verdicts and points must equal the library's bit for bit (its Jacobi sequence is csrc/jacobi.h's text; the rest is restated).
//   usage: newpoints <scene.bin> <out.bin> [reps]      (scene.bin: see tests/test_newpoints_cpp.py)
// -DNEWPOINTS_SEARCH_ONLY builds (a) alone, so that the program links against a library from before the new entry points
// (tools/newpoints_ab.py: A/B against an earlier build under tools/ab/).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include <sched.h>

#include "orbfe_adaptor.hpp"
#include "jacobi.h"

using namespace ORB_SLAM3;

struct MapPoint3D {
    float x3D[3];
};

struct KeyFrame {
    int N = 0;
    std::shared_ptr<std::vector<KeyPoint>> mvKeysUn;
    std::vector<uint8_t> mDescriptors;
    std::map<unsigned, std::vector<unsigned>> mFeatVec;
    std::vector<std::shared_ptr<MapPoint3D>> mvpMapPoints;
    std::vector<float> mvuRight, mvScaleFactors;
    std::shared_ptr<MapPoint3D> GetMapPoint(size_t i) const { return mvpMapPoints[i]; }
    void AddMapPoint(const std::shared_ptr<MapPoint3D>& mp, size_t i) { mvpMapPoints[i] = mp; }
};

struct Reader {
    std::vector<uint8_t> buf;
    size_t at = 0;
    bool ok = true;
    template <class T>
    void get(T* dst, size_t n)
    {
        if (at + n * sizeof(T) > buf.size()) { ok = false; return; }
        if (n) std::memcpy(dst, buf.data() + at, n * sizeof(T));
        at += n * sizeof(T);
    }
};

static std::shared_ptr<KeyFrame> read_keyframe(Reader& r, int n, const std::vector<float>& sf, std::vector<uint8_t>& has)
{
    auto kf = std::make_shared<KeyFrame>();
    kf->N = n;
    kf->mvKeysUn = std::make_shared<std::vector<KeyPoint>>((size_t)n);
    kf->mDescriptors.resize((size_t)n * 32);
    std::vector<int> node((size_t)n);
    has.resize((size_t)n);
    r.get(kf->mvKeysUn->data(), (size_t)n);
    r.get(kf->mDescriptors.data(), (size_t)n * 32);
    r.get(node.data(), (size_t)n);
    r.get(has.data(), (size_t)n);
    for (int i = 0; i < n; i++)
        if (node[(size_t)i] >= 0) kf->mFeatVec[(unsigned)node[(size_t)i]].push_back((unsigned)i);
    kf->mvuRight.assign((size_t)n, -1.0f);  // monocular (src/Frame.cc:89-90)
    kf->mvScaleFactors = sf;
    kf->mvpMapPoints.resize((size_t)n);
    for (int i = 0; i < n; i++)
        if (has[(size_t)i]) kf->mvpMapPoints[(size_t)i] = std::make_shared<MapPoint3D>();
    return kf;
}

// ---- S11 on the host, Pinhole cameras: src/LocalMapping.cc:571-705 + src/GeometricTools.cc:47-66, the operation order of DESIGN.md ----
using orbfe::sym4_min_eigenvector;   // csrc/jacobi.h: the S10 sequence is the kernels' own text, compiled for the host (-I csrc)

static int host_newpoint(const orbfe_newpoint_params& G, const KeyPoint& k1, const KeyPoint& k2, const float* sf1, const float* sf2, float* x3D)
{
    const float* T1 = G.tcw1;
    const float* T2 = G.tcw2;
    x3D[0] = x3D[1] = x3D[2] = 0.0f;
    const float x1 = (k1.pt.x - G.cam1[2]) / G.cam1[0], y1 = (k1.pt.y - G.cam1[3]) / G.cam1[1];
    const float x2 = (k2.pt.x - G.cam2[2]) / G.cam2[0], y2 = (k2.pt.y - G.cam2[3]) / G.cam2[1];
    float r1[3], r2[3];
    for (int i = 0; i < 3; i++) {
        r1[i] = (T1[i] * x1 + T1[4 + i] * y1) + T1[8 + i];
        r2[i] = (T2[i] * x2 + T2[4 + i] * y2) + T2[8 + i];
    }
    const float dot = (r1[0] * r2[0] + r1[1] * r2[1]) + r1[2] * r2[2];
    const float n1 = std::sqrt((r1[0] * r1[0] + r1[1] * r1[1]) + r1[2] * r1[2]);
    const float n2 = std::sqrt((r2[0] * r2[0] + r2[1] * r2[1]) + r2[2] * r2[2]);
    const float cosParallax = dot / (n1 * n2);
    if (!(cosParallax > 0.0f && (double)cosParallax < (G.inertial ? 0.9996 : 0.9998))) return ORBFE_NEWPT_LOW_PARALLAX;
    float A[4][4];
    for (int j = 0; j < 4; j++) {
        A[0][j] = x1 * T1[8 + j] - T1[j];
        A[1][j] = y1 * T1[8 + j] - T1[4 + j];
        A[2][j] = x2 * T2[8 + j] - T2[j];
        A[3][j] = y2 * T2[8 + j] - T2[4 + j];
    }
    double M[4][4], v[4];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) {
            double acc = 0.0;
            for (int k = 0; k < 4; k++) acc = acc + (double)A[k][i] * (double)A[k][j];
            M[i][j] = acc;
        }
    sym4_min_eigenvector(M, v);
    if (v[3] == 0.0) return ORBFE_NEWPT_AT_INFINITY;
    const float X = (float)(v[0] / v[3]), Y = (float)(v[1] / v[3]), Z = (float)(v[2] / v[3]);
    x3D[0] = X; x3D[1] = Y; x3D[2] = Z;
    const float z1 = ((T1[8] * X + T1[9] * Y) + T1[10] * Z) + T1[11];
    if (!(z1 > 0.0f)) return ORBFE_NEWPT_BEHIND_1;
    const float z2 = ((T2[8] * X + T2[9] * Y) + T2[10] * Z) + T2[11];
    if (!(z2 > 0.0f)) return ORBFE_NEWPT_BEHIND_2;
    const float xc1 = ((T1[0] * X + T1[1] * Y) + T1[2] * Z) + T1[3], yc1 = ((T1[4] * X + T1[5] * Y) + T1[6] * Z) + T1[7];
    const float e1x = (G.cam1[0] * xc1 / z1 + G.cam1[2]) - k1.pt.x, e1y = (G.cam1[1] * yc1 / z1 + G.cam1[3]) - k1.pt.y;
    if ((double)(e1x * e1x + e1y * e1y) > 5.991 * (double)G.level_sigma2_1[k1.octave]) return ORBFE_NEWPT_REPROJECTION_1;
    const float xc2 = ((T2[0] * X + T2[1] * Y) + T2[2] * Z) + T2[3], yc2 = ((T2[4] * X + T2[5] * Y) + T2[6] * Z) + T2[7];
    const float e2x = (G.cam2[0] * xc2 / z2 + G.cam2[2]) - k2.pt.x, e2y = (G.cam2[1] * yc2 / z2 + G.cam2[3]) - k2.pt.y;
    if ((double)(e2x * e2x + e2y * e2y) > 5.991 * (double)G.level_sigma2_2[k2.octave]) return ORBFE_NEWPT_REPROJECTION_2;
    const float a0 = X - G.twc1[0], a1 = Y - G.twc1[1], a2 = Z - G.twc1[2];
    const float b0 = X - G.twc2[0], b1 = Y - G.twc2[1], b2 = Z - G.twc2[2];
    const float dist1 = std::sqrt((a0 * a0 + a1 * a1) + a2 * a2), dist2 = std::sqrt((b0 * b0 + b1 * b1) + b2 * b2);
    if (dist1 == 0.0f || dist2 == 0.0f) return ORBFE_NEWPT_ZERO_DISTANCE;
    if (G.far_points && (dist1 >= G.th_far_points || dist2 >= G.th_far_points)) return ORBFE_NEWPT_FAR;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = sf1[k1.octave] / sf2[k2.octave];
    if (ratioDist * G.ratio_factor < ratioOctave || ratioDist > ratioOctave * G.ratio_factor) return ORBFE_NEWPT_SCALE;
    return ORBFE_NEWPT_ACCEPTED;
}

template <class Fn>
static double median_us(Fn fn, int reps)
{
    for (int i = 0; i < 20; i++) fn();
    std::vector<double> t((size_t)reps);
    for (int i = 0; i < reps; i++) {
        const auto t0 = std::chrono::steady_clock::now();
        fn();
        t[(size_t)i] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    }
    std::sort(t.begin(), t.end());
    return t[t.size() / 2];
}

int main(int argc, char** argv)
{
    if (argc < 3) { std::printf("%s\n", orbfe_version()); return 0; }
    const int reps = argc > 3 ? atoi(argv[3]) : 200;
    Reader r;
    {
        std::ifstream f(argv[1], std::ios::binary);
        r.buf.assign((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    }
    int hdr[3] = {0, 0, 0};  // n1, K, levels
    r.get(hdr, 3);
    const int n1 = hdr[0], K = hdr[1], L = hdr[2];
    if (!r.ok || n1 < 0 || K < 0 || L < 1 || L > ORBFE_MAX_LEVELS) return 2;
    std::vector<float> sf((size_t)L);
    r.get(sf.data(), (size_t)L);
    std::vector<uint8_t> has1;
    auto pKF1 = read_keyframe(r, n1, sf, has1);
    std::vector<std::shared_ptr<KeyFrame>> nbs;
    std::vector<std::vector<uint8_t>> has2((size_t)K);
    std::vector<orbfe_tri_params> tp((size_t)K);
    std::vector<orbfe_newpoint_params> np((size_t)K);
    bool pinhole = true;
    for (int k = 0; k < K; k++) {
        int n2 = 0;
        r.get(&n2, 1);
        if (!r.ok || n2 < 0) return 2;
        nbs.push_back(read_keyframe(r, n2, sf, has2[(size_t)k]));
        r.get(&tp[(size_t)k], 1);
        r.get(&np[(size_t)k], 1);
        pinhole = pinhole && np[(size_t)k].camera_model1 == ORBFE_CAMERA_PINHOLE && np[(size_t)k].camera_model2 == ORBFE_CAMERA_PINHOLE;
    }
    if (!r.ok) return 2;

    orbfe_params p = {1000, 40000, 1.2f, 8, 20, 7, 752, 480, 0, 1};
    orbfe_handle* h = nullptr;
    if (orbfe_create(&p, &h) != ORBFE_OK) { std::puts("orbfe_create failed"); return 3; }
    int created = 0, matched = 0, hostSame = 1;
    double hostUs = 0.0;
    size_t hostPairs = 0;
    {
        auto descOf = [](const std::shared_ptr<KeyFrame>& kf) { return kf->mDescriptors.data(); };
        ResidentKeyFrame r1(h, pKF1, descOf);
        std::vector<std::unique_ptr<ResidentKeyFrame>> own;
        std::vector<const ResidentKeyFrame*> r2;
        for (auto& nb : nbs) {
            own.emplace_back(new ResidentKeyFrame(h, nb, descOf));
            r2.push_back(own.back().get());
        }
#ifndef NEWPOINTS_SEARCH_ONLY
        // ---- the loop (:453-725) ----
        std::ofstream out(argv[2], std::ios::binary);
        NewMapPointsBatch batch(h, pKF1, r1, nbs, r2, tp, np);
        std::vector<NewPoint> pts;
        for (int k = 0; k < K; k++) {
            // (the baseline test :463-482 and CheckNewKeyFrames :455 would go here)
            matched += batch.Points(k, pKF1, pts);
            for (const NewPoint& q : pts) {
                auto pMP = std::make_shared<MapPoint3D>();  // :708
                std::memcpy(pMP->x3D, q.x3D, sizeof q.x3D);
                pKF1->AddMapPoint(pMP, q.idx1);  // :715-716
                nbs[(size_t)k]->AddMapPoint(pMP, q.idx2);
                const int rec[3] = {k, (int)q.idx1, (int)q.idx2};
                out.write(reinterpret_cast<const char*>(rec), sizeof rec);
                out.write(reinterpret_cast<const char*>(q.x3D), sizeof q.x3D);
                created++;
            }
        }
        out.close();

#endif
        // ---- timing on the flags the scene came with ----
        std::vector<const orbfe_keyframe*> kf2((size_t)K);
        std::vector<const uint8_t*> h2p((size_t)K);
        for (int k = 0; k < K; k++) {
            kf2[(size_t)k] = r2[(size_t)k]->get();
            has2[(size_t)k].resize(std::max<size_t>(has2[(size_t)k].size(), 1));
            h2p[(size_t)k] = has2[(size_t)k].data();
        }
        has1.resize(std::max<size_t>(has1.size(), 1));
        const size_t cells = (size_t)std::max(K, 1) * std::max(n1, 1);
        std::vector<int> raw(cells, -1), m12((size_t)std::max(n1, 1));
        std::vector<uint8_t> bin(cells, 0), verdict(cells, 0);
        std::vector<float> x3d(cells * 3, 0.0f);
        int rc = 0;
        double a[3], b[3];
        for (int round = 0; round < 3; round++) {
            a[round] = median_us([&] {
                rc |= orbfe_match_triangulation_batch(h, r1.get(), has1.data(), K, kf2.data(), h2p.data(), tp.data(), raw.data(), bin.data());
            }, reps);
#ifndef NEWPOINTS_SEARCH_ONLY
            b[round] = median_us([&] {
                rc |= orbfe_create_new_points_batch(h, r1.get(), has1.data(), K, kf2.data(), h2p.data(), tp.data(), np.data(), raw.data(),
                                                    bin.data(), x3d.data(), verdict.data());
            }, reps);
#else
            b[round] = 0.0;
#endif
        }
        std::sort(a, a + 3);
        std::sort(b, b + 3);
#ifndef NEWPOINTS_SEARCH_ONLY
        // (c): the replay's matches of the K neighbours, triangulated by one host thread
        std::vector<uint8_t> now(has1);
        struct Pair { int k, i1, i2; };
        std::vector<Pair> work;
        for (int k = 0; k < K; k++) {
            int nm = 0;
            rc |= orbfe_triangulation_select(n1, raw.data() + (size_t)k * n1, bin.data() + (size_t)k * n1, now.data(),
                                             tp[(size_t)k].check_orientation, m12.data(), &nm);
            for (int i = 0; i < n1; i++)
                if (m12[(size_t)i] >= 0) {
                    work.push_back(Pair{k, i, m12[(size_t)i]});
                    if (verdict[(size_t)k * n1 + i] == ORBFE_NEWPT_ACCEPTED) now[(size_t)i] = 1;
                }
        }
        hostPairs = work.size();
        if (pinhole && hostPairs) {
            cpu_set_t one;  // (c) is a single thread on one core: stay on the core we are on
            CPU_ZERO(&one);
            CPU_SET(sched_getcpu(), &one);
            (void)sched_setaffinity(0, sizeof one, &one);
            std::vector<float> hx(hostPairs * 3);
            std::vector<uint8_t> hv(hostPairs);
            auto loop = [&] {
                for (size_t w = 0; w < hostPairs; w++) {
                    const Pair& q = work[w];
                    hv[w] = (uint8_t)host_newpoint(np[(size_t)q.k], (*pKF1->mvKeysUn)[(size_t)q.i1], (*nbs[(size_t)q.k]->mvKeysUn)[(size_t)q.i2],
                                                   sf.data(), sf.data(), &hx[3 * w]);
                }
            };
            hostUs = median_us(loop, std::max(reps / 4, 5));
            for (size_t w = 0; w < hostPairs; w++) {
                const size_t o = (size_t)work[w].k * n1 + work[w].i1;
                if (hv[w] != verdict[o] || std::memcmp(&hx[3 * w], &x3d[3 * o], 12) != 0) hostSame = 0;
            }
        }
#endif
        std::printf("newpoints K=%d n1=%d created=%d matched=%d rc=%d\n", K, n1, created, matched, rc);
        std::printf("newpoints_latency_us search_batch=%.1f create_new_points_batch=%.1f host_pairs=%zu host_loop=%.1f host_us_per_pair=%.4f "
                    "host_same=%d pinhole=%d\n",
                    a[1], b[1], hostPairs, hostUs, hostPairs ? hostUs / (double)hostPairs : 0.0, hostSame, (int)pinhole);
        std::printf("newpoints_rounds_us search_batch=%.1f,%.1f,%.1f create_new_points_batch=%.1f,%.1f,%.1f\n", a[0], a[1], a[2], b[0], b[1],
                    b[2]);
    }
    orbfe_destroy(h);
    return 0;
}
