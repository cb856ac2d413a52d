// point_refresh_check.cpp -- csrc/covis_refresh_check.h without a GPU: what the S26 setters decide on the host before the device is
// touched, and the layout of their staged blocks in two heap buffers of exactly host_bytes() and device_bytes().  Built with
// -fsanitize=address,undefined: a validation that reads past the arrays it was given, or a block that reaches past either size, is a
// failure.  Every array below is a heap vector of exactly the length the call names, so a read beyond it is caught.
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "covis_refresh_check.h"

using namespace orbfe;

namespace {

int failures = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond);      \
            failures++;                                                \
        }                                                              \
    } while (0)

const RefreshDims D{/*kfCap*/ 6, /*kfStride*/ 5, /*obsStride*/ 3, /*cap*/ 9, /*nLevels*/ 8};

std::vector<orbfe_keypoint> keypoints(const std::vector<int>& octaves)
{
    std::vector<orbfe_keypoint> kp(octaves.size(), orbfe_keypoint{});
    for (size_t i = 0; i < octaves.size(); i++) kp[i].octave = octaves[i];
    return kp;
}

void features()
{
    const auto kp = keypoints({0, 7, 3, 1, 2});
    const std::vector<uint8_t> d(5 * 32, 1);
    CHECK(refresh_features_ok(D, 0, 5, kp.data(), d.data(), true));
    CHECK(refresh_features_ok(D, 5, 0, nullptr, nullptr, true));
    CHECK(!refresh_features_ok(D, -1, 5, kp.data(), d.data(), true) && !refresh_features_ok(D, 6, 5, kp.data(), d.data(), true));
    CHECK(!refresh_features_ok(D, 0, 6, kp.data(), d.data(), true));   // refused on n before an element is read
    CHECK(!refresh_features_ok(D, 0, -1, kp.data(), d.data(), true));
    CHECK(!refresh_features_ok(D, 0, 5, nullptr, d.data(), true) && !refresh_features_ok(D, 0, 5, kp.data(), nullptr, true));
    CHECK(!refresh_features_ok(D, 0, 2, keypoints({0, 8}).data(), d.data(), true));
    CHECK(!refresh_features_ok(D, 0, 2, keypoints({-1, 0}).data(), d.data(), true));
    // the device form: the pointers are device addresses and are not read
    CHECK(refresh_features_ok(D, 0, 5, reinterpret_cast<const orbfe_keypoint*>(4096), reinterpret_cast<const uint8_t*>(4096), false));
    CHECK(!refresh_features_ok(D, 0, 6, reinterpret_cast<const orbfe_keypoint*>(4096), reinterpret_cast<const uint8_t*>(4096), false));
}

void centres()
{
    const std::vector<int> slots{0, 5, 2};
    std::vector<float> t(9, 0.5f);
    CHECK(refresh_centres_ok(D, 3, slots.data(), t.data()) && refresh_centres_ok(D, 0, nullptr, nullptr));
    CHECK(!refresh_centres_ok(D, 3, nullptr, t.data()) && !refresh_centres_ok(D, 3, slots.data(), nullptr) && !refresh_centres_ok(D, -1, slots.data(), t.data()));
    CHECK(!refresh_centres_ok(D, 1, std::vector<int>{6}.data(), t.data()) && !refresh_centres_ok(D, 1, std::vector<int>{-1}.data(), t.data()));
    CHECK(!refresh_centres_ok(D, 2, std::vector<int>{3, 3}.data(), t.data()));
    t[8] = std::numeric_limits<float>::quiet_NaN();
    CHECK(!refresh_centres_ok(D, 3, slots.data(), t.data()) && refresh_centres_ok(D, 2, slots.data(), t.data()));
    t[8] = std::numeric_limits<float>::infinity();
    CHECK(!refresh_centres_ok(D, 3, slots.data(), t.data()));
}

void observations()
{
    const std::vector<int> ids{4, 0, 8}, off{0, 2, 2, 5}, slots{0, 5, 1, 2, 3}, idx{-1, 4, 0, 0, 2};
    for (bool indexed : {false, true}) {
        CHECK(refresh_observations_ok(D, 3, ids.data(), off.data(), slots.data(), indexed ? idx.data() : nullptr, indexed));
        CHECK(refresh_observations_ok(D, 0, nullptr, nullptr, nullptr, nullptr, indexed));
        CHECK(!refresh_observations_ok(D, 3, nullptr, off.data(), slots.data(), idx.data(), indexed));
        CHECK(!refresh_observations_ok(D, 3, ids.data(), nullptr, slots.data(), idx.data(), indexed));
        CHECK(!refresh_observations_ok(D, 3, ids.data(), off.data(), nullptr, idx.data(), indexed));
        CHECK(!refresh_observations_ok(D, 1, std::vector<int>{9}.data(), off.data(), slots.data(), idx.data(), indexed));
        CHECK(!refresh_observations_ok(D, 1, std::vector<int>{-1}.data(), off.data(), slots.data(), idx.data(), indexed));
        CHECK(!refresh_observations_ok(D, 2, std::vector<int>{4, 4}.data(), off.data(), slots.data(), idx.data(), indexed));
        CHECK(!refresh_observations_ok(D, 1, ids.data(), std::vector<int>{2, 1}.data(), slots.data(), idx.data(), indexed));   // descending
        CHECK(!refresh_observations_ok(D, 1, ids.data(), std::vector<int>{-1, 1}.data(), slots.data(), idx.data(), indexed));
        CHECK(!refresh_observations_ok(D, 1, ids.data(), std::vector<int>{0, 4}.data(), slots.data(), idx.data(), indexed));   // longer than obs_stride
        CHECK(!refresh_observations_ok(D, 1, ids.data(), std::vector<int>{0, 1}.data(), std::vector<int>{6}.data(), idx.data(), indexed));
    }
    CHECK(!refresh_observations_ok(D, 3, ids.data(), off.data(), slots.data(), nullptr, true));
    CHECK(!refresh_observations_ok(D, 1, ids.data(), std::vector<int>{0, 1}.data(), slots.data(), std::vector<int>{5}.data(), true));
    CHECK(!refresh_observations_ok(D, 1, ids.data(), std::vector<int>{0, 1}.data(), slots.data(), std::vector<int>{-2}.data(), true));
    CHECK(refresh_observations_ok(D, 1, ids.data(), std::vector<int>{0, 1}.data(), slots.data(), std::vector<int>{4}.data(), true));
    // an index out of range is not looked at by the setter without indices
    CHECK(refresh_observations_ok(D, 1, ids.data(), std::vector<int>{0, 1}.data(), slots.data(), nullptr, false));
}

void refs()
{
    const std::vector<int> ids{0, 8, 3}, r{-1, 5, 0};
    CHECK(refresh_refs_ok(D, 3, ids.data(), r.data()) && refresh_refs_ok(D, 0, nullptr, nullptr));
    CHECK(!refresh_refs_ok(D, 3, nullptr, r.data()) && !refresh_refs_ok(D, 3, ids.data(), nullptr) && !refresh_refs_ok(D, -2, ids.data(), r.data()));
    CHECK(!refresh_refs_ok(D, 1, std::vector<int>{9}.data(), r.data()) && !refresh_refs_ok(D, 1, std::vector<int>{-1}.data(), r.data()));
    CHECK(!refresh_refs_ok(D, 1, ids.data(), std::vector<int>{6}.data()) && !refresh_refs_ok(D, 1, ids.data(), std::vector<int>{-2}.data()));
    CHECK(!refresh_refs_ok(D, 2, std::vector<int>{3, 3}.data(), r.data()));
}

// bind a Staging to two heap buffers of exactly its sizes
struct Arena {
    std::vector<uint8_t> host, dev;
    explicit Arena(Staging& st) : host(st.host_bytes()), dev(st.device_bytes()) { st.bind(host.data(), dev.data()); }
    void upload(const Staging& st) { memcpy(dev.data(), host.data(), st.inBytes); }
    void download(const Staging& st) { memcpy(host.data() + st.inBytes, dev.data() + st.oRes, st.resBytes); }
};

void layouts()
{
    for (int n : {0, 1, 5}) {
        Staging st;
        const FeaturesStage B(st, n);
        Arena a(st);
        const auto kp = keypoints(std::vector<int>((size_t)n, 3));
        const std::vector<uint8_t> d((size_t)n * 32, 9);
        B.fill(st, n, kp.data(), d.data());
        a.upload(st);
        CHECK(st.ordered && !st.hasRes && st.inBytes == st.device_bytes());
        for (int i = 0; i < n; i++) CHECK(st.dev(B.kp)[i].octave == 3 && st.dev(B.desc)[(size_t)i * 32 + 31] == 9);
    }
    const std::vector<int> ids{4, 0, 8}, off{0, 2, 2, 5}, slots{0, 5, 1, 2, 3}, idx{-1, 4, 0, 0, 2};
    for (bool indexed : {false, true}) {
        Staging st;
        const ObservationsStage B(st, 3, off.data(), indexed);
        Arena a(st);
        B.fill(st, ids.data(), off.data(), slots.data(), indexed ? idx.data() : nullptr);
        a.upload(st);
        CHECK(st.ordered && B.total == 5 && st.dev(B.off)[3] == 5 && st.dev(B.slots)[4] == 3 && st.dev(B.ids)[2] == 8);
        CHECK(indexed ? (B.idx.n == 5 && st.dev(B.idx)[0] == -1 && st.dev(B.idx)[4] == 2) : B.idx.n == 0);
    }
    {   // every list empty: one element is still taken so that no block is of size zero where a pointer is formed
        const std::vector<int> one{2}, none{0, 0};
        Staging st;
        const ObservationsStage B(st, 1, none.data(), true);
        Arena a(st);
        B.fill(st, one.data(), none.data(), nullptr, nullptr);
        CHECK(B.total == 0 && B.slots.n == 1 && B.idx.n == 1);
    }
    for (int n : {1, 63, 257}) {
        Staging st;
        const RefreshStage B(st, n);
        Arena a(st);
        std::vector<int> ids((size_t)n, 7);
        st.put(B.ids, ids.data());
        a.upload(st);
        for (int i = 0; i < n; i++) {   // the "kernel"
            st.dev(B.status)[i] = 3; st.dev(B.minD)[i] = 0.5f; st.dev(B.maxD)[i] = 2.0f;
            st.dev(B.slot)[i] = i; st.dev(B.index)[i] = -1; st.dev(B.median)[i] = st.dev(B.ids)[i];
        }
        a.download(st);
        std::vector<int> status((size_t)n), median((size_t)n), slot((size_t)n);
        std::vector<float> mx((size_t)n);
        st.get(B.status, status.data()); st.get(B.median, median.data()); st.get(B.slot, slot.data()); st.get(B.maxD, mx.data());
        st.get(B.index, nullptr);   // an output the caller does not want
        CHECK(st.ordered && status[(size_t)n - 1] == 3 && median[0] == 7 && slot[(size_t)n - 1] == n - 1 && mx[0] == 2.0f);
    }
}

}  // namespace

int main()
{
    features();
    centres();
    observations();
    refs();
    layouts();
    printf(failures ? "point_refresh_check: %d FAILURES\n" : "point_refresh_check: ok\n", failures);
    return failures ? 1 : 0;
}
