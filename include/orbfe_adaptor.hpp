// orbfe_adaptor.hpp -- header-only C++17 adaptor that keeps the reference's public signatures on
// top of the C ABI (include/orbfe.h), so src/Frame.cc / src/Tracking.cc call the MI355X front-end
// unchanged.
//
//   ORB_SLAM3::ORBextractor   mirrors include/ORBextractor.h:52-130 (ctor :55-56, extractFeatures
//                             :62, the six getters :64-92)
//   ORB_SLAM3::ORBmatcher     mirrors include/ORBmatcher.h:36-84 for the functions on the hot path
//                             (DescriptorDistance :41, SearchByProjection :45, SearchByBoW :55)
//
// Without OpenCV (this repository's build) the image / descriptor containers are plain views and
// std::vector; define ORBFE_WITH_OPENCV in a tree that has OpenCV-CUDA to get the exact reference
// types (cv::cuda::HostMem in, HostMem N x 32 out).  The matcher wrappers are templates over the
// Frame / KeyFrame / MapPoint types: they only name the members the reference functions read
// (mvKeysUn, mDescriptors, mvpMapPoints, mbTrackInView, ...), so they instantiate against the real
// classes in the reference tree and against light mock types in tests/cpp/test_adaptor.cpp.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "orbfe.h"

#ifdef ORBFE_WITH_OPENCV
#include <opencv2/core/cuda.hpp>
#include <KeyPoint.h>  // the reference's ORB_SLAM3::KeyPoint
#endif

namespace ORB_SLAM3 {

#ifndef ORBFE_WITH_OPENCV
// include/KeyPoint.h:7-12 without cv::Point2f (same 24-byte layout: pt.x, pt.y, response, size, octave, angle)
struct KeyPoint {
    struct { float x, y; } pt;
    int response;
    float size;
    int octave;
    float angle;
};
#endif
static_assert(sizeof(KeyPoint) == sizeof(orbfe_keypoint), "KeyPoint must stay memcpy-compatible with orbfe_keypoint");

namespace orbfe_detail {
inline void check(int rc, const orbfe_handle* h, const char* where)
{
    // The reference aborts the process on device errors (include/cuda/HelperCuda.h:44-50); the adaptor
    // throws instead so the caller can decide.
    if (rc != ORBFE_OK)
        throw std::runtime_error(std::string(where) + ": " + orbfe_status_string(rc) + " " + (h ? orbfe_last_error(h) : ""));
}
}  // namespace orbfe_detail

struct GrayImageView {  // stand-in for cv::cuda::HostMem when OpenCV is absent
    const uint8_t* data;
    int pitch;
};

class ORBextractor {
public:
    // include/ORBextractor.h:55-56
    ORBextractor(int nFeatures, int nFastFeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST,
                 int imageWidth, int imageHeight, int deviceId = 0)
    {
        orbfe_params p{nFeatures, nFastFeatures, scaleFactor, nlevels, iniThFAST, minThFAST, imageWidth, imageHeight, deviceId, 1};
        orbfe_detail::check(orbfe_create(&p, &h_), nullptr, "orbfe_create");
        const int n = nlevels;
        mvScaleFactor.resize(n);
        mvInvScaleFactor.resize(n);
        mvLevelSigma2.resize(n);
        mvInvLevelSigma2.resize(n);
        orbfe_detail::check(orbfe_get_scale_tables(h_, mvScaleFactor.data(), mvInvScaleFactor.data(), mvLevelSigma2.data(),
                                                   mvInvLevelSigma2.data()), h_, "orbfe_get_scale_tables");
        cap_ = orbfe_max_keypoints(h_);
        width_ = imageWidth;
        height_ = imageHeight;
    }
    ~ORBextractor() { orbfe_destroy(h_); }
    ORBextractor(const ORBextractor&) = delete;
    ORBextractor& operator=(const ORBextractor&) = delete;

    // include/ORBextractor.h:62 -- nullopt when no keypoint was found (src/ORBextractor.cc:494-496)
    std::optional<std::tuple<std::shared_ptr<std::vector<KeyPoint>>, std::vector<uint8_t>>> extractFeatures(const GrayImageView& im)
    {
        auto keys = std::make_shared<std::vector<KeyPoint>>(cap_);
        std::vector<uint8_t> desc((size_t)cap_ * ORBFE_DESC_BYTES);
        int n = 0;
        orbfe_detail::check(orbfe_extract(h_, im.data, im.pitch, reinterpret_cast<orbfe_keypoint*>(keys->data()), desc.data(), &n,
                                          nullptr), h_, "orbfe_extract");
        if (n == 0) return std::nullopt;
        keys->resize(n);
        desc.resize((size_t)n * ORBFE_DESC_BYTES);
        return {{keys, std::move(desc)}};
    }

#ifdef ORBFE_WITH_OPENCV
    // the exact reference signature
    std::optional<std::tuple<std::shared_ptr<std::vector<KeyPoint>>, cv::cuda::HostMem>> extractFeatures(const cv::cuda::HostMem& im_managed)
    {
        const cv::Mat im = im_managed.createMatHeader();
        auto r = extractFeatures(GrayImageView{im.data, (int)im.step});
        if (!r) return std::nullopt;
        auto& [keys, desc] = *r;
        cv::cuda::HostMem d((int)keys->size(), 32, CV_8UC1, cv::cuda::HostMem::AllocType::SHARED);
        cv::Mat dm = d.createMatHeader();
        for (int i = 0; i < dm.rows; i++) std::memcpy(dm.ptr(i), desc.data() + (size_t)i * 32, 32);
        return {{keys, d}};
    }
#endif

    // Upstream-style call operator (UZ-SLAMLab ORB_SLAM3: ORBextractor::operator()(image, mask, keypoints, descriptors,
    // vLappingArea)).  This fork has no such member (no referent) -- it is offered for callers
    // written against upstream and forwards to the same C ABI call.  Returns the number of keypoints.  Keypoints stay in
    // LEVEL pixels like everywhere in this fork (SPEC DECISION S6) unless toLevel0 is set, which multiplies pt by
    // mvScaleFactor[octave] as upstream does -- a clearly non-reference convenience.
    int operator()(const GrayImageView& image, std::vector<KeyPoint>& keypoints, std::vector<uint8_t>& descriptors, bool toLevel0 = false)
    {
        auto r = extractFeatures(image);
        keypoints.clear();
        descriptors.clear();
        if (!r) return 0;
        keypoints = *std::get<0>(*r);
        descriptors = std::move(std::get<1>(*r));
        if (toLevel0)
            for (auto& k : keypoints) {
                k.pt.x *= mvScaleFactor[k.octave];
                k.pt.y *= mvScaleFactor[k.octave];
            }
        return (int)keypoints.size();
    }

    // include/ORBextractor.h:64-92
    int GetLevels() { return orbfe_get_levels(h_); }
    float GetScaleFactor() { return orbfe_get_scale_factor(h_); }
    std::vector<float> GetScaleFactors() { return mvScaleFactor; }
    std::vector<float> GetInverseScaleFactors() { return mvInvScaleFactor; }
    std::vector<float> GetScaleSigmaSquares() { return mvLevelSigma2; }
    std::vector<float> GetInverseScaleSigmaSquares() { return mvInvLevelSigma2; }

    // mvImagePyramid / mvBlurredImagePyramid (include/ORBextractor.h:94-95): copy of one level of the last frame
    std::vector<uint8_t> PyramidLevel(int level, bool blurred, int* w = nullptr, int* h = nullptr)
    {
        std::vector<int> lw(GetLevels()), lh(GetLevels());
        orbfe_detail::check(orbfe_get_level_info(h_, nullptr, lw.data(), lh.data()), h_, "orbfe_get_level_info");
        std::vector<uint8_t> out((size_t)lw[level] * lh[level]);
        orbfe_detail::check(orbfe_get_pyramid_level(h_, 0, level, blurred, out.data(), lw[level]), h_, "orbfe_get_pyramid_level");
        if (w) *w = lw[level];
        if (h) *h = lh[level];
        return out;
    }

    orbfe_handle* handle() { return h_; }
    int maxKeypoints() const { return cap_; }

private:
    orbfe_handle* h_ = nullptr;
    int cap_ = 0, width_ = 0, height_ = 0;
    std::vector<float> mvScaleFactor, mvInvScaleFactor, mvLevelSigma2, mvInvLevelSigma2;
};

// The image half of ORB_SLAM3::ImageGrabber (ros2_ws/src/mono-inertial/include/image_grabber.hpp:38-49,96-110): the
// undistortion maps are uploaded once (the node passes two cv::cuda::GpuMat built from
// cv::fisheye::initUndistortRectifyMap, mono_inertial_node.cpp:61-71), ConvertImageToGPU turns a BGR camera frame into
// the grey frame the tracker consumes.  extractFeatures() chains the extractor without the grey frame leaving the device.
class ImagePreparer {
public:
    ImagePreparer(ORBextractor& extractor, int srcWidth, int srcHeight, const float* map1, const float* map2, int width, int height)
        : h_(extractor.handle()), cap_(extractor.maxKeypoints()), w_(width), h2_(height)
    {
        orbfe_detail::check(orbfe_prep_create(h_, srcWidth, srcHeight, map1, map2, width, height, &p_), h_, "orbfe_prep_create");
    }
    ~ImagePreparer() { orbfe_prep_destroy(p_); }
    ImagePreparer(const ImagePreparer&) = delete;
    ImagePreparer& operator=(const ImagePreparer&) = delete;

    // image_grabber.hpp:96-110; grey: height rows of `width` bytes
    std::vector<uint8_t> ConvertImageToGPU(const uint8_t* bgr, int pitch)
    {
        std::vector<uint8_t> grey((size_t)w_ * h2_);
        orbfe_detail::check(orbfe_prepare_image(h_, p_, bgr, pitch, grey.data(), w_), h_, "orbfe_prepare_image");
        return grey;
    }

    // ConvertImageToGPU + ORBextractor::extractFeatures (include/ORBextractor.h:62); `greyOut` (optional) receives the frame
    std::optional<std::tuple<std::shared_ptr<std::vector<KeyPoint>>, std::vector<uint8_t>>> extractFeatures(
        const uint8_t* bgr, int pitch, std::vector<uint8_t>* greyOut = nullptr)
    {
        auto keys = std::make_shared<std::vector<KeyPoint>>(cap_);
        std::vector<uint8_t> desc((size_t)cap_ * ORBFE_DESC_BYTES);
        if (greyOut) greyOut->resize((size_t)w_ * h2_);
        int n = 0;
        orbfe_detail::check(orbfe_prepare_and_extract(h_, p_, bgr, pitch, reinterpret_cast<orbfe_keypoint*>(keys->data()), desc.data(),
                                                      &n, nullptr, greyOut ? greyOut->data() : nullptr, w_), h_,
                            "orbfe_prepare_and_extract");
        if (n == 0) return std::nullopt;
        keys->resize(n);
        desc.resize((size_t)n * ORBFE_DESC_BYTES);
        return {{keys, std::move(desc)}};
    }

#ifdef ORBFE_WITH_OPENCV
    // the reference signature: sensor image in, managed grey HostMem out
    cv::cuda::HostMem ConvertImageToGPU(const cv::Mat& cv_im)
    {
        cv::cuda::HostMem grey(h2_, w_, CV_8UC1, cv::cuda::HostMem::AllocType::SHARED);
        cv::Mat g = grey.createMatHeader();
        orbfe_detail::check(orbfe_prepare_image(h_, p_, cv_im.data, (int)cv_im.step, g.data, (int)g.step), h_, "orbfe_prepare_image");
        return grey;
    }
#endif

private:
    orbfe_handle* h_ = nullptr;
    orbfe_prep* p_ = nullptr;
    int cap_ = 0, w_ = 0, h2_ = 0;
};

// All-static like the reference (include/ORBmatcher.h:40-75); the GPU handle is the extractor's.
class ORBmatcher {
public:
    static constexpr int TH_LOW = ORBFE_TH_LOW;
    static constexpr int TH_HIGH = ORBFE_TH_HIGH;
    static constexpr size_t HISTO_LENGTH = ORBFE_HISTO_LENGTH;

    // src/ORBmatcher.cc:1375-1391 (rows of the descriptor matrices)
    static int DescriptorDistance(const uint8_t* a, const uint8_t* b) { return orbfe_hamming(a, b); }

    // src/ORBmatcher.cc:31-123.  `F` needs: mNumKeypoints, mvKeysUn (shared_ptr<vector<KeyPoint>>), descriptor
    // rows via descPtr(F), mvpMapPoints (vector<shared_ptr<MapPoint>>), mvScaleFactors, the static grid members
    // mnMinX, mnMinY, mfGridElementWidthInv/HeightInv, getFrameGridCols()/Rows().  `MapPoint` needs: mbTrackInView,
    // mTrackDepth, isBad(), mnTrackScaleLevel, mTrackViewCos, mTrackProjX/Y, GetDescriptor-like descPtr(), Observations().
    template <class FramePtr, class MapPointPtr, class DescOfFrame, class DescOfMapPoint>
    static int SearchByProjection(orbfe_handle* h, FramePtr F, const std::vector<MapPointPtr>& vpMapPoints, const float th,
                                  const bool bFarPoints, const float thFarPoints, const float nnRatio,
                                  const bool /*checkOrientation: unused by the reference, :31*/, DescOfFrame frameDesc,
                                  DescOfMapPoint mpDesc)
    {
        const int n = F->mNumKeypoints;
        const int M = (int)vpMapPoints.size();
        std::vector<orbfe_map_point> mps(M);
        std::vector<uint8_t> mpd((size_t)M * 32);
        for (int i = 0; i < M; i++) {
            const auto& p = vpMapPoints[i];
            // mbTrackInViewR only exists for the stereo-fisheye case; mono: inView == mbTrackInView (:40-41,49)
            mps[i] = orbfe_map_point{p->mTrackProjX, p->mTrackProjY, p->mTrackViewCos, p->mTrackDepth, p->mnTrackScaleLevel,
                                     p->mbTrackInView ? 1 : 0, p->isBad() ? 1 : 0, p->Observations()};
            std::memcpy(&mpd[(size_t)i * 32], mpDesc(p), 32);
        }
        std::vector<int> initObs(n, -1);
        for (int i = 0; i < n; i++)
            if (F->mvpMapPoints[i]) initObs[i] = F->mvpMapPoints[i]->Observations();
        orbfe_frame_view fv{n, reinterpret_cast<const orbfe_keypoint*>(F->mvKeysUn->data()), frameDesc(F),
                            F->getFrameGridCols(), F->getFrameGridRows(), F->mnMinX, F->mnMinY, F->mfGridElementWidthInv,
                            F->mfGridElementHeightInv, (int)F->mvScaleFactors.size(), F->mvScaleFactors.data()};
        std::vector<int> match(n > 0 ? n : 1);
        int nmatches = 0;
        orbfe_detail::check(orbfe_match_projection(h, &fv, M, mps.data(), mpd.data(), initObs.data(), th, bFarPoints, thFarPoints,
                                                   nnRatio, match.data(), &nmatches), h, "orbfe_match_projection");
        for (int i = 0; i < n; i++)
            if (match[i] >= 0) F->mvpMapPoints[i] = vpMapPoints[match[i]];  // :113
        return nmatches;
    }

    // src/ORBmatcher.cc:329-439 (include/ORBmatcher.h:58): returns {nmatches, vnMatches12}
    template <class FramePtr, class DescOfFrame>
    static std::pair<int, std::vector<int>> SearchForInitialization(orbfe_handle* h, FramePtr F1, FramePtr F2, int windowSize,
                                                                    const float nnRatio, const bool checkOrientation,
                                                                    DescOfFrame frameDesc)
    {
        auto view = [&](const FramePtr& F) {
            return orbfe_frame_view{(int)F->mvKeysUn->size(), reinterpret_cast<const orbfe_keypoint*>(F->mvKeysUn->data()),
                                    frameDesc(F), F->getFrameGridCols(), F->getFrameGridRows(), F->mnMinX, F->mnMinY,
                                    F->mfGridElementWidthInv, F->mfGridElementHeightInv, (int)F->mvScaleFactors.size(),
                                    F->mvScaleFactors.data()};
        };
        const orbfe_frame_view v1 = view(F1), v2 = view(F2);
        std::vector<int> m12(v1.n > 0 ? v1.n : 1, -1);
        int nmatches = 0;
        orbfe_detail::check(orbfe_match_initialization(h, &v1, &v2, windowSize, nnRatio, checkOrientation, m12.data(), &nmatches),
                            h, "orbfe_match_initialization");
        m12.resize(v1.n);
        return {nmatches, m12};
    }

    // src/ORBmatcher.cc:133-327.  FeatureVector = std::map<NodeId, std::vector<unsigned>> (DBoW2).  The merge-walk
    // over the two maps (:161-163,289-301) happens here on the host and is handed over as CSR groups.
    template <class KeyFramePtr, class FramePtr, class MapPointPtr, class FeatureVector, class DescOfKF, class DescOfFrame>
    static int SearchByBoW(orbfe_handle* h, KeyFramePtr pKF, FramePtr F, std::vector<MapPointPtr>& vpMapPointMatches,
                           const FeatureVector& vFeatVecKF, const FeatureVector& vFeatVecF, const float nnRatio,
                           const bool checkOrientation, DescOfKF kfDesc, DescOfFrame frameDesc)
    {
        const auto vpMapPointsKF = pKF->GetMapPointMatches();
        const int nKF = (int)vpMapPointsKF.size();
        const int nF = F->mNumKeypoints;
        vpMapPointMatches.assign(nF, MapPointPtr());
        std::vector<int> kfOff{0}, kfIdx, fOff{0}, fIdx;
        auto KFit = vFeatVecKF.begin(), KFend = vFeatVecKF.end();
        auto Fit = vFeatVecF.begin(), Fend = vFeatVecF.end();
        while (KFit != KFend && Fit != Fend) {
            if (KFit->first == Fit->first) {
                for (unsigned v : KFit->second) kfIdx.push_back((int)v);
                for (unsigned v : Fit->second) fIdx.push_back((int)v);
                kfOff.push_back((int)kfIdx.size());
                fOff.push_back((int)fIdx.size());
                ++KFit;
                ++Fit;
            } else if (KFit->first < Fit->first) {
                KFit = vFeatVecKF.lower_bound(Fit->first);
            } else {
                Fit = vFeatVecF.lower_bound(KFit->first);
            }
        }
        std::vector<uint8_t> hasMP(nKF > 0 ? nKF : 1, 0);
        std::vector<float> kfAngle(nKF > 0 ? nKF : 1), fAngle(nF > 0 ? nF : 1);
        for (int i = 0; i < nKF; i++) {
            hasMP[i] = vpMapPointsKF[i] && !vpMapPointsKF[i]->isBad();  // :172-176
            kfAngle[i] = (*pKF->mvKeysUn)[i].angle;
        }
        for (int i = 0; i < nF; i++) fAngle[i] = (*F->mvKeysUn)[i].angle;
        std::vector<int> match(nF > 0 ? nF : 1);
        int nmatches = 0;
        // F->Nleft != -1 (two-camera rig): features >= Nleft keep their own best / second best (:205-233,263-286)
        orbfe_detail::check(orbfe_match_bow_rig(h, (int)kfOff.size() - 1, kfOff.data(), kfIdx.data(), fOff.data(), fIdx.data(), nKF,
                                                kfDesc(pKF), kfAngle.data(), hasMP.data(), nF, frameDesc(F), fAngle.data(), F->Nleft,
                                                nnRatio, checkOrientation, match.data(), &nmatches), h, "orbfe_match_bow_rig");
        for (int j = 0; j < nF; j++)
            if (match[j] >= 0) vpMapPointMatches[j] = vpMapPointsKF[match[j]];  // :241
        return nmatches;
    }
};

// ORBmatcher::SearchForTriangulation / ORBmatcher::Fuse (src/ORBmatcher.cc:441-676, 678-851): the data-parallel
// search runs on the GPU, the std::map merge-walk and the map-point graph edits stay on the host.
struct KeyFrameMatcher {
    // src/ORBmatcher.cc:441-676.  `KF` needs: N, mvKeysUn, mFeatVec (std::map<NodeId, vector<unsigned>>), GetMapPoint(i),
    // mvuRight, mvScaleFactors; descriptors through descOf(pKF) (N x 32 bytes).  F12 / ep are computed by the caller
    // with the reference's own expressions (Pinhole.cpp:106-109, ORBmatcher.cc:451-454) and passed in `prm`; for
    // KannalaBrandt8 key frames the caller also fills prm's camera block (T12 of :466-468, both parameter vectors,
    // mvLevelSigma2 of pKF1, whether pKF1->mpCamera2 is set) and the test becomes KannalaBrandt8::epipolarConstrain.
    template <class KeyFramePtr, class DescOf>
    static int SearchForTriangulation(orbfe_handle* h, KeyFramePtr pKF1, KeyFramePtr pKF2, const orbfe_tri_params& prm,
                                      std::vector<std::pair<size_t, size_t>>& vMatchedPairs, DescOf descOf)
    {
        std::vector<int> off1{0}, idx1, off2{0}, idx2;
        auto f1 = pKF1->mFeatVec.begin(), f2 = pKF2->mFeatVec.begin();
        while (f1 != pKF1->mFeatVec.end() && f2 != pKF2->mFeatVec.end()) {  // :489-617
            if (f1->first == f2->first) {
                idx1.insert(idx1.end(), f1->second.begin(), f1->second.end());
                idx2.insert(idx2.end(), f2->second.begin(), f2->second.end());
                off1.push_back((int)idx1.size());
                off2.push_back((int)idx2.size());
                ++f1;
                ++f2;
            } else if (f1->first < f2->first) {
                f1 = pKF1->mFeatVec.lower_bound(f2->first);
            } else {
                f2 = pKF2->mFeatVec.lower_bound(f1->first);
            }
        }
        const int n1 = pKF1->N, n2 = pKF2->N;
        std::vector<uint8_t> has1(n1 > 0 ? n1 : 1), has2(n2 > 0 ? n2 : 1), st1(n1 > 0 ? n1 : 1), st2(n2 > 0 ? n2 : 1);
        for (int i = 0; i < n1; i++) {
            has1[i] = pKF1->GetMapPoint(i) ? 1 : 0;
            st1[i] = pKF1->mvuRight[i] >= 0 ? 1 : 0;
        }
        for (int i = 0; i < n2; i++) {
            has2[i] = pKF2->GetMapPoint(i) ? 1 : 0;
            st2[i] = pKF2->mvuRight[i] >= 0 ? 1 : 0;
        }
        std::vector<int> m12(n1 > 0 ? n1 : 1);
        int nmatches = 0;
        orbfe_detail::check(orbfe_match_triangulation(
            h, (int)off1.size() - 1, off1.data(), idx1.data(), off2.data(), idx2.data(), n1,
            reinterpret_cast<const orbfe_keypoint*>(pKF1->mvKeysUn->data()), descOf(pKF1), has1.data(), st1.data(), n2,
            reinterpret_cast<const orbfe_keypoint*>(pKF2->mvKeysUn->data()), descOf(pKF2), has2.data(), st2.data(),
            pKF2->mvScaleFactors.data(), (int)pKF2->mvScaleFactors.size(), &prm, m12.data(), &nmatches), h,
            "orbfe_match_triangulation");
        vMatchedPairs.clear();
        vMatchedPairs.reserve(nmatches);
        for (int i = 0; i < n1; i++)
            if (m12[i] >= 0) vMatchedPairs.emplace_back((size_t)i, (size_t)m12[i]);  // :664-673
        return nmatches;
    }

    // src/ORBmatcher.cc:678-851.  bRight (the key frame of a two-camera rig, src/LocalMapping.cc:824,854): `frustum`
    // carries GetRightPose / GetRightTranslationInverse / mpCamera2, kfView describes the NLeft left features with
    // desc = all of mDescriptors, and the indices written to the graph are idx + NLeft (:820).
    // The search result of every map point is computed first; the
    // loop below then replays :699-849 in list order with the CURRENT graph state (isBad / IsInKeyFrame may have
    // changed through an earlier Replace), exactly like the reference.  `frustum` carries the key frame's pose and
    // pinhole intrinsics (GetPose / GetTranslationInverse), mbf, mfLogScaleFactor, mnScaleLevels, image bounds.
    template <class KeyFramePtr, class MapPointPtr, class DescOfKF, class DescOfMP>
    static int Fuse(orbfe_handle* h, KeyFramePtr pKF, const std::vector<MapPointPtr>& vpMapPoints, const float th,
                    const orbfe_frustum& frustum, const orbfe_frame_view& kfView, DescOfKF, DescOfMP descOfMP,
                    const bool bRight = false)
    {
        const int M = (int)vpMapPoints.size();
        std::vector<orbfe_world_point> pts(M > 0 ? M : 1);
        std::vector<uint8_t> mpd((size_t)(M > 0 ? M : 1) * 32);
        for (int i = 0; i < M; i++) {
            const auto& pMP = vpMapPoints[i];
            orbfe_world_point& p = pts[i];
            p = orbfe_world_point{0, 0, 0, 0, 0, 0, 0, 1};
            if (!pMP) continue;
            const auto P = pMP->GetWorldPos();
            p = orbfe_world_point{P[0], P[1], P[2], pMP->mfMinDistance, pMP->mfMaxDistance, pMP->isBad() ? 1 : 0,
                                  pMP->Observations(), pMP->IsInKeyFrame(pKF) ? 1 : 0};
            std::memcpy(&mpd[(size_t)i * 32], descOfMP(pMP), 32);
        }
        std::vector<int> bestIdx(M > 0 ? M : 1), bestDist(M > 0 ? M : 1);
        if (bRight)
            orbfe_detail::check(orbfe_fuse_search_right(h, &kfView, pKF->NRight, pKF->mvInvLevelSigma2.data(), pKF->mvuRight.data(),
                                                        &frustum, th, M, pts.data(), mpd.data(), bestIdx.data(), bestDist.data()),
                                h, "orbfe_fuse_search_right");
        else
            orbfe_detail::check(orbfe_fuse_search(h, &kfView, pKF->mvInvLevelSigma2.data(), pKF->mvuRight.data(), &frustum, th, M,
                                                  pts.data(), mpd.data(), bestIdx.data(), bestDist.data()), h, "orbfe_fuse_search");
        int nFused = 0;
        for (int i = 0; i < M; i++) {
            const auto& pMP = vpMapPoints[i];
            if (!pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;  // :701-720, re-evaluated in order
            if (bestDist[i] > ORBFE_TH_LOW) continue;                       // :829
            auto pMPinKF = pKF->GetMapPoint(bestIdx[i]);
            if (pMPinKF) {
                if (!pMPinKF->isBad()) {
                    if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
                    else pMPinKF->Replace(pMP);
                }
            } else {
                pMP->AddObservation(pKF, bestIdx[i]);
                pKF->AddMapPoint(pMP, bestIdx[i]);
            }
            nFused++;
        }
        return nFused;
    }

    // src/ORBmatcher.cc:864-975: Fuse(pKF, Scw, vpPoints, th, vpReplacePoint).  `frustum` carries the decomposition
    // the reference makes at :867-868 (rcw = Scw.rotationMatrix(), tcw = Scw.translation() / Scw.scale(), twc =
    // Tcw.inverse().translation()) plus the key frame's camera, bounds and scale pyramid.  spAlreadyFound is taken
    // once on entry like the reference (:871); the replay loop applies :955-971 in list order on the live graph.
    template <class KeyFramePtr, class MapPointPtr, class DescOfMP>
    static int Fuse(orbfe_handle* h, KeyFramePtr pKF, const orbfe_frustum& frustum, const std::vector<MapPointPtr>& vpPoints,
                    float th, std::vector<MapPointPtr>& vpReplacePoint, const orbfe_frame_view& kfView, DescOfMP descOfMP)
    {
        const int M = (int)vpPoints.size();
        const auto spAlreadyFound = pKF->GetMapPoints();
        std::vector<orbfe_world_point> pts(M > 0 ? M : 1);
        std::vector<uint8_t> mpd((size_t)(M > 0 ? M : 1) * 32);
        for (int i = 0; i < M; i++) {
            const auto& pMP = vpPoints[i];
            const auto P = pMP->GetWorldPos();
            pts[i] = orbfe_world_point{P[0], P[1], P[2], pMP->mfMinDistance, pMP->mfMaxDistance, pMP->isBad() ? 1 : 0,
                                       pMP->Observations(), spAlreadyFound.count(pMP) ? 1 : 0};
            std::memcpy(&mpd[(size_t)i * 32], descOfMP(pMP), 32);
        }
        std::vector<int> bestIdx(M > 0 ? M : 1), bestDist(M > 0 ? M : 1);
        orbfe_detail::check(orbfe_fuse_search_sim3(h, &kfView, &frustum, th, M, pts.data(), mpd.data(), bestIdx.data(),
                                                   bestDist.data()), h, "orbfe_fuse_search_sim3");
        int nFused = 0;
        for (int i = 0; i < M; i++) {
            const auto& pMP = vpPoints[i];
            if (pts[i].bad || pts[i].skip) continue;       // :882 (nothing in this loop changes isBad of a later point)
            if (bestDist[i] > ORBFE_TH_LOW) continue;       // :955
            auto pMPinKF = pKF->GetMapPoint(bestIdx[i]);
            if (pMPinKF) {
                if (!pMPinKF->isBad()) vpReplacePoint[i] = pMPinKF;
            } else {
                pMP->AddObservation(pKF, bestIdx[i]);
                pKF->AddMapPoint(pMP, bestIdx[i]);
            }
            nFused++;
        }
        return nFused;
    }

    // src/ORBmatcher.cc:977-1200.  dir12 / dir21 carry the poses and the similarity (T1w + S21, T2w + S12), pKF1's
    // intrinsics and the target key frame's bounds / pyramid; `KF` needs GetMapPointMatches() and the map points
    // GetIndexInKeyFrame(pKF) (a tuple whose first element is the left index, as in the reference, :1007).
    template <class KeyFramePtr, class MapPointPtr, class DescOfMP>
    static int SearchBySim3(orbfe_handle* h, KeyFramePtr pKF1, KeyFramePtr pKF2, std::vector<MapPointPtr>& vpMatches12,
                            const orbfe_sim3_view& dir12, const orbfe_sim3_view& dir21, const float th,
                            const orbfe_frame_view& view1, const orbfe_frame_view& view2, DescOfMP descOfMP)
    {
        const auto vpMapPoints1 = pKF1->GetMapPointMatches();
        const auto vpMapPoints2 = pKF2->GetMapPointMatches();
        const int N1 = (int)vpMapPoints1.size(), N2 = (int)vpMapPoints2.size();
        std::vector<uint8_t> already1(N1 > 0 ? N1 : 1, 0), already2(N2 > 0 ? N2 : 1, 0);
        for (int i = 0; i < N1; i++) {  // :1001-1012
            const auto& pMP = vpMatches12[i];
            if (!pMP) continue;
            already1[i] = 1;
            const int idx2 = std::get<0>(pMP->GetIndexInKeyFrame(pKF2));
            if (idx2 >= 0 && idx2 < N2) already2[idx2] = 1;
        }
        auto pack = [&](const std::vector<MapPointPtr>& v, const std::vector<uint8_t>& already, std::vector<orbfe_world_point>& pts,
                        std::vector<uint8_t>& d) {
            const int n = (int)v.size();
            pts.assign(n > 0 ? n : 1, orbfe_world_point{0, 0, 0, 0, 0, 0, 0, 1});
            d.assign((size_t)(n > 0 ? n : 1) * 32, 0);
            for (int i = 0; i < n; i++) {
                const auto& pMP = v[i];
                if (!pMP || already[i]) continue;
                const auto P = pMP->GetWorldPos();
                pts[i] = orbfe_world_point{P[0], P[1], P[2], pMP->mfMinDistance, pMP->mfMaxDistance, pMP->isBad() ? 1 : 0,
                                           pMP->Observations(), 0};
                std::memcpy(&d[(size_t)i * 32], descOfMP(pMP), 32);
            }
        };
        std::vector<orbfe_world_point> p1, p2;
        std::vector<uint8_t> d1, d2;
        pack(vpMapPoints1, already1, p1, d1);
        pack(vpMapPoints2, already2, p2, d2);
        std::vector<int> m12(N1 > 0 ? N1 : 1, -1);
        int nFound = 0;
        orbfe_detail::check(orbfe_search_by_sim3(h, &view1, &view2, &dir12, &dir21, p1.data(), d1.data(), p2.data(), d2.data(),
                                                 th, m12.data(), &nFound), h, "orbfe_search_by_sim3");
        for (int i1 = 0; i1 < N1; i1++)
            if (m12[i1] >= 0) vpMatches12[i1] = vpMapPoints2[m12[i1]];  // :1184
        return nFound;
    }

    // src/ORBmatcher.cc:1202-1326: the relocalisation overload SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th,
    // checkOrientation).  `frustum` = the current frame's pose (GetPose / Tcw.inverse().translation()), bounds, camera
    // and pyramid; `frameView` its keypoints, descriptors and grid.
    template <class FramePtr, class KeyFramePtr, class MapPointSet, class DescOfMP>
    static int SearchByProjection(orbfe_handle* h, FramePtr CurrentFrame, KeyFramePtr pKF, const MapPointSet& sAlreadyFound,
                                  const float th, const bool checkOrientation, const orbfe_frustum& frustum,
                                  const orbfe_frame_view& frameView, DescOfMP descOfMP)
    {
        const auto vpMPs = pKF->GetMapPointMatches();
        const int M = (int)vpMPs.size(), n = frameView.n;
        std::vector<orbfe_world_point> pts(M > 0 ? M : 1, orbfe_world_point{0, 0, 0, 0, 0, 0, 0, 1});
        std::vector<uint8_t> mpd((size_t)(M > 0 ? M : 1) * 32);
        std::vector<float> ang(M > 0 ? M : 1);
        for (int i = 0; i < M; i++) {
            ang[i] = (*pKF->mvKeysUn)[i].angle;
            const auto& pMP = vpMPs[i];
            if (!pMP) continue;
            const auto P = pMP->GetWorldPos();
            pts[i] = orbfe_world_point{P[0], P[1], P[2], pMP->mfMinDistance, pMP->mfMaxDistance, pMP->isBad() ? 1 : 0,
                                       pMP->Observations(), sAlreadyFound.count(pMP) ? 1 : 0};
            std::memcpy(&mpd[(size_t)i * 32], descOfMP(pMP), 32);
        }
        std::vector<uint8_t> has(n > 0 ? n : 1);
        for (int i = 0; i < n; i++) has[i] = CurrentFrame->mvpMapPoints[i] ? 1 : 0;
        std::vector<int> match(n > 0 ? n : 1, -1);
        int nmatches = 0;
        orbfe_detail::check(orbfe_match_projection_keyframe(h, &frameView, &frustum, M, pts.data(), mpd.data(), ang.data(),
                                                            has.data(), th, checkOrientation ? 1 : 0, match.data(), &nmatches),
                            h, "orbfe_match_projection_keyframe");
        for (int i = 0; i < n; i++)
            if (match[i] >= 0) CurrentFrame->mvpMapPoints[i] = vpMPs[match[i]];  // :1284 (entries the histogram removed stay as they were: empty)
        return nmatches;
    }
};

// A key frame's immutable matcher inputs resident on the GPU (orbfe_keyframe_*): create it where the reference constructs
// the KeyFrame (after ComputeBoW, src/LocalMapping.cc:258), keep it for the key frame's lifetime.  `KF` needs N, mvKeysUn,
// mFeatVec, mvuRight, mvScaleFactors; descriptors through descOf(pKF).
class ResidentKeyFrame {
public:
    template <class KeyFramePtr, class DescOf>
    ResidentKeyFrame(orbfe_handle* h, KeyFramePtr pKF, DescOf descOf)
    {
        const int n = pKF->N;
        std::vector<int> node(n > 0 ? n : 1, -1);
        for (const auto& e : pKF->mFeatVec)
            for (unsigned i : e.second) node[i] = (int)e.first;  // DBoW2::FeatureVector: node -> features, ascending index
        std::vector<uint8_t> st(n > 0 ? n : 1, 0);
        bool anyStereo = false;
        for (int i = 0; i < n && i < (int)pKF->mvuRight.size(); i++) {
            st[i] = pKF->mvuRight[i] >= 0 ? 1 : 0;
            anyStereo = anyStereo || st[i];
        }
        orbfe_detail::check(orbfe_keyframe_create(h, n, reinterpret_cast<const orbfe_keypoint*>(pKF->mvKeysUn->data()), descOf(pKF),
                                                  node.data(), anyStereo ? st.data() : nullptr, pKF->mvScaleFactors.data(),
                                                  (int)pKF->mvScaleFactors.size(), &kf_), h, "orbfe_keyframe_create");
    }
    ~ResidentKeyFrame() { orbfe_keyframe_destroy(kf_); }
    ResidentKeyFrame(const ResidentKeyFrame&) = delete;
    ResidentKeyFrame& operator=(const ResidentKeyFrame&) = delete;
    const orbfe_keyframe* get() const { return kf_; }

    // mGrid of the key frame (src/KeyFrame.cc:33-80 copies the geometry from the Frame), mvInvLevelSigma2 and mvuRight: what the
    // projection searches INTO this key frame read.  Call it once, right after the constructor; KeyFrameMatcher::FuseResident
    // needs it.  `KF` needs mnGridCols, mnGridRows, mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv.
    template <class KeyFramePtr>
    void SetGrid(orbfe_handle* h, KeyFramePtr pKF)
    {
        orbfe_detail::check(orbfe_keyframe_set_grid(h, kf_, pKF->mnGridCols, pKF->mnGridRows, pKF->mnMinX, pKF->mnMinY,
                                                    pKF->mfGridElementWidthInv, pKF->mfGridElementHeightInv, pKF->mvInvLevelSigma2.data(),
                                                    pKF->mvuRight.empty() ? nullptr : pKF->mvuRight.data()), h, "orbfe_keyframe_set_grid");
    }

private:
    orbfe_keyframe* kf_ = nullptr;
};

// Map points resident on the GPU (orbfe_map_*): what isInFrustum, SearchByProjection and Fuse read from a MapPoint, indexed by
// an id the caller assigns (MapPoint::mnId modulo the capacity, or a slot from a free list).  Update(pMP, id) where the
// reference changes a point: the constructors, SetWorldPos, UpdateNormalAndDepth (mfMin/MaxDistance),
// ComputeDistinctiveDescriptors, SetBadFlag / Replace (src/MapPoint.cc).
class ResidentMap {
public:
    ResidentMap(orbfe_handle* h, int capacity) : h_(h)
    {
        orbfe_detail::check(orbfe_map_create(h, capacity, &m_), h, "orbfe_map_create");
    }
    ~ResidentMap() { orbfe_map_destroy(m_); }
    ResidentMap(const ResidentMap&) = delete;
    ResidentMap& operator=(const ResidentMap&) = delete;
    template <class MapPointPtr, class DescOfMP>
    void Update(const std::vector<MapPointPtr>& vpMPs, const std::vector<int>& ids, DescOfMP descOfMP)
    {
        const int n = (int)vpMPs.size();
        std::vector<orbfe_world_point> pts(n > 0 ? n : 1);
        std::vector<uint8_t> d((size_t)(n > 0 ? n : 1) * 32);
        for (int i = 0; i < n; i++) {
            const auto& pMP = vpMPs[i];
            const auto P = pMP->GetWorldPos();
            pts[i] = orbfe_world_point{P[0], P[1], P[2], pMP->mfMinDistance, pMP->mfMaxDistance, pMP->isBad() ? 1 : 0, pMP->Observations(), 0};
            std::memcpy(&d[(size_t)i * 32], descOfMP(pMP), 32);
        }
        orbfe_detail::check(orbfe_map_update(h_, m_, n, ids.data(), pts.data(), d.data()), h_, "orbfe_map_update");
    }
    const orbfe_map* get() const { return m_; }

private:
    orbfe_handle* h_;
    orbfe_map* m_ = nullptr;
};

// The graph Tracking::UpdateLocalMap walks (src/Tracking.cc:1119-1324), resident in HBM over the ids of a ResidentMap (orbfe_covis,
// SPEC DECISION S24).  A key frame is named by a slot in [0, kfCapacity) and a map point by its id in the map; both come from the
// caller's lookups, as ResidentMap's ids do: slotOf(pKF) -> slot or -1 (not resident), idOf(pMP) -> id or -1.  The lookups are
// called with non-null pointers only.  `KF` needs mnId, isBad(), GetParent(), mPrevKF, GetMapPointMatches(),
// GetBestCovisibilityKeyFrames(N) and GetChilds(); `MP` needs GetObservations() (a map keyed by the key frame).
// When to call: INTEGRATION.md, "UpdateLocalMap on the device" -- at the moment Tracking sees mbMapUpdated, for the key frames and
// points the mapping thread touched since the last frame.
class ResidentCovisibility {
public:
    ResidentCovisibility(orbfe_handle* h, const ResidentMap& map, int kfCapacity, int kfStride, int obsStride, int childStride) : h_(h)
    {
        orbfe_detail::check(orbfe_covis_create(h, map.get(), kfCapacity, kfStride, obsStride, childStride, &g_), h, "orbfe_covis_create");
    }
    ~ResidentCovisibility() { orbfe_covis_destroy(g_); }
    ResidentCovisibility(const ResidentCovisibility&) = delete;
    ResidentCovisibility& operator=(const ResidentCovisibility&) = delete;

    // withFeatures == false leaves the stored feature lists alone (a key frame whose flags or links changed, not its matches).
    // The children are listed in ascending mnId: GetChilds() is ordered by address, which S24 does not follow.
    template <class KFPtr, class SlotOf, class IdOf>
    void UpdateKeyFrames(const std::vector<KFPtr>& vpKFs, SlotOf slotOf, IdOf idOf, bool withFeatures = true)
    {
        const size_t n = vpKFs.size();
        std::vector<orbfe_covis_keyframe> recs(n > 0 ? n : 1);
        std::vector<std::vector<int>> pts(n), cov(n), kids(n);
        for (size_t i = 0; i < n; i++) {
            const auto& pKF = vpKFs[i];
            const auto slot_or_none = [&](const auto& p) { return p ? slotOf(p) : -1; };
            if (withFeatures)
                for (const auto& pMP : pKF->GetMapPointMatches()) pts[i].push_back(pMP ? idOf(pMP) : -1);
            for (const auto& pN : pKF->GetBestCovisibilityKeyFrames(ORBFE_COVIS_MAX_COVISIBLE)) cov[i].push_back(slot_or_none(pN));
            std::vector<std::pair<long long, int>> byId;
            for (const auto& pC : pKF->GetChilds())
                if (pC) byId.emplace_back((long long)pC->mnId, slotOf(pC));
            std::sort(byId.begin(), byId.end());
            for (const auto& c : byId) kids[i].push_back(c.second);
            orbfe_covis_keyframe r{};
            r.struct_size = (int)sizeof r;
            r.slot = slotOf(pKF);
            r.mn_id = (int)pKF->mnId;
            r.bad = pKF->isBad() ? 1 : 0;
            r.parent = slot_or_none(pKF->GetParent());
            r.prev = slot_or_none(pKF->mPrevKF);
            r.n_features = (int)pts[i].size();
            r.n_covisible = (int)cov[i].size();
            r.n_children = (int)kids[i].size();
            static const int none = -1;
            r.point_ids = withFeatures ? (pts[i].empty() ? &none : pts[i].data()) : nullptr;
            r.covisible = cov[i].data();
            r.children = kids[i].data();
            recs[i] = r;
        }
        orbfe_detail::check(orbfe_covis_set_keyframes(h_, g_, (int)n, recs.data()), h_, "orbfe_covis_set_keyframes");
    }

    // GetObservations() of every point of the list; an observing key frame that is not resident is left out
    template <class MPPtr, class IdOf, class SlotOf>
    void UpdateObservations(const std::vector<MPPtr>& vpMPs, IdOf idOf, SlotOf slotOf)
    {
        std::vector<int> ids, off(1, 0), slots;
        for (const auto& pMP : vpMPs) {
            ids.push_back(idOf(pMP));
            for (const auto& ob : pMP->GetObservations()) {
                const int s = ob.first ? slotOf(ob.first) : -1;
                if (s >= 0) slots.push_back(s);
            }
            off.push_back((int)slots.size());
        }
        orbfe_detail::check(orbfe_covis_set_observations(h_, g_, (int)ids.size(), ids.data(), off.data(), slots.data()), h_,
                            "orbfe_covis_set_observations");
    }
    // ---- the graph maintained on the device (SPEC DECISION S25): with these three the mapping thread no longer computes
    // UpdateConnections on its own pointer graph and pushes the result through UpdateKeyFrames / UpdateObservations ----

    // the full mConnectedKeyFrameWeights per key frame, up to connStride pairs; once per graph
    void EnableConnections(int connStride)
    {
        orbfe_detail::check(orbfe_covis_enable_connections(h_, g_, connStride), h_, "orbfe_covis_enable_connections");
        connStride_ = connStride;
    }

    // The graph part of LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:338-361) for the new key frame pKF, which takes `slot`:
    // its record and point list, and the key frame appended to the observation list of each of its points.  -> per feature slot 1: the
    // observation was added (the caller owes pMP->AddObservation, UpdateDepth and ComputeDistinctiveDescriptors on its own objects),
    // 2: the point was in the key frame already (:353-356, mlpRecentAddedMapPoints), 0: no point or a bad one.
    template <class KFPtr, class SlotOf, class IdOf>
    std::vector<int> AddKeyFrame(const KFPtr& pKF, int slot, SlotOf slotOf, IdOf idOf)
    {
        std::vector<int> ids;
        for (const auto& pMP : pKF->GetMapPointMatches()) ids.push_back(pMP ? idOf(pMP) : -1);
        const auto slot_or_none = [&](const auto& p) { return p ? slotOf(p) : -1; };
        orbfe_covis_keyframe r{};
        r.struct_size = (int)sizeof r;
        r.slot = slot;
        r.mn_id = (int)pKF->mnId;
        r.bad = pKF->isBad() ? 1 : 0;
        r.parent = slot_or_none(pKF->GetParent());
        r.prev = slot_or_none(pKF->mPrevKF);
        r.n_features = (int)ids.size();
        r.point_ids = ids.data();
        std::vector<int> added(ids.size() > 0 ? ids.size() : 1, 0);
        int status = 0;
        orbfe_detail::check(orbfe_covis_add_keyframe(h_, g_, &r, added.data(), &status), h_, "orbfe_covis_add_keyframe");
        added.resize(ids.size());
        return added;
    }

    // KeyFrame::UpdateConnections (src/KeyFrame.cc:459-553) of the resident key frame pKF.  firstConnection: mbFirstConnection &&
    // mnId != GetInitKFid() (:545), which the caller knows.  -> mvpOrderedConnectedKeyFrames as slots and mvOrderedWeights, the whole
    // list: what GetBestCovisibilityKeyFrames(nn) of the current key frame returns to CreateNewMapPoints and SearchInNeighbors is its
    // first nn.  false: the key frame shares no point with any other (:493) and nothing was written.
    template <class KFPtr, class SlotOf>
    bool UpdateConnections(const KFPtr& pKF, SlotOf slotOf, bool firstConnection, std::vector<int>& orderedSlots, std::vector<int>& orderedWeights,
                           int minWeight = 50)
    {
        const orbfe_covis_update_params p{(int)sizeof(orbfe_covis_update_params), minWeight};
        orderedSlots.assign((size_t)(connStride_ > 0 ? connStride_ : 1), -1);
        orderedWeights.assign(orderedSlots.size(), 0);
        int count = 0, status = 0;
        orbfe_detail::check(orbfe_covis_update_connections(h_, &p, g_, slotOf(pKF), firstConnection ? 1 : 0, orderedSlots.data(),
                                                           orderedWeights.data(), &count, &status),
                            h_, "orbfe_covis_update_connections");
        orderedSlots.resize((size_t)count);
        orderedWeights.resize((size_t)count);
        return status == ORBFE_COVIS_STATUS_OK;
    }

    // ---- map points refreshed from the graph (SPEC DECISION S26): MapPoint::UpdateDepth and ComputeDistinctiveDescriptors run where the
    // map records live, so min_distance / max_distance and the descriptor every per-frame chain reads no longer wait for a host push.
    // EraseObservation, Replace, SetBadFlag and a changed mpRefKF still reach the graph through the setters below. ----

    // descriptors, octaves and centre per key frame, feature index per observation, mpRefKF per point; scaleFactors = mvScaleFactors
    void EnableRefresh(const std::vector<float>& scaleFactors)
    {
        orbfe_detail::check(orbfe_covis_enable_refresh(h_, g_, (int)scaleFactors.size(), scaleFactors.data()), h_, "orbfe_covis_enable_refresh");
    }

    // mvKeysUn[i].octave and mDescriptors.row(i) of the key frame at `slot`: octaves.size() features, 32 descriptor bytes each
    void SetFeatures(int slot, const std::vector<int>& octaves, const std::vector<uint8_t>& descriptors)
    {
        std::vector<orbfe_keypoint> kp(octaves.size() > 0 ? octaves.size() : 1, orbfe_keypoint{});
        for (size_t i = 0; i < octaves.size(); i++) kp[i].octave = octaves[i];
        if (descriptors.size() != octaves.size() * ORBFE_DESC_BYTES) orbfe_detail::check(ORBFE_ERR_INVALID_ARG, h_, "SetFeatures");
        orbfe_detail::check(orbfe_covis_set_features(h_, g_, slot, (int)octaves.size(), kp.data(), descriptors.data()),
                            h_, "orbfe_covis_set_features");
    }

    // GetTranslationInverse() of the key frames at `slots`, 3 floats each: after every bundle adjustment that moved them
    void SetCentres(const std::vector<int>& slots, const std::vector<float>& twc)
    {
        if (twc.size() != slots.size() * 3) orbfe_detail::check(ORBFE_ERR_INVALID_ARG, h_, "SetCentres");
        orbfe_detail::check(orbfe_covis_set_centres(h_, g_, (int)slots.size(), slots.data(), twc.data()), h_, "orbfe_covis_set_centres");
    }

    // GetObservations() of every point of the list with get<0> of each tuple, the leftIndex; an observing key frame that is not
    // resident is left out.  On a graph with refresh state this replaces UpdateObservations, which writes indices of -1.
    template <class MPPtr, class IdOf, class SlotOf>
    void SetObservations(const std::vector<MPPtr>& vpMPs, IdOf idOf, SlotOf slotOf)
    {
        std::vector<int> ids, off(1, 0), slots, idx;
        for (const auto& pMP : vpMPs) {
            ids.push_back(idOf(pMP));
            for (const auto& ob : pMP->GetObservations()) {
                const int s = ob.first ? slotOf(ob.first) : -1;
                if (s < 0) continue;
                slots.push_back(s);
                idx.push_back(std::get<0>(ob.second));
            }
            off.push_back((int)slots.size());
        }
        orbfe_detail::check(orbfe_covis_set_observations_indexed(h_, g_, (int)ids.size(), ids.data(), off.data(), slots.data(), idx.data()), h_,
                            "orbfe_covis_set_observations_indexed");
    }

    // GetReferenceKeyFrame() of every point of the list; none, or one that is not resident: -1
    template <class MPPtr, class IdOf, class SlotOf>
    void SetReferenceKeyFrames(const std::vector<MPPtr>& vpMPs, IdOf idOf, SlotOf slotOf)
    {
        std::vector<int> ids, refs;
        for (const auto& pMP : vpMPs) {
            ids.push_back(idOf(pMP));
            const auto pRef = pMP->GetReferenceKeyFrame();
            refs.push_back(pRef ? slotOf(pRef) : -1);
        }
        orbfe_detail::check(orbfe_covis_set_ref_keyframes(h_, g_, (int)ids.size(), ids.data(), refs.data()), h_, "orbfe_covis_set_ref_keyframes");
    }

    struct Refreshed {
        std::vector<int> status;                     // bit 0: the distances were written, bit 1: the descriptor
        std::vector<float> minDistance, maxDistance; // mfMinDistance / mfMaxDistance as written
        std::vector<int> bestSlot, bestIndex, bestMedian;
    };
    // UpdateDepth (what & 1) and ComputeDistinctiveDescriptors (what & 2) of the points `ids`, written into the resident map's records;
    // the caller orders it against the chains that read the map as it orders ResidentMap::Update
    Refreshed RefreshPoints(const std::vector<int>& ids, int what = ORBFE_REFRESH_DEPTH | ORBFE_REFRESH_DESCRIPTOR)
    {
        Refreshed r;
        const size_t n = ids.size();
        r.status.assign(n, 0);
        r.minDistance.assign(n, 0.0f);
        r.maxDistance.assign(n, 0.0f);
        r.bestSlot.assign(n, -1);
        r.bestIndex.assign(n, -1);
        r.bestMedian.assign(n, -1);
        if (n == 0) return r;
        orbfe_detail::check(orbfe_covis_refresh_points(h_, g_, (int)n, ids.data(), what, r.status.data(), r.minDistance.data(), r.maxDistance.data(),
                                                       r.bestSlot.data(), r.bestIndex.data(), r.bestMedian.data()),
                            h_, "orbfe_covis_refresh_points");
        return r;
    }

    orbfe_covis* get() const { return g_; }

private:
    orbfe_handle* h_;
    orbfe_covis* g_ = nullptr;
    int connStride_ = 0;
};

// Tracking::UpdateLocalMap (src/Tracking.cc:1119-1324) on the device, one frame from host pointers (orbfe_update_local_map).  What the
// caller still does itself: mpReferenceKF is not chosen here (the reference's own choice is commented out, :1316-1320), and
// SetReferenceMapPoints (:1126) is the viewer's.
class LocalMapUpdater {
public:
    LocalMapUpdater(orbfe_handle* h, ResidentCovisibility& graph, int maxPoints, int maxLocalKFCount = 10, int covisibilityKeyFrameNd = 5,
                    int temporalKeyFrameNd = 10)
        : h_(h), g_(graph), ids_((size_t)(maxPoints > 0 ? maxPoints : 1))
    {
        p_ = orbfe_local_map_params{(int)sizeof(orbfe_local_map_params), maxLocalKFCount, covisibilityKeyFrameNd, temporalKeyFrameNd, 0, 0};
    }

    // vpVoters: the mvpMapPoints of the frame whose matches vote -- mCurrentFrame's before the IMU is initialised (markVotersSeen =
    // true: its own points come back as ~id, "seen in this frame"), mLastFrame's after; bad ones are set to null as the reference does
    // (:1181, :1207).  pLastKF: mCurrentFrame->mpLastKeyFrame or null.  kfOfSlot / mpOfId: the inverses of the lookups.
    // -> mvpLocalKeyFrames, mvpLocalMapPoints; Ids() is the row the per-frame chains take as `ids` (LocalPointCount() of it are set).
    template <class MPPtr, class KFPtr, class IdOf, class SlotOf, class KfOfSlot, class MpOfId>
    void Update(std::vector<MPPtr>& vpVoters, const KFPtr& pLastKF, bool inertial, bool markVotersSeen, IdOf idOf, SlotOf slotOf,
                KfOfSlot kfOfSlot, MpOfId mpOfId, std::vector<KFPtr>& vpLocalKeyFrames, std::vector<MPPtr>& vpLocalMapPoints)
    {
        const int n = (int)vpVoters.size();
        votes_.assign((size_t)(n > 0 ? n : 1), -1);
        for (int i = 0; i < n; i++)
            if (vpVoters[i]) votes_[i] = idOf(vpVoters[i]);
        p_.inertial = inertial ? 1 : 0;
        p_.mark_voters_seen = markVotersSeen ? 1 : 0;
        int kfs[ORBFE_LOCAL_KF_MAX], nKfs = 0;
        votesOut_.resize(votes_.size());
        orbfe_detail::check(orbfe_update_local_map(h_, &p_, n, votes_.data(), pLastKF ? slotOf(pLastKF) : -1, g_.get(), (int)ids_.size(),
                                                   ids_.data(), &nPoints_, kfs, &nKfs, votesOut_.data()),
                            h_, "orbfe_update_local_map");
        for (int i = 0; i < n; i++)
            if (vpVoters[i] && votesOut_[i] < 0) vpVoters[i] = MPPtr();
        vpLocalKeyFrames.clear();
        for (int i = 0; i < nKfs; i++) vpLocalKeyFrames.push_back(kfOfSlot(kfs[i]));
        vpLocalMapPoints.clear();
        const int m = nPoints_ < (int)ids_.size() ? nPoints_ : (int)ids_.size();
        for (int i = 0; i < m; i++) vpLocalMapPoints.push_back(mpOfId(ids_[i] < 0 ? ~ids_[i] : ids_[i]));
    }
    const std::vector<int>& Ids() const { return ids_; }
    int LocalPointCount() const { return nPoints_; }   // the true count: above Ids().size() the row was cut

private:
    orbfe_handle* h_;
    ResidentCovisibility& g_;
    orbfe_local_map_params p_{};
    std::vector<int> ids_, votes_, votesOut_;
    int nPoints_ = 0;
};

// The batched many-frame mode over several GPUs (orbfe_pool_*): member k is an extractor on devices[k] with a ring of
// slots x slotFrames; the frames of a call are sharded in contiguous blocks (orbfe_shard_range) and the members run at the
// same time.  Outputs are frame-major with the stride Cap(): frame i at kp[i*Cap()], desc[i*Cap()*32], n[i],
// perLevel[i*Levels()], match[i*Cap()], nMatches[i]; the vectors are grown to fit.  Every frame of a call shares one pitch.
class FramePool {
public:
    FramePool(const orbfe_params& params, const std::vector<int>& devices, int slots = 3, int slotFrames = 0)
    {
        const int rc = orbfe_pool_create(&params, devices.data(), (int)devices.size(), slots, slotFrames > 0 ? slotFrames : params.max_batch,
                                         &p_);
        check(rc, "orbfe_pool_create");
        cap_ = orbfe_max_keypoints(orbfe_pool_member(p_, 0));
        levels_ = orbfe_get_levels(orbfe_pool_member(p_, 0));
    }
    ~FramePool() { orbfe_pool_destroy(p_); }
    FramePool(const FramePool&) = delete;
    FramePool& operator=(const FramePool&) = delete;

    int Size() const { return orbfe_pool_size(p_); }
    int Cap() const { return cap_; }
    int Levels() const { return levels_; }
    const orbfe_handle* Member(int k) const { return orbfe_pool_member(p_, k); }
    long long MemberFrames(int k) const { return orbfe_pool_member_frames(p_, k); }

    void Extract(const std::vector<GrayImageView>& frames, std::vector<orbfe_keypoint>& kp, std::vector<uint8_t>& desc, std::vector<int>& n,
                 std::vector<int>* perLevel = nullptr)
    {
        const std::vector<const uint8_t*> ptrs = pointers(frames);
        size_outputs(ptrs.size(), kp, desc, n, perLevel);
        check(orbfe_pool_extract(p_, ptrs.data(), frames[0].pitch, (int)ptrs.size(), kp.data(), desc.data(), n.data(),
                                 perLevel ? perLevel->data() : nullptr),
              "orbfe_pool_extract");
    }

    void EnableTrack(int mapCapacity, int maxPoints) { check(orbfe_pool_enable_track(p_, mapCapacity, maxPoints), "orbfe_pool_enable_track"); }
    void MapUpdate(const std::vector<int>& ids, const std::vector<orbfe_world_point>& points, const std::vector<uint8_t>& desc)
    {
        if (points.size() < ids.size() || desc.size() < ids.size() * 32) throw std::invalid_argument("FramePool::MapUpdate: short arrays");
        check(orbfe_pool_map_update(p_, (int)ids.size(), ids.data(), points.data(), desc.data()), "orbfe_pool_map_update");
    }

    // frusta[i]: frame i's pose; ids[i*nPoints ..]: its local map points by id (id >= 0, ~id = skipped, outside the map = none)
    void Track(const std::vector<GrayImageView>& frames, const orbfe_track_params& tp, const std::vector<orbfe_frustum>& frusta, int nPoints,
               const std::vector<int>& ids, std::vector<orbfe_keypoint>& kp, std::vector<uint8_t>& desc, std::vector<int>& n,
               std::vector<int>& match, std::vector<int>& nMatches, std::vector<int>* perLevel = nullptr)
    {
        const std::vector<const uint8_t*> ptrs = pointers(frames);
        const size_t N = ptrs.size();
        if (frusta.size() < N || nPoints < 0 || ids.size() < N * (size_t)nPoints) throw std::invalid_argument("FramePool::Track: short arrays");
        size_outputs(N, kp, desc, n, perLevel);
        if (match.size() < N * cap_) match.resize(N * cap_);
        if (nMatches.size() < N) nMatches.resize(N);
        check(orbfe_pool_track(p_, ptrs.data(), frames[0].pitch, (int)N, &tp, frusta.data(), nPoints, ids.data(), kp.data(), desc.data(),
                               n.data(), perLevel ? perLevel->data() : nullptr, match.data(), nMatches.data()),
              "orbfe_pool_track");
    }

private:
    void check(int rc, const char* where) const
    {
        if (rc != ORBFE_OK)
            throw std::runtime_error(std::string(where) + ": " + orbfe_status_string(rc) + " " + (p_ ? orbfe_pool_last_error(p_) : ""));
    }
    static std::vector<const uint8_t*> pointers(const std::vector<GrayImageView>& frames)
    {
        if (frames.empty()) throw std::invalid_argument("FramePool: no frames");
        std::vector<const uint8_t*> ptrs(frames.size());
        for (size_t i = 0; i < frames.size(); i++) {
            if (frames[i].pitch != frames[0].pitch) throw std::invalid_argument("FramePool: the frames of one call share one pitch");
            ptrs[i] = frames[i].data;
        }
        return ptrs;
    }
    void size_outputs(size_t N, std::vector<orbfe_keypoint>& kp, std::vector<uint8_t>& desc, std::vector<int>& n, std::vector<int>* perLevel) const
    {
        if (kp.size() < N * cap_) kp.resize(N * cap_);
        if (desc.size() < N * cap_ * 32) desc.resize(N * cap_ * 32);
        if (n.size() < N) n.resize(N);
        if (perLevel && perLevel->size() < N * levels_) perLevel->resize(N * levels_);
    }
    orbfe_pool* p_ = nullptr;
    size_t cap_ = 0, levels_ = 0;
};

// ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:678-851) for LocalMapping::SearchInNeighbors
// (src/LocalMapping.cc:764-860, calls at :822,:852) on RESIDENT data: the target key frame is a ResidentKeyFrame with SetGrid
// done, the map points are entries of a ResidentMap (ids[i] = the entry of vpMapPoints[i]); a frustum and 4 bytes per map point
// go up instead of the key frame and 64 bytes per point.  The replay loop is KeyFrameMatcher::Fuse's: :699-849 in list order
// on the live graph.  The caller pushes what the loop changed (Replace: descriptor / observations of the surviving point) to
// the ResidentMap before the next neighbour's call, as it would call ComputeDistinctiveDescriptors in the reference (:836-848).
struct ResidentFuse {
    template <class KeyFramePtr, class MapPointPtr>
    static int Fuse(orbfe_handle* h, KeyFramePtr pKF, const ResidentKeyFrame& resident, const ResidentMap& map,
                    const std::vector<MapPointPtr>& vpMapPoints, const std::vector<int>& ids, const float th,
                    const orbfe_frustum& frustum)
    {
        const int M = (int)vpMapPoints.size();
        std::vector<int> call(M > 0 ? M : 1), bestIdx(M > 0 ? M : 1), bestDist(M > 0 ? M : 1);
        for (int i = 0; i < M; i++) {
            const auto& pMP = vpMapPoints[i];
            // "!pMP || pMP->IsInKeyFrame(pKF)" travels with the id (~id); isBad() is the resident entry's own flag (:706-721)
            call[i] = (!pMP || pMP->IsInKeyFrame(pKF)) ? ~ids[i] : ids[i];
        }
        orbfe_detail::check(orbfe_fuse_search_keyframe(h, resident.get(), map.get(), M, call.data(), &frustum, th, bestIdx.data(),
                                                       bestDist.data()), h, "orbfe_fuse_search_keyframe");
        int nFused = 0;
        for (int i = 0; i < M; i++) {
            const auto& pMP = vpMapPoints[i];
            if (!pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;  // :701-720, re-evaluated in order
            if (bestDist[i] > ORBFE_TH_LOW) continue;                       // :829
            auto pMPinKF = pKF->GetMapPoint(bestIdx[i]);
            if (pMPinKF) {
                if (!pMPinKF->isBad()) {
                    if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
                    else pMPinKF->Replace(pMP);
                }
            } else {
                pMP->AddObservation(pKF, bestIdx[i]);
                pKF->AddMapPoint(pMP, bestIdx[i]);
            }
            nFused++;
        }
        return nFused;
    }
};

// The first loop of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:819-824: ORBmatcher::Fuse(pKFi, vpMapPointMatches) for
// every target key frame) with ONE submission for all targets (orbfe_fuse_search_keyframes).  Construct it before the loop: it
// evaluates "!pMP || pMP->IsInKeyFrame(pKFk)" for every pair, remembers the 32 descriptor bytes every point has NOW and makes
// the one call (candCap gated candidates per pair come back with the results).  Inside the loop, in place of
// ResidentFuse::Fuse(h, pKFk, ...), call Fuse(k, pKFk, vpMapPointMatches, descOfMP): the body of ResidentFuse::Fuse for
// target k on the graph as it is NOW --
//   * a pair that is skipped by now (isBad() / IsInKeyFrame, which only ever turn on during the loop) is skipped;
//   * a point whose descriptor bytes differ from the remembered ones (MapPoint::Replace recomputed them, src/MapPoint.cc:311 --
//     judged from the bytes when target k's turn begins, whichever edit changed them) gets its result for this target from
//     orbfe_fuse_select over its candidate list with the bytes of now;
//   * where that list is truncated (more than candCap candidates) the point is collected, and ONE orbfe_fuse_search_keyframe
//     for the collected points runs before target k is processed, after map.Update of exactly those points;
//   * every other pair takes the row of the one call.
// The result -- nFused, the Replace / AddObservation / AddMapPoint calls and their order -- is that of the K sequential
// ResidentFuse::Fuse calls with the ResidentMap updated between them.  The graph edits stay the caller's types' own; the points'
// positions and distance ranges must not change during the loop (the reference runs UpdateNormalAndDepth after it, :857-870).
// candCap = 4: in the project's K = 20, th = 10 scenes no pair has more than 4 gated candidates (overflow rate 0).
class NeighbourFuseBatch {
public:
    template <class KeyFramePtr, class MapPointPtr, class DescOfKF, class DescOfMP>
    NeighbourFuseBatch(orbfe_handle* h, const std::vector<KeyFramePtr>& vpTargetKFs, const std::vector<const ResidentKeyFrame*>& resident,
                       const std::vector<orbfe_frustum>& frusta, ResidentMap& map, const std::vector<MapPointPtr>& vpMapPointMatches,
                       const std::vector<int>& ids, float th, DescOfKF descOfKF, DescOfMP descOfMP, int candCap = 4)
        : h_(h), map_(&map), frusta_(frusta), ids_(ids), th_(th), K_((int)vpTargetKFs.size()), M_((int)vpMapPointMatches.size()),
          cap_(candCap)
    {
        if ((int)resident.size() != K_ || (int)frusta.size() != K_ || (int)ids.size() != M_ || candCap < 1 || candCap > 16)
            throw std::invalid_argument("NeighbourFuseBatch: one ResidentKeyFrame and frustum per target, one id per map point, candCap in [1, 16]");
        const size_t KM = (size_t)(K_ > 0 ? K_ : 1) * (M_ > 0 ? M_ : 1);
        std::vector<uint8_t> skip(KM, 0);
        desc0_.assign((size_t)(M_ > 0 ? M_ : 1) * 32, 0);
        for (int i = 0; i < M_; i++)
            if (vpMapPointMatches[i]) std::memcpy(&desc0_[(size_t)i * 32], descOfMP(vpMapPointMatches[i]), 32);
        for (int k = 0; k < K_; k++) {
            kf_.push_back(resident[k]->get());
            kfDesc_.push_back(descOfKF(vpTargetKFs[k]));
            kfN_.push_back(vpTargetKFs[k]->N);
            for (int i = 0; i < M_; i++) {
                const auto& pMP = vpMapPointMatches[i];
                skip[(size_t)k * M_ + i] = (!pMP || pMP->IsInKeyFrame(vpTargetKFs[k])) ? 1 : 0;
            }
        }
        bestIdx_.assign(KM, -1);
        bestDist_.assign(KM, 256);
        candIdx_.assign(KM * cap_, -1);
        candCount_.assign(KM, 0);
        orbfe_detail::check(orbfe_fuse_search_keyframes(h, K_, kf_.data(), frusta_.data(), map.get(), M_, ids_.data(), skip.data(), th,
                                                        bestIdx_.data(), bestDist_.data(), cap_, candIdx_.data(), candCount_.data()),
                            h, "orbfe_fuse_search_keyframes");
        submissions_ = 1;
    }

    template <class KeyFramePtr, class MapPointPtr, class DescOfMP>
    int Fuse(int k, KeyFramePtr pKF, const std::vector<MapPointPtr>& vpMapPoints, DescOfMP descOfMP)
    {
        if (k < 0 || k >= K_ || (int)vpMapPoints.size() != M_) throw std::invalid_argument("NeighbourFuseBatch::Fuse: target or list out of range");
        const size_t row = (size_t)k * M_;
        std::vector<int> bestIdx(bestIdx_.begin() + row, bestIdx_.begin() + row + M_), bestDist(bestDist_.begin() + row, bestDist_.begin() + row + M_);
        std::vector<int> over;  // dirty points whose candidate list is truncated
        for (int i = 0; i < M_; i++) {
            const auto& pMP = vpMapPoints[i];
            if (!pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
            const uint8_t* d = descOfMP(pMP);
            if (std::memcmp(d, &desc0_[(size_t)i * 32], 32) == 0) continue;
            hostSelects_++;
            const int rc = orbfe_fuse_select(&candIdx_[(row + i) * cap_], candCount_[row + i], cap_, kfDesc_[k], kfN_[k], d, &bestIdx[i], &bestDist[i]);
            if (rc == ORBFE_ERR_UNSUPPORTED) over.push_back(i);
            else orbfe_detail::check(rc, nullptr, "orbfe_fuse_select");
        }
        if (!over.empty()) {
            std::vector<MapPointPtr> pts;
            std::vector<int> sel;
            for (int i : over) {
                pts.push_back(vpMapPoints[i]);
                sel.push_back(ids_[i]);
            }
            map_->Update(pts, sel, descOfMP);
            std::vector<int> a(over.size()), b(over.size());
            orbfe_detail::check(orbfe_fuse_search_keyframe(h_, kf_[k], map_->get(), (int)sel.size(), sel.data(), &frusta_[k], th_, a.data(), b.data()),
                                h_, "orbfe_fuse_search_keyframe");
            for (size_t j = 0; j < over.size(); j++) {
                bestIdx[over[j]] = a[j];
                bestDist[over[j]] = b[j];
            }
            submissions_++;
            overflows_ += (int)over.size();
        }
        int nFused = 0;
        for (int i = 0; i < M_; i++) {
            const auto& pMP = vpMapPoints[i];
            if (!pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;  // :701-720, re-evaluated in order
            if (bestDist[i] > ORBFE_TH_LOW) continue;                       // :829
            auto pMPinKF = pKF->GetMapPoint(bestIdx[i]);
            if (pMPinKF) {
                if (!pMPinKF->isBad()) {
                    if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
                    else pMPinKF->Replace(pMP);
                }
            } else {
                pMP->AddObservation(pKF, bestIdx[i]);
                pKF->AddMapPoint(pMP, bestIdx[i]);
            }
            nFused++;
        }
        return nFused;
    }

    int Submissions() const { return submissions_; }  // 1 + the targets that needed a fallback search
    int HostSelects() const { return hostSelects_; }  // orbfe_fuse_select calls (dirty pairs)
    int Overflows() const { return overflows_; }      // of those: truncated lists, searched again on the device
    // pairs of the one call whose true candidate count exceeds candCap (the measured overflow rate's numerator)
    size_t PairsAboveCap() const
    {
        size_t n = 0;
        for (int c : candCount_) n += c > cap_;
        return n;
    }

private:
    orbfe_handle* h_;
    ResidentMap* map_;
    std::vector<orbfe_frustum> frusta_;
    std::vector<int> ids_;
    float th_;
    int K_, M_, cap_;
    std::vector<const orbfe_keyframe*> kf_;
    std::vector<const uint8_t*> kfDesc_;
    std::vector<int> kfN_;
    std::vector<uint8_t> desc0_;
    std::vector<int> bestIdx_, bestDist_, candIdx_, candCount_;
    int submissions_ = 0, hostSelects_ = 0, overflows_ = 0;
};

// The SearchForTriangulation loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:455-488) with ONE GPU launch for
// all neighbours.  Construct it before the loop (prm[k] = the F12 / epipole / camera block of the pair (pKF1, neighbour
// k), computed with the reference's own expressions); inside the loop, where the reference calls
// ORBmatcher::SearchForTriangulation(mpCurrentKeyFrame, pKF2, vMatchedIndices, ...), call Matches(k, pKF1, ...): it takes
// the map points pKF1 has NOW (those the loop created for earlier neighbours included, :506-509) and returns exactly what
// the k-th sequential call would return.
class TriangulationBatch {
public:
    template <class KeyFramePtr>
    TriangulationBatch(orbfe_handle* h, KeyFramePtr pKF1, const ResidentKeyFrame& r1, const std::vector<KeyFramePtr>& vpNeighKFs,
                       const std::vector<const ResidentKeyFrame*>& r2, const std::vector<orbfe_tri_params>& prm)
        : n1_(pKF1->N), check_(prm.empty() ? 1 : prm[0].check_orientation)
    {
        const int K = (int)vpNeighKFs.size();
        std::vector<uint8_t> has1(n1_ > 0 ? n1_ : 1);
        for (int i = 0; i < n1_; i++) has1[i] = pKF1->GetMapPoint(i) ? 1 : 0;
        std::vector<std::vector<uint8_t>> has2(K);
        std::vector<const uint8_t*> has2p(K);
        std::vector<const orbfe_keyframe*> kf2(K);
        for (int k = 0; k < K; k++) {
            const int n2 = vpNeighKFs[k]->N;
            has2[k].resize(n2 > 0 ? n2 : 1);
            for (int i = 0; i < n2; i++) has2[k][i] = vpNeighKFs[k]->GetMapPoint(i) ? 1 : 0;
            has2p[k] = has2[k].data();
            kf2[k] = r2[k]->get();
        }
        raw_.assign((size_t)(K > 0 ? K : 1) * (n1_ > 0 ? n1_ : 1), -1);
        bin_.assign(raw_.size(), 0);
        orbfe_detail::check(orbfe_match_triangulation_batch(h, r1.get(), has1.data(), K, kf2.data(), has2p.data(), prm.data(), raw_.data(),
                                                            bin_.data()), h, "orbfe_match_triangulation_batch");
    }

    template <class KeyFramePtr>
    int Matches(int k, KeyFramePtr pKF1, std::vector<std::pair<size_t, size_t>>& vMatchedPairs) const
    {
        std::vector<uint8_t> now(n1_ > 0 ? n1_ : 1);
        for (int i = 0; i < n1_; i++) now[i] = pKF1->GetMapPoint(i) ? 1 : 0;
        std::vector<int> m12(n1_ > 0 ? n1_ : 1);
        int nmatches = 0;
        orbfe_detail::check(orbfe_triangulation_select(n1_, raw_.data() + (size_t)k * n1_, bin_.data() + (size_t)k * n1_, now.data(), check_,
                                                       m12.data(), &nmatches), nullptr, "orbfe_triangulation_select");
        vMatchedPairs.clear();
        vMatchedPairs.reserve(nmatches);
        for (int i = 0; i < n1_; i++)
            if (m12[i] >= 0) vMatchedPairs.emplace_back((size_t)i, (size_t)m12[i]);  // src/ORBmatcher.cc:664-673
        return nmatches;
    }

private:
    int n1_, check_;
    std::vector<int> raw_;
    std::vector<uint8_t> bin_;
};

// The whole neighbour loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:453-725) with ONE submission: the K
// SearchForTriangulation calls (:488) AND "triangulate each match" (:501-705) for every raw partner of every neighbour
// (orbfe_create_new_points_batch, SPEC DECISION S11; monocular key frames).  Construct it before the loop -- prm[k] as for
// TriangulationBatch, geo[k] = the poses, cameras, sigma tables and the three LocalMapping settings of the pair (pKF1,
// neighbour k), see orbfe_newpoint_params -- and inside the loop, in place of :488-705, call Points(k, pKF1, out): the
// (idx1, idx2, x3D) of the map points the reference would create for neighbour k, in the order it creates them (ascending
// idx1), given the map points pKF1 has NOW.  The caller keeps what touches the map: make_shared<MapPoint>(x3D, ...),
// AddObservation / AddMapPoint / ComputeDistinctiveDescriptors / UpdateDepth / AddMapPoint (:708-723) -- pKF1->AddMapPoint
// BEFORE the next Points call, that is what the later neighbours see --, the baseline test (:463-482: skip the Points call
// for that neighbour) and CheckNewKeyFrames() (:455).
struct NewPoint {
    size_t idx1, idx2;
    float x3D[3];
};

class NewMapPointsBatch {
public:
    template <class KeyFramePtr>
    NewMapPointsBatch(orbfe_handle* h, KeyFramePtr pKF1, const ResidentKeyFrame& r1, const std::vector<KeyFramePtr>& vpNeighKFs,
                      const std::vector<const ResidentKeyFrame*>& r2, const std::vector<orbfe_tri_params>& prm,
                      const std::vector<orbfe_newpoint_params>& geo)
        : n1_(pKF1->N), check_(prm.empty() ? 1 : prm[0].check_orientation)
    {
        const int K = (int)vpNeighKFs.size();
        std::vector<uint8_t> has1(n1_ > 0 ? n1_ : 1);
        for (int i = 0; i < n1_; i++) has1[i] = pKF1->GetMapPoint(i) ? 1 : 0;
        std::vector<std::vector<uint8_t>> has2(K);
        std::vector<const uint8_t*> has2p(K);
        std::vector<const orbfe_keyframe*> kf2(K);
        for (int k = 0; k < K; k++) {
            const int n2 = vpNeighKFs[k]->N;
            has2[k].resize(n2 > 0 ? n2 : 1);
            for (int i = 0; i < n2; i++) has2[k][i] = vpNeighKFs[k]->GetMapPoint(i) ? 1 : 0;
            has2p[k] = has2[k].data();
            kf2[k] = r2[k]->get();
        }
        const size_t cells = (size_t)(K > 0 ? K : 1) * (n1_ > 0 ? n1_ : 1);
        raw_.assign(cells, -1);
        bin_.assign(cells, 0);
        verdict_.assign(cells, ORBFE_NEWPT_NO_PARTNER);
        x3d_.assign(cells * 3, 0.0f);
        orbfe_detail::check(orbfe_create_new_points_batch(h, r1.get(), has1.data(), K, kf2.data(), has2p.data(), prm.data(), geo.data(),
                                                          raw_.data(), bin_.data(), x3d_.data(), verdict_.data()), h,
                            "orbfe_create_new_points_batch");
    }

    // the new map points of neighbour k; returns how many matches the k-th SearchForTriangulation call had (nmatches, :502)
    template <class KeyFramePtr>
    int Points(int k, KeyFramePtr pKF1, std::vector<NewPoint>& out) const
    {
        std::vector<uint8_t> now(n1_ > 0 ? n1_ : 1);
        for (int i = 0; i < n1_; i++) now[i] = pKF1->GetMapPoint(i) ? 1 : 0;
        std::vector<int> m12(n1_ > 0 ? n1_ : 1);
        int nmatches = 0;
        const size_t base = (size_t)k * n1_;
        orbfe_detail::check(orbfe_triangulation_select(n1_, raw_.data() + base, bin_.data() + base, now.data(), check_, m12.data(), &nmatches),
                            nullptr, "orbfe_triangulation_select");
        out.clear();
        for (int i = 0; i < n1_; i++) {
            if (m12[i] < 0 || verdict_[base + i] != ORBFE_NEWPT_ACCEPTED) continue;
            const float* x = &x3d_[(base + i) * 3];
            out.push_back(NewPoint{(size_t)i, (size_t)m12[i], {x[0], x[1], x[2]}});
        }
        return nmatches;
    }

    // ORBFE_NEWPT_* of (neighbour k, feature idx1 of key frame 1) -- why a match did not become a point
    int Verdict(int k, size_t idx1) const { return verdict_[(size_t)k * n1_ + idx1]; }

private:
    int n1_, check_;
    std::vector<int> raw_;
    std::vector<uint8_t> bin_, verdict_;
    std::vector<float> x3d_;
};

// The isInFrustum loop of Tracking::SearchLocalPoints (src/Tracking.cc:1059-1077) for all local map points in one
// launch.  `frustum` carries what Frame::isInFrustum reads from the frame (GetRcw / GetTcw / GetTwc, image bounds,
// pinhole intrinsics, mbf, mfLogScaleFactor, mnScaleLevels); `MapPoint` needs GetWorldPos() (indexable [0..2]),
// mfMinDistance / mfMaxDistance (the RAW values: the public getters return them scaled by 0.9 / 1.1), isBad(),
// Observations(), mnLastFrameSeen, and the mTrack* fields the reference writes.  Returns nToMatch.
struct LocalPointProjector {
    template <class MapPointPtr>
    static int ProjectLocalMapPoints(orbfe_handle* h, const orbfe_frustum& frustum, long unsigned int currentFrameId,
                                     const std::vector<MapPointPtr>& vpLocalMapPoints)
    {
        const int n = (int)vpLocalMapPoints.size();
        std::vector<orbfe_world_point> pts(n > 0 ? n : 1);
        for (int i = 0; i < n; i++) {
            const auto& pMP = vpLocalMapPoints[i];
            const auto P = pMP->GetWorldPos();
            pts[i] = orbfe_world_point{P[0], P[1], P[2], pMP->mfMinDistance, pMP->mfMaxDistance, pMP->isBad() ? 1 : 0,
                                       pMP->Observations(), pMP->mnLastFrameSeen == currentFrameId ? 1 : 0};
        }
        std::vector<orbfe_map_point> out(n > 0 ? n : 1);
        std::vector<float> xr(n > 0 ? n : 1);
        orbfe_detail::check(orbfe_project_map_points(h, &frustum, n, pts.data(), out.data(), xr.data()), h,
                            "orbfe_project_map_points");
        int nToMatch = 0;
        for (int i = 0; i < n; i++) {
            if (pts[i].skip || pts[i].bad) continue;  // :1066-1069: untouched
            const auto& pMP = vpLocalMapPoints[i];
            pMP->mbTrackInView = out[i].in_view != 0;  // src/Frame.cc:274-276
            pMP->mTrackProjX = out[i].proj_x;
            pMP->mTrackProjY = out[i].proj_y;
            if (out[i].in_view) {  // :319-328
                pMP->mTrackProjXR = xr[i];
                pMP->mTrackDepth = out[i].track_depth;
                pMP->mnTrackScaleLevel = out[i].level;
                pMP->mTrackViewCos = out[i].view_cos;
                nToMatch++;  // the caller still does pMP->IncreaseVisible() (:1073)
            }
        }
        return nToMatch;
    }
};

// The tracking thread's per-frame chain as ONE submission (orbfe_track_frame): what Tracking::GrabImageMonocular does with
// a frame once the IMU is initialised -- Frame::Frame -> ExtractORB (src/Tracking.cc:152-173, src/Frame.cc:178-189), then
// Track() -> TrackWithMotionModel (IMU prediction only, :908-923) -> TrackLocalMap -> SearchLocalPoints: the isInFrustum
// loop (:1059-1077) and ORBmatcher::SearchByProjection(mCurrentFrame, mvpLocalMapPoints, th, false, thFarPoints, nnRatio)
// (:1108-1115).  The caller builds `frustum` from the PREDICTED pose (it does not depend on the frame's features) and
// passes the local map of UpdateLocalMap (:930).  On return `F` carries the fresh keypoints and descriptors and the
// matches in mvpMapPoints, the map points carry their mTrack* fields (LocalPointProjector's contract), *nToMatch is the
// reference's counter.  `F` needs: mNumKeypoints, mvKeysUn, mvpMapPoints, the grid statics (as SearchByProjection above);
// the descriptor rows go to the frame through setDesc(F, rows, n) (cv::cuda::HostMem in the reference, a vector here).
// Returns the match count, or -1 when the frame has no keypoints (the reference returns before Track(), :158-159).
struct FrameTracker {
    template <class FramePtr, class MapPointPtr, class DescOfMapPoint, class SetFrameDesc>
    static int ExtractAndSearchLocalPoints(ORBextractor& extractor, const GrayImageView& im, FramePtr F, const orbfe_frustum& frustum,
                                           long unsigned int currentFrameId, const std::vector<MapPointPtr>& vpLocalMapPoints,
                                           const float th, const bool bFarPoints, const float thFarPoints, const float nnRatio,
                                           DescOfMapPoint mpDesc, SetFrameDesc setDesc, int* nToMatch = nullptr)
    {
        orbfe_handle* h = extractor.handle();
        const int cap = extractor.maxKeypoints();
        const int M = (int)vpLocalMapPoints.size();
        std::vector<orbfe_world_point> pts(M > 0 ? M : 1);
        std::vector<uint8_t> mpd((size_t)(M > 0 ? M : 1) * 32);
        for (int i = 0; i < M; i++) {
            const auto& pMP = vpLocalMapPoints[i];
            const auto P = pMP->GetWorldPos();
            pts[i] = orbfe_world_point{P[0], P[1], P[2], pMP->mfMinDistance, pMP->mfMaxDistance, pMP->isBad() ? 1 : 0,
                                       pMP->Observations(), pMP->mnLastFrameSeen == currentFrameId ? 1 : 0};
            std::memcpy(&mpd[(size_t)i * 32], mpDesc(pMP), 32);
        }
        orbfe_track_params tp = ORBFE_TRACK_PARAMS_INIT;
        tp.grid_cols = F->getFrameGridCols();
        tp.grid_rows = F->getFrameGridRows();
        tp.min_x = F->mnMinX;
        tp.min_y = F->mnMinY;
        tp.grid_inv_w = F->mfGridElementWidthInv;
        tp.grid_inv_h = F->mfGridElementHeightInv;
        tp.th = th;
        tp.nn_ratio = nnRatio;
        tp.far_points = bFarPoints ? 1 : 0;
        tp.th_far_points = thFarPoints;
        auto keys = std::make_shared<std::vector<KeyPoint>>(cap);
        std::vector<uint8_t> desc((size_t)cap * ORBFE_DESC_BYTES);
        std::vector<int> match(cap);
        std::vector<orbfe_map_point> out(M > 0 ? M : 1);
        std::vector<float> xr(M > 0 ? M : 1);
        int n = 0, nmatches = 0;
        orbfe_detail::check(orbfe_track_frame(h, im.data, im.pitch, &frustum, &tp, M, pts.data(), mpd.data(),
                                              reinterpret_cast<orbfe_keypoint*>(keys->data()), desc.data(), &n, nullptr, out.data(),
                                              xr.data(), match.data(), &nmatches), h, "orbfe_track_frame");
        keys->resize(n);
        F->mNumKeypoints = n;
        F->mvKeysUn = keys;
        setDesc(F, desc.data(), n);
        F->mvpMapPoints.assign(n, nullptr);
        int toMatch = 0;
        for (int i = 0; i < M; i++) {  // what isInFrustum leaves in the map points (src/Frame.cc:274-276,319-328)
            if (pts[i].skip || pts[i].bad) continue;
            const auto& pMP = vpLocalMapPoints[i];
            pMP->mbTrackInView = out[i].in_view != 0;
            pMP->mTrackProjX = out[i].proj_x;
            pMP->mTrackProjY = out[i].proj_y;
            if (out[i].in_view) {
                pMP->mTrackProjXR = xr[i];
                pMP->mTrackDepth = out[i].track_depth;
                pMP->mnTrackScaleLevel = out[i].level;
                pMP->mTrackViewCos = out[i].view_cos;
                toMatch++;
            }
        }
        if (nToMatch) *nToMatch = toMatch;
        if (n == 0) return -1;
        for (int i = 0; i < n; i++)
            if (match[i] >= 0) F->mvpMapPoints[i] = vpLocalMapPoints[match[i]];  // src/ORBmatcher.cc:113
        return nmatches;
    }
};

// ORB_SLAM3::ORBVocabulary = DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> (include/ORBVocabulary.h:29-30), the
// part Frame::ComputeBoW / KeyFrame::ComputeBoW use (src/Frame.cc:483-495): load the text vocabulary, transform a
// frame's descriptors into BowVector + FeatureVector.  The tree descent of every feature runs on the GPU
// (orbfe_bow_transform); the <= N map inserts and the normalisation stay on the host, in the reference's order, so
// the doubles are bit-identical.  `BowVector` is any std::map<unsigned, double>-shaped type (DBoW2::BowVector),
// `FeatureVector` any std::map<unsigned, std::vector<unsigned>>-shaped type (DBoW2::FeatureVector).
class ORBVocabulary {
public:
    enum WeightingType { TF_IDF, TF, IDF, BINARY };                                        // BowVector.h:26-32
    enum ScoringType { L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT };     // BowVector.h:35-43

    explicit ORBVocabulary(orbfe_handle* h) : h_(h) {}
    ORBVocabulary(const ORBVocabulary&) = delete;
    ORBVocabulary& operator=(const ORBVocabulary&) = delete;
    ~ORBVocabulary() { orbfe_vocab_destroy(v_); }

    // TemplatedVocabulary::loadFromTextFile (TemplatedVocabulary.h:1349-1436); blank lines are skipped.
    bool loadFromTextFile(const std::string& filename)
    {
        FILE* f = fopen(filename.c_str(), "r");
        if (!f) return false;
        int n1 = 0, n2 = 0;
        if (fscanf(f, "%d %d %d %d", &k_, &L_, &n1, &n2) != 4 || k_ < 0 || k_ > 20 || L_ < 1 || L_ > 10 || n1 < 0 || n1 > 5 ||
            n2 < 0 || n2 > 3) {
            fclose(f);
            return false;
        }
        scoring_ = (ScoringType)n1;
        weighting_ = (WeightingType)n2;
        std::vector<int> parent{0}, leaf{0};
        std::vector<uint8_t> desc(32, 0);
        std::vector<double> weight{0.0};
        for (;;) {
            int pid, isLeaf;
            if (fscanf(f, "%d %d", &pid, &isLeaf) != 2) break;
            uint8_t d[32];
            bool ok = true;
            for (int i = 0; i < 32; i++) {
                int v;
                ok = ok && fscanf(f, "%d", &v) == 1;
                d[i] = (uint8_t)v;
            }
            double w;
            if (!ok || fscanf(f, "%lf", &w) != 1 || pid < 0 || pid >= (int)parent.size()) {
                fclose(f);
                return false;
            }
            parent.push_back(pid);
            leaf.push_back(isLeaf);
            desc.insert(desc.end(), d, d + 32);
            weight.push_back(w);
        }
        fclose(f);
        const int n = (int)parent.size();
        std::vector<int> childOff(n + 1, 0), childIdx(n > 1 ? n - 1 : 1), wordId(n, 0);
        for (int i = 1; i < n; i++) childOff[parent[i] + 1]++;
        for (int i = 0; i < n; i++) childOff[i + 1] += childOff[i];
        std::vector<int> fill(childOff.begin(), childOff.end() - 1);
        for (int i = 1; i < n; i++) childIdx[fill[parent[i]]++] = i;  // ascending id == push_back order (:1403)
        nWords_ = 0;
        for (int i = 1; i < n; i++)
            if (leaf[i] > 0) wordId[i] = nWords_++;  // :1419-1426
        return create(n, childOff.data(), childIdx.data(), desc.data(), wordId.data(), weight.data(), L_);
    }

    // direct construction from DBoW2's node table (for callers that already hold one)
    bool create(int nNodes, const int* childOff, const int* childIdx, const uint8_t* nodeDesc, const int* wordId,
                const double* weight, int L)
    {
        orbfe_vocab_destroy(v_);
        v_ = nullptr;
        L_ = L;
        return orbfe_vocab_create(h_, nNodes, childOff, childIdx, nodeDesc, wordId, weight, L, &v_) == ORBFE_OK;
    }

    bool empty() const { return v_ == nullptr; }
    unsigned size() const { return (unsigned)nWords_; }
    int getBranchingFactor() const { return k_; }
    int getDepthLevels() const { return L_; }
    void setScoringType(ScoringType t) { scoring_ = t; }
    void setWeightingType(WeightingType t) { weighting_ = t; }

    // TemplatedVocabulary::transform(features, v, fv, levelsup) (TemplatedVocabulary.h:1136-1204); `desc` is the
    // frame's N x 32 descriptor matrix (what Converter::toDescriptorVector splits into rows, src/Frame.cc:487).
    template <class BowVector, class FeatureVector>
    void transform(const uint8_t* desc, int n, BowVector& v, FeatureVector& fv, int levelsup) const
    {
        v.clear();
        fv.clear();
        if (empty() || n <= 0) return;
        std::vector<int> word(n), node(n);
        std::vector<double> w(n);
        orbfe_detail::check(orbfe_bow_transform(h_, v_, desc, n, levelsup, word.data(), node.data(), w.data()), h_,
                            "orbfe_bow_transform");
        assemble(word.data(), node.data(), w.data(), n, v, fv);
    }

    // the host half of transform(): BowVector / FeatureVector from the per-feature (word, node, weight) triples, in the
    // reference's insertion order (TemplatedVocabulary.h:1157-1204), so the doubles are bit-identical
    template <class BowVector, class FeatureVector>
    void assemble(const int* word, const int* node, const double* w, int n, BowVector& v, FeatureVector& fv) const
    {
        v.clear();
        fv.clear();
        const bool must = scoring_ != DOT_PRODUCT;  // ScoringObject.h:74-89
        const bool tf = weighting_ == TF || weighting_ == TF_IDF;
        for (int i = 0; i < n; i++) {
            if (!(w[i] > 0)) continue;  // stopped word
            auto it = v.lower_bound(word[i]);
            if (it != v.end() && !(v.key_comp()(word[i], it->first))) {
                if (tf) it->second += w[i];  // BowVector::addWeight; addIfNotExist leaves it
            } else {
                v.insert(it, typename BowVector::value_type(word[i], w[i]));
            }
            fv[node[i]].push_back(i);  // FeatureVector::addFeature
        }
        if (tf && !v.empty() && !must) {
            const double nd = (double)v.size();
            for (auto& e : v) e.second /= nd;
        }
        if (must) {  // BowVector::normalize, src/DBoW2/BowVector.cpp:62-84
            double norm = 0.0;
            if (scoring_ == L2_NORM) {
                for (auto& e : v) norm += e.second * e.second;
                norm = std::sqrt(norm);
            } else {
                for (auto& e : v) norm += std::fabs(e.second);
            }
            if (norm > 0.0)
                for (auto& e : v) e.second /= norm;
        }
    }

    const orbfe_vocab* get() const { return v_; }

private:
    orbfe_handle* h_;
    orbfe_vocab* v_ = nullptr;
    int k_ = 0, L_ = 0, nWords_ = 0;
    ScoringType scoring_ = L1_NORM;
    WeightingType weighting_ = TF_IDF;
};

// The tracking thread's chain of a frame tracked against its reference key frame, as ONE submission
// (orbfe_track_reference_keyframe): what Tracking::GrabImageMonocular + Tracking::TrackReferenceKeyFrame do up to the pose
// solver -- Frame::Frame -> ExtractORB (src/Frame.cc:178-189), mCurrentFrame->ComputeBoW() (src/Tracking.cc:829,
// src/Frame.cc:483-495), ORBmatcher::SearchByBoW(mpReferenceKF, mCurrentFrame, vpMapPointMatches, nnRatio, true) (:835).
// `resident` is the reference key frame's ResidentKeyFrame (made when the key frame was created); its map points are read
// as they stand now.  On return `F` carries the fresh keypoints, descriptors (through setDesc(F, rows, n)), mBowVec and
// mFeatVec; vpMapPointMatches is what SearchByBoW would have filled.  Returns the match count, or -1 when the frame has no
// keypoints (the reference returns before Track(), src/Tracking.cc:158-159).
struct ReferenceKeyFrameTracker {
    template <class FramePtr, class KeyFramePtr, class MapPointPtr, class SetFrameDesc>
    static int ExtractAndSearchByBoW(ORBextractor& extractor, const GrayImageView& im, FramePtr F, const ORBVocabulary& voc,
                                     KeyFramePtr pKF, const ResidentKeyFrame& resident, std::vector<MapPointPtr>& vpMapPointMatches,
                                     const float nnRatio, const bool checkOrientation, SetFrameDesc setDesc, const int levelsup = 4)
    {
        orbfe_handle* h = extractor.handle();
        const int cap = extractor.maxKeypoints();
        const auto vpMapPointsKF = pKF->GetMapPointMatches();
        const int nKF = (int)vpMapPointsKF.size();
        std::vector<uint8_t> hasMP(nKF > 0 ? nKF : 1, 0);
        for (int i = 0; i < nKF; i++) hasMP[i] = vpMapPointsKF[i] && !vpMapPointsKF[i]->isBad();  // src/ORBmatcher.cc:182-187
        auto keys = std::make_shared<std::vector<KeyPoint>>(cap);
        std::vector<uint8_t> desc((size_t)cap * ORBFE_DESC_BYTES);
        std::vector<int> word(cap), node(cap), match(cap);
        std::vector<double> w(cap);
        int n = 0, nmatches = 0;
        orbfe_detail::check(orbfe_track_reference_keyframe(h, im.data, im.pitch, voc.get(), levelsup, resident.get(), hasMP.data(), nnRatio,
                                                           checkOrientation ? 1 : 0, reinterpret_cast<orbfe_keypoint*>(keys->data()),
                                                           desc.data(), &n, nullptr, word.data(), node.data(), w.data(), match.data(),
                                                           &nmatches), h, "orbfe_track_reference_keyframe");
        keys->resize(n);
        F->mNumKeypoints = n;
        F->mvKeysUn = keys;
        setDesc(F, desc.data(), n);
        voc.assemble(word.data(), node.data(), w.data(), n, F->mBowVec, F->mFeatVec);
        vpMapPointMatches.assign(n, MapPointPtr());
        if (n == 0) return -1;
        for (int i = 0; i < n; i++)
            if (match[i] >= 0) vpMapPointMatches[i] = vpMapPointsKF[match[i]];  // src/ORBmatcher.cc:241
        return nmatches;
    }
};

// The tracking thread's chain of a frame while the map is being initialised, as ONE submission (orbfe_track_initialization):
// what Tracking::GrabImageMonocular + Tracking::MonocularInitialization do up to ReconstructWithTwoViews -- Frame::Frame ->
// ExtractORB (src/Frame.cc:178-189), ORBmatcher::SearchForInitialization(mInitialFrame, mCurrentFrame, 40, 0.45, true)
// (src/Tracking.cc:603-607).  Seed(F) where the reference sets mInitialFrame = mCurrentFrame (:569-586) -- the frame's
// keypoints and descriptors go to the GPU once; ExtractAndSearch(...) for every following frame; Reset() where the reference
// clears mbReadyToInitializate (:588-602).  The thresholds around the calls (FEAT_INIT_COUNT, the 2 s time-out) stay in
// Tracking.cc.
class InitializationTracker {
public:
    explicit InitializationTracker(ORBextractor& extractor) : ex_(extractor) {}
    ~InitializationTracker() { orbfe_init_frame_destroy(f1_); }
    InitializationTracker(const InitializationTracker&) = delete;
    InitializationTracker& operator=(const InitializationTracker&) = delete;
    bool Ready() const { return f1_ != nullptr; }
    void Reset()
    {
        orbfe_init_frame_destroy(f1_);
        f1_ = nullptr;
    }
    template <class FramePtr, class DescOf>
    void Seed(FramePtr F, DescOf descOf)
    {
        Reset();
        orbfe_detail::check(orbfe_init_frame_create(ex_.handle(), (int)F->mvKeysUn->size(),
                                                    reinterpret_cast<const orbfe_keypoint*>(F->mvKeysUn->data()), descOf(F), &f1_),
                            ex_.handle(), "orbfe_init_frame_create");
    }
    // -> {nmatches, vnMatches12} as SearchForInitialization; F receives the fresh keypoints and descriptors (setDesc(F, rows, n));
    // nmatches == -1 when the frame has no keypoints (the reference returns before Track(), src/Tracking.cc:158-159)
    template <class FramePtr, class SetFrameDesc>
    std::pair<int, std::vector<int>> ExtractAndSearch(const GrayImageView& im, FramePtr F, SetFrameDesc setDesc, int windowSize = 40,
                                                      float nnRatio = 0.45f, bool checkOrientation = true)
    {
        orbfe_handle* h = ex_.handle();
        const int cap = ex_.maxKeypoints(), n1 = orbfe_init_frame_size(f1_);
        auto keys = std::make_shared<std::vector<KeyPoint>>(cap);
        std::vector<uint8_t> desc((size_t)cap * ORBFE_DESC_BYTES);
        std::vector<int> m12(n1 > 0 ? n1 : 1, -1);
        orbfe_track_params tp = ORBFE_TRACK_PARAMS_INIT;
        tp.grid_cols = F->getFrameGridCols(); tp.grid_rows = F->getFrameGridRows();
        tp.min_x = F->mnMinX; tp.min_y = F->mnMinY;
        tp.grid_inv_w = F->mfGridElementWidthInv; tp.grid_inv_h = F->mfGridElementHeightInv;
        int n = 0, nmatches = 0;
        orbfe_detail::check(orbfe_track_initialization(h, im.data, im.pitch, f1_, &tp, windowSize, nnRatio, checkOrientation ? 1 : 0,
                                                       reinterpret_cast<orbfe_keypoint*>(keys->data()), desc.data(), &n, nullptr, m12.data(),
                                                       &nmatches), h, "orbfe_track_initialization");
        keys->resize(n);
        F->mNumKeypoints = n;
        F->mvKeysUn = keys;
        setDesc(F, desc.data(), n);
        m12.resize(n1);
        return {n == 0 ? -1 : nmatches, std::move(m12)};
    }

private:
    ORBextractor& ex_;
    orbfe_init_frame* f1_ = nullptr;
};

// TwoViewReconstruction (include/TwoViewReconstruction.h, src/TwoViewReconstruction.cc:31-127) for a pinhole K as ONE call
// (orbfe_two_view_reconstruct): the line behind SearchForInitialization in Tracking::MonocularInitialization
// (src/Tracking.cc:616 -> Pinhole::ReconstructWithTwoViews, src/CameraModels/Pinhole.cpp:81-88).  The RANSAC sets are drawn
// here exactly as :64-94 draws them -- srand(0) once per process (DUtils::Random::SeedRandOnce(0)), then the RandomInt formula
// of Thirdparty/DBoW2/src/DUtils/Random.cpp:47-50 on the process's rand() stream -- so a process that replaces the reference's
// class by this one sees the same sets.  std::array / std::vector stand in for Sophus::SE3f / cv::Point3f.
class TwoViewReconstruction {
public:
    TwoViewReconstruction(ORBextractor& extractor, float fx, float fy, float cx, float cy, float sigma = 1.0f, int iterations = 200)
        : ex_(extractor)
    {
        p_ = ORBFE_TWO_VIEW_PARAMS_INIT;
        p_.fx = fx; p_.fy = fy; p_.cx = cx; p_.cy = cy;
        p_.sigma = sigma;
        p_.iterations = iterations;
    }
    // mvSets for N matches (:64-94)
    std::vector<int> DrawSets(int N) const { return DrawSets(N, p_.iterations); }
    // the same draw without an object (and so without a GPU): what DrawSets(N) of a solver with `iterations` returns
    static std::vector<int> DrawSets(int N, int iterations)
    {
        static const bool seeded = (srand(0), true);  // DUtils::Random::SeedRandOnce(0)
        (void)seeded;
        std::vector<int> sets((size_t)iterations * 8, 0);
        std::vector<int> all((size_t)N), avail;
        for (int i = 0; i < N; i++) all[(size_t)i] = i;
        for (int it = 0; it < iterations; it++) {
            avail = all;
            for (int j = 0; j < 8; j++) {
                const int d = (int)avail.size();
                const int randi = int(((double)rand() / ((double)RAND_MAX + 1.0)) * d);
                sets[(size_t)it * 8 + j] = avail[(size_t)randi];
                avail[(size_t)randi] = avail.back();
                avail.pop_back();
            }
        }
        return sets;
    }
    // R21 row-major; vP3D[i] / vbTriangulated[i] per keypoint of frame 1.  info (optional) receives every intermediate.
    bool Reconstruct(const std::vector<KeyPoint>& vKeys1, const std::vector<KeyPoint>& vKeys2, const std::vector<int>& vMatches12,
                     std::array<float, 9>& R21, std::array<float, 3>& t21, std::vector<std::array<float, 3>>& vP3D,
                     std::vector<bool>& vbTriangulated, orbfe_two_view_info* info = nullptr, const std::vector<int>* sets = nullptr)
    {
        const int n1 = (int)vKeys1.size(), n2 = (int)vKeys2.size();
        if ((int)vMatches12.size() != n1) throw std::invalid_argument("TwoViewReconstruction::Reconstruct: vMatches12.size() != vKeys1.size()");
        int N = 0;
        for (int m : vMatches12) N += m >= 0;
        std::vector<int> drawn;
        if (!sets && N >= 8) drawn = DrawSets(N);  // (the reference reads past an empty vector below 8 matches: nothing is drawn)
        const std::vector<int>& use = sets ? *sets : drawn;
        std::vector<float> p3d((size_t)(n1 > 0 ? n1 : 1) * 3);
        std::vector<uint8_t> tri((size_t)(n1 > 0 ? n1 : 1));
        int reconstructed = 0;
        orbfe_handle* h = ex_.handle();
        orbfe_detail::check(orbfe_two_view_reconstruct(h, &p_, n1, reinterpret_cast<const orbfe_keypoint*>(vKeys1.data()), n2,
                                                       reinterpret_cast<const orbfe_keypoint*>(vKeys2.data()), vMatches12.data(),
                                                       use.empty() ? nullptr : use.data(), &reconstructed, R21.data(), t21.data(),
                                                       p3d.data(), tri.data(), info),
                            h, "orbfe_two_view_reconstruct");
        if (!reconstructed) return false;  // the reference leaves its outputs untouched
        vP3D.resize((size_t)n1);
        vbTriangulated.assign((size_t)n1, false);
        for (int i = 0; i < n1; i++) {
            vP3D[(size_t)i] = {p3d[(size_t)3 * i], p3d[(size_t)3 * i + 1], p3d[(size_t)3 * i + 2]};
            vbTriangulated[(size_t)i] = tri[(size_t)i] != 0;
        }
        return true;
    }
    // parallax of a motion hypothesis in degrees, for display (the decisions are made on the cosine: S12)
    static float ParallaxDegrees(float cosParallax) { return (float)(std::acos((double)cosParallax) * 180.0 / 3.14159265358979323846); }
    const orbfe_two_view_params& params() const { return p_; }

private:
    ORBextractor& ex_;
    orbfe_two_view_params p_;
};

// MLPnPsolver (include/MLPnPsolver.h, src/MLPnPsolver.cpp:56-352) as ONE call (orbfe_mlpnp_ransac): the line behind SearchByBoW in
// Tracking::TrackReferenceKeyFrame (src/Tracking.cc:838-845).  The constructor takes what the reference's reads from the frame and
// the matches: mvKeysUn, one world position per keypoint (nullptr = no map point, or a bad one) and the camera.  The min-sets are
// drawn here exactly as :121-141 draws them (the RandomInt formula of Thirdparty/DBoW2/src/DUtils/Random.cpp:47-50 on the process's
// rand() stream, swap with the back), so a process that replaces the reference's class by this one sees the same sets.  The call
// is a fresh solver's first iterate(): a second iterate() on one object throws.  One stated departure: Refine's
// pose is adopted before its CheckInliers, so a refined return carries the refined pose and its inliers; the reference scores and
// returns the unrefined hypothesis there (:323-335 never write mRi / mti).
class MLPnPsolver {
public:
    MLPnPsolver(ORBextractor& extractor, const std::vector<KeyPoint>& vKeysUn, const std::vector<const std::array<float, 3>*>& vpMapPointMatches,
                int cameraModel, const std::array<float, 8>& cameraParameters, float kbPrecision = 1e-6f)
        : ex_(extractor), keys_(vKeysUn)
    {
        if (vpMapPointMatches.size() != vKeysUn.size()) throw std::invalid_argument("MLPnPsolver: one map point slot per keypoint");
        p_ = ORBFE_MLPNP_PARAMS_INIT;
        p_.camera_model = cameraModel;
        for (int i = 0; i < 8; i++) p_.cam[i] = cameraParameters[(size_t)i];
        p_.kb_precision = kbPrecision;
        mpIndex_.assign(vKeysUn.size(), -1);
        for (size_t i = 0; i < vKeysUn.size(); i++)
            if (vpMapPointMatches[i]) {
                mpIndex_[i] = (int)(points_.size() / 3);
                points_.insert(points_.end(), vpMapPointMatches[i]->begin(), vpMapPointMatches[i]->end());
                N_++;
            }
        SetRansacParameters();  // (:96: the reference's defaults until the caller sets its own)
    }
    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 6, float epsilon = 0.4f,
                             float th2 = 5.991f)
    {
        p_.probability = probability; p_.min_inliers = minInliers; p_.max_iterations = maxIterations; p_.min_set = minSet;
        p_.epsilon = epsilon; p_.th2 = th2;
    }
    // the min-sets of a first iterate(nIterations) (:121-141)
    std::vector<int> DrawSets(int nIterations)
    {
        p_.n_iterations = nIterations;
        int minInliers = 0, maxIts = 0, total = 0;
        orbfe_detail::check(orbfe_mlpnp_plan(&p_, N_, &minInliers, &maxIts, &total), nullptr, "orbfe_mlpnp_plan");
        return DrawSets(N_, total, p_.min_set);
    }
    // the same draw without an object (and so without a GPU): `total` min-sets of `minSet` out of N correspondences
    static std::vector<int> DrawSets(int N, int total, int minSet)
    {
        std::vector<int> sets((size_t)total * minSet, 0);
        std::vector<int> all((size_t)N), avail;
        for (int i = 0; i < N; i++) all[(size_t)i] = i;
        for (int it = 0; it < total; it++) {
            avail = all;
            for (int j = 0; j < minSet; j++) {
                const int d = (int)avail.size();
                const int randi = int(((double)rand() / ((double)RAND_MAX + 1.0)) * d);
                sets[(size_t)it * minSet + j] = avail[(size_t)randi];
                avail[(size_t)randi] = avail.back();
                avail.pop_back();
            }
        }
        return sets;
    }
    // Tout row-major 4 x 4; vbInliers per keypoint.  info (optional) receives every intermediate; sets (optional) replaces the draw.
    bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, std::array<float, 16>& Tout,
                 orbfe_mlpnp_info* info = nullptr, const std::vector<int>* sets = nullptr)
    {
        if (iterated_) throw std::logic_error("MLPnPsolver::iterate: the call is a fresh solver's first iterate(); make a new solver");
        iterated_ = true;
        std::vector<int> drawn;
        if (!sets) drawn = DrawSets(nIterations);
        p_.n_iterations = nIterations;
        const std::vector<int>& use = sets ? *sets : drawn;
        const int n = (int)keys_.size();
        std::vector<uint8_t> inl((size_t)(n > 0 ? n : 1));
        int solved = 0, noMore = 0;
        nInliers = 0;
        orbfe_handle* h = ex_.handle();
        orbfe_detail::check(orbfe_mlpnp_ransac(h, &p_, n, reinterpret_cast<const orbfe_keypoint*>(keys_.data()), mpIndex_.data(), N_,
                                               points_.data(), use.empty() ? nullptr : use.data(), (int)(use.size() / (size_t)p_.min_set),
                                               &solved, Tout.data(), inl.data(), &nInliers, &noMore, info),
                            h, "orbfe_mlpnp_ransac");
        bNoMore = noMore != 0;
        vbInliers.clear();  // (:103)
        if (!solved) return false;
        vbInliers.assign((size_t)n, false);
        for (int i = 0; i < n; i++) vbInliers[(size_t)i] = inl[(size_t)i] != 0;
        return true;
    }
    int correspondences() const { return N_; }
    const orbfe_mlpnp_params& params() const { return p_; }

private:
    ORBextractor& ex_;
    std::vector<KeyPoint> keys_;
    std::vector<int> mpIndex_;
    std::vector<float> points_;
    orbfe_mlpnp_params p_;
    int N_ = 0;
    bool iterated_ = false;
};

// Optimizer::PoseOptimization(pFrame) (src/Optimizer.cc:765-1067) as ONE call (orbfe_pose_optimization): the line behind the MLPnP
// solve in Tracking::TrackReferenceKeyFrame (src/Tracking.cc:869) and behind SearchLocalPoints in TrackLocalMap (:935).  It is NOT
// named Optimizer: unlike the classes above it replaces one function, not a class -- Tracking.cc keeps including Optimizer.h for
// GlobalBundleAdjustemnt (:698) and PoseInertialOptimizationLastFrame (:946), so ORB_SLAM3::Optimizer stays the reference's
// (PoseInertialOptimizationLastKeyFrame, :952, is the second wrapper below).
// `F` needs mNumKeypoints, mvKeysUn (shared_ptr<vector<KeyPoint>>), mvpMapPoints (entries with GetWorldPos()[0..2]), mvbOutlier,
// mvuRight and mpCamera2; getPose(F, Rcw[9], tcw[3]) reads pFrame->GetPose() row-major, setPose(F, Tcw[16]) is pFrame->SetPose
// (:1062-1065).  It fills mp_index / points from mvpMapPoints, writes mvbOutlier, sets the pose and returns
// nInitialCorrespondences - nBad.
// A frame with a second camera or a matched keypoint with mvuRight >= 0 throws (ORBFE_ERR_UNSUPPORTED: this fork is mono).
// Three stated departures (include/orbfe.h): the Levenberg loop and SE3Quat::exp are restated from g2o's published
// algorithm (g2o is not in the reference tree; parity with a g2o build is unpinned); the pose is kept as a rotation matrix, not a
// quaternion; the flags of a round are scored on fresh errors at its final pose, where g2o leaves the errors of a rejected last
// trial in the active edges.
struct PoseOptimizer {
    template <class FramePtr, class GetPose, class SetPose>
    static int PoseOptimization(ORBextractor& extractor, FramePtr pFrame, int cameraModel, const std::array<float, 8>& cameraParameters,
                                GetPose getPose, SetPose setPose, orbfe_pose_opt_info* info = nullptr)
    {
        orbfe_pose_opt_params p = ORBFE_POSE_OPT_PARAMS_INIT;
        p.camera_model = cameraModel;
        for (int i = 0; i < 8; i++) p.cam[i] = cameraParameters[(size_t)i];
        if (pFrame->mpCamera2) p.stereo = 1;
        const int n = pFrame->mNumKeypoints;
        std::vector<int> mpIndex((size_t)(n > 0 ? n : 1), -1);
        std::vector<float> points;
        for (int i = 0; i < n; i++) {
            auto pMP = pFrame->mvpMapPoints[(size_t)i];
            if (!pMP) continue;
            if (pFrame->mvuRight[(size_t)i] >= 0) p.stereo = 1;
            const auto P = pMP->GetWorldPos();
            mpIndex[(size_t)i] = (int)(points.size() / 3);
            points.push_back(P[0]);
            points.push_back(P[1]);
            points.push_back(P[2]);
        }
        float Rcw[9], tcw[3];
        getPose(pFrame, Rcw, tcw);
        std::array<float, 16> Tcw;
        std::vector<uint8_t> outlier((size_t)(n > 0 ? n : 1));
        int nInliers = 0;
        orbfe_handle* h = extractor.handle();
        orbfe_detail::check(orbfe_pose_optimization(h, &p, n, reinterpret_cast<const orbfe_keypoint*>(pFrame->mvKeysUn->data()), mpIndex.data(),
                                                    (int)(points.size() / 3), points.empty() ? nullptr : points.data(), Rcw, tcw, Tcw.data(),
                                                    outlier.data(), &nInliers, info),
                            h, "orbfe_pose_optimization");
        for (int i = 0; i < n; i++)
            if (mpIndex[(size_t)i] >= 0) pFrame->mvbOutlier[(size_t)i] = outlier[(size_t)i] != 0;  // (:822: false when nothing ran)
        if ((int)(points.size() / 3) < 3) return 0;  // (:949-950: the pose is not touched)
        setPose(pFrame, Tcw.data());
        return nInliers;
    }

    // Optimizer::PoseInertialOptimizationLastKeyFrame(pFrame, bRecInit) (src/Optimizer.cc:3447-3844; the call: src/Tracking.cc:952) as
    // ONE call (orbfe_pose_inertial_optimization_last_keyframe, SPEC DECISION S19).  `link` holds what the fixed key-frame vertices
    // contribute, computed by the caller with the reference's own code (which calls produce dR / dV / dP / info9 /
    // infoG / infoA), and the extrinsics.  `F` needs what PoseOptimization needs, and its map points mTrackDepth.
    // getState(F, s[33]) fills Rcw (9), tcw (3) = GetPose(), Rwb (9), twb, v = GetImuRotation / GetImuPosition / GetVelocity, bg, ba =
    // mImuBias; setState(F, s[21], H) receives Rwb, twb, v (SetImuPoseVelocity), bg, ba (mImuBias) and the raw 15 x 15 row-major H
    // for new ConstraintPoseImu(Rwb, twb, v, bg, ba, H) (:3795-3839).  It writes mvbOutlier and returns nInitialCorrespondences - nBad.
    // The stated departures are those of include/orbfe.h (no NormalizeRotation, fresh errors at the end of a round, no quaternion round
    // trip, g2o's Gauss-Newton restated).
    template <class FramePtr, class GetState, class SetState>
    static int PoseInertialOptimizationLastKeyFrame(ORBextractor& extractor, FramePtr pFrame, bool bRecInit, int cameraModel,
                                                    const std::array<float, 8>& cameraParameters, const orbfe_imu_link& link,
                                                    GetState getState, SetState setState, orbfe_pose_inertial_info* info = nullptr)
    {
        orbfe_pose_inertial_params p = ORBFE_POSE_INERTIAL_PARAMS_INIT;
        p.camera_model = cameraModel;
        p.rec_init = bRecInit ? 1 : 0;
        for (int i = 0; i < 8; i++) p.cam[i] = cameraParameters[(size_t)i];
        if (pFrame->mpCamera2) p.stereo = 1;
        const int n = pFrame->mNumKeypoints;
        std::vector<int> mpIndex((size_t)(n > 0 ? n : 1), -1);
        std::vector<float> points, depth;
        for (int i = 0; i < n; i++) {
            auto pMP = pFrame->mvpMapPoints[(size_t)i];
            if (!pMP) continue;
            if (pFrame->mvuRight[(size_t)i] >= 0) p.stereo = 1;
            const auto P = pMP->GetWorldPos();
            mpIndex[(size_t)i] = (int)depth.size();
            points.push_back(P[0]);
            points.push_back(P[1]);
            points.push_back(P[2]);
            depth.push_back(pMP->mTrackDepth);
        }
        float s[33], o[21];
        getState(pFrame, s);
        std::array<double, 225> H;
        std::vector<uint8_t> outlier((size_t)(n > 0 ? n : 1));
        int nInliers = 0;
        orbfe_handle* h = extractor.handle();
        orbfe_detail::check(orbfe_pose_inertial_optimization_last_keyframe(
                                h, &p, &link, n, reinterpret_cast<const orbfe_keypoint*>(pFrame->mvKeysUn->data()), mpIndex.data(),
                                (int)depth.size(), points.empty() ? nullptr : points.data(), depth.empty() ? nullptr : depth.data(), s, s + 9,
                                s + 12, s + 21, s + 24, s + 27, s + 30, o, o + 9, o + 12, o + 15, o + 18, H.data(), outlier.data(), &nInliers,
                                info),
                            h, "orbfe_pose_inertial_optimization_last_keyframe");
        for (int i = 0; i < n; i++)
            if (mpIndex[(size_t)i] >= 0) pFrame->mvbOutlier[(size_t)i] = outlier[(size_t)i] != 0;
        setState(pFrame, o, H.data());
        return nInliers;
    }

    // Optimizer::PoseInertialOptimizationLastFrame(pFrame, inlierThreshold, bRecInit) (src/Optimizer.cc:3846-4275; the call:
    // src/Tracking.cc:946) as ONE call (orbfe_pose_inertial_optimization_last_frame, SPEC DECISION S20).  `link` holds the previous
    // frame's state, pFrame->mpImuPreintegratedFrame at its own bias with its bias Jacobians, the informations and the extrinsics
    // (which members fill it); `prior` is pFrame->mpPrevFrame->mpcpi as an orbfe_pose_imu_prior, or nullptr when it
    // does not exist: 1000 is returned and nothing is touched (:4057-4060).  getState is PoseInertialOptimizationLastKeyFrame's;
    // setState(F, s[21], Hprior, H30) is called ONLY when the result is accepted (:4208): it receives Rwb, twb, v (SetImuPoseVelocity),
    // bg, ba (mImuBias), the raw 15 x 15 row-major Hprior for new ConstraintPoseImu(Rwb, twb, v, bg, ba, Hprior) -- its eigenvalue clamp
    // runs there -- and the 30 x 30 Hessian; it deletes the previous frame's mpcpi (:4268-4270).  mvbOutlier is written either way, as
    // the reference does.  Returns nInitialCorrespondences - nBad.
    template <class FramePtr, class GetState, class SetState>
    static int PoseInertialOptimizationLastFrame(ORBextractor& extractor, FramePtr pFrame, int inlierThreshold, bool bRecInit, int cameraModel,
                                                 const std::array<float, 8>& cameraParameters, const orbfe_imu_link_free& link,
                                                 const orbfe_pose_imu_prior* prior, GetState getState, SetState setState,
                                                 orbfe_pose_inertial_prev_info* info = nullptr, bool* acceptedOut = nullptr)
    {
        if (acceptedOut) *acceptedOut = false;
        if (!prior) return 1000;
        orbfe_pose_inertial_prev_params p = ORBFE_POSE_INERTIAL_PREV_PARAMS_INIT;
        p.camera_model = cameraModel;
        p.rec_init = bRecInit ? 1 : 0;
        p.inlier_threshold = inlierThreshold;
        for (int i = 0; i < 8; i++) p.cam[i] = cameraParameters[(size_t)i];
        if (pFrame->mpCamera2) p.stereo = 1;
        const int n = pFrame->mNumKeypoints;
        std::vector<int> mpIndex((size_t)(n > 0 ? n : 1), -1);
        std::vector<float> points, depth;
        for (int i = 0; i < n; i++) {
            auto pMP = pFrame->mvpMapPoints[(size_t)i];
            if (!pMP) continue;
            if (pFrame->mvuRight[(size_t)i] >= 0) p.stereo = 1;
            const auto P = pMP->GetWorldPos();
            mpIndex[(size_t)i] = (int)depth.size();
            points.push_back(P[0]);
            points.push_back(P[1]);
            points.push_back(P[2]);
            depth.push_back(pMP->mTrackDepth);
        }
        float s[33], o[21];
        getState(pFrame, s);
        std::vector<double> H30(900), Hp(225);
        std::vector<uint8_t> outlier((size_t)(n > 0 ? n : 1));
        int nInliers = 0, accepted = 0;
        orbfe_handle* h = extractor.handle();
        orbfe_detail::check(orbfe_pose_inertial_optimization_last_frame(
                                h, &p, &link, prior, n, reinterpret_cast<const orbfe_keypoint*>(pFrame->mvKeysUn->data()), mpIndex.data(),
                                (int)depth.size(), points.empty() ? nullptr : points.data(), depth.empty() ? nullptr : depth.data(), s, s + 9,
                                s + 12, s + 21, s + 24, s + 27, s + 30, o, o + 9, o + 12, o + 15, o + 18, H30.data(), Hp.data(),
                                outlier.data(), &nInliers, &accepted, info),
                            h, "orbfe_pose_inertial_optimization_last_frame");
        for (int i = 0; i < n; i++)
            if (mpIndex[(size_t)i] >= 0) pFrame->mvbOutlier[(size_t)i] = outlier[(size_t)i] != 0;
        if (accepted) setState(pFrame, o, Hp.data(), H30.data());
        if (acceptedOut) *acceptedOut = accepted != 0;
        return nInliers;
    }
};

// Tracking::PreintegrateIMU (src/Tracking.cc:234-290), Tracking::PredictStateIMU (:293-350) and the builders of the two inertial links
// (SPEC DECISION S22): what stands in front of FrameTracker and of PoseOptimizer's two inertial wrappers once the IMU is initialised.
// The caller keeps the reference's queue handling (:201-232) and hands the selected mvImuFromLastFrame over; the records are
// orbfe_imu_preint blocks (IMU::Preintegrated without mvMeasurements), the steps go back for mvMeasurements.  Passing the link to
// PoseOptimizer::PoseInertialOptimizationLastKeyFrame / LastFrame is the caller's one line.
// The stated departures are those of include/orbfe.h (the polar-factor NormalizeRotation, pinned sin / cos, ExpSO3 in binary64, L D L^T
// for the covariance's inverse, Jacobi for its eigen-decomposition).
class ImuPreintegrator {
public:
    // calib.Cov / calib.CovWalk diagonals (ng^2 x 3, na^2 x 3 / ngw^2 x 3, naw^2 x 3), IMU::GRAVITY_VALUE, mImuCalib.mTcb / mTbc
    ImuPreintegrator(ORBextractor& extractor, const std::array<float, 6>& cov, const std::array<float, 6>& covWalk, float gravity,
                     const float* Rcb, const float* tcb, const float* tbc)
        : mExtractor(extractor)
    {
        mNoise.struct_size = (int)sizeof mNoise;
        mNoise.reserved = 0;
        for (int i = 0; i < 6; i++) {
            mNoise.cov[i] = cov[(size_t)i];
            mNoise.cov_walk[i] = covWalk[(size_t)i];
        }
        mParams.struct_size = (int)sizeof mParams;
        mParams.which = ORBFE_IMU_FROM_KEYFRAME;
        mParams.gravity = gravity;
        std::memcpy(mParams.Rcb, Rcb, sizeof mParams.Rcb);
        std::memcpy(mParams.tcb, tcb, sizeof mParams.tcb);
        std::memcpy(mParams.tbc, tbc, sizeof mParams.tbc);
    }

    // new IMU::Preintegrated(bias, calib): Initialize(b) (src/ImuTypes.cc:149-168); bias = bwx bwy bwz bax bay baz
    orbfe_imu_preint Fresh(const float* bias) const { return Reintegrate(bias, std::vector<orbfe_imu_step>()); }

    // The loop of PreintegrateIMU over mvImuFromLastFrame: `fromLastKF` (mpImuPreintegratedFromLastKF) is integrated in place,
    // `fromLastFrame` (pImuPreintegratedFromLastFrame) is made at lastFrameBias (mLastFrame->mImuBias), `steps` receives the n - 1
    // integrable entries.  false = the reference's early return (:235-238): fewer than two samples, nothing touched.
    bool PreintegrateIMU(const std::vector<orbfe_imu_sample>& imuFromLastFrame, double prevStamp, double curStamp, const float* lastFrameBias,
                         orbfe_imu_preint& fromLastKF, orbfe_imu_preint& fromLastFrame, std::vector<orbfe_imu_step>* steps = nullptr) const
    {
        const int n = (int)imuFromLastFrame.size();
        if (steps) steps->assign((size_t)(n > 1 ? n - 1 : 0), orbfe_imu_step{});
        int nSteps = 0;
        orbfe_handle* h = mExtractor.handle();
        fromLastFrame.struct_size = (int)sizeof fromLastFrame;
        orbfe_detail::check(orbfe_imu_preintegrate_frame(h, &mNoise, n, imuFromLastFrame.data(), prevStamp, curStamp, lastFrameBias, &fromLastKF,
                                                         &fromLastFrame, steps && n > 1 ? steps->data() : nullptr, &nSteps),
                            h, "orbfe_imu_preintegrate_frame");
        return nSteps > 0;
    }

    // Preintegrated::Reintegrate() with the record's own list; MergePrevious(pPrev) with pPrev's list followed by the record's
    orbfe_imu_preint Reintegrate(const float* bias, const std::vector<orbfe_imu_step>& measurements) const
    {
        orbfe_imu_preint out;
        orbfe_handle* h = mExtractor.handle();
        orbfe_detail::check(orbfe_imu_reintegrate(h, &mNoise, bias, (int)measurements.size(), measurements.empty() ? nullptr : measurements.data(),
                                                  &out),
                            h, "orbfe_imu_reintegrate");
        return out;
    }

    // PredictStateIMU's mbMapUpdated branch (:301-325) and the link of PoseInertialOptimizationLastKeyFrame.  lastKeyFrameState (21) =
    // GetImuRotation (9, row-major), GetImuPosition, GetVelocity, GetGyroBias, GetAccBias of mpLastKeyFrame; state (33) = Rcw tcw Rwb
    // twb v bg ba: what SetImuPoseVelocity and mImuBias receive, and getState of the pose optimisation.  Returns info_ok.
    bool PredictStateIMU(const float* lastKeyFrameState, const orbfe_imu_preint& fromLastKF, float* state, orbfe_imu_link& link) const
    {
        return Predict(ORBFE_IMU_FROM_KEYFRAME, lastKeyFrameState, fromLastKF, nullptr, state, &link);
    }

    // PredictStateIMU's other branch (:326-347) and the link of PoseInertialOptimizationLastFrame: the last frame's state, the frame
    // record; infoG / infoA come from the key-frame record (src/Optimizer.cc:4046)
    bool PredictStateIMU(const float* lastFrameState, const orbfe_imu_preint& fromLastKF, const orbfe_imu_preint& fromLastFrame, float* state,
                         orbfe_imu_link_free& link) const
    {
        return Predict(ORBFE_IMU_FROM_FRAME, lastFrameState, fromLastKF, &fromLastFrame, state, &link);
    }

    // the links alone (the prediction is computed and dropped)
    bool LinkLastKeyFrame(const float* lastKeyFrameState, const orbfe_imu_preint& fromLastKF, orbfe_imu_link& link) const
    {
        float state[33];
        return PredictStateIMU(lastKeyFrameState, fromLastKF, state, link);
    }
    bool LinkLastFrame(const float* lastFrameState, const orbfe_imu_preint& fromLastKF, const orbfe_imu_preint& fromLastFrame,
                       orbfe_imu_link_free& link) const
    {
        float state[33];
        return PredictStateIMU(lastFrameState, fromLastKF, fromLastFrame, state, link);
    }

    const orbfe_imu_noise& noise() const { return mNoise; }
    const orbfe_imu_predict_params& params() const { return mParams; }

private:
    bool Predict(int which, const float* state1, const orbfe_imu_preint& kf, const orbfe_imu_preint* frame, float* state, void* link) const
    {
        orbfe_imu_predict_params p = mParams;
        p.which = which;
        int ok = 0;
        orbfe_handle* h = mExtractor.handle();
        orbfe_detail::check(orbfe_imu_predict(h, &p, state1, &kf, frame, state, link, &ok), h, "orbfe_imu_predict");
        return ok != 0;
    }

    ORBextractor& mExtractor;
    orbfe_imu_noise mNoise;
    orbfe_imu_predict_params mParams;
};

// Tracking::Track for one frame once the IMU is initialised, as ONE call (orbfe_track_frame_inertial, SPEC DECISION S23): Frame::Frame
// -> ExtractORB, PreintegrateIMU, PredictStateIMU, TrackLocalMap -- SearchLocalPoints against the predicted pose, the inertial pose
// optimisation (src/Tracking.cc:946 / :952) and the loop of :958-982.  It owns what the reference keeps between frames for this: the
// two preintegration records (mpImuPreintegratedFromLastKF, and the frame's own) and the prior the last-frame optimisation leaves
// for the next frame (pFrame->mpcpi).  The local map points are named by id out of a ResidentMap (id >= 0, ~id = mnLastFrameSeen ==
// this frame, src/Tracking.cc:1066).  The caller keeps the queue handling (:201-232), the map-point bookkeeping from `found` /
// `match` (IncreaseVisible for in_view records, IncreaseFound for found ones, mvpMapPoints, mvbOutlier) and the key-frame decision
// (NeedNewKeyFrame reads matchesInliers).
class InertialFrameTracker {
public:
    struct Result {
        int n = 0;                          // keypoints; 0: the reference returns before Track() (:158-159)
        std::vector<KeyPoint> keys;
        std::vector<uint8_t> descriptors;   // n x 32
        std::vector<orbfe_imu_step> steps;  // for mvMeasurements
        float predicted[33];                // Rcw tcw Rwb twb v bg ba
        float state[21];                    // the optimised Rwb twb v bg ba
        float Tcw[12];                      // Rcw then tcw: what SetImuPoseVelocity leaves in the frame
        std::vector<orbfe_map_point> points;// per id slot: the mTrack* fields; in_view = IncreaseVisible
        std::vector<int> match;             // per keypoint: the id slot in mvpMapPoints, or -1
        std::vector<uint8_t> outlier;       // mvbOutlier
        std::vector<uint8_t> found;         // per id slot: IncreaseFound
        int nMatches = 0, nInliers = 0, matchesInliers = 0;
        bool accepted = true, tracked = false, infoOk = false;
    };

    // `params`: grid, matcher, noise, extrinsics, the frustum template and both pose blocks; predict.which is set per call
    InertialFrameTracker(ORBextractor& extractor, const orbfe_track_inertial_params& params) : mExtractor(extractor), mParams(params)
    {
        mFromLastKF.struct_size = mFromLastFrame.struct_size = (int)sizeof(orbfe_imu_preint);
        mPrior.struct_size = (int)sizeof mPrior;
    }

    // a new key frame: mpImuPreintegratedFromLastKF = new IMU::Preintegrated(bias, calib) (src/Tracking.cc:1339), or a record the
    // caller carries over
    void ResetFromLastKF(const orbfe_imu_preint& fresh) { mFromLastKF = fresh; }
    const orbfe_imu_preint& FromLastKF() const { return mFromLastKF; }
    const orbfe_imu_preint& FromLastFrame() const { return mFromLastFrame; }
    bool HasPrior() const { return mHasPrior; }
    void DropPrior() { mHasPrior = false; }

    // mapUpdated (mbMapUpdated, :946-952) or no prior yet: against the last key frame, `startState` = its Rwb twb v bg ba; else against
    // the last frame, `startState` = that frame's: the caller picks it by `mapUpdated || !HasPrior()`.  lastFrameBias =
    // mLastFrame->mImuBias.  The last frame's state afterwards is Result::state -- unless this call ran against the last frame and
    // the result is not accepted (src/Optimizer.cc:4208-4213 did not run): then it is Result::predicted + 12, and no prior is left.
    Result Track(const GrayImageView& im, const std::vector<orbfe_imu_sample>& imuFromLastFrame, double prevStamp, double curStamp,
                 const float* lastFrameBias, const float* startState, bool mapUpdated, const ResidentMap& map, const std::vector<int>& ids)
    {
        orbfe_handle* h = mExtractor.handle();
        const int cap = mExtractor.maxKeypoints(), M = (int)ids.size(), nS = (int)imuFromLastFrame.size();
        const bool fromFrame = !mapUpdated && mHasPrior;
        mParams.predict.which = fromFrame ? ORBFE_IMU_FROM_FRAME : ORBFE_IMU_FROM_KEYFRAME;
        Result R;
        R.keys.resize((size_t)cap);
        R.descriptors.resize((size_t)cap * ORBFE_DESC_BYTES);
        R.steps.resize((size_t)(nS > 1 ? nS - 1 : 1));
        R.points.resize((size_t)(M > 0 ? M : 1));
        R.match.assign((size_t)cap, -1);
        R.outlier.assign((size_t)cap, 0);
        R.found.assign((size_t)(M > 0 ? M : 1), 0);
        std::vector<double> H(fromFrame ? 900 : 225), Hp(225);
        orbfe_track_inertial_result res{};
        res.struct_size = (int)sizeof res;
        res.steps_out = R.steps.data();
        res.state_in = R.predicted;
        res.mp_out = R.points.data();
        res.match_out = R.match.data();
        res.state_out = R.state;
        res.H_out = H.data();
        res.Hprior_out = fromFrame ? Hp.data() : nullptr;
        res.outlier = R.outlier.data();
        res.found = R.found.data();
        orbfe_detail::check(orbfe_track_frame_inertial(h, &mParams, im.data, im.pitch, nS, imuFromLastFrame.data(), prevStamp, curStamp,
                                                       lastFrameBias, startState, &mFromLastKF, &mFromLastFrame, map.get(), M, ids.data(),
                                                       fromFrame ? &mPrior : nullptr, reinterpret_cast<orbfe_keypoint*>(R.keys.data()),
                                                       R.descriptors.data(), &R.n, nullptr, &res),
                            h, "orbfe_track_frame_inertial");
        R.keys.resize((size_t)R.n);
        R.descriptors.resize((size_t)R.n * ORBFE_DESC_BYTES);
        R.steps.resize((size_t)res.n_steps);
        R.points.resize((size_t)M);
        R.found.resize((size_t)M);
        R.match.resize((size_t)R.n);
        R.outlier.resize((size_t)R.n);
        std::memcpy(R.Tcw, res.Tcw, sizeof R.Tcw);
        R.nMatches = res.n_matches;
        R.nInliers = res.n_inliers;
        R.matchesInliers = res.matches_inliers;
        R.accepted = res.accepted != 0;
        R.tracked = res.tracked != 0;
        R.infoOk = res.info_ok != 0;
        // pFrame->mpcpi = new ConstraintPoseImu(Rwb, twb, v, bg, ba, H) (src/Optimizer.cc:3841, :4271): the optimised state and the raw
        // Hessian block; the constructor's eigenvalue clamp (include/G2oTypes.h) stays with the caller, through Prior().
        // A prior exists afterwards if and only if THIS frame left one: the last-frame kind leaves none when it is rejected
        // (:4268 stands inside `if(validPoints >= inlierThreshold)`, :4208) and the frame's own mpcpi starts as nullptr
        // (src/Frame.cc:59), so the next frame falls back to the last key frame (src/Tracking.cc:940-953) instead of running
        // against this one with the prior of the frame before it.  The key-frame kind always accepts.
        mHasPrior = R.accepted;
        if (R.accepted) {
            const double* src = fromFrame ? Hp.data() : H.data();
            for (int i = 0; i < 9; i++) mPrior.Rwb[i] = (double)R.state[i];
            for (int i = 0; i < 3; i++) {
                mPrior.twb[i] = (double)R.state[9 + i];
                mPrior.vwb[i] = (double)R.state[12 + i];
                mPrior.bg[i] = (double)R.state[15 + i];
                mPrior.ba[i] = (double)R.state[18 + i];
            }
            std::memcpy(mPrior.H, src, sizeof mPrior.H);
        }
        return R;
    }

    // the prior as the caller wants the next frame to see it (after the constructor's clamp of negative eigenvalues)
    orbfe_pose_imu_prior& Prior() { return mPrior; }

private:
    ORBextractor& mExtractor;
    orbfe_track_inertial_params mParams;
    orbfe_imu_preint mFromLastKF{}, mFromLastFrame{};
    orbfe_pose_imu_prior mPrior{};
    bool mHasPrior = false;
};

// The numerical core of Tracking::CreateInitialMapMonocular (src/Tracking.cc:698-729) as ONE device call and a host step:
// Optimizer::GlobalBundleAdjustemnt(map, 20) -- two key frames of which the first is fixed, every initial map point seen once in
// either -- is orbfe_initial_bundle_adjustment (SPEC DECISION S17); KeyFrame::ComputeSceneMedianDepth(2) (src/KeyFrame.cc:859-892)
// and the rescale of the baseline and the points (:700-729) run here in binary32, as the reference's floats do:
//   z = ((r20 X + r21 Y) + r22 Z) + t2 with pose 1 and the adjusted points, sorted ascending, element (N - 1) / 2;
//   invMedianDepth = 4.0f / median when inertial (IMU_MONOCULAR, :702-703), else 1.0f / median.
// keys1 / keys2 = the two key frames' mvKeysUn, matches12 = vIniMatches, points = vIniP3D as n1 x 3 floats (in: the triangulated
// points; out: adjusted, and scaled when the result is true; rows without a match are left alone), Rcw1 / tcw1 = pose 1 (fixed),
// Rcw2 / tcw2 = pose 2 (in: the start; out: adjusted, tcw2 scaled when the result is true).
// false = the reference's "Wrong initialization, reseting" (:707): median < 0 or fewer than 50 points -- or a NaN among the depths,
// which the reference would hand to std::sort (undefined behaviour there, a refusal here).  The outputs then hold the adjusted,
// unscaled values.
struct InitialMapAdjuster {
    static bool Adjust(ORBextractor& extractor, int cameraModel, const std::array<float, 8>& cameraParameters, const std::vector<KeyPoint>& keys1,
                       const std::vector<KeyPoint>& keys2, const std::vector<int>& matches12, std::vector<float>& points, const float* Rcw1,
                       const float* tcw1, float* Rcw2, float* tcw2, bool inertial, float* medianDepth = nullptr,
                       orbfe_initial_ba_info* info = nullptr)
    {
        orbfe_initial_ba_params p = ORBFE_INITIAL_BA_PARAMS_INIT;
        p.camera_model = cameraModel;
        for (int i = 0; i < 8; i++) p.cam[i] = cameraParameters[(size_t)i];
        const int n1 = (int)keys1.size(), n2 = (int)keys2.size();
        if ((int)matches12.size() != n1 || (int)points.size() != 3 * n1) throw std::invalid_argument("InitialMapAdjuster::Adjust: sizes");
        std::array<float, 16> Tcw;
        orbfe_handle* h = extractor.handle();
        orbfe_detail::check(orbfe_initial_bundle_adjustment(h, &p, n1, reinterpret_cast<const orbfe_keypoint*>(keys1.data()), n2,
                                                            reinterpret_cast<const orbfe_keypoint*>(keys2.data()), matches12.data(),
                                                            points.data(), Rcw1, tcw1, Rcw2, tcw2, Tcw.data(), points.data(), info),
                            h, "orbfe_initial_bundle_adjustment");
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) Rcw2[3 * i + j] = Tcw[(size_t)(4 * i + j)];
            tcw2[i] = Tcw[(size_t)(4 * i + 3)];
        }
        return MedianDepthScale(matches12, points, Rcw1, tcw1, tcw2, inertial, medianDepth);
    }

    // The host step of Adjust on the C call's outputs (src/KeyFrame.cc:859-892, src/Tracking.cc:700-729): the median depth of the
    // matched rows of `points` in key frame 1, then -- when the result is true -- tcw2 and those rows scaled by 1 / median (4 / median
    // when inertial).  It touches no device: tests/cpp/initial_ba.cpp runs this text on its host loop's results.
    static bool MedianDepthScale(const std::vector<int>& matches12, std::vector<float>& points, const float* Rcw1, const float* tcw1,
                                 float* tcw2, bool inertial, float* medianDepth = nullptr)
    {
        const int n1 = (int)matches12.size();
        std::vector<float> depths;
        bool nan = false;
        for (int i = 0; i < n1; i++) {
            if (matches12[(size_t)i] < 0) continue;
            const float* X = &points[3 * (size_t)i];
            const float z = ((Rcw1[6] * X[0] + Rcw1[7] * X[1]) + Rcw1[8] * X[2]) + tcw1[2];
            nan = nan || z != z;
            depths.push_back(z);
        }
        if (medianDepth) *medianDepth = 0.0f;
        if (depths.empty()) return false;
        if (nan) {
            if (medianDepth) *medianDepth = std::numeric_limits<float>::quiet_NaN();
            return false;
        }
        std::sort(depths.begin(), depths.end());
        const float median = depths[(depths.size() - 1) / 2];
        if (medianDepth) *medianDepth = median;
        if (median < 0 || depths.size() < 50) return false;
        const float invMedianDepth = (inertial ? 4.0f : 1.0f) / median;
        for (int i = 0; i < 3; i++) tcw2[i] = tcw2[i] * invMedianDepth;
        for (int i = 0; i < n1; i++)
            if (matches12[(size_t)i] >= 0)
                for (int k = 0; k < 3; k++) points[3 * (size_t)i + k] = points[3 * (size_t)i + k] * invMedianDepth;
        return true;
    }
};

}  // namespace ORB_SLAM3
