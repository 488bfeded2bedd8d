/*
 * Tracking_coeb.h -- MI355X bodies for Tracking::SearchLocalPoints, Tracking::TrackLocalMap
 * (src/Tracking.cc:1222-1272, 996-1047), Tracking::TrackReferenceKeyFrame (:823-865) and
 * Tracking::TrackWithMotionModel (:933-994, both further down).  The first two: Frame::isInFrustum
 * over the local map, the local-map projection search, the pose optimisation and the inlier count in
 * one library call with one synchronisation (coeb_search_local_points / coeb_track_local_map).
 *
 * Included from the reference's src/Tracking.cc.  SearchLocalPoints' body becomes
 *
 *     int th = 1; if (mSensor == System::RGBD) th = 3;
 *     if (mCurrentFrame.mnId < mnLastRelocFrameId + 2) th = 5;
 *     coeb::SearchLocalPoints(mCurrentFrame, mvpLocalMapPoints, th, 0.8f);
 *
 * and TrackLocalMap's, after UpdateLocalMap() and up to the decision at :1029, becomes
 *
 *     mnMatchesInliers = coeb::TrackLocalMap(mCurrentFrame, mvpLocalMapPoints, th, 0.8f, mbOnlyTracking,
 *                                            mSensor == System::STEREO);
 *
 * What they do, in the reference's terms and in its order:
 *   - the first loop of :1225-1241: a bad MapPoint of the frame is reset to NULL, the others get
 *     IncreaseVisible(), mnLastFrameSeen = F.mnId and mbTrackInView = false;
 *   - snapshot, per local-map point: valid = mnLastFrameSeen != F.mnId && !isBad() (:1249-1252),
 *     GetWorldPos(), GetNormal(), mfMaxDistance / mfMinDistance (the two getters INTEGRATION.md s3
 *     adds), GetDescriptor(), Observations(); per keypoint: Observations() and GetWorldPos() of the
 *     MapPoint it holds (-1 for NULL); positions are read under MapPoint::mGlobalMutex as
 *     Optimizer::PoseOptimization reads them (Optimizer.cc:276);
 *   - the call;
 *   - per valid point what isInFrustum leaves (Frame.cc:447, 493-498): mbTrackInView, and where it
 *     is set mTrackProjX / Y / XR, mnTrackScaleLevel, mTrackViewCos and IncreaseVisible() (:1256);
 *   - F.mvpMapPoints[i] = vpLocalMapPoints[match[i]] (ORBmatcher.cc:123);
 *   - TrackLocalMap only: mvbOutlier for the keypoints that hold a point and F.SetPose (with at
 *     least 3 of them, Optimizer.cc:361-362, 446-448), then IncreaseFound() for the inliers and, for
 *     a stereo sensor, NULL for the outliers (:1013-1026); the return value is mnMatchesInliers.
 *
 * Tracking::TrackReferenceKeyFrame (src/Tracking.cc:823-865) becomes
 *
 *     return coeb::TrackReferenceKeyFrame(mCurrentFrame, mpReferenceKF, mLastFrame.mTcw, *coeb_voc);
 *
 * one library call with one synchronisation (coeb_track_reference_keyframe), where coeb_voc is the
 * coeb::Vocabulary of BoW_coeb.h.  In the reference's order:
 *   - snapshot of the KeyFrame: valid = vpMapPointsKF[i] && !isBad(), the mFeatVec node of every
 *     feature (feature_nodes, ORBmatcher_coeb.h), mDescriptors, mvKeysUn[i].angle, and GetWorldPos()
 *     / Observations() of the valid MapPoints under MapPoint::mGlobalMutex;
 *   - ComputeBoW: with F.mBowVec empty the call runs the transform and F.mBowVec / F.mFeatVec are
 *     filled from its words (coeb_bow_vector: addWeight in feature order, normalize(L1)) and node
 *     ids; otherwise F.mFeatVec's node ids go in and no vocabulary is touched;
 *   - nmatches < 15 (:835): false, with F.mvpMapPoints and the pose as they were;
 *   - F.mvpMapPoints = vpMapPointMatches less the optimiser's outliers, mvbOutlier false on every
 *     matched keypoint (:854 and Optimizer.cc:302), F.SetPose(the optimised pose; mLastFrame.mTcw
 *     with fewer than 3 edges);
 *   - mbTrackInView = false and mnLastFrameSeen = F.mnId on the discarded MapPoints (:855-856);
 *   - the return value is nmatchesMap >= 10.
 *
 * Tracking::TrackWithMotionModel (src/Tracking.cc:933-994) becomes, with UpdateLastFrame cut down to
 * its first lines (:870-873, the pose from mlRelativeFramePoses),
 *
 *     UpdateLastFramePose();
 *     const bool bCreateVO = mnLastKeyFrameId != mLastFrame.mnId && mSensor != System::MONOCULAR && mbOnlyTracking;
 *     return coeb::TrackWithMotionModel(mCurrentFrame, mLastFrame, mVelocity, mSensor != System::STEREO ? 15 : 7,
 *                mSensor == System::MONOCULAR, mbOnlyTracking, bCreateVO, mThDepth,
 *                [&](const cv::Mat& x3D, int i) { return new MapPoint(x3D, mpMap, &mLastFrame, i); },
 *                mlpTemporalPoints, &mbVO);
 *
 * one library call with one synchronisation (coeb_track_motion_model).  In the reference's order:
 *   - snapshot of mLastFrame: per keypoint whether it holds a MapPoint, mvbOutlier, and GetWorldPos() /
 *     GetDescriptor() / Observations() of the point under MapPoint::mGlobalMutex; with bCreateVO also
 *     mvDepth and mDescriptors;
 *   - F.SetPose(mVelocity * mLastFrame.mTcw) (:941), the product in the caller's matrix type;
 *   - the call: the visual-odometry points, the search with its 2*th retry, the gate, the pose
 *     optimisation and the discard;
 *   - with bCreateVO the temporary MapPoints (:913-922): for every created slot, in the order of the
 *     depth sort, newTemporalPoint(x3D, i) goes into mLastFrame.mvpMapPoints[i] and to the back of
 *     mlpTemporalPoints;
 *   - F.mvpMapPoints = the search's assignments less the optimiser's outliers; nmatches < 20 (:960):
 *     false, with the predicted pose; else F.SetPose(the optimised pose), mvbOutlier false on every
 *     matched keypoint, mbTrackInView = false and mnLastFrameSeen = F.mnId on the discarded MapPoints;
 *   - :987-993: in localisation mode mbVO = nmatchesMap < 10 and the return value is nmatches > 20,
 *     otherwise nmatchesMap >= 10.
 *
 * The vocabulary's context has ORB-SLAM2's pyramid (8 levels, 1.2): its mvInvLevelSigma2 weigh the
 * edges, so a frame with another pyramid is refused.
 */
#ifndef COEB_ADAPTER_TRACKING_H
#define COEB_ADAPTER_TRACKING_H

#include <algorithm>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <type_traits>
#include <utility>
#include <vector>

#include <opencv2/core/core.hpp>

#include "coeb_front.h"
#include "BoW_coeb.h"
#include "ORBmatcher_coeb.h"

namespace coeb
{

namespace detail
{

// pose: TrackLocalMap (search + optimisation + inlier count), else SearchLocalPoints alone.
// Returns mnMatchesInliers, or nToMatch for the search alone.
template <class FrameT, class MapPointT>
inline int track_local_map(FrameT& F, const std::vector<MapPointT*>& vpLocalMapPoints, float th, float nnratio, bool pose,
                           bool bOnlyTracking, bool bStereo, coeb_ctx* ctx)
{
    if (!ctx) ctx = matcher_ctx(F.mnScaleLevels, F.mfScaleFactor);
    const int N = F.N, nq = (int)vpLocalMapPoints.size();
    // Do not search map points already matched (:1225-1241)
    for (int i = 0; i < N; ++i) {
        MapPointT* pMP = F.mvpMapPoints[i];
        if (!pMP) continue;
        if (pMP->isBad()) {
            F.mvpMapPoints[i] = static_cast<MapPointT*>(nullptr);
        } else {
            pMP->IncreaseVisible();
            pMP->mnLastFrameSeen = F.mnId;
            pMP->mbTrackInView = false;
        }
    }
    std::vector<uint8_t> valid(nq), desc((size_t)nq * 32);
    std::vector<float> xw((size_t)nq * 3), normal((size_t)nq * 3), maxd(nq), mind(nq), cxw((size_t)N * 3);
    std::vector<int32_t> nobs(nq), cobs((size_t)N);
    {
        std::unique_lock<std::mutex> lock(MapPointT::mGlobalMutex);
        for (int q = 0; q < nq; ++q) {
            MapPointT* pMP = vpLocalMapPoints[q];
            valid[q] = pMP->mnLastFrameSeen != F.mnId && !pMP->isBad();
            if (!valid[q]) continue;
            cv::Mat P = pMP->GetWorldPos(), Pn = pMP->GetNormal();
            for (int k = 0; k < 3; ++k) {
                xw[3 * q + k] = P.at<float>(k);
                normal[3 * q + k] = Pn.at<float>(k);
            }
            maxd[q] = pMP->GetMaxDistance();
            mind[q] = pMP->GetMinDistance();
            cv::Mat d = pMP->GetDescriptor();
            std::memcpy(&desc[32 * (size_t)q], d.ptr<uint8_t>(0), 32);
            nobs[q] = pMP->Observations();
        }
        for (int i = 0; i < N; ++i) {
            MapPointT* pMP = F.mvpMapPoints[i];
            cobs[i] = pMP ? pMP->Observations() : -1;
            if (!pMP) continue;
            cv::Mat P = pMP->GetWorldPos();
            for (int k = 0; k < 3; ++k) cxw[3 * i + k] = P.at<float>(k);
        }
    }
    coeb_local_points pts{nq, valid.data(), xw.data(), normal.data(), maxd.data(), mind.data(), desc.data(), nobs.data()};
    cv::Mat curDesc = F.mDescriptors.isContinuous() ? F.mDescriptors : F.mDescriptors.clone();
    coeb_curframe cur{N, reinterpret_cast<const coeb_keypoint*>(F.mvKeysUn.data()),
                      curDesc.empty() ? nullptr : curDesc.ptr<uint8_t>(0), F.mvuRight.data()};
    const coeb_camera cam = frame_camera(F);
    float T[16];
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) T[4 * r + k] = F.mTcw.template at<float>(r, k);
    std::vector<uint8_t> view(nq), outl((size_t)N);
    std::vector<float> px(nq), py(nq), pxr(nq), vcos(nq);
    std::vector<int32_t> lvl(nq), match((size_t)N);
    coeb_track_fields tf{view.data(), px.data(), py.data(), pxr.data(), lvl.data(), vcos.data()};
    int nToMatch = 0, nlocal = 0, ninl = 0, nMatchesInliers = 0;
    const int rc = pose ? coeb_track_local_map(ctx, &cam, &cur, cobs.data(), cxw.data(), T, &pts, 0.5f, th, nnratio,
                                               bOnlyTracking ? 1 : 0, &tf, match.data(), outl.data(), &nToMatch, &nlocal,
                                               &ninl, &nMatchesInliers)
                        : coeb_search_local_points(ctx, &cam, &cur, cobs.data(), T, &pts, 0.5f, th, nnratio, &tf,
                                                   match.data(), &nToMatch, &nlocal);
    if (rc != COEB_OK) throw std::runtime_error(coeb_last_error(ctx));
    // Project points in frame and check its visibility (:1246-1259)
    for (int q = 0; q < nq; ++q) {
        if (!valid[q]) continue;
        MapPointT* pMP = vpLocalMapPoints[q];
        pMP->mbTrackInView = view[q] != 0;
        if (!view[q]) continue;
        pMP->mTrackProjX = px[q];
        pMP->mTrackProjXR = pxr[q];
        pMP->mTrackProjY = py[q];
        pMP->mnTrackScaleLevel = lvl[q];
        pMP->mTrackViewCos = vcos[q];
        pMP->IncreaseVisible();
    }
    for (int i = 0; i < N; ++i)
        if (match[i] >= 0) F.mvpMapPoints[i] = vpLocalMapPoints[match[i]];
    if (!pose) return nToMatch;
    // Optimizer::PoseOptimization's outputs (Optimizer.cc:361-362, 437-448)
    int nInitial = 0;
    for (int i = 0; i < N; ++i)
        if (F.mvpMapPoints[i]) { F.mvbOutlier[i] = outl[i] != 0; nInitial++; }
    if (nInitial >= 3) {
        cv::Mat Tcw(4, 4, CV_32F);
        for (int r = 0; r < 4; ++r)
            for (int k = 0; k < 4; ++k) Tcw.at<float>(r, k) = T[4 * r + k];
        F.SetPose(Tcw);
    }
    // Update MapPoints Statistics (:1010-1027); the count is the call's
    for (int i = 0; i < N; ++i) {
        if (!F.mvpMapPoints[i]) continue;
        if (!F.mvbOutlier[i]) F.mvpMapPoints[i]->IncreaseFound();
        else if (bStereo) F.mvpMapPoints[i] = static_cast<MapPointT*>(nullptr);
    }
    return nMatchesInliers;
}

}  // namespace detail

// Tracking::SearchLocalPoints (th as the reference picks it at :1263-1269); returns nToMatch
template <class FrameT, class MapPointT>
inline int SearchLocalPoints(FrameT& F, const std::vector<MapPointT*>& vpLocalMapPoints, float th, float nnratio,
                             coeb_ctx* ctx = nullptr)
{
    return detail::track_local_map(F, vpLocalMapPoints, th, nnratio, false, false, false, ctx);
}

// Tracking::TrackLocalMap between UpdateLocalMap() and the decision at :1029; returns mnMatchesInliers
template <class FrameT, class MapPointT>
inline int TrackLocalMap(FrameT& F, const std::vector<MapPointT*>& vpLocalMapPoints, float th, float nnratio,
                         bool bOnlyTracking, bool bStereo = false, coeb_ctx* ctx = nullptr)
{
    return detail::track_local_map(F, vpLocalMapPoints, th, nnratio, true, bOnlyTracking, bStereo, ctx);
}

// Tracking::TrackReferenceKeyFrame; *pnMatchesMap (when given) receives nmatchesMap
template <class FrameT, class KeyFrameT, class MatT>
inline bool TrackReferenceKeyFrame(FrameT& F, KeyFrameT* pRefKF, const MatT& lastTcw, Vocabulary& voc, float nnratio = 0.7f,
                                   bool bCheckOrientation = true, int levelsup = 4, int* pnMatchesMap = nullptr)
{
    auto vpMapPointsKF = pRefKF->GetMapPointMatches();
    typedef typename std::remove_pointer<typename decltype(vpMapPointsKF)::value_type>::type MapPointT;
    const bool bTransform = F.mBowVec.empty();      // ComputeBoW's guard (Frame.cc:572)
    if (bTransform && (F.mnScaleLevels != 8 || F.mfScaleFactor != 1.2f))
        throw std::runtime_error("coeb::TrackReferenceKeyFrame: the frame's pyramid is not the vocabulary context's");
    coeb_ctx* ctx = bTransform ? voc.ctx() : matcher_ctx(F.mnScaleLevels, F.mfScaleFactor);
    const int N = F.N, nq = (int)vpMapPointsKF.size();
    std::vector<uint8_t> valid(nq);
    std::vector<float> kang(nq), xw((size_t)nq * 3);
    std::vector<int32_t> nobs(nq);
    {
        std::unique_lock<std::mutex> lock(MapPointT::mGlobalMutex);
        for (int i = 0; i < nq; ++i) {
            MapPointT* pMP = vpMapPointsKF[i];
            valid[i] = pMP && !pMP->isBad();
            kang[i] = pRefKF->mvKeysUn[i].angle;
            if (!valid[i]) continue;
            cv::Mat P = pMP->GetWorldPos();
            for (int k = 0; k < 3; ++k) xw[3 * i + k] = P.at<float>(k);
            nobs[i] = pMP->Observations();
        }
    }
    const std::vector<int32_t> knode = feature_nodes(pRefKF->mFeatVec, nq);
    std::vector<int32_t> fnode;
    if (!bTransform) {
        fnode = feature_nodes(F.mFeatVec, N);
        if (fnode.empty()) fnode.push_back(-1);     // an empty frame still passes "mBowVec is filled": not NULL
    }
    cv::Mat kfDesc = pRefKF->mDescriptors.isContinuous() ? pRefKF->mDescriptors : pRefKF->mDescriptors.clone();
    cv::Mat curDesc = F.mDescriptors.isContinuous() ? F.mDescriptors : F.mDescriptors.clone();
    coeb_ref_keyframe kf{{nq, valid.data(), kfDesc.empty() ? nullptr : kfDesc.ptr<uint8_t>(0), knode.data(), kang.data()},
                         xw.data(), nobs.data()};
    coeb_curframe cur{N, reinterpret_cast<const coeb_keypoint*>(F.mvKeysUn.data()),
                      curDesc.empty() ? nullptr : curDesc.ptr<uint8_t>(0), F.mvuRight.data()};
    const coeb_camera cam = frame_camera(F);
    float T[16];
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) T[4 * r + k] = lastTcw.template at<float>(r, k);
    std::vector<int32_t> word((size_t)N), node((size_t)N), match((size_t)N), disc((size_t)N);
    std::vector<double> weight((size_t)N);
    int nmatchesBoW = 0, ninl = 0, nmatches = 0, nmatchesMap = 0;
    const int rc = coeb_track_reference_keyframe(ctx, &cam, &cur, bTransform ? nullptr : fnode.data(), levelsup, &kf, T,
                                                 nnratio, bCheckOrientation ? 1 : 0, 15, word.data(), node.data(),
                                                 weight.data(), match.data(), disc.data(), &nmatchesBoW, &ninl, &nmatches,
                                                 &nmatchesMap);
    if (rc != COEB_OK) throw std::runtime_error(coeb_last_error(ctx));
    if (bTransform) {                               // mCurrentFrame.ComputeBoW() (:826)
        std::vector<int32_t> bw((size_t)N);
        std::vector<double> bv((size_t)N);
        int nw = 0;
        if (coeb_bow_vector(word.data(), weight.data(), node.data(), N, 1, bw.data(), bv.data(), N, &nw) != COEB_OK)
            throw std::runtime_error("coeb_bow_vector failed");
        for (int j = 0; j < nw; ++j) F.mBowVec.addWeight(bw[j], bv[j]);
        for (int i = 0; i < N; ++i)
            if (node[i] >= 0) F.mFeatVec.addFeature(node[i], (unsigned int)i);
    }
    if (pnMatchesMap) *pnMatchesMap = nmatchesMap;
    if (nmatchesBoW < 15) return false;             // :835
    cv::Mat Tcw(4, 4, CV_32F);
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) Tcw.at<float>(r, k) = T[4 * r + k];
    F.SetPose(Tcw);
    for (int i = 0; i < N; ++i) {
        F.mvpMapPoints[i] = match[i] >= 0 ? vpMapPointsKF[match[i]] : static_cast<MapPointT*>(nullptr);
        if (match[i] >= 0 || disc[i] >= 0) F.mvbOutlier[i] = false;
        if (disc[i] < 0) continue;
        MapPointT* pMP = vpMapPointsKF[disc[i]];    // :851-856
        pMP->mbTrackInView = false;
        pMP->mnLastFrameSeen = F.mnId;
    }
    return nmatchesMap >= 10;
}

// Tracking::TrackWithMotionModel after UpdateLastFrame has set mLastFrame's pose (:870-873 stay with
// the caller: they read mlRelativeFramePoses).  bCreateVO is UpdateLastFrame's condition to go on
// (:875 negated: mnLastKeyFrameId != mLastFrame.mnId && mSensor != MONOCULAR && mbOnlyTracking);
// newTemporalPoint(x3D, i) returns `new MapPoint(x3D, mpMap, &mLastFrame, i)`.  *pbVO receives mbVO
// in localisation mode and is left alone otherwise; *pnMatchesMap (when given) receives nmatchesMap.
template <class FrameT, class MatT, class ListT, class NewPointF>
inline bool TrackWithMotionModel(FrameT& F, FrameT& LastFrame, const MatT& mVelocity, float th, bool bMono,
                                 bool bOnlyTracking, bool bCreateVO, float thDepth, NewPointF newTemporalPoint,
                                 ListT& mlpTemporalPoints, bool* pbVO, bool bCheckOrientation = true,
                                 int* pnMatchesMap = nullptr, coeb_ctx* ctx = nullptr)
{
    typedef typename std::remove_pointer<typename std::decay<decltype(LastFrame.mvpMapPoints[0])>::type>::type MapPointT;
    if (!ctx) ctx = matcher_ctx(F.mnScaleLevels, F.mfScaleFactor);
    const int N = F.N, nl = LastFrame.N;
    std::vector<uint8_t> has(nl), outl(nl), mpdesc((size_t)nl * 32);
    std::vector<float> xw((size_t)nl * 3);
    std::vector<int32_t> nobs(nl);
    {
        std::unique_lock<std::mutex> lock(MapPointT::mGlobalMutex);
        for (int i = 0; i < nl; ++i) {
            MapPointT* pMP = LastFrame.mvpMapPoints[i];
            has[i] = pMP != nullptr;
            outl[i] = LastFrame.mvbOutlier[i];
            if (!pMP) continue;
            cv::Mat P = pMP->GetWorldPos();
            for (int k = 0; k < 3; ++k) xw[3 * i + k] = P.at<float>(k);
            cv::Mat d = pMP->GetDescriptor();
            std::memcpy(&mpdesc[32 * (size_t)i], d.ptr<uint8_t>(0), 32);
            nobs[i] = pMP->Observations();
        }
    }
    coeb_lastframe last{nl, has.data(), outl.data(), xw.data(), mpdesc.data(), nobs.data(),
                        reinterpret_cast<const coeb_keypoint*>(LastFrame.mvKeysUn.data())};
    cv::Mat curDesc = F.mDescriptors.isContinuous() ? F.mDescriptors : F.mDescriptors.clone();
    cv::Mat lastDesc = LastFrame.mDescriptors.isContinuous() ? LastFrame.mDescriptors : LastFrame.mDescriptors.clone();
    coeb_curframe cur{N, reinterpret_cast<const coeb_keypoint*>(F.mvKeysUn.data()),
                      curDesc.empty() ? nullptr : curDesc.ptr<uint8_t>(0), F.mvuRight.data()};
    std::vector<uint8_t> created(nl);
    std::vector<float> cpos((size_t)nl * 3);
    coeb_vo_points vo{LastFrame.mvDepth.data(), lastDesc.empty() ? nullptr : lastDesc.ptr<uint8_t>(0), thDepth,
                      created.data(), cpos.data()};
    const coeb_camera cam = frame_camera(F);
    F.SetPose(mVelocity * LastFrame.mTcw);          // :941
    float T[16], Tl[16];
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) {
            T[4 * r + k] = F.mTcw.template at<float>(r, k);
            Tl[4 * r + k] = LastFrame.mTcw.template at<float>(r, k);
        }
    std::vector<int32_t> match((size_t)N), disc((size_t)N);
    int nmatchesSearch = 0, ninl = 0, nmatches = 0, nmatchesMap = 0;
    const int rc = coeb_track_motion_model(ctx, &cam, &cur, &last, bCreateVO ? &vo : nullptr, Tl, T, th, bMono ? 1 : 0,
                                           bCheckOrientation ? 1 : 0, 20, match.data(), disc.data(), nullptr,
                                           &nmatchesSearch, &ninl, &nmatches, &nmatchesMap);
    if (rc != COEB_OK) throw std::runtime_error(coeb_last_error(ctx));
    if (bCreateVO) {                                // :913-922, in the order of the depth sort
        std::vector<std::pair<float, int>> vDepthIdx;
        for (int i = 0; i < nl; ++i)
            if (created[i]) vDepthIdx.push_back(std::make_pair(LastFrame.mvDepth[i], i));
        std::sort(vDepthIdx.begin(), vDepthIdx.end());
        for (size_t j = 0; j < vDepthIdx.size(); ++j) {
            const int i = vDepthIdx[j].second;
            cv::Mat x3D(3, 1, CV_32F);
            for (int k = 0; k < 3; ++k) x3D.at<float>(k) = cpos[3 * (size_t)i + k];
            MapPointT* pNewMP = newTemporalPoint(x3D, i);
            LastFrame.mvpMapPoints[i] = pNewMP;
            mlpTemporalPoints.push_back(pNewMP);
        }
    }
    // :943, :956 and the search's assignments less the discards
    for (int i = 0; i < N; ++i)
        F.mvpMapPoints[i] = match[i] >= 0 ? LastFrame.mvpMapPoints[match[i]] : static_cast<MapPointT*>(nullptr);
    if (pnMatchesMap) *pnMatchesMap = nmatchesMap;
    if (nmatchesSearch < 20) return false;          // :960
    cv::Mat Tcw(4, 4, CV_32F);
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) Tcw.at<float>(r, k) = T[4 * r + k];
    F.SetPose(Tcw);
    for (int i = 0; i < N; ++i) {
        if (match[i] >= 0 || disc[i] >= 0) F.mvbOutlier[i] = false;    // Optimizer.cc:302, Tracking.cc:977
        if (disc[i] < 0) continue;
        MapPointT* pMP = LastFrame.mvpMapPoints[disc[i]];              // :974-979
        pMP->mbTrackInView = false;
        pMP->mnLastFrameSeen = F.mnId;
    }
    if (bOnlyTracking) {                            // :987-991
        if (pbVO) *pbVO = nmatchesMap < 10;
        return nmatches > 20;
    }
    return nmatchesMap >= 10;
}

}  // namespace coeb

#endif
