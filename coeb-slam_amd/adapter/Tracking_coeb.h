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
 *
 * Tracking::Relocalization (src/Tracking.cc:1417-1580) keeps its front half (ComputeBoW,
 * DetectRelocalizationCandidates, the SearchByBoW loop and the PnP solvers: KeyFrameDatabase_coeb.h,
 * ORBmatcher_coeb.h and the integrator's own solver) and its while loop (:1477-1568) becomes
 *
 *     bool bMatch = coeb::Relocalization(mCurrentFrame, vpCandidateKFs, vpPnPsolvers, vvpMapPointMatches,
 *                                        vbDiscarded, nCandidates);
 *
 * one library call with one synchronisation per round of the loop (coeb_reloc_refine) instead of up to
 * five per candidate.  Per round, in the reference's order: every candidate that is not discarded runs
 * pSolver->iterate(5, bNoMore, vbInliers, nInliers) and bNoMore discards it (:1490-1497); the
 * candidates that returned a pose are snapshot (the KeyFrame's GetMapPointMatches(): valid = pMP &&
 * !isBad(), GetWorldPos(), GetDescriptor(), mfMaxDistance / mfMinDistance, mvKeysUn[i].angle; the
 * KeyFrame index of every vvpMapPointMatches[i][j]) and refined side by side; the first with nGood >= 50
 * is the one the reference's loop breaks on, and its mvpMapPoints, mvbOutlier (where an optimisation
 * saw a point) and pose go into the frame.  With no such candidate the frame gets the state of the
 * last one, as the reference's sequential loop leaves it, and the next round runs.
 */
#ifndef COEB_ADAPTER_TRACKING_H
#define COEB_ADAPTER_TRACKING_H

#include <algorithm>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <type_traits>
#include <unordered_map>
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

// a 4x4 CV_32F pose as the C-ABI's row-major float[16], and back
template <class MatT>
inline void pose_to_array(const MatT& M, float T[16])
{
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) T[4 * r + k] = M.template at<float>(r, k);
}
inline cv::Mat pose_to_mat(const float T[16])
{
    cv::Mat M(4, 4, CV_32F);
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) M.at<float>(r, k) = T[4 * r + k];
    return M;
}

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
    pose_to_array(F.mTcw, T);
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
    if (nInitial >= 3) F.SetPose(pose_to_mat(T));
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
    detail::pose_to_array(lastTcw, T);
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
    F.SetPose(detail::pose_to_mat(T));
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
    detail::pose_to_array(F.mTcw, T);
    detail::pose_to_array(LastFrame.mTcw, Tl);
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
    F.SetPose(detail::pose_to_mat(T));
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

// One PnP hypothesis as Tracking::Relocalization holds it behind vpPnPsolvers[i]->iterate (:1490)
template <class KeyFrameT, class MapPointT>
struct RelocHypothesis {
    KeyFrameT* pKF;                                         // vpCandidateKFs[i]
    const std::vector<MapPointT*>* vpMapPointMatches;       // &vvpMapPointMatches[i]
    std::vector<bool> vbInliers;
    cv::Mat Tcw;
};

// Tracking.cc:1502-1565 for up to COEB_RELOC_MAX_HYP hypotheses of one round in one call.  Returns the
// index of the first hypothesis with nGood >= 50 (the one the reference breaks on), or -1; the frame
// gets that hypothesis' mvpMapPoints, mvbOutlier and pose, or with -1 those of the last one (what the
// reference's loop leaves behind it).  pnGood (when given) receives every hypothesis' nGood.
template <class FrameT, class KeyFrameT, class MapPointT>
inline int RelocalizationRefine(FrameT& F, const std::vector<RelocHypothesis<KeyFrameT, MapPointT>>& hyps,
                                bool bCheckOrientation = true, std::vector<int>* pnGood = nullptr, coeb_ctx* ctx = nullptr)
{
    const int H = (int)hyps.size(), N = F.N;
    if (H < 1 || H > COEB_RELOC_MAX_HYP) throw std::runtime_error("coeb::RelocalizationRefine: 1..COEB_RELOC_MAX_HYP hypotheses");
    if (!ctx) ctx = matcher_ctx(F.mnScaleLevels, F.mfScaleFactor);
    struct Snap {
        std::vector<MapPointT*> pts;                        // by KeyFrame index; past vpMPs: matched points the KeyFrame lost
        std::vector<uint8_t> valid, desc, inl;
        std::vector<float> xw, maxd, mind, ang;
        std::vector<int32_t> match;
    };
    std::vector<Snap> snap((size_t)H);
    std::vector<coeb_reloc_hypothesis> hy((size_t)H);
    for (int h = 0; h < H; ++h) {
        Snap& s = snap[h];
        KeyFrameT* pKF = hyps[h].pKF;
        s.pts = pKF->GetMapPointMatches();
        const int nkf = (int)s.pts.size();
        std::unordered_map<MapPointT*, int> index;
        for (int i = nkf - 1; i >= 0; --i)
            if (s.pts[i]) index[s.pts[i]] = i;
        s.match.assign((size_t)N, -1);
        s.inl.assign((size_t)N, 0);
        const std::vector<MapPointT*>& vpM = *hyps[h].vpMapPointMatches;
        for (int j = 0; j < N; ++j) {
            MapPointT* pMP = j < (int)vpM.size() ? vpM[j] : static_cast<MapPointT*>(nullptr);
            if (!pMP) continue;                             // an inlier always has a point (PnPsolver.cc keeps matched keypoints only)
            auto it = index.find(pMP);
            if (it == index.end()) {                        // no longer in the KeyFrame: an extra slot no search can reach
                it = index.emplace(pMP, (int)s.pts.size()).first;
                s.pts.push_back(pMP);
            }
            s.match[j] = it->second;
            s.inl[j] = j < (int)hyps[h].vbInliers.size() && hyps[h].vbInliers[j];
        }
        const int nq = (int)s.pts.size();
        s.valid.assign(nq, 0); s.desc.assign((size_t)nq * 32, 0);
        s.xw.assign((size_t)nq * 3, 0.f); s.maxd.assign(nq, 0.f); s.mind.assign(nq, 0.f); s.ang.assign(nq, 0.f);
        {
            std::unique_lock<std::mutex> lock(MapPointT::mGlobalMutex);
            for (int i = 0; i < nq; ++i) {
                MapPointT* pMP = s.pts[i];
                if (!pMP) continue;
                cv::Mat P = pMP->GetWorldPos();             // read for bad points too: the optimiser does not ask (Optimizer.cc:276)
                for (int k = 0; k < 3; ++k) s.xw[3 * (size_t)i + k] = P.at<float>(k);
                s.valid[i] = i < nkf && !pMP->isBad();
                if (!s.valid[i]) continue;
                cv::Mat d = pMP->GetDescriptor();
                std::memcpy(&s.desc[32 * (size_t)i], d.ptr<uint8_t>(0), 32);
                s.maxd[i] = pMP->GetMaxDistance();
                s.mind[i] = pMP->GetMinDistance();
                s.ang[i] = pKF->mvKeysUn[i].angle;
            }
        }
        hy[h].kf = coeb_keyframe_points{nq, s.valid.data(), s.xw.data(), s.desc.data(), s.maxd.data(), s.mind.data(), s.ang.data()};
        hy[h].match = s.match.data();
        hy[h].inlier = s.inl.data();
        detail::pose_to_array(hyps[h].Tcw, hy[h].Tcw);
    }
    cv::Mat curDesc = F.mDescriptors.isContinuous() ? F.mDescriptors : F.mDescriptors.clone();
    coeb_curframe cur{N, reinterpret_cast<const coeb_keypoint*>(F.mvKeysUn.data()),
                      curDesc.empty() ? nullptr : curDesc.ptr<uint8_t>(0), F.mvuRight.data()};
    const coeb_camera cam = frame_camera(F);
    std::vector<int32_t> match((size_t)H * N), ngood(H), nadd1(H), nadd2(H), stage(H);
    std::vector<uint8_t> outl((size_t)H * N, 2);            // 2: no optimisation saw a point there
    int first = -1;
    const int rc = coeb_reloc_refine(ctx, &cam, &cur, hy.data(), H, 10.f, 100, 3.f, 64, bCheckOrientation ? 1 : 0, 10, 30, 50,
                                     match.data(), outl.data(), ngood.data(), nadd1.data(), nadd2.data(), stage.data(), &first);
    if (rc != COEB_OK) throw std::runtime_error(coeb_last_error(ctx));
    if (pnGood) pnGood->assign(ngood.begin(), ngood.end());
    const int w = first >= 0 ? first : H - 1;
    int nInliers = 0;
    for (int j = 0; j < N; ++j) {
        const int m = match[(size_t)w * N + j];
        F.mvpMapPoints[j] = m >= 0 ? snap[w].pts[m] : static_cast<MapPointT*>(nullptr);
        if (outl[(size_t)w * N + j] != 2) F.mvbOutlier[j] = outl[(size_t)w * N + j] != 0;
        nInliers += snap[w].inl[j];
    }
    // Tcw.copyTo(mCurrentFrame.mTcw) (:1502), then PoseOptimization's SetPose with at least 3 edges (Optimizer.cc:361-362, 446-448)
    F.mTcw = hyps[w].Tcw.clone();
    if (nInliers >= 3) F.SetPose(detail::pose_to_mat(hy[w].Tcw));
    return first;
}

// The while loop of Tracking::Relocalization (:1477-1568) over any solver type with the reference's
// `cv::Mat iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers)`.  A round
// collects the hypotheses of every candidate that is not discarded, refines them in one call (several
// when a round has more than COEB_RELOC_MAX_HYP) and stops at the first with nGood >= 50.  rand() is
// consumed in the reference's order up to the winning candidate; the candidates behind it in the
// winning round have iterated as well, which the reference's `break` spares them: their solvers are
// not used again.  vbDiscarded and nCandidates are updated as the reference updates them.
template <class FrameT, class KeyFrameT, class MapPointT, class Solver>
inline bool Relocalization(FrameT& F, const std::vector<KeyFrameT*>& vpCandidateKFs, const std::vector<Solver*>& vpPnPsolvers,
                           const std::vector<std::vector<MapPointT*>>& vvpMapPointMatches, std::vector<bool>& vbDiscarded,
                           int& nCandidates, bool bCheckOrientation = true, coeb_ctx* ctx = nullptr)
{
    const int nKFs = (int)vpCandidateKFs.size();
    while (nCandidates > 0) {
        std::vector<RelocHypothesis<KeyFrameT, MapPointT>> round;
        for (int i = 0; i < nKFs; ++i) {
            if (vbDiscarded[i]) continue;
            std::vector<bool> vbInliers;                    // Perform 5 Ransac Iterations (:1484-1490)
            int nInliers = 0;
            bool bNoMore = false;
            cv::Mat Tcw = vpPnPsolvers[i]->iterate(5, bNoMore, vbInliers, nInliers);
            if (bNoMore) {                                  // :1493-1497
                vbDiscarded[i] = true;
                nCandidates--;
            }
            if (!Tcw.empty()) round.push_back(RelocHypothesis<KeyFrameT, MapPointT>{vpCandidateKFs[i], &vvpMapPointMatches[i], vbInliers, Tcw.clone()});
        }
        for (size_t at = 0; at < round.size(); at += COEB_RELOC_MAX_HYP) {
            const size_t end = std::min(round.size(), at + (size_t)COEB_RELOC_MAX_HYP);
            const std::vector<RelocHypothesis<KeyFrameT, MapPointT>> part(round.begin() + at, round.begin() + end);
            if (RelocalizationRefine(F, part, bCheckOrientation, static_cast<std::vector<int>*>(nullptr), ctx) >= 0) return true;   // :1561-1565
        }
    }
    return false;
}

}  // namespace coeb

#endif
