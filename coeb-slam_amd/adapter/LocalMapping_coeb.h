/*
 * LocalMapping_coeb.h -- MI355X body for the matching half of LocalMapping::CreateNewMapPoints
 *   ORBmatcher::SearchForTriangulation per neighbour   src/LocalMapping.cc:255-270,
 *                                                       src/ORBmatcher.cc:657-824
 * as one call for all neighbours of the new keyframe.
 *
 * coeb::KeyFrameStore<KeyFrame> is a coeb_kfdb used purely as a device cache of what the search
 * reads of a keyframe and what never changes after KeyFrame::ComputeBoW: descriptors, feature-vector
 * nodes, angles (coeb_kfdb_add with an empty BowVector) and mvKeysUn / mvuRight
 * (coeb_kfdb_set_geometry).  LocalMapping keeps one as a member:
 *
 *     void LocalMapping::ProcessNewKeyFrame() { ... mpCurrentKeyFrame->ComputeBoW(); mCoebStore.add(mpCurrentKeyFrame); ... }
 *     void KeyFrame::SetBadFlag()             { ... mpLocalMapper's store .erase(this) ... }
 *
 * It is deliberately NOT KeyFrameDatabase::mCoeb (KeyFrameDatabase_coeb.h): the reference adds a
 * keyframe to its database only in LoopClosing (LoopClosing.cc:117,147,216), and a keyframe that
 * entered earlier would be seen by relocalisation earlier than in the reference.  The store owns its
 * context (the keyframes' pyramid: mnScaleLevels, mfScaleFactor) and holds its mutex around every
 * call: SetBadFlag runs on other threads, and a context is not reentrant.
 *
 * coeb::SearchForTriangulationNeighbors snapshots GetMapPoint(i) != NULL of every keyframe,
 * computes each neighbour's epipole with the reference's own expressions (:664-670; F12 comes from
 * the caller's ComputeF12) and fills one vMatchedPairs per neighbour.  A neighbour that is not in
 * the store gets no pairs.  The triangulation stays the caller's.  The line and epipole tests use
 * the fused forms seen in the reference binary; parity against it is UNPINNED.
 */
#ifndef COEB_ADAPTER_LOCALMAPPING_H
#define COEB_ADAPTER_LOCALMAPPING_H

#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "ORBmatcher_coeb.h"

namespace coeb
{

template <class KeyFrameT>
class KeyFrameStore
{
public:
    KeyFrameStore(int nlevels, float scale_factor, int max_features = 4095, int initial_slots = 64)
    {
        coeb_orb_params p{1000, scale_factor, nlevels, 20, 7};
        mCtx = coeb_create(&p, 0, 640, 480, 1);
        if (!mCtx) throw std::runtime_error(coeb_last_error(nullptr));
        if (coeb_kfdb_create(mCtx, max_features, initial_slots, &mDb) != COEB_OK) {
            const std::string msg = coeb_last_error(mCtx);
            coeb_destroy(mCtx);
            throw std::runtime_error(msg);
        }
    }
    ~KeyFrameStore()
    {
        coeb_kfdb_destroy(mDb);
        coeb_destroy(mCtx);
    }
    KeyFrameStore(const KeyFrameStore&) = delete;
    KeyFrameStore& operator=(const KeyFrameStore&) = delete;

    // after pKF->ComputeBoW(); a keyframe already stored is left alone
    void add(KeyFrameT* pKF)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        if (mSlot.count(pKF)) return;
        const int n = (int)pKF->mvKeysUn.size();
        std::vector<float> ang((size_t)n);
        std::vector<coeb_keypoint> keys((size_t)n);
        for (int i = 0; i < n; ++i) {
            const cv::KeyPoint& kp = pKF->mvKeysUn[i];
            ang[i] = kp.angle;
            keys[i] = coeb_keypoint{kp.pt.x, kp.pt.y, kp.size, kp.angle, kp.response, kp.octave, kp.class_id};
        }
        const std::vector<int32_t> node = feature_nodes(pKF->mFeatVec, n);
        cv::Mat desc = pKF->mDescriptors.isContinuous() ? pKF->mDescriptors : pKF->mDescriptors.clone();
        coeb_kfdb_keyframe kf{n, desc.empty() ? nullptr : desc.ptr<uint8_t>(0), node.data(), ang.data(), nullptr, nullptr, 0};
        int slot = -1;
        if (coeb_kfdb_add(mDb, &kf, &slot) != COEB_OK) throw std::runtime_error(coeb_last_error(mCtx));
        if (coeb_kfdb_set_geometry(mDb, slot, keys.data(), pKF->mvuRight.data()) != COEB_OK) {
            const std::string msg = coeb_last_error(mCtx);
            coeb_kfdb_erase(mDb, slot);
            throw std::runtime_error(msg);
        }
        mSlot[pKF] = slot;
    }

    void erase(KeyFrameT* pKF)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        typename std::map<KeyFrameT*, int>::iterator it = mSlot.find(pKF);
        if (it == mSlot.end()) return;
        if (coeb_kfdb_erase(mDb, it->second) != COEB_OK) throw std::runtime_error(coeb_last_error(mCtx));
        mSlot.erase(it);
    }

    size_t size()
    {
        std::unique_lock<std::mutex> lock(mMutex);
        return mSlot.size();
    }

    // for SearchForTriangulationNeighbors; slot() is read under mutex()
    std::mutex& mutex() { return mMutex; }
    coeb_kfdb* handle() { return mDb; }
    coeb_ctx* ctx() { return mCtx; }
    int slot(KeyFrameT* pKF) const
    {
        typename std::map<KeyFrameT*, int>::const_iterator it = mSlot.find(pKF);
        return it == mSlot.end() ? -1 : it->second;
    }

private:
    coeb_ctx* mCtx = nullptr;
    coeb_kfdb* mDb = nullptr;
    std::mutex mMutex;
    std::map<KeyFrameT*, int> mSlot;
};

// GetMapPoint(i) != NULL for i < N
template <class KeyFrameT>
inline std::vector<uint8_t> has_map_point(KeyFrameT* pKF)
{
    const size_t n = pKF->mvKeysUn.size();
    std::vector<uint8_t> has(n);
    for (size_t i = 0; i < n; ++i) has[i] = pKF->GetMapPoint(i) != nullptr;
    return has;
}

// ORBmatcher(_, bCheckOrientation).SearchForTriangulation(pKF1, vpKF2[j], vF12[j], vvMatchedPairs[j], bOnlyStereo)
// for every j in one call per 32 neighbours; returns the sum of the matches.
template <class KeyFrameT>
inline int SearchForTriangulationNeighbors(KeyFrameStore<KeyFrameT>& store, KeyFrameT* pKF1,
                                           const std::vector<KeyFrameT*>& vpKF2, const std::vector<cv::Mat>& vF12,
                                           std::vector<std::vector<std::pair<size_t, size_t> > >& vvMatchedPairs,
                                           bool bOnlyStereo, bool bCheckOrientation = false)
{
    const size_t nKFs = vpKF2.size();
    if (vF12.size() != nKFs) throw std::invalid_argument("SearchForTriangulationNeighbors: one F12 per neighbour");
    vvMatchedPairs.assign(nKFs, std::vector<std::pair<size_t, size_t> >());
    std::unique_lock<std::mutex> lock(store.mutex());
    const int slot1 = store.slot(pKF1);
    if (slot1 < 0) throw std::runtime_error("SearchForTriangulationNeighbors: pKF1 is not in the store");
    const std::vector<uint8_t> has1 = has_map_point(pKF1);
    const int n1 = (int)has1.size();
    std::vector<size_t> which;
    std::vector<int32_t> slots;
    std::vector<std::vector<uint8_t> > has2;
    std::vector<float> F, epi;
    for (size_t j = 0; j < nKFs; ++j) {
        KeyFrameT* pKF2 = vpKF2[j];
        const int slot2 = store.slot(pKF2);
        if (slot2 < 0) continue;
        which.push_back(j);
        slots.push_back(slot2);
        has2.push_back(has_map_point(pKF2));
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) F.push_back(vF12[j].template at<float>(r, c));
        // Compute epipole in second image (:664-670)
        cv::Mat Cw = pKF1->GetCameraCenter();
        cv::Mat R2w = pKF2->GetRotation();
        cv::Mat t2w = pKF2->GetTranslation();
        cv::Mat C2 = R2w * Cw + t2w;
        const float invz = 1.0f / C2.template at<float>(2);
        const float ex = pKF2->fx * C2.template at<float>(0) * invz + pKF2->cx;
        const float ey = pKF2->fy * C2.template at<float>(1) * invz + pKF2->cy;
        epi.push_back(ex);
        epi.push_back(ey);
    }
    int total = 0;
    for (size_t done = 0; done < which.size(); done += COEB_TRI_MAX_NEIGHBOURS) {
        const int nnb = (int)std::min<size_t>(COEB_TRI_MAX_NEIGHBOURS, which.size() - done);
        std::vector<const uint8_t*> hptr((size_t)nnb);
        for (int j = 0; j < nnb; ++j) hptr[j] = has2[done + j].empty() ? nullptr : has2[done + j].data();
        std::vector<int32_t> match((size_t)nnb * n1 + 1), nm((size_t)nnb);
        if (coeb_kfdb_search_triangulation(store.handle(), slot1, has1.empty() ? nullptr : has1.data(), slots.data() + done,
                                           nnb, hptr.data(), F.data() + done * 9, epi.data() + done * 2, bOnlyStereo ? 1 : 0,
                                           bCheckOrientation ? 1 : 0, match.data(), nm.data()) != COEB_OK)
            throw std::runtime_error(coeb_last_error(store.ctx()));
        for (int j = 0; j < nnb; ++j) {
            std::vector<std::pair<size_t, size_t> >& pairs = vvMatchedPairs[which[done + j]];
            pairs.reserve((size_t)nm[j]);
            for (int i = 0; i < n1; ++i) {
                const int32_t m = match[(size_t)j * n1 + i];
                if (m >= 0) pairs.push_back(std::make_pair((size_t)i, (size_t)m));
            }
            total += nm[j];
        }
    }
    return total;
}

}  // namespace coeb

#endif
