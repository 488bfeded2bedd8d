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
 * the store gets no pairs.  The line and epipole tests use the fused forms seen in the reference
 * binary; parity against it is UNPINNED.
 *
 * coeb::CreateNewMapPointsNeighbors goes on from there (src/LocalMapping.cc:271-433): it
 * snapshots the views (pose, camera) and masks of all keyframes once and returns, per neighbour, the
 * pairs that reach `new MapPoint` with their x3D, in the reference's order.  KeyFrameStore::add uploads
 * mvKeys / mvDepth for it (coeb_kfdb_set_stereo) when the keyframe type has them.  The triangulated point
 * is a canonical float32 Jacobi's, not cv::SVD's bit for bit; parity is UNPINNED.  A MapPoint that
 * another thread adds to one of the keyframes after the snapshot is not seen, as in
 * SearchForTriangulationNeighbors.
 *
 * The two loops of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:455-535):
 *   coeb::FuseSearch   the snapshot of a point list (under MapPoint::mGlobalMutex) and one
 *                      coeb_kfdb_fuse_search over any number of (keyframe, skip) jobs on it;
 *   coeb::Fuse         ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:826-976): one job, then
 *                      the reference's loop replayed on the host with the search results;
 *   coeb::FuseTargets  Fuse(vpTargetKFs[j], vpMapPointMatches) for j in order: one call for all targets,
 *                      the replay target by target, and a further call whenever a Replace changed the
 *                      descriptor of a listed point before a later target looks at it.
 * The search (bestIdx, bestDist) reads only the point's position, normal, distances and descriptor, the
 * keyframe's constant features and pose, and the camera; the skips (!pMP, isBad(), IsInKeyFrame) and the
 * action (GetMapPoint(bestIdx), Observations(), Replace / AddObservation) are evaluated by the replay at
 * the moment the reference evaluates them.  MapPoint::Replace ends in ComputeDistinctiveDescriptors on the
 * survivor, so a survivor's descriptor can change.  Within one Fuse call that cannot matter: a survivor
 * is an earlier point of the list or a point of the keyframe, and IsInKeyFrame skips it.  Across targets
 * it can, which FuseTargets detects by comparing GetDescriptor() of the survivor with the uploaded bytes.
 * A keyframe that was never added to the store fuses nothing (as s3l's neighbour without pairs); a
 * keyframe that is in the store always takes the device path.
 */
#ifndef COEB_ADAPTER_LOCALMAPPING_H
#define COEB_ADAPTER_LOCALMAPPING_H

#include <cstring>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "ORBmatcher_coeb.h"

namespace coeb
{

// mvKeys / mvDepth of a keyframe type that has them (the reference's KeyFrame), for coeb_kfdb_set_stereo;
// false for a stand-in without them, whose slots then refuse coeb_kfdb_create_new_map_points
template <class KeyFrameT>
inline auto stereo_arrays(KeyFrameT* pKF, std::vector<float>& xy, std::vector<float>& depth, int)
    -> decltype(pKF->mvKeys.size(), pKF->mvDepth.size(), bool())
{
    const size_t n = pKF->mvKeys.size();
    xy.resize(2 * n);
    for (size_t i = 0; i < n; ++i) {
        xy[2 * i] = pKF->mvKeys[i].pt.x;
        xy[2 * i + 1] = pKF->mvKeys[i].pt.y;
    }
    depth.assign(pKF->mvDepth.begin(), pKF->mvDepth.end());
    return true;
}
template <class KeyFrameT>
inline bool stereo_arrays(KeyFrameT*, std::vector<float>&, std::vector<float>&, long)
{
    return false;
}

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
        std::vector<float> xy, depth;
        const bool stereo = stereo_arrays(pKF, xy, depth, 0);
        if (coeb_kfdb_set_geometry(mDb, slot, keys.data(), pKF->mvuRight.data()) != COEB_OK ||
            (stereo && ((int)depth.size() != n || coeb_kfdb_set_stereo(mDb, slot, xy.data(), depth.data()) != COEB_OK))) {
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

// One pair that reaches `new MapPoint` (LocalMapping.cc:435): the features and x3D.
struct NewMapPointPair {
    size_t idx1, idx2;
    float x3D[3];
};

template <class KeyFrameT>
inline coeb_kf_view kf_view(KeyFrameT* pKF)
{
    coeb_kf_view v;
    const cv::Mat R = pKF->GetRotation(), t = pKF->GetTranslation(), O = pKF->GetCameraCenter();
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) v.Rcw[3 * r + c] = R.template at<float>(r, c);
        v.tcw[r] = t.template at<float>(r);
        v.Ow[r] = O.template at<float>(r);
    }
    v.fx = pKF->fx; v.fy = pKF->fy; v.cx = pKF->cx; v.cy = pKF->cy;
    v.invfx = pKF->invfx; v.invfy = pKF->invfy; v.mb = pKF->mb; v.mbf = pKF->mbf;
    return v;
}

// The loop of LocalMapping::CreateNewMapPoints from SearchForTriangulation to the scale test (:269-433) for
// every neighbour vpKF2[j] with vF12[j], in one call per 32 neighbours: vvNewPoints[j] holds, ascending in
// idx1, the pairs of neighbour j for which the reference reaches `new MapPoint`, in its order -- a feature of
// pKF1 that an earlier neighbour gave a MapPoint is skipped by the later ones.  Views and masks are read once,
// before the first call.  A neighbour that is not in the store gets no pairs.  Returns the number of pairs.
template <class KeyFrameT>
inline int CreateNewMapPointsNeighbors(KeyFrameStore<KeyFrameT>& store, KeyFrameT* pKF1,
                                       const std::vector<KeyFrameT*>& vpKF2, const std::vector<cv::Mat>& vF12,
                                       std::vector<std::vector<NewMapPointPair> >& vvNewPoints)
{
    const size_t nKFs = vpKF2.size();
    if (vF12.size() != nKFs) throw std::invalid_argument("CreateNewMapPointsNeighbors: one F12 per neighbour");
    vvNewPoints.assign(nKFs, std::vector<NewMapPointPair>());
    std::unique_lock<std::mutex> lock(store.mutex());
    const int slot1 = store.slot(pKF1);
    if (slot1 < 0) throw std::runtime_error("CreateNewMapPointsNeighbors: pKF1 is not in the store");
    std::vector<uint8_t> has1 = has_map_point(pKF1);
    const int n1 = (int)has1.size();
    const coeb_kf_view view1 = kf_view(pKF1);
    std::vector<size_t> which;
    std::vector<int32_t> slots;
    std::vector<std::vector<uint8_t> > has2;
    std::vector<coeb_kf_view> views;
    std::vector<float> F, epi;
    for (size_t j = 0; j < nKFs; ++j) {
        KeyFrameT* pKF2 = vpKF2[j];
        const int slot2 = store.slot(pKF2);
        if (slot2 < 0) continue;
        which.push_back(j);
        slots.push_back(slot2);
        has2.push_back(has_map_point(pKF2));
        views.push_back(kf_view(pKF2));
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) F.push_back(vF12[j].template at<float>(r, c));
        // Compute epipole in second image (ORBmatcher.cc:664-670)
        cv::Mat Cw = pKF1->GetCameraCenter();
        cv::Mat R2w = pKF2->GetRotation();
        cv::Mat t2w = pKF2->GetTranslation();
        cv::Mat C2 = R2w * Cw + t2w;
        const float invz = 1.0f / C2.template at<float>(2);
        epi.push_back(pKF2->fx * C2.template at<float>(0) * invz + pKF2->cx);
        epi.push_back(pKF2->fy * C2.template at<float>(1) * invz + pKF2->cy);
    }
    int total = 0;
    for (size_t done = 0; done < which.size(); done += COEB_TRI_MAX_NEIGHBOURS) {
        const int nnb = (int)std::min<size_t>(COEB_TRI_MAX_NEIGHBOURS, which.size() - done);
        std::vector<const uint8_t*> hptr((size_t)nnb);
        for (int j = 0; j < nnb; ++j) hptr[j] = has2[done + j].empty() ? nullptr : has2[done + j].data();
        const size_t rows = (size_t)nnb * n1;
        std::vector<int32_t> match(rows + 1), first((size_t)n1 + 1), nm((size_t)nnb);
        std::vector<int8_t> status(rows + 1);
        std::vector<float> x3d(3 * rows + 1);
        if (coeb_kfdb_create_new_map_points(store.handle(), slot1, &view1, has1.empty() ? nullptr : has1.data(),
                                            slots.data() + done, nnb, views.data() + done, hptr.data(), F.data() + done * 9,
                                            epi.data() + done * 2, 0, match.data(), status.data(), x3d.data(), first.data(),
                                            nm.data()) != COEB_OK)
            throw std::runtime_error(coeb_last_error(store.ctx()));
        for (int i = 0; i < n1; ++i) {
            const int j = first[i];
            if (j < 0) continue;
            const size_t e = (size_t)j * n1 + i;
            NewMapPointPair p;
            p.idx1 = (size_t)i; p.idx2 = (size_t)match[e];
            p.x3D[0] = x3d[3 * e]; p.x3D[1] = x3d[3 * e + 1]; p.x3D[2] = x3d[3 * e + 2];
            vvNewPoints[which[done + j]].push_back(p);        // i ascends: so does every neighbour's list
            has1[i] = 1;                                      // the MapPoint the caller adds: later neighbours skip it
            ++total;
        }
    }
    return total;
}

// The point list of a fuse call as the device reads it; descriptor keeps the uploaded bytes.
struct FusePointSnapshot {
    std::vector<uint8_t> valid, descriptor;
    std::vector<float> pos, normal, maxd, mind;
    coeb_fuse_points c() const
    {
        return coeb_fuse_points{(int32_t)valid.size(), valid.data(), pos.data(), normal.data(), maxd.data(), mind.data(),
                                descriptor.data()};
    }
};

template <class MapPointT>
inline void fuse_snapshot_point(FusePointSnapshot& s, size_t i, MapPointT* pMP)
{
    s.valid[i] = pMP && !pMP->isBad();
    s.maxd[i] = s.mind[i] = 1.f;
    if (!s.valid[i]) return;
    const cv::Mat p = pMP->GetWorldPos(), nrm = pMP->GetNormal(), d = pMP->GetDescriptor();
    for (int k = 0; k < 3; ++k) {
        s.pos[3 * i + k] = p.template at<float>(k);
        s.normal[3 * i + k] = nrm.template at<float>(k);
    }
    s.maxd[i] = pMP->GetMaxDistance();
    s.mind[i] = pMP->GetMinDistance();
    if (d.empty()) s.valid[i] = 0;                   // no descriptor yet: nothing to compare (the reference would read an empty Mat)
    else std::memcpy(&s.descriptor[32 * i], d.template ptr<uint8_t>(0), 32);
}

template <class MapPointT>
inline FusePointSnapshot fuse_snapshot(const std::vector<MapPointT*>& vpMapPoints)
{
    const size_t n = vpMapPoints.size();
    FusePointSnapshot s;
    s.valid.assign(n, 0); s.descriptor.assign(n * 32, 0);
    s.pos.assign(n * 3, 0.f); s.normal.assign(n * 3, 0.f); s.maxd.assign(n, 1.f); s.mind.assign(n, 1.f);
    std::unique_lock<std::mutex> lock(MapPointT::mGlobalMutex);
    for (size_t i = 0; i < n; ++i) fuse_snapshot_point(s, i, vpMapPoints[i]);
    return s;
}

template <class KeyFrameT>
inline coeb_camera fuse_camera(KeyFrameT* pKF)
{
    return coeb_camera{pKF->fx, pKF->fy, pKF->cx, pKF->cy, pKF->mbf, (float)pKF->mnMinX, (float)pKF->mnMaxX,
                       (float)pKF->mnMinY, (float)pKF->mnMaxY};
}

// One coeb_kfdb_fuse_search: points[first[j] .. first[j] + count[j]) against vpKFs[j], all under cam, for up to
// COEB_FUSE_MAX_JOBS keyframes that are in the store (the caller has checked).  skip[j][i] = IsInKeyFrame at
// the time of the call.  bestIdx[j] / bestDist[j] hold count[j] entries.
template <class KeyFrameT, class MapPointT>
inline void FuseSearch(KeyFrameStore<KeyFrameT>& store, const coeb_camera& cam, const FusePointSnapshot& snap,
                       const std::vector<MapPointT*>& vpMapPoints, const std::vector<KeyFrameT*>& vpKFs,
                       const std::vector<int>& first, const std::vector<int>& count, float th,
                       std::vector<std::vector<int32_t> >& bestIdx, std::vector<std::vector<int32_t> >& bestDist)
{
    const size_t nj = vpKFs.size();
    std::vector<coeb_fuse_job> jobs(nj);
    std::vector<std::vector<uint8_t> > skip(nj);
    size_t total = 0;
    std::unique_lock<std::mutex> lock(store.mutex());
    for (size_t j = 0; j < nj; ++j) {
        KeyFrameT* pKF = vpKFs[j];
        coeb_fuse_job& b = jobs[j];
        b.slot = store.slot(pKF);
        if (b.slot < 0) throw std::runtime_error("FuseSearch: a keyframe is not in the store");
        const cv::Mat R = pKF->GetRotation(), t = pKF->GetTranslation(), O = pKF->GetCameraCenter();
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) b.Rcw[3 * r + c] = R.template at<float>(r, c);
            b.tcw[r] = t.template at<float>(r);
            b.Ow[r] = O.template at<float>(r);
        }
        b.first = first[j]; b.count = count[j];
        skip[j].resize((size_t)count[j]);
        for (int i = 0; i < count[j]; ++i) {
            MapPointT* pMP = vpMapPoints[(size_t)first[j] + i];
            skip[j][i] = snap.valid[(size_t)first[j] + i] && pMP->IsInKeyFrame(pKF);
        }
        b.skip = count[j] ? skip[j].data() : nullptr;
        total += (size_t)count[j];
    }
    std::vector<int32_t> bi(total + 1), bd(total + 1);
    const coeb_fuse_points pts = snap.c();
    if (coeb_kfdb_fuse_search(store.handle(), &cam, &pts, jobs.data(), (int)nj, th, bi.data(), bd.data()) != COEB_OK)
        throw std::runtime_error(coeb_last_error(store.ctx()));
    bestIdx.assign(nj, std::vector<int32_t>());
    bestDist.assign(nj, std::vector<int32_t>());
    size_t at = 0;
    for (size_t j = 0; j < nj; ++j) {
        bestIdx[j].assign(bi.begin() + at, bi.begin() + at + count[j]);
        bestDist[j].assign(bd.begin() + at, bd.begin() + at + count[j]);
        at += (size_t)count[j];
    }
}

// The tail of ORBmatcher::Fuse's loop body (:953-971) for one point with a match; *survivor = the point a
// Replace kept (its descriptor was recomputed), else NULL.
template <class KeyFrameT, class MapPointT>
inline void fuse_act(KeyFrameT* pKF, MapPointT* pMP, int bestIdx, MapPointT** survivor)
{
    *survivor = nullptr;
    MapPointT* pMPinKF = pKF->GetMapPoint(bestIdx);
    if (pMPinKF) {
        if (!pMPinKF->isBad()) {
            if (pMPinKF->Observations() > pMP->Observations()) {
                pMP->Replace(pMPinKF);
                *survivor = pMPinKF;
            } else {
                pMPinKF->Replace(pMP);
                *survivor = pMP;
            }
        }
    } else {
        pMP->AddObservation(pKF, bestIdx);
        pKF->AddMapPoint(pMP, bestIdx);
    }
}

// ORBmatcher::Fuse(pKF, vpMapPoints, th): one device call, then the reference's loop with its own skips.
template <class KeyFrameT, class MapPointT>
inline int Fuse(KeyFrameStore<KeyFrameT>& store, KeyFrameT* pKF, const std::vector<MapPointT*>& vpMapPoints, float th = 3.0f)
{
    {
        std::unique_lock<std::mutex> lock(store.mutex());
        if (store.slot(pKF) < 0) return 0;               // never added: nothing fused
    }
    const int n = (int)vpMapPoints.size();
    if (!n) return 0;
    const FusePointSnapshot snap = fuse_snapshot(vpMapPoints);
    std::vector<std::vector<int32_t> > bi, bd;
    FuseSearch(store, fuse_camera(pKF), snap, vpMapPoints, std::vector<KeyFrameT*>(1, pKF), std::vector<int>(1, 0),
               std::vector<int>(1, n), th, bi, bd);
    int nFused = 0;
    for (int i = 0; i < n; ++i) {
        MapPointT* pMP = vpMapPoints[i];
        if (!pMP) continue;
        if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
        if (!snap.valid[i] || bi[0][i] < 0) continue;
        MapPointT* survivor;
        fuse_act(pKF, pMP, bi[0][i], &survivor);
        nFused++;
    }
    return nFused;
}

// for (pKFi : vpTargetKFs) matcher.Fuse(pKFi, vpMapPointMatches) (LocalMapping.cc:497-503) in one device call per
// COEB_FUSE_MAX_JOBS targets, plus one call whenever a listed point's descriptor changed before a later target
// reads it.  vnFused (may be NULL) receives nFused per target.  Returns the number of device calls.
template <class KeyFrameT, class MapPointT>
inline int FuseTargets(KeyFrameStore<KeyFrameT>& store, KeyFrameT* pKFcur, const std::vector<KeyFrameT*>& vpTargetKFs,
                       const std::vector<MapPointT*>& vpMapPointMatches, float th = 3.0f, std::vector<int>* vnFused = nullptr,
                       bool bRequery = true)
{
    const int n = (int)vpMapPointMatches.size(), T = (int)vpTargetKFs.size();
    if (vnFused) vnFused->assign((size_t)T, 0);
    if (!n || !T) return 0;
    std::vector<uint8_t> stored((size_t)T);
    {
        std::unique_lock<std::mutex> lock(store.mutex());
        for (int j = 0; j < T; ++j) stored[j] = store.slot(vpTargetKFs[j]) >= 0;
    }
    const coeb_camera cam = fuse_camera(pKFcur);
    FusePointSnapshot snap = fuse_snapshot(vpMapPointMatches);
    std::map<MapPointT*, int> index;                     // pointer -> first index in the list
    for (int i = n - 1; i >= 0; --i)
        if (vpMapPointMatches[i]) index[vpMapPointMatches[i]] = i;
    std::vector<std::vector<int32_t> > bi((size_t)T), bd((size_t)T);
    std::vector<uint8_t> stale((size_t)n, 0);
    int nstale = 0, ncalls = 0, have = 0;                // results of targets [0, have) are in bi
    for (int j = 0; j < T; ++j) {
        if (!stored[j]) continue;                        // never added: nothing fused
        KeyFrameT* pKF = vpTargetKFs[j];
        if (j >= have) {                                 // the next first call: targets j .. over the whole list
            std::vector<KeyFrameT*> kfs;
            std::vector<int> which;
            for (int k = j; k < T && (int)kfs.size() < COEB_FUSE_MAX_JOBS; ++k)
                if (stored[k]) { kfs.push_back(vpTargetKFs[k]); which.push_back(k); }
            if (nstale) {                                // every point afresh: the marks are cleared
                snap = fuse_snapshot(vpMapPointMatches);
                std::fill(stale.begin(), stale.end(), 0);
                nstale = 0;
            }
            std::vector<std::vector<int32_t> > ri, rd;
            FuseSearch(store, cam, snap, vpMapPointMatches, kfs, std::vector<int>(kfs.size(), 0),
                       std::vector<int>(kfs.size(), n), th, ri, rd);
            ncalls++;
            for (size_t q = 0; q < which.size(); ++q) { bi[which[q]].swap(ri[q]); bd[which[q]].swap(rd[q]); }
            have = which.back() + 1;
        }
        int nFused = 0;
        for (int i = 0; i < n; ++i) {
            MapPointT* pMP = vpMapPointMatches[i];
            if (!pMP) continue;
            if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
            if (stale[i] && bRequery) {
                // the stale points, with their descriptors of now, against the targets j .. have - 1
                std::vector<int> idx;
                for (int k = 0; k < n; ++k)
                    if (stale[k]) idx.push_back(k);
                std::vector<MapPointT*> pts(idx.size());
                for (size_t q = 0; q < idx.size(); ++q) pts[q] = vpMapPointMatches[idx[q]];
                const FusePointSnapshot fresh = fuse_snapshot(pts);
                std::vector<KeyFrameT*> kfs;
                std::vector<int> which;
                for (int k = j; k < have; ++k)
                    if (stored[k]) { kfs.push_back(vpTargetKFs[k]); which.push_back(k); }
                std::vector<std::vector<int32_t> > ri, rd;
                FuseSearch(store, cam, fresh, pts, kfs, std::vector<int>(kfs.size(), 0),
                           std::vector<int>(kfs.size(), (int)idx.size()), th, ri, rd);
                ncalls++;
                for (size_t w = 0; w < which.size(); ++w)
                    for (size_t q = 0; q < idx.size(); ++q) {
                        bi[which[w]][idx[q]] = ri[w][q];
                        bd[which[w]][idx[q]] = rd[w][q];
                    }
                for (size_t q = 0; q < idx.size(); ++q) {
                    const int k = idx[q];
                    snap.valid[k] = fresh.valid[q];
                    std::memcpy(&snap.descriptor[32 * k], &fresh.descriptor[32 * q], 32);
                    stale[k] = 0;
                }
                nstale = 0;
            }
            if (!snap.valid[i] || bi[j][i] < 0) continue;
            MapPointT* survivor;
            fuse_act(pKF, pMP, bi[j][i], &survivor);
            nFused++;
            if (survivor) {
                typename std::map<MapPointT*, int>::const_iterator it = index.find(survivor);
                if (it != index.end()) {
                    const cv::Mat d = survivor->GetDescriptor();
                    for (int k = it->second; k < n; ++k) {           // every index the survivor is listed at
                        if (vpMapPointMatches[k] != survivor || stale[k]) continue;
                        if (d.empty() || std::memcmp(&snap.descriptor[32 * k], d.template ptr<uint8_t>(0), 32)) {
                            stale[k] = 1;
                            nstale++;
                        }
                    }
                }
            }
        }
        if (vnFused) (*vnFused)[j] = nFused;
    }
    return ncalls;
}

}  // namespace coeb

#endif
