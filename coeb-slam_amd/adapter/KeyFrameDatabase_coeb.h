/*
 * KeyFrameDatabase_coeb.h -- MI355X bodies for the relocalisation half of KeyFrameDatabase
 *   add / erase / clear                      src/KeyFrameDatabase.cc:40-73
 *   DetectRelocalizationCandidates(Frame*)   src/KeyFrameDatabase.cc:199-309
 * and for the SearchByBoW loop of Tracking::Relocalization (src/Tracking.cc:1449-1470).
 *
 * coeb::KeyFrameDatabase<KeyFrame, Frame> keeps every keyframe's descriptors, feature-vector
 * nodes, keypoint angles and BowVector on the device (coeb_kfdb_add, once per keyframe: they do
 * not change after KeyFrame::ComputeBoW).  The reference's class keeps it as a member and forwards:
 *
 *     void KeyFrameDatabase::add(KeyFrame* pKF)   { mCoeb.add(pKF); }
 *     void KeyFrameDatabase::erase(KeyFrame* pKF) { mCoeb.erase(pKF); }
 *     void KeyFrameDatabase::clear()              { mCoeb.clear(); }
 *     vector<KeyFrame*> KeyFrameDatabase::DetectRelocalizationCandidates(Frame* F)
 *     { return mCoeb.DetectRelocalizationCandidates(F); }
 *
 * (mvInvertedFile stays for DetectLoopCandidates, which is not covered.)  There is no inverted
 * file on the device: mnRelocWords = |words(F) & words(KF)| is counted per keyframe, and
 * lKFsSharingWords comes back in the inverted file's order (ascending smallest common word, then
 * insertion).  DetectRelocalizationCandidates writes mnRelocQuery, mnRelocWords and mRelocScore as
 * the reference does and runs the covisibility accumulation (:258-308) here on the host, on the
 * reference's own KeyFrame graph (GetBestCovisibilityKeyFrames(10)).
 *
 * The loop of Relocalization becomes one call:
 *
 *     vector<int> vnMatches;
 *     coeb::SearchByBoWCandidates(db, vpCandidateKFs, mCurrentFrame, vvpMapPointMatches, vnMatches, 0.75f, true);
 *     for (int i = 0; i < nKFs; i++)
 *         if (vpCandidateKFs[i]->isBad() || vnMatches[i] < 15) vbDiscarded[i] = true; else { PnPsolver ... }
 *
 * It snapshots each candidate's isBad() and GetMapPointMatches() validity (pMP && !pMP->isBad());
 * a bad keyframe gets 0 matches and an all-NULL vector.  mMutex is held around every database
 * call, as in the reference: LocalMapping adds while Tracking queries, and the context behind the
 * database is not reentrant.  The database uses the Vocabulary's context (BoW_coeb.h).
 * BowVector scoring restates DBoW2's L1Scoring; parity against DBoW2 itself is UNPINNED
 * (DESIGN.md s4.13).
 */
#ifndef COEB_ADAPTER_KEYFRAMEDATABASE_H
#define COEB_ADAPTER_KEYFRAMEDATABASE_H

#include <list>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <utility>
#include <vector>

#include "BoW_coeb.h"
#include "ORBmatcher_coeb.h"

namespace coeb
{

template <class KeyFrameT, class FrameT>
class KeyFrameDatabase
{
public:
    explicit KeyFrameDatabase(Vocabulary& voc, int max_features = 4095, int initial_slots = 256) : mCtx(voc.ctx())
    {
        if (coeb_kfdb_create(mCtx, max_features, initial_slots, &mDb) != COEB_OK)
            throw std::runtime_error(coeb_last_error(mCtx));
    }
    ~KeyFrameDatabase() { coeb_kfdb_destroy(mDb); }       // before the Vocabulary that owns the context
    KeyFrameDatabase(const KeyFrameDatabase&) = delete;
    KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

    void add(KeyFrameT* pKF)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        const int n = (int)pKF->mvKeysUn.size();
        std::vector<int32_t> word;
        std::vector<double> value;
        for (typename BowVecOf<KeyFrameT>::const_iterator it = pKF->mBowVec.begin(); it != pKF->mBowVec.end(); ++it) {
            word.push_back((int32_t)it->first);
            value.push_back(it->second);
        }
        std::vector<float> ang((size_t)n);
        for (int i = 0; i < n; ++i) ang[i] = pKF->mvKeysUn[i].angle;
        const std::vector<int32_t> node = feature_nodes(pKF->mFeatVec, n);
        cv::Mat desc = pKF->mDescriptors.isContinuous() ? pKF->mDescriptors : pKF->mDescriptors.clone();
        coeb_kfdb_keyframe kf{n, desc.empty() ? nullptr : desc.ptr<uint8_t>(0), node.data(), ang.data(), word.data(),
                              value.data(), (int32_t)word.size()};
        int slot = -1;
        if (coeb_kfdb_add(mDb, &kf, &slot) != COEB_OK) throw std::runtime_error(coeb_last_error(mCtx));
        if ((int)mKF.size() <= slot) mKF.resize((size_t)slot + 1, nullptr);
        mKF[slot] = pKF;
        mSlot[pKF] = slot;
    }

    void erase(KeyFrameT* pKF)
    {
        std::unique_lock<std::mutex> lock(mMutex);
        typename std::map<KeyFrameT*, int>::iterator it = mSlot.find(pKF);
        if (it == mSlot.end()) return;                    // not in the database: the reference's loop finds nothing
        if (coeb_kfdb_erase(mDb, it->second) != COEB_OK) throw std::runtime_error(coeb_last_error(mCtx));
        mKF[it->second] = nullptr;
        mSlot.erase(it);
    }

    void clear()
    {
        std::unique_lock<std::mutex> lock(mMutex);
        if (coeb_kfdb_clear(mDb) != COEB_OK) throw std::runtime_error(coeb_last_error(mCtx));
        mKF.clear();
        mSlot.clear();
    }

    std::vector<KeyFrameT*> DetectRelocalizationCandidates(FrameT* F)
    {
        // lKFsSharingWords with mnRelocWords, and the scores of those above minCommonWords
        std::list<std::pair<float, KeyFrameT*> > lScoreAndMatch;
        {
            std::unique_lock<std::mutex> lock(mMutex);
            std::vector<int32_t> word;
            std::vector<double> value;
            for (typename BowVecOf<FrameT>::const_iterator it = F->mBowVec.begin(); it != F->mBowVec.end(); ++it) {
                word.push_back((int32_t)it->first);
                value.push_back(it->second);
            }
            int nkf = 0, ns = 0, nsharing = 0, maxCommonWords = 0, minCommonWords = 0;
            coeb_kfdb_size(mDb, &nkf, &ns);
            std::vector<int32_t> common((size_t)ns + 1), order((size_t)ns + 1);
            std::vector<float> score((size_t)ns + 1);
            if (coeb_kfdb_query(mDb, word.data(), value.data(), (int)word.size(), common.data(), score.data(), order.data(),
                                &nsharing, &maxCommonWords, &minCommonWords) != COEB_OK)
                throw std::runtime_error(coeb_last_error(mCtx));
            for (int j = 0; j < nsharing; ++j) {
                KeyFrameT* pKFi = mKF[order[j]];
                pKFi->mnRelocQuery = F->mnId;
                pKFi->mnRelocWords = common[order[j]];
                if (pKFi->mnRelocWords > minCommonWords) {
                    pKFi->mRelocScore = score[order[j]];
                    lScoreAndMatch.push_back(std::make_pair(score[order[j]], pKFi));
                }
            }
        }
        if (lScoreAndMatch.empty()) return std::vector<KeyFrameT*>();

        // accumulate over covisibility: per scored keyframe the sum over itself and those of its ten
        // best neighbours this query touched, and the best-scoring keyframe of that group
        std::vector<std::pair<float, KeyFrameT*> > groups;
        float bestAccScore = 0;
        for (typename std::list<std::pair<float, KeyFrameT*> >::iterator it = lScoreAndMatch.begin();
             it != lScoreAndMatch.end(); ++it) {
            KeyFrameT* pBestKF = it->second;
            float bestScore = it->first, accScore = it->first;
            const std::vector<KeyFrameT*> vpNeighs = it->second->GetBestCovisibilityKeyFrames(10);
            for (size_t k = 0; k < vpNeighs.size(); ++k) {
                KeyFrameT* pKF2 = vpNeighs[k];
                if (pKF2->mnRelocQuery != F->mnId) continue;
                accScore += pKF2->mRelocScore;
                if (pKF2->mRelocScore > bestScore) {
                    pBestKF = pKF2;
                    bestScore = pKF2->mRelocScore;
                }
            }
            groups.push_back(std::make_pair(accScore, pBestKF));
            if (accScore > bestAccScore) bestAccScore = accScore;
        }
        // every group above three quarters of the best, each keyframe once
        const float minScoreToRetain = 0.75f * bestAccScore;
        std::set<KeyFrameT*> spAlreadyAddedKF;
        std::vector<KeyFrameT*> vpRelocCandidates;
        for (size_t g = 0; g < groups.size(); ++g)
            if (groups[g].first > minScoreToRetain && spAlreadyAddedKF.insert(groups[g].second).second)
                vpRelocCandidates.push_back(groups[g].second);
        return vpRelocCandidates;
    }

    // for SearchByBoWCandidates; the slot of a keyframe (-1: not in the database) is read under mutex()
    std::mutex& mutex() { return mMutex; }
    coeb_kfdb* handle() { return mDb; }
    coeb_ctx* ctx() { return mCtx; }
    int slot(KeyFrameT* pKF) const
    {
        typename std::map<KeyFrameT*, int>::const_iterator it = mSlot.find(pKF);
        return it == mSlot.end() ? -1 : it->second;
    }

private:
    template <class T>
    struct BowVecOfImpl { typedef decltype(T::mBowVec) type; };
    template <class T>
    using BowVecOf = typename BowVecOfImpl<T>::type;

    coeb_ctx* mCtx;
    coeb_kfdb* mDb = nullptr;
    std::mutex mMutex;
    std::vector<KeyFrameT*> mKF;            // by slot
    std::map<KeyFrameT*, int> mSlot;
};

// SearchByBoW(vpCandidateKFs[i], F, vvpMapPointMatches[i]) for every candidate in one call;
// nmatches[i] is its return value (0, and an all-NULL vector, for a bad keyframe or one that is
// not in the database).
template <class KeyFrameT, class FrameT, class MapPointT>
inline void SearchByBoWCandidates(KeyFrameDatabase<KeyFrameT, FrameT>& db, const std::vector<KeyFrameT*>& vpCandidateKFs,
                                  FrameT& F, std::vector<std::vector<MapPointT*> >& vvpMapPointMatches,
                                  std::vector<int>& nmatches, float mfNNratio, bool mbCheckOrientation)
{
    const int nKFs = (int)vpCandidateKFs.size();
    vvpMapPointMatches.assign((size_t)nKFs, std::vector<MapPointT*>((size_t)F.N, static_cast<MapPointT*>(nullptr)));
    nmatches.assign((size_t)nKFs, 0);
    std::unique_lock<std::mutex> lock(db.mutex());
    std::vector<int> which;                               // candidates that are matched
    std::vector<int32_t> slots;
    std::vector<std::vector<MapPointT*> > points;
    std::vector<std::vector<uint8_t> > valid;
    for (int i = 0; i < nKFs; ++i) {
        KeyFrameT* pKF = vpCandidateKFs[i];
        const int slot = db.slot(pKF);
        if (slot < 0 || pKF->isBad()) continue;
        which.push_back(i);
        slots.push_back(slot);
        points.push_back(pKF->GetMapPointMatches());
        const std::vector<MapPointT*>& vp = points.back();
        std::vector<uint8_t> v(vp.size());
        for (size_t k = 0; k < vp.size(); ++k) v[k] = vp[k] && !vp[k]->isBad();
        valid.push_back(v);
    }
    std::vector<float> fang((size_t)F.N);
    for (int i = 0; i < F.N; ++i) fang[i] = F.mvKeys[i].angle;
    const std::vector<int32_t> fnode = feature_nodes(F.mFeatVec, F.N);
    cv::Mat curDesc = F.mDescriptors.isContinuous() ? F.mDescriptors : F.mDescriptors.clone();
    coeb_bow_frame cur{F.N, curDesc.empty() ? nullptr : curDesc.ptr<uint8_t>(0), fnode.data(), fang.data()};
    for (size_t done = 0; done < which.size(); done += 256) {          // 256 candidates per call
        const int nc = (int)std::min<size_t>(256, which.size() - done);
        std::vector<const uint8_t*> vptr((size_t)nc);
        for (int j = 0; j < nc; ++j) vptr[j] = valid[done + j].empty() ? nullptr : valid[done + j].data();
        std::vector<int32_t> match((size_t)nc * F.N + 1), nm((size_t)nc);
        if (coeb_match_bow_kfdb(db.handle(), slots.data() + done, nc, vptr.data(), &cur, mfNNratio, mbCheckOrientation ? 1 : 0,
                                match.data(), nm.data()) != COEB_OK)
            throw std::runtime_error(coeb_last_error(db.ctx()));
        for (int j = 0; j < nc; ++j) {
            const int i = which[done + j];
            nmatches[i] = nm[j];
            for (int f = 0; f < F.N; ++f) {
                const int32_t m = match[(size_t)j * F.N + f];
                if (m >= 0) vvpMapPointMatches[i][f] = points[done + j][m];
            }
        }
    }
}

}  // namespace coeb

#endif
