/*
 * BoW_coeb.h -- MI355X body for Frame::ComputeBoW / KeyFrame::ComputeBoW
 *   src/Frame.cc:570-577:   mpORBvocabulary->transform(vCurrentDesc, mBowVec, mFeatVec, 4)
 * and the vocabulary it needs (ORBVocabulary::loadFromTextFile, src/System.cc:72).
 *
 * DBoW2 stays in the build for its containers only: coeb::ComputeBoW is templated on the two
 * container types and needs
 *     bowVec.addWeight(WordId, WordValue)        (DBoW2::BowVector)
 *     featVec.addFeature(NodeId, unsigned int)   (DBoW2::FeatureVector)
 * The body of Frame::ComputeBoW becomes
 *
 *     if (mBowVec.empty()) {
 *         coeb::ComputeBoW(mDescriptors, *coeb_voc, mBowVec, mFeatVec, 4);
 *         mBowVec.normalize(DBoW2::L1);      // what transform() does for ORBvoc.txt (TF_IDF, L1_NORM)
 *     }
 *
 * where coeb_voc is a coeb::Vocabulary loaded once from the same ORBvoc.txt.  Per feature the
 * word, its weight and the node at levelsup levels above the leaves come from
 * coeb_bow_transform; as in DBoW2 a word whose weight is not > 0 is added to neither container.
 * The tree walk restates TemplatedVocabulary::transform; parity against DBoW2 itself is
 * UNPINNED.  Normalisation stays with the caller's DBoW2 types.
 */
#ifndef COEB_ADAPTER_BOW_H
#define COEB_ADAPTER_BOW_H

#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

#include <opencv2/core/core.hpp>

#include "coeb_front.h"

namespace coeb
{

// ORBVocabulary's place: the parsed file and a context that holds its tables on the device.
class Vocabulary
{
public:
    Vocabulary() {}
    ~Vocabulary()
    {
        if (mCtx) coeb_destroy(mCtx);
        if (mVoc) coeb_voc_destroy(mVoc);
    }
    Vocabulary(const Vocabulary&) = delete;
    Vocabulary& operator=(const Vocabulary&) = delete;

    // as ORBVocabulary::loadFromTextFile: false when the file is missing or malformed
    bool loadFromTextFile(const std::string& path)
    {
        std::ifstream f(path.c_str(), std::ios::binary);
        if (!f) return false;
        const std::string text((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        return loadFromText(text.data(), text.size());
    }
    bool loadFromText(const char* text, size_t len)
    {
        coeb_voc* v = nullptr;
        if (coeb_voc_from_text(text, len, &v) != COEB_OK) return false;
        if (mVoc) coeb_voc_destroy(mVoc);
        mVoc = v;
        if (mCtx && coeb_bow_set_vocabulary(mCtx, mVoc) != COEB_OK) throw std::runtime_error(coeb_last_error(mCtx));
        return true;
    }
    bool empty() const { return mVoc == nullptr; }
    const coeb_voc* voc() const { return mVoc; }
    // the context whose device holds the tables (created at first use, on the calling thread's device 0)
    coeb_ctx* ctx()
    {
        if (!mVoc) throw std::runtime_error("coeb::Vocabulary: no vocabulary loaded");
        if (!mCtx) {
            if (coeb_abi_version() != COEB_ABI_VERSION) throw std::runtime_error("libcoeb_front ABI differs from the header");
            coeb_orb_params p{1000, 1.2f, 8, 20, 7};
            mCtx = coeb_create(&p, 0, 640, 480, 1);
            if (!mCtx) throw std::runtime_error(coeb_last_error(nullptr));
            if (coeb_bow_set_vocabulary(mCtx, mVoc) != COEB_OK) throw std::runtime_error(coeb_last_error(mCtx));
        }
        return mCtx;
    }

private:
    coeb_voc* mVoc = nullptr;
    coeb_ctx* mCtx = nullptr;
};

template <class BowVectorT, class FeatureVectorT>
inline void ComputeBoW(const cv::Mat& mDescriptors, Vocabulary& voc, BowVectorT& bowVec, FeatureVectorT& featVec,
                       int levelsup = 4)
{
    const cv::Mat desc = mDescriptors.isContinuous() ? mDescriptors : mDescriptors.clone();
    const int n = desc.rows;
    std::vector<int32_t> word((size_t)n), node((size_t)n);
    std::vector<double> weight((size_t)n);
    coeb_ctx* ctx = voc.ctx();
    const int rc = coeb_bow_transform(ctx, n ? desc.ptr<uint8_t>(0) : nullptr, n, levelsup, word.data(), node.data(),
                                      weight.data(), nullptr, nullptr, nullptr, 0, nullptr);
    if (rc != COEB_OK) throw std::runtime_error(coeb_last_error(ctx));
    for (int i = 0; i < n; ++i)
        if (node[i] >= 0) {                       // weight > 0
            bowVec.addWeight(word[i], weight[i]);
            featVec.addFeature(node[i], (unsigned int)i);
        }
}

}  // namespace coeb

#endif
