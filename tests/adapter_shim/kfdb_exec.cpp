// Runs the keyframe-database drop-in adapter (adapter/KeyFrameDatabase_coeb.h) against
// libcoeb_front.so on the GPU, with reference-shaped KeyFrame / Frame / MapPoint types, stand-ins
// for DBoW2's two containers and a fixed covisibility table.
//
//   kfdb_exec DIR
//
// DIR holds what tests/test_adapter_kfdb.py writes: voc.txt (ORBvoc.txt format), counts.i32 (features
// per keyframe), kf_desc.u8 / kf_valid.u8 / kf_angle.f32 (the keyframes' features, concatenated),
// cur_desc.u8 / cur_angle.f32, covis.i32 (per keyframe 10 neighbour ids, -1: none), bad.i32 (the id
// of a bad keyframe appended to the candidates).  Every keyframe is added, keyframe 7 is erased and
// added again, and DIR receives cands.i32 (candidate ids in order), reloc_query.i32 / reloc_words.i32 /
// reloc_score.f32 (per keyframe), match.i32 ([candidates + the bad one][N]: the keyframe feature
// whose MapPoint the keypoint got, -1) and nmatch.i32.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "KeyFrameDatabase_coeb.h"

struct BowVector : std::map<unsigned int, double> {
    void addWeight(unsigned int id, double v)
    {
        iterator it = lower_bound(id);
        if (it != end() && !key_comp()(id, it->first)) it->second += v;
        else insert(it, value_type(id, v));
    }
    void normalizeL1()
    {
        double norm = 0.0;
        for (iterator it = begin(); it != end(); ++it) norm += std::fabs(it->second);
        if (norm > 0.0)
            for (iterator it = begin(); it != end(); ++it) it->second /= norm;
    }
};
struct FeatureVector : std::map<unsigned int, std::vector<unsigned int>> {
    void addFeature(unsigned int id, unsigned int i) { (*this)[id].push_back(i); }
};

struct MapPoint {
    bool bad = false;
    bool isBad() { return bad; }
};
struct KeyFrame {
    long unsigned int mnId = 0;
    bool bad = false;
    bool isBad() { return bad; }
    std::vector<MapPoint> points;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
    std::vector<KeyFrame*> neighbours;
    std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N)
    {
        return (int)neighbours.size() > N ? std::vector<KeyFrame*>(neighbours.begin(), neighbours.begin() + N) : neighbours;
    }
    std::vector<cv::KeyPoint> mvKeysUn;
    cv::Mat mDescriptors;
    BowVector mBowVec;
    FeatureVector mFeatVec;
    long unsigned int mnRelocQuery = 0;
    int mnRelocWords = 0;
    float mRelocScore = 0;
};
struct Frame {
    long unsigned int mnId = 0;
    int N = 0;
    int mnScaleLevels = 8;
    float mfScaleFactor = 1.2f;
    std::vector<cv::KeyPoint> mvKeys;
    cv::Mat mDescriptors;
    BowVector mBowVec;
    FeatureVector mFeatVec;
};

template <class T>
static std::vector<T> load(const std::string& path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) { std::cerr << "missing " << path << "\n"; std::exit(2); }
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<T> v(raw.size() / sizeof(T));
    if (!v.empty()) std::memcpy(v.data(), raw.data(), v.size() * sizeof(T));
    return v;
}

template <class T>
static void save(const std::string& path, const std::vector<T>& v)
{
    std::ofstream(path, std::ios::binary).write((const char*)v.data(), (std::streamsize)(v.size() * sizeof(T)));
}

static cv::Mat desc_mat(const uint8_t* d, int n)
{
    cv::Mat m(n, 32, CV_8U);
    if (n) std::memcpy(m.ptr<uint8_t>(0), d, (size_t)n * 32);
    return m;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    coeb::Vocabulary voc;
    if (!voc.loadFromTextFile(dir + "/voc.txt")) return 4;
    const std::vector<int32_t> counts = load<int32_t>(dir + "/counts.i32"), covis = load<int32_t>(dir + "/covis.i32");
    const std::vector<uint8_t> kdesc = load<uint8_t>(dir + "/kf_desc.u8"), kvalid = load<uint8_t>(dir + "/kf_valid.u8");
    const std::vector<float> kang = load<float>(dir + "/kf_angle.f32"), fang = load<float>(dir + "/cur_angle.f32");
    const std::vector<uint8_t> cdesc = load<uint8_t>(dir + "/cur_desc.u8");
    const int bad_id = load<int32_t>(dir + "/bad.i32")[0];
    const int nkf = (int)counts.size();
    std::vector<KeyFrame> kfs((size_t)nkf);
    size_t at = 0;
    for (int k = 0; k < nkf; k++) {
        KeyFrame& kf = kfs[k];
        const int n = counts[k];
        kf.mnId = (long unsigned int)k;
        kf.mDescriptors = desc_mat(kdesc.data() + at * 32, n);
        kf.points.resize((size_t)n);
        kf.mvKeysUn.resize((size_t)n);
        for (int i = 0; i < n; i++) {
            // invalid: alternately no MapPoint and a bad one
            const bool valid = kvalid[at + i] != 0;
            kf.points[i].bad = !valid && (i & 1);
            kf.mvpMapPoints.push_back(!valid && !(i & 1) ? nullptr : &kf.points[i]);
            kf.mvKeysUn[i].angle = kang[at + i];
        }
        at += (size_t)n;
        coeb::ComputeBoW(kf.mDescriptors, voc, kf.mBowVec, kf.mFeatVec, 4);
        kf.mBowVec.normalizeL1();
        for (int j = 0; j < 10; j++)
            if (covis[(size_t)k * 10 + j] >= 0) kf.neighbours.push_back(&kfs[covis[(size_t)k * 10 + j]]);
    }
    Frame F;
    F.mnId = 5;
    F.N = (int)fang.size();
    F.mDescriptors = desc_mat(cdesc.data(), F.N);
    F.mvKeys.resize(fang.size());
    for (size_t i = 0; i < fang.size(); i++) F.mvKeys[i].angle = fang[i];
    coeb::ComputeBoW(F.mDescriptors, voc, F.mBowVec, F.mFeatVec);
    F.mBowVec.normalizeL1();
    {
        coeb::KeyFrameDatabase<KeyFrame, Frame> db(voc, 1000, 2);       // 12 keyframes: the storage grows
        for (int k = 0; k < nkf; k++) db.add(&kfs[k]);
        db.erase(&kfs[7]);
        db.erase(&kfs[7]);                                              // a second erase finds nothing
        db.add(&kfs[7]);
        std::vector<KeyFrame*> cands = db.DetectRelocalizationCandidates(&F);
        std::vector<int32_t> ids, rq, rw;
        std::vector<float> rs;
        for (size_t i = 0; i < cands.size(); i++) ids.push_back((int32_t)cands[i]->mnId);
        for (int k = 0; k < nkf; k++) {
            rq.push_back((int32_t)kfs[k].mnRelocQuery);
            rw.push_back(kfs[k].mnRelocWords);
            rs.push_back(kfs[k].mRelocScore);
        }
        save(dir + "/cands.i32", ids);
        save(dir + "/reloc_query.i32", rq);
        save(dir + "/reloc_words.i32", rw);
        save(dir + "/reloc_score.f32", rs);
        kfs[bad_id].bad = true;
        cands.push_back(&kfs[bad_id]);
        std::vector<std::vector<MapPoint*> > vvpMapPointMatches;
        std::vector<int> nmatches;
        coeb::SearchByBoWCandidates(db, cands, F, vvpMapPointMatches, nmatches, 0.75f, true);
        if (vvpMapPointMatches.size() != cands.size() || nmatches.size() != cands.size()) return 5;
        std::vector<int32_t> match, nm(nmatches.begin(), nmatches.end());
        for (size_t c = 0; c < cands.size(); c++) {
            if ((int)vvpMapPointMatches[c].size() != F.N) return 6;
            for (int i = 0; i < F.N; i++) {
                MapPoint* p = vvpMapPointMatches[c][i];
                match.push_back(p ? (int32_t)(p - cands[c]->points.data()) : -1);
            }
        }
        save(dir + "/match.i32", match);
        save(dir + "/nmatch.i32", nm);
        db.clear();
        if (!db.DetectRelocalizationCandidates(&F).empty()) return 7;
    }
    printf("ok\n");
    return 0;
}
