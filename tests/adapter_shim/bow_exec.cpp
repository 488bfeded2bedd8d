// Runs the bag-of-words drop-in adapters (adapter/BoW_coeb.h, ORBmatcher_coeb.h's SearchByBoW)
// against libcoeb_front.so on the GPU, with reference-shaped KeyFrame / Frame / MapPoint types
// and stand-ins for DBoW2's two containers (BowVector: map word -> value with addWeight,
// FeatureVector: map node -> indices with addFeature).
//
//   bow_exec DIR
//
// DIR holds what tests/test_adapter_bow.py writes: voc.txt (ORBvoc.txt format), kf_desc.u8 /
// cur_desc.u8 (N x 32), kf_valid.u8, kf_angle.f32, cur_angle.f32, and receives kf_bow.txt /
// cur_bow.txt ("w word value" and "f node index.." lines in container order), match.i32 (per
// frame keypoint the KeyFrame index whose MapPoint it got, -1) and nmatch.i32.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "BoW_coeb.h"
#include "ORBmatcher_coeb.h"

struct BowVector : std::map<unsigned int, double> {
    void addWeight(unsigned int id, double v)
    {
        iterator it = lower_bound(id);
        if (it != end() && !key_comp()(id, it->first)) it->second += v;
        else insert(it, value_type(id, v));
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
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
    std::vector<cv::KeyPoint> mvKeysUn;
    cv::Mat mDescriptors;
    BowVector mBowVec;
    FeatureVector mFeatVec;
};
struct Frame {
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

static cv::Mat desc_mat(const std::vector<uint8_t>& d)
{
    const int n = (int)(d.size() / 32);
    cv::Mat m(n, 32, CV_8U);
    if (n) std::memcpy(m.ptr<uint8_t>(0), d.data(), d.size());
    return m;
}

static void dump(const std::string& path, const BowVector& bv, const FeatureVector& fv)
{
    FILE* f = fopen(path.c_str(), "w");
    for (BowVector::const_iterator it = bv.begin(); it != bv.end(); ++it) fprintf(f, "w %u %.17g\n", it->first, it->second);
    for (FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it) {
        fprintf(f, "f %u", it->first);
        for (size_t j = 0; j < it->second.size(); j++) fprintf(f, " %u", it->second[j]);
        fprintf(f, "\n");
    }
    fclose(f);
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    coeb::Vocabulary voc;
    if (voc.loadFromTextFile(dir + "/missing.txt")) return 3;
    if (!voc.loadFromTextFile(dir + "/voc.txt")) return 4;
    KeyFrame kf;
    Frame F;
    kf.mDescriptors = desc_mat(load<uint8_t>(dir + "/kf_desc.u8"));
    F.mDescriptors = desc_mat(load<uint8_t>(dir + "/cur_desc.u8"));
    const std::vector<uint8_t> valid = load<uint8_t>(dir + "/kf_valid.u8");
    const std::vector<float> kang = load<float>(dir + "/kf_angle.f32"), fang = load<float>(dir + "/cur_angle.f32");
    std::vector<MapPoint> points(valid.size());
    kf.mvKeysUn.resize(valid.size());
    for (size_t i = 0; i < valid.size(); i++) {
        // invalid: alternately no MapPoint and a bad one
        points[i].bad = !valid[i] && (i & 1);
        kf.mvpMapPoints.push_back(!valid[i] && !(i & 1) ? nullptr : &points[i]);
        kf.mvKeysUn[i].angle = kang[i];
    }
    F.N = (int)fang.size();
    F.mvKeys.resize(fang.size());
    for (size_t i = 0; i < fang.size(); i++) F.mvKeys[i].angle = fang[i];
    coeb::ComputeBoW(kf.mDescriptors, voc, kf.mBowVec, kf.mFeatVec, 4);
    coeb::ComputeBoW(F.mDescriptors, voc, F.mBowVec, F.mFeatVec);          // levelsup = 4
    dump(dir + "/kf_bow.txt", kf.mBowVec, kf.mFeatVec);
    dump(dir + "/cur_bow.txt", F.mBowVec, F.mFeatVec);
    std::vector<MapPoint*> vpMapPointMatches;
    const int nmatches = coeb::SearchByBoW(&kf, F, vpMapPointMatches, 0.7f, true, voc.ctx());
    if ((int)vpMapPointMatches.size() != F.N) return 5;
    std::vector<int32_t> match(F.N, -1);
    for (int i = 0; i < F.N; i++)
        if (vpMapPointMatches[i]) match[i] = (int32_t)(vpMapPointMatches[i] - points.data());
    std::ofstream(dir + "/match.i32", std::ios::binary).write((const char*)match.data(), (std::streamsize)match.size() * 4);
    std::ofstream(dir + "/nmatch.i32", std::ios::binary).write((const char*)&nmatches, 4);
    printf("ok\n");
    return 0;
}
