// Runs adapter/Tracking_coeb.h's TrackReferenceKeyFrame against libcoeb_front.so on the GPU with
// reference-shaped Frame / KeyFrame / MapPoint types that record what the adapter does to them.
//
//   trackref_exec DIR
//
// DIR holds what tests/test_adapter_trackref.py writes: cam.f32 (fx fy cx cy bf minX maxX minY maxY),
// T.f32 (mLastFrame.mTcw, 4x4), flags.i32 (prefill mBowVec / mFeatVec, frame id, levelsup), voc.txt
// (ORBvoc.txt format), kps.bin (cv::KeyPoint records), desc.u8, ur.f32, and with prefill bow_w.i32 /
// bow_v.f64 (mBowVec) and cur_node.i32 (the mFeatVec node per feature); the KeyFrame: k_kind.u8 (0 a good
// MapPoint, 1 isBad(), 2 NULL), k_kps.bin, k_desc.u8, k_node.i32, k_xw.f32, k_obs.i32.  Every
// MapPoint starts with mbTrackInView = true and mnLastFrameSeen = frame id - 1, the frame with
// mvpMapPoints all NULL, mvbOutlier all true and the identity pose.  DIR receives mvp.i32 (per
// keypoint the KeyFrame index of its MapPoint, -1 NULL), outl.u8, T_out.f32, ret.i32 (the return
// value, nmatchesMap), mp_inview.u8 / mp_seen.i32 (per KeyFrame slot), out_bow_w.i32 / out_bow_v.f64
// (mBowVec in word order) and out_fv.i32 (mFeatVec as (node, feature) pairs in map order).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "Tracking_coeb.h"

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
    cv::Mat pos;
    int nobs = 0;
    bool bad = false;
    cv::Mat GetWorldPos() { return pos.clone(); }
    int Observations() { return nobs; }
    bool isBad() { return bad; }
    bool mbTrackInView = true;
    long unsigned int mnLastFrameSeen = 0;
    static std::mutex mGlobalMutex;
};
std::mutex MapPoint::mGlobalMutex;

struct KeyFrame {
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
    std::vector<cv::KeyPoint> mvKeysUn;
    cv::Mat mDescriptors;
    FeatureVector mFeatVec;
};

struct Frame {
    static float fx, fy, cx, cy, mnMinX, mnMaxX, mnMinY, mnMaxY;
    long unsigned int mnId = 0;
    float mbf = 0;
    int N = 0;
    int mnScaleLevels = 8;
    float mfScaleFactor = 1.2f;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    cv::Mat mDescriptors, mTcw;
    BowVector mBowVec;
    FeatureVector mFeatVec;
    void SetPose(cv::Mat Tcw) { mTcw = Tcw.clone(); }
};
float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;

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

int main(int argc, char** argv)
{
    if (argc != 2) { std::cerr << "usage: trackref_exec DIR\n"; return 2; }
    const std::string d = std::string(argv[1]) + "/";
    const std::vector<float> cam = load<float>(d + "cam.f32"), T = load<float>(d + "T.f32");
    const std::vector<int32_t> flags = load<int32_t>(d + "flags.i32");
    Frame::fx = cam[0]; Frame::fy = cam[1]; Frame::cx = cam[2]; Frame::cy = cam[3];
    Frame::mnMinX = cam[5]; Frame::mnMaxX = cam[6]; Frame::mnMinY = cam[7]; Frame::mnMaxY = cam[8];
    const long unsigned int id = (long unsigned int)flags[1];
    coeb::Vocabulary voc;
    if (!voc.loadFromTextFile(d + "voc.txt")) { std::cerr << "bad voc.txt\n"; return 2; }

    const std::vector<uint8_t> kind = load<uint8_t>(d + "k_kind.u8");
    std::vector<uint8_t> kdesc = load<uint8_t>(d + "k_desc.u8");
    const std::vector<int32_t> knode = load<int32_t>(d + "k_node.i32"), kobs = load<int32_t>(d + "k_obs.i32");
    const std::vector<float> kxw = load<float>(d + "k_xw.f32");
    const int nq = (int)kind.size();
    std::vector<MapPoint> mps((size_t)nq);
    KeyFrame KF;
    KF.mvKeysUn = load<cv::KeyPoint>(d + "k_kps.bin");
    KF.mDescriptors = cv::Mat(nq, 32, CV_8U, kdesc.data());
    for (int i = 0; i < nq; i++) {
        MapPoint& m = mps[i];
        m.pos = cv::Mat(3, 1, CV_32F);
        for (int k = 0; k < 3; k++) m.pos.at<float>(k) = kxw[3 * i + k];
        m.nobs = kobs[i];
        m.bad = kind[i] == 1;
        m.mnLastFrameSeen = id - 1;
        KF.mvpMapPoints.push_back(kind[i] == 2 ? nullptr : &m);
        if (knode[i] >= 0) KF.mFeatVec.addFeature((unsigned int)knode[i], (unsigned int)i);
    }

    Frame F;
    F.mvKeysUn = load<cv::KeyPoint>(d + "kps.bin");
    std::vector<uint8_t> desc = load<uint8_t>(d + "desc.u8");
    const int N = (int)F.mvKeysUn.size();
    F.mnId = id;
    F.mbf = cam[4];
    F.N = N;
    F.mvuRight = load<float>(d + "ur.f32");
    F.mDescriptors = cv::Mat(N, 32, CV_8U, desc.data());
    F.mvbOutlier.assign((size_t)N, true);
    F.mvpMapPoints.assign((size_t)N, nullptr);
    F.mTcw = cv::Mat(4, 4, CV_32F);
    cv::Mat last(4, 4, CV_32F);
    for (int r = 0; r < 4; r++)
        for (int k = 0; k < 4; k++) {
            F.mTcw.at<float>(r, k) = r == k ? 1.f : 0.f;
            last.at<float>(r, k) = T[4 * r + k];
        }
    if (flags[0]) {
        const std::vector<int32_t> bw = load<int32_t>(d + "bow_w.i32"), cnode = load<int32_t>(d + "cur_node.i32");
        const std::vector<double> bv = load<double>(d + "bow_v.f64");
        for (size_t j = 0; j < bw.size(); j++) F.mBowVec.addWeight((unsigned int)bw[j], bv[j]);
        for (int i = 0; i < N; i++)
            if (cnode[i] >= 0) F.mFeatVec.addFeature((unsigned int)cnode[i], (unsigned int)i);
    }

    int nmatchesMap = -1;
    const bool ret = coeb::TrackReferenceKeyFrame(F, &KF, last, voc, 0.7f, true, flags[2], &nmatchesMap);

    std::vector<int32_t> mvp((size_t)N, -1), seen((size_t)nq), obw, ofv;
    std::vector<uint8_t> outl((size_t)N), inview((size_t)nq);
    std::vector<double> obv;
    std::vector<float> To(16);
    for (int i = 0; i < N; i++) {
        if (F.mvpMapPoints[i]) mvp[i] = (int32_t)(F.mvpMapPoints[i] - mps.data());
        outl[i] = F.mvbOutlier[i] ? 1 : 0;
    }
    for (int q = 0; q < nq; q++) {
        inview[q] = mps[q].mbTrackInView;
        seen[q] = (int32_t)mps[q].mnLastFrameSeen;
    }
    for (int r = 0; r < 4; r++)
        for (int k = 0; k < 4; k++) To[4 * r + k] = F.mTcw.at<float>(r, k);
    for (BowVector::const_iterator it = F.mBowVec.begin(); it != F.mBowVec.end(); ++it) {
        obw.push_back((int32_t)it->first);
        obv.push_back(it->second);
    }
    for (FeatureVector::const_iterator it = F.mFeatVec.begin(); it != F.mFeatVec.end(); ++it)
        for (size_t j = 0; j < it->second.size(); j++) {
            ofv.push_back((int32_t)it->first);
            ofv.push_back((int32_t)it->second[j]);
        }
    save(d + "mvp.i32", mvp);
    save(d + "outl.u8", outl);
    save(d + "T_out.f32", To);
    save(d + "ret.i32", std::vector<int32_t>{ret ? 1 : 0, nmatchesMap});
    save(d + "mp_inview.u8", inview);
    save(d + "mp_seen.i32", seen);
    save(d + "out_bow_w.i32", obw);
    save(d + "out_bow_v.f64", obv);
    save(d + "out_fv.i32", ofv);
    printf("ok\n");
    return 0;
}
