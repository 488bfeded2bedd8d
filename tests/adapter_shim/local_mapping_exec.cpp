// Runs the LocalMapping drop-in adapter (adapter/LocalMapping_coeb.h) against libcoeb_front.so on
// the GPU, with a reference-shaped KeyFrame and a stand-in for DBoW2's FeatureVector.
//
//   local_mapping_exec DIR
//
// DIR holds what tests/test_adapter_tri.py writes: counts.i32 (features per keyframe), desc.u8,
// node.i32 (the mFeatVec node of every feature, -1: none), keys.f32 ([x, y, angle, uRight] per
// feature), octave.i32, has_mp.u8 (all concatenated over the keyframes), pose.f32 (per keyframe R
// row-major, t, camera centre: 15 floats), cam.f32 (fx, fy, cx, cy), F12.f32 ([neighbour][9]) and
// flags.i32 (bOnlyStereo, bCheckOrientation).  Every keyframe enters a KeyFrameStore of one slot
// (it grows), keyframe 3 leaves and enters again, and keyframe 0 is searched against keyframes
// 1 .. n-1 and against one keyframe the store has never seen.  DIR receives match.i32
// ([neighbours][n0], from vvMatchedPairs, -1: none) and nmatch.i32 (the pair counts, then the total).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include <opencv2/core/core.hpp>

// the two cv::Mat expressions of ORBmatcher.cc:667 the stand-in Mat lacks: float, in element order
namespace cv {
inline Mat operator*(const Mat& a, const Mat& b)
{
    Mat m(a.rows, b.cols, CV_32F);
    for (int r = 0; r < a.rows; r++)
        for (int c = 0; c < b.cols; c++) {
            float s = 0.f;
            for (int k = 0; k < a.cols; k++) s += a.at<float>(r, k) * b.at<float>(k, c);
            m.at<float>(r, c) = s;
        }
    return m;
}
inline Mat operator+(const Mat& a, const Mat& b)
{
    Mat m(a.rows, a.cols, CV_32F);
    for (int r = 0; r < a.rows; r++)
        for (int c = 0; c < a.cols; c++) m.at<float>(r, c) = a.at<float>(r, c) + b.at<float>(r, c);
    return m;
}
}  // namespace cv

#include "LocalMapping_coeb.h"

struct FeatureVector : std::map<unsigned int, std::vector<unsigned int>> {
    void addFeature(unsigned int id, unsigned int i) { (*this)[id].push_back(i); }
};
struct MapPoint {};
struct KeyFrame {
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight;
    cv::Mat mDescriptors;
    FeatureVector mFeatVec;
    std::vector<MapPoint*> mvpMapPoints;
    MapPoint* GetMapPoint(const size_t& idx) { return mvpMapPoints[idx]; }
    cv::Mat R, t, Ow;
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    cv::Mat GetRotation() { return R.clone(); }
    cv::Mat GetTranslation() { return t.clone(); }
    float fx = 0, fy = 0, cx = 0, cy = 0;
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

static cv::Mat fmat(const float* p, int r, int c)
{
    cv::Mat m(r, c, CV_32F);
    std::memcpy(m.ptr<float>(0), p, (size_t)r * c * 4);
    return m;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    const std::vector<int32_t> counts = load<int32_t>(dir + "/counts.i32"), node = load<int32_t>(dir + "/node.i32");
    const std::vector<int32_t> octave = load<int32_t>(dir + "/octave.i32"), flags = load<int32_t>(dir + "/flags.i32");
    const std::vector<uint8_t> desc = load<uint8_t>(dir + "/desc.u8"), has_mp = load<uint8_t>(dir + "/has_mp.u8");
    const std::vector<float> keys = load<float>(dir + "/keys.f32"), pose = load<float>(dir + "/pose.f32");
    const std::vector<float> cam = load<float>(dir + "/cam.f32"), F12 = load<float>(dir + "/F12.f32");
    const int nkf = (int)counts.size();
    if (nkf < 5 || flags.size() != 2 || cam.size() != 4 || (int)pose.size() != nkf * 15 || (int)F12.size() != (nkf - 1) * 9)
        return 3;
    static MapPoint some_point;
    std::vector<KeyFrame> kfs((size_t)nkf);
    size_t at = 0;
    for (int k = 0; k < nkf; k++) {
        KeyFrame& kf = kfs[k];
        const int n = counts[k];
        kf.mDescriptors = cv::Mat(n, 32, CV_8U);
        if (n) std::memcpy(kf.mDescriptors.ptr<uint8_t>(0), desc.data() + at * 32, (size_t)n * 32);
        kf.mvKeysUn.resize((size_t)n);
        for (int i = 0; i < n; i++) {
            const float* q = keys.data() + (at + i) * 4;
            kf.mvKeysUn[i].pt = cv::Point2f(q[0], q[1]);
            kf.mvKeysUn[i].angle = q[2];
            kf.mvKeysUn[i].octave = octave[at + i];
            kf.mvuRight.push_back(q[3]);
            kf.mvpMapPoints.push_back(has_mp[at + i] ? &some_point : nullptr);
            if (node[at + i] >= 0) kf.mFeatVec.addFeature((unsigned int)node[at + i], (unsigned int)i);
        }
        at += (size_t)n;
        const float* p = pose.data() + (size_t)k * 15;
        kf.R = fmat(p, 3, 3); kf.t = fmat(p + 9, 3, 1); kf.Ow = fmat(p + 12, 3, 1);
        kf.fx = cam[0]; kf.fy = cam[1]; kf.cx = cam[2]; kf.cy = cam[3];
    }
    {
        coeb::KeyFrameStore<KeyFrame> store(8, 1.2f, 1000, 1);
        for (int k = 0; k < nkf; k++) store.add(&kfs[k]);
        store.add(&kfs[2]);                                  // already stored: left alone
        store.erase(&kfs[3]);
        store.erase(&kfs[3]);                                // a second erase finds nothing
        if (store.size() != (size_t)nkf - 1) return 4;
        store.add(&kfs[3]);                                  // the freed slot again, with its geometry
        KeyFrame stranger = kfs[1];
        std::vector<KeyFrame*> vpKF2;
        std::vector<cv::Mat> vF12;
        for (int k = 1; k < nkf; k++) {
            vpKF2.push_back(&kfs[k]);
            vF12.push_back(fmat(F12.data() + (size_t)(k - 1) * 9, 3, 3));
        }
        vpKF2.insert(vpKF2.begin() + 2, &stranger);          // not in the store: no pairs
        vF12.insert(vF12.begin() + 2, vF12[0]);
        std::vector<std::vector<std::pair<size_t, size_t> > > vvMatchedPairs;
        const int total = coeb::SearchForTriangulationNeighbors(store, &kfs[0], vpKF2, vF12, vvMatchedPairs, flags[0] != 0,
                                                                flags[1] != 0);
        if (vvMatchedPairs.size() != vpKF2.size() || !vvMatchedPairs[2].empty()) return 5;
        vvMatchedPairs.erase(vvMatchedPairs.begin() + 2);
        std::vector<int32_t> match((size_t)(nkf - 1) * counts[0], -1), nm;
        for (int j = 0; j < nkf - 1; j++) {
            size_t last = 0;
            for (size_t q = 0; q < vvMatchedPairs[j].size(); q++) {
                const std::pair<size_t, size_t>& pr = vvMatchedPairs[j][q];
                if (q && pr.first <= last) return 6;         // ascending idx1
                last = pr.first;
                match[(size_t)j * counts[0] + pr.first] = (int32_t)pr.second;
            }
            nm.push_back((int32_t)vvMatchedPairs[j].size());
        }
        nm.push_back(total);
        save(dir + "/match.i32", match);
        save(dir + "/nmatch.i32", nm);
        store.erase(&kfs[0]);
        try {
            coeb::SearchForTriangulationNeighbors(store, &kfs[0], vpKF2, vF12, vvMatchedPairs, false, false);
            return 7;                                        // pKF1 has left the store
        } catch (const std::runtime_error&) {
        }
    }
    printf("ok\n");
    return 0;
}
