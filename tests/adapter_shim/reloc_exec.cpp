// Runs adapter/Tracking_coeb.h's Relocalization<Solver> against libcoeb_front.so on the GPU with
// reference-shaped Frame / KeyFrame / MapPoint types and a scripted solver type that returns canned
// poses and inlier sets.
//
//   reloc_exec DIR
//
// DIR holds what tests/test_adapter_reloc.py writes: cam.f32 (fx fy cx cy bf minX maxX minY maxY),
// kps.bin (cv::KeyPoint records), desc.u8, ur.f32, ncand.i32 (the number of candidates), and per
// candidate c: kf<c>_valid.u8 (0: NULL, 1: a good point, 2: isBad()), kf<c>_xw.f32, kf<c>_desc.u8,
// kf<c>_maxd.f32, kf<c>_mind.f32, kf<c>_angle.f32, m<c>.i32 (vvpMapPointMatches as KeyFrame indices, -1
// NULL), s<c>_flags.i32 (per iterate call: bNoMore, a pose was found), s<c>_T.f32 (per call 16 floats),
// s<c>_inl.u8 (per call N flags).  The frame starts with mvpMapPoints all NULL, mvbOutlier all true and
// the identity pose.  DIR receives mvp.i32 (per keypoint the KeyFrame index of its MapPoint, -1 NULL),
// mvp_kf.i32 (the candidate that point belongs to), outl.u8, T_out.f32, ret.i32 (the return value,
// nCandidates afterwards), calls.i32 (iterate calls per candidate), discarded.u8.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "Tracking_coeb.h"

struct MapPoint {
    cv::Mat pos, desc;
    float maxd = 0, mind = 0;
    int slot = -1, kf = -1;
    bool bad = false;
    cv::Mat GetWorldPos() { return pos.clone(); }
    cv::Mat GetDescriptor() { return desc.clone(); }
    float GetMaxDistance() { return maxd; }
    float GetMinDistance() { return mind; }
    bool isBad() { return bad; }
    static std::mutex mGlobalMutex;
};
std::mutex MapPoint::mGlobalMutex;

struct KeyFrame {
    std::vector<MapPoint*> mps;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<MapPoint*> GetMapPointMatches() { return mps; }
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
    void SetPose(cv::Mat Tcw) { mTcw = Tcw.clone(); }
};
float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;

// what the script says iterate returns, call after call
struct ScriptedSolver {
    std::vector<int32_t> flags;
    std::vector<float> T;
    std::vector<uint8_t> inl;
    int N = 0, calls = 0;
    cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers)
    {
        if (nIterations != 5 || 2 * (size_t)calls >= flags.size()) { std::cerr << "unexpected iterate call\n"; std::exit(3); }
        const int k = calls++;
        bNoMore = flags[2 * k] != 0;
        vbInliers.assign((size_t)N, false);
        nInliers = 0;
        if (!flags[2 * k + 1]) return cv::Mat();
        for (int j = 0; j < N; j++) {
            vbInliers[j] = inl[(size_t)k * N + j] != 0;
            nInliers += vbInliers[j];
        }
        cv::Mat m(4, 4, CV_32F);
        for (int i = 0; i < 16; i++) m.at<float>(i / 4, i % 4) = T[16 * (size_t)k + i];
        return m;
    }
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

int main(int argc, char** argv)
{
    if (argc != 2) { std::cerr << "usage: reloc_exec DIR\n"; return 2; }
    const std::string d = std::string(argv[1]) + "/";
    const std::vector<float> cam = load<float>(d + "cam.f32");
    Frame::fx = cam[0]; Frame::fy = cam[1]; Frame::cx = cam[2]; Frame::cy = cam[3];
    Frame::mnMinX = cam[5]; Frame::mnMaxX = cam[6]; Frame::mnMinY = cam[7]; Frame::mnMaxY = cam[8];
    Frame F;
    F.mvKeysUn = load<cv::KeyPoint>(d + "kps.bin");
    std::vector<uint8_t> desc = load<uint8_t>(d + "desc.u8");
    const int N = (int)F.mvKeysUn.size();
    F.mbf = cam[4];
    F.N = N;
    F.mvuRight = load<float>(d + "ur.f32");
    F.mDescriptors = cv::Mat(N, 32, CV_8U, desc.data());
    F.mvbOutlier.assign((size_t)N, true);
    F.mvpMapPoints.assign((size_t)N, nullptr);
    F.mTcw = cv::Mat(4, 4, CV_32F);
    for (int i = 0; i < 16; i++) F.mTcw.at<float>(i / 4, i % 4) = i % 5 == 0 ? 1.f : 0.f;

    const int K = load<int32_t>(d + "ncand.i32")[0];
    std::vector<KeyFrame> kfs((size_t)K);
    std::vector<std::vector<MapPoint>> pts((size_t)K);
    std::vector<std::vector<uint8_t>> kdesc((size_t)K);
    std::vector<ScriptedSolver> solvers((size_t)K);
    std::vector<KeyFrame*> vpCandidateKFs;
    std::vector<ScriptedSolver*> vpPnPsolvers;
    std::vector<std::vector<MapPoint*>> vvpMapPointMatches((size_t)K);
    for (int c = 0; c < K; c++) {
        const std::string p = d + "kf" + std::to_string(c) + "_";
        const std::vector<uint8_t> valid = load<uint8_t>(p + "valid.u8");
        const std::vector<float> xw = load<float>(p + "xw.f32"), maxd = load<float>(p + "maxd.f32"),
                                 mind = load<float>(p + "mind.f32"), ang = load<float>(p + "angle.f32");
        kdesc[c] = load<uint8_t>(p + "desc.u8");
        const int nq = (int)valid.size();
        pts[c].resize((size_t)nq);
        kfs[c].mvKeysUn.resize((size_t)nq);
        for (int i = 0; i < nq; i++) {
            MapPoint& m = pts[c][i];
            m.pos = cv::Mat(3, 1, CV_32F);
            for (int k = 0; k < 3; k++) m.pos.at<float>(k) = xw[3 * (size_t)i + k];
            m.desc = cv::Mat(1, 32, CV_8U, kdesc[c].data() + 32 * (size_t)i);
            m.maxd = maxd[i]; m.mind = mind[i]; m.slot = i; m.kf = c; m.bad = valid[i] == 2;
            kfs[c].mvKeysUn[i].angle = ang[i];
            kfs[c].mps.push_back(valid[i] ? &m : nullptr);
        }
        const std::vector<int32_t> match = load<int32_t>(d + "m" + std::to_string(c) + ".i32");
        for (int j = 0; j < N; j++) vvpMapPointMatches[c].push_back(match[j] >= 0 ? &pts[c][match[j]] : nullptr);
        const std::string s = d + "s" + std::to_string(c) + "_";
        solvers[c].flags = load<int32_t>(s + "flags.i32");
        solvers[c].T = load<float>(s + "T.f32");
        solvers[c].inl = load<uint8_t>(s + "inl.u8");
        solvers[c].N = N;
        vpCandidateKFs.push_back(&kfs[c]);
        vpPnPsolvers.push_back(&solvers[c]);
    }
    std::vector<bool> vbDiscarded((size_t)K, false);
    int nCandidates = K;
    const bool ret = coeb::Relocalization(F, vpCandidateKFs, vpPnPsolvers, vvpMapPointMatches, vbDiscarded, nCandidates);

    std::vector<int32_t> mvp((size_t)N, -1), mvp_kf((size_t)N, -1), calls;
    std::vector<uint8_t> outl((size_t)N), disc;
    std::vector<float> To(16);
    for (int j = 0; j < N; j++) {
        if (F.mvpMapPoints[j]) { mvp[j] = F.mvpMapPoints[j]->slot; mvp_kf[j] = F.mvpMapPoints[j]->kf; }
        outl[j] = F.mvbOutlier[j] ? 1 : 0;
    }
    for (int i = 0; i < 16; i++) To[i] = F.mTcw.at<float>(i / 4, i % 4);
    for (int c = 0; c < K; c++) { calls.push_back(solvers[c].calls); disc.push_back(vbDiscarded[c] ? 1 : 0); }
    save(d + "mvp.i32", mvp);
    save(d + "mvp_kf.i32", mvp_kf);
    save(d + "outl.u8", outl);
    save(d + "T_out.f32", To);
    save(d + "ret.i32", std::vector<int32_t>{ret ? 1 : 0, nCandidates});
    save(d + "calls.i32", calls);
    save(d + "discarded.u8", disc);
    printf("ok\n");
    return 0;
}
