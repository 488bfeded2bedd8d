// Runs adapter/Tracking_coeb.h against libcoeb_front.so on the GPU with reference-shaped Frame /
// MapPoint types that record what the adapter does to them.
//
//   tracklm_exec DIR
//
// DIR holds what tests/test_adapter_tracklm.py writes: cam.f32 (fx fy cx cy bf minX maxX minY maxY),
// T.f32 (4x4), flags.i32 (mbOnlyTracking, frame id), kps.bin (cv::KeyPoint records), desc.u8,
// ur.f32, cur_obs.i32 (-1: no entry MapPoint), cur_xw.f32, cur_bad.u8 (the entry MapPoint isBad()),
// and the local map: p_kind.u8 (0 good, 1 isBad(), 2 mnLastFrameSeen == frame id), p_xw.f32,
// p_normal.f32, p_maxd.f32, p_mind.f32, p_desc.u8, p_obs.i32.  Every MapPoint starts with
// mbTrackInView = true.  TrackLocalMap runs on one copy of that state and SearchLocalPoints on
// another; DIR receives, for TrackLocalMap, mvp.i32 (per keypoint: -1 NULL, q a local-map point,
// 1000000 + i its entry MapPoint), outl.u8, T_out.f32, ret.i32, p_visible.i32 / p_found.i32 /
// p_inview.u8 / p_fields.f32 (x, y, xr, cos, level per point), e_visible.i32 / e_found.i32 /
// e_inview.u8 / e_seen.i32 (entry MapPoints), and for SearchLocalPoints s_mvp.i32, s_ret.i32,
// s_p_visible.i32.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "Tracking_coeb.h"

struct MapPoint {
    cv::Mat pos, normal, desc;
    int nobs = 0, mnVisible = 0, mnFound = 0;
    bool bad = false;
    float maxd = 0, mind = 0;
    cv::Mat GetWorldPos() { return pos.clone(); }
    cv::Mat GetNormal() { return normal.clone(); }
    cv::Mat GetDescriptor() { return desc.clone(); }
    int Observations() { return nobs; }
    bool isBad() { return bad; }
    void IncreaseVisible(int n = 1) { mnVisible += n; }
    void IncreaseFound(int n = 1) { mnFound += n; }
    float GetMaxDistance() { return maxd; }
    float GetMinDistance() { return mind; }
    bool mbTrackInView = true;
    float mTrackProjX = -1, mTrackProjY = -1, mTrackProjXR = -1;
    int mnTrackScaleLevel = -1;
    float mTrackViewCos = -1;
    long unsigned int mnLastFrameSeen = 0;
    static std::mutex mGlobalMutex;
};
std::mutex MapPoint::mGlobalMutex;

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

static cv::Mat vec3(const float* p)
{
    cv::Mat m(3, 1, CV_32F);
    for (int k = 0; k < 3; k++) m.at<float>(k) = p[k];
    return m;
}

struct State {
    std::vector<MapPoint> local, entry;
    std::vector<MapPoint*> vpLocal;
    Frame F;
};

int main(int argc, char** argv)
{
    if (argc != 2) { std::cerr << "usage: tracklm_exec DIR\n"; return 2; }
    const std::string d = std::string(argv[1]) + "/";
    const std::vector<float> cam = load<float>(d + "cam.f32"), T = load<float>(d + "T.f32");
    const std::vector<int32_t> flags = load<int32_t>(d + "flags.i32");
    Frame::fx = cam[0]; Frame::fy = cam[1]; Frame::cx = cam[2]; Frame::cy = cam[3];
    Frame::mnMinX = cam[5]; Frame::mnMaxX = cam[6]; Frame::mnMinY = cam[7]; Frame::mnMaxY = cam[8];
    const std::vector<cv::KeyPoint> kps = load<cv::KeyPoint>(d + "kps.bin");
    std::vector<uint8_t> desc = load<uint8_t>(d + "desc.u8");
    const std::vector<float> ur = load<float>(d + "ur.f32"), cxw = load<float>(d + "cur_xw.f32");
    const std::vector<int32_t> cobs = load<int32_t>(d + "cur_obs.i32"), pobs = load<int32_t>(d + "p_obs.i32");
    const std::vector<uint8_t> cbad = load<uint8_t>(d + "cur_bad.u8"), kind = load<uint8_t>(d + "p_kind.u8");
    const std::vector<uint8_t> pdesc = load<uint8_t>(d + "p_desc.u8");
    const std::vector<float> pxw = load<float>(d + "p_xw.f32"), pn = load<float>(d + "p_normal.f32");
    const std::vector<float> pmax = load<float>(d + "p_maxd.f32"), pmin = load<float>(d + "p_mind.f32");
    const int N = (int)kps.size(), nq = (int)kind.size();
    const long unsigned int id = (long unsigned int)flags[1];

    auto build = [&](State& s) {
        s.local.assign((size_t)nq, MapPoint());
        s.entry.assign((size_t)N, MapPoint());
        for (int q = 0; q < nq; q++) {
            MapPoint& m = s.local[q];
            m.pos = vec3(&pxw[3 * q]);
            m.normal = vec3(&pn[3 * q]);
            m.desc = cv::Mat(1, 32, CV_8U);
            std::memcpy(m.desc.data, &pdesc[32 * (size_t)q], 32);
            m.nobs = pobs[q];
            m.maxd = pmax[q];
            m.mind = pmin[q];
            m.bad = kind[q] == 1;
            m.mnLastFrameSeen = kind[q] == 2 ? id : id - 1;
            s.vpLocal.push_back(&m);
        }
        Frame& F = s.F;
        F.mnId = id;
        F.mbf = cam[4];
        F.N = N;
        F.mvKeysUn = kps;
        F.mvuRight = ur;
        F.mDescriptors = cv::Mat(N, 32, CV_8U, desc.data());
        F.mvbOutlier.assign((size_t)N, false);
        F.mTcw = cv::Mat(4, 4, CV_32F);
        for (int r = 0; r < 4; r++)
            for (int k = 0; k < 4; k++) F.mTcw.at<float>(r, k) = T[4 * r + k];
        F.mvpMapPoints.assign((size_t)N, nullptr);
        for (int i = 0; i < N; i++) {
            if (cobs[i] < 0) continue;
            MapPoint& m = s.entry[i];
            m.pos = vec3(&cxw[3 * i]);
            m.nobs = cobs[i];
            m.bad = cbad[i] != 0;
            m.mnLastFrameSeen = id - 1;
            F.mvpMapPoints[i] = &m;
        }
    };
    auto held = [&](const State& s) {
        std::vector<int32_t> v((size_t)N, -1);
        for (int i = 0; i < N; i++) {
            const MapPoint* p = s.F.mvpMapPoints[i];
            if (!p) continue;
            if (p >= s.local.data() && p < s.local.data() + nq) v[i] = (int32_t)(p - s.local.data());
            else v[i] = 1000000 + (int32_t)(p - s.entry.data());
        }
        return v;
    };

    State a;
    build(a);
    const int ret = coeb::TrackLocalMap(a.F, a.vpLocal, 3.0f, 0.8f, flags[0] != 0);
    save(d + "mvp.i32", held(a));
    std::vector<uint8_t> outl((size_t)N), pin((size_t)nq), ein((size_t)N);
    std::vector<int32_t> pvis((size_t)nq), pfound((size_t)nq), evis((size_t)N), efound((size_t)N), eseen((size_t)N);
    std::vector<float> pf((size_t)nq * 5), To(16);
    for (int i = 0; i < N; i++) {
        outl[i] = a.F.mvbOutlier[i] ? 1 : 0;
        evis[i] = a.entry[i].mnVisible;
        efound[i] = a.entry[i].mnFound;
        ein[i] = a.entry[i].mbTrackInView;
        eseen[i] = (int32_t)a.entry[i].mnLastFrameSeen;
    }
    for (int q = 0; q < nq; q++) {
        const MapPoint& m = a.local[q];
        pvis[q] = m.mnVisible;
        pfound[q] = m.mnFound;
        pin[q] = m.mbTrackInView;
        pf[5 * q + 0] = m.mTrackProjX; pf[5 * q + 1] = m.mTrackProjY; pf[5 * q + 2] = m.mTrackProjXR;
        pf[5 * q + 3] = m.mTrackViewCos; pf[5 * q + 4] = (float)m.mnTrackScaleLevel;
    }
    for (int r = 0; r < 4; r++)
        for (int k = 0; k < 4; k++) To[4 * r + k] = a.F.mTcw.at<float>(r, k);
    save(d + "outl.u8", outl);
    save(d + "T_out.f32", To);
    save(d + "ret.i32", std::vector<int32_t>(1, ret));
    save(d + "p_visible.i32", pvis);
    save(d + "p_found.i32", pfound);
    save(d + "p_inview.u8", pin);
    save(d + "p_fields.f32", pf);
    save(d + "e_visible.i32", evis);
    save(d + "e_found.i32", efound);
    save(d + "e_inview.u8", ein);
    save(d + "e_seen.i32", eseen);

    State b;
    build(b);
    const int sret = coeb::SearchLocalPoints(b.F, b.vpLocal, 3.0f, 0.8f);
    save(d + "s_mvp.i32", held(b));
    save(d + "s_ret.i32", std::vector<int32_t>(1, sret));
    for (int q = 0; q < nq; q++) pvis[q] = b.local[q].mnVisible;
    save(d + "s_p_visible.i32", pvis);
    printf("ok\n");
    return 0;
}
