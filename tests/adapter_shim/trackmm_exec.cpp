// Runs adapter/Tracking_coeb.h's TrackWithMotionModel against libcoeb_front.so on the GPU with
// reference-shaped Frame / MapPoint types that record what the adapter does to them.
//
//   trackmm_exec DIR
//
// DIR holds what tests/test_adapter_trackmm.py writes: cam.f32 (fx fy cx cy bf minX maxX minY maxY),
// V.f32 (mVelocity, 4x4), T_last.f32 (mLastFrame.mTcw), flags.i32 (localisation mode, frame id),
// thdepth.f32, kps.bin (cv::KeyPoint records), desc.u8, ur.f32; the last frame: l_kps.bin, l_desc.u8
// (mDescriptors), l_depth.f32, l_outl.u8, l_has.u8, l_xw.f32, l_mpdesc.u8, l_obs.i32 (its MapPoints).
// Every MapPoint starts with mbTrackInView = true and mnLastFrameSeen = frame id - 1, the frame with
// mvpMapPoints all NULL, mvbOutlier all true and the identity pose, mbVO as true.  DIR receives
// mvp.i32 (per keypoint the last-frame slot of its MapPoint, -1 NULL), outl.u8, T_out.f32, ret.i32
// (the return value, nmatchesMap, mbVO), mp_inview.u8 / mp_seen.i32 / mp_new.u8 (per last-frame slot,
// of the point it holds afterwards; mp_new: a temporary point), tmp_slot.i32 / tmp_pos.f32
// (mlpTemporalPoints in list order: the slot and the position each was made with).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <list>
#include <memory>
#include <string>
#include <vector>

#include "Tracking_coeb.h"

// cv::Mat's product for the 4x4 float poses of this program: row by column, summed in float in order
namespace cv
{
static Mat operator*(const Mat& a, const Mat& b)
{
    Mat c(4, 4, CV_32F);
    for (int r = 0; r < 4; r++)
        for (int k = 0; k < 4; k++) {
            float s = 0.f;
            for (int j = 0; j < 4; j++) s += a.at<float>(r, j) * b.at<float>(j, k);
            c.at<float>(r, k) = s;
        }
    return c;
}
}  // namespace cv

struct MapPoint {
    cv::Mat pos, desc;
    int nobs = 0, slot = -1;
    bool temporal = false;
    cv::Mat GetWorldPos() { return pos.clone(); }
    cv::Mat GetDescriptor() { return desc.clone(); }
    int Observations() { return nobs; }
    bool mbTrackInView = true;
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
    std::vector<float> mvuRight, mvDepth;
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

static cv::Mat mat4(const std::vector<float>& v)
{
    cv::Mat m(4, 4, CV_32F);
    for (int r = 0; r < 4; r++)
        for (int k = 0; k < 4; k++) m.at<float>(r, k) = v[4 * r + k];
    return m;
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::cerr << "usage: trackmm_exec DIR\n"; return 2; }
    const std::string d = std::string(argv[1]) + "/";
    const std::vector<float> cam = load<float>(d + "cam.f32"), thd = load<float>(d + "thdepth.f32");
    const std::vector<int32_t> flags = load<int32_t>(d + "flags.i32");
    Frame::fx = cam[0]; Frame::fy = cam[1]; Frame::cx = cam[2]; Frame::cy = cam[3];
    Frame::mnMinX = cam[5]; Frame::mnMaxX = cam[6]; Frame::mnMinY = cam[7]; Frame::mnMaxY = cam[8];
    const bool bOnlyTracking = flags[0] != 0;
    const long unsigned int id = (long unsigned int)flags[1];

    Frame L;
    L.mvKeysUn = load<cv::KeyPoint>(d + "l_kps.bin");
    const int nl = (int)L.mvKeysUn.size();
    std::vector<uint8_t> ldesc = load<uint8_t>(d + "l_desc.u8"), mpdesc = load<uint8_t>(d + "l_mpdesc.u8");
    const std::vector<uint8_t> lhas = load<uint8_t>(d + "l_has.u8"), loutl = load<uint8_t>(d + "l_outl.u8");
    const std::vector<float> lxw = load<float>(d + "l_xw.f32");
    const std::vector<int32_t> lobs = load<int32_t>(d + "l_obs.i32");
    L.mnId = id - 1;
    L.mbf = cam[4];
    L.N = nl;
    L.mvDepth = load<float>(d + "l_depth.f32");
    L.mDescriptors = cv::Mat(nl, 32, CV_8U, ldesc.data());
    L.mTcw = mat4(load<float>(d + "T_last.f32"));
    std::vector<MapPoint> mps((size_t)nl);
    for (int i = 0; i < nl; i++) {
        MapPoint& m = mps[i];
        m.pos = cv::Mat(3, 1, CV_32F);
        for (int k = 0; k < 3; k++) m.pos.at<float>(k) = lxw[3 * i + k];
        m.desc = cv::Mat(1, 32, CV_8U, mpdesc.data() + 32 * (size_t)i);
        m.nobs = lobs[i];
        m.slot = i;
        m.mnLastFrameSeen = id - 1;
        L.mvpMapPoints.push_back(lhas[i] ? &m : nullptr);
        L.mvbOutlier.push_back(loutl[i] != 0);
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
    F.mTcw = mat4({1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1});

    std::list<MapPoint*> mlpTemporalPoints;
    std::vector<std::unique_ptr<MapPoint>> owned;
    std::vector<float> tmp_pos;
    auto newPoint = [&](const cv::Mat& x3D, int i) {
        owned.emplace_back(new MapPoint());
        MapPoint* p = owned.back().get();
        p->pos = x3D.clone();
        p->desc = cv::Mat(1, 32, CV_8U, ldesc.data() + 32 * (size_t)i);
        p->slot = i;
        p->temporal = true;
        p->mnLastFrameSeen = id - 1;
        return p;
    };
    bool mbVO = true;
    int nmatchesMap = -1;
    const bool ret = coeb::TrackWithMotionModel(F, L, mat4(load<float>(d + "V.f32")), 15.f, false, bOnlyTracking,
                                                bOnlyTracking, thd[0], newPoint, mlpTemporalPoints, &mbVO, true,
                                                &nmatchesMap);

    std::vector<int32_t> mvp((size_t)N, -1), seen((size_t)nl, -1), tmp_slot;
    std::vector<uint8_t> outl((size_t)N), inview((size_t)nl, 2), isnew((size_t)nl);
    std::vector<float> To(16);
    for (int i = 0; i < N; i++) {
        if (F.mvpMapPoints[i]) mvp[i] = F.mvpMapPoints[i]->slot;
        outl[i] = F.mvbOutlier[i] ? 1 : 0;
    }
    for (int q = 0; q < nl; q++) {
        const MapPoint* p = L.mvpMapPoints[q];
        if (!p) continue;
        inview[q] = p->mbTrackInView;
        seen[q] = (int32_t)p->mnLastFrameSeen;
        isnew[q] = p->temporal;
    }
    for (MapPoint* p : mlpTemporalPoints) {
        tmp_slot.push_back(p->slot);
        for (int k = 0; k < 3; k++) tmp_pos.push_back(p->pos.at<float>(k));
    }
    for (int r = 0; r < 4; r++)
        for (int k = 0; k < 4; k++) To[4 * r + k] = F.mTcw.at<float>(r, k);
    save(d + "mvp.i32", mvp);
    save(d + "outl.u8", outl);
    save(d + "T_out.f32", To);
    save(d + "ret.i32", std::vector<int32_t>{ret ? 1 : 0, nmatchesMap, mbVO ? 1 : 0});
    save(d + "mp_inview.u8", inview);
    save(d + "mp_seen.i32", seen);
    save(d + "mp_new.u8", isnew);
    save(d + "tmp_slot.i32", tmp_slot);
    save(d + "tmp_pos.f32", tmp_pos);
    printf("ok\n");
    return 0;
}
