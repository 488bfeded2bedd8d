// Runs the two loops of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:497-530) two ways over a small
// functional map of KeyFrame / MapPoint stand-ins: with a host loop restated from ORBmatcher::Fuse
// (src/ORBmatcher.cc:826-976) in the project's float forms, and through coeb::FuseTargets /
// coeb::Fuse (adapter/LocalMapping_coeb.h) against libcoeb_front.so on the GPU.  The two final maps have to be
// identical: every keyframe's point per feature, every point's observations, bad flags, mpReplaced,
// descriptors, and every nFused.
//
//   fuse_exec plain       a random scene in which no descriptor can change (all observations of a world point
//                         carry one descriptor): direction 1 takes one device call
//   fuse_exec hazard      the same scene plus a point of the current keyframe that absorbs a target's point at
//                         target 1, gets another descriptor from ComputeDistinctiveDescriptors, and no longer
//                         matches the feature of target 2 that its uploaded descriptor matches: two calls
//   fuse_exec norequery   the hazard scene through an adapter without the re-query: the maps must differ
//   fuse_exec time T      wall times on a scene of T targets with 1000 features each (tools/fuse_time.py)
// Prints "ok calls=<n>" (or the JSON of the timing).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include <opencv2/core/core.hpp>

// the two cv::Mat expressions of LocalMapping_coeb.h's triangulation half that the stand-in Mat lacks
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

static const int TH_LOW = 50;
static const int NLEVELS = 8;

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 2862933555777941757ULL + 3037000493ULL) {}
    uint32_t next() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (uint32_t)(s >> 33); }
    float uni(float a, float b) { return a + (b - a) * (float)(next() & 0xFFFFFF) / 16777216.0f; }
    int below(int n) { return (int)(next() % (uint32_t)n); }
};

static int hamming(const uint8_t* a, const uint8_t* b)
{
    int d = 0;
    for (int k = 0; k < 32; k++) d += __builtin_popcount((unsigned)(a[k] ^ b[k]));
    return d;
}

struct KeyFrame;
struct ById { bool operator()(const KeyFrame* a, const KeyFrame* b) const; };

struct FeatureVector : std::map<unsigned int, std::vector<unsigned int>> {};

struct MapPoint {
    static std::mutex mGlobalMutex;
    int id = 0;
    cv::Mat mWorldPos, mNormal, mDescriptor;
    float mfMaxDistance = 1, mfMinDistance = 1;
    bool mbBad = false;
    MapPoint* mpReplaced = nullptr;
    std::map<KeyFrame*, size_t, ById> mObservations;
    int nObs = 0;
    bool isBad() { return mbBad; }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    cv::Mat GetNormal() { return mNormal.clone(); }
    cv::Mat GetDescriptor() { return mDescriptor.clone(); }
    float GetMaxDistance() { return mfMaxDistance; }
    float GetMinDistance() { return mfMinDistance; }
    int Observations() { return nObs; }
    bool IsInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) != 0; }
    void AddObservation(KeyFrame* pKF, size_t idx);
    void Replace(MapPoint* pMP);
    void ComputeDistinctiveDescriptors();
};
std::mutex MapPoint::mGlobalMutex;

struct KeyFrame {
    int id = 0;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight;
    cv::Mat mDescriptors;
    FeatureVector mFeatVec;
    std::vector<MapPoint*> mvpMapPoints;
    cv::Mat R, t, Ow;
    float fx = 517.3f, fy = 516.5f, cx = 318.6f, cy = 255.3f, mbf = 40.f;
    int mnMinX = 0, mnMaxX = 640, mnMinY = 0, mnMaxY = 480;
    MapPoint* GetMapPoint(const size_t& idx) { return mvpMapPoints[idx]; }
    void AddMapPoint(MapPoint* pMP, const size_t& idx) { mvpMapPoints[idx] = pMP; }
    void ReplaceMapPointMatch(const size_t& idx, MapPoint* pMP) { mvpMapPoints[idx] = pMP; }
    void EraseMapPointMatch(const size_t& idx) { mvpMapPoints[idx] = nullptr; }
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    cv::Mat GetRotation() { return R.clone(); }
    cv::Mat GetTranslation() { return t.clone(); }
    int add(float x, float y, int octave, float ur, const uint8_t* d)
    {
        cv::KeyPoint kp;
        kp.pt = cv::Point2f(x, y);
        kp.octave = octave;
        kp.angle = 0.f;
        mvKeysUn.push_back(kp);
        mvuRight.push_back(ur);
        rows.insert(rows.end(), d, d + 32);
        mvpMapPoints.push_back(nullptr);
        return (int)mvKeysUn.size() - 1;
    }
    void seal()
    {
        const int n = (int)mvKeysUn.size();
        mDescriptors = cv::Mat(n, 32, CV_8U);
        if (n) std::memcpy(mDescriptors.ptr<uint8_t>(0), rows.data(), rows.size());
    }
    std::vector<uint8_t> rows;
};
bool ById::operator()(const KeyFrame* a, const KeyFrame* b) const { return a->id < b->id; }

void MapPoint::AddObservation(KeyFrame* pKF, size_t idx)          // MapPoint.cc:84-95
{
    if (mObservations.count(pKF)) return;
    mObservations[pKF] = idx;
    nObs += pKF->mvuRight[idx] >= 0 ? 2 : 1;
}

void MapPoint::Replace(MapPoint* pMP)                              // MapPoint.cc:171-215
{
    if (pMP->id == id) return;
    std::map<KeyFrame*, size_t, ById> obs = mObservations;
    mObservations.clear();
    mbBad = true;
    mpReplaced = pMP;
    for (std::map<KeyFrame*, size_t, ById>::iterator mit = obs.begin(); mit != obs.end(); ++mit) {
        KeyFrame* pKF = mit->first;
        if (!pMP->IsInKeyFrame(pKF)) {
            pKF->ReplaceMapPointMatch(mit->second, pMP);
            pMP->AddObservation(pKF, mit->second);
        } else {
            pKF->EraseMapPointMatch(mit->second);
        }
    }
    pMP->ComputeDistinctiveDescriptors();
}

void MapPoint::ComputeDistinctiveDescriptors()                     // MapPoint.cc:236-305: the least median distance
{
    if (mbBad || mObservations.empty()) return;
    std::vector<const uint8_t*> v;
    for (std::map<KeyFrame*, size_t, ById>::iterator mit = mObservations.begin(); mit != mObservations.end(); ++mit)
        v.push_back(mit->first->mDescriptors.ptr<uint8_t>((int)mit->second));
    const size_t N = v.size();
    int BestMedian = 0x7fffffff, BestIdx = 0;
    for (size_t i = 0; i < N; i++) {
        std::vector<int> vDists(N);
        for (size_t j = 0; j < N; j++) vDists[j] = hamming(v[i], v[j]);
        std::sort(vDists.begin(), vDists.end());
        const int median = vDists[(size_t)(0.5 * (N - 1))];
        if (median < BestMedian) { BestMedian = median; BestIdx = (int)i; }
    }
    mDescriptor = cv::Mat(1, 32, CV_8U);
    std::memcpy(mDescriptor.ptr<uint8_t>(0), v[BestIdx], 32);
}

struct Tables { float scale[NLEVELS], inv_sigma2[NLEVELS], log_sf; };
static Tables tables()
{
    Tables t;
    const double sf = (double)1.2f;
    t.scale[0] = 1.f;
    float sigma2[NLEVELS] = {1.f};
    for (int i = 1; i < NLEVELS; i++) { t.scale[i] = (float)(t.scale[i - 1] * sf); sigma2[i] = t.scale[i] * t.scale[i]; }
    for (int i = 0; i < NLEVELS; i++) t.inv_sigma2[i] = 1.0f / sigma2[i];
    t.log_sf = (float)std::log((double)1.2f);
    return t;
}

// The 64 x 48 grid of a keyframe, as Frame::AssignFeaturesToGrid fills it.
struct Grid {
    std::vector<std::vector<int>> cell;
    float inv_w, inv_h;
    explicit Grid(KeyFrame* kf) : cell(64 * 48)
    {
        inv_w = 64.f / (float)(kf->mnMaxX - kf->mnMinX);
        inv_h = 48.f / (float)(kf->mnMaxY - kf->mnMinY);
        for (size_t i = 0; i < kf->mvKeysUn.size(); i++) {
            const int px = (int)roundf((kf->mvKeysUn[i].pt.x - kf->mnMinX) * inv_w), py = (int)roundf((kf->mvKeysUn[i].pt.y - kf->mnMinY) * inv_h);
            if (px < 0 || px >= 64 || py < 0 || py >= 48) continue;
            cell[px * 48 + py].push_back((int)i);
        }
    }
};

// The search of ORBmatcher::Fuse for one point (:853-950): bestIdx where bestDist <= TH_LOW, else -1.
static int fuse_search_host(KeyFrame* pKF, const Grid& g, const Tables& tb, MapPoint* pMP, float th)
{
    const float* R = pKF->R.ptr<float>(0);
    const float* t = pKF->t.ptr<float>(0);
    const float* O = pKF->Ow.ptr<float>(0);
    const float* P = pMP->mWorldPos.ptr<float>(0);
    const float* Pn = pMP->mNormal.ptr<float>(0);
    float Pc[3];
    for (int k = 0; k < 3; k++) {
        float v = R[3 * k] * P[0] + R[3 * k + 1] * P[1];
        v = v + R[3 * k + 2] * P[2];
        Pc[k] = (float)((double)v + (double)t[k]);
    }
    if (Pc[2] < 0.0f) return -1;
    const float invz = 1.0f / Pc[2];
    const float x = Pc[0] * invz, y = Pc[1] * invz;
    const float u = std::fmaf(pKF->fx, x, pKF->cx), v = std::fmaf(pKF->fy, y, pKF->cy);
    if (!(u >= pKF->mnMinX && u < pKF->mnMaxX && v >= pKF->mnMinY && v < pKF->mnMaxY)) return -1;
    const float ur = std::fmaf(-pKF->mbf, invz, u);
    const float PO[3] = {P[0] - O[0], P[1] - O[1], P[2] - O[2]};
    double ss = 0.0, dot = 0.0;
    for (int k = 0; k < 3; k++) { ss += (double)PO[k] * (double)PO[k]; dot += (double)PO[k] * (double)Pn[k]; }
    const float dist3D = (float)std::sqrt(ss);
    if (dist3D < 0.8f * pMP->mfMinDistance || dist3D > 1.2f * pMP->mfMaxDistance) return -1;
    if (dot < 0.5 * (double)dist3D) return -1;
    const float ratio = pMP->mfMaxDistance / dist3D;
    int lvl = (int)std::ceil((float)std::log((double)ratio) / tb.log_sf);
    lvl = lvl < 0 ? 0 : (lvl >= NLEVELS ? NLEVELS - 1 : lvl);
    const float r = th * tb.scale[lvl];
    const int x0 = std::max(0, (int)std::floor((u - pKF->mnMinX - r) * g.inv_w));
    if (x0 >= 64) return -1;
    const int x1 = std::min(63, (int)std::ceil((u - pKF->mnMinX + r) * g.inv_w));
    if (x1 < 0) return -1;
    const int y0 = std::max(0, (int)std::floor((v - pKF->mnMinY - r) * g.inv_h));
    if (y0 >= 48) return -1;
    const int y1 = std::min(47, (int)std::ceil((v - pKF->mnMinY + r) * g.inv_h));
    if (y1 < 0) return -1;
    const uint8_t* dMP = pMP->mDescriptor.ptr<uint8_t>(0);
    int bestDist = 256, bestIdx = -1;
    for (int ix = x0; ix <= x1; ix++)
        for (int iy = y0; iy <= y1; iy++)
            for (int idx : g.cell[ix * 48 + iy]) {
                const cv::KeyPoint& kp = pKF->mvKeysUn[idx];
                if (!(std::fabs(kp.pt.x - u) < r && std::fabs(kp.pt.y - v) < r)) continue;
                if (kp.octave < lvl - 1 || kp.octave > lvl) continue;
                const float ex = u - kp.pt.x, ey = v - kp.pt.y;
                float e2 = std::fmaf(ex, ex, ey * ey);
                if (pKF->mvuRight[idx] >= 0) {
                    const float er = ur - pKF->mvuRight[idx];
                    e2 = std::fmaf(er, er, e2);
                    if (e2 * tb.inv_sigma2[kp.octave] > 7.8) continue;
                } else if (e2 * tb.inv_sigma2[kp.octave] > 5.99) {
                    continue;
                }
                const int dist = hamming(dMP, pKF->mDescriptors.ptr<uint8_t>(idx));
                if (dist < bestDist) { bestDist = dist; bestIdx = idx; }
            }
    return bestDist <= TH_LOW ? bestIdx : -1;
}

static int fuse_host(KeyFrame* pKF, const std::vector<MapPoint*>& vpMapPoints, const Tables& tb, float th = 3.0f)
{
    const Grid g(pKF);
    int nFused = 0;
    for (MapPoint* pMP : vpMapPoints) {
        if (!pMP) continue;
        if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
        const int bestIdx = fuse_search_host(pKF, g, tb, pMP, th);
        if (bestIdx < 0) continue;
        MapPoint* pMPinKF = pKF->GetMapPoint(bestIdx);
        if (pMPinKF) {
            if (!pMPinKF->isBad()) {
                if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
                else pMPinKF->Replace(pMP);
            }
        } else {
            pMP->AddObservation(pKF, bestIdx);
            pKF->AddMapPoint(pMP, bestIdx);
        }
        nFused++;
    }
    return nFused;
}

// ------------------------------------------------------------------ the map
struct World {
    std::vector<KeyFrame*> kfs;          // kfs[0] is the current keyframe, then the targets, then bystanders
    std::vector<MapPoint*> mps;
    int ntargets = 0;
    ~World()
    {
        for (KeyFrame* k : kfs) delete k;
        for (MapPoint* m : mps) delete m;
    }
};

static cv::Mat vec3(float a, float b, float c)
{
    cv::Mat m(3, 1, CV_32F);
    m.at<float>(0) = a; m.at<float>(1) = b; m.at<float>(2) = c;
    return m;
}

static KeyFrame* new_kf(World& w, float tx, float ty, float tz)
{
    KeyFrame* k = new KeyFrame;
    k->id = (int)w.kfs.size();
    k->R = cv::Mat(3, 3, CV_32F);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) k->R.at<float>(r, c) = r == c ? 1.f : 0.f;
    k->t = vec3(tx, ty, tz);
    k->Ow = vec3(-tx, -ty, -tz);
    w.kfs.push_back(k);
    return k;
}

static MapPoint* new_mp(World& w, float X, float Y, float Z, float maxd)
{
    MapPoint* m = new MapPoint;
    m->id = (int)w.mps.size();
    m->mWorldPos = vec3(X, Y, Z);
    const float n = std::sqrt(X * X + Y * Y + Z * Z);
    m->mNormal = vec3(X / n, Y / n, Z / n);
    m->mfMaxDistance = maxd;
    m->mfMinDistance = maxd / 3.5f;
    w.mps.push_back(m);
    return m;
}

// the feature of (X, Y, Z) in k: pixel (with an offset), level from maxd, stereo or mono
static int observe(KeyFrame* k, const Tables& tb, float X, float Y, float Z, float maxd, const uint8_t* d, float dx, float dy,
                   bool stereo)
{
    const float xc = X + k->t.at<float>(0), yc = Y + k->t.at<float>(1), zc = Z + k->t.at<float>(2);
    const float u = k->fx * xc / zc + k->cx + dx, v = k->fy * yc / zc + k->cy + dy;
    const float ox = X - k->Ow.at<float>(0), oy = Y - k->Ow.at<float>(1), oz = Z - k->Ow.at<float>(2);
    const float dist = std::sqrt(ox * ox + oy * oy + oz * oz);
    int lvl = (int)std::ceil(std::log(maxd / dist) / std::log(1.2f));
    lvl = std::max(0, std::min(NLEVELS - 1, lvl));
    return k->add(u, v, lvl, stereo ? u - k->mbf / zc : -1.f, d);
}

static void link(MapPoint* m, KeyFrame* k, int idx)
{
    k->mvpMapPoints[idx] = m;
    m->AddObservation(k, (size_t)idx);
}

static void flip(uint8_t* d, int from, int count)
{
    for (int b = from; b < from + count; b++) d[b >> 3] ^= (uint8_t)(1u << (b & 7));
}

// npts world points seen by the current keyframe and the targets.  Each world point has a MapPoint A held by the
// current keyframe (and some targets) and, for half of them, a duplicate B held by other targets; the rest of
// the targets see the feature without a point.  All observations of a world point carry one descriptor.
static void build(World& w, int ntargets, int npts, int nextra, bool hazard, uint64_t seed)
{
    const Tables tb = tables();
    Rng rng(seed);
    w.ntargets = ntargets;
    new_kf(w, 0, 0, 0);
    for (int j = 0; j < ntargets; j++) new_kf(w, rng.uni(-0.25f, 0.25f), rng.uni(-0.15f, 0.15f), rng.uni(-0.1f, 0.1f));
    KeyFrame* cur = w.kfs[0];
    for (int p = 0; p < npts; p++) {
        const float X = rng.uni(-2.2f, 2.2f), Y = rng.uni(-1.5f, 1.5f), Z = rng.uni(3.f, 8.f);
        const float maxd = std::sqrt(X * X + Y * Y + Z * Z) * std::pow(1.2f, rng.uni(0.3f, 5.5f));
        uint8_t d[32];
        for (int k = 0; k < 32; k++) d[k] = (uint8_t)rng.next();
        MapPoint* A = nullptr;
        MapPoint* B = nullptr;
        const bool in_cur = p % 4 != 3;                  // a quarter of the points is not in the current keyframe
        if (in_cur) {
            A = new_mp(w, X, Y, Z, maxd);
            link(A, cur, observe(cur, tb, X, Y, Z, maxd, d, 0, 0, p % 2 == 0));
        }
        for (int j = 1; j <= ntargets; j++) {
            const int what = rng.below(5);               // 0: not seen, 1: seen without a point, 2: holds A, 3, 4: holds B
            if (what == 0) continue;
            const int idx = observe(w.kfs[j], tb, X, Y, Z, maxd, d, rng.uni(-0.8f, 0.8f), rng.uni(-0.8f, 0.8f), rng.below(2) == 0);
            if (what == 2 && A) link(A, w.kfs[j], idx);
            if (what >= 3) {
                if (!B) B = new_mp(w, X, Y, Z, maxd);
                link(B, w.kfs[j], idx);
            }
        }
    }
    for (int j = 0; j <= ntargets; j++)                  // features that belong to nothing
        for (int e = 0; e < nextra; e++) {
            uint8_t d[32];
            for (int k = 0; k < 32; k++) d[k] = (uint8_t)rng.next();
            w.kfs[j]->add(rng.uni(5, 635), rng.uni(5, 475), rng.below(NLEVELS), rng.below(2) ? rng.uni(0, 600) : -1.f, d);
        }
    if (hazard) {
        // P: in the current keyframe and two bystanders, stereo (6 observations), descriptor D0.  Q: in target 1 and
        // three bystanders, mono (4), descriptor D1 = D0 with 10 bits flipped.  Target 1: Q is replaced by P, whose
        // descriptor becomes D1 (4 of 7).  Target 2 sees P's place with G = D0 with 45 other bits flipped: 45 from
        // D0, 55 from D1.
        const float X = 0.4f, Y = -0.3f, Z = 5.f;
        const float maxd = std::sqrt(X * X + Y * Y + Z * Z) * 1.3f;
        uint8_t D0[32], D1[32], G[32];
        for (int k = 0; k < 32; k++) D0[k] = (uint8_t)(37 * k + 11);
        std::memcpy(D1, D0, 32); flip(D1, 0, 10);
        std::memcpy(G, D0, 32); flip(G, 100, 45);
        MapPoint* P = new_mp(w, X, Y, Z, maxd);
        MapPoint* Q = new_mp(w, X, Y, Z, maxd);
        link(P, cur, observe(cur, tb, X, Y, Z, maxd, D0, 0, 0, true));
        for (int b = 0; b < 5; b++) {
            KeyFrame* k = new_kf(w, 0.05f * (b + 1), 0.02f, 0);
            if (b < 2) link(P, k, observe(k, tb, X, Y, Z, maxd, D0, 0, 0, true));
            else link(Q, k, observe(k, tb, X, Y, Z, maxd, D1, 0, 0, false));
        }
        link(Q, w.kfs[1], observe(w.kfs[1], tb, X, Y, Z, maxd, D1, 0.3f, -0.2f, false));
        observe(w.kfs[2], tb, X, Y, Z, maxd, G, 0.2f, 0.1f, false);
    }
    for (KeyFrame* k : w.kfs) k->seal();
    for (MapPoint* m : w.mps) m->ComputeDistinctiveDescriptors();
}

// what the comparison reads of a map, by ids
static std::vector<int> dump(World& w)
{
    std::vector<int> out;
    for (KeyFrame* k : w.kfs)
        for (MapPoint* m : k->mvpMapPoints) out.push_back(m ? m->id : -1);
    for (MapPoint* m : w.mps) {
        out.push_back(m->mbBad);
        out.push_back(m->mpReplaced ? m->mpReplaced->id : -1);
        out.push_back(m->nObs);
        for (auto& o : m->mObservations) { out.push_back(o.first->id); out.push_back((int)o.second); }
        out.push_back(-7);
        for (int k = 0; k < 32; k++) out.push_back(m->mDescriptor.empty() ? -1 : m->mDescriptor.ptr<uint8_t>(0)[k]);
    }
    return out;
}

// LocalMapping.cc:507-530: the targets' points that are not yet candidates
static std::vector<MapPoint*> fuse_candidates(World& w)
{
    std::vector<MapPoint*> v;
    std::set<MapPoint*> seen;
    for (int j = 1; j <= w.ntargets; j++)
        for (MapPoint* m : w.kfs[j]->mvpMapPoints) {
            if (!m || m->isBad() || seen.count(m)) continue;
            seen.insert(m);
            v.push_back(m);
        }
    return v;
}

static int run(const std::string& mode)
{
    const bool hazard = mode != "plain";
    const Tables tb = tables();
    World a, b;
    build(a, 6, 90, 25, hazard, 5);
    build(b, 6, 90, 25, hazard, 5);
    if (dump(a) != dump(b)) return 3;
    // the host loops
    std::vector<int> nf_a;
    {
        const std::vector<MapPoint*> list = a.kfs[0]->mvpMapPoints;
        for (int j = 1; j <= a.ntargets; j++) nf_a.push_back(fuse_host(a.kfs[j], list, tb));
        nf_a.push_back(fuse_host(a.kfs[0], fuse_candidates(a), tb));
    }
    int sum = 0;
    for (int v : nf_a) sum += v;
    if (sum < 60) return 4;                              // the scene fuses
    // the adapter
    std::vector<int> nf_b;
    int calls;
    {
        coeb::KeyFrameStore<KeyFrame> store(NLEVELS, 1.2f, 400, 1);
        for (KeyFrame* k : b.kfs) store.add(k);
        KeyFrame stranger = *b.kfs[1];                   // never added: nothing fused, no call for it
        std::vector<KeyFrame*> targets(b.kfs.begin() + 1, b.kfs.begin() + 1 + b.ntargets);
        targets.insert(targets.begin() + 3, &stranger);
        const std::vector<MapPoint*> list = b.kfs[0]->mvpMapPoints;
        calls = coeb::FuseTargets(store, b.kfs[0], targets, list, 3.0f, &nf_b, mode != "norequery");
        if (nf_b[3] != 0) return 5;
        nf_b.erase(nf_b.begin() + 3);
        nf_b.push_back(coeb::Fuse(store, b.kfs[0], fuse_candidates(b)));
        if (coeb::Fuse(store, &stranger, list) != 0) return 6;
    }
    const bool same = nf_a == nf_b && dump(a) == dump(b);
    if (mode == "norequery") {
        if (same) return 7;                              // the scene does not notice the missing re-query
        if (calls != 1) return 8;
    } else {
        if (!same) {
            for (size_t j = 0; j < nf_a.size(); j++) fprintf(stderr, "nFused[%zu]: host %d adapter %d\n", j, nf_a[j], nf_b[j]);
            return 9;
        }
    }
    if (hazard) {                                        // the hazard took place: P absorbed Q and changed its descriptor
        MapPoint* P = a.mps[a.mps.size() - 2];
        MapPoint* Q = a.mps.back();
        if (!Q->mbBad || Q->mpReplaced != P || P->IsInKeyFrame(a.kfs[2]) || hamming(P->mDescriptor.ptr<uint8_t>(0), Q->mDescriptor.ptr<uint8_t>(0)))
            return 10;
    }
    printf("ok calls=%d\n", calls);
    return 0;
}

// ------------------------------------------------------------------ timing
typedef std::chrono::steady_clock Clock;
static double us_since(Clock::time_point t0) { return std::chrono::duration<double, std::micro>(Clock::now() - t0).count(); }

static void stats(std::vector<double> v, const char* name, bool last = false)
{
    std::sort(v.begin(), v.end());
    printf("\"%s\": {\"median_us\": %.1f, \"min_us\": %.1f, \"max_us\": %.1f}%s", name, v[v.size() / 2], v.front(), v.back(),
           last ? "" : ", ");
}

static int time_mode(int T)
{
    const Tables tb = tables();
    World w;
    build(w, T, 670, 500, false, 9);                     // ~1000 features per keyframe, half of them with MapPoints
    KeyFrame* cur = w.kfs[0];
    const std::vector<MapPoint*> list = cur->mvpMapPoints;
    std::vector<KeyFrame*> targets(w.kfs.begin() + 1, w.kfs.begin() + 1 + T);
    coeb::KeyFrameStore<KeyFrame> store(NLEVELS, 1.2f, 4095, 64);
    for (KeyFrame* k : w.kfs) store.add(k);
    const coeb_camera cam = coeb::fuse_camera(cur);
    const std::vector<int> zeros((size_t)T, 0), counts((size_t)T, (int)list.size());
    std::vector<std::vector<int32_t> > bi, bd;
    std::vector<Grid> grids;
    for (KeyFrame* k : targets) grids.push_back(Grid(k));    // KeyFrame::mGrid exists in the reference: not timed
    long found_host = 0, found_dev = 0, pairs = 0;
    for (KeyFrame* k : targets)
        for (MapPoint* m : list) pairs += m && !m->isBad() && !m->IsInKeyFrame(k);
    const auto host_loop = [&]() {
        long f = 0;
        for (int j = 0; j < T; j++)
            for (MapPoint* m : list) {
                if (!m || m->isBad() || m->IsInKeyFrame(targets[j])) continue;
                f += fuse_search_host(targets[j], grids[j], tb, m, 3.0f) >= 0;
            }
        return f;
    };
    const auto one_call = [&]() {
        const coeb::FusePointSnapshot snap = coeb::fuse_snapshot(list);
        coeb::FuseSearch(store, cam, snap, list, targets, zeros, counts, 3.0f, bi, bd);
    };
    const auto t_calls = [&]() {
        const coeb::FusePointSnapshot snap = coeb::fuse_snapshot(list);
        std::vector<std::vector<int32_t> > i1, d1;
        for (int j = 0; j < T; j++)
            coeb::FuseSearch(store, cam, snap, list, std::vector<KeyFrame*>(1, targets[j]), std::vector<int>(1, 0),
                             std::vector<int>(1, (int)list.size()), 3.0f, i1, d1);
    };
    one_call();                                          // builds the grids
    found_host = host_loop();
    for (int j = 0; j < T; j++)
        for (int32_t v : bi[j]) found_dev += v >= 0;
    if (found_host != found_dev) { fprintf(stderr, "host %ld device %ld matches\n", found_host, found_dev); return 11; }
    std::vector<double> th, t1, tT;
    for (int round = 0; round < 7; round++) {            // the three alternate within a round
        Clock::time_point t0 = Clock::now();
        for (int k = 0; k < 20; k++) host_loop();
        th.push_back(us_since(t0) / 20);
        t0 = Clock::now();
        for (int k = 0; k < 20; k++) one_call();
        t1.push_back(us_since(t0) / 20);
        t0 = Clock::now();
        for (int k = 0; k < 20; k++) t_calls();
        tT.push_back(us_since(t0) / 20);
    }
    // direction 2: the targets' points, deduplicated, against the current keyframe
    const std::vector<MapPoint*> cand = fuse_candidates(w);
    const Grid gcur(cur);
    std::vector<double> d2h, d2d;
    for (int round = 0; round < 7; round++) {
        Clock::time_point t0 = Clock::now();
        long f = 0;
        for (int k = 0; k < 20; k++)
            for (MapPoint* m : cand) {
                if (m->isBad() || m->IsInKeyFrame(cur)) continue;
                f += fuse_search_host(cur, gcur, tb, m, 3.0f) >= 0;
            }
        d2h.push_back(us_since(t0) / 20);
        t0 = Clock::now();
        for (int k = 0; k < 20; k++) {
            const coeb::FusePointSnapshot snap = coeb::fuse_snapshot(cand);
            coeb::FuseSearch(store, cam, snap, cand, std::vector<KeyFrame*>(1, cur), std::vector<int>(1, 0),
                             std::vector<int>(1, (int)cand.size()), 3.0f, bi, bd);
        }
        d2d.push_back(us_since(t0) / 20);
        if (f < 0) return 12;
    }
    // device time per kernel by HIP events, in rounds of their own
    coeb_profile_enable(store.ctx(), 1);
    std::vector<double> kf;
    for (int round = 0; round < 7; round++) {
        coeb_profile_reset(store.ctx());
        for (int k = 0; k < 20; k++) one_call();
        char names[4096];
        double ms[64];
        int64_t launches[64];
        int nk = 0;
        coeb_profile_read(store.ctx(), names, sizeof(names), ms, launches, 64, &nk);
        int i = 0;
        for (char* tok = strtok(names, ","); tok && i < nk; tok = strtok(nullptr, ","), i++)
            if (!strcmp(tok, "k_fuse") && launches[i]) kf.push_back(ms[i] * 1000.0 / (double)launches[i]);
    }
    coeb_profile_enable(store.ctx(), 0);
    printf("{\"targets\": %d, \"list\": %zu, \"pairs_searched\": %ld, \"matches\": %ld, \"features_per_keyframe\": %zu, "
           "\"direction2_candidates\": %zu, ", T, list.size(), pairs, found_host, targets[0]->mvKeysUn.size(), cand.size());
    stats(th, "host_loop_search");
    stats(t1, "one_call_with_snapshot");
    stats(tT, "one_job_calls");
    stats(d2h, "direction2_host_loop");
    stats(d2d, "direction2_one_call");
    if (kf.empty()) kf.push_back(0);
    stats(kf, "k_fuse_device", true);
    printf("}\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    try {
        if (mode == "time") return time_mode(argc > 2 ? atoi(argv[2]) : 10);
        return run(mode);
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
