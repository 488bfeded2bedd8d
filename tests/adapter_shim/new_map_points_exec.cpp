// Runs coeb::KeyFrameStore and coeb::CreateNewMapPointsNeighbors (adapter/LocalMapping_coeb.h) against
// libcoeb_front.so on the GPU, with the reference-shaped KeyFrame of new_map_points_types.h.
//
//   new_map_points_exec DIR
//
// DIR holds what tests/test_adapter_newpts.py writes: counts.i32 (features per keyframe), desc.u8, node.i32,
// keys.f32 ([x, y, uRight, raw x, raw y, depth] per feature), octave.i32, has_mp.u8 (all concatenated over the
// keyframes), view.f32 (per keyframe the 23 floats of coeb_kf_view) and F12.f32 ([neighbour][9]).  Every
// keyframe enters a KeyFrameStore of one slot (it grows), keyframe 3 leaves and enters again, and keyframe 0
// goes against keyframes 1 .. n-1 with one keyframe the store has never seen in between.  DIR receives
// pairs.i32 ([neighbour, idx1, idx2] in the order of `new MapPoint`) and x3d.f32 ([3] per pair).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "new_map_points_types.h"

#include "LocalMapping_coeb.h"

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
    const std::vector<int32_t> octave = load<int32_t>(dir + "/octave.i32");
    const std::vector<uint8_t> desc = load<uint8_t>(dir + "/desc.u8"), has_mp = load<uint8_t>(dir + "/has_mp.u8");
    const std::vector<float> keys = load<float>(dir + "/keys.f32"), view = load<float>(dir + "/view.f32");
    const std::vector<float> F12 = load<float>(dir + "/F12.f32");
    const int nkf = (int)counts.size();
    if (nkf < 5 || (int)view.size() != nkf * 23 || (int)F12.size() != (nkf - 1) * 9) return 3;
    static MapPoint some_point;
    std::vector<KeyFrame> kfs((size_t)nkf);
    size_t at = 0;
    for (int k = 0; k < nkf; k++) {
        KeyFrame& kf = kfs[k];
        const int n = counts[k];
        kf.mDescriptors = cv::Mat(n, 32, CV_8U);
        if (n) std::memcpy(kf.mDescriptors.ptr<uint8_t>(0), desc.data() + at * 32, (size_t)n * 32);
        kf.mvKeysUn.resize((size_t)n);
        kf.mvKeys.resize((size_t)n);
        for (int i = 0; i < n; i++) {
            const float* q = keys.data() + (at + i) * 6;
            kf.mvKeysUn[i].pt = cv::Point2f(q[0], q[1]);
            kf.mvKeysUn[i].octave = octave[at + i];
            kf.mvKeys[i].pt = cv::Point2f(q[3], q[4]);
            kf.mvKeys[i].octave = octave[at + i];
            kf.mvuRight.push_back(q[2]);
            kf.mvDepth.push_back(q[5]);
            kf.mvpMapPoints.push_back(has_mp[at + i] ? &some_point : nullptr);
            if (node[at + i] >= 0) kf.mFeatVec.addFeature((unsigned int)node[at + i], (unsigned int)i);
        }
        at += (size_t)n;
        const float* p = view.data() + (size_t)k * 23;
        kf.R = fmat(p, 3, 3); kf.t = fmat(p + 9, 3, 1); kf.Ow = fmat(p + 12, 3, 1);
        kf.fx = p[15]; kf.fy = p[16]; kf.cx = p[17]; kf.cy = p[18];
        kf.invfx = p[19]; kf.invfy = p[20]; kf.mb = p[21]; kf.mbf = p[22];
    }
    {
        coeb::KeyFrameStore<KeyFrame> store(8, 1.2f, 1000, 1);
        for (int k = 0; k < nkf; k++) store.add(&kfs[k]);
        store.erase(&kfs[3]);
        store.add(&kfs[3]);                                  // the freed slot again, with geometry and stereo data
        KeyFrame stranger = kfs[1];
        std::vector<KeyFrame*> vpKF2;
        std::vector<cv::Mat> vF12;
        for (int k = 1; k < nkf; k++) {
            vpKF2.push_back(&kfs[k]);
            vF12.push_back(fmat(F12.data() + (size_t)(k - 1) * 9, 3, 3));
        }
        vpKF2.insert(vpKF2.begin() + 2, &stranger);          // not in the store: no pairs
        vF12.insert(vF12.begin() + 2, vF12[0]);
        std::vector<std::vector<coeb::NewMapPointPair> > vvNew;
        const int total = coeb::CreateNewMapPointsNeighbors(store, &kfs[0], vpKF2, vF12, vvNew);
        if (vvNew.size() != vpKF2.size() || !vvNew[2].empty()) return 5;
        vvNew.erase(vvNew.begin() + 2);
        std::vector<int32_t> pairs;
        std::vector<float> x3d;
        std::vector<uint8_t> seen((size_t)counts[0], 0);
        for (int j = 0; j < nkf - 1; j++) {
            for (size_t q = 0; q < vvNew[j].size(); q++) {
                const coeb::NewMapPointPair& p = vvNew[j][q];
                if (q && p.idx1 <= vvNew[j][q - 1].idx1) return 6;      // ascending idx1
                if (seen[p.idx1]) return 7;                              // one MapPoint per feature of keyframe 1
                seen[p.idx1] = 1;
                pairs.push_back(j); pairs.push_back((int32_t)p.idx1); pairs.push_back((int32_t)p.idx2);
                x3d.insert(x3d.end(), p.x3D, p.x3D + 3);
            }
        }
        if ((int)pairs.size() != 3 * total) return 8;
        save(dir + "/pairs.i32", pairs);
        save(dir + "/x3d.f32", x3d);
        store.erase(&kfs[0]);
        try {
            coeb::CreateNewMapPointsNeighbors(store, &kfs[0], vpKF2, vF12, vvNew);
            return 9;                                        // pKF1 has left the store
        } catch (const std::runtime_error&) {
        }
    }
    printf("ok\n");
    return 0;
}
