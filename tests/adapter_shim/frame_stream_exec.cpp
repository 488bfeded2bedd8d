// Runs coeb::FrameRGBDStream (coeb-slam_amd/adapter/Frame_coeb.h), what the reference's RGB-D Frame
// constructor (src/Frame.cc:157-223) collapses to on a stream of frames, against libcoeb_front.so on
// the GPU, with a reference-shaped Frame and the cv stand-in of tests/adapter_shim/opencv2.  Built
// and run by tests/test_adapter_stream.py.
//
//   frame_stream_exec DIR
//
//   in : size.i32 (W, H, frames >= 6, boxes per frame), frames.u8, depth.f32 (W*H), cam.f32 (fx fy cx cy bf),
//        dist.f32 (k1 k2 p1 p2 k3), boxes.f32 (frames x boxes x 4)
//   out, per step TAG: TAG.kps.bin, TAG.kps_un.bin, TAG.desc.u8, TAG.ur.f32, TAG.dep.f32, TAG.tm.f32,
//        TAG.blur.i32, TAG.n.i32.  Steps: f0 f1 f2 f3 (four frames in a row), then coeb::FrameStreamReset
//        (Tracking::Reset), r4 r5 (frame 4 is a first frame, frame 5 pairs with it), then frame 4 through
//        a SECOND extractor (the adaptive nFeatures switch; b4) and frame 5 through the first again (s5:
//        a first frame, its predecessor went to the other extractor).  checks.txt: the empty-image rule.
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "ORBextractor.h"
#include "Frame_coeb.h"

struct Frame {
    cv::Mat mK, mDistCoef, mDescriptors;
    float mbf = 0;
    int N = 0;
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    std::vector<float> mvuRight, mvDepth;
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
static void save(const std::string& path, const T* p, size_t n)
{
    std::ofstream f(path, std::ios::binary);
    f.write(reinterpret_cast<const char*>(p), (std::streamsize)(n * sizeof(T)));
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::cerr << "usage: frame_stream_exec DIR\n"; return 2; }
    const std::string d = std::string(argv[1]) + "/";
    const std::vector<int32_t> size = load<int32_t>(d + "size.i32");
    const int W = size[0], H = size[1], NF = size[2], NB = size[3];
    std::vector<uint8_t> frames = load<uint8_t>(d + "frames.u8");
    std::vector<float> depth = load<float>(d + "depth.f32");
    const std::vector<float> cam = load<float>(d + "cam.f32"), dist = load<float>(d + "dist.f32");
    const std::vector<float> boxes = load<float>(d + "boxes.f32");
    if (NF < 6 || frames.size() != (size_t)W * H * NF || depth.size() != (size_t)W * H || cam.size() != 5 ||
        dist.size() != 5 || boxes.size() != (size_t)NF * NB * 4) {
        std::cerr << "bad input sizes\n";
        return 2;
    }

    Frame F0;
    F0.mK = cv::Mat(3, 3, CV_32F);
    std::memset(F0.mK.data, 0, 9 * sizeof(float));
    F0.mK.at<float>(0, 0) = cam[0]; F0.mK.at<float>(1, 1) = cam[1]; F0.mK.at<float>(0, 2) = cam[2];
    F0.mK.at<float>(1, 2) = cam[3]; F0.mK.at<float>(2, 2) = 1.0f;
    F0.mbf = cam[4];
    F0.mDistCoef = cv::Mat(5, 1, CV_32F);
    for (int i = 0; i < 5; i++) F0.mDistCoef.at<float>(i) = dist[i];

    ORB_SLAM2::ORBextractor exA(1000, 1.2f, 8, 20, 7), exB(1500, 1.2f, 8, 20, 7);
    cv::Mat imDepth(H, W, CV_32F, depth.data());
    // the constructor for frame f through extractor ex; the outputs saved under tag
    auto step = [&](ORB_SLAM2::ORBextractor* ex, int f, const std::string& tag) {
        Frame F = F0;
        std::vector<std::vector<float>> box;
        for (int b = 0; b < NB; b++) {
            const float* q = &boxes[((size_t)f * NB + b) * 4];
            box.push_back(std::vector<float>(q, q + 4));
        }
        std::vector<cv::Point2f> tm(3, cv::Point2f(-1.f, -1.f));      // stale content the call must replace
        std::vector<int> blur(7, 9);
        cv::Mat imGray(H, W, CV_8U, frames.data() + (size_t)f * W * H);
        coeb::FrameRGBDStream(F, ex, imGray, imDepth, box, tm, blur);
        const std::string t = d + tag + ".";
        save(t + "kps.bin", F.mvKeys.data(), F.mvKeys.size());
        save(t + "kps_un.bin", F.mvKeysUn.data(), F.mvKeysUn.size());
        save(t + "desc.u8", F.mDescriptors.data, (size_t)F.mDescriptors.rows * 32);
        save(t + "ur.f32", F.mvuRight.data(), F.mvuRight.size());
        save(t + "dep.f32", F.mvDepth.data(), F.mvDepth.size());
        save(t + "tm.f32", reinterpret_cast<const float*>(tm.data()), tm.size() * 2);
        save(t + "blur.i32", blur.data(), blur.size());
        save(t + "n.i32", &F.N, 1);
    };
    for (int f = 0; f < 3; f++) step(&exA, f, "f" + std::to_string(f));

    std::ofstream checks(d + "checks.txt");
    {   // empty image: return without touching the outputs (ORBextractor.cc:1096-1097) or the stream
        Frame G = F0;
        G.mvKeys.resize(3);
        G.mvKeys[0].octave = 77;
        std::vector<std::vector<float>> box;
        std::vector<cv::Point2f> tm(2, cv::Point2f(4.f, 5.f));
        std::vector<int> blur(1, 3);
        cv::Mat empty;
        coeb::FrameRGBDStream(G, &exA, empty, imDepth, box, tm, blur);
        checks << "empty_untouched " << (G.mvKeys.size() == 3 && G.mvKeys[0].octave == 77 && tm.size() == 2 && blur.size() == 1 && G.N == 3)
               << "\n";
    }
    step(&exA, 3, "f3");                            // still pairs with frame 2
    coeb::FrameStreamReset(&exA);                   // Tracking::Reset
    step(&exA, 4, "r4");
    step(&exA, 5, "r5");
    step(&exB, 4, "b4");                            // the adaptive nFeatures switch: another extractor takes a frame
    step(&exA, 5, "s5");
    std::cout << "frame_stream_exec: done\n";
    return 0;
}
