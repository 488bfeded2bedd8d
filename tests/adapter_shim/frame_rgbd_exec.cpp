// Runs coeb::FrameRGBD (coeb-slam_amd/adapter/Frame_coeb.h), what the reference's RGB-D Frame
// constructor tail (src/Frame.cc:214-223) collapses to, against libcoeb_front.so on the GPU, with
// a reference-shaped Frame (include/Frame.h member names) and the cv stand-in of
// tests/adapter_shim/opencv2.  Built and run by tests/test_gpu_frame_rgbd.py; the compile-only
// check of tests/test_frame_rgbd_host.py needs no GPU.
//
//   frame_rgbd_exec DIR
//
//   in : size.i32 (W, H), frame.u8 (W*H gray), depth.f32 (W*H), cam.f32 (fx fy cx cy bf),
//        dist.f32 (k1 k2 p1 p2 k3)
//   out: kps.bin, kps_un.bin (cv::KeyPoint records), desc.u8, ur.f32, dep.f32, n.i32 (Frame::N),
//        checks.txt (the conventions of ORBextractor::operator(): empty image, zero keypoints)
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
    if (argc != 2) { std::cerr << "usage: frame_rgbd_exec DIR\n"; return 2; }
    const std::string d = std::string(argv[1]) + "/";
    const std::vector<int32_t> size = load<int32_t>(d + "size.i32");
    const int W = size[0], H = size[1];
    std::vector<uint8_t> gray = load<uint8_t>(d + "frame.u8");
    std::vector<float> depth = load<float>(d + "depth.f32");
    const std::vector<float> cam = load<float>(d + "cam.f32"), dist = load<float>(d + "dist.f32");
    if (gray.size() != (size_t)W * H || depth.size() != (size_t)W * H || cam.size() != 5 || dist.size() != 5) {
        std::cerr << "bad input sizes\n";
        return 2;
    }

    Frame F;
    F.mK = cv::Mat(3, 3, CV_32F);
    std::memset(F.mK.data, 0, 9 * sizeof(float));
    F.mK.at<float>(0, 0) = cam[0]; F.mK.at<float>(1, 1) = cam[1]; F.mK.at<float>(0, 2) = cam[2];
    F.mK.at<float>(1, 2) = cam[3]; F.mK.at<float>(2, 2) = 1.0f;
    F.mbf = cam[4];
    F.mDistCoef = cv::Mat(5, 1, CV_32F);
    for (int i = 0; i < 5; i++) F.mDistCoef.at<float>(i) = dist[i];

    ORB_SLAM2::ORBextractor ex(1000, 1.2f, 8, 20, 7);
    std::vector<std::vector<float>> box;
    std::vector<cv::Point2f> tm;
    std::vector<int> blur;
    cv::Mat imGray(H, W, CV_8U, gray.data()), imDepth(H, W, CV_32F, depth.data());
    coeb::FrameRGBD(F, &ex, imGray, imDepth, box, tm, blur);
    save(d + "kps.bin", F.mvKeys.data(), F.mvKeys.size());
    save(d + "kps_un.bin", F.mvKeysUn.data(), F.mvKeysUn.size());
    save(d + "desc.u8", F.mDescriptors.data, (size_t)F.mDescriptors.rows * 32);
    save(d + "ur.f32", F.mvuRight.data(), F.mvuRight.size());
    save(d + "dep.f32", F.mvDepth.data(), F.mvDepth.size());
    save(d + "n.i32", &F.N, 1);

    std::ofstream checks(d + "checks.txt");
    {   // empty image: return without touching the outputs (ORBextractor.cc:1096-1097)
        Frame G = F;
        G.mvKeys.resize(3);
        G.mvKeys[0].octave = 77;
        G.mvuRight.assign(3, 5.0f);
        cv::Mat empty;
        coeb::FrameRGBD(G, &ex, empty, imDepth, box, tm, blur);
        checks << "empty_untouched " << (G.mvKeys.size() == 3 && G.mvKeys[0].octave == 77 && G.mvuRight.size() == 3 &&
                                         G.mDescriptors.rows == F.mDescriptors.rows && G.N == 3)
               << "\n";
    }
    {   // no keypoints: descriptors.release() (:1296-1297), every vector empty, N = 0
        std::vector<uint8_t> flat((size_t)W * H, 128);
        cv::Mat im(H, W, CV_8U, flat.data());
        Frame G = F;
        coeb::FrameRGBD(G, &ex, im, imDepth, box, tm, blur);
        checks << "flat_released " << (G.mvKeys.empty() && G.mvKeysUn.empty() && G.mvuRight.empty() && G.mvDepth.empty() &&
                                       G.mDescriptors.empty() && G.N == 0)
               << "\n";
    }
    std::cout << "frame_rgbd_exec: " << F.N << " keypoints\n";
    return 0;
}
