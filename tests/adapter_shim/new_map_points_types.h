// Reference-shaped stand-ins for tests/adapter_shim/new_map_points_exec.cpp: the KeyFrame of
// local_mapping_exec.cpp with what CreateNewMapPoints' loop reads besides -- mvKeys, mvDepth, invfx, invfy,
// mb, mbf -- and the two cv::Mat expressions of ORBmatcher.cc:667 the stand-in Mat lacks.
#ifndef COEB_SHIM_NEW_MAP_POINTS_TYPES_H
#define COEB_SHIM_NEW_MAP_POINTS_TYPES_H
#include <map>
#include <vector>

#include <opencv2/core/core.hpp>

namespace cv {
// float, in element order
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

struct FeatureVector : std::map<unsigned int, std::vector<unsigned int>> {
    void addFeature(unsigned int id, unsigned int i) { (*this)[id].push_back(i); }
};
struct MapPoint {};
struct KeyFrame {
    std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
    std::vector<float> mvuRight, mvDepth;
    cv::Mat mDescriptors;
    FeatureVector mFeatVec;
    std::vector<MapPoint*> mvpMapPoints;
    MapPoint* GetMapPoint(const size_t& idx) { return mvpMapPoints[idx]; }
    cv::Mat R, t, Ow;
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    cv::Mat GetRotation() { return R.clone(); }
    cv::Mat GetTranslation() { return t.clone(); }
    float fx = 0, fy = 0, cx = 0, cy = 0, invfx = 0, invfy = 0, mb = 0, mbf = 0;
};
#endif
