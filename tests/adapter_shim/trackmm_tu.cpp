// Compile check of adapter/Tracking_coeb.h's TrackWithMotionModel against reference-shaped Frame /
// MapPoint types (include/Frame.h, include/MapPoint.h member names and types), std::list as
// mlpTemporalPoints and a factory lambda as the reference's `new MapPoint(x3D, mpMap, &mLastFrame, i)`.
#include <list>

#include "Tracking_coeb.h"

namespace cv
{
Mat operator*(const Mat& a, const Mat& b);
}
struct MapPoint {
    cv::Mat GetWorldPos() { return cv::Mat(); }
    cv::Mat GetDescriptor() { return cv::Mat(); }
    int Observations() { return 2; }
    bool mbTrackInView = false;
    long unsigned int mnLastFrameSeen = 0;
    static std::mutex mGlobalMutex;
};
std::mutex MapPoint::mGlobalMutex;
struct Frame {
    static float fx, fy, cx, cy, mnMinX, mnMaxX, mnMinY, mnMaxY;
    long unsigned int mnId = 0;
    float mbf = 0, mb = 0;
    int N = 0;
    int mnScaleLevels = 8;
    float mfScaleFactor = 1.2f;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight, mvDepth;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    cv::Mat mDescriptors, mTcw;
    void SetPose(cv::Mat Tcw) { mTcw = Tcw; }
};
float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;

bool use_trackmm_adapter(Frame& mCurrentFrame, Frame& mLastFrame, const cv::Mat& mVelocity, bool mbOnlyTracking,
                         float mThDepth, std::list<MapPoint*>& mlpTemporalPoints, bool& mbVO)
{
    auto newPoint = [&](const cv::Mat&, int) { return new MapPoint(); };
    int nmatchesMap = 0;
    return coeb::TrackWithMotionModel(mCurrentFrame, mLastFrame, mVelocity, 15, false, mbOnlyTracking, mbOnlyTracking,
                                      mThDepth, newPoint, mlpTemporalPoints, &mbVO) &&
           coeb::TrackWithMotionModel(mCurrentFrame, mLastFrame, mVelocity, 7, true, false, false, mThDepth, newPoint,
                                      mlpTemporalPoints, nullptr, false, &nmatchesMap);
}
