// Compile check of adapter/Tracking_coeb.h against reference-shaped Frame / MapPoint types
// (include/Frame.h, include/MapPoint.h member names and types; the two distance getters are the
// ones INTEGRATION.md s3 adds).
#include "Tracking_coeb.h"

struct MapPoint {
    cv::Mat GetWorldPos() { return cv::Mat(); }
    cv::Mat GetNormal() { return cv::Mat(); }
    cv::Mat GetDescriptor() { return cv::Mat(); }
    int Observations() { return 2; }
    bool isBad() { return false; }
    void IncreaseVisible(int n = 1) { (void)n; }
    void IncreaseFound(int n = 1) { (void)n; }
    float GetMaxDistance() { return 0; }
    float GetMinDistance() { return 0; }
    bool mbTrackInView = false;
    float mTrackProjX = 0, mTrackProjY = 0, mTrackProjXR = 0;
    int mnTrackScaleLevel = 0;
    float mTrackViewCos = 0;
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
    std::vector<float> mvuRight;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    cv::Mat mDescriptors, mTcw;
    void SetPose(cv::Mat Tcw) { mTcw = Tcw; }
};
float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;

int use_tracking_adapter(Frame& F, std::vector<MapPoint*>& vpLocalMapPoints, bool mbOnlyTracking)
{
    return coeb::SearchLocalPoints(F, vpLocalMapPoints, 3.0f, 0.8f) +
           coeb::TrackLocalMap(F, vpLocalMapPoints, 3.0f, 0.8f, mbOnlyTracking) +
           coeb::TrackLocalMap(F, vpLocalMapPoints, 1.0f, 0.8f, mbOnlyTracking, true);
}
