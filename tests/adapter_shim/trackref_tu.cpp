// Compile check of adapter/Tracking_coeb.h's TrackReferenceKeyFrame against reference-shaped
// Frame / KeyFrame / MapPoint types (include/Frame.h, include/KeyFrame.h, include/MapPoint.h
// member names and types) and stand-ins for DBoW2's two containers.
#include <map>

#include "Tracking_coeb.h"

struct BowVector : std::map<unsigned int, double> {
    void addWeight(unsigned int id, double v) { (*this)[id] += v; }
};
struct FeatureVector : std::map<unsigned int, std::vector<unsigned int>> {
    void addFeature(unsigned int id, unsigned int i) { (*this)[id].push_back(i); }
};
struct MapPoint {
    cv::Mat GetWorldPos() { return cv::Mat(); }
    int Observations() { return 2; }
    bool isBad() { return false; }
    bool mbTrackInView = false;
    long unsigned int mnLastFrameSeen = 0;
    static std::mutex mGlobalMutex;
};
std::mutex MapPoint::mGlobalMutex;
struct KeyFrame {
    std::vector<MapPoint*> GetMapPointMatches() { return std::vector<MapPoint*>(); }
    std::vector<cv::KeyPoint> mvKeysUn;
    cv::Mat mDescriptors;
    FeatureVector mFeatVec;
};
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
    BowVector mBowVec;
    FeatureVector mFeatVec;
    void SetPose(cv::Mat Tcw) { mTcw = Tcw; }
};
float Frame::fx, Frame::fy, Frame::cx, Frame::cy, Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;

bool use_trackref_adapter(Frame& F, KeyFrame* pRefKF, Frame& mLastFrame, coeb::Vocabulary& voc)
{
    int nmatchesMap = 0;
    return coeb::TrackReferenceKeyFrame(F, pRefKF, mLastFrame.mTcw, voc) &&
           coeb::TrackReferenceKeyFrame(F, pRefKF, mLastFrame.mTcw, voc, 0.7f, true, 4, &nmatchesMap);
}
