/*
 * ORBextractor.h -- drop-in replacement of COEB-SLAM's include/ORBextractor.h backed by the
 * MI355X HIP front end (include/coeb_front.h).
 *
 * Same class name, namespace, constructor, operator() and accessors as the reference
 * (include/ORBextractor.h:44-128), so src/Frame.cc:413-419 (ExtractORB) and
 * src/Tracking.cc:115-120 compile unchanged.  Header-only; link libcoeb_front.so.
 *
 *   ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)    ORBextractor.h:50-51
 *   operator()(image, mask, img, imD, keypoints, descriptors, box, T_M,
 *              mask_result, blur_flag)                                     ORBextractor.h:73-75
 *   GetLevels / GetScaleFactor / GetScaleFactors / GetInverseScaleFactors /
 *   GetScaleSigmaSquares / GetInverseScaleSigmaSquares                     ORBextractor.h:77-99
 *   ExtractRGBD(...)  (an addition: the Frame RGB-D ctor tail, Frame.cc:214-223, in one call;
 *                      coeb::FrameRGBD of Frame_coeb.h wraps it)
 *   ExtractRGBDStream(...)  (an addition: the whole RGB-D ctor, Frame.cc:157-223, on the frame stream
 *                      that lives with the pooled context; coeb::FrameRGBDStream wraps it)
 *
 * Behaviour kept from the reference: empty image -> return without touching the outputs
 * (:1096-1097); non-8UC1 -> assert (:1099); zero keypoints -> descriptors.release()
 * (:1296-1297); mask / img / imD / mask_result are accepted and unused (SURVEY.md s8a note).
 * Device contexts are pooled per (host thread, device, parameters) so Tracking's leak-and-recreate
 * of extractors on tracking failure (Tracking.cc:434-465) stays cheap; a context grows to the
 * largest image it has seen (no fixed size cap) and is freed when its thread exits.
 */
#ifndef COEB_ADAPTER_ORBEXTRACTOR_H
#define COEB_ADAPTER_ORBEXTRACTOR_H

#include <algorithm>
#include <cassert>
#include <cstdlib>
#include <cstring>
#include <list>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include <opencv2/core/core.hpp>
#include <opencv2/features2d/features2d.hpp>

#include "coeb_front.h"

namespace ORB_SLAM2
{

class ExtractorNode   // kept for source compatibility (unused by the GPU path)
{
public:
    ExtractorNode() : bNoMore(false) {}
    std::vector<cv::KeyPoint> vKeys;
    cv::Point2i UL, UR, BL, BR;
    std::list<ExtractorNode>::iterator lit;
    bool bNoMore;
};

namespace coeb_detail
{
// One context per (host thread, device, ORB parameters): coeb_ctx is not reentrant.  The pool
// is thread_local and destroys its contexts when the thread exits, so thread churn frees device
// memory.  A context is created for at least 1280 x 960 and re-created larger when an image
// exceeds it; extractors therefore look their context up per call instead of caching it.
// A context carries the coeb_rgbd_stream of ExtractRGBDStream (created on first use): the stream
// holds the previous frame for this thread's extractors with these parameters.  It is destroyed
// before its context, always; a context re-created larger starts with a fresh stream.
struct CtxPool {
    typedef std::tuple<int, int, float, int, int, int> Key;
    struct Entry { coeb_ctx* ctx; int max_w, max_h; coeb_rgbd_stream* stream; int sw, sh; };
    std::map<Key, Entry> m;
    Key last_stream;                // whose stream took the last frame (has_last: any did)
    bool has_last = false;
    static void drop(Entry& e)
    {
        if (e.stream) coeb_rgbd_stream_destroy(e.stream);
        e.stream = nullptr;
        coeb_destroy(e.ctx);
    }
    ~CtxPool()
    {
        for (auto& kv : m) drop(kv.second);
    }
};

inline CtxPool& ctx_pool()
{
    thread_local CtxPool pool;
    return pool;
}

inline CtxPool::Key pool_key(const coeb_orb_params& p, int device)
{
    return std::make_tuple(device, p.nfeatures, p.scale_factor, p.nlevels, p.ini_th_fast, p.min_th_fast);
}

inline coeb_ctx* pooled_context(const coeb_orb_params& p, int device, int w, int h)
{
    CtxPool& pool = ctx_pool();
    const auto key = pool_key(p, device);
    auto it = pool.m.find(key);
    if (it != pool.m.end() && w <= it->second.max_w && h <= it->second.max_h) return it->second.ctx;
    int mw = std::max(w, 1280), mh = std::max(h, 960);
    if (it != pool.m.end()) {               // grow: keep the larger of the old and new bounds
        mw = std::max(mw, it->second.max_w);
        mh = std::max(mh, it->second.max_h);
        CtxPool::drop(it->second);
        pool.m.erase(it);
    }
    if (coeb_abi_version() != COEB_ABI_VERSION)      // header and loaded library must agree
        throw std::runtime_error("libcoeb_front ABI " + std::to_string(coeb_abi_version()) + ", header " +
                                 std::to_string(COEB_ABI_VERSION));
    coeb_ctx* c = coeb_create(&p, device, mw, mh, 1);
    if (!c) throw std::runtime_error(std::string("coeb_create: ") + coeb_last_error(nullptr));
    pool.m[key] = CtxPool::Entry{c, mw, mh, nullptr, 0, 0};
    return c;
}

// The frame stream of the pooled context for a w x h frame, ready to take it.  The next frame is a
// first frame (no imGrayPre, as in a new process) when the stream is new, when the frame size
// changed, and when the last frame of this thread went to another extractor's stream (Tracking's
// adaptive nFeatures switch, Tracking.cc:434-465): a stream never pairs a frame with one that was
// not the frame before it.
inline coeb_rgbd_stream* pooled_stream(const coeb_orb_params& p, int device, int w, int h, coeb_ctx** ctx_out)
{
    coeb_ctx* c = pooled_context(p, device, w, h);
    CtxPool& pool = ctx_pool();
    const auto key = pool_key(p, device);
    CtxPool::Entry& e = pool.m[key];
    if (!e.stream && coeb_rgbd_stream_create(c, 0, &e.stream) != COEB_OK) throw std::runtime_error(coeb_last_error(c));
    const bool switched = pool.has_last && pool.last_stream != key;
    if (switched || e.sw != w || e.sh != h) coeb_rgbd_stream_reset(e.stream);
    e.sw = w; e.sh = h;
    pool.last_stream = key;
    pool.has_last = true;
    *ctx_out = c;
    return e.stream;
}

// Tracking::Reset (on the tracking thread): every stream of this thread starts over
inline void reset_streams()
{
    CtxPool& pool = ctx_pool();
    for (auto& kv : pool.m)
        if (kv.second.stream) coeb_rgbd_stream_reset(kv.second.stream);
    pool.has_last = false;
}
}  // namespace coeb_detail

class ORBextractor
{
public:
    enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };

    ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST)
        : nfeatures(nfeatures), scaleFactor(scaleFactor), nlevels(nlevels), iniThFAST(iniThFAST),
          minThFAST(minThFAST)
    {
        params_.nfeatures = nfeatures;
        params_.scale_factor = scaleFactor;
        params_.nlevels = nlevels;
        params_.ini_th_fast = iniThFAST;
        params_.min_th_fast = minThFAST;
        coeb_ctx* ctx = coeb_detail::pooled_context(params_, device(), 0, 0);
        coeb_orb_tables t;
        if (coeb_orb_tables_get(ctx, &t) != COEB_OK) throw std::runtime_error(coeb_last_error(ctx));
        mvScaleFactor.assign(t.scale, t.scale + nlevels);
        mvInvScaleFactor.assign(t.inv_scale, t.inv_scale + nlevels);
        mvLevelSigma2.assign(t.sigma2, t.sigma2 + nlevels);
        mvInvLevelSigma2.assign(t.inv_sigma2, t.inv_sigma2 + nlevels);
        mnFeaturesPerLevel.assign(t.features_per_level, t.features_per_level + nlevels);
        umax.assign(t.umax, t.umax + 16);
        mvImagePyramid.resize(nlevels);
    }

    ~ORBextractor() {}

    void operator()(cv::InputArray _image, cv::InputArray /*mask*/, const cv::Mat& /*img*/, const cv::Mat& /*imD*/,
                    std::vector<cv::KeyPoint>& _keypoints, cv::OutputArray _descriptors,
                    std::vector<std::vector<float>>& box, std::vector<cv::Point2f> T_M, cv::Mat& /*mask_result*/,
                    std::vector<int> blur_flag)
    {
        if (_image.empty()) return;
        cv::Mat image = _image.getMat();
        assert(image.type() == CV_8UC1);
        std::vector<coeb_box> boxes;
        for (const auto& b : box) boxes.push_back(coeb_box{b[0], b[1], b[2], b[3]});
        std::vector<float> tm;
        for (const auto& p : T_M) { tm.push_back(p.x); tm.push_back(p.y); }
        coeb_ctx* ctx_ = coeb_detail::pooled_context(params_, device(), image.cols, image.rows);
        const int cap = coeb_max_keypoints(ctx_, image.cols, image.rows);
        if (cap < 0) throw std::runtime_error(coeb_last_error(ctx_));
        std::vector<coeb_keypoint> kps((size_t)cap);
        cv::Mat desc((int)cap, 32, CV_8U);
        int n = 0;
        const int rc = coeb_extract(ctx_, image.data, image.cols, image.rows, image.step[0],
                                    boxes.empty() ? nullptr : boxes.data(), (int)boxes.size(),
                                    tm.empty() ? nullptr : tm.data(), (int)T_M.size(),
                                    blur_flag.empty() ? nullptr : blur_flag.data(), (int)blur_flag.size(),
                                    kps.data(), desc.data, cap, &n);
        if (rc != COEB_OK) throw std::runtime_error(coeb_last_error(ctx_));
        _keypoints.resize((size_t)n);
        static_assert(sizeof(coeb_keypoint) == sizeof(cv::KeyPoint), "coeb_keypoint must mirror cv::KeyPoint");
        // cv::KeyPoint is trivially copyable and layout-identical to coeb_keypoint (static_assert above)
        if (n) std::memcpy(static_cast<void*>(&_keypoints[0]), kps.data(), sizeof(coeb_keypoint) * (size_t)n);
        if (n == 0) {
            _descriptors.release();
        } else {
            _descriptors.create(n, 32, CV_8U);
            desc.rowRange(0, n).copyTo(_descriptors.getMat());
        }
    }

    // The RGB-D Frame constructor's tail (Frame.cc:214-223) in one device call (coeb_frame_rgbd):
    // operator() as above, mvKeysUn = UndistortKeyPoints (:579-609) with K and distCoef (4 or 5
    // CV_32F coefficients; distCoef(0) == 0 copies), and ComputeStereoFromRGBD (:820-842): depth
    // at the raw keypoint, uRight from the undistorted x.  imDepth is the CV_32F map
    // Tracking::GrabImageRGBD converted (Tracking.cc:227).  Same conventions as operator(): an
    // empty image returns without touching the outputs, zero keypoints release the descriptors.
    void ExtractRGBD(const cv::Mat& imGray, const cv::Mat& imDepth, const cv::Mat& K, const cv::Mat& distCoef, float bf,
                     std::vector<std::vector<float>>& box, const std::vector<cv::Point2f>& T_M,
                     const std::vector<int>& blur_flag, std::vector<cv::KeyPoint>& mvKeys, cv::Mat& mDescriptors,
                     std::vector<cv::KeyPoint>& mvKeysUn, std::vector<float>& mvuRight, std::vector<float>& mvDepth)
    {
        if (imGray.empty()) return;
        assert(imGray.type() == CV_8UC1);
        if (imDepth.empty() || imDepth.type() != CV_32F || imDepth.rows != imGray.rows || imDepth.cols != imGray.cols)
            throw std::invalid_argument("ORBextractor::ExtractRGBD: a CV_32F depth map of the image's size expected");
        std::vector<coeb_box> boxes;
        for (const auto& b : box) boxes.push_back(coeb_box{b[0], b[1], b[2], b[3]});
        std::vector<float> tm;
        for (const auto& p : T_M) { tm.push_back(p.x); tm.push_back(p.y); }
        coeb_camera cam{};
        cam.fx = K.at<float>(0, 0); cam.fy = K.at<float>(1, 1); cam.cx = K.at<float>(0, 2); cam.cy = K.at<float>(1, 2);
        cam.bf = bf;
        cam.max_x = (float)imGray.cols; cam.max_y = (float)imGray.rows;
        float dist[5] = {0, 0, 0, 0, 0};
        const int nd = distCoef.empty() ? 0 : std::min(5, distCoef.rows * distCoef.cols);
        for (int i = 0; i < nd; i++) dist[i] = distCoef.at<float>(i);
        coeb_ctx* ctx_ = coeb_detail::pooled_context(params_, device(), imGray.cols, imGray.rows);
        const int cap = coeb_max_keypoints(ctx_, imGray.cols, imGray.rows);
        if (cap < 0) throw std::runtime_error(coeb_last_error(ctx_));
        std::vector<coeb_keypoint> kps((size_t)cap), kun((size_t)cap);
        std::vector<float> ur((size_t)cap), dep((size_t)cap);
        cv::Mat desc((int)cap, 32, CV_8U);
        int n = 0;
        const int rc = coeb_frame_rgbd(ctx_, imGray.data, imGray.cols, imGray.rows, imGray.step[0], imDepth.data,
                                       imDepth.step[0], COEB_DEPTH_F32, 1.0f, &cam, nd ? dist : nullptr,
                                       boxes.empty() ? nullptr : boxes.data(), (int)boxes.size(),
                                       tm.empty() ? nullptr : tm.data(), (int)T_M.size(),
                                       blur_flag.empty() ? nullptr : blur_flag.data(), (int)blur_flag.size(), kps.data(),
                                       kun.data(), desc.data, ur.data(), dep.data(), cap, &n);
        if (rc != COEB_OK) throw std::runtime_error(coeb_last_error(ctx_));
        static_assert(sizeof(coeb_keypoint) == sizeof(cv::KeyPoint), "coeb_keypoint must mirror cv::KeyPoint");
        mvKeys.resize((size_t)n);
        mvKeysUn.resize((size_t)n);
        if (n) {
            std::memcpy(static_cast<void*>(&mvKeys[0]), kps.data(), sizeof(coeb_keypoint) * (size_t)n);
            std::memcpy(static_cast<void*>(&mvKeysUn[0]), kun.data(), sizeof(coeb_keypoint) * (size_t)n);
        }
        mvuRight.assign(ur.begin(), ur.begin() + n);
        mvDepth.assign(dep.begin(), dep.begin() + n);
        if (n == 0) {
            mDescriptors.release();
        } else {
            mDescriptors.create(n, 32, CV_8U);
            desc.rowRange(0, n).copyTo(mDescriptors);
        }
    }

    // The whole RGB-D Frame constructor (Frame.cc:157-223) in one device call (coeb_rgbd_stream_frame) on
    // the stream that lives with this extractor's pooled context: ProcessMovingObject against the
    // previous frame (kept on the device), the blur flag of every box, then ExtractRGBD's steps.
    // T_M and blur_flag are outputs here.  A frame without predecessor leaves T_M empty and every
    // flag 0 (:205-209); so does an empty fundamental matrix for T_M.  Same conventions as
    // operator(): an empty image returns without touching the outputs or the stream.
    void ExtractRGBDStream(const cv::Mat& imGray, const cv::Mat& imDepth, const cv::Mat& K, const cv::Mat& distCoef, float bf,
                           std::vector<std::vector<float>>& box, std::vector<cv::Point2f>& T_M, std::vector<int>& blur_flag,
                           std::vector<cv::KeyPoint>& mvKeys, cv::Mat& mDescriptors, std::vector<cv::KeyPoint>& mvKeysUn,
                           std::vector<float>& mvuRight, std::vector<float>& mvDepth)
    {
        if (imGray.empty()) return;
        assert(imGray.type() == CV_8UC1);
        if (imDepth.empty() || imDepth.type() != CV_32F || imDepth.rows != imGray.rows || imDepth.cols != imGray.cols)
            throw std::invalid_argument("ORBextractor::ExtractRGBDStream: a CV_32F depth map of the image's size expected");
        if (box.size() > (size_t)COEB_MAX_BOXES)
            throw std::invalid_argument("ORBextractor::ExtractRGBDStream: more than COEB_MAX_BOXES boxes");
        std::vector<coeb_box> boxes;
        for (const auto& b : box) boxes.push_back(coeb_box{b[0], b[1], b[2], b[3]});
        coeb_camera cam{};
        cam.fx = K.at<float>(0, 0); cam.fy = K.at<float>(1, 1); cam.cx = K.at<float>(0, 2); cam.cy = K.at<float>(1, 2);
        cam.bf = bf;
        cam.max_x = (float)imGray.cols; cam.max_y = (float)imGray.rows;
        float dist[5] = {0, 0, 0, 0, 0};
        const int nd = distCoef.empty() ? 0 : std::min(5, distCoef.rows * distCoef.cols);
        for (int i = 0; i < nd; i++) dist[i] = distCoef.at<float>(i);
        coeb_ctx* ctx_ = nullptr;
        coeb_rgbd_stream* st = coeb_detail::pooled_stream(params_, device(), imGray.cols, imGray.rows, &ctx_);
        const int cap = coeb_max_keypoints(ctx_, imGray.cols, imGray.rows);
        if (cap < 0) throw std::runtime_error(coeb_last_error(ctx_));
        std::vector<coeb_keypoint> kps((size_t)cap), kun((size_t)cap);
        std::vector<float> ur((size_t)cap), dep((size_t)cap), tm(2 * 1024);
        std::vector<int32_t> flags(boxes.size() + 1);
        cv::Mat desc((int)cap, 32, CV_8U);
        coeb_rgbd_stream_out o{};
        o.tm_xy = tm.data(); o.tm_cap = 1024; o.blur_flag = flags.data();
        o.kp = kps.data(); o.kp_un = kun.data(); o.desc = desc.data; o.u_right = ur.data(); o.depth = dep.data(); o.cap = cap;
        const int rc = coeb_rgbd_stream_frame(st, imGray.data, imGray.step[0], 1, 1, imGray.cols, imGray.rows, imDepth.data,
                                              imDepth.step[0], COEB_DEPTH_F32, 1.0f, &cam, nd ? dist : nullptr,
                                              boxes.empty() ? nullptr : boxes.data(), (int)boxes.size(), &o);
        if (rc != COEB_OK) throw std::runtime_error(coeb_last_error(ctx_));
        T_M.clear();
        for (int i = 0; i < o.n_tm; i++) T_M.push_back(cv::Point2f(tm[2 * i], tm[2 * i + 1]));
        blur_flag.assign(flags.begin(), flags.begin() + boxes.size());
        const int n = o.n;
        mvKeys.resize((size_t)n);
        mvKeysUn.resize((size_t)n);
        if (n) {
            std::memcpy(static_cast<void*>(&mvKeys[0]), kps.data(), sizeof(coeb_keypoint) * (size_t)n);
            std::memcpy(static_cast<void*>(&mvKeysUn[0]), kun.data(), sizeof(coeb_keypoint) * (size_t)n);
        }
        mvuRight.assign(ur.begin(), ur.begin() + n);
        mvDepth.assign(dep.begin(), dep.begin() + n);
        if (n == 0) {
            mDescriptors.release();
        } else {
            mDescriptors.create(n, 32, CV_8U);
            desc.rowRange(0, n).copyTo(mDescriptors);
        }
    }

    // Tracking::Reset: the next frame of every extractor of this thread is a first frame
    static void ResetFrameStreams() { coeb_detail::reset_streams(); }

    int inline GetLevels() { return nlevels; }
    float inline GetScaleFactor() { return (float)scaleFactor; }
    std::vector<float> inline GetScaleFactors() { return mvScaleFactor; }
    std::vector<float> inline GetInverseScaleFactors() { return mvInvScaleFactor; }
    std::vector<float> inline GetScaleSigmaSquares() { return mvLevelSigma2; }
    std::vector<float> inline GetInverseScaleSigmaSquares() { return mvInvLevelSigma2; }

    // Left empty (nlevels default-constructed Mats): the pyramid stays on the device.  The
    // reference's readers of it, Frame.cc:651, 741 and 758, are all in ComputeStereoMatches, which
    // the RGB-D constructor never calls.
    std::vector<cv::Mat> mvImagePyramid;

protected:
    static int device()
    {
        const char* e = std::getenv("COEB_DEVICE");
        return e ? std::atoi(e) : 0;
    }
    int nfeatures;
    double scaleFactor;
    int nlevels;
    int iniThFAST;
    int minThFAST;
    std::vector<int> mnFeaturesPerLevel;
    std::vector<int> umax;
    std::vector<float> mvScaleFactor;
    std::vector<float> mvInvScaleFactor;
    std::vector<float> mvLevelSigma2;
    std::vector<float> mvInvLevelSigma2;
    coeb_orb_params params_{};
};

}  // namespace ORB_SLAM2

#endif
