/*
 * coeb_front.h -- C-ABI of the MI355X-native COEB-SLAM per-frame ORB front end.
 *
 * Plain C: pointers, sizes and POD structs only (no OpenCV, no torch types).  Every entry
 * point names the reference interface it replaces (paths are into biscuitzb/COEB-SLAM):
 *
 *   coeb_create / coeb_orb_tables   <- ORBextractor::ORBextractor(nfeatures, scaleFactor,
 *                                      nlevels, iniThFAST, minThFAST)  include/ORBextractor.h:50-51,
 *                                      src/ORBextractor.cc:418-477, accessors ORBextractor.h:77-99
 *   coeb_extract                    <- ORBextractor::operator()(image, mask, img, imD, keypoints,
 *                                      descriptors, box, T_M, mask_result, blur_flag)
 *                                      include/ORBextractor.h:73-75, src/ORBextractor.cc:1088-1342
 *   coeb_extract_batch_device       <- the same, for a device-resident batch of frames
 *   coeb_blur_flags                 <- Frame RGB-D ctor blur-flag loop + Frame::detect_laplacian
 *                                      src/Frame.cc:171-202, 905-913
 *   coeb_rgbd_preprocess            <- Tracking::GrabImageRGBD cvtColor / depth convertTo
 *                                      src/Tracking.cc:207-228
 *   coeb_undistort_keypoints        <- Frame::UndistortKeyPoints  src/Frame.cc:579-609
 *   coeb_boxes_from_int64           <- ImageGrabber::GrabRGBD box copy
 *                                      Examples/ROS/ORB-SLAM2/src/ros_rgbd.cc:106-115
 *   coeb_stereo_from_rgbd           <- Frame::ComputeStereoFromRGBD  src/Frame.cc:820-842
 *   coeb_frame_rgbd                 <- the RGB-D Frame constructor's tail  src/Frame.cc:214-223:
 *                                      ExtractORB, N = mvKeys.size(), UndistortKeyPoints (:579-609)
 *                                      and ComputeStereoFromRGBD (:820-842) on one host frame
 *   coeb_rgbd_stream_frame          <- the whole RGB-D Frame constructor  src/Frame.cc:157-223 on a stream
 *                                      of host frames: ProcessMovingObject against the previous frame
 *                                      (kept on the device), the blur flags, then coeb_frame_rgbd's steps
 *   coeb_match_lastframe            <- ORBmatcher::SearchByProjection(Frame&, const Frame&,
 *                                      const float th, const bool bMono)
 *                                      include/ORBmatcher.h:52, src/ORBmatcher.cc:1329-1471
 *                                      (with Frame::GetFeaturesInArea / AssignFeaturesToGrid,
 *                                      src/Frame.cc:396-411, 503-568)
 *   coeb_match_localmap             <- ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&,
 *                                      const float th)  include/ORBmatcher.h:46,
 *                                      src/ORBmatcher.cc:44-129 (RadiusByViewingCos :131-137),
 *                                      the call in Tracking::SearchLocalPoints  src/Tracking.cc:1222-1271
 *   coeb_search_local_points        <- Tracking::SearchLocalPoints from the projection loop on
 *                                      src/Tracking.cc:1246-1271: Frame::isInFrustum(pMP, 0.5)
 *                                      src/Frame.cc:445-501 (MapPoint::PredictScale
 *                                      src/MapPoint.cc:402-417) over vpLocalMapPoints, then the
 *                                      SearchByProjection above, on one host frame in one call
 *   coeb_track_local_map            <- Tracking::TrackLocalMap  src/Tracking.cc:996-1047 after
 *                                      UpdateLocalMap: SearchLocalPoints (:1222-1272, as above),
 *                                      Optimizer::PoseOptimization (:1006) and mnMatchesInliers
 *                                      (:1010-1027), one call and one synchronisation
 *   coeb_match_keyframe             <- ORBmatcher::SearchByProjection(Frame&, KeyFrame*,
 *                                      const set<MapPoint*>&, const float th, const int ORBdist)
 *                                      include/ORBmatcher.h:55, src/ORBmatcher.cc:1473-1600
 *                                      (MapPoint::PredictScale  src/MapPoint.cc:402-417), the
 *                                      calls in Tracking::Relocalization  src/Tracking.cc:1531,1545
 *   coeb_pose_optimization          <- Optimizer::PoseOptimization(Frame*)  include/Optimizer.h:47,
 *                                      src/Optimizer.cc:239-451 (g2o LM; g2o itself is not vendored,
 *                                      parity UNPINNED); calls Tracking.cc:841,964,1006
 *   coeb_pose_batch_device          <- Tracking::TrackWithMotionModel after the projection search
 *                                      src/Tracking.cc:947-964 (mvpMapPoints from the matches,
 *                                      nmatches < 20 -> not tracked, PoseOptimization :964)
 *   coeb_good_features, coeb_corner_subpix, coeb_optical_flow_pyr_lk, coeb_moving_tail,
 *   coeb_moving_object_points[_device]  <- Frame::ProcessMovingObject  src/Frame.cc:311-393
 *                                      (OpenCV goodFeaturesToTrack / cornerSubPix / calcOpticalFlowPyrLK /
 *                                      findFundamentalMat as called there)
 *   coeb_descriptor_distance        <- ORBmatcher::DescriptorDistance  src/ORBmatcher.cc:1648-1664
 *   coeb_voc_from_text / _from_arrays <- ORBVocabulary::loadFromTextFile as System::System calls it
 *                                      src/System.cc:66-76 (DBoW2's TemplatedVocabulary is not
 *                                      vendored: the format and the transform are restated, parity
 *                                      against DBoW2 UNPINNED)
 *   coeb_bow_transform              <- Frame::ComputeBoW  src/Frame.cc:570-577 =
 *                                      mpORBvocabulary->transform(vCurrentDesc, mBowVec, mFeatVec, 4),
 *                                      per feature TemplatedVocabulary::transform(feature, word,
 *                                      weight, &nid, levelsup); the calls in
 *                                      Tracking::TrackReferenceKeyFrame  src/Tracking.cc:826 and
 *                                      Tracking::Relocalization  src/Tracking.cc:1420
 *   coeb_bow_batch_device           <- the same, over the last extracted device batch
 *   coeb_match_bow                  <- ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&)
 *                                      include/ORBmatcher.h:65, src/ORBmatcher.cc:159-288; the calls
 *                                      in TrackReferenceKeyFrame  src/Tracking.cc:833 and
 *                                      Relocalization  src/Tracking.cc:1456
 *   coeb_track_reference_keyframe   <- Tracking::TrackReferenceKeyFrame  src/Tracking.cc:823-865:
 *                                      ComputeBoW (:826), SearchByBoW (:833), the nmatches < 15 gate
 *                                      (:835), Optimizer::PoseOptimization (:841) and the outlier
 *                                      discard with nmatchesMap (:843-862) on one host frame, one
 *                                      call and one synchronisation
 *   coeb_track_motion_model         <- Tracking::TrackWithMotionModel  src/Tracking.cc:933-994 with
 *                                      UpdateLastFrame's visual-odometry points (:878-930):
 *                                      SearchByProjection (:951), the 2*th retry (:954-958), the
 *                                      nmatches < 20 gate (:960), Optimizer::PoseOptimization (:964)
 *                                      and the outlier discard with nmatchesMap (:966-985) on one
 *                                      host frame, one call and one synchronisation
 *   coeb_reloc_refine               <- Tracking::Relocalization behind PnPsolver::iterate
 *                                      src/Tracking.cc:1502-1565, for the hypotheses of one round of
 *                                      the while loop (:1477-1568) side by side: the inliers (:1508-1517),
 *                                      PoseOptimization (:1519), the nGood < 10 gate and the discard
 *                                      (:1521-1526), SearchByProjection(.., 10, 100) (:1531),
 *                                      PoseOptimization (:1535), SearchByProjection(.., 3, 64) over the
 *                                      rebuilt sFound (:1541-1545), PoseOptimization and the discard
 *                                      (:1550-1554); one call and one synchronisation.  The PnP solver
 *                                      stays the caller's
 *   coeb_bow_vector                <- DBoW2 BowVector::addWeight / normalize(L1) as transform() fills
 *                                      mBowVec (host only; restated, parity against DBoW2 UNPINNED)
 *   coeb_kfdb_add / _erase / _clear <- KeyFrameDatabase::add / erase / clear
 *                                      src/KeyFrameDatabase.cc:40-73
 *   coeb_kfdb_query                 <- KeyFrameDatabase::DetectRelocalizationCandidates up to
 *                                      lScoreAndMatch  src/KeyFrameDatabase.cc:199-253 (the
 *                                      covisibility tail :258-308 stays on the host, in the adapters)
 *   coeb_match_bow_kfdb             <- the SearchByBoW loop of Tracking::Relocalization
 *                                      src/Tracking.cc:1449-1470
 *   coeb_kfdb_search_triangulation  <- the SearchForTriangulation loop of
 *                                      LocalMapping::CreateNewMapPoints  src/LocalMapping.cc:255-270,
 *                                      src/ORBmatcher.cc:657-824 (coeb_kfdb_set_geometry: the
 *                                      KeyFrame's mvKeysUn / mvuRight it reads)
 *   coeb_kfdb_create_new_map_points <- that search and the loop body behind it, src/LocalMapping.cc:271-433
 *                                      (coeb_kfdb_set_stereo: the KeyFrame's mvKeys / mvDepth it reads)
 *   coeb_kfdb_fuse_search           <- the search of ORBmatcher::Fuse (src/ORBmatcher.cc:826-951) for
 *                                      the loops of LocalMapping::SearchInNeighbors
 *                                      src/LocalMapping.cc:455-535
 *   coeb_tum_read_list            <- associate.py read_file_list  associate.py:49-69
 *   coeb_tum_associate              <- associate.py associate  associate.py:71-102 (host only)
 *
 * Conventions: 0 on success, negative COEB_E* code on failure (the reference has no error
 * returns: it asserts or is UB).  The caller owns host buffers; the context
 * owns device buffers and streams.  One context per host thread; calls are not reentrant.
 */
#ifndef COEB_FRONT_H
#define COEB_FRONT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define COEB_OK 0
#define COEB_EINVAL (-22)    /* bad argument / shape outside the context limits */
#define COEB_ENOMEM (-12)    /* device allocation failed */
#define COEB_EDEVICE (-5)    /* HIP runtime error (see coeb_last_error) */
#define COEB_ERANGE (-34)    /* an internal capacity was exceeded (see coeb_last_error) */
#define COEB_ENODEV (-19)    /* no usable gfx950 device */

/* ABI revision of this header.  Bumped whenever an entry point's signature or a struct layout
 * changes (3: coeb_rgbd_preprocess gained channels/depth_type and a byte depth stride); the
 * adapters compare it with coeb_abi_version() of the loaded library and refuse a mismatch. */
#define COEB_ABI_VERSION 3
/* Entry points added since (coeb_kfdb_search_triangulation, coeb_kfdb_fuse_search, coeb_kfdb_set_stereo,
 * coeb_kfdb_create_new_map_points) do not move the number: no existing signature or layout changed.  A
 * client built against this header therefore passes the coeb_abi_version() check against an older library
 * and fails at symbol lookup instead. */
int coeb_abi_version(void);

#define COEB_MAX_LEVELS 16
#define COEB_MAX_BOXES 16

typedef struct coeb_ctx coeb_ctx;

/* ORBextractor ctor arguments.  iniThFAST/minThFAST are accepted but, as in the reference,
 * overridden per frame to 20/7 (30/10 when the dynamic area exceeds 200000 px)
 * (src/ORBextractor.cc:775-784). */
typedef struct {
    int32_t nfeatures;
    float scale_factor;
    int32_t nlevels;
    int32_t ini_th_fast;
    int32_t min_th_fast;
} coeb_orb_params;

/* layout-identical to cv::KeyPoint {Point2f pt; float size, angle, response; int octave, class_id;} */
typedef struct {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} coeb_keypoint;

/* YOLO person box, xyxy, as std::vector<float>{xmin,ymin,xmax,ymax} (ros_rgbd.cc:106-115) */
typedef struct {
    float xmin, ymin, xmax, ymax;
} coeb_box;

/* ORBextractor accessors (include/ORBextractor.h:77-99) and derived per-level constants */
typedef struct {
    int32_t nlevels;
    float scale_factor;
    float scale[COEB_MAX_LEVELS];          /* GetScaleFactors() */
    float inv_scale[COEB_MAX_LEVELS];      /* GetInverseScaleFactors() */
    float sigma2[COEB_MAX_LEVELS];         /* GetScaleSigmaSquares() */
    float inv_sigma2[COEB_MAX_LEVELS];     /* GetInverseScaleSigmaSquares() */
    int32_t features_per_level[COEB_MAX_LEVELS];
    int32_t umax[16];
} coeb_orb_tables;

/* Camera + Frame constants used by the matcher (Frame.cc:231-246, ComputeImageBounds :611-641) */
typedef struct {
    float fx, fy, cx, cy;
    float bf;                   /* mbf */
    float min_x, max_x, min_y, max_y;
} coeb_camera;

/* Snapshot of the previous Frame taken by the caller (MapPoint accessors under their mutexes):
 * ORBmatcher.cc:1352-1396 reads exactly these. */
typedef struct {
    int32_t n;                        /* LastFrame.N */
    const uint8_t* has_mappoint;      /* LastFrame.mvpMapPoints[i] != NULL */
    const uint8_t* outlier;           /* LastFrame.mvbOutlier[i] */
    const float* world_pos;           /* n x 3, MapPoint::GetWorldPos() */
    const uint8_t* mp_descriptor;     /* n x 32, MapPoint::GetDescriptor() */
    const int32_t* mp_observations;   /* MapPoint::Observations() */
    const coeb_keypoint* keys_un;     /* LastFrame.mvKeysUn (octave, angle) */
} coeb_lastframe;

/* The current Frame (after ExtractORB + ComputeStereoFromRGBD) */
typedef struct {
    int32_t n;                        /* CurrentFrame.N */
    const coeb_keypoint* keys_un;     /* CurrentFrame.mvKeysUn */
    const uint8_t* descriptors;       /* n x 32 */
    const float* u_right;             /* CurrentFrame.mvuRight */
} coeb_curframe;

/* ---- context ---- */
coeb_ctx* coeb_create(const coeb_orb_params* params, int device, int max_width, int max_height,
                      int max_batch);
void coeb_destroy(coeb_ctx* ctx);
const char* coeb_last_error(const coeb_ctx* ctx);   /* also valid with ctx == NULL */
int coeb_orb_tables_get(const coeb_ctx* ctx, coeb_orb_tables* out);
/* keypoint capacity per frame needed by coeb_extract for a w x h image */
int coeb_max_keypoints(const coeb_ctx* ctx, int width, int height);

/* ---- ORBextractor::operator() on one host frame ----
 * gray: 8UC1 (stride in bytes).  boxes/T_M/blur_flag as passed by Frame::ExtractORB.
 * Writes up to `cap` keypoints and their 32-byte descriptors; *n_out = keypoint count.
 * An empty image (width or height 0) returns COEB_OK with *n_out = 0 (:1096-1097). */
int coeb_extract(coeb_ctx* ctx, const uint8_t* gray, int width, int height, size_t stride,
                 const coeb_box* boxes, int nbox, const float* tm_xy, int ntm,
                 const int32_t* blur_flag, int nblur,
                 coeb_keypoint* kp_out, uint8_t* desc_out, int cap, int* n_out);

/* ---- device-resident batch (the throughput path) ----
 * d_gray: device pointer, nframes x height x width bytes, packed.  boxes/T_M/blur flags are
 * host arrays: per frame f, boxes[box_off[f] .. box_off[f+1]) etc. (offset arrays of length
 * nframes+1; all may be NULL for "no boxes").  Results stay on the device; fetch them with
 * coeb_batch_results.  Returns without synchronising: the frames are split into contiguous
 * chunks, one per batch stream (coeb_set_batch_streams), so the kernels of different chunks
 * overlap on the device; every other call on the context waits for them. */
int coeb_extract_batch_device(coeb_ctx* ctx, const uint8_t* d_gray, int nframes, int width, int height,
                              const coeb_box* boxes, const int32_t* box_off,
                              const float* tm_xy, const int32_t* tm_off,
                              const int32_t* blur_flag);
/* The RGB-D Frame constructor on a device-resident batch (src/Frame.cc:157-214): for frame f,
 * ProcessMovingObject(frame f-1, frame f) -> T_M (:164-166, coeb_moving_object_points), the
 * detect_laplacian blur flag of every box (:171-202; frame 0 is the sequence's first frame: no
 * T_M, flags 0, :205-208), then ORBextractor::operator() with those boxes, T_M and flags (:214).
 * T_M and the flags never leave the device (coeb_batch_frame_results exposes them).  Boxes are
 * host arrays as in coeb_extract_batch_device (NULL: none).  Runs on the context stream only;
 * results as coeb_extract_batch_device's (coeb_batch_results), and the batch matcher / pose
 * entry points follow it. */
int coeb_frame_batch_device(coeb_ctx* ctx, const uint8_t* d_gray, int nframes, int width, int height,
                            const coeb_box* boxes, const int32_t* box_off);
/* Device pointers of the last coeb_frame_batch_device: T_M of frame f at d_tm + f * tm_cap * 2
 * (x, y floats), |T_M| in d_ntm[f] (-1: the fundamental matrix was empty), blur flags per box
 * (NULL without boxes). */
int coeb_batch_frame_results(coeb_ctx* ctx, const float** d_tm, const int32_t** d_ntm, int* tm_cap,
                             const int32_t** d_blur);
/* Device pointers to the batch outputs: keypoints [nframes][kcap], descriptors
 * [nframes][kcap][32], counts [nframes]. */
int coeb_batch_results(coeb_ctx* ctx, const coeb_keypoint** d_kps, const uint8_t** d_desc,
                       const int32_t** d_counts, int* kcap);
/* Number of HIP streams a batch is spread over (1..16, default 1; chunks of >= 16 frames).
 * 1 = every kernel of the batch on the context stream, one after another. */
int coeb_set_batch_streams(coeb_ctx* ctx, int nstreams);

/* Batch TrackWithMotionModel matching (Tracking.cc:933-958 call pattern): for f = 1..nframes-1
 * frame f is matched to frame f-1 of the last extracted batch.  Frame f-1 is the LastFrame and
 * defines the world frame (its Tcw = I): its map points are its keypoints with depth > 0
 * unprojected with Twc = I (Frame::UnprojectStereo, Frame.cc:844-858), Observations() = nobs.
 * Tcw[f] (row-major 4x4, host, nframes x 16 floats; entry 0 unused) is the pose of frame f
 * relative to frame f-1 (the motion-model prediction mVelocity*mLastFrame.mTcw,
 * Tracking.cc:937).  SearchByProjection(th) and, if < 20 matches, again with 2*th.
 * d_depth: nframes x height x width float (device).  Results: coeb_batch_match_results. */
int coeb_match_batch_device(coeb_ctx* ctx, const float* d_depth, int nframes, int width, int height,
                            const coeb_camera* cam, const float* Tcw, float th, int32_t nobs);
/* The same with the poses already in device memory (d_Tcw: nframes x 16 floats). */
int coeb_match_batch_device_tcw(coeb_ctx* ctx, const float* d_depth, int nframes, int width, int height,
                                const coeb_camera* cam, const float* d_Tcw, float th, int32_t nobs);
int coeb_batch_match_results(coeb_ctx* ctx, const int32_t** d_match, const int32_t** d_nmatches);

/* ---- Tracking::TrackWithMotionModel tail on the batch (Tracking.cc:947-964) ----
 * After coeb_match_batch_device*: for every pair, CurrentFrame.mvpMapPoints = the matcher's
 * assignments (positions from the LastFrame snapshot), then, if nmatches >= min_matches (20 in
 * the reference, :954-958), Optimizer::PoseOptimization (as coeb_pose_optimization) from the
 * prediction d_Tcw (the same nframes x 16 device array the matcher used).  Results (device,
 * frame 0 = halo): coeb_batch_pose_results -> Tcw nframes x 16 (the prediction where the frame
 * was not optimised), ninliers per frame (0: not tracked), outlier flags nframes x capacity. */
int coeb_pose_batch_device(coeb_ctx* ctx, const coeb_camera* cam, int nframes, const float* d_Tcw,
                           int32_t min_matches);
int coeb_batch_pose_results(coeb_ctx* ctx, const float** d_Tcw, const int32_t** d_ninliers,
                            const uint8_t** d_outlier);

/* ---- Tracking::TrackLocalMap on the batch (Tracking.cc:966-993, 996-1047, 1222-1272) ----
 * After coeb_pose_batch_device on the same batch, for every frame f >= 1:
 *   - TrackWithMotionModel's tail: matched keypoints the first PoseOptimization flagged outlier
 *     lose their MapPoint; nmatchesMap = kept MapPoints with Observations() > 0; the frame goes
 *     on only if the motion model ran (>= min_matches) and nmatchesMap >= 10 (:993);
 *   - the local map: the MapPoints of KeyFrames f-1 (KF1, the pair's world frame) and, with
 *     nkf = 2, f-2 (KF2, placed by frame f-1's motion-model pose), one MapPoint per keypoint with
 *     depth > 0; points matched by the motion model are skipped (mnLastFrameSeen),
 *     the rest go through Frame::isInFrustum(pMP, 0.5) with the first pose;
 *   - ORBmatcher(nnratio).SearchByProjection(F, vpLocalMapPoints, th) (3 for RGB-D, :1264-1270);
 *   - Optimizer::PoseOptimization from the first pose over the kept and the new MapPoints.
 * Observations() of every MapPoint = the nobs of coeb_match_batch_device.  Work is enqueued
 * behind the first k_pose on the pose stream.  Results (device, frame 0 = halo):
 * coeb_batch_track_results -> Tcw nframes x 16 (the first pose where TrackLocalMap did not run),
 * ninliers per frame (the second PoseOptimization's return = mnMatchesInliers when nobs > 0;
 * 0: not run), nmatches_map per frame, nlocal = SearchByProjection's return, local_match
 * nframes x capacity (local-map index per keypoint: [0, capacity) KF2 slot, [capacity,
 * 2 capacity) KF1 slot, -1), outlier flags nframes x capacity (mvbOutlier of the second run). */
int coeb_track_local_map_batch_device(coeb_ctx* ctx, const coeb_camera* cam, int nframes, int32_t nkf, float th,
                                      float nnratio);
int coeb_batch_track_results(coeb_ctx* ctx, const float** d_Tcw, const int32_t** d_ninliers,
                             const int32_t** d_nmatches_map, const int32_t** d_nlocal,
                             const int32_t** d_local_match, const uint8_t** d_outlier);

/* ---- ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) ----
 * match_out[i2] (length cur->n) = index of the LastFrame slot whose MapPoint was assigned to
 * current keypoint i2 (CurrentFrame.mvpMapPoints[i2]), or -1; *nmatches = the return value.
 * CurrentFrame.mvpMapPoints is taken as all-NULL on entry (Tracking.cc:943). */
int coeb_match_lastframe(coeb_ctx* ctx, const coeb_camera* cam, const coeb_curframe* cur,
                         const coeb_lastframe* last, const float Tcw_cur[16], const float Tcw_last[16],
                         float th, int bmono, int check_orientation, int32_t* match_out, int* nmatches);

/* Local-map points as Frame::isInFrustum left them (Frame.cc:445-501 writes mbTrackInView,
 * mTrackProjX/Y/XR, mnTrackScaleLevel, mTrackViewCos); ORBmatcher.cc:50-80 reads exactly these. */
typedef struct {
    int32_t n;                        /* vpMapPoints.size() */
    const uint8_t* in_view;           /* mbTrackInView && !isBad() */
    const float* proj_x;              /* mTrackProjX */
    const float* proj_y;              /* mTrackProjY */
    const float* proj_xr;             /* mTrackProjXR */
    const int32_t* level;             /* mnTrackScaleLevel (0 .. nlevels-1 where in_view) */
    const float* view_cos;            /* mTrackViewCos */
    const uint8_t* descriptor;        /* n x 32, GetDescriptor() */
    const int32_t* observations;      /* Observations() */
} coeb_localmap;

/* ---- ORBmatcher::SearchByProjection(CurrentFrame, vpLocalMapPoints, th) ----
 * cur_observations[i] (length cur->n, may be NULL = all NULL): Observations() of the MapPoint
 * already in CurrentFrame.mvpMapPoints[i], or -1 for NULL; keypoints whose holder has
 * Observations() > 0 are skipped (ORBmatcher.cc:86-88), as are keypoints given on the way to a
 * point with Observations() > 0.  match_out[i] (length cur->n) = index of the local-map point
 * assigned to keypoint i by this call (the last one when several were), or -1; *nmatches = the
 * return value (every assignment counts, as in the reference).  nnratio = mfNNratio. */
int coeb_match_localmap(coeb_ctx* ctx, const coeb_camera* cam, const coeb_curframe* cur,
                        const int32_t* cur_observations, const coeb_localmap* mp, float th,
                        float nnratio, int32_t* match_out, int* nmatches);

/* vpLocalMapPoints as Tracking::SearchLocalPoints reads them before isInFrustum. */
typedef struct {
    int32_t n;                        /* mvpLocalMapPoints.size() */
    const uint8_t* valid;             /* !isBad() && mnLastFrameSeen != mCurrentFrame.mnId (Tracking.cc:1249-1252) */
    const float* world_pos;           /* n x 3, GetWorldPos() */
    const float* normal;              /* n x 3, GetNormal() */
    const float* max_distance;        /* mfMaxDistance (GetMaxDistanceInvariance() = 1.2f * it) */
    const float* min_distance;        /* mfMinDistance (GetMinDistanceInvariance() = 0.8f * it) */
    const uint8_t* descriptor;        /* n x 32, GetDescriptor() */
    const int32_t* observations;      /* Observations() */
} coeb_local_points;

/* The fields Frame::isInFrustum leaves on every local-map point (Frame.cc:447, 493-498), each of
 * length points->n: mbTrackInView, mTrackProjX / Y / XR, mnTrackScaleLevel, mTrackViewCos (zeros
 * where in_view is 0).  Any pointer may be NULL. */
typedef struct {
    uint8_t* in_view;
    float* proj_x;
    float* proj_y;
    float* proj_xr;
    int32_t* level;
    float* view_cos;
} coeb_track_fields;

/* ---- Tracking::SearchLocalPoints from :1246 on ----
 * isInFrustum(pMP, cos_limit) for every valid point with the pose Tcw (CurrentFrame.mTcw, row-major
 * 4x4), then SearchByProjection(CurrentFrame, vpLocalMapPoints, th) with nnratio on the points in
 * view; cur_observations, match_out and *nmatches as coeb_match_localmap's.  *n_to_match = the
 * number of points in view (nToMatch; with none the search is skipped in the reference and finds
 * nothing here).  track_fields_out may be NULL.  The frame and the local map together are bounded
 * by the matcher's on-chip memory: COEB_ERANGE beyond it, as coeb_match_localmap.  COEB_EINVAL,
 * with nothing written, for a missing array, a valid point with a non-finite position or normal,
 * or a valid point whose distances are not 0 < min_distance <= max_distance < inf (PredictScale
 * is undefined there). */
int coeb_search_local_points(coeb_ctx* ctx, const coeb_camera* cam, const coeb_curframe* cur,
                             const int32_t* cur_observations, const float Tcw[16],
                             const coeb_local_points* points, float cos_limit, float th, float nnratio,
                             const coeb_track_fields* track_fields_out, int32_t* match_out,
                             int* n_to_match, int* nmatches);

/* ---- Tracking::TrackLocalMap after UpdateLocalMap ----
 * coeb_search_local_points, then Optimizer::PoseOptimization from Tcw over the keypoints that hold
 * a point afterwards: the local-map point the search gave them, else the MapPoint they entered
 * with (cur_observations[i] >= 0, position cur_world_pos[3 i ..], read only there;
 * cur_observations[i] = -1 where mvpMapPoints[i] is NULL or was bad and reset at :1230-1233).
 * Tcw holds the optimised pose on return (untouched with < 3 edges, *ninliers_pose = 0 then);
 * outlier_out[i] (length cur->n, may be NULL) = mvbOutlier[i], written where keypoint i holds a
 * point; *nlocal = SearchByProjection's return value; *ninliers_pose = PoseOptimization's;
 * *nmatches_inliers = mnMatchesInliers (:1010-1027): keypoints holding a point that is no outlier
 * and, unless only_tracking (mbOnlyTracking), has Observations() > 0.  Every keypoint's octave
 * must lie inside the pyramid. */
int coeb_track_local_map(coeb_ctx* ctx, const coeb_camera* cam, const coeb_curframe* cur,
                         const int32_t* cur_observations, const float* cur_world_pos, float Tcw[16],
                         const coeb_local_points* points, float cos_limit, float th, float nnratio,
                         int only_tracking, const coeb_track_fields* track_fields_out, int32_t* match_out,
                         uint8_t* outlier_out, int* n_to_match, int* nlocal, int* ninliers_pose,
                         int* nmatches_inliers);

/* Map points of a KeyFrame as ORBmatcher.cc:1487-1530 reads them (pKF->GetMapPointMatches()). */
typedef struct {
    int32_t n;                        /* vpMPs.size() */
    const uint8_t* valid;             /* pMP && !pMP->isBad() && !sAlreadyFound.count(pMP) */
    const float* world_pos;           /* n x 3, GetWorldPos() */
    const uint8_t* descriptor;        /* n x 32, GetDescriptor() */
    const float* max_distance;        /* mfMaxDistance (GetMaxDistanceInvariance() = 1.2f * it) */
    const float* min_distance;        /* mfMinDistance (GetMinDistanceInvariance() = 0.8f * it) */
    const float* angle;               /* pKF->mvKeysUn[i].angle */
} coeb_keyframe_points;

/* ---- ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) ----
 * cur_has_mappoint[i] (length cur->n, may be NULL = all NULL): CurrentFrame.mvpMapPoints[i] !=
 * NULL on entry; such keypoints are skipped, as are keypoints given earlier in the call.
 * Tcw: CurrentFrame.mTcw (row-major 4x4).  The scale pyramid is the context's (mnScaleLevels,
 * mvScaleFactors, mfLogScaleFactor).  match_out[i] = index of the KeyFrame point assigned to
 * keypoint i, or -1; *nmatches = the return value (after the rotation filter when
 * check_orientation = mbCheckOrientation).  cur->u_right is not read (may be NULL). */
int coeb_match_keyframe(coeb_ctx* ctx, const coeb_camera* cam, const coeb_curframe* cur,
                        const uint8_t* cur_has_mappoint, const coeb_keyframe_points* kf,
                        const float Tcw[16], float th, int orb_dist, int check_orientation,
                        int32_t* match_out, int* nmatches);

/* ---- bag of words: vocabulary, Frame::ComputeBoW, ORBmatcher::SearchByBoW ----
 * The vocabulary is host data (no context, no device).  coeb_voc_from_text parses ORB-SLAM2's
 * ORBvoc.txt: first line "k L scoring weighting" (k 2..20, L 1..10, scoring 0..5, weighting 0..3),
 * then one line "parent is_leaf d0 .. d31 weight" per node; node ids are 1, 2, .. in line order
 * (0 is the root), a line appends its node to children[parent], leaves take word ids 0, 1, .. in
 * line order.  COEB_EINVAL (never a crash) for an empty text, a header out of range, a short or
 * over-long line, a byte outside 0..255, a parent that is not a node already defined or is a
 * leaf, more than k children, a node below level L, an inner node without children.
 * coeb_voc_from_arrays takes the same lines as arrays: node i + 1 = (parent[i], is_leaf[i],
 * desc[32 i ..], weight[i]) for i < nlines.  coeb_voc_info: nnodes counts the root.
 * coeb_voc_tables copies the tables the device walks (any pointer may be NULL): nodes renumbered
 * into slots, slot 0 the root, the children of a slot contiguous in their original order from
 * child_first[slot], child_count[slot] of them (0: a leaf); word[slot] (-1: inner node),
 * node_id[slot], positive[slot] (leaf weight > 0), desc[slot][32]; per word its weight and node id. */
typedef struct coeb_voc coeb_voc;
int coeb_voc_from_text(const char* text, size_t len, coeb_voc** voc);
int coeb_voc_from_arrays(int k, int L, int nlines, const int32_t* parent, const uint8_t* is_leaf,
                         const uint8_t* desc, const double* weight, coeb_voc** voc);
int coeb_voc_info(const coeb_voc* voc, int* k, int* L, int* nnodes, int* nwords);
int coeb_voc_tables(const coeb_voc* voc, int32_t* child_first, int32_t* child_count, int32_t* word,
                    int32_t* node_id, uint8_t* positive, uint8_t* desc, double* word_weight, int32_t* word_node);
void coeb_voc_destroy(coeb_voc* voc);
/* Uploads the vocabulary's tables to the context's device; a second call replaces them.  The
 * context keeps nothing of `voc` afterwards. */
int coeb_bow_set_vocabulary(coeb_ctx* ctx, const coeb_voc* voc);

/* ---- Frame::ComputeBoW on one host frame ----
 * desc: n x 32 (n <= 4095).  Per feature i, transform(desc[i], word, weight, &nid, levelsup):
 * from the root, the child with the smallest DescriptorDistance (the first one on a tie) until a
 * leaf; word_out[i] = its word id, weight_out[i] = its weight, nid = the id of the node passed at
 * level L - levelsup (0 when levelsup >= L; the leaf itself when it lies above that level, where
 * the reference leaves nid uninitialised).  As in BowVector / FeatureVector filling (`if (w > 0)`),
 * a feature whose word weight is not > 0 keeps its word id but has node_out[i] = -1 and is not in
 * the feature vector; the caller skips addWeight for it.  The feature vector is a CSR: fv_node
 * [*nfv_out] distinct node ids ascending, fv_off[*nfv_out + 1], and under node j the feature
 * indices fv_idx[fv_off[j] .. fv_off[j+1]) ascending (fv_node, fv_off, fv_idx hold fv_cap,
 * fv_cap + 1 and n entries; all three NULL: not wanted; more than fv_cap nodes: COEB_ERANGE with
 * *nfv_out set).  word_out / node_out / weight_out may be NULL.  COEB_EINVAL before
 * coeb_bow_set_vocabulary. */
int coeb_bow_transform(coeb_ctx* ctx, const uint8_t* desc, int n, int levelsup, int32_t* word_out,
                       int32_t* node_out, double* weight_out, int32_t* fv_node, int32_t* fv_off,
                       int32_t* fv_idx, int fv_cap, int* nfv_out);
/* The same transform over the descriptors of the last extracted batch ([nframes][kcap][32] with
 * their counts); coeb_batch_bow_results -> device pointers to word ids and node ids
 * [nframes][kcap] (-1 past a frame's count; node id -1 as above).  Enqueued on the context stream. */
int coeb_bow_batch_device(coeb_ctx* ctx, int levelsup);
int coeb_batch_bow_results(coeb_ctx* ctx, const int32_t** d_word, const int32_t** d_node);

/* The KeyFrame fields SearchByBoW reads (ORBmatcher.cc:161-199, 234). */
typedef struct {
    int32_t n;                        /* pKF->N */
    const uint8_t* valid;             /* vpMapPointsKF[i] && !isBad() */
    const uint8_t* descriptor;        /* n x 32, pKF->mDescriptors */
    const int32_t* node_id;           /* the mFeatVec node that lists feature i, -1: none */
    const float* angle;               /* pKF->mvKeysUn[i].angle */
} coeb_bow_keyframe;
/* ... and of the Frame (:176-212, 238). */
typedef struct {
    int32_t n;                        /* F.N */
    const uint8_t* descriptor;        /* n x 32, F.mDescriptors */
    const int32_t* node_id;           /* the F.mFeatVec node that lists feature i, -1: none */
    const float* angle;               /* F.mvKeys[i].angle */
} coeb_bow_frame;

/* ---- ORBmatcher::SearchByBoW(pKF, F, vpMapPointMatches) ----
 * For every node in both feature vectors, the KeyFrame's valid features in index order, each
 * against the node's frame features (index order) not yet given away: bestDist1 / bestIdxF the
 * first strict minimum, bestDist2 the second smallest distance (both from 256); accepted when
 * bestDist1 <= TH_LOW (50) and (float)bestDist1 < nnratio * (float)bestDist2; then the
 * rotation-histogram filter when check_orientation.  match_out[i] (length cur->n) = the KeyFrame
 * index whose MapPoint vpMapPointMatches[i] holds, or -1; *nmatches = the return value.
 * At most 4095 features per side. */
int coeb_match_bow(coeb_ctx* ctx, const coeb_bow_keyframe* kf, const coeb_bow_frame* cur, float nnratio,
                   int check_orientation, int32_t* match_out, int* nmatches);

/* mpReferenceKF as TrackReferenceKeyFrame reads it: the SearchByBoW fields, plus what
 * PoseOptimization and the discard loop read from the matched MapPoints. */
typedef struct {
    coeb_bow_keyframe bow;            /* n, valid, descriptor, node_id, angle */
    const float* world_pos;           /* n x 3, GetWorldPos(), read where valid */
    const int32_t* observations;      /* Observations(), read where valid */
} coeb_ref_keyframe;

/* ---- Tracking::TrackReferenceKeyFrame (Tracking.cc:823-865) on one host frame ----
 * One upload, one download and one synchronisation; in the reference's order:
 *   - ComputeBoW (Frame.cc:570-577).  cur_node_id == NULL: the transform of cur->descriptors runs
 *     with levelsup as coeb_bow_transform's does, and word_out / node_out / weight_out (each may be
 *     NULL) receive what that call writes.  cur_node_id != NULL (length cur->n, the mFeatVec node
 *     that lists feature i or -1): mBowVec is already filled, the transform is skipped, no
 *     vocabulary is needed and the three outputs are not written.
 *   - SearchByBoW(pKF, F, vpMapPointMatches) with nnratio and check_orientation, as coeb_match_bow.
 *     The frame's angles are cur->keys_un[i].angle: UndistortKeyPoints copies the key and changes
 *     only pt, so this is mvKeys[i].angle.  *nmatches_bow = the return value.
 *   - the gate (:835): with *nmatches_bow < min_matches (the reference uses 15) the call stops:
 *     match_out holds SearchByBoW's assignments, discarded_out is all -1, Tcw is untouched,
 *     *ninliers_pose = 0, *nmatches = *nmatches_bow and *nmatches_map = 0.
 *   - PoseOptimization (:841) from Tcw (mLastFrame.mTcw, row-major 4x4) over the keypoints that got
 *     a match: position kf->world_pos[match], measurement cur->keys_un[i] with cur->u_right[i]
 *     (< 0: monocular edge), information the context's mvInvLevelSigma2.  Tcw holds the optimised
 *     pose on return; with fewer than 3 edges it is untouched and *ninliers_pose = 0, as in
 *     coeb_pose_optimization (reachable with min_matches <= 2).
 *   - the discard loop (:843-862): a matched keypoint flagged outlier loses its point, match_out[i]
 *     = -1 and discarded_out[i] = the KeyFrame index it had (the caller sets mbTrackInView = false
 *     and mnLastFrameSeen on that MapPoint); discarded_out is -1 everywhere else and may be NULL.
 *     *nmatches = *nmatches_bow minus the discarded; *nmatches_map = the kept keypoints whose point
 *     has observations > 0, which the caller compares with 10 (:864).
 * match_out has cur->n entries.  COEB_EINVAL, with nothing written, for a missing required pointer
 * or array, a negative size or levelsup, more than 4095 features on either side, cur_node_id ==
 * NULL before coeb_bow_set_vocabulary, or a keypoint octave outside the pyramid.  n == 0 on either
 * side is COEB_OK with zero counts. */
int coeb_track_reference_keyframe(coeb_ctx* ctx, const coeb_camera* cam, const coeb_curframe* cur,
                                  const int32_t* cur_node_id, int levelsup, const coeb_ref_keyframe* kf,
                                  float Tcw[16], float nnratio, int check_orientation, int min_matches,
                                  int32_t* word_out, int32_t* node_out, double* weight_out,
                                  int32_t* match_out, int32_t* discarded_out, int* nmatches_bow,
                                  int* ninliers_pose, int* nmatches, int* nmatches_map);

/* What Tracking::UpdateLastFrame (Tracking.cc:867-931) needs in localisation mode (mbOnlyTracking)
 * to create its "visual odometry" MapPoints on the last frame. */
typedef struct {
    const float* depth;               /* last->n, LastFrame.mvDepth */
    const uint8_t* descriptors;       /* last->n x 32, LastFrame.mDescriptors (a new MapPoint copies its row) */
    float th_depth;                   /* mThDepth */
    uint8_t* created_out;             /* last->n, 1 where a temporary MapPoint was created, else 0; may be NULL */
    float* created_pos;               /* last->n x 3, its position, written where created; may be NULL */
} coeb_vo_points;

/* The most LastFrame keypoints coeb_track_motion_model accepts with vo != NULL. */
#define COEB_VO_MAX_LAST 16384

/* ---- Tracking::TrackWithMotionModel (Tracking.cc:933-994) on one host frame ----
 * One upload, one download and one synchronisation; in the reference's order:
 *   - UpdateLastFrame's visual-odometry points (:878-930), only with vo != NULL (NULL: SLAM mode,
 *     :875 returns early).  The keypoints of `last` with vo->depth > 0 (NaN, 0 and negative are out)
 *     are taken in the order of sort(vector<pair<float,int>>), by depth then index, and walked until
 *     the first one farther than vo->th_depth with more than 100 counted.  A visited keypoint whose
 *     slot has !has_mappoint or mp_observations < 1 gets a new MapPoint: position
 *     Frame::UnprojectStereo(i) (Frame.cc:844-858: ((u - cx) z / fx, (v - cy) z / fy, z) from
 *     last->keys_un and cam, taken to the world by mRwc and mOw of Tcw_last), descriptor
 *     vo->descriptors[i], Observations() = 0.  last->outlier is left as it is: a replaced slot with
 *     mvbOutlier set is still skipped by the search.  The caller's arrays are not modified;
 *     vo->created_out / created_pos report what was created (the caller news the MapPoints and
 *     appends them to mlpTemporalPoints).  At most COEB_VO_MAX_LAST last-frame keypoints.
 *   - SearchByProjection(CurrentFrame, LastFrame, th, bMono) as coeb_match_lastframe, over the last
 *     frame as the step above left it, from the pose Tcw (mVelocity * mLastFrame.mTcw); with fewer
 *     than min_matches (the reference uses 20) the search runs again with 2 * th (:954-958).
 *     *nmatches_search = the final return value.
 *   - the gate (:960): with *nmatches_search < min_matches the call stops: match_out holds the last
 *     search's assignments, discarded_out is all -1, outlier_out all 0, Tcw is untouched,
 *     *ninliers_pose = 0, *nmatches = *nmatches_search and *nmatches_map = 0.
 *   - PoseOptimization (:964) from Tcw over the keypoints that got a match: position = that of the
 *     last-frame slot match_out[i] (created points included), measurement cur->keys_un[i] with
 *     cur->u_right[i] (< 0: monocular edge), information the context's mvInvLevelSigma2.  Tcw holds
 *     the optimised pose on return; with fewer than 3 edges it is untouched and *ninliers_pose = 0
 *     (reachable with min_matches <= 2).
 *   - the discard loop (:966-985): a matched keypoint flagged outlier loses its point, match_out[i] =
 *     -1 and discarded_out[i] = the last-frame slot it held (the caller sets mbTrackInView = false and
 *     mnLastFrameSeen on that MapPoint); discarded_out is -1 everywhere else.  outlier_out[i] = the
 *     optimiser's flag, 1 exactly on the discarded keypoints (the reference resets mvbOutlier there).
 *     *nmatches = *nmatches_search minus the discarded (the search's return counts assignments, so
 *     both can exceed the number of keypoints that hold a point); *nmatches_map = the kept keypoints whose point
 *     has Observations() > 0, so created points never count.  The caller applies :987-993: in
 *     localisation mode mbVO = *nmatches_map < 10 and the verdict is *nmatches > 20, otherwise the
 *     verdict is *nmatches_map >= 10.
 * match_out has cur->n entries; discarded_out and outlier_out (cur->n each) may be NULL.
 * COEB_EINVAL, with nothing written, for a missing required pointer or array, a negative size, more
 * than 4095 current keypoints, a last-frame or current keypoint octave outside the pyramid (every
 * keypoint of both frames is checked: which slots take a point is decided on the device), vo given
 * with depth or descriptors missing, or vo given with last->n > COEB_VO_MAX_LAST.  COEB_ERANGE, with
 * nothing written, when the two frames exceed the matcher's LDS budget (as coeb_match_lastframe
 * fails: 4095 current keypoints leave room for 14780 last-frame ones).  n == 0 on either side is
 * COEB_OK with zero counts. */
int coeb_track_motion_model(coeb_ctx* ctx, const coeb_camera* cam, const coeb_curframe* cur,
                            const coeb_lastframe* last, const coeb_vo_points* vo, const float Tcw_last[16],
                            float Tcw[16], float th, int bmono, int check_orientation, int min_matches,
                            int32_t* match_out, int32_t* discarded_out, uint8_t* outlier_out,
                            int* nmatches_search, int* ninliers_pose, int* nmatches, int* nmatches_map);

/* The most hypotheses one coeb_reloc_refine call refines. */
#define COEB_RELOC_MAX_HYP 16

/* One PnP hypothesis of Tracking::Relocalization: candidate KeyFrame i with the result of
 * vpPnPsolvers[i]->iterate (Tracking.cc:1490). */
typedef struct {
    coeb_keyframe_points kf;   /* vpCandidateKFs[i]->GetMapPointMatches(); valid = pMP && !isBad()
                                  only: sAlreadyFound is built by the call */
    const int32_t* match;      /* cur->n: KeyFrame index of vvpMapPointMatches[i][j], -1: none */
    const uint8_t* inlier;     /* cur->n: vbInliers[j] of PnPsolver::iterate */
    float Tcw[16];             /* in: the PnP pose; out: mCurrentFrame.mTcw as the reference leaves it */
} coeb_reloc_hypothesis;

/* ---- Tracking::Relocalization behind PnPsolver::iterate (Tracking.cc:1502-1565), nhyp hypotheses ----
 * The hypotheses of one round of the while loop (:1477-1568) do not depend on each other until the
 * first reaches nGood >= 50, so they are refined side by side: one upload, one download and one
 * synchronisation for all of them.  Each hypothesis h follows the reference literally:
 *   - entry (:1508-1517): mvpMapPoints[j] = inlier[j] ? match[j] : NULL; sFound = the inliers' points.
 *   - PoseOptimization (:1519) from Tcw, as coeb_pose_optimization: measurement cur->keys_un[j] with
 *     cur->u_right[j] (< 0: monocular edge), information the context's mvInvLevelSigma2, position
 *     kf.world_pos[match[j]], read whether or not kf.valid is set there.  With nGood < min_good (the
 *     reference uses 10) the hypothesis stops and keeps its inlier points, as `continue` does (stage 0).
 *   - the discard (:1524-1526): outliers lose their point and stay in sFound.  With nGood >=
 *     enough_good (50) the hypothesis is done (stage 1).
 *   - SearchByProjection(CurrentFrame, pKF, sFound, th1, orb_dist1) (:1531; 10, 100), as
 *     coeb_match_keyframe with cur_has_mappoint = mvpMapPoints != NULL, valid = kf.valid && !sFound and
 *     the optimised pose.  Its assignments enter mvpMapPoints even when nadditional1 + nGood <
 *     enough_good stops the hypothesis (stage 2).
 *   - PoseOptimization (:1535), with no discard in front of it: outlier-flagged keypoints keep their
 *     point.  With nGood outside (low_good, enough_good) (30, 50) the hypothesis is done (stage 3).
 *   - sFound rebuilt from every non-NULL mvpMapPoints, outlier-flagged ones included (:1541-1544), and
 *     SearchByProjection(.., th2, orb_dist2) (:1545; 3, 64).  nGood + nadditional2 < enough_good stops
 *     the hypothesis with the assignments made (stage 4).
 *   - PoseOptimization and the discard (:1550-1554) (stage 5).
 * check_orientation is matcher2's mbCheckOrientation (true in the reference).
 * Outputs, per hypothesis h, exactly what the reference leaves in mCurrentFrame after it, the failing
 * branches included: match_out[h * cur->n + j] = the KeyFrame index mvpMapPoints[j] holds or -1;
 * outlier_out[h * cur->n + j] = mvbOutlier[j], written only where keypoint j held a point at the last
 * optimisation that ran (elsewhere the reference's flag is whatever an earlier call left; the entry
 * is not touched); hyp[h].Tcw = mTcw; stage[h] = the branch that ended it (above); ngood[h] = the last
 * PoseOptimization return; nadditional1/2[h] = the searches' returns, 0 where a search did not run.
 * *first_good = the lowest h with ngood[h] >= enough_good, or -1: the candidate the reference's loop
 * breaks on (:1561-1565); the state of later hypotheses is what the reference would not have computed.
 * Assumption: a MapPoint occupies at most one index of a KeyFrame, so sFound over KeyFrame indices
 * equals the reference's set<MapPoint*>.
 * COEB_EINVAL, with nothing written and no Tcw touched, for a missing pointer or array (outlier_out
 * may be NULL), nhyp outside 1..COEB_RELOC_MAX_HYP, a negative size, cur->n > 4095, a match outside
 * [-1, kf.n), an inlier with match < 0, or a keypoint octave outside the pyramid (every keypoint is
 * checked: which take a point is decided on the device).  COEB_ERANGE, with nothing written, when any
 * (cur->n, kf.n) pair exceeds the relocalisation matcher's LDS budget (as coeb_match_keyframe fails),
 * decided before anything is enqueued.  cur->n == 0 is COEB_OK with zero counts and stage 0. */
int coeb_reloc_refine(coeb_ctx* ctx, const coeb_camera* cam, const coeb_curframe* cur,
                      coeb_reloc_hypothesis* hyp, int nhyp,
                      float th1, int orb_dist1, float th2, int orb_dist2,   /* 10,100, 3,64 */
                      int check_orientation,                               /* matcher2(0.9,true) */
                      int min_good, int low_good, int enough_good,         /* 10, 30, 50 */
                      int32_t* match_out,   /* nhyp x cur->n: KeyFrame index mvpMapPoints[j] holds, -1 */
                      uint8_t* outlier_out, /* nhyp x cur->n, may be NULL */
                      int32_t* ngood, int32_t* nadditional1, int32_t* nadditional2,
                      int32_t* stage, int* first_good);

/* ---- BowVector filling: addWeight in feature order, then normalize(L1) (host only, no context) ----
 * For every feature i < n with node[i] >= 0 (coeb_bow_transform's "weight > 0"), in order:
 * value[word[i]] += weight[i] when the word is present (sequential double adds, not count * weight),
 * else the word is inserted with weight[i].  With normalize_l1: norm = the sum of fabs(value) in
 * ascending word order; when norm > 0.0 every value /= norm.  word_out / value_out (cap entries)
 * get the words ascending; more than cap words: COEB_ERANGE with *nw_out set, nothing written. */
int coeb_bow_vector(const int32_t* word, const double* weight, const int32_t* node, int n, int normalize_l1,
                    int32_t* word_out, double* value_out, int cap, int* nw_out);

/* ---- the keyframe database: KeyFrameDatabase::add / erase / clear and the query half of
 * DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:40-73, 199-253), SearchByBoW against
 * many keyframes (the loop of Tracking::Relocalization, src/Tracking.cc:1449-1470) ----
 * A database lives on its context's device and stream, holds per keyframe what never changes after
 * KeyFrame::ComputeBoW and is bound by the context's non-reentrancy rule.  Destroy it before its
 * context (coeb_destroy releases the device memory of the databases still alive; their handles
 * then only take coeb_kfdb_destroy).  BowVector scoring restates DBoW2's L1Scoring; parity against
 * DBoW2 itself is UNPINNED. */
typedef struct coeb_kfdb coeb_kfdb;
typedef struct {
    int32_t n;                        /* pKF->N */
    const uint8_t* descriptor;        /* n x 32, pKF->mDescriptors */
    const int32_t* node_id;           /* the mFeatVec node that lists feature i, -1: none */
    const float* angle;               /* pKF->mvKeysUn[i].angle */
    const int32_t* bow_word;          /* pKF->mBowVec: nw word ids, strictly ascending */
    const double* bow_value;          /* ... and their values */
    int32_t nw;
} coeb_kfdb_keyframe;
/* max_features (1..4095) bounds n and nw of every keyframe and nw of a query; initial_slots >= 1. */
int coeb_kfdb_create(coeb_ctx* ctx, int max_features, int initial_slots, coeb_kfdb** db);
void coeb_kfdb_destroy(coeb_kfdb* db);
/* One staged upload; the keyframe's feature-vector CSR is built once, over all features with
 * node_id >= 0.  *slot_out = the lowest free slot; past the allocated slots the storage doubles
 * (slot ids stay valid).  Every add takes the next insertion sequence number.  COEB_EINVAL when n
 * or nw exceeds max_features or bow_word is not strictly ascending. */
int coeb_kfdb_add(coeb_kfdb* db, const coeb_kfdb_keyframe* kf, int* slot_out);
int coeb_kfdb_erase(coeb_kfdb* db, int slot);       /* COEB_EINVAL for an empty or out-of-range slot */
int coeb_kfdb_clear(coeb_kfdb* db);
/* nslots = one past the highest slot ever handed out (the length of the query's arrays). */
int coeb_kfdb_size(const coeb_kfdb* db, int* nkeyframes, int* nslots);
/* The query BowVector (word ascending, nw <= max_features) against every keyframe:
 * common[slot] = |words(F) & words(KF)| = mnRelocWords (0 for empty slots); *max_common its
 * maximum; *min_common = (int)(max_common * 0.8f); score[slot] = (float)L1Scoring::score(F, KF)
 * where common[slot] > *min_common, -1.0f elsewhere; order[0 .. *n_sharing) = the slots with
 * common > 0 as lKFsSharingWords lists them (ascending smallest common word, then insertion).
 * common, score, order hold nslots entries.  An empty database or nw == 0: all three counts 0. */
int coeb_kfdb_query(coeb_kfdb* db, const int32_t* word, const double* value, int nw, int32_t* common,
                    float* score, int32_t* order, int* n_sharing, int* max_common, int* min_common);
/* coeb_match_bow of `cur` against keyframes slots[0 .. ncand) (ncand <= 256; a slot may repeat),
 * candidate j with valid[j] (n_kf bytes: vpMapPointsKF[i] && !isBad(), may be NULL when n_kf is 0):
 * match_out[j][cur->n] and nmatches[j] are what coeb_match_bow returns for that keyframe.  One
 * upload, one download, one synchronisation.  COEB_EINVAL (nothing written) for an empty or
 * out-of-range slot or more than 256 candidates. */
int coeb_match_bow_kfdb(coeb_kfdb* db, const int32_t* slots, int ncand, const uint8_t* const* valid,
                        const coeb_bow_frame* cur, float nnratio, int check_orientation, int32_t* match_out,
                        int32_t* nmatches);

/* ---- ORBmatcher::SearchForTriangulation against many keyframes (src/ORBmatcher.cc:657-824, the
 * loop of LocalMapping::CreateNewMapPoints, src/LocalMapping.cc:255-270) ----
 * coeb_kfdb_set_geometry uploads what the search reads of a stored keyframe beyond coeb_kfdb_add's
 * arrays: mvKeysUn[i].pt, mvKeysUn[i].octave and mvuRight[i] of the slot's n features (const
 * members of KeyFrame).  They live in a slab of their own (16 bytes per feature, allocated by the
 * first call, growing with the slots); erase, clear and the reuse of a slot drop them, a second call
 * replaces them.  COEB_EINVAL for an empty or out-of-range slot, a NULL array with n > 0 or an
 * octave outside the context's pyramid. */
int coeb_kfdb_set_geometry(coeb_kfdb* db, int slot, const coeb_keypoint* keys_un, const float* u_right);
#define COEB_TRI_MAX_NEIGHBOURS 32
/* SearchForTriangulation(pKF1 = slot1, pKF2 = slots2[j], F12[j], vMatchedPairs, only_stereo) of an
 * ORBmatcher(_, check_orientation) for j < nnb (nnb <= 32; a slot may repeat and may be slot1), in
 * one upload, one download and one synchronisation.  has_mp1[i] = pKF1->GetMapPoint(i) != NULL,
 * has_mp2[j][i] likewise for neighbour j (may be NULL where that keyframe has no features).
 * F12 [nnb][9] row-major and epipole [nnb][2] = {ex, ey} (:664-670) are the caller's: nothing is
 * derived from poses here.  match_out[j][n1] = vMatches12 (the feature of keyframe 2 or -1; the pair
 * list of :816-821 is its ascending read), nmatches[j] = the return value.  mvScaleFactors and
 * mvLevelSigma2 are the context's.  The line and epipole tests are written with the fused
 * multiply-adds the reference binary shows; parity against the binary is UNPINNED.
 * COEB_EINVAL, with nothing written, for a slot that is empty, out of range or without geometry,
 * nnb outside 0..32 or a missing pointer; nnb == 0 or a keyframe without features: COEB_OK, counts 0. */
int coeb_kfdb_search_triangulation(coeb_kfdb* db, int slot1, const uint8_t* has_mp1, const int32_t* slots2, int nnb,
                                   const uint8_t* const* has_mp2, const float* F12, const float* epipole,
                                   int only_stereo, int check_orientation, int32_t* match_out, int32_t* nmatches);

/* ---- the loop body of LocalMapping::CreateNewMapPoints for all neighbours (src/LocalMapping.cc:271-433) ----
 * coeb_kfdb_set_stereo uploads what the triangulation reads of a stored keyframe beyond the geometry: the raw
 * mvKeys[i].pt (key_xy [n][2]; KeyFrame::UnprojectStereo, src/KeyFrame.cc:615-631) and mvDepth[i] of the
 * slot's n features.  They live in a slab of their own (16 bytes per feature, allocated by the first call,
 * growing with the slots); erase, clear and the reuse of a slot drop them, a second call replaces them.
 * COEB_EINVAL for an empty or out-of-range slot, a NULL array with n > 0 or an entry that is not finite. */
int coeb_kfdb_set_stereo(coeb_kfdb* db, int slot, const float* key_xy, const float* depth);
typedef struct {                       /* one keyframe as the loop reads it; nothing is derived here */
    float Rcw[9], tcw[3], Ow[3];       /* GetRotation / GetTranslation / GetCameraCenter (Rwc is Rcw transposed) */
    float fx, fy, cx, cy, invfx, invfy, mb, mbf;
} coeb_kf_view;
/* status[j][i]: the low four bits say how the pair (i, match_out[j][i]) left the loop body */
#define COEB_NEWPTS_NO_PAIR 0          /* match_out[j][i] < 0 */
#define COEB_NEWPTS_ACCEPTED 1         /* reached `new MapPoint` (:435) */
#define COEB_NEWPTS_LOW_PARALLAX 2     /* :350, no stereo and very low parallax */
#define COEB_NEWPTS_W_ZERO 3           /* :334, x3D[3] == 0 */
#define COEB_NEWPTS_Z1 4               /* :356 */
#define COEB_NEWPTS_Z2 5               /* :360 */
#define COEB_NEWPTS_REPROJ1 6          /* :375 / :386 */
#define COEB_NEWPTS_REPROJ2 7          /* :401 / :412 */
#define COEB_NEWPTS_ZERO_DIST 8        /* :423 */
#define COEB_NEWPTS_RATIO 9            /* :431 */
/* ... and (status >> 4) & 3 where x3D came from (0 for the first two ways out above and for low parallax) */
#define COEB_NEWPTS_SRC_TRIANGULATED 1 /* :321-340 */
#define COEB_NEWPTS_SRC_STEREO1 2      /* :343, pKF1->UnprojectStereo(idx1) */
#define COEB_NEWPTS_SRC_STEREO2 3      /* :347, pKF2->UnprojectStereo(idx2) */
/* SearchForTriangulation(pKF1 = slot1, pKF2 = slots2[j], F12[j], vMatchedIndices, only_stereo) of an
 * ORBmatcher(0.6, false) and then :285-433 on its pairs, for every neighbour j < nnb (nnb <= 32) in one
 * upload, one download and one synchronisation.  view1 / views2[j] are the caller's poses and cameras;
 * ratioFactor = 1.5f * mfScaleFactor, mvScaleFactors and mvLevelSigma2 are the context's.  The search's
 * arguments are coeb_kfdb_search_triangulation's, without check_orientation.  Dense and neighbour-major, n1
 * entries per neighbour:
 *   match_out[j][i]  what coeb_kfdb_search_triangulation returns with check_orientation = 0;
 *   status[j][i]     above; a pure function of the pair, whatever other neighbours decide;
 *   x3d[j][i][3]     x3D of an accepted pair, untouched for every other entry;
 *   first_ok[i]      the lowest j with (status & 15) == COEB_NEWPTS_ACCEPTED, else -1: a feature that got its
 *                    MapPoint from an earlier neighbour is skipped by the later ones, so the host creates
 *                    MapPoints for exactly the pairs (first_ok[i], i) in (j, i) ascending order;
 *   nmatches[j]      the pairs of neighbour j.
 * The null vector of the 4x4 system is a one-sided Jacobi's in float32, a canonical form that differs from
 * cv::SVD by construction, and the stereo parallax bound cos(2 atan2(mb / 2, depth)) is evaluated as
 * (d^2 - h^2) / (d^2 + h^2) in double; the float forms are listed in DESIGN.md s2.1 and parity against the
 * reference binary is UNPINNED.
 * COEB_EINVAL, with nothing written: the refusals of coeb_kfdb_search_triangulation; a slot without
 * geometry or stereo data; a pose or camera entry that is not finite; a stored feature with u_right >= 0 and
 * depth <= 0 (UnprojectStereo returns an empty Mat there); a repeated neighbour slot or slots2[j] == slot1.
 * nnb == 0 or a keyframe 1 without features: COEB_OK, counts 0, first_ok all -1. */
int coeb_kfdb_create_new_map_points(coeb_kfdb* db, int slot1, const coeb_kf_view* view1, const uint8_t* has_mp1,
                                    const int32_t* slots2, int nnb, const coeb_kf_view* views2,
                                    const uint8_t* const* has_mp2, const float* F12, const float* epipole,
                                    int only_stereo, int32_t* match_out, int8_t* status, float* x3d,
                                    int32_t* first_ok, int32_t* nmatches);

/* ---- ORBmatcher::Fuse's search against many stored keyframes (src/ORBmatcher.cc:826-951, the loops of
 * LocalMapping::SearchInNeighbors, src/LocalMapping.cc:455-535) ----
 * The search half of Fuse (bestIdx, bestDist) is a pure function of the point, the keyframe's constant
 * features, its pose and the camera; the skips and the action (Replace / AddObservation, :953-971)
 * depend on the map's state and stay on the host (adapter/LocalMapping_coeb.h). */
typedef struct {                       /* the MapPoints of a call, as Fuse reads them */
    int32_t n;
    const uint8_t* valid;              /* pMP && !pMP->isBad() */
    const float* world_pos;            /* n x 3 */
    const float* normal;               /* n x 3 */
    const float* max_distance;         /* mfMaxDistance (invariance = 1.2f * it; PredictScale reads it raw) */
    const float* min_distance;         /* mfMinDistance (0.8f * it) */
    const uint8_t* descriptor;         /* n x 32 */
} coeb_fuse_points;
typedef struct {
    int32_t slot;                      /* a stored keyframe with geometry */
    float Rcw[9], tcw[3], Ow[3];       /* GetRotation / GetTranslation / GetCameraCenter: the caller's, nothing derived here */
    int32_t first, count;              /* the points first .. first+count of the list */
    const uint8_t* skip;               /* count bytes, pMP->IsInKeyFrame(pKF); may be NULL */
} coeb_fuse_job;
#define COEB_FUSE_MAX_JOBS 128
/* The (job, point) pairs of one call, and the points of its list.  A pair costs 8 bytes of result and a
 * point 56 bytes of upload in the page-locked staging buffer and on the device: at most 8 MiB + 56 MiB
 * (about 64 MiB on each side).  128 targets over a list of 8192 points take 8.5 MiB. */
#define COEB_FUSE_MAX_PAIRS (1 << 20)
/* For job j and its point i (entry = the counts of the jobs before j, plus i - first): the search of
 * Fuse(KF[slot], points, th) for that point.  best_idx = bestIdx where bestDist <= TH_LOW (50), else -1;
 * best_dist = bestDist (256 when no candidate was accepted).  A point with valid 0 or skip 1, or one
 * the projection tests reject, gets -1 / 256.  Jobs may repeat a slot and overlap in range.  One upload,
 * one download, one synchronisation.  The keyframe's 64 x 48 feature grid (AssignFeaturesToGrid under
 * cam's bounds) is built on the device by the first call that names the slot and kept with it; add on a
 * reused slot, erase, clear and coeb_kfdb_set_geometry drop it, other bounds rebuild it.
 * mvScaleFactors, mvInvLevelSigma2, mfLogScaleFactor and mnScaleLevels are the context's.  The float
 * forms are listed in DESIGN.md s2.1; parity against the reference binary is UNPINNED.
 * COEB_EINVAL, with nothing written: a slot that is empty, out of range or without geometry; njobs
 * outside 0..128; a range outside the list; a missing array; th or a pose entry that is not finite (th
 * negative); camera bounds that are not finite with max > min; a valid point with a non-finite position
 * or normal, or whose distances are not 0 < min <= max < inf.  COEB_ERANGE: more than
 * COEB_FUSE_MAX_PAIRS pairs or points.  njobs == 0 or all counts 0: COEB_OK. */
int coeb_kfdb_fuse_search(coeb_kfdb* db, const coeb_camera* cam, const coeb_fuse_points* pts,
                          const coeb_fuse_job* jobs, int njobs, float th,
                          int32_t* best_idx, int32_t* best_dist);   /* job-major, sum of counts entries */

/* The Frame fields Optimizer::PoseOptimization reads (Optimizer.cc:276-357). */
typedef struct {
    int32_t n;                        /* pFrame->N */
    const uint8_t* has_mappoint;      /* mvpMapPoints[i] != NULL */
    const float* world_pos;           /* n x 3, GetWorldPos() (read where has_mappoint) */
    const coeb_keypoint* keys_un;     /* mvKeysUn (pt, octave) */
    const float* u_right;             /* mvuRight (< 0: monocular edge) */
} coeb_pose_frame;

/* ---- Optimizer::PoseOptimization(pFrame) ----
 * Tcw: pFrame->mTcw on entry (row-major 4x4), the optimised pose on return (SetPose).
 * outlier_out[i] (length n) = mvbOutlier[i], written where has_mappoint[i].  *ninliers = the
 * return value (nInitialCorrespondences - nBad; 0 and Tcw untouched with < 3 edges).  The
 * information matrices use the context's mvInvLevelSigma2; cam supplies fx, fy, cx, cy, mbf. */
int coeb_pose_optimization(coeb_ctx* ctx, const coeb_camera* cam, const coeb_pose_frame* frame, float Tcw[16],
                           uint8_t* outlier_out, int* ninliers);

/* ---- Frame helpers ---- */
int coeb_blur_flags(coeb_ctx* ctx, const uint8_t* gray, int width, int height, size_t stride,
                    const coeb_box* boxes, int nbox, int32_t* flags_out);
int coeb_stereo_from_rgbd(coeb_ctx* ctx, const coeb_keypoint* kps, int n, const float* depth,
                          int width, int height, size_t depth_stride_floats, float bf,
                          float* u_right_out, float* depth_out);
/* Tracking::GrabImageRGBD's input conversions (src/Tracking.cc:212-228).
 * img: `channels` = 1 (8UC1, copied), 3 (8UC3: RGB2GRAY when rgb_order = 1, as Camera.RGB = 1,
 * else BGR2GRAY) or 4 (8UC4: RGBA2GRAY / BGRA2GRAY, alpha ignored); img_stride in bytes.
 * depth: depth_type COEB_DEPTH_U16 (16UC1) or COEB_DEPTH_F32 (32FC1), depth_stride in bytes;
 * imDepth.convertTo(CV_32F, depth_scale) with depth_scale = mDepthMapFactor (= 1/DepthMapFactor),
 * except that a 32F map with |depth_scale - 1| <= 1e-5 is passed through unchanged (:227).
 * Either input may be NULL. */
#define COEB_DEPTH_U16 0
#define COEB_DEPTH_F32 1
int coeb_rgbd_preprocess(coeb_ctx* ctx, const uint8_t* img, size_t img_stride, int channels, int rgb_order,
                         const void* depth, size_t depth_stride, int depth_type, float depth_scale,
                         int width, int height, uint8_t* gray_out, float* depth_out);

/* The same conversions over a packed device batch: d_img nframes x height x width x channels,
 * d_depth nframes x height x width (16UC1 or 32FC1), outputs packed gray / float depth; width a
 * multiple of 4, image buffers 4-byte and depth buffers 16-byte aligned.  Enqueued on the
 * context stream (the batch pipeline's first step, BASELINE configs[4]). */
int coeb_rgbd_preprocess_batch_device(coeb_ctx* ctx, const uint8_t* d_img, int channels, int rgb_order,
                                      const void* d_depth, int depth_type, float depth_scale, int nframes, int width,
                                      int height, uint8_t* d_gray, float* d_depth_out);
/* mvKeysUn from mvKeys: cv::undistortPoints(.., mK, mDistCoef, Mat(), mK) (OpenCV 3.4, 5
 * iterations) with dist = (k1, k2, p1, p2, k3) (k3 = 0 for a 4-coefficient mDistCoef);
 * dist[0] == 0 copies (Frame.cc:581-585).  out may equal kps. */
int coeb_undistort_keypoints(coeb_ctx* ctx, const coeb_camera* cam, const float dist[5], const coeb_keypoint* kps,
                             int n, coeb_keypoint* out);
/* Frame RGB-D ctor tail on one host frame (src/Frame.cc:214-223): ORBextractor::operator(),
 * UndistortKeyPoints (:579-609), ComputeStereoFromRGBD (:820-842), one synchronisation.
 * gray / stride / boxes / tm_xy / blur_flag / cap / n_out as in coeb_extract (an empty image
 * returns COEB_OK with *n_out = 0; n > cap returns COEB_ERANGE with the first cap entries of every
 * output written); kp_out and desc_out are byte-identical to coeb_extract's.
 * depth: width x height, depth_stride in bytes, depth_type / depth_scale as in
 * coeb_rgbd_preprocess (a 32F map with |depth_scale - 1| <= 1e-5 is read unchanged); only the
 * values under the keypoints are converted, so a 16U map needs no convertTo beforehand
 * (Tracking.cc:227).  dist = (k1, k2, p1, p2, k3); NULL or dist[0] == 0 copies the keys
 * (Frame.cc:581-585).  cam supplies fx, fy, cx, cy (undistortion) and bf.  Per keypoint i:
 * d = depth(int(kp.y), int(kp.x)) at the RAW keypoint; depth_out[i] = d > 0 ? d : -1;
 * u_right_out[i] = d > 0 ? kp_un.x - bf / d : -1 from the UNDISTORTED x (:829-839); NaN and
 * negative depth give -1.  kp_un_out may be NULL; the other outputs are required.  The context
 * holds the frame afterwards as after coeb_extract (coeb_debug_read). */
int coeb_frame_rgbd(coeb_ctx* ctx, const uint8_t* gray, int width, int height, size_t stride,
                    const void* depth, size_t depth_stride, int depth_type, float depth_scale,
                    const coeb_camera* cam, const float dist[5],
                    const coeb_box* boxes, int nbox, const float* tm_xy, int ntm,
                    const int32_t* blur_flag, int nblur,
                    coeb_keypoint* kp_out, coeb_keypoint* kp_un_out, uint8_t* desc_out,
                    float* u_right_out, float* depth_out, int cap, int* n_out);
/* yolov5_ros_msgs/BoundingBox (int64 xmin, ymin, xmax, ymax) -> coeb_box, as GrabRGBD converts */
int coeb_boxes_from_int64(const int64_t* xyxy, int nbox, coeb_box* out);

/* ---- TUM RGB-D time-stamp lists (associate.py, the ingest step before GrabImageRGBD) ----
 * Host-only (no context, no device).  coeb_tum_read_list parses a list file's text
 * (associate.py:49-69): lines split at '\n'; ',' and TAB separate fields like ' '; a line whose
 * first byte is '#' is a comment; lines with fewer than two fields are ignored; the first field
 * must be a decimal float literal (else COEB_EINVAL, where read_file_list raises).  A stamp that
 * occurs twice keeps its last line at the position of its first (the reference's dict).  Per
 * entry: the stamp, and the byte offset / length in `text` of its data fields (second field to
 * the end of the last).  *n_out = entries; COEB_ERANGE when that exceeds cap (nothing written).
 * coeb_tum_associate (associate.py:71-102): candidates |a - (b + offset)| < max_difference in
 * double, taken greedily by increasing (difference, a, b), each stamp once, returned as index
 * pairs into first / second ordered by (a, b); a stamp given twice is its last index, NaN never
 * matches.  *n_out = matches; COEB_ERANGE when that exceeds cap. */
int coeb_tum_read_list(const char* text, size_t len, double* stamps, int64_t* data_off, int32_t* data_len, int cap,
                       int* n_out);
int coeb_tum_associate(const double* first, int n_first, const double* second, int n_second, double offset,
                       double max_difference, int32_t* first_idx, int32_t* second_idx, int cap, int* n_out);

/* ---- Frame::ProcessMovingObject (src/Frame.cc:311-393): T_M from imGrayPre and imgray ----
 * Each stage replaces the OpenCV 3.4 call Frame.cc makes, in the canonical forms of DESIGN.md
 * s2.1 / s4.10 (parity against the oracle; OpenCV itself is absent, parity vs it UNPINNED):
 *   coeb_good_features        <- cv::goodFeaturesToTrack(img, pts, 1000, 0.01, 8, Mat(), 3, true, 0.04)  :333
 *                                (*n_out = corner count; COEB_ERANGE past 16384 local maxima)
 *   coeb_corner_subpix        <- cv::cornerSubPix(img, pts, Size(10,10), Size(-1,-1), (ITER|EPS, 20, 0.03))  :334
 *                                (in place; win must be 10)
 *   coeb_optical_flow_pyr_lk  <- cv::calcOpticalFlowPyrLK(prev, next, pts, next_pts, status, err,
 *                                Size(22,22), 5, (ITER|EPS, 20, 0.01))  :335  (win <= 22)
 *   coeb_moving_tail          <- the SAD check (:337-365), cv::findFundamentalMat(.., FM_RANSAC, 0.1, 0.99)
 *                                (:373) and the epipolar distance test (:375-384); state in/out
 *   coeb_moving_object_points <- the whole of ProcessMovingObject; *n_tm = |T_M|, or -1 when
 *                                findFundamentalMat returns an empty Mat (the reference then reads
 *                                an empty Mat: undefined behaviour)
 * At most 1024 points per call (the reference asks for 1000 corners). */
typedef struct {
    float* corners_raw;   /* 1000 x 2: goodFeaturesToTrack output (optional) */
    float* corners;       /* 1000 x 2: after cornerSubPix (optional) */
    int* ncorners;
    float* next_pts;      /* 1000 x 2: calcOpticalFlowPyrLK output */
    uint8_t* status;      /* 1000: LK status */
    uint8_t* state;       /* 1000: state after the SAD check */
    double* F;            /* 9: the fundamental matrix */
    int* nf;              /* |F_prepoint| */
} coeb_flow_debug;
int coeb_good_features(coeb_ctx* ctx, const uint8_t* img, int width, int height, size_t stride, int max_corners,
                       double quality, double min_distance, double k, float* xy_out, int cap, int* n_out);
int coeb_corner_subpix(coeb_ctx* ctx, const uint8_t* img, int width, int height, size_t stride, float* xy, int n,
                       int win, int max_iter, double eps);
int coeb_optical_flow_pyr_lk(coeb_ctx* ctx, const uint8_t* prev, const uint8_t* next, int width, int height,
                             size_t stride, const float* prev_xy, int n, int win, int max_level, int max_count,
                             double eps, float* next_xy, uint8_t* status);
int coeb_moving_tail(coeb_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int width, int height, size_t stride,
                     const float* prev_xy, const float* next_xy, uint8_t* state, int n, float* tm_xy, int tm_cap,
                     int* n_tm, double F_out[9], int* nf_out);
int coeb_moving_object_points(coeb_ctx* ctx, const uint8_t* prev, const uint8_t* cur, int width, int height,
                              size_t stride, float* tm_xy, int tm_cap, int* n_tm, coeb_flow_debug* dbg);
/* the same on device-resident frames (pitch stride) */
int coeb_moving_object_points_device(coeb_ctx* ctx, const uint8_t* d_prev, const uint8_t* d_cur, int width,
                                     int height, size_t stride, float* tm_xy, int tm_cap, int* n_tm,
                                     coeb_flow_debug* dbg);

/* ---- The RGB-D Frame constructor on a stream of frames (src/Frame.cc:157-223), one call per frame ----
 * A coeb_rgbd_stream keeps what the constructor needs of the previous frame on the device (gray
 * level 0, its LK pyramid, Scharr derivatives and refined corners), in memory of its own: other
 * calls on the context between two frames, and other streams on the same context, do not touch it.
 * Call f computes what coeb_moving_object_points(frame f-1, frame f) -> coeb_blur_flags(frame f) ->
 * coeb_frame_rgbd(frame f, boxes, that T_M, those flags) compute, bit for bit, with one upload (the
 * boxes and the image rows; the depth rows are not uploaded: as in coeb_frame_rgbd they stay in
 * page-locked host memory, where the tail kernel reads the values under the keypoints), one pyramid
 * and one synchronisation: T_M and the flags never leave the device on their way to the extraction.  img / channels / rgb_order as coeb_rgbd_preprocess (1-channel rows are mImGray itself);
 * depth / cam / dist / cap as coeb_frame_rgbd; at most COEB_MAX_BOXES boxes; width and height >= 32.
 * A frame without predecessor (the first, or the first after coeb_rgbd_stream_reset) is a first
 * frame (:205-209): first = 1, n_tm = 0, every flag 0, extraction without T_M.  n_tm = -1:
 * findFundamentalMat returned an empty matrix; the frame is then extracted without T_M, as
 * coeb_frame_batch_device does.  At most min(n_tm, tm_cap) points are written to tm_xy.
 * Errors: COEB_EINVAL (nothing written, the stream unchanged) for a bad argument or a size that
 * differs from the previous frame's without a reset; COEB_ERANGE with n > cap as coeb_frame_rgbd;
 * COEB_ERANGE with nothing written when the PREVIOUS frame had more corner candidates than the
 * exact selection covers (as coeb_moving_object_points on that pair) -- the stream then carries on
 * with the current frame as the next predecessor.  An empty image returns COEB_OK with n = 0 and
 * leaves the stream as it was.
 * The previous-frame-only work (goodFeaturesToTrack, cornerSubPix, the Scharr derivatives) of frame
 * f runs behind call f on a HIP stream the object owns, and call f + 1 waits for it on the device;
 * with COEB_STREAM_NO_SHADOW it runs at the start of call f + 1 on the context stream instead.
 * Destroy the stream before its context. */
typedef struct coeb_rgbd_stream coeb_rgbd_stream;
#define COEB_STREAM_NO_SHADOW 1   /* previous-frame-only work runs inside the next call instead of behind this one */
int coeb_rgbd_stream_create(coeb_ctx* ctx, unsigned flags, coeb_rgbd_stream** out);
void coeb_rgbd_stream_destroy(coeb_rgbd_stream* st);      /* before coeb_destroy(ctx); joins the shadow work */
int coeb_rgbd_stream_reset(coeb_rgbd_stream* st);         /* the next frame has no imGrayPre (sequence start, tracking reset) */

typedef struct {
    float* tm_xy; int tm_cap; int n_tm;        /* T_M in the reference's order; n_tm = -1: F empty; 0 on a first frame */
    int32_t* blur_flag;                        /* nbox flags (Frame.cc:171-202); all 0 on a first frame (:205-209) */
    uint8_t* gray; size_t gray_stride;         /* optional: mImGray as GrabImageRGBD makes it */
    coeb_keypoint *kp, *kp_un; uint8_t* desc; float *u_right, *depth; int cap; int n;   /* as coeb_frame_rgbd */
    int first;                                 /* 1 when the frame had no predecessor */
} coeb_rgbd_stream_out;

int coeb_rgbd_stream_frame(coeb_rgbd_stream* st,
                           const uint8_t* img, size_t img_stride, int channels, int rgb_order,
                           int width, int height,
                           const void* depth, size_t depth_stride, int depth_type, float depth_scale,
                           const coeb_camera* cam, const float dist[5],
                           const coeb_box* boxes, int nbox,
                           coeb_rgbd_stream_out* out);

int coeb_descriptor_distance(const uint8_t* a, const uint8_t* b);

/* ---- device memory owned by the caller (for the device-resident batch entry points) ----
 * Plain hipMalloc'ed buffers on the context's device.  Copies are synchronous w.r.t. the
 * context stream (they are enqueued on it and waited for). */
int coeb_device_alloc(coeb_ctx* ctx, size_t bytes, void** dptr);
int coeb_device_free(coeb_ctx* ctx, void* dptr);
int coeb_memcpy_h2d(coeb_ctx* ctx, void* dst, const void* src, size_t bytes);
int coeb_memcpy_d2h(coeb_ctx* ctx, void* dst, const void* src, size_t bytes);
/* Host-resident batches with copy / kernel overlap: page-locked host memory, and copies
 * enqueued on the context stream behind the work already there (returning at once; the data
 * is in place after coeb_synchronize).  From page-locked memory the copies run on the DMA
 * engines beside the kernels of other contexts' streams. */
int coeb_host_alloc(size_t bytes, void** ptr);
int coeb_host_free(void* ptr);
int coeb_memcpy_h2d_async(coeb_ctx* ctx, void* dst, const void* src, size_t bytes);
int coeb_memcpy_d2h_async(coeb_ctx* ctx, void* dst, const void* src, size_t bytes);
/* Copy queues: a HIP stream of their own on a context's device, for pipelines whose uploads
 * must run back to back (one upload queue for all batches: concurrent uploads only split the
 * PCIe bandwidth) while earlier batches compute on the contexts' streams.  Copies are
 * asynchronous (page-locked host memory); ordering against a context is explicit:
 *   coeb_copyq_after_ctx(q, ctx)  work enqueued on q from now on waits for everything enqueued
 *                                 on ctx so far (e.g. the kernels reading the buffer to refill);
 *   coeb_ctx_after_copyq(ctx, q)  work enqueued on ctx from now on waits for everything
 *                                 enqueued on q so far (e.g. the upload of the next batch). */
typedef struct coeb_copyq coeb_copyq;
coeb_copyq* coeb_copyq_create(coeb_ctx* ctx);
int coeb_copyq_destroy(coeb_copyq* q);
int coeb_copyq_h2d(coeb_copyq* q, void* dst, const void* src, size_t bytes);
int coeb_copyq_d2h(coeb_copyq* q, void* dst, const void* src, size_t bytes);
int coeb_copyq_after_ctx(coeb_copyq* q, coeb_ctx* ctx);
int coeb_ctx_after_copyq(coeb_ctx* ctx, coeb_copyq* q);
int coeb_copyq_synchronize(coeb_copyq* q);
/* Markers: a point recorded on a context or copy queue now and waited for later (by another
 * context or queue, or by the host), for pipelines whose waits refer to work enqueued several
 * steps earlier (e.g. "the kernels of batch i - 3 are done with this input buffer"). */
typedef struct coeb_marker coeb_marker;
coeb_marker* coeb_marker_create(coeb_ctx* ctx);
int coeb_marker_destroy(coeb_marker* m);
int coeb_marker_record_ctx(coeb_marker* m, coeb_ctx* ctx);       /* after all work enqueued on ctx */
int coeb_marker_record_copyq(coeb_marker* m, coeb_copyq* q);     /* after all work enqueued on q */
int coeb_ctx_wait_marker(coeb_ctx* ctx, coeb_marker* m);         /* later work on ctx waits for m */
int coeb_copyq_wait_marker(coeb_copyq* q, coeb_marker* m);       /* later work on q waits for m */
int coeb_marker_synchronize(coeb_marker* m);                     /* host waits for m */

/* ---- measurement ---- */
/* Per-kernel device time accumulated with HIP events on the context stream while profiling
 * is enabled.  names: comma-separated list written to `names` (cap bytes). */
int coeb_profile_enable(coeb_ctx* ctx, int enable);
int coeb_profile_read(coeb_ctx* ctx, char* names, int cap, double* total_ms, int64_t* launches,
                      int max_kernels, int* nkernels);
int coeb_profile_reset(coeb_ctx* ctx);
int coeb_synchronize(coeb_ctx* ctx);
int coeb_device_count(void);

/* Test support: copy an intermediate buffer of frame `frame` of the last batch to the host.
 * what: "pyr" (levels 1..L-1, packed), "blur" (levels 0..L-1), "cand_n" (FAST corners per
 * cell), "lvl_n" (keypoints per level), "lvl_kp" (packed level keypoints), "dyn" (mask
 * rectangles), "plan", "u_right" / "kp_depth" (float mvuRight / mvDepth of the frame's keypoint
 * slots as the last coeb_match_batch_device* computed them from the frame's own depth map;
 * COEB_EINVAL before any batch match), "search_path" (int32 {path, iterations} of the last
 * coeb_match_localmap / coeb_match_keyframe / coeb_search_local_points / coeb_track_local_map: 0 parallel claims, 1 forced sequential,
 * 2 candidate-list overflow, 3 no convergence; frame ignored; alias "localmap_path").  Copies min(bytes, size); *size_out = full size. */
int coeb_debug_read(coeb_ctx* ctx, const char* what, int frame, void* host, size_t bytes, size_t* size_out);

#ifdef __cplusplus
}
#endif
#endif
