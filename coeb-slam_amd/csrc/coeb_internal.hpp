// coeb_internal.hpp -- shared host/device definitions of the MI355X ORB front end.
//
// HBM layout (per frame slot f of a context, all packed, byte offsets 256-aligned):
//   gray      [f][H][W]                 u8   level 0 (caller's device buffer or ctx staging)
//   pyr       [f][pyr_stride]           u8   levels 1..L-1, level l at pyr_off[l], row stride W_l
//   blur      [f][blur_stride]          u8   7x7 Gaussian of levels 0..L-1 (descriptor input), each
//                                            level in 16 x 8 tiles (blur_tile_off; rows padded to 8)
//   cand_n    [f][ncells]               i32  FAST corners kept per cell
//   cand      [f][ncells][cell_cap]     u32  packed (x_rel | y_rel<<12 | score<<24), row-major
//   keys      [f][2][kbuf_stride]       u32  octree key ping-pong buffers (per level kcap_off)
//   nodes     [f][L][2][NCAP] records        octree node scratch (start,cnt,rect,alloc)
//   lvl_n     [f][L]                    i32  keypoints per level after culls
//   lvl_kp    [f][lvl_stride]           u32  packed level keypoints in output order
//   kps       [f][kcap]                 28B  coeb_keypoint (== cv::KeyPoint)
//   desc      [f][kcap][32]             u8
//   dyn       [f]                       DynMask (area flag + zeroed rectangles)
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>
#include <mutex>
#include <set>
#include <utility>

#include "coeb_plan.hpp"     // LevelGeom, Plan, CellDesc: the geometry the kernels take as arguments

// Runtime switches, the only environment reads of the library (coeb_capi.hip):
// coeb_switch(name) returns the value of a product switch -- one of kSwitches, each run by the
// GPU test suite against the oracle (side-stream modes, the matcher's sequential / split forms,
// the pyramid's byte form, the general FAST slab layout, k_fm's threads per pair) -- or nullptr;
// a name that is no product switch is never read.
const char* coeb_switch(const char* name);

// Diagnostic phase clocks, compiled in only by the tools' own builds (-DCOEB_*_CLOCK=1): the
// product build has no hook.  A clock build fills its timing buffer on every launch.
#ifndef COEB_FAST_CLOCK
#define COEB_FAST_CLOCK 0      // per-cell k_fast phase clocks (fast_timing)
#endif
#ifndef COEB_OCT_CLOCK
#define COEB_OCT_CLOCK 0       // per-workgroup k_octree clocks (oct_timing)
#endif
#ifndef COEB_MATCH_CLOCK
#define COEB_MATCH_CLOCK 0     // k_match phase clocks (match_timing, tools/_match_timing.py)
#endif
#ifndef COEB_POSE_CLOCK
#define COEB_POSE_CLOCK 0      // k_pose phase clocks (pose_timing, tools/_pose_timing.py)
#endif

// Raise a kernel's dynamic-LDS limit once per (kernel, device), to the most any launch may use
// (the CU's 160 KB; the launch's own size still sets the occupancy).  The attribute is
// process-wide: setting it per launch to that launch's size let another host thread's launch of
// the same kernel with a larger size run under a smaller limit set in between.
constexpr int kLdsLimit = 160 * 1024;
inline void lds_limit_max(const void* kern)
{
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> g(mu);
    if (!done.insert({kern, dev}).second) return;
    // the device's per-workgroup maximum less the kernel's static LDS
    int lim = kLdsLimit, v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) == hipSuccess && v > 0)
        lim = v < lim ? v : lim;
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, kern) == hipSuccess) lim -= (int)fa.sharedSizeBytes;
    if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, lim) != hipSuccess)
        (void)hipGetLastError();        // not sticky: the launch itself reports a size it cannot take
}

// Byte (x, y) of a blurred level with row pitch bpitch (a 64-byte multiple): the level is stored
// in 128-byte tiles of 16 columns x 8 rows, one tile per cache line, tiles row-major (bpitch / 16
// per tile row).  k_describe reads 37-row x 64-byte patches: row-major, every patch row would be its
// own line (37-74 line lookups per patch, half of each 128-B line unused); tiled, a patch is
// 4 x 5-6 whole lines.
__host__ __device__ inline int64_t blur_tile_off(int x, int y, int bpitch)
{
    return ((int64_t)(y >> 3) * (bpitch >> 4) + (x >> 4)) * 128 + (y & 7) * 16 + (x & 15);
}

#define COEB_GRID_COLS 64
#define COEB_GRID_ROWS 48
#define COEB_GRID_CELLS (COEB_GRID_COLS * COEB_GRID_ROWS)

// Dynamic-object mask of one frame (ORBextractor.cc:1101-1195): the mask is the complement of
// the union of these rectangles (x in [x0,x1), y in [y0,y1)), so the W x H byte mask never
// needs to be materialised.
struct DynMask {
    int area_flag;
    int nrect;
    int rect[COEB_MAXBOX][4];
};

struct NodeSet {           // SoA node records (one set of a level)
    int* start;
    int* cnt;
    int4* rect;            // x0, y0, x1, y1 (relative coordinates)
    int* alloc;
    int* buf;
};

static inline __host__ __device__ uint32_t pack_key(int x, int y, int s)
{
    return (uint32_t)x | ((uint32_t)y << 12) | ((uint32_t)s << 24);
}
static inline __host__ __device__ int key_x(uint32_t k) { return (int)(k & 0xFFFu); }
static inline __host__ __device__ int key_y(uint32_t k) { return (int)((k >> 12) & 0xFFFu); }
static inline __host__ __device__ int key_s(uint32_t k) { return (int)(k >> 24); }

// Frame::UndistortKeyPoints (Frame.cc:579-609) for one point: cv::undistortPoints(.., mK,
// mDistCoef, Mat(), mK) of OpenCV 3.4 (cvUndistortPointsInternal, 5 fixed iterations) in double
// with the oracle's operation order.  k = (k1, k2, p1, p2, k3); the remaining rational /
// thin-prism terms of the 14-coefficient model are zero and kept so the sums match.  The one
// copy of this arithmetic: k_undistort (coeb_frame.hip) and k_frame_tail (coeb_capi.hip) call it.
struct DistK { double k[12]; double fx, fy, cx, cy; };
__device__ __forceinline__ void undistort_point(const DistK& d, float& px, float& py)
{
    const double* k = d.k;
    const double ifx = 1. / d.fx, ify = 1. / d.fy;
    double x = ((double)px - d.cx) * ifx, y = ((double)py - d.cy) * ify;
    const double x0 = x, y0 = y;
    for (int j = 0; j < 5; j++) {
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
        const double deltaX = ((((2 * k[2]) * x) * y + k[3] * (r2 + (2 * x) * x)) + k[8] * r2) + (k[9] * r2) * r2;
        const double deltaY = ((k[2] * (r2 + (2 * y) * y) + ((2 * k[3]) * x) * y) + k[10] * r2) + (k[11] * r2) * r2;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    px = (float)(d.fx * x + d.cx);
    py = (float)(d.fy * y + d.cy);
}

// ---- launch wrappers (coeb_extract.hip / coeb_match.hip) ----
int oct_timing_read(long long* out);   // COEB_OCT_CLOCK builds: [4096][6] per-workgroup k_octree clocks
int fast_timing_read(unsigned long long* out);   // COEB_FAST_CLOCK builds: per-cell k_fast phase sums
struct ExtractBufs {
    const uint8_t* gray;   // [F][H][W]
    uint8_t* pyr;
    uint8_t* blur;
    int* cand_n;
    uint32_t* cand;
    uint32_t* keys;
    uint8_t* nodes;        // raw node scratch
    int* lvl_n;
    uint32_t* lvl_kp;
    void* kps;             // coeb_keypoint
    uint8_t* desc;
    int* counts;
    DynMask* dyn;
    const int* rtab;
    const CellDesc* cells;
    const int8_t* pattern; // 512 x (x, y)
    // dynamic-mask inputs
    const float* boxes;    // [nbox_total][4]
    const int* box_off;    // [F+1]
    const float* tm;       // [ntm_total][2]
    const int* tm_off;     // [F+1]
    const int* blurf;      // [nbox_total]
    // T_M computed on the device (coeb_frame_batch_device): frame f's points at
    // tmd + f * tmd_cap * 2, count ntmd[f] (-1: none); used instead of tm / tm_off when set
    const float* tmd;
    const int* ntmd;
    int tmd_cap;
    int* err;              // device error word (capacity overflows)
};

struct ProfileHook {
    void* impl = nullptr;   // owned by the context (coeb_capi.hip)
};
void prof_begin(ProfileHook* p, const char* name, hipStream_t s);
void prof_end(ProfileHook* p, hipStream_t s);

// side (optional): blur + FAST of level 0 run on side.s while the pyramid builds levels 1..;
// those of level 1 follow there once the pyramid has built it, and s does FAST of levels 2..L-1
// after the pyramid, beside their blur on side.s; s joins side.s before the octree.
struct SideStream { hipStream_t s; hipEvent_t fork, mid, pyr_done, join; };
int launch_extract(const Plan& plan, const Plan* d_plan, const ExtractBufs& b, int F, hipStream_t s,
                   ProfileHook* prof, const SideStream* side = nullptr);

// Matcher limits shared by the kernels (coeb_match.hip) and the buffers the C-ABI sizes for them
constexpr int kCQ = 64;         // candidate-list entries per query (LastFrame point / local-map point)
constexpr int kMaxSplit = 8;    // split-list workgroups per pair (k_match_lists): qn rows hold that many flags
constexpr int kCurMax = 4095;   // current keypoints per frame (12-bit indices in the candidate lists)

struct MatchCam {
    float fx, fy, cx, cy, bf, mb;
    float min_x, max_x, min_y, max_y;
    float grid_inv_w, grid_inv_h;
    float scale[COEB_MAXL];
    int nlevels;       // mnScaleLevels
    float log_sf;      // mfLogScaleFactor = log(mfScaleFactor) (Frame.cc:85), correctly rounded
};
struct MatchBufs {
    // current frames
    const void* cur_kps;       // coeb_keypoint [P][cur_stride]
    const uint8_t* cur_desc;   // [P][cur_stride][32]
    const int* cur_n;          // [P]
    const float* cur_ur;       // [P][cur_stride] (may be computed by prep)
    int cur_stride;
    // last frames
    const void* last_kps;      // coeb_keypoint [P][last_stride]
    const uint8_t* last_desc;  // [P][last_stride][32] MapPoint descriptors
    const int* last_n;         // [P]
    const uint8_t* last_has;   // [P][last_stride]
    const uint8_t* last_out;   // [P][last_stride]
    const float* last_xw;      // [P][last_stride][3]
    const int* last_nobs;      // [P][last_stride]
    int last_stride;
    const float* Tcw_cur;      // [P][16]
    const float* Tcw_last;     // [P][16]
    int* match;                // [P][cur_stride]
    int* nmatch;               // [P]
    int* scratch;              // [P][scratch_stride]
    int scratch_stride;
    int* qn;                   // optional [P][qn_stride >= last_stride + kMaxSplit]: split-list counts + flags
    int qn_stride;
    long long* timing;         // [P][16] phase clocks (COEB_MATCH_CLOCK builds), else nullptr
    int* err;
};
int launch_match(const MatchCam& cam, const MatchBufs& b, int P, float th, int bmono, int check_ori,
                 int retry_below, hipStream_t s, ProfileHook* prof);

// local-map projection search (ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>, th))
// (k_match_local and k_match_kf take LocalBufs / KfBufs by value: the field order is their argument layout)
struct LocalBufs {
    const void* cur_kps; const uint8_t* cur_desc; const float* cur_ur; const int* cur_obs; int cur_n;
    const uint8_t* in_view; const float* proj_x; const float* proj_y; const float* proj_xr;
    const int* level; const float* view_cos; const uint8_t* desc; const int* nobs; int mp_n;
    int* match; int* nmatch; uint32_t* lists; int* err;
    int* path;   // [0]: 0 parallel claims, 1 forced sequential, 2 list overflow, 3 no convergence; [1]: iterations
    // batch form: npairs workgroups, pair p reads cur_* + p*cur_stride (keypoint count
    // cur_n_arr[p]), the local-map arrays + p*mp_stride, desc + p*mp_desc_stride*32,
    // lists + p*mp_stride*kCQ, and writes match + p*cur_stride, nmatch[p], path[2p..];
    // active[p] == 0 skips the pair (no matches).  cur_n_arr == null: the single search above.
    const int* cur_n_arr = nullptr; const uint8_t* active = nullptr;
    int cur_stride = 0, mp_stride = 0, mp_desc_stride = 0;
    int npairs = 1;   // read by the launcher only
};
int launch_match_local(const MatchCam& cam, const LocalBufs& b, float th, float nnratio, hipStream_t s,
                       ProfileHook* prof);

// Optimizer::PoseOptimization (coeb_pose.hip): per frame f, keypoints [f][stride]
struct PoseEdgeRec { float x, y, z, u, v, ur, w; int stereo, kp; };
struct PoseBufs {
    const int* n;                 // [F] keypoints
    const uint8_t* has_mp;        // [F][stride]
    const float* xw;              // [F][stride][3]
    const void* kps;              // [F][stride] coeb_keypoint
    const float* ur;              // [F][stride]
    const float* inv_sigma2;      // [COEB_MAXL] mvInvLevelSigma2
    float* Tcw;                   // [F][16] in/out
    uint8_t* outlier;             // [F][stride] out (mvbOutlier, where has_mp)
    int* result;                  // [F] nInitialCorrespondences - nBad
    PoseEdgeRec* edges;           // scratch [F][stride]
    uint8_t* active;              // scratch [F][stride]
    double* chi2;                 // scratch [F][stride]
    int stride;
    long long* timing;            // [F][8] phase clocks (COEB_POSE_CLOCK builds), else null
};
int launch_pose(const PoseBufs& b, int F, double fx, double fy, double cx, double cy, double bf, hipStream_t s,
                ProfileHook* prof);

// TrackWithMotionModel tail on a device batch (coeb_pose.hip): pair p = (frame p, frame p+1).
// All arrays are indexed from frame 0 ([F][stride]); frame 0 (the halo) is never written.
struct TrackPrepBufs {
    const int32_t* match;         // [F][stride] LastFrame index per current keypoint, or -1
    const int32_t* nmatch;        // [F] SearchByProjection result (after the 2*th retry)
    const int32_t* counts;        // [F] keypoints
    const float* last_xw;         // [F][stride][3] LastFrame MapPoint positions (k_prep)
    const void* kps_in;           // [F][stride] coeb_keypoint (batch output) -> kps_out
    const float* ur_in;           // [F][stride] mvuRight (k_prep) -> ur_out
    void* kps_out;
    float* ur_out;
    const float* Tin;             // [F][16] motion-model prediction
    float* Tout;                  // [F][16] <- Tin, then PoseOptimization's result
    uint8_t* has;                 // [F][stride] CurrentFrame.mvpMapPoints[i] != NULL
    float* xw;                    // [F][stride][3] position of that MapPoint
    int32_t* n;                   // [F] keypoints handed to the optimiser (0: not tracked)
    float* isg_out;               // [COEB_MAXL] device copy of isg
    float isg[COEB_MAXL];         // mvInvLevelSigma2
    int stride, min_matches;
};
int launch_track_prep(const TrackPrepBufs& t, int F, hipStream_t s, ProfileHook* prof);

// Tracking::TrackLocalMap on a device batch (coeb_track.hip), after the TrackWithMotionModel
// tail: current frame f = 1..F-1, KF1 = frame f-1 (the world frame of pair f), KF2 = frame f-2.
// Every [F][K] array is indexed from frame 0; the local map of frame f is [f][2K]: slots [0, K)
// = KF2's keypoint slots, [K, 2K) = KF1's.
struct TlmBufs {
    int K, nkf, nobs, min_matches, min_map;
    // batch outputs of the extraction / matcher (main stream), read by k_tlm_snapshot only
    const void* kps; const uint8_t* desc; const int* counts; const int* match1; const int* nmatch1;
    const uint8_t* has; const float* xw;
    // snapshot (main stream): s_desc holds frame g at row g + 1 (row 0: KF2 of frame 1, never read)
    uint8_t* s_desc; int8_t* s_oct; uint8_t* s_has; float* s_xw; int* s_m1; int* s_cnt; int* s_nm1;
    // TrackWithMotionModel's PoseOptimization (t_* of coeb_pose_batch_device)
    const float* T1; const uint8_t* has1; const uint8_t* outl1; const float* xw1;
    // discard + SearchLocalPoints state
    uint8_t* seen;       // [F][K] KF1 slot matched by the motion model (mnLastFrameSeen)
    int* cur_obs;        // [F][K] Observations() of the MapPoint a keypoint keeps, -1: none
    int* nmap;           // [F] nmatchesMap (Tracking.cc:967-985)
    uint8_t* active;     // [F] TrackWithMotionModel returned true -> TrackLocalMap runs
    uint8_t* in_view; float* px; float* py; float* pxr; int* level; float* vcos; int* lm_nobs; float* lm_xw;
    const int* lmatch;   // [F][K] SearchByProjection(F, vpLocalMapPoints) assignments
    // second PoseOptimization's inputs
    uint8_t* has2; float* xw2; float* T2; uint8_t* outl2; int* n2;
};
int launch_tlm_snapshot(const TlmBufs& t, int F, hipStream_t s, ProfileHook* prof);
int launch_tlm_frustum(const MatchCam& cam, const TlmBufs& t, int F, hipStream_t s, ProfileHook* prof);
int launch_tlm_pose_prep(const TlmBufs& t, int F, hipStream_t s, ProfileHook* prof);

// Tracking::TrackLocalMap on one host frame (coeb_track.hip), every array in device memory:
// k_frustum -> k_match_local -> k_lm_pose_prep -> k_pose -> k_lm_tail, no host step between.
struct LmBufs {
    // vpLocalMapPoints before isInFrustum, and CurrentFrame.mTcw as the call received it
    int mp_n; const uint8_t* valid; const float* xw; const float* normal; const float* maxd; const float* mind;
    const int* nobs; const float* Tcw; float cos_limit;
    // k_frustum: what isInFrustum leaves on the points (zeros where not in view) and nToMatch (zero on entry)
    uint8_t* in_view; float* px; float* py; float* pxr; int* level; float* vcos; int* n_to_match;
    // k_lm_pose_prep: mvpMapPoints at entry (cur_obs >= 0: held, position cur_xw) merged with the search's lmatch
    int cur_n; const int* cur_obs; const float* cur_xw; const int* lmatch;
    uint8_t* has2; float* xw2; int* obs2;
    // k_lm_tail: mnMatchesInliers from k_pose's outlier flags (zero on entry)
    const uint8_t* outl; int only_tracking; int* ninl;
};
int launch_frustum(const MatchCam& cam, const LmBufs& t, hipStream_t s, ProfileHook* prof);
int launch_lm_pose_prep(const LmBufs& t, hipStream_t s, ProfileHook* prof);
int launch_lm_tail(const LmBufs& t, hipStream_t s, ProfileHook* prof);
// launch_match_local's LDS-budget verdict for cur_n keypoints and mp_n points, before anything is enqueued
bool match_local_fits(int cur_n, int mp_n);

// Tracking::TrackReferenceKeyFrame on one host frame (coeb_track.hip), every array in device memory:
// k_bow_transform -> k_bow_csr -> k_match_bow -> k_bow_rot -> k_trk_pose_prep -> k_pose -> k_trk_tail,
// no host step between.
struct TrkBufs {
    // SearchByBoW's result as k_bow_rot left it (the KeyFrame index per keypoint, its count), the gate (:835)
    int cur_n; int* match; const int* nm_bow; int min_matches;
    // mpReferenceKF's MapPoints by KeyFrame index: GetWorldPos() and Observations()
    const float* kf_xw; const int* kf_nobs;
    // k_trk_pose_prep: mvpMapPoints for PoseOptimization (:841), its keypoint count (0: gated), mvbOutlier cleared
    uint8_t* has; float* xw; int* pose_n; uint8_t* outl;
    // k_trk_tail: the discard loop (:843-862); match loses the discarded, nmatches / nmap zero on entry
    int* discarded; int* nmatches; int* nmap;
};
int launch_trk_pose_prep(const TrkBufs& t, hipStream_t s, ProfileHook* prof);
int launch_trk_tail(const TrkBufs& t, hipStream_t s, ProfileHook* prof);

// Tracking::TrackWithMotionModel on one host frame (coeb_track.hip), every array in device memory:
// k_vo_points (localisation mode only) -> k_match_lists -> k_match (retry in-kernel) ->
// k_trk_pose_prep -> k_pose -> k_mm_tail, no host step between.  The gate and the gather are
// TrackReferenceKeyFrame's with the last frame's slots in the KeyFrame's place (TrkBufs.kf_xw /
// kf_nobs = the arrays below); the tail counts nmatches as the reference does here (k_mm_tail).
//
// k_vo_points: Tracking::UpdateLastFrame's "visual odometry" points (Tracking.cc:878-930) written
// into the last-frame arrays k_match reads.
constexpr int kVoMaxLast = 16384;   // last-frame keypoints k_vo_points ranks (their depths sit in LDS)
struct VoBufs {
    int n;                        // LastFrame.N
    const void* kps;              // [n] coeb_keypoint, LastFrame.mvKeysUn
    const float* depth;           // [n] LastFrame.mvDepth
    const uint8_t* desc_in;       // [n][32] LastFrame.mDescriptors
    const float* Tcw_last;        // [16] LastFrame.mTcw
    float th_depth, fx, fy, cx, cy;
    // the last frame as the caller snapshot it; a created point replaces slot i in place
    uint8_t* has; float* xw; uint8_t* desc; int* nobs;
    uint8_t* created;             // [n] 1 where a point was created, else 0
    float* created_pos;           // [n][3] written where created
};
int launch_vo_points(const VoBufs& v, hipStream_t s, ProfileHook* prof);
int launch_mm_tail(const TrkBufs& t, hipStream_t s, ProfileHook* prof);
// launch_match's LDS-budget verdict for one pair of cur_n x last_n keypoints, before anything is enqueued
bool match_lastframe_fits(int cur_n, int last_n);

// relocalisation projection search (ORBmatcher::SearchByProjection(Frame&, KeyFrame*, set, th, ORBdist))
struct KfBufs {
    const void* cur_kps; const uint8_t* cur_desc; const uint8_t* cur_has; int cur_n;
    const uint8_t* valid; const float* xw; const uint8_t* desc; const float* maxd; const float* mind;
    const float* angle; int kf_n;
    const float* Tcw;   // device, 16 floats row-major
    int* match; int* nmatch; uint32_t* lists; int* err;
    int* path;          // as LocalBufs::path
    // batch form (coeb_reloc_refine): npairs workgroups over ONE current frame (cur_kps, cur_desc, cur_n
    // shared).  Pair p reads cur_has + p*cur_stride, the KeyFrame arrays + p*kf_stride (xw * 3, desc * 32;
    // kf_n_arr[p] points; kf_n = the largest, read by the launcher only), Tcw + 16p, lists +
    // p*kf_stride*kCQ, and writes match + p*cur_stride, nmatch[p], path[2p..]; active[p] == 0 skips the
    // pair (nmatch[p] = 0, no assignment).  kf_n_arr == null: the single search above.
    const int* kf_n_arr = nullptr; const uint8_t* active = nullptr;
    int cur_stride = 0, kf_stride = 0;
    int npairs = 1;     // read by the launcher only
};
int launch_match_kf(const MatchCam& cam, const KfBufs& b, float th, int orb_dist, int check_ori, hipStream_t s,
                    ProfileHook* prof);
// launch_match_kf's LDS-budget verdict for cur_n keypoints and kf_n KeyFrame points, before anything is enqueued
bool match_kf_fits(int cur_n, int kf_n);

// Tracking::Relocalization's refinement of nhyp PnP hypotheses (src/Tracking.cc:1502-1565) on one host
// frame (coeb_track.hip), every array in device memory, workgroup h of every launch = hypothesis h:
// k_rr_enter -> k_pose -> k_rr_after1 -> k_match_kf -> k_rr_merge -> k_pose -> k_rr_after2 -> k_match_kf
// -> k_rr_merge -> k_pose -> k_rr_tail, no host step between.  [H][cs] arrays have row stride cs (the
// current frame), [H][ks] arrays row stride ks (the KeyFrames); a gated optimisation has pose_n = 0,
// a gated search active = 0.
struct RrBufs {
    int nhyp, cur_n, cs, ks;
    int min_good, low_good, enough_good;
    // inputs: the shared current frame, per hypothesis vvpMapPointMatches / vbInliers and the KeyFrame
    const void* kps; const float* ur;                                   // [cur_n]
    const int* match_in; const uint8_t* inlier;                         // [H][cs]
    const int* kf_n; const uint8_t* kf_valid; const float* kf_xw;       // [H], [H][ks], [H][ks][3]
    // mCurrentFrame per hypothesis: mvpMapPoints as KeyFrame indices (-1: NULL), what k_pose and the
    // search read of it, mvbOutlier, and k_pose's own copies of the keypoints
    int* held; uint8_t* has; float* xw; uint8_t* outl;                  // [H][cs]
    uint8_t* at_opt;                                                    // [H][cs] held a point at the last optimisation run
    void* kps_h; float* ur_h;                                           // [H][cs]
    // sAlreadyFound over KeyFrame indices, the `valid` of the next search, the search's result
    uint8_t* found; uint8_t* valid_s;                                   // [H][ks]
    const int* smatch; const int* snm;                                  // [H][cs], [H]
    uint8_t* active;                                                    // [2][H] search 1, search 2
    int* pose_n; const int* pose_res;                                   // [3][H] each
    // results: {stage, ngood, nadditional1, nadditional2} per hypothesis, first_good (nhyp: none; zero /
    // nhyp on entry), the packed mvbOutlier (2: not written)
    int* cnt; int* first_good; uint8_t* outl_out;                       // [H][4], [1], [H][cs]
};
int launch_rr_enter(const RrBufs& r, hipStream_t s, ProfileHook* prof);
int launch_rr_after1(const RrBufs& r, hipStream_t s, ProfileHook* prof);
int launch_rr_merge(const RrBufs& r, int which, hipStream_t s, ProfileHook* prof);   // which = 1, 2: the search merged
int launch_rr_after2(const RrBufs& r, hipStream_t s, ProfileHook* prof);
int launch_rr_tail(const RrBufs& r, hipStream_t s, ProfileHook* prof);

// frame preparation for batch matching: u_right/depth per keypoint + LastFrame map snapshot
struct PrepBufs {
    const void* kps; const int* n; int stride;
    const float* depth; int W, H;
    float bf, fx, fy, cx, cy;
    float* ur; float* dep;
    uint8_t* has; uint8_t* outl; float* xw; int* nobs; int nobs_value;
    const float* Twc;          // [F][16] inverse poses for UnprojectStereo (may be NULL = I)
};
int launch_prep(const PrepBufs& b, int F, hipStream_t s, ProfileHook* prof);
