// coeb_track.hip -- Tracking::TrackLocalMap on a device batch (BASELINE configs[4]):
//   TrackWithMotionModel's outlier discard          src/Tracking.cc:966-993   (k_tlm_discard)
//   SearchLocalPoints: skip matched points,         src/Tracking.cc:1222-1272 (k_tlm_frustum)
//     Frame::isInFrustum(pMP, 0.5)                  src/Frame.cc:445-501
//     MapPoint::PredictScale                        src/MapPoint.cc:402-417
//   ORBmatcher::SearchByProjection(F, vpLocalMapPoints, th)     k_match_local (coeb_match.hip)
//   second Optimizer::PoseOptimization (:1006)      k_tlm_pose_prep + k_pose (coeb_pose.hip)
//
// The local map of frame f is the MapPoints of two KeyFrames, KF2 = frame f-2 and KF1 = frame
// f-1, each keypoint with depth > 0 one MapPoint with a single observation
// (MapPoint::UpdateNormalAndDepth, MapPoint.cc:330-371).  KF1 is the world frame of the pair
// (as in the motion-model step); KF2's points are placed by KF1's motion-model pose.  The
// definition and its canonical float forms are DESIGN.md s4.3; oracle/orb_oracle.c
// (oc_local_map_build) restates them for the parity tests.
//
// The same step on one host frame over an arbitrary local map (coeb_search_local_points /
// coeb_track_local_map): k_frustum -> k_match_local -> k_lm_pose_prep -> k_pose -> k_lm_tail on
// the context stream, the map as the caller snapshots it (normals and distance ranges given).
//
// Tracking::TrackReferenceKeyFrame on one host frame (coeb_track_reference_keyframe,
// src/Tracking.cc:823-865): behind SearchByBoW (coeb_bow.hip) k_trk_pose_prep -> k_pose -> k_trk_tail.
//
// Tracking::TrackWithMotionModel on one host frame (coeb_track_motion_model, src/Tracking.cc:933-994
// with UpdateLastFrame's visual-odometry points, :878-930): k_vo_points in front of the last-frame
// search (coeb_match.hip), then k_trk_pose_prep -> k_pose -> k_mm_tail.
//
// Tracking::Relocalization behind PnPsolver::iterate for a round of hypotheses on one host frame
// (coeb_reloc_refine, src/Tracking.cc:1502-1565), workgroup h of every launch = hypothesis h: k_rr_enter ->
// k_pose -> k_rr_after1 -> k_match_kf (batch form, coeb_match.hip) -> k_rr_merge -> k_pose -> k_rr_after2 ->
// k_match_kf -> k_rr_merge -> k_pose -> k_rr_tail.
//
// Batch launch order: k_tlm_snapshot on the context stream (it copies every batch array the rest
// reads, so the next batch's extraction may overwrite them), then on the pose stream after
// the first k_pose: k_tlm_discard -> k_tlm_frustum -> k_match_local -> k_tlm_pose_prep -> k_pose.
#include <hip/hip_runtime.h>

#include "coeb_internal.hpp"
#include "coeb_track_dev.hpp"

namespace {

constexpr int kT = 256;

struct KpT { float x, y, size, angle, response; int octave, class_id; };   // coeb_keypoint

// ---- k_tlm_snapshot: frame f's slots into the s_* arrays; seen / nmap cleared ----
__global__ __launch_bounds__(kT) void k_tlm_snapshot(TlmBufs t)
{
    const int f = blockIdx.y;
    const int i = blockIdx.x * kT + threadIdx.x;
    const int n = t.counts[f];
    const int64_t K = t.K;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        t.s_cnt[f] = n;
        t.s_nm1[f] = f ? t.nmatch1[f] : 0;
        t.nmap[f] = 0;
    }
    if (i < t.K) t.seen[f * K + i] = 0;
    if (i >= n) return;
    const int64_t o = f * K + i;
    const uint4* src = reinterpret_cast<const uint4*>(t.desc + o * 32);
    uint4* dst = reinterpret_cast<uint4*>(t.s_desc + (o + K) * 32);
    dst[0] = src[0];
    dst[1] = src[1];
    t.s_oct[o] = (int8_t)reinterpret_cast<const KpT*>(t.kps)[o].octave;
    t.s_has[o] = t.has[o];
    t.s_xw[3 * o + 0] = t.xw[3 * o + 0];
    t.s_xw[3 * o + 1] = t.xw[3 * o + 1];
    t.s_xw[3 * o + 2] = t.xw[3 * o + 2];
    t.s_m1[o] = f ? t.match1[o] : -1;
}

// ---- k_tlm_discard: Tracking.cc:966-985 ----
// A matched keypoint flagged outlier by the first PoseOptimization loses its MapPoint; the
// MapPoints the matcher assigned (inliers and outliers) get mnLastFrameSeen = current, so
// SearchLocalPoints skips them (:979, :1237, :1249).  nmatchesMap counts the kept ones with
// Observations() > 0.
__global__ __launch_bounds__(kT) void k_tlm_discard(TlmBufs t)
{
    const int f = blockIdx.y + 1;
    const int i = blockIdx.x * kT + threadIdx.x;
    const int64_t K = t.K;
    const bool go = t.s_nm1[f] >= t.min_matches;                  // PoseOptimization ran (:954-964)
    const int n = t.s_cnt[f];
    bool kept = false;
    if (i < n) {
        const int64_t o = f * K + i;
        const int m = t.s_m1[o];
        if (go && m >= 0) t.seen[f * K + m] = 1;
        const bool inl = go && t.has1[o] && !t.outl1[o];
        t.cur_obs[o] = inl ? t.nobs : -1;
        kept = inl && t.nobs > 0;
    }
    const uint64_t b = __ballot(kept);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(&t.nmap[f], (int)__popcll(b));
}

// ---- k_tlm_frustum: the local map of frame f through Frame::isInFrustum(pMP, 0.5) ----
__global__ __launch_bounds__(kT) void k_tlm_frustum(MatchCam cam, TlmBufs t)
{
    const int f = blockIdx.y + 1;
    const int q = blockIdx.x * kT + threadIdx.x;
    const int64_t K = t.K, M = 2 * K;
    if (q >= M) return;
    // TrackWithMotionModel's verdict (:954-961, :993): TrackLocalMap runs only when it held
    const bool ok = t.s_nm1[f] >= t.min_matches && t.nmap[f] >= t.min_map;
    if (q == 0) t.active[f] = ok ? 1 : 0;
    const int64_t o = f * M + q;
    int in = 0, lvl = 0;
    if (ok) {
        const bool kf1 = q >= K;
        const int j = kf1 ? (int)(q - K) : q;
        const int g = kf1 ? f - 1 : f - 2;
        bool exists = g >= 0 && (kf1 || t.nkf >= 2);
        if (exists) exists = j < t.s_cnt[g] && t.s_has[g * K + j] && !(kf1 && t.seen[f * K + j]);
        if (exists) {
            const float* X = t.s_xw + 3 * (g * K + j);
            float P[3], Ow[3];
            if (kf1) {
                P[0] = X[0]; P[1] = X[1]; P[2] = X[2];
                Ow[0] = Ow[1] = Ow[2] = 0.0f;
            } else {                                               // UnprojectStereo with KF2's Twc
                const float* T = t.T1 + (int64_t)(f - 1) * 16;
                const float Xl[3] = {X[0], X[1], X[2]};
                gemm_add(T, Xl, P);
                Ow[0] = T[3]; Ow[1] = T[7]; Ow[2] = T[11];
            }
            // UpdateNormalAndDepth, one observation (MapPoint.cc:348-370)
            const float d[3] = {P[0] - Ow[0], P[1] - Ow[1], P[2] - Ow[2]};
            const double nd = norm3(d);
            float Pn[3];
            for (int k = 0; k < 3; k++) Pn[k] = (float)((double)d[k] / nd);
            const int oct = t.s_oct[g * K + j];
            const float maxd = (float)nd * cam.scale[oct];
            const float mind = maxd / cam.scale[cam.nlevels - 1];
            // isInFrustum (Frame.cc:445-501) with PredictScale
            const FrustumView fv = is_in_frustum(cam, t.T1 + (int64_t)f * 16, P, Pn, maxd, mind, 0.5f);
            if (fv.in_view) {
                lvl = fv.level;
                in = 1;
                t.px[o] = fv.u;
                t.py[o] = fv.v;
                t.pxr[o] = fv.ur;
                t.vcos[o] = fv.view_cos;
                t.lm_xw[3 * o + 0] = P[0];
                t.lm_xw[3 * o + 1] = P[1];
                t.lm_xw[3 * o + 2] = P[2];
            }
        }
    }
    t.in_view[o] = (uint8_t)in;
    t.level[o] = lvl;
    t.lm_nobs[o] = t.nobs;
}

// ---- k_tlm_pose_prep: CurrentFrame.mvpMapPoints for the second PoseOptimization ----
// A keypoint holds the local-map point SearchByProjection gave it, else the motion-model
// MapPoint it kept through the discard; the pose starts at the first optimisation's result.
__global__ __launch_bounds__(kT) void k_tlm_pose_prep(TlmBufs t)
{
    const int f = blockIdx.y + 1;
    const int i = blockIdx.x * kT + threadIdx.x;
    const int64_t K = t.K;
    const bool ok = t.active[f] != 0;
    const int n = t.s_cnt[f];
    if (blockIdx.x == 0) {
        if (threadIdx.x < 16) t.T2[(int64_t)f * 16 + threadIdx.x] = t.T1[(int64_t)f * 16 + threadIdx.x];
        if (threadIdx.x == 16) t.n2[f] = ok ? n : 0;
    }
    if (i >= n) return;
    const int64_t o = f * K + i;
    if (!ok) {          // TrackLocalMap does not run: no second optimisation, nothing is an outlier
        t.has2[o] = 0;
        t.outl2[o] = 0;
        return;
    }
    const int lm = t.lmatch[o];
    t.outl2[o] = 0;
    if (lm >= 0) {
        const int64_t p = f * 2 * K + lm;
        t.has2[o] = 1;
        t.xw2[3 * o + 0] = t.lm_xw[3 * p + 0];
        t.xw2[3 * o + 1] = t.lm_xw[3 * p + 1];
        t.xw2[3 * o + 2] = t.lm_xw[3 * p + 2];
    } else if (t.cur_obs[o] >= 0) {
        t.has2[o] = 1;
        t.xw2[3 * o + 0] = t.xw1[3 * o + 0];
        t.xw2[3 * o + 1] = t.xw1[3 * o + 1];
        t.xw2[3 * o + 2] = t.xw1[3 * o + 2];
    } else {
        t.has2[o] = 0;
    }
}

// ---- k_frustum: an arbitrary local map through Frame::isInFrustum(pMP, cos_limit) ----
// One thread per point of vpLocalMapPoints (Tracking.cc:1246-1259); the points in view are
// counted as k_tlm_discard counts: a ballot and one atomic per wave.
__global__ __launch_bounds__(kT) void k_frustum(MatchCam cam, LmBufs t)
{
    const int q = blockIdx.x * kT + threadIdx.x;
    FrustumView fv{false, 0.f, 0.f, 0.f, 0.f, 0};
    if (q < t.mp_n) {
        if (t.valid[q]) {
            const float P[3] = {t.xw[3 * q + 0], t.xw[3 * q + 1], t.xw[3 * q + 2]};
            const float Pn[3] = {t.normal[3 * q + 0], t.normal[3 * q + 1], t.normal[3 * q + 2]};
            fv = is_in_frustum(cam, t.Tcw, P, Pn, t.maxd[q], t.mind[q], t.cos_limit);
        }
        t.in_view[q] = fv.in_view ? 1 : 0;
        t.px[q] = fv.u;
        t.py[q] = fv.v;
        t.pxr[q] = fv.ur;
        t.level[q] = fv.level;
        t.vcos[q] = fv.view_cos;
    }
    const uint64_t b = __ballot(fv.in_view);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(t.n_to_match, (int)__popcll(b));
}

// ---- k_lm_pose_prep: CurrentFrame.mvpMapPoints for TrackLocalMap's PoseOptimization (:1006) ----
// A keypoint holds the local-map point the search gave it, else the MapPoint it entered with.
__global__ __launch_bounds__(kT) void k_lm_pose_prep(LmBufs t)
{
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= t.cur_n) return;
    const int lm = t.lmatch[i];
    const float* X = nullptr;
    int obs = -1;
    if (lm >= 0) {
        X = t.xw + 3 * (int64_t)lm;
        obs = t.nobs[lm];
    } else if (t.cur_obs[i] >= 0) {
        X = t.cur_xw + 3 * (int64_t)i;
        obs = t.cur_obs[i];
    }
    t.has2[i] = X ? 1 : 0;
    t.obs2[i] = obs;
    t.xw2[3 * i + 0] = X ? X[0] : 0.f;
    t.xw2[3 * i + 1] = X ? X[1] : 0.f;
    t.xw2[3 * i + 2] = X ? X[2] : 0.f;
}

// ---- k_lm_tail: mnMatchesInliers (Tracking.cc:1010-1027) ----
__global__ __launch_bounds__(kT) void k_lm_tail(LmBufs t)
{
    const int i = blockIdx.x * kT + threadIdx.x;
    bool inl = false;
    if (i < t.cur_n) inl = t.has2[i] && !t.outl[i] && (t.only_tracking || t.obs2[i] > 0);
    const uint64_t b = __ballot(inl);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(t.ninl, (int)__popcll(b));
}

// ---- k_trk_pose_prep: TrackReferenceKeyFrame between SearchByBoW and PoseOptimization (:835-841) ----
// mCurrentFrame.mvpMapPoints = vpMapPointMatches: keypoint i holds the MapPoint of KeyFrame feature
// match[i].  `if (nmatches < 15) return false` (:835) is decided here: such a frame reaches the
// optimiser with no keypoints, so k_pose leaves the pose and reports 0 (as k_track_prep does).
__global__ __launch_bounds__(kT) void k_trk_pose_prep(TrkBufs t)
{
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i == 0) *t.pose_n = *t.nm_bow >= t.min_matches ? t.cur_n : 0;
    if (i >= t.cur_n) return;
    const int m = t.match[i];
    const float* X = m >= 0 ? t.kf_xw + 3 * (int64_t)m : nullptr;
    t.has[i] = X ? 1 : 0;
    t.outl[i] = 0;                                  // k_pose writes the flags of the edges it takes
    t.xw[3 * i + 0] = X ? X[0] : 0.f;
    t.xw[3 * i + 1] = X ? X[1] : 0.f;
    t.xw[3 * i + 2] = X ? X[2] : 0.f;
}

// ---- k_trk_tail: "Discard outliers" (:843-862) ----
// A matched keypoint k_pose flagged loses its point (discarded[i] = the KeyFrame index it had);
// nmatches counts the keypoints that keep one, nmatches_map those whose point has
// Observations() > 0 (both zero on entry).  A gated frame keeps every match and counts no map point.
__global__ __launch_bounds__(kT) void k_trk_tail(TrkBufs t)
{
    __shared__ int s_cnt[2];
    const int i = blockIdx.x * kT + threadIdx.x;
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const bool go = *t.nm_bow >= t.min_matches;
    bool kept = false, map = false;
    if (i < t.cur_n) {
        const int m = t.match[i];
        const bool out = go && m >= 0 && t.outl[i];
        t.discarded[i] = out ? m : -1;
        if (out) t.match[i] = -1;
        kept = m >= 0 && !out;
        map = go && kept && t.kf_nobs[m] > 0;
    }
    const uint64_t bk = __ballot(kept), bm = __ballot(map);
    if ((threadIdx.x & 63) == 0) {
        if (bk) atomicAdd(&s_cnt[0], (int)__popcll(bk));
        if (bm) atomicAdd(&s_cnt[1], (int)__popcll(bm));
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt[0]) atomicAdd(t.nmatches, s_cnt[0]);
    if (threadIdx.x == 1 && s_cnt[1]) atomicAdd(t.nmap, s_cnt[1]);
}

// ---- k_mm_tail: TrackWithMotionModel's "Discard outliers" (:966-985) ----
// As k_trk_tail over the last frame's slots, but for nmatches: SearchByProjection's return counts
// assignments, and a keypoint two last-frame points were assigned to counts twice while holding one
// point (ORBmatcher.cc:1425-1426), so nmatches is that return less the discards (`nmatches--`),
// not the number of keypoints that keep a point.  nmatches / nmap zero on entry.
__global__ __launch_bounds__(kT) void k_mm_tail(TrkBufs t)
{
    __shared__ int s_cnt[2];
    const int i = blockIdx.x * kT + threadIdx.x;
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int nm = *t.nm_bow;
    const bool go = nm >= t.min_matches;
    bool out = false, map = false;
    if (i < t.cur_n) {
        const int m = t.match[i];
        out = go && m >= 0 && t.outl[i];
        t.discarded[i] = out ? m : -1;
        if (out) t.match[i] = -1;
        map = go && m >= 0 && !out && t.kf_nobs[m] > 0;
    }
    const uint64_t bo = __ballot(out), bm = __ballot(map);
    if ((threadIdx.x & 63) == 0) {
        if (bo) atomicAdd(&s_cnt[0], (int)__popcll(bo));
        if (bm) atomicAdd(&s_cnt[1], (int)__popcll(bm));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int d = (blockIdx.x == 0 ? nm : 0) - s_cnt[0];
        if (d) atomicAdd(t.nmatches, d);
    }
    if (threadIdx.x == 1 && s_cnt[1]) atomicAdd(t.nmap, s_cnt[1]);
}

// ---- k_vo_points: UpdateLastFrame's "visual odometry" points (Tracking.cc:878-930) ----
// The reference sorts (depth, index) over the keypoints with depth > 0 and walks the order,
// counting every entry, until one is farther than th_depth with more than 100 counted.  With M
// entries, c of them not farther than th_depth, entry j (from 0) is reached iff no earlier entry
// stopped the walk, and entry j' stops it iff j' >= 100 and j' >= c: the visited entries are
// j <= max(c, 100).  Every workgroup stages all depths in LDS (-1 where not > 0: NaN, 0,
// negative); thread i counts the entries that precede its own, (z_j, j) < (z_i, i), and c.  A
// visited keypoint whose slot holds no point or one nobody observes gets Frame::UnprojectStereo(i)
// (Frame.cc:844-858) with mRwc / mOw from Tcw_last as UpdatePoseMatrices forms them, its own
// descriptor and Observations() = 0.
__global__ __launch_bounds__(kT) void k_vo_points(VoBufs v)
{
    extern __shared__ __attribute__((aligned(16))) float s_z[];    // n rounded up to 4 entries, the pad -1
    const int n = v.n, n4 = (n + 3) & ~3;
    for (int j = threadIdx.x; j < n4; j += kT) {
        const float z = j < n ? v.depth[j] : -1.0f;
        s_z[j] = z > 0 ? z : -1.0f;
    }
    __syncthreads();
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= n) return;
    const float zi = s_z[i];
    int before = 0, close = 0;
#pragma unroll 4
    for (int j = 0; j < n4; j += 4) {                      // four depths per LDS read
        const float4 q = *reinterpret_cast<const float4*>(s_z + j);
        const float zq[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float zj = zq[k];
            const bool in = zj > 0;
            before += in && (zj < zi || (zj == zi && j + k < i));
            close += in && !(zj > v.th_depth);             // the walk stops on `z > mThDepth` only
        }
    }
    const bool visited = zi > 0 && before <= max(close, 100);
    const bool create = visited && (!v.has[i] || v.nobs[i] < 1);
    v.created[i] = create ? 1 : 0;
    if (!create) return;
    const KpT kp = reinterpret_cast<const KpT*>(v.kps)[i];
    const float invfx = 1.0f / v.fx, invfy = 1.0f / v.fy;
    const float Xc[3] = {(kp.x - v.cx) * zi * invfx, (kp.y - v.cy) * zi * invfy, zi};
    const float* T = v.Tcw_last;
    float Twc[12], P[3];
    for (int k = 0; k < 3; k++) {                          // mRwc = mRcw.t(), mOw = -mRcw.t()*mtcw (GEMM_1_T)
        double s = (double)T[0 * 4 + k] * T[3] + (double)T[1 * 4 + k] * T[7];
        s = s + (double)T[2 * 4 + k] * T[11];
        Twc[k * 4 + 0] = T[0 * 4 + k];
        Twc[k * 4 + 1] = T[1 * 4 + k];
        Twc[k * 4 + 2] = T[2 * 4 + k];
        Twc[k * 4 + 3] = (float)(s * -1.0);
    }
    gemm_add(Twc, Xc, P);                                  // mRwc*x3Dc + mOw
    for (int k = 0; k < 3; k++) {
        v.xw[3 * i + k] = P[k];
        v.created_pos[3 * i + k] = P[k];
    }
    v.has[i] = 1;
    v.nobs[i] = 0;
    const uint4* src = reinterpret_cast<const uint4*>(v.desc_in + (int64_t)i * 32);
    uint4* dst = reinterpret_cast<uint4*>(v.desc + (int64_t)i * 32);
    dst[0] = src[0];
    dst[1] = src[1];
}

// ---- Tracking::Relocalization after PnPsolver::iterate (Tracking.cc:1502-1565), workgroup h = hypothesis h ----
// mvpMapPoints is `held`, the KeyFrame index a keypoint's MapPoint has in vpCandidateKFs[h] (-1: NULL);
// sFound is a byte per KeyFrame index (a MapPoint occupies at most one index of a KeyFrame).  cnt[4h..]
// = {stage, ngood, nadditional1, nadditional2}; every kernel that decides a branch writes the stage the
// hypothesis ends in if nothing further runs.
constexpr int kRrStage = 0, kRrGood = 1, kRrAdd = 2;

__device__ __forceinline__ void rr_take(const RrBufs& r, int h, int64_t o, int m)
{
    const float* X = r.kf_xw + 3 * ((int64_t)h * r.ks + m);
    r.held[o] = m;
    r.has[o] = 1;
    r.xw[3 * o + 0] = X[0];
    r.xw[3 * o + 1] = X[1];
    r.xw[3 * o + 2] = X[2];
}

// sFound = the KeyFrame indices of `held`, valid_s = kf_valid && !sFound
__device__ __forceinline__ void rr_search_valid(const RrBufs& r, int h, bool rebuild)
{
    const int kn = r.kf_n[h];
    uint8_t* found = r.found + (int64_t)h * r.ks;
    if (rebuild) {                                              // sFound.clear(); insert every non-NULL mvpMapPoints (:1541-1544)
        for (int q = threadIdx.x; q < kn; q += kT) found[q] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < r.cur_n; i += kT) {
            const int m = r.held[(int64_t)h * r.cs + i];
            if (m >= 0) found[m] = 1;
        }
        __syncthreads();
    }
    for (int q = threadIdx.x; q < kn; q += kT)
        r.valid_s[(int64_t)h * r.ks + q] = r.kf_valid[(int64_t)h * r.ks + q] && !found[q];
}

// :1502-1517: mvpMapPoints[j] = vbInliers[j] ? vvpMapPointMatches[h][j] : NULL, sFound = the inliers' points
__global__ __launch_bounds__(kT) void k_rr_enter(RrBufs r)
{
    const int h = blockIdx.x, n = r.cur_n, kn = r.kf_n[h];
    uint8_t* found = r.found + (int64_t)h * r.ks;
    for (int q = threadIdx.x; q < kn; q += kT) found[q] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += kT) {
        const int64_t o = (int64_t)h * r.cs + i;
        const int m = r.inlier[o] ? r.match_in[o] : -1;
        if (m >= 0) {
            rr_take(r, h, o, m);
            found[m] = 1;
        } else {
            r.held[o] = -1;
            r.has[o] = 0;
        }
        r.at_opt[o] = m >= 0 ? 1 : 0;
        r.outl[o] = 0;                                          // k_pose writes the flags of the edges it takes
        reinterpret_cast<KpT*>(r.kps_h)[o] = reinterpret_cast<const KpT*>(r.kps)[i];   // k_pose indexes [h][cs]
        r.ur_h[o] = r.ur[i];
    }
    if (threadIdx.x == 0) r.pose_n[h] = n;
}

// :1521-1529 behind the first PoseOptimization: `nGood < 10 -> continue`, the discard, `nGood < 50` -> search
__global__ __launch_bounds__(kT) void k_rr_after1(RrBufs r)
{
    const int h = blockIdx.x, n = r.cur_n;
    const int ng = r.pose_res[h];
    const bool stop = ng < r.min_good, search = !stop && ng < r.enough_good;
    if (threadIdx.x == 0) {
        r.cnt[4 * h + kRrStage] = stop ? 0 : search ? 2 : 1;
        r.active[h] = search ? 1 : 0;
    }
    if (stop) return;
    for (int i = threadIdx.x; i < n; i += kT) {                 // outliers lose their point and stay in sFound
        const int64_t o = (int64_t)h * r.cs + i;
        if (r.has[o] && r.outl[o]) { r.held[o] = -1; r.has[o] = 0; }
    }
    if (search) rr_search_valid(r, h, false);
}

// Behind search `which`: its assignments enter mvpMapPoints (whatever the gate says), then
// `nadditional + nGood >= 50` (:1533, :1548) lets the next PoseOptimization run
__global__ __launch_bounds__(kT) void k_rr_merge(RrBufs r, int which)
{
    const int h = blockIdx.x, n = r.cur_n;
    int* pose_n = r.pose_n + which * r.nhyp;
    if (!r.active[(which - 1) * r.nhyp + h]) {
        if (threadIdx.x == 0) pose_n[h] = 0;
        return;
    }
    const int nadd = r.snm[h];
    const bool go = nadd + r.pose_res[(which - 1) * r.nhyp + h] >= r.enough_good;
    for (int i = threadIdx.x; i < n; i += kT) {
        const int64_t o = (int64_t)h * r.cs + i;
        const int m = r.smatch[o];
        if (m >= 0) rr_take(r, h, o, m);
        if (go) r.at_opt[o] = m >= 0 || r.has[o];
    }
    if (threadIdx.x == 0) {
        pose_n[h] = go ? n : 0;
        r.cnt[4 * h + kRrAdd + which - 1] = nadd;
        r.cnt[4 * h + kRrStage] = which == 1 ? (go ? 3 : 2) : (go ? 5 : 4);
    }
}

// :1539-1545 behind the second PoseOptimization (no discard in front of it): `nGood > 30 && nGood < 50` -> search
__global__ __launch_bounds__(kT) void k_rr_after2(RrBufs r)
{
    const int h = blockIdx.x;
    const bool ran = r.pose_n[r.nhyp + h] > 0;
    const int ng = r.pose_res[r.nhyp + h];
    const bool search = ran && ng > r.low_good && ng < r.enough_good;
    if (threadIdx.x == 0) r.active[r.nhyp + h] = search ? 1 : 0;
    if (search) rr_search_valid(r, h, true);
}

// The final discard (:1552-1554, stage 5 only), nGood of the last optimisation run, the packed
// mvbOutlier and `nGood >= 50 -> break` (:1561) as the lowest such h
__global__ __launch_bounds__(kT) void k_rr_tail(RrBufs r)
{
    const int h = blockIdx.x, n = r.cur_n;
    const int stage = r.cnt[4 * h + kRrStage];
    const int ng = r.pose_res[(stage >= 5 ? 2 : stage >= 3 ? 1 : 0) * r.nhyp + h];
    for (int i = threadIdx.x; i < n; i += kT) {
        const int64_t o = (int64_t)h * r.cs + i;
        const uint8_t fl = r.outl[o];
        if (stage == 5 && r.has[o] && fl) { r.held[o] = -1; r.has[o] = 0; }
        r.outl_out[o] = r.at_opt[o] ? fl : 2;
    }
    if (threadIdx.x == 0) {
        r.cnt[4 * h + kRrGood] = ng;
        if (ng >= r.enough_good) atomicMin(r.first_good, h);
    }
}

}  // namespace

#define COEB_RR_LAUNCH(name, ...)                                                       \
    do {                                                                                \
        prof_begin(prof, #name, s);                                                     \
        hipLaunchKernelGGL(name, dim3(r.nhyp), dim3(kT), 0, s, __VA_ARGS__);            \
        prof_end(prof, s);                                                              \
        return hipGetLastError() == hipSuccess ? 0 : -1;                                \
    } while (0)
int launch_rr_enter(const RrBufs& r, hipStream_t s, ProfileHook* prof) { COEB_RR_LAUNCH(k_rr_enter, r); }
int launch_rr_after1(const RrBufs& r, hipStream_t s, ProfileHook* prof) { COEB_RR_LAUNCH(k_rr_after1, r); }
int launch_rr_merge(const RrBufs& r, int which, hipStream_t s, ProfileHook* prof) { COEB_RR_LAUNCH(k_rr_merge, r, which); }
int launch_rr_after2(const RrBufs& r, hipStream_t s, ProfileHook* prof) { COEB_RR_LAUNCH(k_rr_after2, r); }
int launch_rr_tail(const RrBufs& r, hipStream_t s, ProfileHook* prof) { COEB_RR_LAUNCH(k_rr_tail, r); }
#undef COEB_RR_LAUNCH

// One kT-thread workgroup per kT of `count` elements; nothing to do (0) when there are none.  `name` is
// the kernel's key in coeb_profile_read.
template <class K, class... A>
int launch_1d(const char* name, K kernel, int count, size_t lds, hipStream_t s, ProfileHook* prof, const A&... args)
{
    if (count <= 0) return 0;
    prof_begin(prof, name, s);
    hipLaunchKernelGGL(kernel, dim3((count + kT - 1) / kT), dim3(kT), lds, s, args...);
    prof_end(prof, s);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// without keypoints the counts these kernels accumulate (nmatches, nmap, pose_n, ninl) stay 0, as uploaded;
// without local-map points so does n_to_match
int launch_mm_tail(const TrkBufs& t, hipStream_t s, ProfileHook* prof) { return launch_1d("k_mm_tail", k_mm_tail, t.cur_n, 0, s, prof, t); }
int launch_frustum(const MatchCam& cam, const LmBufs& t, hipStream_t s, ProfileHook* prof)
{
    return launch_1d("k_frustum", k_frustum, t.mp_n, 0, s, prof, cam, t);
}
int launch_lm_pose_prep(const LmBufs& t, hipStream_t s, ProfileHook* prof)
{
    return launch_1d("k_lm_pose_prep", k_lm_pose_prep, t.cur_n, 0, s, prof, t);
}
int launch_lm_tail(const LmBufs& t, hipStream_t s, ProfileHook* prof) { return launch_1d("k_lm_tail", k_lm_tail, t.cur_n, 0, s, prof, t); }
int launch_trk_pose_prep(const TrkBufs& t, hipStream_t s, ProfileHook* prof)
{
    return launch_1d("k_trk_pose_prep", k_trk_pose_prep, t.cur_n, 0, s, prof, t);
}
int launch_trk_tail(const TrkBufs& t, hipStream_t s, ProfileHook* prof) { return launch_1d("k_trk_tail", k_trk_tail, t.cur_n, 0, s, prof, t); }

int launch_vo_points(const VoBufs& v, hipStream_t s, ProfileHook* prof)
{
    if (v.n <= 0) return 0;
    if (v.n > kVoMaxLast) return -2;
    lds_limit_max((const void*)k_vo_points);        // kVoMaxLast depths are the default limit exactly
    return launch_1d("k_vo_points", k_vo_points, v.n, (size_t)((v.n + 3) & ~3) * sizeof(float), s, prof, v);
}

int launch_tlm_snapshot(const TlmBufs& t, int F, hipStream_t s, ProfileHook* prof)
{
    prof_begin(prof, "k_tlm_snapshot", s);
    hipLaunchKernelGGL(k_tlm_snapshot, dim3((t.K + kT - 1) / kT, F), dim3(kT), 0, s, t);
    prof_end(prof, s);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_tlm_frustum(const MatchCam& cam, const TlmBufs& t, int F, hipStream_t s, ProfileHook* prof)
{
    if (F < 2) return 0;
    prof_begin(prof, "k_tlm_discard", s);
    hipLaunchKernelGGL(k_tlm_discard, dim3((t.K + kT - 1) / kT, F - 1), dim3(kT), 0, s, t);
    prof_end(prof, s);
    prof_begin(prof, "k_tlm_frustum", s);
    hipLaunchKernelGGL(k_tlm_frustum, dim3((2 * t.K + kT - 1) / kT, F - 1), dim3(kT), 0, s, cam, t);
    prof_end(prof, s);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_tlm_pose_prep(const TlmBufs& t, int F, hipStream_t s, ProfileHook* prof)
{
    if (F < 2) return 0;
    prof_begin(prof, "k_tlm_pose_prep", s);
    hipLaunchKernelGGL(k_tlm_pose_prep, dim3((t.K + kT - 1) / kT, F - 1), dim3(kT), 0, s, t);
    prof_end(prof, s);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
