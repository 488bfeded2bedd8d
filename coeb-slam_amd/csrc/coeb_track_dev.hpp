// coeb_track_dev.hpp -- the device arithmetic of Frame::isInFrustum (Frame.cc:445-501) with
// MapPoint::PredictScale (MapPoint.cc:402-417), shared by the two kernels of coeb_track.hip that
// put a local map through it: k_tlm_frustum (the batch chain's two-keyframe map) and k_frustum
// (an arbitrary map from host buffers).  The float forms are those of oracle/orb_oracle.c
// (oc_is_in_frustum); DESIGN.md s4.3 lists them.
#pragma once
#include <hip/hip_runtime.h>

#include "coeb_internal.hpp"

// x = R*X + t (cv::Mat R*X + t: small-matrix float products, the addend added in double)
__device__ __forceinline__ void gemm_add(const float* T, const float* X, float* out)
{
#pragma unroll
    for (int k = 0; k < 3; k++) {
        float v = T[k * 4 + 0] * X[0] + T[k * 4 + 1] * X[1];
        v = v + T[k * 4 + 2] * X[2];
        out[k] = (float)((double)v + (double)T[k * 4 + 3]);
    }
}

// cv::norm of a float 3-vector: float components squared and summed in double
__device__ __forceinline__ double norm3(const float* d)
{
    double ss = 0.0;
    ss += (double)d[0] * (double)d[0];
    ss += (double)d[1] * (double)d[1];
    ss += (double)d[2] * (double)d[2];
    return sqrt(ss);
}

// What isInFrustum leaves on the MapPoint: mbTrackInView, mTrackProjX / Y / XR,
// mnTrackScaleLevel, mTrackViewCos (zeros when not in view).
struct FrustumView {
    bool in_view;
    float u, v, ur, view_cos;
    int level;
};

// T: mTcw (row-major 4x4).  P: GetWorldPos(), Pn: GetNormal(), maxd / mind: mfMaxDistance /
// mfMinDistance (the invariance range is 1.2f / 0.8f of them), cos_limit: viewingCosLimit.
__device__ __forceinline__ FrustumView is_in_frustum(const MatchCam& cam, const float* T, const float* P,
                                                     const float* Pn, float maxd, float mind, float cos_limit)
{
    FrustumView r{false, 0.f, 0.f, 0.f, 0.f, 0};
    float Pc[3];
    gemm_add(T, P, Pc);                                    // Pc = mRcw*P + mtcw (:453)
    bool v = !(Pc[2] < 0.0f);                              // :459-460
    float u = 0.f, vv = 0.f, invz = 0.f;
    if (v) {
        invz = 1.0f / Pc[2];
        u = __builtin_fmaf(cam.fx * Pc[0], invz, cam.cx);  // :464-465, fused
        vv = __builtin_fmaf(cam.fy * Pc[1], invz, cam.cy);
        if (u < cam.min_x || u > cam.max_x) v = false;     // :467-470
        if (vv < cam.min_y || vv > cam.max_y) v = false;
    }
    float dist = 0.f, viewCos = 0.f;
    if (v) {
        float Oc[3];
        for (int k = 0; k < 3; k++) {                      // mOw = -mRcw.t()*mtcw (GEMM_1_T)
            double s = (double)T[0 * 4 + k] * T[3] + (double)T[1 * 4 + k] * T[7];
            s = s + (double)T[2 * 4 + k] * T[11];
            Oc[k] = (float)(s * -1.0);
        }
        const float PO[3] = {P[0] - Oc[0], P[1] - Oc[1], P[2] - Oc[2]};
        dist = (float)norm3(PO);                           // :476
        if (dist < 0.8f * mind || dist > 1.2f * maxd) v = false;   // :478-479
        if (v) {
            double dot = 0.0;                              // Mat::dot of floats accumulates in double (:484)
            dot += (double)PO[0] * (double)Pn[0];
            dot += (double)PO[1] * (double)Pn[1];
            dot += (double)PO[2] * (double)Pn[2];
            viewCos = (float)(dot / (double)dist);
            if (viewCos < cos_limit) v = false;            // :486-487
        }
    }
    if (v) {
        const float ratio = maxd / dist;                   // PredictScale
        int s = (int)ceilf((float)log((double)ratio) / cam.log_sf);
        r.level = s < 0 ? 0 : (s >= cam.nlevels ? cam.nlevels - 1 : s);
        r.in_view = true;
        r.u = u;
        r.v = vv;
        r.ur = __builtin_fmaf(-cam.bf, invz, u);           // u - mbf*invz (fused)
        r.view_cos = viewCos;
    }
    return r;
}
