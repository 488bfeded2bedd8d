// coeb_frame_rgbd_host.hpp -- what coeb_frame_rgbd (coeb_capi.hip) does before its first HIP
// call: the argument check, the layout of its inputs and results in the context's page-locked
// buffer, and the row staging.  Plain C++ with no HIP type, so tests/host/frame_rgbd_host_main.cpp
// runs it under ASan + UBSan without a device.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/coeb_front.h"

// 0: run the frame; 1: empty image (COEB_OK with *n_out = 0, ORBextractor.cc:1096-1097);
// COEB_EINVAL: *why names the argument.  The first four cases are coeb_extract's, in its order.
inline int frame_rgbd_check(const uint8_t* gray, int W, int H, size_t stride, const void* depth, size_t depth_stride,
                            int depth_type, const coeb_camera* cam, const coeb_box* boxes, int nbox, const float* tm_xy,
                            int ntm, int nblur, const coeb_keypoint* kp_out, const uint8_t* desc_out,
                            const float* u_right_out, const float* depth_out, const char** why)
{
    *why = "";
    if (!gray || W <= 0 || H <= 0) return 1;
    if (stride < (size_t)W) { *why = "stride < width"; return COEB_EINVAL; }
    if (nbox < 0 || nbox > COEB_MAX_BOXES || ntm < 0 || nblur < 0) { *why = "bad box/T_M counts"; return COEB_EINVAL; }
    if ((nbox && !boxes) || (ntm && !tm_xy)) { *why = "null box / T_M array"; return COEB_EINVAL; }
    if (depth_type != COEB_DEPTH_U16 && depth_type != COEB_DEPTH_F32) { *why = "bad depth_type"; return COEB_EINVAL; }
    if (!depth) { *why = "null depth map"; return COEB_EINVAL; }
    if (depth_stride < (size_t)W * (depth_type == COEB_DEPTH_F32 ? 4 : 2)) { *why = "depth_stride < one row"; return COEB_EINVAL; }
    if (!cam) { *why = "null camera"; return COEB_EINVAL; }
    if (!kp_out || !desc_out || !u_right_out || !depth_out) { *why = "null output array"; return COEB_EINVAL; }
    return 0;
}

// Byte offsets into the page-locked buffer, all 16-byte aligned.  [0, o_n) holds the gray rows on
// their way to the device; o_n .. o_tm are the regions coeb_extract uses (count + error word,
// records, descriptors, then the dynamic-mask inputs); the tail kernel's own results and the
// depth rows it gathers from follow them, so a coeb_extract call before or after finds its own
// regions as it left them.
struct FrameRgbdLayout {
    size_t o_n, o_k, o_d, o_dyn, o_bo, o_bl, o_to, o_tm;
    size_t o_kun, o_ur, o_dep;     // kp_un records, uRight, depth per keypoint (kcap entries each)
    size_t o_depth;                // W x H depth values, packed rows of depth_row bytes
    size_t depth_row, total;
};

inline size_t frame_rgbd_al256(size_t v) { return (v + 255) & ~(size_t)255; }

inline FrameRgbdLayout frame_rgbd_layout(int W, int H, int kcap, int nbox, int ntm, int depth_type)
{
    FrameRgbdLayout L;
    const size_t k = (size_t)kcap;
    L.o_n = frame_rgbd_al256((size_t)W * H);
    L.o_k = L.o_n + 256;
    L.o_d = L.o_k + frame_rgbd_al256(k * sizeof(coeb_keypoint));
    L.o_dyn = L.o_d + frame_rgbd_al256(k * 32);
    L.o_bo = L.o_dyn + (size_t)nbox * sizeof(coeb_box);
    L.o_bl = L.o_bo + 16;
    L.o_to = L.o_bl + (size_t)nbox * 4 + 16;
    L.o_tm = L.o_to + 16;
    L.o_kun = frame_rgbd_al256(L.o_tm + (size_t)ntm * 8);
    L.o_ur = L.o_kun + frame_rgbd_al256(k * sizeof(coeb_keypoint));
    L.o_dep = L.o_ur + frame_rgbd_al256(k * 4);
    L.o_depth = L.o_dep + frame_rgbd_al256(k * 4);
    L.depth_row = (size_t)W * (depth_type == COEB_DEPTH_F32 ? 4 : 2);
    L.total = L.o_depth + frame_rgbd_al256(L.depth_row * H);
    return L;
}

// Tracking.cc:227: a 32F map with mDepthMapFactor == 1 is not converted
inline int frame_rgbd_depth_copy(int depth_type, float depth_scale)
{
    const float d = depth_scale - 1.0f;
    return depth_type == COEB_DEPTH_F32 && !((d < 0 ? -d : d) > 1e-5f);
}

// records the tail kernel packs: all the caller can take, never more than the device holds
inline int frame_rgbd_guess(int kcap, int cap) { return cap < 0 ? 0 : (cap < kcap ? cap : kcap); }

// `rows` rows of `row_bytes` bytes, `stride` bytes apart in src, packed into dst
inline void frame_rgbd_stage_rows(uint8_t* dst, const void* src, int rows, size_t row_bytes, size_t stride)
{
    if (stride == row_bytes) {
        memcpy(dst, src, row_bytes * (size_t)rows);
        return;
    }
    for (int y = 0; y < rows; y++) memcpy(dst + (size_t)y * row_bytes, static_cast<const uint8_t*>(src) + (size_t)y * stride, row_bytes);
}
