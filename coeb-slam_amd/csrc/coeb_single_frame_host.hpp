// coeb_single_frame_host.hpp -- what the single-frame host-buffer calls coeb_extract and
// coeb_frame_rgbd (coeb_capi.hip) do before their first HIP call: the argument checks, the layout
// of their inputs and results in the context's page-locked buffer, and the row staging.  Plain
// C++ with no HIP type, so tests/host/frame_rgbd_host_main.cpp runs it under ASan + UBSan
// without a device.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/coeb_front.h"

// coeb_extract prefixes this one refusal with its name, coeb_frame_rgbd all of them
inline constexpr const char* kWhyNullDynArrays = "null box / T_M array";

// The arguments both calls take.  0: run the frame; 1: empty image (COEB_OK with *n_out = 0,
// ORBextractor.cc:1096-1097); COEB_EINVAL: *why names the argument.
inline int single_frame_check(const uint8_t* gray, int W, int H, size_t stride, const coeb_box* boxes, int nbox,
                              const float* tm_xy, int ntm, int nblur, const char** why)
{
    *why = "";
    if (!gray || W <= 0 || H <= 0) return 1;
    if (stride < (size_t)W) { *why = "stride < width"; return COEB_EINVAL; }
    if (nbox < 0 || nbox > COEB_MAX_BOXES || ntm < 0 || nblur < 0) { *why = "bad box/T_M counts"; return COEB_EINVAL; }
    if ((nbox && !boxes) || (ntm && !tm_xy)) { *why = kWhyNullDynArrays; return COEB_EINVAL; }
    return 0;
}

// single_frame_check, then coeb_frame_rgbd's own depth / camera / output arguments
inline int frame_rgbd_check(const uint8_t* gray, int W, int H, size_t stride, const void* depth, size_t depth_stride,
                            int depth_type, const coeb_camera* cam, const coeb_box* boxes, int nbox, const float* tm_xy,
                            int ntm, int nblur, const coeb_keypoint* kp_out, const uint8_t* desc_out,
                            const float* u_right_out, const float* depth_out, const char** why)
{
    if (int rc = single_frame_check(gray, W, H, stride, boxes, nbox, tm_xy, ntm, nblur, why)) return rc;
    if (depth_type != COEB_DEPTH_U16 && depth_type != COEB_DEPTH_F32) { *why = "bad depth_type"; return COEB_EINVAL; }
    if (!depth) { *why = "null depth map"; return COEB_EINVAL; }
    if (depth_stride < (size_t)W * (depth_type == COEB_DEPTH_F32 ? 4 : 2)) { *why = "depth_stride < one row"; return COEB_EINVAL; }
    if (!cam) { *why = "null camera"; return COEB_EINVAL; }
    if (!kp_out || !desc_out || !u_right_out || !depth_out) { *why = "null output array"; return COEB_EINVAL; }
    return 0;
}

// Byte offsets into the page-locked buffer, all 16-byte aligned.  [0, o_n) holds the gray rows on
// their way to the device; then the count + error word, the records, the descriptors and the
// dynamic-mask inputs (boxes, their offsets, blur flags, T_M offsets, T_M points).  Both calls
// use these regions; total is what coeb_extract asks of the buffer.
struct SingleFrameLayout {
    size_t o_n, o_k, o_d, o_dyn, o_bo, o_bl, o_to, o_tm;
    size_t total;
};

// coeb_frame_rgbd: the tail kernel's own results and the depth rows it gathers from follow the
// shared regions, so a coeb_extract call before or after finds its regions as it left them.
struct FrameRgbdLayout : SingleFrameLayout {
    size_t o_kun, o_ur, o_dep;     // kp_un records, uRight, depth per keypoint (kcap entries each)
    size_t o_depth;                // W x H depth values, packed rows of depth_row bytes
    size_t depth_row;
};

inline size_t single_frame_al256(size_t v) { return (v + 255) & ~(size_t)255; }

inline SingleFrameLayout single_frame_layout(int W, int H, int kcap, int nbox, int ntm)
{
    SingleFrameLayout L;
    const size_t k = (size_t)kcap;
    L.o_n = single_frame_al256((size_t)W * H);
    L.o_k = L.o_n + 256;
    L.o_d = L.o_k + single_frame_al256(k * sizeof(coeb_keypoint));
    L.o_dyn = L.o_d + single_frame_al256(k * 32);
    L.o_bo = L.o_dyn + (size_t)nbox * sizeof(coeb_box);
    L.o_bl = L.o_bo + 16;
    L.o_to = L.o_bl + (size_t)nbox * 4 + 16;
    L.o_tm = L.o_to + 16;
    L.total = L.o_tm + (size_t)ntm * 8;
    return L;
}

inline FrameRgbdLayout frame_rgbd_layout(int W, int H, int kcap, int nbox, int ntm, int depth_type)
{
    FrameRgbdLayout L;
    static_cast<SingleFrameLayout&>(L) = single_frame_layout(W, H, kcap, nbox, ntm);
    const size_t k = (size_t)kcap;
    L.o_kun = single_frame_al256(L.total);
    L.o_ur = L.o_kun + single_frame_al256(k * sizeof(coeb_keypoint));
    L.o_dep = L.o_ur + single_frame_al256(k * 4);
    L.o_depth = L.o_dep + single_frame_al256(k * 4);
    L.depth_row = (size_t)W * (depth_type == COEB_DEPTH_F32 ? 4 : 2);
    L.total = L.o_depth + single_frame_al256(L.depth_row * H);
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
inline void single_frame_stage_rows(uint8_t* dst, const void* src, int rows, size_t row_bytes, size_t stride)
{
    if (stride == row_bytes) {
        memcpy(dst, src, row_bytes * (size_t)rows);
        return;
    }
    for (int y = 0; y < rows; y++) memcpy(dst + (size_t)y * row_bytes, static_cast<const uint8_t*>(src) + (size_t)y * stride, row_bytes);
}
