// coeb_rgbd_stream_host.hpp -- what coeb_rgbd_stream_frame (coeb_capi.hip) does before its first
// HIP call: the argument checks, the layout of one call in the context's page-locked buffer, the
// layout of the device memory a stream owns, and the slot arithmetic.  Plain C++ with no HIP
// type, so tests/host/rgbd_stream_host_main.cpp runs it under ASan + UBSan without a device.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/coeb_front.h"
#include "coeb_single_frame_host.hpp"

constexpr int kStreamTmCap = 1024;          // T_M points k_fm can leave (coeb_flow.hip's kMaxPts)
constexpr int kStreamLkLevels = 8;          // coeb_flow.hip's kLkMaxLevels
constexpr int kStreamLkWin = 22, kStreamLkMaxLevel = 5;     // Frame.cc:335

// The block of results a call's kernels leave behind the current frame's gray level 0 in its
// slot, copied back in one piece: T_M, its count (-1: F empty), the predecessor's corner count
// (-1: COEB_ERANGE) and the blur flags.
struct RgbdStreamRes {
    float tm[kStreamTmCap * 2];
    int32_t ntm, ncorners, pad[2];
    int32_t flag[COEB_MAX_BOXES];
};
inline constexpr size_t kStreamResBytes = (sizeof(RgbdStreamRes) + 255) & ~(size_t)255;

// The head of the one upload: {0, nbox} as launch_extract's box offsets, then the boxes.
struct RgbdStreamHdr {
    int32_t box_off[4];
    coeb_box box[COEB_MAX_BOXES];
};
inline constexpr size_t kStreamHdrBytes = (sizeof(RgbdStreamHdr) + 255) & ~(size_t)255;

// 0: run the frame; 1: empty image (COEB_OK, n = 0, the stream untouched); COEB_EINVAL: *why
// names the argument.  prev_w / prev_h: the stream's predecessor (0: none, any size is taken).
inline int rgbd_stream_check(const uint8_t* img, size_t img_stride, int channels, int W, int H, const void* depth,
                             size_t depth_stride, int depth_type, const coeb_camera* cam, const coeb_box* boxes, int nbox,
                             const coeb_rgbd_stream_out* out, int prev_w, int prev_h, const char** why)
{
    *why = "";
    if (!out) { *why = "null output struct"; return COEB_EINVAL; }
    if (!img || W <= 0 || H <= 0) return 1;
    if (channels != 1 && channels != 3 && channels != 4) { *why = "channels must be 1, 3 or 4"; return COEB_EINVAL; }
    if (img_stride < (size_t)W * channels) { *why = "img_stride < one row"; return COEB_EINVAL; }
    if (nbox < 0 || nbox > COEB_MAX_BOXES) { *why = "bad box count"; return COEB_EINVAL; }
    if (nbox && !boxes) { *why = "null box array"; return COEB_EINVAL; }
    if (depth_type != COEB_DEPTH_U16 && depth_type != COEB_DEPTH_F32) { *why = "bad depth_type"; return COEB_EINVAL; }
    if (!depth) { *why = "null depth map"; return COEB_EINVAL; }
    if (depth_stride < (size_t)W * (depth_type == COEB_DEPTH_F32 ? 4 : 2)) { *why = "depth_stride < one row"; return COEB_EINVAL; }
    if (!cam) { *why = "null camera"; return COEB_EINVAL; }
    if (!out->kp || !out->desc || !out->u_right || !out->depth) { *why = "null output array"; return COEB_EINVAL; }
    if (out->tm_cap < 0 || (out->tm_cap > 0 && !out->tm_xy)) { *why = "null T_M array"; return COEB_EINVAL; }
    if (nbox && !out->blur_flag) { *why = "null blur_flag array"; return COEB_EINVAL; }
    if (out->gray && out->gray_stride < (size_t)W) { *why = "gray_stride < width"; return COEB_EINVAL; }
    if (W < 32 || H < 32 || (size_t)W * H > (size_t)1 << 26) { *why = "frame size outside 32 x 32 .. 2^26 pixels"; return COEB_EINVAL; }
    if (prev_w && (W != prev_w || H != prev_h)) { *why = "frame size differs from the stream's previous frame (reset first)"; return COEB_EINVAL; }
    return 0;
}

// One call in the page-locked buffer, every offset 256-byte aligned.  [0, up_bytes) is the one
// upload: the head, then the image rows (channels bytes per pixel, packed).  The records the tail
// kernel writes through the buffer's device address follow as in FrameRgbdLayout; then the copy
// back -- the gray level 0 (kept only when the caller asks for it and the kernels made it) with
// the result block right behind it, as they lie in the slot -- and the depth rows the tail kernel
// gathers from.
struct RgbdStreamLayout {
    size_t o_hdr, o_img, img_row, up_bytes;
    size_t o_n, o_k, o_d, o_kun, o_ur, o_dep;
    size_t o_gray, o_res;
    size_t o_depth, depth_row;
    size_t total;
};

inline RgbdStreamLayout rgbd_stream_layout(int W, int H, int channels, int kcap, int depth_type)
{
    RgbdStreamLayout L;
    const size_t k = (size_t)kcap;
    L.o_hdr = 0;
    L.o_img = kStreamHdrBytes;
    L.img_row = (size_t)W * channels;
    L.up_bytes = L.o_img + L.img_row * H;
    L.o_n = single_frame_al256(L.up_bytes);
    L.o_k = L.o_n + 256;
    L.o_d = L.o_k + single_frame_al256(k * sizeof(coeb_keypoint));
    L.o_kun = L.o_d + single_frame_al256(k * 32);
    L.o_ur = L.o_kun + single_frame_al256(k * sizeof(coeb_keypoint));
    L.o_dep = L.o_ur + single_frame_al256(k * 4);
    L.o_gray = L.o_dep + single_frame_al256(k * 4);
    L.o_res = L.o_gray + single_frame_al256((size_t)W * H);
    L.o_depth = L.o_res + kStreamResBytes;
    L.depth_row = (size_t)W * (depth_type == COEB_DEPTH_F32 ? 4 : 2);
    L.total = L.o_depth + single_frame_al256(L.depth_row * H);
    return L;
}

// calcOpticalFlowPyrLK's level count for a frame (buildOpticalFlowPyramid stops at the window)
inline int rgbd_stream_lk_levels(int w, int h)
{
    for (int level = 0; level <= kStreamLkMaxLevel; level++) {
        w = (w + 1) / 2; h = (h + 1) / 2;
        if (w <= kStreamLkWin || h <= kStreamLkWin) return level + 1;
    }
    return kStreamLkMaxLevel + 1;
}

// The device memory of a stream: two slots, one per frame parity, then the scratch of the
// previous-frame-only work and of the LK / fundamental-matrix step (sized by coeb_flow.hip).
// A slot holds what the next call needs of its frame: the head and gray level 0 (a 1-channel
// upload lands on both at once), the result block, LK levels 1.., the Scharr planes of every
// level (written behind the call, read by the next call's k_lk while the work behind that call
// already fills the other slot's) and the refined corners with their count.
struct RgbdStreamSlot {
    int L;                                   // LK levels of the frame
    int lw[kStreamLkLevels], lh[kStreamLkLevels];
    size_t s_hdr, s_gray, s_res;
    size_t s_lvl[kStreamLkLevels];           // level l >= 1 (pitch lw[l])
    size_t s_der[kStreamLkLevels];           // Scharr plane of level l, 4 bytes per pixel
    size_t s_pts, s_npts;
    size_t bytes;
};

inline RgbdStreamSlot rgbd_stream_slot(int W, int H)
{
    RgbdStreamSlot S;
    memset(&S, 0, sizeof(S));
    S.L = rgbd_stream_lk_levels(W, H);
    S.lw[0] = W; S.lh[0] = H;
    for (int l = 1; l < S.L; l++) { S.lw[l] = (S.lw[l - 1] + 1) / 2; S.lh[l] = (S.lh[l - 1] + 1) / 2; }
    S.s_hdr = 0;
    S.s_gray = kStreamHdrBytes;
    S.s_res = S.s_gray + single_frame_al256((size_t)W * H);
    size_t o = S.s_res + kStreamResBytes;
    for (int l = 1; l < S.L; l++) { S.s_lvl[l] = o; o += single_frame_al256((size_t)S.lw[l] * S.lh[l]); }
    for (int l = 0; l < S.L; l++) { S.s_der[l] = o; o += single_frame_al256((size_t)S.lw[l] * S.lh[l] * 4); }
    S.s_pts = o; o += single_frame_al256((size_t)kStreamTmCap * 8);
    S.s_npts = o; o += 256;
    S.bytes = o;
    return S;
}

// frame `seq` of a stream (0, 1, ..; a reset does not restart it) lives in slot seq & 1, its
// predecessor in the other one
inline int rgbd_stream_slot_of(uint64_t seq) { return (int)(seq & 1); }

// T_M points handed to the caller: all k_fm found, never more than the caller's array takes
inline int rgbd_stream_tm_count(int n_tm, int tm_cap) { return n_tm < 0 ? 0 : (n_tm < tm_cap ? n_tm : tm_cap); }
