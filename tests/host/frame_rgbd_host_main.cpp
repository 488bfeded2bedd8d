// The host part of coeb_extract and coeb_frame_rgbd (coeb-slam_amd/csrc/coeb_single_frame_host.hpp:
// argument checks, page-locked buffer layout, row staging) run without a device, built with
// ASan + UBSan by tests/test_frame_rgbd_host.py.  Exit status 0 and "ok" on stdout: every check held.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "coeb_single_frame_host.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            g_fail++;                                                    \
        }                                                                \
    } while (0)

// every region of the layout: [offset, offset + bytes)
struct Region { const char* name; size_t off, bytes; };

static void check_layout(int W, int H, int kcap, int nbox, int ntm, int dtype)
{
    const FrameRgbdLayout L = frame_rgbd_layout(W, H, kcap, nbox, ntm, dtype);
    const size_t k = (size_t)kcap, db = dtype == COEB_DEPTH_F32 ? 4 : 2;
    const Region r[] = {
        {"gray", 0, (size_t)W * H},        {"n+err", L.o_n, 20},           {"kps", L.o_k, k * 28},
        {"desc", L.o_d, k * 32},           {"boxes", L.o_dyn, (size_t)nbox * 16}, {"box_off", L.o_bo, 8},
        {"blur", L.o_bl, (size_t)nbox * 4}, {"tm_off", L.o_to, 8},         {"tm", L.o_tm, (size_t)ntm * 8},
        {"kps_un", L.o_kun, k * 28},       {"ur", L.o_ur, k * 4},          {"dep", L.o_dep, k * 4},
        {"depth", L.o_depth, (size_t)W * H * db},
    };
    const int nr = (int)(sizeof r / sizeof r[0]);
    for (int i = 0; i < nr; i++) {
        CHECK(r[i].off % 4 == 0);                                   // 32-bit words everywhere
        CHECK(r[i].off + r[i].bytes <= L.total);
        if (i + 1 < nr) CHECK(r[i].off + r[i].bytes <= r[i + 1].off);   // in order, no overlap
    }
    CHECK(L.o_k % 16 == 0 && L.o_d % 16 == 0);                       // k_frame_tail's uint4 descriptor stores
    CHECK(L.o_kun % 256 == 0 && L.o_depth % 256 == 0);
    CHECK(L.depth_row == (size_t)W * db);
    // coeb_extract's layout for the same frame: a prefix of this one whatever the depth type, so
    // either call finds the shared regions where the other left them, and coeb_extract's buffer
    // ends with its T_M points
    const SingleFrameLayout S = single_frame_layout(W, H, kcap, nbox, ntm);
    const FrameRgbdLayout O = frame_rgbd_layout(W, H, kcap, nbox, ntm, dtype == COEB_DEPTH_F32 ? COEB_DEPTH_U16 : COEB_DEPTH_F32);
    for (const SingleFrameLayout& q : {SingleFrameLayout(L), SingleFrameLayout(O)}) {
        CHECK(q.o_n == S.o_n && q.o_k == S.o_k && q.o_d == S.o_d && q.o_dyn == S.o_dyn);
        CHECK(q.o_bo == S.o_bo && q.o_bl == S.o_bl && q.o_to == S.o_to && q.o_tm == S.o_tm);
    }
    CHECK(S.total == S.o_tm + (size_t)ntm * 8 && S.total <= L.o_kun);
    // the staging writes of the call, on a buffer of exactly `total` bytes (ASan sees an overrun):
    // strided sources whose padding must not arrive
    std::vector<uint8_t> pin(L.total, 0xEE);
    const size_t gs = (size_t)W + 9, ds = L.depth_row + 6;
    std::vector<uint8_t> gray(gs * H, 0xAA), dep(ds * H, 0xBB);
    for (int y = 0; y < H; y++) {
        for (int x = 0; x < W; x++) gray[y * gs + x] = (uint8_t)(x + 3 * y);
        for (size_t b = 0; b < L.depth_row; b++) dep[y * ds + b] = (uint8_t)(b + 5 * y);
    }
    single_frame_stage_rows(pin.data(), gray.data(), H, (size_t)W, gs);
    single_frame_stage_rows(pin.data() + L.o_depth, dep.data(), H, L.depth_row, ds);
    bool ok = true;
    for (int y = 0; y < H && ok; y++) {
        for (int x = 0; x < W; x++) ok = ok && pin[(size_t)y * W + x] == (uint8_t)(x + 3 * y);
        for (size_t b = 0; b < L.depth_row; b++) ok = ok && pin[L.o_depth + y * L.depth_row + b] == (uint8_t)(b + 5 * y);
    }
    CHECK(ok);
    for (size_t i = (size_t)W * H; i < L.o_n; i++) ok = ok && pin[i] == 0xEE;
    for (size_t i = L.o_depth + L.depth_row * H; i < L.total; i++) ok = ok && pin[i] == 0xEE;
    CHECK(ok);
    // packed sources take the one-memcpy branch
    std::vector<uint8_t> pin2(L.total, 0xEE), g2((size_t)W * H, 7);
    single_frame_stage_rows(pin2.data(), g2.data(), H, (size_t)W, (size_t)W);
    CHECK(pin2[0] == 7 && pin2[(size_t)W * H - 1] == 7 && (L.o_n == (size_t)W * H || pin2[(size_t)W * H] == 0xEE));
}

static void check_einval()
{
    uint8_t g[16] = {0}, desc[32];
    float depth[16] = {0}, ur[1], dd[1], tm[2] = {0, 0};
    coeb_keypoint kp[1];
    coeb_box box[1] = {{0, 0, 1, 1}};
    const coeb_camera cam{500, 500, 2, 2, 40, 0, 4, 0, 4};
    const char* why = nullptr;
    auto run = [&](const uint8_t* gray, int W, int H, size_t stride, const void* dp, size_t dstride, int dtype,
                   const coeb_camera* c, const coeb_box* b, int nbox, const float* t, int ntm, int nblur,
                   const coeb_keypoint* ko, const uint8_t* dsc, const float* u, const float* d) {
        return frame_rgbd_check(gray, W, H, stride, dp, dstride, dtype, c, b, nbox, t, ntm, nblur, ko, dsc, u, d, &why);
    };
    // the good call, both depth types, with and without the optional arrays
    CHECK(run(g, 4, 4, 4, depth, 16, COEB_DEPTH_F32, &cam, nullptr, 0, nullptr, 0, 0, kp, desc, ur, dd) == 0);
    CHECK(run(g, 4, 4, 4, depth, 8, COEB_DEPTH_U16, &cam, box, 1, tm, 1, 1, kp, desc, ur, dd) == 0);
    CHECK(run(g, 4, 4, 9, depth, 40, COEB_DEPTH_F32, &cam, box, 1, nullptr, 0, 0, kp, desc, ur, dd) == 0);
    // empty image first, whatever else is wrong (ORBextractor.cc:1096-1097)
    CHECK(run(nullptr, 4, 4, 4, nullptr, 0, 7, nullptr, nullptr, -1, nullptr, -1, -1, nullptr, nullptr, nullptr, nullptr) == 1);
    CHECK(run(g, 0, 4, 4, depth, 16, COEB_DEPTH_F32, &cam, nullptr, 0, nullptr, 0, 0, kp, desc, ur, dd) == 1);
    CHECK(run(g, 4, -1, 4, depth, 16, COEB_DEPTH_F32, &cam, nullptr, 0, nullptr, 0, 0, kp, desc, ur, dd) == 1);
    // coeb_extract's cases
    CHECK(run(g, 4, 4, 3, depth, 16, COEB_DEPTH_F32, &cam, nullptr, 0, nullptr, 0, 0, kp, desc, ur, dd) == COEB_EINVAL);
    CHECK(run(g, 4, 4, 4, depth, 16, COEB_DEPTH_F32, &cam, box, -1, nullptr, 0, 0, kp, desc, ur, dd) == COEB_EINVAL);
    CHECK(run(g, 4, 4, 4, depth, 16, COEB_DEPTH_F32, &cam, box, COEB_MAX_BOXES + 1, nullptr, 0, 0, kp, desc, ur, dd) == COEB_EINVAL);
    CHECK(run(g, 4, 4, 4, depth, 16, COEB_DEPTH_F32, &cam, nullptr, 0, tm, -1, 0, kp, desc, ur, dd) == COEB_EINVAL);
    CHECK(run(g, 4, 4, 4, depth, 16, COEB_DEPTH_F32, &cam, nullptr, 0, nullptr, 0, -1, kp, desc, ur, dd) == COEB_EINVAL);
    CHECK(run(g, 4, 4, 4, depth, 16, COEB_DEPTH_F32, &cam, nullptr, 1, nullptr, 0, 0, kp, desc, ur, dd) == COEB_EINVAL);
    CHECK(run(g, 4, 4, 4, depth, 16, COEB_DEPTH_F32, &cam, nullptr, 0, nullptr, 1, 0, kp, desc, ur, dd) == COEB_EINVAL);
    // the depth map
    CHECK(run(g, 4, 4, 4, nullptr, 16, COEB_DEPTH_F32, &cam, nullptr, 0, nullptr, 0, 0, kp, desc, ur, dd) == COEB_EINVAL);
    CHECK(run(g, 4, 4, 4, depth, 15, COEB_DEPTH_F32, &cam, nullptr, 0, nullptr, 0, 0, kp, desc, ur, dd) == COEB_EINVAL);
    CHECK(run(g, 4, 4, 4, depth, 7, COEB_DEPTH_U16, &cam, nullptr, 0, nullptr, 0, 0, kp, desc, ur, dd) == COEB_EINVAL);
    CHECK(run(g, 4, 4, 4, depth, 16, 2, &cam, nullptr, 0, nullptr, 0, 0, kp, desc, ur, dd) == COEB_EINVAL);
    CHECK(run(g, 4, 4, 4, depth, 16, -1, &cam, nullptr, 0, nullptr, 0, 0, kp, desc, ur, dd) == COEB_EINVAL);
    // camera and the required outputs
    CHECK(run(g, 4, 4, 4, depth, 16, COEB_DEPTH_F32, nullptr, nullptr, 0, nullptr, 0, 0, kp, desc, ur, dd) == COEB_EINVAL);
    CHECK(run(g, 4, 4, 4, depth, 16, COEB_DEPTH_F32, &cam, nullptr, 0, nullptr, 0, 0, nullptr, desc, ur, dd) == COEB_EINVAL);
    CHECK(run(g, 4, 4, 4, depth, 16, COEB_DEPTH_F32, &cam, nullptr, 0, nullptr, 0, 0, kp, nullptr, ur, dd) == COEB_EINVAL);
    CHECK(run(g, 4, 4, 4, depth, 16, COEB_DEPTH_F32, &cam, nullptr, 0, nullptr, 0, 0, kp, desc, nullptr, dd) == COEB_EINVAL);
    CHECK(run(g, 4, 4, 4, depth, 16, COEB_DEPTH_F32, &cam, nullptr, 0, nullptr, 0, 0, kp, desc, ur, nullptr) == COEB_EINVAL);
    CHECK(why && why[0]);                                           // a refusal names its argument
}

int main()
{
    // the sizes of tests/test_gpu_frame_rgbd.py (640x480; kcap is a few thousand there) and the
    // edges: one pixel, odd sizes, no keypoint capacity, full box / T_M arrays, both depth types
    const int sizes[][2] = {{640, 480}, {1, 1}, {321, 243}, {3, 5}, {255, 1}, {256, 1}, {257, 3}, {1280, 960}};
    const int kcaps[] = {0, 1, 9, 1000, 2744};
    for (const auto& s : sizes)
        for (int kcap : kcaps)
            for (int dtype : {COEB_DEPTH_U16, COEB_DEPTH_F32}) {
                check_layout(s[0], s[1], kcap, 0, 0, dtype);
                check_layout(s[0], s[1], kcap, COEB_MAX_BOXES, 1000, dtype);
                check_layout(s[0], s[1], kcap, 3, 1, dtype);
            }
    check_einval();
    // pass-through rule of Tracking.cc:227 and the packed-record count
    CHECK(frame_rgbd_depth_copy(COEB_DEPTH_F32, 1.0f) == 1 && frame_rgbd_depth_copy(COEB_DEPTH_F32, 1.000005f) == 1);
    CHECK(frame_rgbd_depth_copy(COEB_DEPTH_F32, 1.0001f) == 0 && frame_rgbd_depth_copy(COEB_DEPTH_F32, 0.0002f) == 0);
    CHECK(frame_rgbd_depth_copy(COEB_DEPTH_U16, 1.0f) == 0);
    CHECK(frame_rgbd_guess(1000, 2000) == 1000 && frame_rgbd_guess(1000, 7) == 7 && frame_rgbd_guess(1000, 0) == 0 &&
          frame_rgbd_guess(1000, -5) == 0);
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    puts("ok");
    return 0;
}
