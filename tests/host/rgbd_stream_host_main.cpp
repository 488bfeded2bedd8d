// The host part of coeb_rgbd_stream_frame (coeb-slam_amd/csrc/coeb_rgbd_stream_host.hpp: argument
// checks, the page-locked layout of one call, the slot layout of the stream's device memory, the
// slot arithmetic) run without a device, built with ASan + UBSan by tests/test_rgbd_stream_host.py.
// Exit status 0 and "ok" on stdout: every check held.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "coeb_rgbd_stream_host.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            g_fail++;                                                    \
        }                                                                \
    } while (0)

struct Region { const char* name; size_t off, bytes; };

static void check_regions(const Region* r, int nr, size_t total)
{
    for (int i = 0; i < nr; i++) {
        CHECK(r[i].off % 256 == 0);
        CHECK(r[i].off + r[i].bytes <= total);
        if (i + 1 < nr) CHECK(r[i].off + r[i].bytes <= r[i + 1].off);   // in order, no overlap
    }
}

// one call's page-locked layout and the staging writes into a buffer of exactly `total` bytes
static void check_layout(int W, int H, int ch, int kcap, int nbox, int dtype)
{
    const RgbdStreamLayout L = rgbd_stream_layout(W, H, ch, kcap, dtype);
    const size_t k = (size_t)kcap, db = dtype == COEB_DEPTH_F32 ? 4 : 2;
    const Region r[] = {
        {"hdr", L.o_hdr, sizeof(RgbdStreamHdr)}, {"img", L.o_img, (size_t)W * H * ch}, {"n+err", L.o_n, 20},
        {"kps", L.o_k, k * 28},                  {"desc", L.o_d, k * 32},              {"kps_un", L.o_kun, k * 28},
        {"ur", L.o_ur, k * 4},                   {"dep", L.o_dep, k * 4},              {"gray", L.o_gray, (size_t)W * H},
        {"res", L.o_res, sizeof(RgbdStreamRes)}, {"depth", L.o_depth, (size_t)W * H * db},
    };
    check_regions(r, (int)(sizeof r / sizeof r[0]), L.total);
    CHECK(L.up_bytes == L.o_img + (size_t)W * H * ch && L.img_row == (size_t)W * ch && L.depth_row == (size_t)W * db);
    // the copy back: gray and the result block as far apart as in the slot
    const RgbdStreamSlot S = rgbd_stream_slot(W, H);
    CHECK(L.o_res - L.o_gray == S.s_res - S.s_gray);
    // a 1-channel upload lands on the slot's head and gray level in one piece
    CHECK(L.o_img - L.o_hdr == S.s_gray - S.s_hdr);
    CHECK(nbox <= COEB_MAX_BOXES ? sizeof(coeb_box) * (size_t)nbox <= sizeof(RgbdStreamHdr::box) : true);

    std::vector<uint8_t> pin(L.total, 0xEE);
    const size_t is = L.img_row + 7, ds = L.depth_row + 6;
    std::vector<uint8_t> img(is * H, 0xAA), dep(ds * H, 0xBB);
    for (int y = 0; y < H; y++) {
        for (size_t x = 0; x < L.img_row; x++) img[y * is + x] = (uint8_t)(x + 3 * y);
        for (size_t b = 0; b < L.depth_row; b++) dep[y * ds + b] = (uint8_t)(b + 5 * y);
    }
    RgbdStreamHdr* hdr = reinterpret_cast<RgbdStreamHdr*>(pin.data() + L.o_hdr);
    memset(hdr, 0, sizeof(*hdr));
    // the head holds COEB_MAX_BOXES boxes: a count past it (64) is refused by the check (check_args) and never written
    hdr->box_off[1] = nbox <= COEB_MAX_BOXES ? nbox : 0;
    for (int i = 0; i < hdr->box_off[1]; i++) hdr->box[i] = coeb_box{(float)i, 1.f, 2.f, 3.f};
    single_frame_stage_rows(pin.data() + L.o_img, img.data(), H, L.img_row, is);
    single_frame_stage_rows(pin.data() + L.o_depth, dep.data(), H, L.depth_row, ds);
    bool ok = true;
    for (int y = 0; y < H && ok; y++) {
        for (size_t x = 0; x < L.img_row; x++) ok = ok && pin[L.o_img + (size_t)y * L.img_row + x] == (uint8_t)(x + 3 * y);
        for (size_t b = 0; b < L.depth_row; b++) ok = ok && pin[L.o_depth + y * L.depth_row + b] == (uint8_t)(b + 5 * y);
    }
    CHECK(ok);
    for (size_t i = L.up_bytes; i < L.o_n; i++) ok = ok && pin[i] == 0xEE;      // strides' padding never arrives
    for (size_t i = L.o_depth + L.depth_row * H; i < L.total; i++) ok = ok && pin[i] == 0xEE;
    CHECK(ok);
}

static void check_slot(int W, int H)
{
    const RgbdStreamSlot S = rgbd_stream_slot(W, H);
    CHECK(S.L >= 1 && S.L <= kStreamLkLevels && S.L == rgbd_stream_lk_levels(W, H));
    std::vector<Region> r;
    r.push_back({"hdr", S.s_hdr, sizeof(RgbdStreamHdr)});
    r.push_back({"gray", S.s_gray, (size_t)W * H});
    r.push_back({"res", S.s_res, sizeof(RgbdStreamRes)});
    CHECK(S.lw[0] == W && S.lh[0] == H);
    for (int l = 1; l < S.L; l++) {
        CHECK(S.lw[l] == (S.lw[l - 1] + 1) / 2 && S.lh[l] == (S.lh[l - 1] + 1) / 2);
        r.push_back({"lvl", S.s_lvl[l], (size_t)S.lw[l] * S.lh[l]});
    }
    // every level above the last still has both sides longer than the LK window (the pyramid's stop rule)
    for (int l = 1; l + 1 < S.L; l++) CHECK(S.lw[l] > kStreamLkWin && S.lh[l] > kStreamLkWin);
    for (int l = 0; l < S.L; l++) r.push_back({"der", S.s_der[l], (size_t)S.lw[l] * S.lh[l] * 4});
    r.push_back({"pts", S.s_pts, (size_t)kStreamTmCap * 8});
    r.push_back({"npts", S.s_npts, 4});
    check_regions(r.data(), (int)r.size(), S.bytes);
}

static void check_args()
{
    std::vector<uint8_t> img(64 * 64 * 4, 0);
    std::vector<float> depth(64 * 64, 1.f);
    uint8_t desc[32], gray[64 * 64];
    float ur[1], dd[1], tm[2];
    int32_t flags[COEB_MAX_BOXES];
    coeb_keypoint kp[1];
    coeb_box box[COEB_MAX_BOXES] = {};
    const coeb_camera cam{500, 500, 32, 32, 40, 0, 64, 0, 64};
    const char* why = nullptr;
    auto good = [&]() {
        coeb_rgbd_stream_out o{};
        o.tm_xy = tm; o.tm_cap = 1; o.blur_flag = flags; o.kp = kp; o.desc = desc; o.u_right = ur; o.depth = dd; o.cap = 1;
        return o;
    };
    auto run = [&](const uint8_t* im, size_t istride, int ch, int W, int H, const void* dp, size_t dstride, int dtype,
                   const coeb_camera* c, const coeb_box* b, int nbox, const coeb_rgbd_stream_out* o, int pw, int ph) {
        return rgbd_stream_check(im, istride, ch, W, H, dp, dstride, dtype, c, b, nbox, o, pw, ph, &why);
    };
    coeb_rgbd_stream_out o = good();
    // the good call: every channel count, both depth types, boxes 0 / 1 / the most, strided rows, with and without a predecessor
    for (int ch : {1, 3, 4})
        for (int nbox : {0, 1, COEB_MAX_BOXES}) {
            CHECK(run(img.data(), 64 * ch, ch, 64, 64, depth.data(), 256, COEB_DEPTH_F32, &cam, box, nbox, &o, 0, 0) == 0);
            CHECK(run(img.data(), 64 * ch + 5, ch, 48, 48, depth.data(), 100, COEB_DEPTH_U16, &cam, box, nbox, &o, 48, 48) == 0);
        }
    CHECK(run(img.data(), 64, 1, 64, 64, depth.data(), 256, COEB_DEPTH_F32, &cam, nullptr, 0, &o, 0, 0) == 0);
    o.gray = gray; o.gray_stride = 64;
    CHECK(run(img.data(), 64, 1, 64, 64, depth.data(), 256, COEB_DEPTH_F32, &cam, nullptr, 0, &o, 0, 0) == 0);
    o.gray_stride = 63;
    CHECK(run(img.data(), 64, 1, 64, 64, depth.data(), 256, COEB_DEPTH_F32, &cam, nullptr, 0, &o, 0, 0) == COEB_EINVAL);
    o = good();
    // no output struct, then the empty image whatever else is wrong
    CHECK(run(img.data(), 64, 1, 64, 64, depth.data(), 256, COEB_DEPTH_F32, &cam, nullptr, 0, nullptr, 0, 0) == COEB_EINVAL);
    CHECK(run(nullptr, 0, 7, 64, 64, nullptr, 0, 9, nullptr, nullptr, -1, &o, 5, 5) == 1);
    CHECK(run(img.data(), 64, 1, 0, 64, depth.data(), 256, COEB_DEPTH_F32, &cam, nullptr, 0, &o, 0, 0) == 1);
    CHECK(run(img.data(), 64, 1, 64, -2, depth.data(), 256, COEB_DEPTH_F32, &cam, nullptr, 0, &o, 0, 0) == 1);
    // the image
    CHECK(run(img.data(), 64, 2, 64, 64, depth.data(), 256, COEB_DEPTH_F32, &cam, nullptr, 0, &o, 0, 0) == COEB_EINVAL);
    CHECK(run(img.data(), 191, 3, 64, 64, depth.data(), 256, COEB_DEPTH_F32, &cam, nullptr, 0, &o, 0, 0) == COEB_EINVAL);
    CHECK(run(img.data(), 31, 1, 31, 64, depth.data(), 256, COEB_DEPTH_F32, &cam, nullptr, 0, &o, 0, 0) == COEB_EINVAL);
    CHECK(run(img.data(), 64, 1, 64, 31, depth.data(), 256, COEB_DEPTH_F32, &cam, nullptr, 0, &o, 0, 0) == COEB_EINVAL);
    // the boxes: more than COEB_MAX_BOXES (64 among them) is refused, never laid out
    CHECK(run(img.data(), 64, 1, 64, 64, depth.data(), 256, COEB_DEPTH_F32, &cam, box, -1, &o, 0, 0) == COEB_EINVAL);
    CHECK(run(img.data(), 64, 1, 64, 64, depth.data(), 256, COEB_DEPTH_F32, &cam, box, COEB_MAX_BOXES + 1, &o, 0, 0) == COEB_EINVAL);
    CHECK(run(img.data(), 64, 1, 64, 64, depth.data(), 256, COEB_DEPTH_F32, &cam, box, 64, &o, 0, 0) == COEB_EINVAL);
    CHECK(run(img.data(), 64, 1, 64, 64, depth.data(), 256, COEB_DEPTH_F32, &cam, nullptr, 1, &o, 0, 0) == COEB_EINVAL);
    // the depth map and the camera
    CHECK(run(img.data(), 64, 1, 64, 64, nullptr, 256, COEB_DEPTH_F32, &cam, nullptr, 0, &o, 0, 0) == COEB_EINVAL);
    CHECK(run(img.data(), 64, 1, 64, 64, depth.data(), 255, COEB_DEPTH_F32, &cam, nullptr, 0, &o, 0, 0) == COEB_EINVAL);
    CHECK(run(img.data(), 64, 1, 64, 64, depth.data(), 127, COEB_DEPTH_U16, &cam, nullptr, 0, &o, 0, 0) == COEB_EINVAL);
    CHECK(run(img.data(), 64, 1, 64, 64, depth.data(), 256, 2, &cam, nullptr, 0, &o, 0, 0) == COEB_EINVAL);
    CHECK(run(img.data(), 64, 1, 64, 64, depth.data(), 256, COEB_DEPTH_F32, nullptr, nullptr, 0, &o, 0, 0) == COEB_EINVAL);
    // the outputs
    for (int miss = 0; miss < 6; miss++) {
        coeb_rgbd_stream_out q = good();
        if (miss == 0) q.kp = nullptr;
        if (miss == 1) q.desc = nullptr;
        if (miss == 2) q.u_right = nullptr;
        if (miss == 3) q.depth = nullptr;
        if (miss == 4) q.tm_xy = nullptr;
        if (miss == 5) q.tm_cap = -1;
        CHECK(run(img.data(), 64, 1, 64, 64, depth.data(), 256, COEB_DEPTH_F32, &cam, nullptr, 0, &q, 0, 0) == COEB_EINVAL);
    }
    {
        coeb_rgbd_stream_out q = good();
        q.tm_xy = nullptr; q.tm_cap = 0; q.kp_un = nullptr;             // T_M not wanted, kp_un optional
        CHECK(run(img.data(), 64, 1, 64, 64, depth.data(), 256, COEB_DEPTH_F32, &cam, nullptr, 0, &q, 0, 0) == 0);
        q.blur_flag = nullptr;                                           // flags are required once there are boxes
        CHECK(run(img.data(), 64, 1, 64, 64, depth.data(), 256, COEB_DEPTH_F32, &cam, nullptr, 0, &q, 0, 0) == 0);
        CHECK(run(img.data(), 64, 1, 64, 64, depth.data(), 256, COEB_DEPTH_F32, &cam, box, 1, &q, 0, 0) == COEB_EINVAL);
    }
    // a size change needs a reset
    CHECK(run(img.data(), 64, 1, 64, 64, depth.data(), 256, COEB_DEPTH_F32, &cam, nullptr, 0, &o, 64, 48) == COEB_EINVAL);
    CHECK(run(img.data(), 64, 1, 64, 64, depth.data(), 256, COEB_DEPTH_F32, &cam, nullptr, 0, &o, 48, 64) == COEB_EINVAL);
    CHECK(why && why[0]);
}

int main()
{
    const int sizes[][3] = {{32, 32, 1}, {333, 251, 3}, {640, 480, 1}, {640, 480, 4}, {1280, 960, 1}, {1280, 960, 3}, {33, 47, 4}};
    for (const auto& s : sizes) {
        check_slot(s[0], s[1]);
        for (int kcap : {0, 9, 2744})
            for (int nbox : {0, 1, COEB_MAX_BOXES, 64})
                for (int dtype : {COEB_DEPTH_U16, COEB_DEPTH_F32}) check_layout(s[0], s[1], s[2], kcap, nbox, dtype);
    }
    check_args();
    // LK level counts (calcOpticalFlowPyrLK, window 22, maxLevel 5): the pyramid stops once a side reaches the window
    CHECK(rgbd_stream_lk_levels(640, 480) == 5 && rgbd_stream_lk_levels(1280, 960) == 6 && rgbd_stream_lk_levels(32, 32) == 1);
    CHECK(rgbd_stream_lk_levels(160, 120) == 3 && rgbd_stream_lk_levels(333, 251) == 4);
    // slot arithmetic: consecutive frames alternate, whatever the count
    for (uint64_t q : {(uint64_t)0, (uint64_t)1, (uint64_t)2, (uint64_t)0xFFFFFFFFull, ~(uint64_t)0})
        CHECK(rgbd_stream_slot_of(q) != rgbd_stream_slot_of(q + 1) && (rgbd_stream_slot_of(q) | 1) == 1);
    CHECK(rgbd_stream_tm_count(-1, 10) == 0 && rgbd_stream_tm_count(5, 10) == 5 && rgbd_stream_tm_count(50, 10) == 10 &&
          rgbd_stream_tm_count(3, 0) == 0);
    CHECK(sizeof(RgbdStreamRes) <= kStreamResBytes && sizeof(RgbdStreamHdr) <= kStreamHdrBytes);
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    puts("ok");
    return 0;
}
