// The single-frame drop-in path with and without coeb_frame_rgbd, on the same frames in one
// process, driven from C++ as the reference's Tracking thread drives it (tools/single_frame_c.cpp
// is pattern (a) alone).  Per frame i, matched against frame i-1:
//   (a) coeb_extract + coeb_stereo_from_rgbd + coeb_match_lastframe
//   (b) coeb_extract + coeb_undistort_keypoints + coeb_stereo_from_rgbd + coeb_match_lastframe
//       (TUM1 distortion; the stereo call gets the raw keys, as INTEGRATION.md s4b had it)
//   (c) coeb_frame_rgbd (no distortion) + coeb_match_lastframe
//   (c_dist) the same with the TUM1 distortion: what (b) costs when mvuRight is also right
// The match is TrackWithMotionModel's SearchByProjection th 15, retried at 30 below 20 matches
// (Tracking.cc:947-958).  The LastFrame MapPoint arrays are Tracking state built outside the
// timed calls.
//
// usage: frame_rgbd_c <frames.u8> <W> <H> <N> [warm]   (N frames of W*H gray bytes; depth 2 m)
// prints one JSON line: per pattern the median / min / max ms per frame over the N - 1 - warm
// timed frames, and the median / min match count.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "coeb_front.h"

static double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

static double median(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    return v.empty() ? 0.0 : v[v.size() / 2];
}

int main(int argc, char** argv)
{
    if (argc < 5) {
        fprintf(stderr, "usage: %s frames.u8 W H N [warm]\n", argv[0]);
        return 2;
    }
    const int W = atoi(argv[2]), H = atoi(argv[3]), N = atoi(argv[4]), warm = argc > 5 ? atoi(argv[5]) : 5;
    std::vector<uint8_t> frames((size_t)N * W * H);
    FILE* f = fopen(argv[1], "rb");
    if (!f || fread(frames.data(), 1, frames.size(), f) != frames.size()) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    fclose(f);
    const float fx = 535.4f, fy = 539.2f, cx = 320.1f, cy = 247.6f, bf = 40.0f, z = 2.0f;
    const float tum1[5] = {0.262383f, -0.953104f, -0.005358f, 0.002628f, 1.163314f};
    std::vector<float> depth((size_t)W * H, z);
    coeb_orb_params p{1000, 1.2f, 8, 20, 7};
    coeb_ctx* ctx = coeb_create(&p, 0, W, H, 1);
    if (!ctx) {
        fprintf(stderr, "coeb_create: %s\n", coeb_last_error(nullptr));
        return 1;
    }
    const int cap = coeb_max_keypoints(ctx, W, H);
    const coeb_camera cam{fx, fy, cx, cy, bf, 0.f, (float)W, 0.f, (float)H};
    float Tc[16] = {1, 0, 0, 2.f * z / fx, 0, 1, 0, 1.f * z / fy, 0, 0, 1, 0, 0, 0, 0, 1};   // synth.motion_pose
    float Tl[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    struct Fr { std::vector<coeb_keypoint> k, ku; std::vector<uint8_t> d; std::vector<float> ur, dep; int n = 0; };
    Fr cur, prev;
    for (Fr* x : {&cur, &prev}) {
        x->k.resize(cap); x->ku.resize(cap); x->d.resize((size_t)cap * 32); x->ur.resize(cap); x->dep.resize(cap);
    }
    std::vector<uint8_t> has(cap), outl(cap, 0);
    std::vector<float> xw((size_t)cap * 3);
    std::vector<int32_t> nobs(cap, 2), match(cap);
    auto check = [&](int rc, const char* what) {
        if (rc != COEB_OK) {
            fprintf(stderr, "%s: %s\n", what, coeb_last_error(ctx));
            exit(1);
        }
    };
    enum Pattern { A, B, C, C_DIST, NPAT };
    // the Frame constructor's tail of one frame; x.ku = mvKeysUn
    auto frame = [&](Pattern pat, Fr& x, int i) {
        const uint8_t* g = frames.data() + (size_t)i * W * H;
        if (pat == C || pat == C_DIST) {
            check(coeb_frame_rgbd(ctx, g, W, H, W, depth.data(), (size_t)W * 4, COEB_DEPTH_F32, 1.0f, &cam,
                                  pat == C_DIST ? tum1 : nullptr, nullptr, 0, nullptr, 0, nullptr, 0, x.k.data(), x.ku.data(),
                                  x.d.data(), x.ur.data(), x.dep.data(), cap, &x.n), "coeb_frame_rgbd");
            return;
        }
        check(coeb_extract(ctx, g, W, H, W, nullptr, 0, nullptr, 0, nullptr, 0, x.k.data(), x.d.data(), cap, &x.n),
              "coeb_extract");
        if (pat == B) check(coeb_undistort_keypoints(ctx, &cam, tum1, x.k.data(), x.n, x.ku.data()), "coeb_undistort_keypoints");
        check(coeb_stereo_from_rgbd(ctx, x.k.data(), x.n, depth.data(), W, H, W, bf, x.ur.data(), x.dep.data()),
              "coeb_stereo_from_rgbd");
    };
    struct Stat { double med, lo, hi; int nm, nm_min; size_t frames; };
    Stat st[NPAT];
    for (int pat = 0; pat < NPAT; pat++) {
        const bool undist = pat == B || pat == C_DIST;
        frame((Pattern)pat, prev, 0);
        std::vector<double> tot, nms;
        for (int i = 1; i < N; i++) {
            // LastFrame MapPoints of frame i-1 (untimed: Tracking state)
            const std::vector<coeb_keypoint>& pk = (undist || pat == C) ? prev.ku : prev.k;
            for (int k = 0; k < prev.n; k++) {
                const float d = prev.dep[k];
                has[k] = d > 0;
                xw[3 * k] = (pk[k].x - cx) * d / fx;
                xw[3 * k + 1] = (pk[k].y - cy) * d / fy;
                xw[3 * k + 2] = d;
            }
            const coeb_lastframe last{prev.n, has.data(), outl.data(), xw.data(), prev.d.data(), nobs.data(), pk.data()};
            const double t0 = now_ms();
            frame((Pattern)pat, cur, i);
            const coeb_curframe cf{cur.n, (undist || pat == C) ? cur.ku.data() : cur.k.data(), cur.d.data(), cur.ur.data()};
            int nm = 0;
            check(coeb_match_lastframe(ctx, &cam, &cf, &last, Tc, Tl, 15.f, 0, 1, match.data(), &nm), "coeb_match_lastframe");
            if (nm < 20) check(coeb_match_lastframe(ctx, &cam, &cf, &last, Tc, Tl, 30.f, 0, 1, match.data(), &nm),
                               "coeb_match_lastframe");
            const double t1 = now_ms();
            if (i > warm) { tot.push_back(t1 - t0); nms.push_back(nm); }
            std::swap(cur, prev);
        }
        st[pat].med = median(tot);
        st[pat].lo = tot.empty() ? 0.0 : *std::min_element(tot.begin(), tot.end());
        st[pat].hi = tot.empty() ? 0.0 : *std::max_element(tot.begin(), tot.end());
        st[pat].nm = (int)median(nms);
        st[pat].nm_min = nms.empty() ? 0 : (int)*std::min_element(nms.begin(), nms.end());
        st[pat].frames = tot.size();
    }
    coeb_destroy(ctx);
    static const char* const names[NPAT] = {"a_extract_stereo_match", "b_extract_undistort_stereo_match",
                                            "c_frame_rgbd_match", "c_dist_frame_rgbd_match"};
    std::string out = "{";
    for (int pat = 0; pat < NPAT; pat++) {
        char buf[256];
        snprintf(buf, sizeof buf, "%s\"%s\": {\"ms_median\": %.4f, \"ms_min\": %.4f, \"ms_max\": %.4f, \"matches\": %d, "
                 "\"min_matches\": %d}", pat ? ", " : "", names[pat], st[pat].med, st[pat].lo, st[pat].hi, st[pat].nm,
                 st[pat].nm_min);
        out += buf;
    }
    char buf[96];
    snprintf(buf, sizeof buf, ", \"frames\": %zu, \"warm\": %d, \"width\": %d, \"height\": %d}", st[0].frames, warm, W, H);
    out += buf;
    puts(out.c_str());
    return 0;
}
