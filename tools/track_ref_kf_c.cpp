// Tracking::TrackReferenceKeyFrame on one host frame as the C++ Tracking thread would drive it:
// the fused coeb_track_reference_keyframe against the composition it replaces
// (coeb_bow_transform -> coeb_match_bow -> host gather -> coeb_pose_optimization -> host discard
// loop), on the scene tools/trk_time.py writes.  Both are timed after a warm-up, each call on its
// own with the device otherwise idle; the results of the two must agree.  The fused call's
// per-kernel device time comes from coeb_profile_read over a separate run of calls.
//
// usage: track_ref_kf_c DIR [calls] [warm]
//   DIR: voc.txt, meta.i32 (levelsup), cam.f32 (fx fy cx cy bf W H), T.f32, kps.bin, desc.u8, ur.f32,
//        k_valid.u8, k_desc.u8, k_node.i32, k_angle.f32, k_xw.f32, k_obs.i32
// prints one JSON line.  With -DCOEB_TIME_COMPOSED_ONLY the fused entry point is not referenced,
// so the program links against a library built before it existed.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "coeb_front.h"

static double now_us()
{
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

template <class T>
static std::vector<T> load(const std::string& path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) { fprintf(stderr, "missing %s\n", path.c_str()); exit(2); }
    std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    std::vector<T> v(raw.size() / sizeof(T));
    if (!v.empty()) memcpy(v.data(), raw.data(), v.size() * sizeof(T));
    return v;
}

struct Stats { double med, p10, p90, min; };
static Stats stats(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    const size_t n = v.size();
    return Stats{v[n / 2], v[n / 10], v[(9 * n) / 10], v[0]};
}

struct Result {
    std::vector<int32_t> match, disc;
    float T[16];
    int nmb = 0, nin = 0, nm = 0, nmap = 0;
    bool operator==(const Result& o) const
    {
        return match == o.match && disc == o.disc && !memcmp(T, o.T, 64) && nmb == o.nmb && nin == o.nin && nm == o.nm &&
               nmap == o.nmap;
    }
};

#define CHECK(expr)                                                                       \
    do {                                                                                  \
        if ((expr) != COEB_OK) { fprintf(stderr, "%s: %s\n", #expr, coeb_last_error(ctx)); return 1; } \
    } while (0)

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s DIR [calls] [warm]\n", argv[0]); return 2; }
    const std::string d = std::string(argv[1]) + "/";
    const int calls = argc > 2 ? atoi(argv[2]) : 300, warm = argc > 3 ? atoi(argv[3]) : 30;
    const std::vector<char> voc_text = load<char>(d + "voc.txt");
    const int levelsup = load<int32_t>(d + "meta.i32")[0];
    const std::vector<float> cm = load<float>(d + "cam.f32"), T0 = load<float>(d + "T.f32");
    const std::vector<coeb_keypoint> kps = load<coeb_keypoint>(d + "kps.bin");
    const std::vector<uint8_t> desc = load<uint8_t>(d + "desc.u8"), kvalid = load<uint8_t>(d + "k_valid.u8");
    const std::vector<uint8_t> kdesc = load<uint8_t>(d + "k_desc.u8");
    const std::vector<float> ur = load<float>(d + "ur.f32"), kang = load<float>(d + "k_angle.f32"), kxw = load<float>(d + "k_xw.f32");
    const std::vector<int32_t> knode = load<int32_t>(d + "k_node.i32"), kobs = load<int32_t>(d + "k_obs.i32");
    const int n = (int)kps.size(), nq = (int)kvalid.size();
    coeb_orb_params p{1000, 1.2f, 8, 20, 7};
    coeb_ctx* ctx = coeb_create(&p, 0, 640, 480, 1);
    if (!ctx) { fprintf(stderr, "coeb_create: %s\n", coeb_last_error(nullptr)); return 1; }
    coeb_voc* voc = nullptr;
    CHECK(coeb_voc_from_text(voc_text.data(), voc_text.size(), &voc));
    CHECK(coeb_bow_set_vocabulary(ctx, voc));
    const coeb_camera cam{cm[0], cm[1], cm[2], cm[3], cm[4], 0.f, cm[5], 0.f, cm[6]};
    const coeb_curframe cur{n, kps.data(), desc.data(), ur.data()};
    const coeb_bow_keyframe bkf{nq, kvalid.data(), kdesc.data(), knode.data(), kang.data()};
    const float nnratio = 0.7f;
    const int min_matches = 15;
    std::vector<int32_t> word(n), node(n);
    std::vector<double> weight(n);

    // the composition: three uploads, three downloads, three synchronisations and the host steps between
    std::vector<float> angle(n), xw((size_t)n * 3);
    std::vector<uint8_t> has(n), outl(n);
    auto composed = [&](Result& r) -> int {
        r.match.assign(n, -1);
        r.disc.assign(n, -1);
        memcpy(r.T, T0.data(), 64);
        r.nin = r.nmap = 0;
        CHECK(coeb_bow_transform(ctx, desc.data(), n, levelsup, word.data(), node.data(), weight.data(), nullptr, nullptr,
                                 nullptr, 0, nullptr));
        for (int i = 0; i < n; i++) angle[i] = kps[i].angle;
        const coeb_bow_frame bf{n, desc.data(), node.data(), angle.data()};
        CHECK(coeb_match_bow(ctx, &bkf, &bf, nnratio, 1, r.match.data(), &r.nmb));
        r.nm = r.nmb;
        if (r.nmb < min_matches) return 0;
        for (int i = 0; i < n; i++) {
            has[i] = r.match[i] >= 0;
            if (has[i]) memcpy(&xw[3 * (size_t)i], &kxw[3 * (size_t)r.match[i]], 12);
        }
        const coeb_pose_frame pf{n, has.data(), xw.data(), kps.data(), ur.data()};
        CHECK(coeb_pose_optimization(ctx, &cam, &pf, r.T, outl.data(), &r.nin));
        for (int i = 0; i < n; i++) {               // Tracking.cc:843-862
            if (r.match[i] < 0) continue;
            if (outl[i]) { r.disc[i] = r.match[i]; r.match[i] = -1; r.nm--; }
            else if (kobs[r.match[i]] > 0) r.nmap++;
        }
        return 0;
    };
    Result rc;
    std::vector<double> tc;
    for (int it = 0; it < warm + calls; it++) {
        const double t0 = now_us();
        if (composed(rc)) return 1;
        if (it >= warm) tc.push_back(now_us() - t0);
    }
    const Stats sc = stats(tc);
    printf("{\"n_cur\": %d, \"n_kf\": %d, \"calls\": %d, \"warm\": %d, \"nmatches_bow\": %d, \"ninliers_pose\": %d, "
           "\"nmatches\": %d, \"nmatches_map\": %d, \"composed_us\": {\"median\": %.1f, \"p10\": %.1f, \"p90\": %.1f, \"min\": %.1f}",
           n, nq, calls, warm, rc.nmb, rc.nin, rc.nm, rc.nmap, sc.med, sc.p10, sc.p90, sc.min);
#ifndef COEB_TIME_COMPOSED_ONLY
    const coeb_ref_keyframe rkf{bkf, kxw.data(), kobs.data()};
    auto fused = [&](Result& r) -> int {
        r.match.assign(n, -1);
        r.disc.assign(n, -1);
        memcpy(r.T, T0.data(), 64);
        CHECK(coeb_track_reference_keyframe(ctx, &cam, &cur, nullptr, levelsup, &rkf, r.T, nnratio, 1, min_matches,
                                            word.data(), node.data(), weight.data(), r.match.data(), r.disc.data(), &r.nmb,
                                            &r.nin, &r.nm, &r.nmap));
        return 0;
    };
    Result rf;
    std::vector<double> tf;
    for (int it = 0; it < warm + calls; it++) {
        const double t0 = now_us();
        if (fused(rf)) return 1;
        if (it >= warm) tf.push_back(now_us() - t0);
    }
    const Stats sf = stats(tf);
    printf(", \"fused_us\": {\"median\": %.1f, \"p10\": %.1f, \"p90\": %.1f, \"min\": %.1f}, \"same_results\": %s", sf.med,
           sf.p10, sf.p90, sf.min, rf == rc ? "true" : "false");
    // per-kernel device time of the fused call (the events serialise the launches: not part of the timing above)
    CHECK(coeb_profile_enable(ctx, 1));
    CHECK(coeb_profile_reset(ctx));
    const int pcalls = 50;
    for (int it = 0; it < pcalls; it++)
        if (fused(rf)) return 1;
    char names[4096];
    double ms[64];
    int64_t launches[64];
    int nk = 0;
    CHECK(coeb_profile_read(ctx, names, sizeof(names), ms, launches, 64, &nk));
    printf(", \"fused_kernels_us\": {");
    int k = 0;
    bool first = true;
    for (char* tok = strtok(names, ","); tok && k < nk; tok = strtok(nullptr, ","), k++) {
        if (!launches[k]) continue;
        printf("%s\"%s\": %.2f", first ? "" : ", ", tok, 1000.0 * ms[k] / (double)launches[k]);
        first = false;
    }
    printf("}");
    CHECK(coeb_profile_enable(ctx, 0));
    if (!(rf == rc)) { printf("}\n"); fprintf(stderr, "fused and composed results differ\n"); return 1; }
#else
    (void)cur;
#endif
    printf("}\n");
    coeb_voc_destroy(voc);
    coeb_destroy(ctx);
    return 0;
}
