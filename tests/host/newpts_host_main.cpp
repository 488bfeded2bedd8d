// The host half of coeb_kfdb_set_stereo / coeb_kfdb_create_new_map_points (csrc/coeb_kfdb_host.cpp: the
// stereo records, the argument rules, the unpacking of the downloaded rows) as a stand-alone program, built
// under ASan + UBSan by tests/test_newpts_host.py (no Python process, no GPU, no HIP).  Every buffer has
// exactly the size the rules promise, so a read or write past it is a heap overflow the sanitizer reports.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "coeb_front.h"
#include "coeb_kfdb_host.hpp"

#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } \
    } while (0)

static bool says(const char* msg, const char* part) { return msg && strstr(msg, part); }

static int stereo()
{
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<float> xy = {1.f, 2.f, 3.f, 4.f, 5.f, 6.f}, d = {2.5f, 0.f, -1.f};
    std::vector<KfdbStereo> out(3);
    std::vector<uint8_t> pos(3);
    CHECK(kfdb_pack_stereo(xy.data(), d.data(), 3, out.data(), pos.data()));
    for (int i = 0; i < 3; i++) CHECK(out[i].kx == xy[2 * i] && out[i].ky == xy[2 * i + 1] && out[i].depth == d[i]);
    CHECK(pos[0] == 1 && pos[1] == 0 && pos[2] == 0);
    CHECK(kfdb_pack_stereo(nullptr, nullptr, 0, nullptr, nullptr));
    d[2] = inf;
    CHECK(!kfdb_pack_stereo(xy.data(), d.data(), 3, out.data(), pos.data()));
    CHECK(kfdb_pack_stereo(xy.data(), d.data(), 2, out.data(), pos.data()));
    d[2] = 1.f; xy[3] = std::nanf("");
    CHECK(!kfdb_pack_stereo(xy.data(), d.data(), 3, out.data(), pos.data()));
    const std::vector<uint8_t> st = {1, 0, 1}, p1 = {1, 0, 1}, p2 = {1, 1, 0};
    CHECK(!kfdb_stereo_conflict(st.data(), p1.data(), 3) && kfdb_stereo_conflict(st.data(), p2.data(), 3));
    CHECK(!kfdb_stereo_conflict(st.data(), p2.data(), 2) && !kfdb_stereo_conflict(nullptr, nullptr, 0));
    return 0;
}

static coeb_kf_view a_view()
{
    coeb_kf_view v{};
    v.Rcw[0] = v.Rcw[4] = v.Rcw[8] = 1.f;
    v.fx = v.fy = 500.f; v.cx = 320.f; v.cy = 240.f; v.invfx = v.invfy = 0.002f; v.mb = 0.08f; v.mbf = 40.f;
    return v;
}

static int rules()
{
    // slots: 0 (3 features), 1 (no features), 2 (2 features, no stereo data), 3 empty, 4 (1 feature, a stereo
    // feature without depth), 5 (2 features), 6 (no geometry)
    const std::vector<uint8_t> used = {1, 1, 1, 0, 1, 1, 1}, geo = {1, 1, 1, 0, 1, 1, 0}, ste = {1, 1, 0, 0, 1, 1, 1},
                               bad = {0, 0, 0, 0, 1, 0, 0};
    const std::vector<int> n = {3, 0, 2, 0, 1, 2, 2};
    const std::vector<uint8_t> m0(3), m2(2), m4(1);
    const coeb_kf_view v1 = a_view();
    std::vector<coeb_kf_view> v2(3, a_view());
    std::vector<float> F(3 * 9), e(3 * 2), x3d(3 * 3 * 3);
    std::vector<int32_t> match(3 * 3), nm(3), first(3);
    std::vector<int8_t> status(3 * 3);
    std::vector<int32_t> slots = {5, 1, 5};
    std::vector<const uint8_t*> has = {m2.data(), nullptr, m2.data()};
    auto check = [&](int slot1, const coeb_kf_view* a, const uint8_t* h1, int nnb, const coeb_kf_view* b, const int8_t* st,
                     const float* x, const int32_t* f) {
        return kfdb_newpts_check(used.data(), geo.data(), ste.data(), bad.data(), n.data(), 7, slot1, a, h1, slots.data(), nnb,
                                 b, has.data(), F.data(), e.data(), match.data(), st, x, f, nm.data());
    };
    CHECK(!check(0, &v1, m0.data(), 2, v2.data(), status.data(), x3d.data(), first.data()));
    CHECK(!check(0, &v1, m0.data(), 0, nullptr, nullptr, nullptr, first.data()));                  // nnb == 0
    CHECK(!check(1, &v1, nullptr, 1, v2.data(), nullptr, nullptr, nullptr));                       // n1 == 0
    CHECK(says(check(0, &v1, m0.data(), 3, v2.data(), status.data(), x3d.data(), first.data()), "repeated"));
    CHECK(says(check(0, &v1, m0.data(), 33, v2.data(), status.data(), x3d.data(), first.data()), "0..32"));
    CHECK(says(check(3, &v1, m0.data(), 2, v2.data(), status.data(), x3d.data(), first.data()), "no keyframe"));
    CHECK(says(check(6, &v1, m2.data(), 2, v2.data(), status.data(), x3d.data(), first.data()), "geometry"));
    CHECK(says(check(2, &v1, m2.data(), 2, v2.data(), status.data(), x3d.data(), first.data()), "stereo data"));
    CHECK(says(check(4, &v1, m4.data(), 2, v2.data(), status.data(), x3d.data(), first.data()), "depth <= 0"));
    CHECK(says(check(0, nullptr, m0.data(), 2, v2.data(), status.data(), x3d.data(), first.data()), "missing"));
    CHECK(says(check(0, &v1, m0.data(), 2, nullptr, status.data(), x3d.data(), first.data()), "missing"));
    CHECK(says(check(0, &v1, m0.data(), 2, v2.data(), nullptr, x3d.data(), first.data()), "missing"));
    CHECK(says(check(0, &v1, m0.data(), 2, v2.data(), status.data(), nullptr, first.data()), "missing"));
    CHECK(says(check(0, &v1, m0.data(), 2, v2.data(), status.data(), x3d.data(), nullptr), "missing"));
    CHECK(says(check(5, &v1, m2.data(), 2, v2.data(), status.data(), x3d.data(), first.data()), "itself"));
    slots[0] = 2;
    CHECK(says(check(0, &v1, m0.data(), 2, v2.data(), status.data(), x3d.data(), first.data()), "stereo data"));
    slots[0] = 4; has[0] = m4.data();
    CHECK(says(check(0, &v1, m0.data(), 2, v2.data(), status.data(), x3d.data(), first.data()), "depth <= 0"));
    slots[0] = 5; has[0] = m2.data();
    // every entry of a view, not finite in turn
    for (size_t k = 0; k < sizeof(coeb_kf_view) / sizeof(float); k++) {
        coeb_kf_view w = a_view();
        reinterpret_cast<float*>(&w)[k] = k & 1 ? std::nanf("") : -std::numeric_limits<float>::infinity();
        CHECK(says(check(0, &w, m0.data(), 2, v2.data(), status.data(), x3d.data(), first.data()), "keyframe 1 is not finite"));
        v2[1] = w;
        CHECK(says(check(0, &v1, m0.data(), 2, v2.data(), status.data(), x3d.data(), first.data()), "neighbour is not finite"));
        v2[1] = a_view();
    }
    return 0;
}

static int unpacking()
{
    // 2 neighbours, 3 features
    const std::vector<int32_t> match = {4, -1, 0, -1, 2, 1}, first_dev = {0, INT_MAX, 1};
    const std::vector<int8_t> status = {(int8_t)(kNpAccepted | 16), 0, (int8_t)(kNpRatio | 32), 0, (int8_t)kNpLowParallax,
                                        (int8_t)(kNpAccepted | 48)};
    std::vector<float> dev(18);
    for (int k = 0; k < 18; k++) dev[k] = 100.f + k;
    std::vector<float> x3d(18, -7.f);
    std::vector<int32_t> first(3, 55), nm(2, 55);
    kfdb_newpts_unpack(match.data(), status.data(), dev.data(), first_dev.data(), 2, 3, x3d.data(), first.data(), nm.data());
    for (int e = 0; e < 6; e++)
        for (int k = 0; k < 3; k++) CHECK(x3d[3 * e + k] == ((e == 0 || e == 5) ? dev[3 * e + k] : -7.f));
    CHECK(first[0] == 0 && first[1] == -1 && first[2] == 1 && nm[0] == 2 && nm[1] == 2);
    kfdb_newpts_unpack(nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, nullptr);
    return 0;
}

int main()
{
    if (stereo() || rules() || unpacking()) return 1;
    printf("ok\n");
    return 0;
}
