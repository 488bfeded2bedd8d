// The host half of coeb_kfdb_fuse_search (csrc/coeb_kfdb_host.cpp: the argument rules, the job
// table, the packed skip bytes and the list of grids to build) as a stand-alone program, built under
// ASan + UBSan by tests/test_fuse_host.py (no Python process, no GPU, no HIP).  Every buffer has exactly
// the size the rules promise, so a read or write past it is a heap overflow the sanitizer reports.
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

struct Points {
    std::vector<uint8_t> valid, desc;
    std::vector<float> pos, nrm, maxd, mind;
    coeb_fuse_points c;
    explicit Points(int n) : valid((size_t)n, 1), desc((size_t)n * 32, 0), pos((size_t)n * 3, 1.f), nrm((size_t)n * 3, 0.5f),
                             maxd((size_t)n, 4.f), mind((size_t)n, 1.f)
    {
        c = coeb_fuse_points{n, valid.data(), pos.data(), nrm.data(), maxd.data(), mind.data(), desc.data()};
    }
};

static coeb_fuse_job make_job(int slot, int first, int count, const uint8_t* skip)
{
    coeb_fuse_job j;
    memset(&j, 0, sizeof(j));
    j.slot = slot; j.first = first; j.count = count; j.skip = skip;
    j.Rcw[0] = j.Rcw[4] = j.Rcw[8] = 1.f;
    j.tcw[0] = 0.25f * slot;
    j.Ow[0] = -0.25f * slot;
    return j;
}

static int rules()
{
    const uint8_t used[4] = {1, 1, 0, 1}, geo[4] = {1, 1, 0, 0};
    const coeb_camera cam{500.f, 500.f, 320.f, 240.f, 40.f, 0.f, 640.f, 0.f, 480.f};
    Points p(7);
    std::vector<int32_t> bi(7 + 3), bd(7 + 3);
    std::vector<uint8_t> skip(3, 0);
    std::vector<coeb_fuse_job> jobs{make_job(0, 0, 7, nullptr), make_job(1, 4, 3, skip.data())};
    int code = 1;
    int64_t total = -1;
    const auto chk = [&](const coeb_camera* cm, const coeb_fuse_points* pp, const coeb_fuse_job* jj, int nj, float th) {
        return kfdb_fuse_check(used, geo, 4, cm, pp, jj, nj, th, bi.data(), bd.data(), &code, &total);
    };
    CHECK(!chk(&cam, &p.c, jobs.data(), 2, 3.f) && code == COEB_OK && total == 10);
    CHECK(!chk(&cam, &p.c, nullptr, 0, 3.f) && total == 0);
    CHECK(says(chk(nullptr, &p.c, jobs.data(), 2, 3.f), "missing") && code == COEB_EINVAL);
    CHECK(says(chk(&cam, nullptr, jobs.data(), 2, 3.f), "missing"));
    CHECK(says(chk(&cam, &p.c, nullptr, 2, 3.f), "missing job"));
    CHECK(says(chk(&cam, &p.c, jobs.data(), -1, 3.f), "0..128"));
    CHECK(says(chk(&cam, &p.c, jobs.data(), 129, 3.f), "0..128"));
    CHECK(says(chk(&cam, &p.c, jobs.data(), 2, -1.f), "th"));
    CHECK(says(chk(&cam, &p.c, jobs.data(), 2, std::numeric_limits<float>::quiet_NaN()), "th"));
    CHECK(says(kfdb_fuse_check(used, geo, 4, &cam, &p.c, jobs.data(), 2, 3.f, nullptr, bd.data(), &code, &total), "output"));
    {
        coeb_camera c2 = cam;
        c2.max_x = c2.min_x;
        CHECK(says(chk(&c2, &p.c, jobs.data(), 2, 3.f), "bounds"));
        c2 = cam;
        c2.min_y = std::numeric_limits<float>::infinity();
        CHECK(says(chk(&c2, &p.c, jobs.data(), 2, 3.f), "bounds"));
    }
    for (const int slot : {-1, 2, 4}) {
        std::vector<coeb_fuse_job> j{make_job(slot, 0, 1, nullptr)};
        CHECK(says(chk(&cam, &p.c, j.data(), 1, 3.f), "no keyframe"));
    }
    {
        std::vector<coeb_fuse_job> j{make_job(3, 0, 1, nullptr)};
        CHECK(says(chk(&cam, &p.c, j.data(), 1, 3.f), "geometry"));
    }
    const int bad_range[][2] = {{0, 8}, {7, 1}, {-1, 2}, {2, -1}, {0x7fffffff, 0x7fffffff}};
    for (const auto& r : bad_range) {
        std::vector<coeb_fuse_job> j{make_job(0, r[0], r[1], nullptr)};
        CHECK(says(chk(&cam, &p.c, j.data(), 1, 3.f), "range"));
    }
    {
        std::vector<coeb_fuse_job> j{make_job(0, 7, 0, nullptr)};       // an empty range at the list's end
        CHECK(!chk(&cam, &p.c, j.data(), 1, 3.f) && total == 0);
        j[0].Ow[2] = std::numeric_limits<float>::quiet_NaN();
        CHECK(says(chk(&cam, &p.c, j.data(), 1, 3.f), "pose"));
    }
    {
        Points q(7);
        q.c.normal = nullptr;
        CHECK(says(chk(&cam, &q.c, jobs.data(), 2, 3.f), "missing point"));
    }
    {
        Points q(7);
        q.pos[3 * 6 + 2] = std::numeric_limits<float>::infinity();
        CHECK(says(chk(&cam, &q.c, jobs.data(), 2, 3.f), "non-finite"));
        q.valid[6] = 0;
        CHECK(!chk(&cam, &q.c, jobs.data(), 2, 3.f));
        q.mind[0] = 0.f;
        CHECK(says(chk(&cam, &q.c, jobs.data(), 2, 3.f), "distance range"));
        q.mind[0] = 5.f;                                                // min > max
        CHECK(says(chk(&cam, &q.c, jobs.data(), 2, 3.f), "distance range"));
        q.mind[0] = 1.f;
        q.maxd[0] = std::numeric_limits<float>::infinity();
        CHECK(says(chk(&cam, &q.c, jobs.data(), 2, 3.f), "distance range"));
    }
    {   // the pair bound: 128 jobs over 8193 points is one job's worth too many
        Points q(8193);
        std::vector<coeb_fuse_job> j(128, make_job(0, 0, 8193, nullptr));
        std::vector<int32_t> o(1);
        CHECK(says(kfdb_fuse_check(used, geo, 4, &cam, &q.c, j.data(), 128, 3.f, o.data(), o.data(), &code, &total), "pairs") &&
              code == COEB_ERANGE);
        j[127].count = 8192 - 127;
        CHECK(!kfdb_fuse_check(used, geo, 4, &cam, &q.c, j.data(), 128, 3.f, o.data(), o.data(), &code, &total) &&
              total == COEB_FUSE_MAX_PAIRS);
    }
    return 0;
}

static int pack()
{
    const coeb_camera cam{500.f, 500.f, 320.f, 240.f, 40.f, 0.f, 640.f, 0.f, 480.f};
    coeb_camera other = cam;
    other.max_x = 600.f;
    std::vector<KfdbGridRec> rec(4, KfdbGridRec{});
    rec[1] = KfdbGridRec{1, cam.min_x, cam.max_x, cam.min_y, cam.max_y};
    rec[3] = KfdbGridRec{1, other.min_x, other.max_x, other.min_y, other.max_y};
    CHECK(kfdb_grid_current(rec[1], &cam) && !kfdb_grid_current(rec[1], &other) && !kfdb_grid_current(rec[0], &cam));
    std::vector<uint8_t> s17(17, 0), s1(1, 1);
    s17[16] = 1;
    std::vector<coeb_fuse_job> jobs{make_job(3, 0, 17, s17.data()), make_job(1, 5, 4, nullptr), make_job(0, 2, 1, s1.data()),
                                    make_job(3, 1, 2, nullptr), make_job(2, 9, 0, s1.data()), make_job(0, 0, 3, nullptr)};
    std::vector<KfdbFuseJob> tab;
    std::vector<uint8_t> skip;
    std::vector<int32_t> build;
    kfdb_fuse_pack(jobs.data(), (int)jobs.size(), rec.data(), &cam, tab, skip, build);
    CHECK(tab.size() == 6 && skip.size() == 32 + 16);
    const int out[6] = {0, 17, 21, 22, 24, 24}, sk[6] = {0, -1, 32, -1, -1, -1};
    for (int j = 0; j < 6; j++) {
        CHECK(tab[j].slot == jobs[j].slot && tab[j].first == jobs[j].first && tab[j].count == jobs[j].count);
        CHECK(tab[j].out_off == out[j] && tab[j].skip_off == sk[j]);
        CHECK(!memcmp(tab[j].Rcw, jobs[j].Rcw, 36) && !memcmp(tab[j].tcw, jobs[j].tcw, 12) && !memcmp(tab[j].Ow, jobs[j].Ow, 12));
    }
    CHECK(skip[16] == 1 && skip[15] == 0 && skip[17] == 0 && skip[32] == 1 && skip[33] == 0);
    // slot 3 was built under other bounds, slot 0 never; slot 1 is current; the zero-count job of slot 2 builds nothing
    CHECK(build.size() == 2 && build[0] == 0 && build[1] == 3);
    kfdb_fuse_pack(jobs.data(), (int)jobs.size(), rec.data(), &other, tab, skip, build);
    CHECK(build.size() == 2 && build[0] == 0 && build[1] == 1);
    kfdb_fuse_pack(nullptr, 0, rec.data(), &cam, tab, skip, build);
    CHECK(tab.empty() && skip.empty() && build.empty());
    return 0;
}

int main()
{
    if (rules() || pack()) return 1;
    puts("ok");
    return 0;
}
