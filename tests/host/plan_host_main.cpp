// The plan builder (coeb-slam_amd/csrc/coeb_plan.cpp: make_tables, make_plan and their tables) run
// without a device against the oracle's tables and its own layout invariants, built with
// ASan + UBSan by tests/test_plan_host.py.  Exit status 0 and "ok" on stdout: every check held.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "coeb_plan.hpp"
#include "orb_oracle.h"

static int g_fail = 0;
static char g_case[96] = "";
#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "%s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, g_case);   \
            g_fail++;                                                    \
        }                                                                \
    } while (0)

struct Params { int nfeatures; float scale_factor; int nlevels; };

static coeb_orb_params orb_params(const Params& q)
{
    coeb_orb_params p;
    memset(&p, 0, sizeof p);
    p.nfeatures = q.nfeatures; p.scale_factor = q.scale_factor; p.nlevels = q.nlevels;
    p.ini_th_fast = 20; p.min_th_fast = 7;
    return p;
}

// make_tables against ORBextractor's constructor as the oracle restates it, compared exactly
static void check_tables(const Params& q, const Tables& t)
{
    static oc_params o;          // 4 KB of pattern: not on the stack of every call
    CHECK(oc_init(&o, q.nfeatures, q.scale_factor, q.nlevels, 20, 7) == 0);
    const size_t fl = sizeof(float) * (size_t)q.nlevels;
    CHECK(t.nfeatures == o.nfeatures && t.nlevels == o.nlevels && t.scale_factor == o.scale_factor);
    CHECK(memcmp(t.scale, o.scale, fl) == 0 && memcmp(t.inv_scale, o.inv_scale, fl) == 0);
    CHECK(memcmp(t.sigma2, o.sigma2, fl) == 0 && memcmp(t.inv_sigma2, o.inv_sigma2, fl) == 0);
    CHECK(memcmp(t.nfeat, o.nfeat, sizeof(int) * (size_t)q.nlevels) == 0);
    CHECK(memcmp(t.umax, o.umax, sizeof(t.umax)) == 0);
    for (int l = q.nlevels; l < COEB_MAXL; l++) CHECK(t.scale[l] == 0 && t.nfeat[l] == 0);
}

static int expected_oct_kl(const Tables& t)
{
    int nmax = 0, kl = 512;
    for (int l = 0; l < t.nlevels; l++) nmax = t.nfeat[l] > nmax ? t.nfeat[l] : nmax;
    while (kl < 4096 && kl < (9 * nmax + 1) / 2) kl *= 2;
    return kl;
}

static void check_plan(const Params& q, int W, int H)
{
    snprintf(g_case, sizeof g_case, "%dx%d, %d features, %g, %d levels", W, H, q.nfeatures, q.scale_factor, q.nlevels);
    Tables t;
    CHECK(make_tables(orb_params(q), t));
    check_tables(q, t);
    Plan P;
    std::vector<int> rtab;
    std::vector<CellDesc> cells;
    std::string err;
    const bool ok = make_plan(t, W, H, 0, P, rtab, cells, err);
    CHECK(ok && err.empty());
    if (!ok) return;
    static oc_params o;
    oc_init(&o, q.nfeatures, q.scale_factor, q.nlevels, 20, 7);
    int og[7];
    oc_gauss_kernel7(og);
    CHECK(memcmp(P.gauss, og, sizeof og) == 0);
    CHECK(memcmp(P.umax, t.umax, sizeof P.umax) == 0);
    CHECK(P.W == W && P.H == H && P.L == q.nlevels);
    CHECK(P.rtab_ints == (int)rtab.size() && P.ncells == (int)cells.size());

    int64_t pyr_end = 0, blur_end = 0, node = 0;
    int kcap = 0, out = 0, ncells = 0, ncap_max = 0;
    size_t rtab_end = 0;
    for (int l = 0; l < P.L; l++) {
        const LevelGeom& g = P.lv[l];
        int ow, oh;
        oc_level_size(&o, W, H, l, &ow, &oh);
        CHECK(g.w == ow && g.h == oh);
        CHECK(g.pitch >= g.w && g.bpitch >= g.w && g.bpitch % 64 == 0 && (l == 0 ? g.pitch == W : g.pitch % 64 == 0));
        // level images and blurred levels: 256-aligned, in order, disjoint, inside the frame block
        if (l == 0) {
            CHECK(g.pyr_off == -1);
        } else {
            CHECK(g.pyr_off % 256 == 0 && g.pyr_off >= pyr_end);
            pyr_end = g.pyr_off + (int64_t)g.pitch * g.h;
            CHECK(pyr_end <= P.pyr_stride);
        }
        CHECK(g.blur_off % 256 == 0 && g.blur_off >= blur_end);
        blur_end = g.blur_off + (int64_t)g.bpitch * ((g.h + 7) / 8 * 8);      // whole 8-row tiles
        CHECK(blur_end <= P.blur_stride);
        if (l > 0) {
            const LevelGeom& s = P.lv[l - 1];
            CHECK(g.rtab_off % 4 == 0 && g.yrow_off % 4 == 0);
            CHECK((size_t)g.rtab_off >= rtab_end && (size_t)g.rtab_off + 2 * g.w + 2 * g.h <= (size_t)g.yrow_off);
            rtab_end = (size_t)g.yrow_off + 4 * (size_t)g.h;
            CHECK(rtab_end <= rtab.size());
            if (rtab_end > rtab.size()) return;
            const int* xofs = rtab.data() + g.rtab_off;
            const int* beta = xofs + 2 * g.w + g.h;
            bool xs = true, rows = true;
            for (int x = 0; x < g.w; x++) xs = xs && xofs[x] >= 0 && xofs[x] < s.w;
            CHECK(xs);
            CHECK(g.xmax >= 0 && g.xmax <= g.w);
            for (int dy = 0; dy < g.h; dy++) {
                const int* d = rtab.data() + g.yrow_off + 4 * dy;
                for (int k = 0; k < 2; k++) rows = rows && d[k] >= 0 && d[k] % s.pitch == 0 && d[k] / s.pitch < s.h;
                rows = rows && d[1] >= d[0] && d[1] - d[0] <= s.pitch && d[2] == beta[dy] && d[3] == dy * g.pitch;
            }
            CHECK(rows);
        }
        // FAST cells: inside the level, ROI <= 64 px, candidate bound within the cell slot
        CHECK(g.cell0 == ncells && g.ncells > 0 && g.ncols > 0 && g.nrows > 0);
        ncells += g.ncells;
        CHECK(ncells <= (int)cells.size());
        if (ncells > (int)cells.size()) return;
        bool in = true;
        for (int i = g.cell0; i < g.cell0 + g.ncells; i++) {
            const CellDesc& c = cells[i];
            in = in && c.level == l && c.x0 >= 0 && c.y0 >= 0 && c.rw > 0 && c.rh > 0 && c.rw <= 64 && c.rh <= 64;
            in = in && c.x0 + c.rw <= g.w && c.y0 + c.rh <= g.h && c.i >= 0 && c.i < g.nrows && c.j >= 0 && c.j < g.ncols;
            const int ww = c.rw > 6 ? c.rw - 6 : 0, wh = c.rh > 6 ? c.rh - 6 : 0;
            in = in && ((ww + 1) / 2) * ((wh + 1) / 2) <= P.cell_cap;
            in = in && c.rw <= P.max_roi_w && c.rh <= P.max_roi_h;
        }
        CHECK(in);
        // cumulative offsets
        CHECK(g.kcap_off == kcap && g.kcap == g.ncells * P.cell_cap);
        kcap += g.kcap;
        CHECK(g.out_off == out && g.out_cap > g.nfeat && g.ncap > g.out_cap);
        out += g.out_cap;
        CHECK(g.node_off == node);
        node += 2 * 8 * (int64_t)g.ncap;
        ncap_max = g.ncap > ncap_max ? g.ncap : ncap_max;
        CHECK(g.nfeat == t.nfeat[l] && g.nini >= 1 && g.nini <= 4);
        for (int i = 0; i < g.nini; i++) CHECK(g.ini_bound[i] <= g.ini_bound[i + 1]);
    }
    CHECK(ncells == P.ncells);
    CHECK(P.kbuf_stride == kcap && P.kcap == out && P.lvl_stride == out && P.node_stride == node);
    CHECK(P.max_roi_w <= 64 && P.max_roi_h <= 64);
    CHECK(P.oct_w % 16 == 0 && P.oct_w >= ncap_max);
    CHECK(P.oct_kl == expected_oct_kl(t));
    CHECK(P.oct_lds == P.oct_w * (4 + 16 + 4 + 4 + 4 + 1 + 64) + 8 * P.oct_kl && P.oct_lds <= 150 * 1024);
}

static void check_rejected(const Params& q, int W, int H, const char* msg)
{
    snprintf(g_case, sizeof g_case, "rejection of %dx%d, %d levels", W, H, q.nlevels);
    Tables t;
    CHECK(make_tables(orb_params(q), t));
    Plan P;
    std::vector<int> rtab;
    std::vector<CellDesc> cells;
    std::string err;
    CHECK(!make_plan(t, W, H, 0, P, rtab, cells, err));
    CHECK(err == msg);
}

static void check_oct_kl_override()
{
    snprintf(g_case, sizeof g_case, "oct_kl override");
    const Params q{1000, 1.2f, 8};
    Tables t;
    CHECK(make_tables(orb_params(q), t));
    const int give[] = {0, 256, 8192, 1, 100000}, take[] = {expected_oct_kl(t), 256, 8192, 256, 8192};
    for (int i = 0; i < 5; i++) {
        Plan P;
        std::vector<int> rtab;
        std::vector<CellDesc> cells;
        std::string err;
        CHECK(make_plan(t, 640, 480, give[i], P, rtab, cells, err));
        CHECK(P.oct_kl == take[i]);
        CHECK(P.oct_lds == P.oct_w * (4 + 16 + 4 + 4 + 4 + 1 + 64) + 8 * P.oct_kl);
    }
}

// The key capacity k_octree is launched with (oct_launch_keys).  tests/test_gpu_octree_layouts.py
// places its level-0 candidate counts one below, at and one above these two capacities.
static void check_oct_launch_keys()
{
    snprintf(g_case, sizeof g_case, "oct_launch_keys 640x480 default");
    Tables t;
    CHECK(make_tables(orb_params(Params{1000, 1.2f, 8}), t));
    Plan P;
    std::vector<int> rtab;
    std::vector<CellDesc> cells;
    std::string err;
    CHECK(make_plan(t, 640, 480, 0, P, rtab, cells, err));
    CHECK(P.oct_kl == 1024);
    const int F[] = {1, 16, 64, 65, 256}, want[] = {4096, 4096, 4096, 1024, 1024};
    for (int i = 0; i < 5; i++) {
        int kl = -1, lds = -1;
        oct_launch_keys(P, F[i], &kl, &lds);
        CHECK(kl == want[i]);
        CHECK(lds == P.oct_w * (4 + 16 + 4 + 4 + 4 + 1 + 64) + 8 * kl && lds <= 150 * 1024);
        CHECK(kl >= P.oct_kl && (kl == P.oct_kl) == (F[i] * P.L > 512));
    }
    // a plan whose node records leave no room for 4096 keys stops doubling inside the budget
    snprintf(g_case, sizeof g_case, "oct_launch_keys LDS budget");
    const int sizes[][2] = {{640, 480}, {1280, 960}, {4096, 4096}};
    const Params sets[] = {{1000, 1.2f, 8}, {2000, 1.2f, 8}, {500, 1.5f, 4}};
    for (const auto& s : sizes)
        for (const Params& q : sets) {
            CHECK(make_tables(orb_params(q), t));
            CHECK(make_plan(t, s[0], s[1], 0, P, rtab, cells, err));
            for (int f : {1, 512 / q.nlevels, 512 / q.nlevels + 1}) {
                int kl = -1, lds = -1;
                oct_launch_keys(P, f, &kl, &lds);
                CHECK(kl >= P.oct_kl && kl <= 4096 && (kl & (kl - 1)) == 0 && lds <= 150 * 1024);
                CHECK(lds == P.oct_w * (4 + 16 + 4 + 4 + 4 + 1 + 64) + 8 * kl);
                if (f * q.nlevels > 512) CHECK(kl == P.oct_kl && lds == P.oct_lds);
            }
        }
}

int main()
{
    const int sizes[][2] = {{640, 480}, {1280, 960}, {752, 480}, {1241, 376}, {321, 243}, {4096, 4096}};
    const Params sets[] = {{1000, 1.2f, 8}, {2000, 1.2f, 8}, {500, 1.5f, 4}, {1000, 1.2f, 2}};
    for (const auto& s : sizes)
        for (const Params& q : sets) check_plan(q, s[0], s[1]);
    // the smallest frame: two levels fit, the deeper pyramids end below the 30-px grid
    const char* small = "pyramid level too small for the 30-px FAST grid";
    check_plan(sets[3], 160, 120);
    for (int k = 0; k < 3; k++) check_rejected(sets[k], 160, 120, small);
    check_rejected(sets[0], 64, 48, small);
    check_rejected(sets[0], 4097, 480, "image larger than 4096 px is not supported (12-bit key packing)");
    check_rejected(sets[0], 640, 4097, "image larger than 4096 px is not supported (12-bit key packing)");
    check_rejected(Params{1000, 1.2f, 1}, 1200, 100, "aspect ratio gives an unsupported number of initial octree nodes");
    snprintf(g_case, sizeof g_case, "make_tables rejections");
    Tables t;
    CHECK(!make_tables(orb_params(Params{1000, 1.2f, 0}), t));
    CHECK(!make_tables(orb_params(Params{1000, 1.2f, 17}), t));
    CHECK(!make_tables(orb_params(Params{-1, 1.2f, 8}), t));
    CHECK(!make_tables(orb_params(Params{1000, 0.0f, 8}), t));
    CHECK(!make_tables(orb_params(Params{1000, -1.2f, 8}), t));
    CHECK(make_tables(orb_params(Params{0, 1.2f, 16}), t));
    check_oct_kl_override();
    check_oct_launch_keys();
    if (g_fail) {
        fprintf(stderr, "%d check(s) failed\n", g_fail);
        return 1;
    }
    puts("ok");
    return 0;
}
