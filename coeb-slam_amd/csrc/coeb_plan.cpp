// coeb_plan.cpp -- builder of the extraction's geometry plan (coeb_plan.hpp).  Host work of
// O(levels + cells) per image size, cached by the context (ensure_plan, coeb_capi.hip).  Built
// with the library's own compiler and floating-point flags: the level sizes, hx and ini_bound
// are float arithmetic the kernels' results depend on.
#include "coeb_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace {

enum { PATCH_SIZE = 31, HALF_PATCH_SIZE = 15, EDGE_THRESHOLD = 19 };
constexpr int kRoiMax = 64;

inline int cv_round(float v) { return (int)lrintf(v); }
inline int cv_round_d(double v) { return (int)lrint(v); }
inline int cv_floor(float v) { int i = (int)v; return i - (i > v); }
inline int cv_ceil_d(double v) { int i = (int)v; return i + (i < v); }
inline int64_t align256(int64_t v) { return (v + 255) & ~int64_t(255); }

}  // namespace

bool make_tables(const coeb_orb_params& prm, Tables& t)
{
    if (prm.nlevels < 1 || prm.nlevels > COEB_MAXL || prm.nfeatures < 0 || !(prm.scale_factor > 0)) return false;
    memset(&t, 0, sizeof(t));
    t.nfeatures = prm.nfeatures;
    t.scale_factor = prm.scale_factor;
    t.nlevels = prm.nlevels;
    t.scale[0] = 1.0f;
    t.sigma2[0] = 1.0f;
    for (int i = 1; i < t.nlevels; i++) {
        t.scale[i] = (float)((double)t.scale[i - 1] * t.scale_factor);
        t.sigma2[i] = t.scale[i] * t.scale[i];
    }
    for (int i = 0; i < t.nlevels; i++) {
        t.inv_scale[i] = 1.0f / t.scale[i];
        t.inv_sigma2[i] = 1.0f / t.sigma2[i];
    }
    const float factor = (float)(1.0f / t.scale_factor);
    float ndesired = t.nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)t.nlevels));
    int sum = 0;
    for (int l = 0; l < t.nlevels - 1; l++) {
        t.nfeat[l] = cv_round(ndesired);
        sum += t.nfeat[l];
        ndesired *= factor;
    }
    t.nfeat[t.nlevels - 1] = std::max(t.nfeatures - sum, 0);
    int v, v0;
    const int vmax = cv_floor(HALF_PATCH_SIZE * sqrtf(2.f) / 2 + 1);
    const int vmin = cv_ceil_d(HALF_PATCH_SIZE * sqrtf(2.f) / 2);
    const double hp2 = HALF_PATCH_SIZE * HALF_PATCH_SIZE;
    for (v = 0; v <= vmax; ++v) t.umax[v] = cv_round_d(std::sqrt(hp2 - v * v));
    for (v = HALF_PATCH_SIZE, v0 = 0; v >= vmin; --v) {
        while (t.umax[v0] == t.umax[v0 + 1]) ++v0;
        t.umax[v] = v0;
        ++v0;
    }
    return true;
}

void gauss_kernel7(int k[7])
{
    const int n = 7, n2 = 3;
    const double scale2X = -0.125 / (2.0 * 2.0);
    double values[3], sum = 0.0;
    for (int i = 0, x = 1 - n; i < n2; i++, x += 2) {
        const double t = std::exp((double)(x * x) * scale2X);
        values[i] = t;
        sum += t;
    }
    sum = sum * 2.0 + 1.0;
    const double mul1 = 1.0 / sum;
    double err = 0.0;
    int64_t s = 0;
    for (int i = 0; i < n2; i++) {
        const double adj = values[i] * mul1 * 256.0 + err;
        const int64_t q = cv_round_d(adj);
        err = adj - (double)q;
        k[i] = k[n - 1 - i] = (int)q;
        s += q;
    }
    k[n2] = (int)(256 - 2 * s);
}

int resize_tables(int sw, int sh, int dw, int dh, std::vector<int>& tab)
{
    const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
    const size_t base = tab.size();
    tab.resize(base + 2 * dw + 2 * dh);
    int* xofs = tab.data() + base;
    int* alpha = xofs + dw;
    int* yofs = alpha + dw;
    int* beta = yofs + dh;
    int xmax = dw;
    for (int dx = 0; dx < dw; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = cv_floor(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx + 1 >= sw) {
            xmax = std::min(xmax, dx);
            if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
        }
        xofs[dx] = sx;
        const int a0 = std::max(-32768, std::min(32767, cv_round((1.f - fx) * 2048)));
        const int a1 = std::max(-32768, std::min(32767, cv_round(fx * 2048)));
        alpha[dx] = (a0 & 0xFFFF) | (a1 << 16);
    }
    for (int dy = 0; dy < dh; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        const int sy = cv_floor(fy);
        fy -= sy;
        yofs[dy] = sy;
        const int b0 = std::max(-32768, std::min(32767, cv_round((1.f - fy) * 2048)));
        const int b1 = std::max(-32768, std::min(32767, cv_round(fy * 2048)));
        beta[dy] = (b0 & 0xFFFF) | (b1 << 16);
    }
    return xmax;
}

static_assert(sizeof(PyrBand) == kPyrBandInts * sizeof(int) && kPyrBandInts % 4 == 0, "PyrBand: whole 16-byte table rows");

int pyr_band_pattern(const int* yofs, int oy, int dh, int sh)
{
    if (oy + kPyrBandRows > dh) return kPyrBandGeneric;                      // the partial band
    if (yofs[oy] < 0 || yofs[oy + kPyrBandRows - 1] + 1 > sh - 1) return kPyrBandGeneric;   // a clamped row
    unsigned mask = 0;
    for (int i = 0; i + 1 < kPyrBandRows; i++) {
        const int step = yofs[oy + i + 1] - yofs[oy + i];
        if (step != 1 && step != 2) return kPyrBandGeneric;
        mask |= (unsigned)(step - 1) << i;
    }
    for (int p = 0; p < kPyrPatterns; p++)
        if (kPyrPatternMask[p] == mask) return p;
    return kPyrBandGeneric;
}

bool make_plan(const Tables& t, int W, int H, int oct_kl_override, Plan& P, std::vector<int>& rtab,
               std::vector<CellDesc>& cells, std::string& err)
{
    memset(&P, 0, sizeof(P));
    P.W = W; P.H = H; P.L = t.nlevels;
    rtab.clear();
    cells.clear();
    if (W > 4096 || H > 4096) { err = "image larger than 4096 px is not supported (12-bit key packing)"; return false; }
    int64_t pyr = 0, blur = 0, node = 0;
    int kcap_total = 0, out_total = 0, cell_cap = 1;
    for (int l = 0; l < t.nlevels; l++) {
        LevelGeom& g = P.lv[l];
        g.w = cv_round((float)W * t.inv_scale[l]);     // ComputePyramid :1349
        g.h = cv_round((float)H * t.inv_scale[l]);
        g.scale = t.scale[l];
        g.size_i = (int)(PATCH_SIZE * t.scale[l]);
        g.pitch = l == 0 ? W : (g.w + 63) & ~63;
        g.bpitch = (g.w + 63) & ~63;
        if (l == 0) g.pyr_off = -1;
        else { g.pyr_off = pyr; pyr = align256(pyr + (int64_t)g.pitch * g.h); }
        g.blur_off = blur;
        blur = align256(blur + (int64_t)g.bpitch * ((g.h + 7) & ~7));    // whole 8-row tiles
        if (l > 0) {
            while (rtab.size() % 4) rtab.push_back(0);     // 16-byte aligned table rows
            g.rtab_off = (int)rtab.size();
            g.xmax = resize_tables(P.lv[l - 1].w, P.lv[l - 1].h, g.w, g.h, rtab);
            g.rows_ok = 1;
            for (int c = 0; c < g.w; c += 2) {
                const int* xofs = rtab.data() + g.rtab_off;
                if (xofs[std::min(c + 1, g.w - 1)] - (xofs[c] & ~3) > 5) g.rows_ok = 0;
            }
            // k_pyr_rows' row descriptors: one 16-byte scalar load per output row
            while (rtab.size() % 4) rtab.push_back(0);
            g.yrow_off = (int)rtab.size();
            const int sh = P.lv[l - 1].h, sp = P.lv[l - 1].pitch;
            for (int dy = 0; dy < g.h; dy++) {
                const int q0 = rtab[g.rtab_off + 2 * g.w + dy], bb = rtab[g.rtab_off + 2 * g.w + g.h + dy];
                const int r0 = q0 >= 0 ? (q0 < sh ? q0 : sh - 1) : 0;
                const int r1 = q0 + 1 >= 0 ? (q0 + 1 < sh ? q0 + 1 : sh - 1) : 0;
                rtab.push_back(r0 * sp);
                rtab.push_back(r1 * sp);
                rtab.push_back(bb);
                rtab.push_back(dy * g.pitch);
            }
            // k_pyr_rows' band descriptors (PyrBand, coeb_plan.hpp)
            g.band_off = (int)rtab.size();
            rtab.reserve(rtab.size() + (size_t)kPyrBandInts * ((g.h + kPyrBandRows - 1) / kPyrBandRows));
            const int* yofs = rtab.data() + g.rtab_off + 2 * g.w;      // stays valid: reserved above
            for (int oy = 0; oy < g.h; oy += kPyrBandRows) {
                PyrBand bd;
                memset(&bd, 0, sizeof bd);
                bd.pattern = pyr_band_pattern(yofs, oy, g.h, sh);
                bd.src_off = std::max(0, std::min(yofs[oy], sh - 1)) * sp;
                bd.dst_off = oy * g.pitch;
                for (int r = 0; r < kPyrBandRows && oy + r < g.h; r++) bd.beta[r] = yofs[g.h + oy + r];
                int v[kPyrBandInts];
                memcpy(v, &bd, sizeof v);
                rtab.insert(rtab.end(), v, v + kPyrBandInts);
            }
        }
        // FAST cells (ComputeKeyPointsOctTree :795-829)
        const int minBorderX = EDGE_THRESHOLD - 3, minBorderY = minBorderX;
        const int maxBorderX = g.w - EDGE_THRESHOLD + 3, maxBorderY = g.h - EDGE_THRESHOLD + 3;
        const float width = (float)(maxBorderX - minBorderX), height = (float)(maxBorderY - minBorderY);
        const float Wc = 30;
        g.ncols = (int)(width / Wc);
        g.nrows = (int)(height / Wc);
        if (g.ncols <= 0 || g.nrows <= 0) { err = "pyramid level too small for the 30-px FAST grid"; return false; }
        g.wcell = (int)ceilf(width / g.ncols);
        g.hcell = (int)ceilf(height / g.nrows);
        g.cell0 = (int)cells.size();
        for (int i = 0; i < g.nrows; i++) {
            const float iniY = (float)(minBorderY + i * g.hcell);
            float maxY = iniY + g.hcell + 6;
            if (iniY >= maxBorderY - 3) continue;
            if (maxY > maxBorderY) maxY = (float)maxBorderY;
            for (int j = 0; j < g.ncols; j++) {
                const float iniX = (float)(minBorderX + j * g.wcell);
                float maxX = iniX + g.wcell + 6;
                if (iniX >= maxBorderX - 6) continue;
                if (maxX > maxBorderX) maxX = (float)maxBorderX;
                CellDesc c;
                c.level = (int16_t)l; c.pad = 0;
                c.x0 = (int16_t)(int)iniX; c.y0 = (int16_t)(int)iniY;
                c.rw = (int16_t)((int)maxX - (int)iniX); c.rh = (int16_t)((int)maxY - (int)iniY);
                c.i = (int16_t)i; c.j = (int16_t)j;
                if (c.rw > kRoiMax || c.rh > kRoiMax) { err = "FAST cell ROI exceeds 64 px"; return false; }
                const int ww = std::max(0, c.rw - 6), wh = std::max(0, c.rh - 6);
                cell_cap = std::max(cell_cap, ((ww + 1) / 2) * ((wh + 1) / 2));
                P.max_roi_w = std::max(P.max_roi_w, (int)c.rw);
                P.max_roi_h = std::max(P.max_roi_h, (int)c.rh);
                cells.push_back(c);
            }
        }
        g.ncells = (int)cells.size() - g.cell0;
        // DistributeOctTree constants (:549-552, :866-875)
        g.nfeat = t.nfeat[l];
        g.nfeat_area = (int)((double)t.nfeat[l] * 0.7);
        g.maxX = maxBorderX - minBorderX;
        g.maxY = maxBorderY - minBorderY;
        g.nini = (int)roundf((float)g.maxX / g.maxY);
        if (g.nini < 1 || g.nini > 4) { err = "aspect ratio gives an unsupported number of initial octree nodes"; return false; }
        g.hx = (float)g.maxX / g.nini;
        int b = 0;
        for (int i = 0; i <= g.nini; i++) {
            while (b <= g.maxX + 1 && (int)((float)b / g.hx) < i) b++;
            g.ini_bound[i] = b;
        }
        g.ini_bound[g.nini] = 1 << 20;
        // list size never exceeds max(N + 2, 4 * nIni)
        g.out_cap = std::max(g.nfeat + 3, 4 * g.nini) + 5;
        g.ncap = g.out_cap + 8;
        g.node_off = node;
        node += 2 * 8 * (int64_t)g.ncap;
        g.out_off = out_total;
        out_total += g.out_cap;
    }
    P.ncells = (int)cells.size();
    P.cell_cap = cell_cap;
    for (int l = 0; l < t.nlevels; l++) {
        P.lv[l].kcap_off = kcap_total;
        P.lv[l].kcap = P.lv[l].ncells * cell_cap;
        kcap_total += P.lv[l].kcap;
    }
    P.pyr_stride = std::max<int64_t>(pyr, 256);
    P.blur_stride = blur;
    P.kbuf_stride = kcap_total;
    P.node_stride = node;
    P.lvl_stride = out_total;
    P.kcap = out_total;
    P.rtab_ints = (int)rtab.size();
    P.oct_w = 0;
    for (int l = 0; l < t.nlevels; l++) P.oct_w = std::max(P.oct_w, P.lv[l].ncap);
    P.oct_w = (P.oct_w + 15) & ~15;
    // keys kept in LDS per level (more candidates: global ping-pong buffers, slower but exact):
    // the power of two >= 4.5 x the largest level's features (FAST leaves ~3.8 candidates per
    // level-0 feature on the config-A frames: 818 median, 934 max for 217), so that config A's
    // octree needs 31 KB of LDS and five workgroups share a CU (0.091 -> 0.075 ms per step; 768
    // keys pushed level 0 to the global buffers, 0.102 ms); oct_kl_override replaces it
    int nmax = 0;
    for (int l = 0; l < t.nlevels; l++) nmax = std::max(nmax, P.lv[l].nfeat);
    P.oct_kl = 512;
    while (P.oct_kl < 4096 && P.oct_kl < (9 * nmax + 1) / 2) P.oct_kl *= 2;
    if (oct_kl_override) P.oct_kl = std::max(256, std::min(8192, oct_kl_override));
    P.oct_lds = P.oct_w * (4 + 16 + 4 + 4 + 4 + 1 + 64) + 8 * P.oct_kl;
    if (P.oct_lds > 150 * 1024) { err = "octree LDS budget exceeded (features per level too large)"; return false; }
    memcpy(P.umax, t.umax, sizeof(P.umax));
    // k_describe folds the IC_Angle disc (umax for HALF_PATCH_SIZE 15) into constants
    static const int kUmaxDisc[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
    if (memcmp(t.umax, kUmaxDisc, sizeof(kUmaxDisc)) != 0) { err = "unexpected IC_Angle disc (umax)"; return false; }
    gauss_kernel7(P.gauss);

    return true;
}

void oct_launch_keys(const Plan& plan, int F, int* kl_out, int* lds_out)
{
    int oct_kl = plan.oct_kl, oct_lds = plan.oct_lds;
    if (F * plan.L <= 2 * 256) {
        int kl = oct_kl;
        while (kl < 4096 && plan.oct_w * (4 + 16 + 4 + 4 + 4 + 1 + 64) + 8 * (2 * kl) <= 150 * 1024) kl *= 2;
        oct_kl = kl;
        oct_lds = plan.oct_w * (4 + 16 + 4 + 4 + 4 + 1 + 64) + 8 * kl;
    }
    *kl_out = oct_kl;
    *lds_out = oct_lds;
}
