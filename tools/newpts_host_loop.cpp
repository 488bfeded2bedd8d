// The loop body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:285-433) as a plain single-thread C++
// loop without cv::Mat: the arithmetic of k_tri_points (csrc/coeb_kfdb.hip) statement by
// statement, on the pairs a search call returned.  tools/newpts_time.py compiles it (-O2 -ffp-contract=off),
// loads it through ctypes and times it behind coeb_kfdb_search_triangulation: figure (c).  It has no
// allocation and no cv::Mat temporary per step, so it understates the reference's host cost.
#include <climits>
#include <cmath>
#include <cstdint>

namespace {
struct View { float Rcw[9], tcw[3], Ow[3], fx, fy, cx, cy, invfx, invfy, mb, mbf; };
struct Feat { float x, y, ur, kx, ky, depth; };
const float kEps = 4.76837158203125e-07f;

inline float sq4(const float* a) { return std::fmaf(a[3], a[3], std::fmaf(a[2], a[2], std::fmaf(a[1], a[1], a[0] * a[0]))); }

bool jacobi_pair(float (*a)[4], float (*v)[4], int P, int Q)
{
    const float alpha = sq4(a[P]), beta = sq4(a[Q]);
    const float gamma = std::fmaf(a[P][3], a[Q][3], std::fmaf(a[P][2], a[Q][2], std::fmaf(a[P][1], a[Q][1], a[P][0] * a[Q][0])));
    if (std::fabs(gamma) <= kEps * std::sqrt(alpha * beta)) return false;
    const float zeta = (beta - alpha) / (2.0f * gamma);
    const float t = std::copysign(1.0f, zeta) / (std::fabs(zeta) + std::sqrt(std::fmaf(zeta, zeta, 1.0f)));
    const float c = 1.0f / std::sqrt(std::fmaf(t, t, 1.0f));
    const float s = c * t;
    for (int r = 0; r < 4; r++) {
        const float x = a[P][r], y = a[Q][r];
        a[P][r] = std::fmaf(c, x, -(s * y));
        a[Q][r] = std::fmaf(s, x, c * y);
        const float vx = v[P][r], vy = v[Q][r];
        v[P][r] = std::fmaf(c, vx, -(s * vy));
        v[Q][r] = std::fmaf(s, vx, c * vy);
    }
    return true;
}

void jacobi_null4(float (*a)[4], float* out)
{
    float v[4][4];
    for (int c = 0; c < 4; c++)
        for (int r = 0; r < 4; r++) v[c][r] = c == r ? 1.0f : 0.0f;
    bool active = true;
    for (int sweep = 0; sweep < 12 && active; sweep++) {
        bool rot = jacobi_pair(a, v, 0, 1);
        rot |= jacobi_pair(a, v, 0, 2);
        rot |= jacobi_pair(a, v, 0, 3);
        rot |= jacobi_pair(a, v, 1, 2);
        rot |= jacobi_pair(a, v, 1, 3);
        rot |= jacobi_pair(a, v, 2, 3);
        active = rot;
    }
    int best = 0;
    float bs = sq4(a[0]);
    for (int c = 1; c < 4; c++) {
        const float s = sq4(a[c]);
        if (s <= bs) { bs = s; best = c; }
    }
    for (int r = 0; r < 4; r++) out[r] = v[best][r];
}

inline void rwc_mul(const float* R, const float* x, float* out)
{
    for (int k = 0; k < 3; k++) {
        float t = R[k] * x[0] + R[3 + k] * x[1];
        t = t + R[6 + k] * x[2];
        out[k] = t;
    }
}
inline double norm3(const float* d)
{
    double ss = 0.0;
    ss += (double)d[0] * (double)d[0];
    ss += (double)d[1] * (double)d[1];
    ss += (double)d[2] * (double)d[2];
    return std::sqrt(ss);
}
inline float row_dot_add(const View& V, int r, const float* X)
{
    double d = 0.0;
    d += (double)V.Rcw[3 * r] * (double)X[0];
    d += (double)V.Rcw[3 * r + 1] * (double)X[1];
    d += (double)V.Rcw[3 * r + 2] * (double)X[2];
    return (float)(d + (double)V.tcw[r]);
}
inline float bound(float mb, float depth)
{
    const double h = (double)(mb / 2.0f), d = (double)depth;
    return (float)((d * d - h * h) / (d * d + h * h));
}
inline void unproject(const View& V, const Feat& f, float* X)
{
    const float z = f.depth;
    const float Pc[3] = {(f.kx - V.cx) * z * V.invfx, (f.ky - V.cy) * z * V.invfy, z};
    float t[3];
    rwc_mul(V.Rcw, Pc, t);
    for (int k = 0; k < 3; k++) X[k] = (float)((double)t[k] + (double)V.Ow[k]);
}
inline bool reproj_fails(const View& V, float mbf, const float* X, float z, const Feat& g, float sigma2)
{
    const float x = row_dot_add(V, 0, X), y = row_dot_add(V, 1, X);
    const float invz = (float)(1.0 / (double)z);
    const float u = std::fmaf(V.fx * x, invz, V.cx), v = std::fmaf(V.fy * y, invz, V.cy);
    const float ex = u - g.x, ey = v - g.y;
    float e2 = std::fmaf(ex, ex, ey * ey);
    if (!(g.ur >= 0)) return (double)e2 > 5.991 * (double)sigma2;
    const float er = std::fmaf(-mbf, invz, u) - g.ur;
    e2 = std::fmaf(er, er, e2);
    return (double)e2 > 7.8 * (double)sigma2;
}
}  // namespace

// views: keyframe 1, then the neighbours, 23 floats each.  feat[k] / oct[k]: keyframe 1 (k = 0) and neighbour
// k - 1: [x, y, u_right, raw x, raw y, depth] per feature and its octave.  match [nnb][n1] as the search returns
// it.  status [nnb][n1] (code | source << 4), x3d [nnb][n1][3] (accepted entries only), first_ok [n1].
extern "C" void newpts_host_loop(const float* views, int nnb, int n1, const float* const* feat, const int32_t* const* oct,
                                 const int32_t* match, const float* scale, const float* sigma2, float ratio_factor,
                                 int8_t* status, float* x3d, int32_t* first_ok)
{
    const View* V = reinterpret_cast<const View*>(views);
    const View& V1 = V[0];
    const Feat* f1 = reinterpret_cast<const Feat*>(feat[0]);
    for (int i = 0; i < n1; i++) first_ok[i] = -1;
    for (int j = 0; j < nnb; j++) {
        const View& V2 = V[1 + j];
        const Feat* f2 = reinterpret_cast<const Feat*>(feat[1 + j]);
        for (int i = 0; i < n1; i++) {
            const long e = (long)j * n1 + i;
            const int i2 = match[e];
            if (i2 < 0) { status[e] = 0; continue; }
            const Feat g1 = f1[i], g2 = f2[i2];
            const int o1 = oct[0][i], o2 = oct[1 + j][i2];
            const bool st1 = g1.ur >= 0, st2 = g2.ur >= 0;
            const float xn1[3] = {(g1.x - V1.cx) * V1.invfx, (g1.y - V1.cy) * V1.invfy, 1.0f};
            const float xn2[3] = {(g2.x - V2.cx) * V2.invfx, (g2.y - V2.cy) * V2.invfy, 1.0f};
            float ray1[3], ray2[3];
            rwc_mul(V1.Rcw, xn1, ray1);
            rwc_mul(V2.Rcw, xn2, ray2);
            double dot = 0.0;
            dot += (double)ray1[0] * (double)ray2[0];
            dot += (double)ray1[1] * (double)ray2[1];
            dot += (double)ray1[2] * (double)ray2[2];
            const float cos_rays = (float)(dot / (norm3(ray1) * norm3(ray2)));
            float cps1 = cos_rays + 1.0f, cps2 = cps1;
            if (st1) cps1 = bound(V1.mb, g1.depth);
            else if (st2) cps2 = bound(V2.mb, g2.depth);
            const float cps = cps2 < cps1 ? cps2 : cps1;
            float X[3];
            int src;
            if (cos_rays < cps && cos_rays > 0.0f && (st1 || st2 || (double)cos_rays < 0.9998)) {
                src = 1;
                float A[4][4];
                for (int c = 0; c < 4; c++) {
                    const float t10 = c < 3 ? V1.Rcw[c] : V1.tcw[0], t11 = c < 3 ? V1.Rcw[3 + c] : V1.tcw[1];
                    const float t12 = c < 3 ? V1.Rcw[6 + c] : V1.tcw[2];
                    const float t20 = c < 3 ? V2.Rcw[c] : V2.tcw[0], t21 = c < 3 ? V2.Rcw[3 + c] : V2.tcw[1];
                    const float t22 = c < 3 ? V2.Rcw[6 + c] : V2.tcw[2];
                    A[c][0] = xn1[0] * t12 - t10;
                    A[c][1] = xn1[1] * t12 - t11;
                    A[c][2] = xn2[0] * t22 - t20;
                    A[c][3] = xn2[1] * t22 - t21;
                }
                float h[4];
                jacobi_null4(A, h);
                if (h[3] == 0.0f) { status[e] = (int8_t)(3 | (src << 4)); continue; }
                const float inv = (float)(1.0 / (double)h[3]);
                X[0] = h[0] * inv; X[1] = h[1] * inv; X[2] = h[2] * inv;
            } else if (st1 && cps1 < cps2) {
                src = 2;
                unproject(V1, g1, X);
            } else if (st2 && cps2 < cps1) {
                src = 3;
                unproject(V2, g2, X);
            } else {
                status[e] = 2;
                continue;
            }
            int code = 1;
            const float z1 = row_dot_add(V1, 2, X), z2 = row_dot_add(V2, 2, X);
            if (z1 <= 0.0f) code = 4;
            else if (z2 <= 0.0f) code = 5;
            else if (reproj_fails(V1, V1.mbf, X, z1, g1, sigma2[o1])) code = 6;
            else if (reproj_fails(V2, V1.mbf, X, z2, g2, sigma2[o2])) code = 7;
            else {
                const float d1[3] = {X[0] - V1.Ow[0], X[1] - V1.Ow[1], X[2] - V1.Ow[2]};
                const float d2[3] = {X[0] - V2.Ow[0], X[1] - V2.Ow[1], X[2] - V2.Ow[2]};
                const float dist1 = (float)norm3(d1), dist2 = (float)norm3(d2);
                if (dist1 == 0.0f || dist2 == 0.0f) code = 8;
                else {
                    const float rd = dist2 / dist1, ro = scale[o1] / scale[o2];
                    if (rd * ratio_factor < ro || rd > ro * ratio_factor) code = 9;
                }
            }
            status[e] = (int8_t)(code | (src << 4));
            if (code == 1) {
                x3d[3 * e] = X[0]; x3d[3 * e + 1] = X[1]; x3d[3 * e + 2] = X[2];
                if (first_ok[i] < 0) first_ok[i] = j;
            }
        }
    }
}
