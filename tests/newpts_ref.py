"""CPU reference of the loop body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:285-433) with
KeyFrame::UnprojectStereo (src/KeyFrame.cc:615-631), as literal Python in float32 / float64 for one pair.
The float forms are those DESIGN.md s2.1 lists: fused multiply-adds are fmaf() here, everything else is
one float32 (or, where said, float64) operation per step.  Two forms differ from the reference by
construction: the null vector of the 4x4 system is the canonical one-sided Jacobi of jacobi_null4(), not
cv::SVD's, and the stereo parallax bound cos(2 atan2(mb / 2, depth)) is (d^2 - h^2) / (d^2 + h^2) in
double.  tests/test_newpts_ref.py pins this file on a hand-worked pair and against a float64 model; `mut`
selects the wrong readings tests/newpts_cases.py shows its cases notice."""
import numpy as np

import tri_ref as T
from tri_ref import f32, fmaf

NO_PAIR, ACCEPTED, LOW_PARALLAX, W_ZERO, Z1, Z2, REPROJ1, REPROJ2, ZERO_DIST, RATIO = range(10)
SRC_NONE, SRC_TRI, SRC_STEREO1, SRC_STEREO2 = range(4)
STATUS_NAMES = ("no_pair", "accepted", "low_parallax", "w_zero", "z1", "z2", "reproj1", "reproj2", "zero_dist", "ratio")

MUTATIONS = ("else_if_to_if", "mbf_kf2", "chi2_float", "last_accepted", "z_lt", "ratio_swapped",
             "undistorted_unproject", "no_9998", "w_after_division")
# no float32 equals the double product 5.991 * sigma2 or 7.8 * sigma2 of any level (test_newpts_ref checks it)
EQUIVALENT = ("chi2_ge",)

JACOBI_SWEEPS = 12
JACOBI_EPS = f32(2.0 ** -21)
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def sq4(a):
    return fmaf(a[3], a[3], fmaf(a[2], a[2], fmaf(a[1], a[1], f32(a[0] * a[0]))))


def jacobi_null4(A, sweeps_out=None):
    """A [4, 4] float32 (rows as the reference fills them) -> the right singular vector of its smallest
    singular value, by one-sided Jacobi on the columns in float32: pairs in PAIRS order, a pair left alone
    where |ap.aq| <= 2^-21 sqrt(|ap|^2 |aq|^2), done after a sweep without a rotation or JACOBI_SWEEPS
    sweeps; the smallest column norm picks the column of V, the last of equals."""
    a = [[f32(A[r][c]) for r in range(4)] for c in range(4)]         # a[c][r]
    v = [[f32(1.0 if r == c else 0.0) for r in range(4)] for c in range(4)]
    one = f32(1.0)
    nsweep = 0
    with np.errstate(all="ignore"):
        for _ in range(JACOBI_SWEEPS):
            nsweep += 1
            rot = False
            for p, q in PAIRS:
                ap, aq = a[p], a[q]
                alpha, beta = sq4(ap), sq4(aq)
                gamma = fmaf(ap[3], aq[3], fmaf(ap[2], aq[2], fmaf(ap[1], aq[1], f32(ap[0] * aq[0]))))
                if abs(gamma) <= f32(JACOBI_EPS * np.sqrt(f32(alpha * beta))):
                    continue
                rot = True
                zeta = f32(f32(beta - alpha) / f32(f32(2.0) * gamma))
                t = f32(np.copysign(one, zeta) / f32(abs(zeta) + np.sqrt(fmaf(zeta, zeta, one))))
                c = f32(one / np.sqrt(fmaf(t, t, one)))
                s = f32(c * t)
                for m in (a, v):
                    for r in range(4):
                        x, y = m[p][r], m[q][r]
                        m[p][r] = fmaf(c, x, -f32(s * y))
                        m[q][r] = fmaf(s, x, f32(c * y))
            if not rot:
                break
        best, out = sq4(a[0]), v[0]
        for c in range(1, 4):
            s = sq4(a[c])
            if s <= best:
                best, out = s, v[c]
    if sweeps_out is not None:
        sweeps_out.append(nsweep)
    return np.array(out, f32)


def rwc_mul(Rcw, x):
    """Rwc * x, Rwc = Rcw.t(): cv::Mat's small gemm, float products summed left to right."""
    out = []
    for k in range(3):
        t = f32(f32(Rcw[0 + k] * x[0]) + f32(Rcw[3 + k] * x[1]))
        out.append(f32(t + f32(Rcw[6 + k] * x[2])))
    return out


def dot64(a, b):
    d = 0.0
    for x, y in zip(a, b):
        d += float(x) * float(y)
    return d


def norm3(a):
    return float(np.sqrt(dot64(a, a)))


def row_dot_add(V, r, X):
    """Rcw.row(r).dot(x3Dt) + tcw(r): Mat::dot in double, the sum in double, to float."""
    return f32(dot64(V["Rcw"][3 * r:3 * r + 3], X) + float(V["tcw"][r]))


def stereo_parallax_bound(mb, depth):
    h, d = float(f32(f32(mb) / f32(2.0))), float(f32(depth))
    with np.errstate(all="ignore"):
        return f32(np.float64(d * d - h * h) / np.float64(d * d + h * h))


def unproject_stereo(V, kx, ky, depth):
    z = f32(depth)
    Pc = [f32(f32(f32(f32(kx) - V["cx"]) * z) * V["invfx"]), f32(f32(f32(f32(ky) - V["cy"]) * z) * V["invfy"]), z]
    t = rwc_mul(V["Rcw"], Pc)
    return [f32(float(t[k]) + float(V["Ow"][k])) for k in range(3)]


def reproj_fails(V, mbf, X, z, g, sigma2, mut):
    x, y = row_dot_add(V, 0, X), row_dot_add(V, 1, X)
    with np.errstate(all="ignore"):
        invz = f32(np.float64(1.0) / np.float64(z))
        u, v = fmaf(f32(V["fx"] * x), invz, V["cx"]), fmaf(f32(V["fy"] * y), invz, V["cy"])
        ex, ey = f32(u - f32(g["x"])), f32(v - f32(g["y"]))
        e2 = fmaf(ex, ex, f32(ey * ey))
        if not f32(g["u_right"]) >= 0:
            k = 5.991
        else:
            er = f32(fmaf(-f32(mbf), invz, u) - f32(g["u_right"]))
            e2 = fmaf(er, er, e2)
            k = 7.8
        if "chi2_float" in mut:
            return bool(e2 > f32(f32(k) * f32(sigma2)))
        if "chi2_ge" in mut:
            return bool(float(e2) >= k * float(f32(sigma2)))
        return bool(float(e2) > k * float(f32(sigma2)))


def view_dict(v):
    """A KF_VIEW record (or a dict of the same names) as float32 scalars / arrays."""
    names = ("Rcw", "tcw", "Ow", "fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf")
    return {k: (np.asarray(v[k], f32).reshape(-1) if k in ("Rcw", "tcw", "Ow") else f32(v[k])) for k in names}


def new_map_point(V1, V2, g1, g2, scale, sigma2, ratio_factor, mut=frozenset(), trace=None):
    """One pair of :285-433.  g: dict(x, y, u_right, octave, kx, ky, depth) of the feature.
    -> (status, source, x3D [3] float32 or None).  trace: a dict that receives the gate quantities."""
    mut = frozenset(mut)
    tr = trace if trace is not None else {}
    st1, st2 = bool(f32(g1["u_right"]) >= 0), bool(f32(g2["u_right"]) >= 0)
    one = f32(1.0)
    with np.errstate(all="ignore"):
        xn1 = [f32(f32(f32(g1["x"]) - V1["cx"]) * V1["invfx"]), f32(f32(f32(g1["y"]) - V1["cy"]) * V1["invfy"]), one]
        xn2 = [f32(f32(f32(g2["x"]) - V2["cx"]) * V2["invfx"]), f32(f32(f32(g2["y"]) - V2["cy"]) * V2["invfy"]), one]
        ray1, ray2 = rwc_mul(V1["Rcw"], xn1), rwc_mul(V2["Rcw"], xn2)
        cos_rays = f32(np.float64(dot64(ray1, ray2)) / np.float64(norm3(ray1) * norm3(ray2)))
        cps1 = cps2 = f32(cos_rays + one)
        if st1:
            cps1 = stereo_parallax_bound(V1["mb"], g1["depth"])
        if st2 and (not st1 or "else_if_to_if" in mut):
            cps2 = stereo_parallax_bound(V2["mb"], g2["depth"])
        cps = cps2 if cps2 < cps1 else cps1
        tr.update(cos_rays=cos_rays, cps1=cps1, cps2=cps2)
        below = cos_rays < cps
        far = True if "no_9998" in mut else float(cos_rays) < 0.9998
        if below and cos_rays > 0 and (st1 or st2 or far):
            src = SRC_TRI
            T1 = [list(V1["Rcw"][3 * r:3 * r + 3]) + [V1["tcw"][r]] for r in range(3)]
            T2 = [list(V2["Rcw"][3 * r:3 * r + 3]) + [V2["tcw"][r]] for r in range(3)]
            A = [[f32(f32(xn1[0] * T1[2][k]) - T1[0][k]) for k in range(4)],
                 [f32(f32(xn1[1] * T1[2][k]) - T1[1][k]) for k in range(4)],
                 [f32(f32(xn2[0] * T2[2][k]) - T2[0][k]) for k in range(4)],
                 [f32(f32(xn2[1] * T2[2][k]) - T2[1][k]) for k in range(4)]]
            tr["A"] = np.array(A, f32)
            h = jacobi_null4(A)
            if h[3] == 0 and "w_after_division" not in mut:
                return W_ZERO, src, None
            inv = f32(np.float64(1.0) / np.float64(h[3]))
            X = [f32(h[k] * inv) for k in range(3)]
        elif st1 and cps1 < cps2:
            src = SRC_STEREO1
            k = ("x", "y") if "undistorted_unproject" in mut else ("kx", "ky")
            X = unproject_stereo(V1, g1[k[0]], g1[k[1]], g1["depth"])
        elif st2 and cps2 < cps1:
            src = SRC_STEREO2
            k = ("x", "y") if "undistorted_unproject" in mut else ("kx", "ky")
            X = unproject_stereo(V2, g2[k[0]], g2[k[1]], g2["depth"])
        else:
            return LOW_PARALLAX, SRC_NONE, None
        z1, z2 = row_dot_add(V1, 2, X), row_dot_add(V2, 2, X)
        tr.update(X=np.array(X, f32), z1=z1, z2=z2)
        if (z1 < 0) if "z_lt" in mut else (z1 <= 0):
            return Z1, src, None
        if (z2 < 0) if "z_lt" in mut else (z2 <= 0):
            return Z2, src, None
        if reproj_fails(V1, V1["mbf"], X, z1, g1, sigma2[int(g1["octave"])], mut):
            return REPROJ1, src, None
        if reproj_fails(V2, V2["mbf"] if "mbf_kf2" in mut else V1["mbf"], X, z2, g2, sigma2[int(g2["octave"])], mut):
            return REPROJ2, src, None
        dist1 = f32(norm3([f32(X[k] - V1["Ow"][k]) for k in range(3)]))
        dist2 = f32(norm3([f32(X[k] - V2["Ow"][k]) for k in range(3)]))
        if dist1 == 0 or dist2 == 0:
            return ZERO_DIST, src, None
        ratio_dist = f32(dist2 / dist1)
        ratio_oct = f32(f32(scale[int(g1["octave"])]) / f32(scale[int(g2["octave"])]))
        rf = f32(ratio_factor)
        tr.update(ratio_dist=ratio_dist, ratio_oct=ratio_oct)
        if "ratio_swapped" in mut:
            bad = f32(ratio_oct * rf) < ratio_dist and ratio_oct > f32(ratio_dist * rf)
        else:
            bad = f32(ratio_dist * rf) < ratio_oct or ratio_dist > f32(ratio_oct * rf)
        if bad:
            return RATIO, src, None
        return ACCEPTED, src, np.array(X, f32)


def feature(kf, i):
    return {k: kf[k][i] for k in ("x", "y", "u_right", "octave", "kx", "ky", "depth")}


def create_new_map_points(kf1, kfs2, view1, views2, F12, epipole, scale, sigma2, ratio_factor, only_stereo,
                          mut=frozenset()):
    """Keyframes as tri_ref takes them, with has_mp, kx, ky (mvKeys[i].pt) and depth (mvDepth) besides.
    -> dict(match, status, source [nnb, n1], x3d [nnb, n1, 3] (NaN unless accepted), first_ok [n1], nmatches)."""
    mut = frozenset(mut)
    nnb, n1 = len(kfs2), len(kf1["node"])
    out = dict(match=np.full((nnb, n1), -1, np.int32), status=np.zeros((nnb, n1), np.int8),
               source=np.zeros((nnb, n1), np.int8), x3d=np.full((nnb, n1, 3), np.nan, f32),
               first_ok=np.full(n1, -1, np.int32), nmatches=np.zeros(nnb, np.int32))
    V1 = view_dict(view1)
    for j, kf2 in enumerate(kfs2):
        V2 = view_dict(views2[j])
        out["match"][j], out["nmatches"][j] = T.search_for_triangulation(
            kf1, kf2, kf1["has_mp"], kf2["has_mp"], F12[j], epipole[j], scale, sigma2, only_stereo, False)
        for i in range(n1):
            i2 = int(out["match"][j, i])
            if i2 < 0:
                continue
            st, src, X = new_map_point(V1, V2, feature(kf1, i), feature(kf2, i2), scale, sigma2, ratio_factor, mut)
            out["status"][j, i], out["source"][j, i] = st, src
            if st == ACCEPTED:
                out["x3d"][j, i] = X
                if out["first_ok"][i] < 0 or "last_accepted" in mut:
                    out["first_ok"][i] = j
    return out
