"""CPU reference of ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:657-824) and
CheckDistEpipolarLine (:140-157) as literal Python loops in float32 / float64, for one pair of
keyframes.  F12 and the epipole are inputs (the caller computes them, :664-670).  The float forms
are those of the reference binary: the fused multiply-adds it shows are fmaf()
here, everything else is one float32 operation per step.  tests/test_tri_ref.py pins this file on a
hand-worked case; `mut` selects the wrong readings tests/tri_cases.py shows its cases notice."""
import math
import struct

import numpy as np

from bow_ref import csr, hamming, three_maxima  # noqa: F401  (csr: the CSR order the lists are walked in)

TH_LOW = 50
HISTO_LENGTH = 30
f32 = np.float32

MUTATIONS = ("tie_first", "dist_ge_50", "best_before_geometry", "epipole_one_stereo", "epipole_le", "chi2_float",
             "no_has_mp2", "no_has_mp1", "stereo_one_side", "claim", "rot_rint", "rot_no_360", "rot_bin30_kept")
EQUIVALENT = ("no_den_guard",)          # x / 0 is inf or nan, and neither is < the bound


def fmaf(a, b, c):
    """float32 fused multiply-add, rounded once.  The product of two float32 is exact in float64;
    the sum is rounded to odd there (53 >= 2 * 24 + 2 bits), so the final rounding is the only one."""
    a, b, c = float(a), float(b), float(c)
    p = a * b
    s = p + c
    if math.isfinite(s):
        bb = s - p
        err = (p - (s - bb)) + (c - bb)                 # TwoSum: p + c = s + err exactly
        if err != 0.0 and not struct.unpack("<q", struct.pack("<d", s))[0] & 1:
            s = math.nextafter(s, math.inf if err > 0 else -math.inf)
    return f32(s)


def epipolar_line(x1, y1, F):
    """(a, b, c, den) of l = x1' F12 (:143-149)."""
    F = np.asarray(F, f32).reshape(3, 3)
    x1, y1 = f32(x1), f32(y1)
    a = f32(fmaf(x1, F[0, 0], f32(y1 * F[1, 0])) + F[2, 0])
    b = f32(fmaf(x1, F[0, 1], f32(y1 * F[1, 1])) + F[2, 1])
    c = f32(fmaf(y1, F[1, 2], f32(x1 * F[0, 2])) + F[2, 2])
    den = fmaf(a, a, f32(b * b))
    return a, b, c, den


def check_dist_epipolar_line(x1, y1, x2, y2, F, sigma2, mut=frozenset()):
    a, b, c, den = epipolar_line(x1, y1, F)
    num = f32(fmaf(b, f32(y2), f32(a * f32(x2))) + c)
    if den == 0 and "no_den_guard" not in mut:
        return False
    with np.errstate(divide="ignore", invalid="ignore"):
        dsqr = f32(f32(num * num) / den)
    if "chi2_float" in mut:
        return bool(dsqr < f32(f32(3.84) * f32(sigma2)))
    return bool(float(dsqr) < 3.84 * float(f32(sigma2)))


def near_epipole(ex, ey, x2, y2, scale, mut=frozenset()):
    """distex * distex + distey * distey < 100 * mvScaleFactors[octave] (:745-748)."""
    dx, dy = f32(f32(ex) - f32(x2)), f32(f32(ey) - f32(y2))
    d2 = fmaf(dx, dx, f32(dy * dy))
    r = f32(f32(100.0) * f32(scale))
    return bool(d2 <= r) if "epipole_le" in mut else bool(d2 < r)


def rot_bin(a1, a2, mut=frozenset()):
    """:767-773.  HISTO_LENGTH: no bin (the reference's assert), never kept."""
    rot = f32(f32(a1) - f32(a2))
    if rot < 0.0 and "rot_no_360" not in mut:
        rot = f32(rot + f32(360.0))
    fb = float(f32(rot * (f32(1.0) / f32(HISTO_LENGTH))))
    if "rot_rint" in mut:
        b = int(np.rint(fb))
    else:                                   # C round(): halves away from zero
        b = int(math.floor(fb + 0.5)) if fb >= 0 else -int(math.floor(-fb + 0.5))
    if b == HISTO_LENGTH and "rot_bin30_kept" not in mut:
        b = 0
    return b if 0 <= b < HISTO_LENGTH else HISTO_LENGTH


def feature_lists(node):
    """mFeatVec: node id -> the features it lists, ascending (the order csr() stores)."""
    fv = {}
    for i, nd in enumerate(node):
        if nd >= 0:
            fv.setdefault(int(nd), []).append(i)
    return fv


def search_for_triangulation(kf1, kf2, has_mp1, has_mp2, F12, epipole, scale, sigma2, only_stereo, check_ori,
                             mut=frozenset(), trace=None):
    """kf: dict(desc [n, 32] u8, node [n], angle [n], x [n], y [n], octave [n], u_right [n]).
    -> (vMatches12 [n1] int32, nmatches).  trace: a list that receives (idx1, idx2, what) for every
    candidate looked at, what in {"has_mp", "mono", "dist", "epipole", "line", "accepted"}."""
    mut = frozenset(mut)
    n1 = len(kf1["node"])
    ex, ey = f32(epipole[0]), f32(epipole[1])
    match = np.full(n1, -1, np.int32)
    matched2 = set()
    rot_hist = [[] for _ in range(HISTO_LENGTH + 1)]
    nmatches = 0
    fv1, fv2 = feature_lists(kf1["node"]), feature_lists(kf2["node"])

    def note(i1, i2, what):
        if trace is not None:
            trace.append((i1, i2, what))

    for nd in sorted(fv1):
        if nd not in fv2:
            continue
        for idx1 in fv1[nd]:
            if has_mp1[idx1] and "no_has_mp1" not in mut:
                continue
            stereo1 = bool(f32(kf1["u_right"][idx1]) >= 0)
            if only_stereo and not stereo1:
                continue
            best_dist, best_idx2 = TH_LOW, -1
            for idx2 in fv2[nd]:
                if idx2 in matched2 or (has_mp2[idx2] and "no_has_mp2" not in mut):
                    note(idx1, idx2, "has_mp")
                    continue
                stereo2 = bool(f32(kf2["u_right"][idx2]) >= 0)
                if only_stereo and not stereo2 and "stereo_one_side" not in mut:
                    note(idx1, idx2, "mono")
                    continue
                dist = int(hamming(kf1["desc"][idx1], kf2["desc"][idx2]))
                if (dist >= TH_LOW if "dist_ge_50" in mut else dist > TH_LOW) or \
                        (dist >= best_dist and best_idx2 >= 0 if "tie_first" in mut else dist > best_dist):
                    note(idx1, idx2, "dist")
                    continue
                if "best_before_geometry" in mut:
                    best_dist = dist
                oct2 = int(kf2["octave"][idx2])
                mono = (not (stereo1 and stereo2)) if "epipole_one_stereo" in mut else (not stereo1 and not stereo2)
                if mono and near_epipole(ex, ey, kf2["x"][idx2], kf2["y"][idx2], scale[oct2], mut):
                    note(idx1, idx2, "epipole")
                    continue
                if check_dist_epipolar_line(kf1["x"][idx1], kf1["y"][idx1], kf2["x"][idx2], kf2["y"][idx2], F12,
                                            sigma2[oct2], mut):
                    best_idx2, best_dist = idx2, dist
                    note(idx1, idx2, "accepted")
                else:
                    note(idx1, idx2, "line")
            if best_idx2 >= 0:
                match[idx1] = best_idx2
                if "claim" in mut:
                    matched2.add(best_idx2)
                nmatches += 1
                if check_ori:
                    rot_hist[rot_bin(kf1["angle"][idx1], kf2["angle"][best_idx2], mut)].append(idx1)
    if check_ori:
        keep = three_maxima([len(h) for h in rot_hist[:HISTO_LENGTH]])
        for b in range(HISTO_LENGTH + 1):
            if b in keep:
                continue
            for i in rot_hist[b]:
                match[i] = -1
                nmatches -= 1
    return match, nmatches


def matched_pairs(match):
    """vMatchedPairs (:816-821)."""
    return [(i, int(m)) for i, m in enumerate(match) if m >= 0]
