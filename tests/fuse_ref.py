"""CPU reference of the search half of ORBmatcher::Fuse (src/ORBmatcher.cc:826-951) with
KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:569-608), KeyFrame::IsInImage (:610-613),
MapPoint::PredictScale (src/MapPoint.cc:385-400) and the grid of Frame::AssignFeaturesToGrid
(src/Frame.cc:396-411, PosInGrid :560-571) as literal Python loops, float32 / float64 where the
reference has them.  Where the reference writes a * b + c in float, the fused form the project chose
is fmaf(): u = fma(fx, x, cx), ur = fma(-bf, invz, u), e2 = fma(ex, ex, ey * ey) and
then fma(er, er, .).  tests/test_fuse_ref.py pins this file on a hand-worked case; `mut` selects the
wrong readings tests/fuse_cases.py shows its cases notice."""
import math

import numpy as np

from tri_ref import fmaf

TH_LOW = 50
GRID_COLS, GRID_ROWS = 64, 48
f32, f64 = np.float32, np.float64

MUTATIONS = ("tie_le", "tie_last", "win_le", "level_plus1", "chi_double", "chi_swapped", "stereo_gt0", "best_lt_50",
             "range_raw", "scale_invariance", "grid_floor", "index_order", "dot_float")
# equivalent under the 1.2 / 8-level tables: no float e2 separates the two products (fuse_cases.chi_products_disagree)
EQUIVALENT = ("chi_double",)


class Cam:
    """coeb_camera and the context's level tables as the search reads them."""

    def __init__(self, fx=500.0, fy=500.0, cx=320.0, cy=240.0, bf=40.0, min_x=0.0, max_x=640.0, min_y=0.0, max_y=480.0,
                 scale_factor=1.2, nlevels=8):
        self.fx, self.fy, self.cx, self.cy, self.bf = f32(fx), f32(fy), f32(cx), f32(cy), f32(bf)
        self.min_x, self.max_x, self.min_y, self.max_y = f32(min_x), f32(max_x), f32(min_y), f32(max_y)
        self.nlevels = nlevels
        sf = float(f32(scale_factor))                       # ORBextractor: float tables, the factor a double
        scale, sigma2 = [f32(1.0)], [f32(1.0)]
        for _ in range(1, nlevels):
            scale.append(f32(float(scale[-1]) * sf))
            sigma2.append(f32(scale[-1] * scale[-1]))
        self.scale = np.array(scale, f32)
        self.inv_sigma2 = (f32(1.0) / np.array(sigma2, f32)).astype(f32)
        self.log_sf = f32(math.log(f64(f32(scale_factor))))
        self.grid_inv_w = f32(f32(GRID_COLS) / f32(self.max_x - self.min_x))
        self.grid_inv_h = f32(f32(GRID_ROWS) / f32(self.max_y - self.min_y))

    def tuple(self):
        return tuple(float(v) for v in (self.fx, self.fy, self.cx, self.cy, self.bf, self.min_x, self.max_x, self.min_y,
                                        self.max_y))


def c_round(x):
    """C round(): halves away from zero."""
    x = float(x)
    return int(math.floor(x + 0.5)) if x >= 0 else -int(math.floor(-x + 0.5))


def assign_features_to_grid(kf, cam, mut=frozenset()):
    """mGrid[ix][iy]: the features of a cell in index order; outside the grid: listed nowhere."""
    grid = [[[] for _ in range(GRID_ROWS)] for _ in range(GRID_COLS)]
    rnd = math.floor if "grid_floor" in mut else c_round
    for i in range(len(kf["x"])):
        px = rnd(f32(f32(f32(kf["x"][i]) - cam.min_x) * cam.grid_inv_w))
        py = rnd(f32(f32(f32(kf["y"][i]) - cam.min_y) * cam.grid_inv_h))
        if px < 0 or px >= GRID_COLS or py < 0 or py >= GRID_ROWS:
            continue
        grid[int(px)][int(py)].append(i)
    return grid


def features_in_area(kf, grid, cam, x, y, r, mut=frozenset(), ret=None):
    """KeyFrame::GetFeaturesInArea(x, y, r).  ret: a list that receives which early return was taken."""
    x, y, r = f32(x), f32(y), f32(r)
    out = []

    def early(k):
        if ret is not None:
            ret.append(k)
        return out

    x0 = max(0, int(math.floor(f32(f32(f32(x - cam.min_x) - r) * cam.grid_inv_w))))
    if x0 >= GRID_COLS:
        return early(1)
    x1 = min(GRID_COLS - 1, int(math.ceil(f32(f32(f32(x - cam.min_x) + r) * cam.grid_inv_w))))
    if x1 < 0:
        return early(2)
    y0 = max(0, int(math.floor(f32(f32(f32(y - cam.min_y) - r) * cam.grid_inv_h))))
    if y0 >= GRID_ROWS:
        return early(3)
    y1 = min(GRID_ROWS - 1, int(math.ceil(f32(f32(f32(y - cam.min_y) + r) * cam.grid_inv_h))))
    if y1 < 0:
        return early(4)
    for ix in range(x0, x1 + 1):
        for iy in range(y0, y1 + 1):
            for i in grid[ix][iy]:
                dx, dy = f32(f32(kf["x"][i]) - x), f32(f32(kf["y"][i]) - y)
                if "win_le" in mut:
                    ok = abs(dx) <= r and abs(dy) <= r
                else:
                    ok = abs(dx) < r and abs(dy) < r
                if ok:
                    out.append(i)
    if "index_order" in mut:
        out.sort()
    return out


def predict_scale(cam, max_distance, dist):
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = f32(f32(max_distance) / f32(dist))
        s = int(math.ceil(f32(f32(math.log(f64(ratio))) / cam.log_sf)))
    return 0 if s < 0 else (cam.nlevels - 1 if s >= cam.nlevels else s)


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))).sum())


def project(cam, Rcw, tcw, P):
    """(z, invz, u, v, ur) of :854-871; None where z < 0."""
    R = np.asarray(Rcw, f32).reshape(3, 3)
    t = np.asarray(tcw, f32).reshape(3)
    P = np.asarray(P, f32).reshape(3)
    Pc = []
    for k in range(3):                                   # cv::Mat small gemm: float products, tcw added in double
        s = f32(f32(R[k, 0] * P[0]) + f32(R[k, 1] * P[1]))
        s = f32(s + f32(R[k, 2] * P[2]))
        Pc.append(f32(f64(s) + f64(t[k])))
    if Pc[2] < f32(0.0):
        return None
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invz = f32(f32(1.0) / Pc[2])
        x, y = f32(Pc[0] * invz), f32(Pc[1] * invz)
        u, v = fmaf(cam.fx, x, cam.cx), fmaf(cam.fy, y, cam.cy)
        ur = fmaf(-cam.bf, invz, u)
    return Pc[2], invz, u, v, ur


def fuse_point(kf, grid, cam, Rcw, tcw, Ow, P, Pn, max_distance, min_distance, desc, th, mut=frozenset(), trace=None):
    """One pass of the loop body :853-950 -> (bestIdx, bestDist); bestIdx is the reference's (set
    whenever a candidate was accepted).  trace: a dict that receives 'why' (the test that ended the
    point, or 'compared') and the counts 'stereo' / 'mono' of candidates that reached a chi test."""
    mut = frozenset(mut)
    tr = {} if trace is None else trace
    tr.update(why="", stereo=0, mono=0, ndist=0, ret=[])
    pr = project(cam, Rcw, tcw, P)
    if pr is None:
        tr["why"] = "z"
        return -1, 256
    _, _, u, v, ur = pr
    if not (u >= cam.min_x and u < cam.max_x and v >= cam.min_y and v < cam.max_y):
        tr["why"] = "image"
        return -1, 256
    P, Pn, Ow = np.asarray(P, f32), np.asarray(Pn, f32), np.asarray(Ow, f32)
    PO = [f32(P[k] - Ow[k]) for k in range(3)]
    ss = 0.0
    for k in range(3):                                   # cv::norm: squares summed in double
        ss += float(PO[k]) * float(PO[k])
    dist3D = f32(math.sqrt(ss))
    maxd, mind = f32(max_distance), f32(min_distance)
    lo, hi = (mind, maxd) if "range_raw" in mut else (f32(f32(0.8) * mind), f32(f32(1.2) * maxd))
    if dist3D < lo or dist3D > hi:
        tr["why"] = "range"
        return -1, 256
    dot = 0.0
    for k in range(3):                                   # Mat::dot: double accumulation
        dot += float(PO[k]) * float(Pn[k])
    if "dot_float" in mut:
        bad = f32(dot) < f32(f32(0.5) * dist3D)
    else:
        bad = dot < 0.5 * float(dist3D)
    if bad:
        tr["why"] = "angle"
        return -1, 256
    level = predict_scale(cam, f32(f32(1.2) * maxd) if "scale_invariance" in mut else maxd, dist3D)
    radius = f32(f32(th) * cam.scale[level])
    cand = features_in_area(kf, grid, cam, u, v, radius, mut, tr["ret"])
    if not cand:
        tr["why"] = "empty"
        return -1, 256
    best_dist, best_idx = 256, -1
    for idx in cand:
        lvl = int(kf["octave"][idx])
        if lvl < level - 1 or lvl > level + (1 if "level_plus1" in mut else 0):
            continue
        kur = f32(kf["u_right"][idx])
        stereo = kur > 0 if "stereo_gt0" in mut else kur >= 0
        ex, ey = f32(u - f32(kf["x"][idx])), f32(v - f32(kf["y"][idx]))
        e2 = fmaf(ex, ex, f32(ey * ey))
        if stereo:
            er = f32(ur - kur)
            e2 = fmaf(er, er, e2)
        tr["stereo" if stereo else "mono"] += 1
        bound = (5.99 if stereo else 7.8) if "chi_swapped" in mut else (7.8 if stereo else 5.99)
        if "chi_double" in mut:
            chi = float(e2) * float(cam.inv_sigma2[lvl])
        else:
            chi = float(f32(e2 * cam.inv_sigma2[lvl]))
        if chi > bound:
            continue
        dist = hamming(desc, kf["desc"][idx])
        tr["ndist"] += 1
        if "tie_le" in mut:
            better = dist <= best_dist
        elif "tie_last" in mut:
            better = dist < best_dist or (dist == best_dist and best_idx >= 0)
        else:
            better = dist < best_dist
        if better:
            best_dist, best_idx = dist, idx
    tr["why"] = "compared" if tr["ndist"] else "filtered"
    return best_idx, best_dist


def fuse_search(kf, cam, Rcw, tcw, Ow, pts, th=3.0, first=0, count=None, skip=None, mut=frozenset(), traces=None):
    """What coeb_kfdb_fuse_search returns for one job: (best_idx [count], best_dist [count]).
    kf: dict(desc [n, 32], x, y, octave, u_right).  pts: dict(valid, world_pos, normal, max_distance,
    min_distance, descriptor)."""
    mut = frozenset(mut)
    n = len(pts["valid"])
    count = n - first if count is None else count
    grid = assign_features_to_grid(kf, cam, mut)
    bi, bd = np.full(count, -1, np.int32), np.full(count, 256, np.int32)
    for k in range(count):
        i = first + k
        tr = {}
        if traces is not None:
            traces.append(tr)
        if not pts["valid"][i] or (skip is not None and skip[k]):
            tr["why"] = "skipped"
            continue
        idx, dist = fuse_point(kf, grid, cam, Rcw, tcw, Ow, pts["world_pos"][i], pts["normal"][i], pts["max_distance"][i],
                               pts["min_distance"][i], pts["descriptor"][i], th, mut, tr)
        bd[k] = dist
        limit = dist < TH_LOW if "best_lt_50" in mut else dist <= TH_LOW
        bi[k] = idx if limit else -1
    return bi, bd
