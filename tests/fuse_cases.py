"""Directed inputs of the Fuse search (tests/fuse_ref.py is the model, tests/test_fuse_ref.py shows
what every case is for, tests/test_gpu_fuse_directed.py runs them on the device).

Unless a case says otherwise the pose is the identity (Rcw = I, tcw = Ow = 0) and a point lies at
depth 1, so invz = 1 and u = fma(fx, X, cx); at() solves X and Y over neighbouring floats until the
model's own projection lands on the requested pixel exactly.  Descriptors are built bit by bit:
low(d) has bits 0 .. d-1 set, so the distance to the all-zero point descriptor is d.  A case is a
dict: cam, kfs (keyframes as fuse_ref takes them), pts, jobs (dicts: kf, Rcw, tcw, Ow, first, count,
skip), th and mutants: the wrong readings of fuse_ref.MUTATIONS that have to change its output."""
import functools
import math

import numpy as np

import fuse_ref as F

f32 = np.float32
I3, Z3 = np.eye(3, dtype=f32), np.zeros(3, f32)
LANES = 4                                   # kFuseLanes of k_fuse: the lanes that share a point's window columns


def low(d):
    b = np.zeros(256, np.uint8)
    b[:d] = 1
    return np.packbits(b, bitorder="little")


def near(v, k):
    """v and its k float32 neighbours on either side, nearest first."""
    v = f32(v)
    out, lo, hi = [v], v, v
    for _ in range(k):
        lo, hi = np.nextafter(lo, f32(-np.inf)), np.nextafter(hi, f32(np.inf))
        out += [lo, hi]
    return out


def up(v, k=1):
    v = f32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, f32(np.inf if k > 0 else -np.inf))
    return v


class KF:
    def __init__(self):
        self.rows = []

    def add(self, x, y, octave=0, ur=-1.0, d=0):
        self.rows.append((x, y, octave, ur, low(d) if np.isscalar(d) else d))
        return len(self.rows) - 1

    def done(self):
        r = self.rows
        col = lambda k, dt: np.array([q[k] for q in r], dt)        # noqa: E731
        return dict(x=col(0, f32), y=col(1, f32), octave=col(2, np.int32), u_right=col(3, f32),
                    desc=np.array([q[4] for q in r], np.uint8).reshape(len(r), 32))


def at(cam, u, v, z=1.0):
    """World point (identity pose) whose model projection is exactly (u, v)."""
    u, v, z = f32(u), f32(v), f32(z)
    X0, Y0 = f32(f32(u - cam.cx) / cam.fx * z), f32(f32(v - cam.cy) / cam.fy * z)
    for X in near(X0, 200):
        pr = F.project(cam, I3, Z3, (X, 0, z))
        if pr[2] == u:
            break
    else:
        raise AssertionError("no X projects to u = %r" % u)
    for Y in near(Y0, 200):
        pr = F.project(cam, I3, Z3, (X, Y, z))
        if pr[3] == v:
            return np.array([X, Y, z], f32)
    raise AssertionError("no Y projects to v = %r" % v)


def dist_of(P, Ow=Z3):
    PO = [f32(f32(P[k]) - f32(Ow[k])) for k in range(3)]
    return f32(math.sqrt(sum(float(c) * float(c) for c in PO)))


class Pts:
    def __init__(self, cam):
        self.cam, self.rows = cam, []

    def add(self, P, level=0, d=0, valid=1, Pn=None, maxd=None, mind=None):
        """The point P, seen head-on, whose mfMaxDistance predicts `level` (ratio = 1.2^(level - 0.5))."""
        P = np.asarray(P, f32)
        dist = dist_of(P)
        if maxd is None:
            maxd = f32(float(dist) * 1.2 ** (level - 0.5))
        if mind is None:
            mind = f32(float(maxd) / 4.0)
        if Pn is None:
            Pn = (P / dist).astype(f32) if dist > 0 else np.array([0, 0, 1], f32)
        self.rows.append((valid, P, np.asarray(Pn, f32), f32(maxd), f32(mind), low(d) if np.isscalar(d) else d))
        return len(self.rows) - 1

    def px(self, u, v, level=0, d=0, **kw):
        return self.add(at(self.cam, u, v), level, d, **kw)

    def done(self):
        r = self.rows
        n = len(r)
        return dict(valid=np.array([q[0] for q in r], np.uint8), world_pos=np.array([q[1] for q in r], f32).reshape(n, 3),
                    normal=np.array([q[2] for q in r], f32).reshape(n, 3), max_distance=np.array([q[3] for q in r], f32),
                    min_distance=np.array([q[4] for q in r], f32),
                    descriptor=np.array([q[5] for q in r], np.uint8).reshape(n, 32))


def job(kf=0, first=0, count=None, skip=None, Rcw=I3, tcw=Z3, Ow=Z3):
    return dict(kf=kf, first=first, count=count, skip=skip, Rcw=np.asarray(Rcw, f32), tcw=np.asarray(tcw, f32),
                Ow=np.asarray(Ow, f32))


def _case(cam, kfs, pts, mutants=(), jobs=None, th=3.0):
    kfs = [k.done() if isinstance(k, KF) else k for k in (kfs if isinstance(kfs, list) else [kfs])]
    pts = pts.done() if isinstance(pts, Pts) else pts
    return dict(cam=cam, kfs=kfs, pts=pts, jobs=jobs or [job()], th=th, mutants=tuple(mutants))


# fx = fy = 512: X = (u - cx) / 512 is exact for every pixel coordinate with a few fraction bits, so at() hits it
CAM = F.Cam(fx=512.0, fy=512.0)
CAM_B = F.Cam(fx=512.0, fy=512.0, min_x=10.0, max_x=600.0, min_y=20.0, max_y=440.0)     # bounds that are not (0, w, 0, h)


def c_depth():
    """z negative, zero, tiny positive outside the image, and tiny positive inside it (X scaled with z)."""
    kf, p = KF(), Pts(CAM)
    kf.add(320, 240, d=3)
    p.add((0, 0, -1.0), maxd=2.0, mind=0.1)
    p.add((0, 0, 0.0), maxd=2.0, mind=1e-3)                 # invz = inf, x = nan
    p.add((0.5, 0, 0.0), maxd=2.0, mind=0.1)                # x = inf
    p.add((0.1, 0, 1e-30), maxd=2.0, mind=0.05)             # u overflows the image
    z = f32(2.0 ** -60)
    p.add((0, 0, z), maxd=f32(z * f32(0.95)), mind=f32(z / 2))   # still projects to (cx, cy), level 0
    p.add((0, 0, -0.0), maxd=2.0, mind=1e-3)                # -0.0 < 0 is false: goes on, then out of the image
    return _case(CAM, kf, p)


def c_image_bounds():
    """u, v exactly on min (in) and on max (out) under CAM_B; a feature under every projection."""
    kf, p = KF(), Pts(CAM_B)
    for u, v in ((10, 100), (600, 100), (300, 20), (300, 440), (up(600, -1), 100), (300, up(440, -1)), (10 - 2.0 ** -10, 100)):
        kf.add(u, v, d=1)
        p.px(u, v)
    return _case(CAM_B, kf, p)


def c_range():
    """dist3D on both invariance bounds and one ulp outside each; a distance only the 0.8 / 1.2 admit."""
    kf, p = KF(), Pts(CAM)
    for o in range(8):
        kf.add(320, 240, octave=o, d=2)                     # whatever level the distances predict
    P = np.array([0, 0, 1], f32)
    for m in near(f32(1.0 / 0.8), 50):                      # 0.8f * mind == 1 exactly
        if f32(f32(0.8) * m) == f32(1.0):
            mind = m
            break
    while f32(f32(0.8) * up(mind)) == f32(1.0):
        mind = up(mind)
    p.add(P, maxd=3.0, mind=mind)                           # dist == bound: in
    p.add(P, maxd=3.0, mind=up(mind))                       # bound one ulp above dist: out
    for m in near(f32(1.0 / 1.2), 50):
        if f32(f32(1.2) * m) == f32(1.0):
            maxd = m
            break
    while f32(f32(1.2) * up(maxd, -1)) == f32(1.0):
        maxd = up(maxd, -1)
    p.add(P, maxd=maxd, mind=0.1)
    p.add(P, maxd=up(maxd, -1), mind=0.1)
    p.add(P, maxd=0.9, mind=0.1)                            # mfMaxDistance < dist <= 1.2 * it
    p.add(P, maxd=3.0, mind=1.1)                            # 0.8 * it <= dist < mfMinDistance
    return _case(CAM, kf, p, ("range_raw",))


def c_angle():
    """PO.Pn exactly 0.5 * dist3D (kept), one ulp less (dropped), and 0.5 - 2^-40 where only the
    double comparison drops it."""
    kf, p = KF(), Pts(CAM)
    kf.add(320, 240, d=2)
    p.add((0, 0, 1), Pn=(0, 0, 0.5), maxd=1.0, mind=0.5)
    p.add((0, 0, 1), Pn=(0, 0, up(0.5, -1)), maxd=1.0, mind=0.5)
    e = f32(2.0 ** -20)
    p.add((e, 0, 1), Pn=(-e, 0, 0.5), maxd=1.0, mind=0.5)
    assert dist_of((e, 0, 1)) == f32(1.0)
    return _case(CAM, kf, p, ("dot_float",))


def _maxd_step(dist, k):
    """The largest mfMaxDistance whose unclamped level is k, searched upward from the middle of the step."""
    def lvl(m):
        ratio = f32(f32(m) / f32(dist))
        return f32(f32(math.log(np.float64(ratio))) / CAM.log_sf)
    m = f32(float(dist) * 1.2 ** (k - 0.5))
    step = f32(float(m) * 2.0 ** -6)
    while step > 0 and up(m) != m:
        n = f32(m + step)
        if n == m:
            break
        if math.ceil(lvl(n)) <= k:
            m = n
        else:
            step = f32(step / 2)
    return m, lvl(m)


def c_predict_scale():
    """The step of ceil(log(ratio) / logScale) between levels 2 and 3, the quotient exactly 3.0 (asserted)
    and one float above, both clamps, level 0 with level-0 and level-1 features, features at pred - 2 ..
    pred + 1, and a ratio that the 1.2f invariance distance would move one level up."""
    kf, p = KF(), Pts(CAM)
    for o in range(8):
        kf.add(100, 100, octave=o, d=20 - o)                # one feature per level under (100, 100), the coarser the nearer
    P = at(CAM, 100, 100)
    dist = dist_of(P)
    m, q = _maxd_step(dist, 2)
    p.add(P, maxd=m, mind=0.1)                              # level 2: features 1, 2 -> 2
    p.add(P, maxd=up(m), mind=0.1)                          # level 3: features 2, 3 -> 3
    p.add(P, maxd=f32(dist * f32(0.9)), mind=0.1)           # ratio < 1: clamped to 0
    p.add(P, maxd=f32(float(dist) * 1.2 ** 9.5), mind=0.1)  # clamped to 7: features 6, 7 -> 7
    p.add(P, level=0)                                       # window [-1, 0]: feature 0 only
    p.add(P, level=5)                                       # features at 3 .. 6: 4 and 5 pass -> 5; 6 is nearer
    p.add(P, maxd=f32(float(dist) * 1.2 ** 3.9), mind=0.1)  # level 4; from 1.2 * maxd it would be 5
    # at (40, 100) a float mfMaxDistance puts the quotient on 3.0 exactly (at (100, 100) the last float of
    # level 2 gives 1.9999999): ceil keeps level 3, the next float is level 4
    for o in range(8):
        kf.add(40, 100, octave=o, d=20 - o)
    P3 = at(CAM, 40, 100)
    m3, q3 = _maxd_step(dist_of(P3), 3)
    assert float(q3) == 3.0
    p.add(P3, maxd=m3, mind=0.1)                            # feature 8 + 3
    p.add(P3, maxd=up(m3), mind=0.1)                        # feature 8 + 4
    return _case(CAM, kf, p, ("level_plus1", "scale_invariance"))


def c_window_edge():
    """|dx| exactly r (out) and one ulp inside (in), the same along y.  th = 2, r = 2 at level 0: at
    th = 3 the mono chi-square bound (2.45 px at level 0) is inside the window and hides its edge."""
    kf, p = KF(), Pts(CAM)
    kf.add(322, 240, d=1)
    kf.add(up(322, -1), 240, d=9)
    kf.add(120, 202, d=1)
    kf.add(120, up(198, 1), d=9)
    p.px(320, 240)
    p.px(120, 200)
    return _case(CAM, kf, p, ("win_le",), th=2.0)


def c_grid_edges():
    """Windows clipped at the four edges and corners of the grid, under CAM_B; th = 0 next to max_x and
    max_y, where the float product rounds the first cell up to 64 / 48 (early returns 1 and 3; the
    other two cannot be reached from Fuse, which has u >= min_x, v >= min_y and r >= 0)."""
    kf, p = KF(), Pts(CAM_B)
    for u, v in ((11, 21), (594, 21), (11, 435), (594, 435), (300, 21), (300, 435), (11, 200), (594, 200)):
        kf.add(u, v, d=4)                                   # 594 and 435 round into the last column / row
        p.px(u + 0.5, v + 0.5)
    return _case(CAM_B, kf, p)


@functools.lru_cache(maxsize=None)
def _rounding_cam():
    """Bounds (0, w, 0, h) under which the last float below w, times the cell-width inverse, rounds to 64.0
    (and the last below h to 48.0): with th = 0 GetFeaturesInArea takes its first / third early return."""
    w = h = None
    for k in range(600, 1300):
        cam = F.Cam(fx=512.0, fy=512.0, max_x=float(k), max_y=float(k))
        if w is None and f32(up(k, -1) * cam.grid_inv_w) >= 64:
            w = k
        if h is None and f32(up(k, -1) * cam.grid_inv_h) >= 48:
            h = k
    assert w and h
    return F.Cam(fx=512.0, fy=512.0, max_x=float(w), max_y=float(h))


def c_early_returns():
    cam = _rounding_cam()
    kf, p = KF(), Pts(cam)
    kf.add(float(cam.max_x) - 1, 100, d=1)
    kf.add(100, float(cam.max_y) - 1, d=1)
    p.px(up(cam.max_x, -1), 100)
    p.px(100, up(cam.max_y, -1))
    return _case(cam, kf, p, th=0.0)


def c_outside_grid():
    """round((x - min_x) * inv_w) = 64 or -1: listed nowhere, although inside the window; x = -4 rounds
    to cell 0 and is listed."""
    kf, p = KF(), Pts(CAM)
    kf.add(636, 100, d=1)                                   # round(63.6) = 64; floor would list it
    kf.add(634, 100, d=7)                                   # round(63.4) = 63
    kf.add(100, 476, d=1)                                   # round(47.6) = 48
    kf.add(-6, 300, octave=3, d=1)                          # round(-0.6) = -1
    kf.add(-4, 300, octave=3, d=5)                          # round(-0.4) = 0
    kf.add(1.5, 300, octave=6, d=9)
    p.px(635, 100)
    p.px(100, 475)
    p.px(0, 300, level=3)                                   # r = 5.18: -4 is inside, -6 is not
    p.px(1, 300, level=6)                                   # r = 8.96: -6 is inside the window, in no cell
    return _case(CAM, kf, p, ("grid_floor",))


def chi_products_disagree(cam):
    """(level, bound, e2) for every float e2 whose float product e2 * invSigma2[level] and whose double
    product fall on different sides of 5.99 or 7.8.  A float product is a float, so they can differ only
    where the exact product lies within half an ulp of the bound: e2 within a few ulps of bound / invSigma2.
    The result depends on the level tables: fuse_ref.EQUIVALENT holds for the 1.2 / 8-level pyramid only, and
    tests/test_fuse_ref.py has to be rerun, with a directed case added, for any other pyramid setting."""
    out = []
    for lvl in range(cam.nlevels):
        isg = cam.inv_sigma2[lvl]
        for bound in (5.99, 7.8):
            for e2 in near(f32(bound / float(isg)), 8):
                if (float(f32(e2 * isg)) > bound) != (float(e2) * float(isg) > bound):
                    out.append((lvl, bound, e2))
    return out


def c_chi():
    """Mono and stereo e2 * invSigma2 on both sides of 5.99 / 7.8, a stereo error between the two
    bounds, u_right = 0 (stereo) and -1 (mono) and a pure right-coordinate error.  Under the 1.2 / 8-level
    tables no float e2 puts the float product and the double product on different sides of a bound
    (chi_products_disagree is empty; tests/test_fuse_ref.py checks it), so that reading has no case."""
    cam = CAM
    kf, p = KF(), Pts(cam)
    ur0 = F.project(cam, I3, Z3, at(cam, 100, 100))[4]     # the points' own ur = u - bf
    # level-0 points at (100 k, 100): mono 2.4 px off (5.76 <= 5.99) / 2.5 px (6.25 >)
    kf.add(100, 102.4, d=1)
    kf.add(200, 102.5, d=1)
    # stereo: 2.7 px off (7.29 <= 7.8; > 5.99) / 2.8 px (7.84 >)
    kf.add(300, 102.7, ur=300 - 40, d=1)
    kf.add(400, 102.8, ur=400 - 40, d=1)
    # u_right = 0: a stereo feature with er = ur - 0 = 460: rejected; as mono it would pass
    kf.add(500, 101, ur=0.0, d=1)
    # pure er error: ex = ey = 0, er = 2.7 / 2.8
    kf.add(100, 300, ur=100 - 40 - 2.7, d=1)
    kf.add(200, 300, ur=200 - 40 - 2.8, d=1)
    for u in (100, 200, 300, 400, 500):
        p.px(u, 100)
    p.px(100, 300)
    p.px(200, 300)
    assert ur0 == f32(60.0)
    return _case(cam, kf, p, ("chi_swapped", "stereo_gt0"))


def c_ties():
    """Equal minima in two grid columns where index order and cell order disagree; equal minima inside
    one cell; a nearer candidate that fails the chi-square test and shadows nothing."""
    kf, p = KF(), Pts(CAM)
    kf.add(106, 100, d=5)          # column 11 (round(10.6)), index 0
    kf.add(103, 100, d=5)          # column 10, index 1: first in cell order
    kf.add(300, 200, d=5)          # one cell, indices 2, 3
    kf.add(300.5, 200.5, d=5)
    kf.add(500, 102.6, d=0)        # nearer, but 2.6 px off: chi 6.76 > 5.99
    kf.add(500, 101, d=6)
    p.px(104.5, 100, level=1)
    p.px(300, 200)
    p.px(500, 100)
    return _case(CAM, kf, p, ("index_order", "tie_le", "tie_last"))


def c_best_dist():
    """bestDist 50 | 51, and every candidate at distance 256."""
    kf, p = KF(), Pts(CAM)
    kf.add(100, 100, d=50)
    kf.add(200, 100, d=51)
    kf.add(300, 100, d=256)
    kf.add(301, 100, d=256)
    for u in (100, 200, 300):
        p.px(u, 100)
    return _case(CAM, kf, p, ("best_lt_50",))


def c_lane_groups():
    """Windows of LANES - 1 .. 2 LANES + 1 grid columns (th chosen per case through the level) and
    cells of LANES - 1 .. 2 LANES + 1 candidates; the winner sits in the last column / last position."""
    kf, p = KF(), Pts(CAM)
    # cells with 3, 4, 5, 8, 9 features around (100 + 60 k, 300); the last is the nearest
    for k, cnt in enumerate((LANES - 1, LANES, LANES + 1, 2 * LANES, 2 * LANES + 1)):
        for j in range(cnt):
            kf.add(100 + 60 * k + 0.1 * j, 300, d=20 - j)
        p.px(100 + 60 * k, 300)
    # a row of features 10 px apart, level 7; points with growing radius through th (set by the case):
    for j in range(12):
        kf.add(200 + 10 * j, 100, octave=7, d=30 - j)
    p.px(255, 100, level=7)                                 # r = 50.2: columns 20 .. 31, 12 columns over 4 lanes
    for u in (13, 22):                                      # clipped at the left edge: columns 0 .. 7 and 0 .. 8
        kf.add(u + 3, 200, octave=7, d=3)
        kf.add(u + 70, 200, octave=7, d=1)                  # outside the window
        p.px(u, 200, level=7)
    return _case(CAM, kf, p, th=14.0)


def c_wide_windows():
    """th = 5 at level 7 (r = 17.9): windows of LANES - 1, LANES and LANES + 1 columns at the left edge
    and inside, over a row of level-7 features 4 px apart; the chi-square bound (8.8 px) picks among them."""
    kf, p = KF(), Pts(CAM)
    for j in range(31):
        kf.add(4 * j, 100, octave=7, d=40 - (j * 7) % 31)
    for u in (2, 12, 22, 60, 117):
        p.px(u, 100, level=7)
    return _case(CAM, kf, p, th=5.0)


def c_jobs():
    """valid 0, skip bytes, an empty keyframe, a zero-count job, a repeated slot, overlapping ranges and
    a second pose."""
    a, b, e, p = KF(), KF(), KF(), Pts(CAM)
    for k in range(6):
        a.add(100 + 50 * k, 100, d=1 + k)
        b.add(100 + 50 * k, 101, d=11 + k)
        p.px(100 + 50 * k, 100, valid=0 if k == 2 else 1)
    skip = np.array([0, 1, 0, 0], np.uint8)
    t = np.array([0.01, 0, 0], f32)                          # a shifted camera: u moves by 5 px
    jobs = [job(0), job(1, 1, 4, skip), job(2), job(0, 3, 0), job(0, 2, 4), job(1, 0, 3, tcw=t, Ow=-t), job(2, 5, 1)]
    return _case(CAM, [a, b, e], p, jobs=jobs)


def c_128_jobs():
    kf, p = KF(), Pts(CAM)
    for k in range(8):
        kf.add(100 + 50 * k, 100, d=1 + k)
        p.px(100 + 50 * k, 100)
    jobs = [job(0, j % 8, 1 + (j % 3) if j % 8 + 1 + (j % 3) <= 8 else 1) for j in range(128)]
    return _case(CAM, kf, p, jobs=jobs)


CASES = dict(depth=c_depth, image_bounds=c_image_bounds, range=c_range, angle=c_angle, predict_scale=c_predict_scale,
             window_edge=c_window_edge, grid_edges=c_grid_edges, early_returns=c_early_returns, outside_grid=c_outside_grid,
             chi=c_chi, ties=c_ties, best_dist=c_best_dist, lane_groups=c_lane_groups, wide_windows=c_wide_windows,
             jobs=c_jobs, jobs_128=c_128_jobs)


def names():
    return sorted(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def reference(c, mut=frozenset(), traces=None):
    """The model's (best_idx, best_dist) per job of a case."""
    out_i, out_d = [], []
    for jb in c["jobs"]:
        tr = None if traces is None else []
        bi, bd = F.fuse_search(c["kfs"][jb["kf"]], c["cam"], jb["Rcw"], jb["tcw"], jb["Ow"], c["pts"], c["th"], jb["first"],
                               jb["count"], jb["skip"], mut, tr)
        out_i.append(bi)
        out_d.append(bd)
        if traces is not None:
            traces.append(tr)
    return out_i, out_d


@functools.lru_cache(maxsize=None)
def expected(name):
    return reference(case(name))
