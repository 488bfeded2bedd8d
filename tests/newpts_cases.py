"""Directed inputs of coeb_kfdb_create_new_map_points (tests/newpts_ref.py is the model, tests/test_newpts_ref.py
shows what every case is for, tests/test_gpu_newpts_directed.py runs them on the device).

The search in front of the loop body is steered as in tests/tri_cases.py: every intended pair has a node of
its own, descriptors one bit apart, F12 = LINE_Y (the epipolar line of (x1, y1) is y2 = y1) and the epipole far
away, so a pair exists exactly where the two features share node and image row.  The base world is a camera
of fx = fy = 500, cx = 320, cy = 240, mb = 0.08, mbf = 40 with keyframe 1 at the identity and neighbour j
moved along x by its baseline; a point (X, Y, Z) is seen at u = fx X / Z + cx in keyframe 1 and fx b / Z to
the left of that in the neighbour, on the same row.  The views are the caller's and nothing is derived from
them, so the edge cases use poses that no rigid motion gives (an Ow that is not -Rwc tcw, a singular Rcw):
they put a chosen float on a threshold.  A case is a dict: kfs (keyframes as newpts_ref takes them), views
(one per keyframe), slot1, slots2, F12, epipole, mutants (the wrong readings of newpts_ref.MUTATIONS that have
to change its expected output)."""
import functools

import numpy as np

import newpts_ref as N
import tri_cases as TC
from tri_cases import LINE_Y, FAR, SCALE, SIGMA2, low, solve_radius

f32 = np.float32
FX = FY = 500.0
CX, CY = 320.0, 240.0
MB, MBF = 0.08, 40.0
RATIO_FACTOR = f32(f32(1.5) * f32(1.2))
EYE = np.eye(3, dtype=f32)


def view(R=EYE, t=(0, 0, 0), Ow=None, fx=FX, fy=FY, cx=CX, cy=CY, mb=MB, mbf=MBF, invfx=None, invfy=None):
    R = np.asarray(R, f32).reshape(3, 3)
    t = np.asarray(t, f32)
    Ow = (-(R.T.astype(np.float64) @ t.astype(np.float64))).astype(f32) if Ow is None else np.asarray(Ow, f32)
    return dict(Rcw=R.reshape(9), tcw=t, Ow=Ow, fx=f32(fx), fy=f32(fy), cx=f32(cx), cy=f32(cy),
                invfx=f32(1.0 / fx if invfx is None else invfx), invfy=f32(1.0 / fy if invfy is None else invfy),
                mb=f32(mb), mbf=f32(mbf))


def shifted(b, **kw):
    """the base camera moved along x by b"""
    return view(t=(-b, 0, 0), **kw)


class KF:
    """tri_cases.KF with the raw keypoint and the depth besides"""
    def __init__(self):
        self.kf, self.extra = TC.KF(), []

    def add(self, node, desc, x, y, octave=0, ur=-1.0, depth=-1.0, kx=None, ky=None, mp=0):
        self.extra.append((x if kx is None else kx, y if ky is None else ky, depth))
        return self.kf.add(node, desc, x=x, y=y, octave=octave, ur=ur, mp=mp)

    def done(self):
        d = self.kf.done()
        e = np.array(self.extra, f32).reshape(len(self.extra), 3)
        d.update(kx=e[:, 0].copy(), ky=e[:, 1].copy(), depth=e[:, 2].copy())
        return d


def see(kf, node, desc, P, b=0.0, stereo=False, octave=0, du=0.0, dk=0.0, cam=(FX, FY, CX, CY, MBF)):
    """The point P of the world as the base camera moved by b sees it (du: the keypoint moved along x, dk: the
    raw keypoint apart from the undistorted one)."""
    fx, fy, cx, cy, mbf = cam
    X, Y, Z = P
    u, v = fx * (X - b) / Z + cx + du, fy * Y / Z + cy
    return kf.add(node, desc, u, v, octave=octave, ur=(u - mbf / Z) if stereo else -1.0, depth=Z if stereo else -1.0,
                  kx=u + dk)


def _case(kfs, views, slots2, mutants, slot1=0, F12=None, epipole=None):
    nnb = len(slots2)
    return dict(kfs=[k.done() for k in kfs], views=views, slot1=slot1, slots2=list(slots2),
                F12=np.array([LINE_Y] * nnb if F12 is None else F12, f32).reshape(nnb, 3, 3),
                epipole=np.array([FAR] * nnb if epipole is None else epipole, f32).reshape(nnb, 2), mutants=tuple(mutants))


def _points(n, seed):
    rng = np.random.RandomState(seed)
    return np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(2.0, 9.0, n)], 1)


# ---------------------------------------------------------------- the cases
def case_pairs(L, nnb=1, seed=5):
    """L pairs per neighbour over the four stereo combinations, octaves mixed, every fifth keypoint of a
    neighbour moved by 6 px (a reprojection failure); baselines 0.1, 0.2, .."""
    P = _points(L, seed + L)
    a, nbs = KF(), [KF() for _ in range(nnb)]
    for i in range(L):
        see(a, i, low(0), P[i], stereo=bool(i & 1), octave=i % 4)
        for j, k in enumerate(nbs):
            see(k, i, low(1), P[i], b=0.1 * (j + 1), stereo=bool(i & 2), octave=(i + j) % 4,
                du=6.0 if (i + 2 * j) % 5 == 4 else 0.0)
    return _case([a] + nbs, [view()] + [shifted(0.1 * (j + 1)) for j in range(nnb)], range(1, nnb + 1), [])


def case_first_ok():
    """Six neighbours.  Feature 0 is accepted everywhere (first_ok 0, and not the last); feature 1 is rejected at
    j = 0, 1 (the neighbour's feature lies at the top octave there: the scale test) and accepted from j = 2; feature 2 from j = 5; feature 3 nowhere;
    feature 4 has no pair at j = 0 (another row) and is accepted at j = 1."""
    P = _points(5, 77)
    a, nbs = KF(), [KF() for _ in range(6)]
    first = (0, 2, 5, 6, 1)
    for i in range(5):
        see(a, i, low(0), P[i], stereo=i == 2)
        for j, k in enumerate(nbs):
            if i == 4 and j == 0:
                k.add(i, low(1), 100.0, 5.0)
            else:
                see(k, i, low(1), P[i], b=0.15 * (j + 1), octave=0 if j >= first[i] else 7)
    return _case([a] + nbs, [view()] + [shifted(0.15 * (j + 1)) for j in range(6)], range(1, 7), ["last_accepted"])


def case_parallax():
    """Neighbour 0 (slot 1) looks along the world's x axis from the origin: a feature at its principal point has
    the ray (1, 0, 0) and one of keyframe 1's at the principal point (0, 0, 1): cosParallaxRays = 0 exactly,
    and a little to either side with the neighbour's keypoint one pixel left or right.  Neighbours 1 and 2
    (baselines 0.07 and 0.09 against mb = 0.08): a stereo feature's bound lies below / above cosParallaxRays, so
    keyframe 1's (or, where it is mono, the neighbour's) UnprojectStereo / the triangulation is taken; the
    point at depth 40 makes A nearly singular.  Neighbours 3 and 4: mono pairs on either side of 0.9998.
    Neighbour 5 (mb = 0.5): both features stereo, only cosParallaxStereo1 is set (`else if`).  The raw keypoints
    of the stereo features lie 3 px from the undistorted ones."""
    a = KF()
    for i in range(3):
        a.add(i, low(0), CX, CY)
    side = KF()
    for i, du in enumerate((0.0, -1.0, 1.0)):
        side.add(i, low(1), CX + du, CY)
    Rside = np.array([[0, 0, -1], [0, 1, 0], [1, 0, 0]], f32)          # Rwc maps (x, y, z) to (z, y, -x)
    P = [(0.3, 0.2, 4.0), (-0.5, 0.1, 6.0), (0.2, -0.3, 40.0), (0.1, 0.1, 5.0)]
    nb = [KF(), KF(), KF(), KF(), KF()]
    node = 10
    for p in P[:3]:
        for st1, st2 in ((True, False), (False, True), (True, True)):
            see(a, node, low(0), p, stereo=st1, dk=3.0)
            see(nb[0], node, low(1), p, b=0.07, stereo=st2, dk=3.0)
            see(nb[1], node, low(1), p, b=0.09, stereo=st2, dk=3.0)
            see(nb[4], node, low(1), p, b=0.09, stereo=st2, dk=3.0, cam=(FX, FY, CX, CY, 250.0))
            node += 1
    see(a, node, low(0), P[3])
    see(nb[2], node, low(1), P[3], b=5.0 * 0.0195)                     # cos = 0.99981
    see(nb[3], node, low(1), P[3], b=5.0 * 0.0205)                     # cos = 0.99979
    views = [view(), view(R=Rside), shifted(0.07), shifted(0.09), shifted(5.0 * 0.0195), shifted(5.0 * 0.0205),
             shifted(0.09, mb=0.5, mbf=250.0)]
    return _case([a, side] + nb, views, range(1, 7), ["else_if_to_if", "undistorted_unproject", "no_9998"])


def case_mbf():
    """u2_r takes keyframe 1's mbf (:407): the neighbour's own mbf of 80 is never read.  The neighbour's stereo
    features carry the u_right that keyframe 1's mbf predicts."""
    P = _points(4, 3)
    a, b = KF(), KF()
    for i in range(4):
        see(a, i, low(0), P[i], stereo=bool(i & 1))
        see(b, i, low(1), P[i], b=0.3, stereo=True)
    return _case([a, b], [view(), shifted(0.3, mbf=80.0)], [1], ["mbf_kf2"])


def _z_case(which):
    """Keyframe 1's stereo features at its principal point with depth 4 and one float to either side, both
    keyframes at the same place: x3D = (0, 0, depth) from UnprojectStereo.  tcw(2) = -4 of keyframe 1 (z1) or of
    the neighbour (z2) puts z on 0 and on the smallest float either side of it."""
    a, b = KF(), KF()
    for i, d in enumerate((4.0, np.nextafter(f32(4), f32(5)), np.nextafter(f32(4), f32(3)), 5.0)):
        a.add(i, low(0), CX, CY, ur=CX - 10.0, depth=d)
        b.add(i, low(1), CX, CY)
    t = (0, 0, -4.0)
    views = [view(t=t, Ow=(0, 0, 0)), view()] if which == 1 else [view(), view(t=t, Ow=(0, 0, 0))]
    return _case([a, b], views, [1], ["z_lt"])


def chi2_edge(k, sigma2):
    """-> the float32 e2 on which `e2 > k * sigma2` in double and in float disagree, or None"""
    bound = k * float(f32(sigma2))
    fb = f32(f32(k) * f32(sigma2))
    for e2 in TC._floats_near(f32(bound), 3):
        if (float(e2) > bound) != bool(e2 > fb):
            return e2
    return None


def case_chi2():
    """cx = cy = 0, mbf = 0 and x3D = (0, 0, 4) on both optical axes: u = v = u_r = 0, so the errors are the
    keypoint's own coordinates and e2 = fma(x, x, y * y) is chosen: per octave (0 and the top) and per bound
    (5.991 mono, 7.8 stereo with u_right = 0), the float on which the double and the float product disagree, and
    the floats next to the double bound on either side; first on keyframe 1's side, then on the neighbour's.
    Both features of a pair share their row, and the other side's keypoint has x = 0 (e2 = y * y, about 1)."""
    top = TC.NLEVELS - 1
    a, b = KF(), KF()
    node = 0
    notes = []
    for side in (1, 2):
        for octv in (0, top):
            for k, stereo in ((5.991, False), (7.8, True)):
                bound = k * float(SIGMA2[octv])
                lo = f32(bound)
                if float(lo) > bound:
                    lo = np.nextafter(lo, f32(0))
                targets = [lo, np.nextafter(lo, f32(np.inf))]
                edge = chi2_edge(k, SIGMA2[octv])
                assert edge is not None, (k, octv)
                targets.append(edge)
                for t in targets:
                    dx, dy = solve_radius(t)
                    # exactly one feature of a pair is stereo: x3D is its UnprojectStereo
                    s1 = stereo if side == 1 else not stereo
                    s2 = stereo if side == 2 else not stereo
                    a.add(node, low(0), -dx if side == 1 else 0.0, -dy, octave=octv if side == 1 else 0,
                          ur=0.0 if s1 else -1.0, depth=4.0 if s1 else -1.0, kx=0.0, ky=0.0)
                    b.add(node, low(1), -dx if side == 2 else 0.0, -dy, octave=octv if side == 2 else 0,
                          ur=0.0 if s2 else -1.0, depth=4.0 if s2 else -1.0, kx=0.0, ky=0.0)
                    notes.append((node, side, octv, k, float(t)))
                    node += 1
    v = view(fx=50000.0, fy=50000.0, cx=0, cy=0, mbf=0.0)      # the rays of a pair stay 2e-4 rad apart
    c = _case([a, b], [v, v], [1], ["chi2_float"])
    c["notes"] = notes
    return c


def case_zero_distance():
    """The neighbour's stereo feature unprojects to (0, 0, 4), which keyframe 1's view names as its camera centre
    (its tcw says otherwise: z1 = 5): dist1 == 0.  case_zero_distance2 swaps the roles."""
    a, b = KF(), KF()
    a.add(0, low(0), CX, CY)
    b.add(0, low(1), CX, CY, ur=CX - MBF / 4.0, depth=4.0)
    return _case([a, b], [view(t=(0, 0, 1.0), Ow=(0, 0, 4.0)), view()], [1], [])


def case_zero_distance2():
    """Keyframe 1's stereo feature unprojects to (0, 0, 4), which the neighbour's view names as its camera centre
    (its tcw says z2 = 5): dist1 = 4, dist2 == 0."""
    a, b = KF(), KF()
    a.add(0, low(0), CX, CY, ur=CX - MBF / 4.0, depth=4.0)
    b.add(0, low(1), CX, CY)
    return _case([a, b], [view(), view(t=(0, 0, 1.0), Ow=(0, 0, 4.0))], [1], [])


def case_ratio():
    """dist2 / dist1 is close to 1 and ratioFactor = 1.8: octaves (7, 0) fail the first comparison (1.8 < 3.58),
    (0, 7) the second (1 > 0.28 * 1.8), (3, 1) and (4, 7) pass; (3, 0) passes by a little (1.728 < 1.8) and
    (4, 0) fails by a little (2.07).  The last two pairs see (0.2, 0, 5) from either side of the baseline's
    middle (dist2 / dist1 = 1): (0, 3) passes the second comparison by a little (1 < 0.579 * 1.8 = 1.04), (0, 4)
    fails it by a little (0.87)."""
    P = _points(6, 11)
    a, b = KF(), KF()
    for i, (o1, o2) in enumerate(((7, 0), (0, 7), (3, 1), (4, 7), (3, 0), (4, 0))):
        see(a, i, low(0), P[i], octave=o1)
        see(b, i, low(1), P[i], b=0.4, octave=o2)
    for i, o2 in ((6, 3), (7, 4)):
        see(a, i, low(0), (0.2, 0.0, 5.0), octave=0)
        see(b, i, low(1), (0.2, 0.0, 5.0), b=0.4, octave=o2)
    return _case([a, b], [view(), shifted(0.4)], [1], ["ratio_swapped"])


def case_shared_idx2():
    """Two features of keyframe 1 on one feature of the neighbour: both are accepted."""
    p = (0.4, -0.2, 5.0)
    a, b = KF(), KF()
    see(a, 1, low(0), p); see(a, 1, low(4), p)
    see(b, 1, low(2), p, b=0.3)
    return _case([a, b], [view(), shifted(0.3)], [1], [])


def case_w_zero():
    """x3D[3] == 0 can be had exactly only with a matrix no rotation gives: both Rcw have a zero first column, so
    A's first column is zero, stays zero under the Jacobi and wins with the null vector (1, 0, 0, 0).  Feature 1
    sees the same through ordinary poses (accepted)."""
    a, b = KF(), KF()
    a.add(0, low(0), CX + 100.0, CY)
    b.add(0, low(1), CX - 150.0, CY)
    R = np.array([[0, 1, 0], [0, 0, 1], [0, 0.5, 1]], f32)
    return _case([a, b], [view(R=R, t=(0.5, 0.25, 1.0), Ow=(0, 0, 0)), view(R=R, t=(-0.5, 0.125, 2.0), Ow=(1, 0, 0))], [1],
                 ["w_after_division"])


def case_empty():
    """keyframe 1 without features against two neighbours"""
    a, b, c = KF(), KF(), KF()
    b.add(1, low(0), 1.0, 1.0); c.add(1, low(0), 1.0, 1.0)
    return _case([a, b, c], [view(), shifted(0.1), shifted(0.2)], [1, 2], [])


# ---------------------------------------------------------------- the seeded random scene
NKF, NFEAT, NPTS = 6, 300, 260


def skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


@functools.lru_cache(maxsize=None)
def random_scene():
    """260 world points 3 to 12 units in front of six keyframes of 300 features each, 640 x 480, the base camera.
    Keyframe k is turned by a few degrees about y and moved by up to 0.9 units; a feature is a random point
    (with repeats) seen with 0.4 px of noise, at depths up to 3.2 (40 mb) stereo with probability 0.7, one in
    twelve put 5 px off its row or column, its descriptor the point's with up to 10 bits flipped and its node
    the point's number / 3 (lists of about three features).  F12 and the epipole are computed in double from
    the poses as ComputeF12 and SearchForTriangulation do.  A third of the features already have MapPoints."""
    rng = np.random.RandomState(2024)
    K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1.0]])
    pts = np.stack([rng.uniform(-4, 4, NPTS), rng.uniform(-3, 3, NPTS), rng.uniform(3, 12, NPTS)], 1)
    pts[:60, 2] = rng.uniform(1.5, 3.2, 60)
    base_d = rng.randint(0, 256, (NPTS, 32)).astype(np.uint8)
    kfs, views, poses = [], [], []
    for k in range(NKF):
        ang = np.deg2rad(rng.uniform(-4, 4))
        R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        Ow = np.array([0.18 * k * (1 if k % 2 else -1), rng.uniform(-0.1, 0.1), rng.uniform(-0.2, 0.2)]) if k else np.zeros(3)
        t = -R @ Ow
        poses.append((R, t))
        views.append(view(R=R, t=t, Ow=Ow))
        src = rng.randint(0, NPTS, NFEAT)
        Pc = pts[src] @ R.T + t
        u = FX * Pc[:, 0] / Pc[:, 2] + CX + rng.normal(0, 0.4, NFEAT)
        v = FY * Pc[:, 1] / Pc[:, 2] + CY + rng.normal(0, 0.4, NFEAT)
        off = rng.rand(NFEAT) < 1 / 12.0
        u = u + off * rng.choice([-5.0, 5.0], NFEAT) * (rng.rand(NFEAT) < 0.5)
        v = v + off * 5.0 * (u == u)
        z = Pc[:, 2] * (1 + rng.normal(0, 0.002, NFEAT))
        stereo = (Pc[:, 2] < 3.2) & (rng.rand(NFEAT) < 0.7)
        d = np.unpackbits(base_d[src], axis=1)
        for i in range(NFEAT):
            d[i, rng.choice(256, rng.randint(0, 11), replace=False)] ^= 1
        kfs.append(dict(desc=np.packbits(d, axis=1), node=(src // 3).astype(np.int32), x=u.astype(f32), y=v.astype(f32),
                        octave=rng.randint(0, 4, NFEAT).astype(np.int32), angle=np.zeros(NFEAT, f32),
                        u_right=np.where(stereo, u - MBF / z, -1.0).astype(f32), has_mp=(rng.rand(NFEAT) < 0.33).astype(np.uint8),
                        kx=(u + rng.normal(0, 0.3, NFEAT)).astype(f32), ky=(v + rng.normal(0, 0.3, NFEAT)).astype(f32),
                        depth=np.where(stereo, z, -1.0).astype(f32)))
    Kinv = np.linalg.inv(K)
    F12, epi = [], []
    R1, t1 = poses[0]
    for k in range(1, NKF):
        R2, t2 = poses[k]
        R12 = R1 @ R2.T
        t12 = -R12 @ t2 + t1
        F12.append(Kinv.T @ skew(t12) @ R12 @ Kinv)
        C2 = R2 @ np.zeros(3) + t2                  # keyframe 1's centre (the origin) in keyframe 2
        epi.append((FX * C2[0] / C2[2] + CX, FY * C2[1] / C2[2] + CY) if abs(C2[2]) > 1e-9 else FAR)
    return dict(kfs=kfs, views=views, slot1=0, slots2=list(range(1, NKF)), F12=np.array(F12, f32),
                epipole=np.array(epi, f32), mutants=())


CASES = {
    "first_ok": case_first_ok, "parallax": case_parallax, "mbf": case_mbf, "z1": functools.partial(_z_case, 1),
    "z2": functools.partial(_z_case, 2), "chi2": case_chi2, "zero_distance": case_zero_distance,
    "zero_distance2": case_zero_distance2, "ratio": case_ratio,
    "shared_idx2": case_shared_idx2, "w_zero": case_w_zero, "empty": case_empty,
    "nnb2": functools.partial(case_pairs, 7, 2), "nnb32": functools.partial(case_pairs, 5, 32),
}
for _L in (1, 63, 64, 65, 130):
    CASES["pairs_%d" % _L] = functools.partial(case_pairs, _L)


def names():
    return sorted(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def reference(c, only_stereo=False, mut=frozenset()):
    kfs = c["kfs"]
    return N.create_new_map_points(kfs[c["slot1"]], [kfs[s] for s in c["slots2"]], c["views"][c["slot1"]],
                                   [c["views"][s] for s in c["slots2"]], c["F12"], c["epipole"], SCALE, SIGMA2,
                                   RATIO_FACTOR, only_stereo, mut)


@functools.lru_cache(maxsize=None)
def expected(name, only_stereo=False):
    return reference(case(name), only_stereo)
