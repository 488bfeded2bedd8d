"""Directed inputs of SearchForTriangulation (tests/tri_ref.py is the model, tests/test_tri_ref.py
shows what every case is for, tests/test_gpu_tri_directed.py runs them on the device).

Descriptors are built bit by bit: low(d) has bits 0 .. d-1 set, so low(a) and low(b) are |a - b|
apart and every distance below is chosen.  Unless a case says otherwise F12 = LINE_Y, for which
the epipolar line of (x1, y1) is y2 = y1 (a = 0, b = 1, c = -y1, den = 1, dsqr = (y2 - y1)^2), and
the epipole lies far away at FAR.  A case is a dict: kfs (keyframes as tri_ref takes them, each
with its has_mp mask), slot1, slots2, F12 [nnb, 3, 3], epipole [nnb, 2], only_stereo, check_ori and
mutants: the wrong readings of tri_ref.MUTATIONS that have to change its expected output."""
import functools

import numpy as np

import tri_ref as T

f32 = np.float32
NLEVELS = 8
LINE_Y = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], f32)
FAR = (5000.0, 5000.0)


def level_tables(scale_factor=1.2, nlevels=NLEVELS):
    """mvScaleFactors / mvLevelSigma2 as ORBextractor's constructor fills them (float32 tables, the
    factor a double holding the float argument)."""
    sf = float(f32(scale_factor))
    scale, sigma2 = [f32(1.0)], [f32(1.0)]
    for _ in range(1, nlevels):
        scale.append(f32(float(scale[-1]) * sf))
        sigma2.append(f32(scale[-1] * scale[-1]))
    return np.array(scale, f32), np.array(sigma2, f32)


SCALE, SIGMA2 = level_tables()


def bits(positions):
    d = np.zeros(256, np.uint8)
    d[list(positions)] = 1
    return np.packbits(d, bitorder="little")


def low(d):
    return bits(range(d))


class KF:
    def __init__(self):
        self.rows = []

    def add(self, node, desc, x=0.0, y=0.0, octave=0, ur=-1.0, angle=0.0, mp=0):
        self.rows.append((node, desc, x, y, octave, ur, angle, mp))
        return len(self.rows) - 1

    def done(self):
        r = self.rows
        col = lambda k, dt: np.array([q[k] for q in r], dt)        # noqa: E731
        desc = np.array([q[1] for q in r], np.uint8).reshape(len(r), 32)
        return dict(desc=desc, node=col(0, np.int32), x=col(2, f32), y=col(3, f32), octave=col(4, np.int32),
                    u_right=col(5, f32), angle=col(6, f32), has_mp=col(7, np.uint8))


def _case(kfs, slot1, slots2, mutants, F12=None, epipole=None, only_stereo=False, check_ori=False):
    nnb = len(slots2)
    F12 = np.array([LINE_Y] * nnb if F12 is None else F12, f32).reshape(nnb, 3, 3)
    epipole = np.array([FAR] * nnb if epipole is None else epipole, f32).reshape(nnb, 2)
    return dict(kfs=[k.done() if isinstance(k, KF) else k for k in kfs], slot1=slot1, slots2=list(slots2), F12=F12,
                epipole=epipole, only_stereo=only_stereo, check_ori=check_ori, mutants=tuple(mutants))


# ---------------------------------------------------------------- solved float coincidences
def _floats_near(v, k):
    v = f32(v)
    out = [v]
    lo = hi = v
    for _ in range(k):
        lo, hi = np.nextafter(lo, f32(-np.inf)), np.nextafter(hi, f32(np.inf))
        out += [lo, hi]
    return out


@functools.lru_cache(maxsize=None)
def solve_dsqr(target):
    """(a, c) with b = 0: den = fma(a, a, 0) and fl(fl(c * c) / den) == target exactly."""
    target = f32(target)
    for k in range(4000):
        a = f32(1.0 + k * 2.0 ** -23)
        den = T.fmaf(a, a, f32(0.0))
        for c in _floats_near(np.sqrt(float(target) * float(den)), 2):
            if f32(f32(c * c) / den) == target:
                return float(a), float(c)
    raise AssertionError("no (a, c) reaches %r" % target)


@functools.lru_cache(maxsize=None)
def solve_radius(target):
    """(dx, dy) with fma(dx, dx, fl(dy * dy)) == target exactly."""
    target = f32(target)
    for k in range(4000):
        dy = f32(1.0 + k * 2.0 ** -10)
        dy2 = f32(dy * dy)
        for dx in _floats_near(np.sqrt(max(float(target) - float(dy2), 0.0)), 2):
            if T.fmaf(dx, dx, dy2) == target:
                return float(dx), float(dy)
    raise AssertionError("no (dx, dy) reaches %r" % target)


# ---------------------------------------------------------------- the cases
def case_dist_49_50_51():
    a, b = KF(), KF()
    for nd, d in ((1, 49), (2, 50), (3, 51)):
        a.add(nd, low(0), y=nd)
        b.add(nd, low(d), y=nd)
    return _case([a, b], 0, [1], ["dist_ge_50"])


def case_ties():
    """node 1: two tied minima, the last wins.  node 2: two tied, the last fails the line.  node 3:
    three tied, the last fails the line.  node 4: 30 passes, 20 fails the line, 25 passes -- the 25
    wins, the failed 20 shadows nothing."""
    a, b = KF(), KF()
    for nd in (1, 2, 3, 4):
        a.add(nd, low(0), y=10.0 * nd)
    on, off = lambda nd: 10.0 * nd, lambda nd: 10.0 * nd + 3.0         # noqa: E731  (3^2 > 3.84)
    b.add(1, low(20), y=on(1)); b.add(1, bits(range(1, 21)), y=on(1))
    b.add(2, low(20), y=on(2)); b.add(2, bits(range(1, 21)), y=off(2))
    b.add(3, low(20), y=on(3)); b.add(3, bits(range(1, 21)), y=on(3)); b.add(3, bits(range(2, 22)), y=off(3))
    b.add(4, low(30), y=on(4)); b.add(4, low(20), y=off(4)); b.add(4, low(25), y=on(4))
    return _case([a, b], 0, [1], ["tie_first", "best_before_geometry"])


def case_epipole():
    """All mono unless said.  The epipole is the origin.  node 1: the nearer
    candidate lies 5 px from the epipole (skipped), the farther 20 px (kept).  node 2: exactly on the
    radius at octave 0 (10 px: 100 < 100 is false, kept).  node 3: exactly on the radius at the top
    octave.  node 4: keyframe 1 stereo, the candidate mono and 5 px away (no test, kept).  node 5:
    keyframe 1 mono, the candidate stereo and 5 px away (kept).  node 6: one ulp inside the radius
    at the top octave (skipped)."""
    top = NLEVELS - 1
    r_top = f32(f32(100.0) * SCALE[top])
    dx, dy = solve_radius(r_top)
    dxi, dyi = solve_radius(np.nextafter(r_top, f32(0)))
    ex, ey = 0.0, 0.0               # distex = 0 - x2 is exact
    a, b = KF(), KF()
    for nd in (1, 2, 3, 4, 5, 6):
        a.add(nd, low(0), y=ey - (dy if nd == 3 else dyi if nd == 6 else 0.0), ur=7.0 if nd == 4 else -1.0)
    b.add(1, low(10), x=ex - 5, y=ey); b.add(1, low(30), x=ex - 20, y=ey)
    b.add(2, low(10), x=ex - 10, y=ey)
    b.add(3, low(10), x=ex - dx, y=ey - dy, octave=top)
    b.add(4, low(10), x=ex - 5, y=ey)
    b.add(5, low(10), x=ex - 5, y=ey, ur=3.0)
    b.add(6, low(10), x=ex - dxi, y=ey - dyi, octave=top)
    return _case([a, b], 0, [1], ["epipole_le", "epipole_one_stereo"], epipole=[(ex, ey)])


def case_chi2_bound():
    """Neighbour 0, F12 = [[0,0,0],[0,0,0],[a,0,c]] and every point at the origin: num = c, den = a^2
    and dsqr lands exactly on the float product 3.84f * sigma2 of octave 0, which is below the double
    product 3.84 * sigma2: the reference accepts, a float comparison does not.  node 2's candidate
    lies at the top octave, where the same dsqr is far inside the bound.  Neighbour 1: an all-zero
    F12 (den == 0) matches nothing.  Neighbour 2: dsqr is the largest float below the double bound
    of the top octave (accepted; node 1's octave-0 candidate is far outside), neighbour 3: the
    smallest float not below it (rejected)."""
    top = NLEVELS - 1
    t0 = f32(f32(3.84) * SIGMA2[0])
    assert float(t0) < 3.84 * float(SIGMA2[0])
    a, b = KF(), KF()
    a.add(1, low(0))
    b.add(1, low(7))
    a.add(2, low(0))
    b.add(2, low(9), octave=top)
    bound = 3.84 * float(SIGMA2[top])
    below = f32(bound)
    if float(below) >= bound:
        below = np.nextafter(below, f32(0))
    F = np.zeros((4, 3, 3), f32)
    for j, t in ((0, t0), (2, below), (3, np.nextafter(below, f32(np.inf)))):
        F[j, 2, 0], F[j, 2, 2] = solve_dsqr(t)
    return _case([a, b], 0, [1, 1, 1, 1], ["chi2_float"], F12=F)


def case_masks():
    """node 1: the nearest candidate has a MapPoint, the farther one is taken.  node 2: keyframe 1's
    feature has a MapPoint.  node 3 / 4 matter under only_stereo (case_only_stereo)."""
    a, b = KF(), KF()
    a.add(1, low(0), y=1); b.add(1, low(5), y=1, mp=1); b.add(1, low(30), y=1)
    a.add(2, low(0), y=2, mp=1); b.add(2, low(5), y=2)
    a.add(3, low(0), y=3, ur=4.0); b.add(3, low(5), y=3); b.add(3, low(30), y=3, ur=2.0)
    a.add(4, low(0), y=4); b.add(4, low(5), y=4, ur=2.0)
    return a, b


def case_has_mp():
    return _case(list(case_masks()), 0, [1], ["no_has_mp2", "no_has_mp1"])


def case_only_stereo():
    """node 3: keyframe 1 stereo, the mono candidate is nearer, the stereo one is taken.  node 4:
    keyframe 1 mono, nothing is looked at.  u_right = 0 counts as stereo (>= 0), -0.5 does not."""
    a, b = case_masks()
    a.add(5, low(0), y=5, ur=0.0); b.add(5, low(5), y=5, ur=-0.5); b.add(5, low(9), y=5, ur=0.0)
    return _case([a, b], 0, [1], ["stereo_one_side"], only_stereo=True)


def case_nodes():
    """Nodes on one side only, features without a node (identical descriptors, never compared), and
    node ids far apart so that the binary search runs over several steps."""
    a, b = KF(), KF()
    a.add(-1, low(0)); b.add(-1, low(0))
    a.add(5, low(0)); b.add(7, low(0))
    for nd in (9, 40, 41, 1000, 70000):
        b.add(nd, low(3), y=nd % 97)
    for nd in (2, 9, 41, 70000, 70001):
        a.add(nd, low(0), y=nd % 97)
    return _case([a, b], 0, [1], [])


def case_trips(L):
    """Keyframe 2 lists L features under node 1.  A = low(0) wins at position 0, B = low(200) at
    position L - 1; C (filler + bits 200..255) has equal candidates spread over the trips and keeps
    the last.  The fillers (low(120)) are farther than 50 from all three."""
    filler = set(range(120))
    a, b = KF(), KF()
    ia = a.add(1, low(0), y=1)
    ib = a.add(1, low(200), y=1)
    ic = a.add(1, bits(filler | set(range(200, 256))), y=1)
    tied = bits(filler | set(range(200, 240)))
    ties = [p for p in (3, 64, 70, L - 2) if 0 < p < L - 1]
    for p in range(L):
        d = low(10) if p == 0 else low(190) if p == L - 1 else tied if p in ties else low(120)
        b.add(1, d, y=1)
    b.add(2, low(0), y=1)           # another node behind the long list
    c = _case([a, b], 0, [1], ["tie_first"] if len(ties) > 1 else [])
    c["want"] = {ia: 0, ib: L - 1 if L > 1 else -1, ic: ties[-1] if ties else -1}
    return c


def case_shared_idx2():
    """Two features of keyframe 1 keep the same feature of keyframe 2 (nothing is claimed)."""
    a, b = KF(), KF()
    a.add(1, low(0), y=1); a.add(1, low(4), y=1)
    b.add(1, low(2), y=1); b.add(1, low(40), y=1)
    return _case([a, b], 0, [1], ["claim"])


def case_rotation():
    """One match per node, angle1 - angle2 chosen per node:
      10 x   60       bin 2                         the first maximum
       5 x  -30       + 360 = 330, bin 11           the second
       1 x  900       900 / 30 = 30 -> bin 0        the third: 1 < 0.1f * 10 is false, so it stays
       1 x   15       half a bin: round -> 1        loses the third place to bin 0 (first in bin order)
       1 x  359.9     bin 12                        dropped
    """
    rots = [60.0] * 10 + [-30.0] * 5 + [900.0, 15.0, 359.9]
    a, b = KF(), KF()
    for nd, r in enumerate(rots):
        a2 = 30.0 if r < 0 else 0.0
        a.add(nd, low(0), y=nd, angle=a2 + r)
        b.add(nd, low(1), y=nd, angle=a2)
    return _case([a, b], 0, [1], ["rot_rint", "rot_no_360", "rot_bin30_kept"], check_ori=True)


def case_empty():
    """n1 = 0 against two neighbours, and (case_empty_neighbour) a neighbour without features."""
    a, b = KF(), KF()
    b.add(1, low(0))
    return _case([a, b], 0, [1, 1], [])


def case_empty_neighbour():
    a, b, e = KF(), KF(), KF()
    a.add(1, low(0)); b.add(1, low(1))
    return _case([a, e, b], 0, [1, 2, 1], [])


def case_repeat_self():
    """The same neighbour twice with different F12, and keyframe 1 as its own neighbour."""
    a, b = case_masks()
    F = np.array([LINE_Y, np.zeros((3, 3)), LINE_Y, LINE_Y], f32)
    return _case([a, b], 0, [1, 1, 0, 1], [], F12=F, check_ori=True)


def case_nnb32():
    a, b = case_masks()
    c = case_ties()["kfs"]
    kfs = [a.done(), b.done(), c[0], c[1]]
    slots2 = [(1, 3, 0, 2)[j % 4] for j in range(32)]
    F = np.array([LINE_Y if j % 5 else np.zeros((3, 3)) for j in range(32)], f32)
    return _case(kfs, 2, slots2, [], F12=F)


CASES = {
    "dist_49_50_51": case_dist_49_50_51, "ties": case_ties, "epipole": case_epipole, "chi2_bound": case_chi2_bound,
    "has_mp": case_has_mp, "only_stereo": case_only_stereo, "nodes": case_nodes, "shared_idx2": case_shared_idx2,
    "rotation": case_rotation, "empty": case_empty, "empty_neighbour": case_empty_neighbour,
    "repeat_self": case_repeat_self, "nnb32": case_nnb32,
}
for _L in (1, 63, 64, 65, 130):
    CASES["trips_%d" % _L] = functools.partial(case_trips, _L)


def names():
    return sorted(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def reference(c, mut=frozenset(), only_stereo=None, check_ori=None):
    """-> (match [nnb, n1], nmatches [nnb]) of the model."""
    kfs = c["kfs"]
    k1 = kfs[c["slot1"]]
    only_stereo = c["only_stereo"] if only_stereo is None else only_stereo
    check_ori = c["check_ori"] if check_ori is None else check_ori
    out = np.full((len(c["slots2"]), len(k1["node"])), -1, np.int32)
    nm = np.zeros(len(c["slots2"]), np.int32)
    for j, s2 in enumerate(c["slots2"]):
        out[j], nm[j] = T.search_for_triangulation(k1, kfs[s2], k1["has_mp"], kfs[s2]["has_mp"], c["F12"][j],
                                                   c["epipole"][j], SCALE, SIGMA2, only_stereo, check_ori, mut)
    return out, nm


@functools.lru_cache(maxsize=None)
def expected(name):
    return reference(case(name))
