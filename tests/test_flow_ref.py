"""The CPU oracle's flow stages (oracle/orb_oracle.c: goodFeaturesToTrack, cornerSubPix,
calcOpticalFlowPyrLK, run7Point) against the independent numpy model of tests/flow_ref.py.  The
bounds and their derivations are in flow_ref's docstrings; each test asserts the precondition its
comparison rests on (separated decisions, or a capped share of ill-conditioned points), on the
model alone."""
import numpy as np
import pytest

import flow_ref as R
import flow_shapes as fs
from coeb_front import synth

# (w, h, seed) of synth.make_frames whose Harris decisions are separated from the float32 rounding
GF_CASES = [(96, 64, 1), (91, 93, 0), (181, 95, 0)]
KAPPA_MAX = 2.0 ** 10
SKIP_CAP = 0.10


def exact_rows(a, b, tag):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and np.array_equal(a, b), (tag, a.shape, b.shape, a[:5], b[:5])


# ---------------------------------------------------------------- Harris / goodFeaturesToTrack
@pytest.mark.parametrize("w,h,seed", GF_CASES)
def test_good_features_lists(oracle_mod, w, h, seed):
    """Ordered corner lists, equal on inputs whose candidates, threshold and local maxima are
    separated by more than twice 2^-18 (a + c)^2 in the model (flow_ref.harris)."""
    img = synth.make_frames(w, h, 1, seed=seed)[0]
    for md in (1.0, 3.0, 7.5, 8.5, 20.0):
        for q in (0.01, 0.5):
            for mc in (1, 1024):
                got, ok = R.good_features(img, mc, q, md, check=True)
                assert ok, (w, h, seed, md, q)                      # the precondition, on the model alone
                ref = oracle_mod.good_features(img, mc, q, md)
                assert q > 0.1 or mc == 1 or md > 10 or len(ref) >= 10
                exact_rows(got, ref, (w, h, md, q, mc))


def test_good_features_exact_ties(oracle_mod):
    """Equal corners: the regular grid of test_good_features_edges, and the image whose corners
    sit on the first and last candidate rows and columns.  In the model (integer box sums) all
    140 corners of the grid tie.  In the oracle the translated copies of one corner tie exactly
    (the same float32 operations on the same numbers), but a block's four corners are mirror
    images, whose float32 sums run in another order and differ in the last bits: the oracle
    lists one kind after the other.  So the lists are equal as sets (the corners are 9 px apart,
    over minDistance, whatever their order), equal as ordered lists within each kind of corner
    (the index tie-break), and the model's R along the oracle's order never rises by more than
    twice the Harris bound."""
    grid = np.zeros((120, 160), np.uint8)
    for y in range(10, 110, 20):
        for x in range(10, 150, 20):
            grid[y:y + 10, x:x + 10] = 200
    ref = oracle_mod.good_features(grid)
    got = R.good_features(grid)
    assert len(ref) == 140 and sorted(map(tuple, got.tolist())) == sorted(map(tuple, ref.astype(np.float64).tolist()))
    kind = lambda a: ((a[:, 0].astype(int) - 10) % 20 > 0) * 2 + ((a[:, 1].astype(int) - 10) % 20 > 0)
    for k in range(4):
        assert (kind(ref) == k).sum() == 35
        exact_rows(got[kind(got) == k], ref[kind(ref) == k], "grid, corner kind %d" % k)
    Rm, apc = R.harris(grid)
    v = Rm[ref[:, 1].astype(int), ref[:, 0].astype(int)]
    assert np.all(v[1:] - v[:-1] <= 2 * R.harris_bound(apc).max())
    img = fs.gf_border_image()
    for md in (1.0, 8.0):
        exact_rows(R.good_features(img, min_distance=md), oracle_mod.good_features(img, min_distance=md), "border")


def test_harris_border_is_reflect_101():
    """The model's own border rule, against the definition written out for one corner pixel:
    pixel -1 is pixel 1."""
    img = np.random.default_rng(5).integers(0, 256, (9, 11)).astype(np.uint8)
    p = np.pad(img.astype(np.int64), 2, mode="reflect")
    assert p[2 - 1, 2 - 1] == img[1, 1] and p[2 + 9, 2 + 11] == img[7, 9]
    Rm, apc = R.harris(img)
    gx = lambda y, x: sum(wy * (p[y + 2 + dy, x + 3] - p[y + 2 + dy, x + 1]) for dy, wy in ((-1, 1), (0, 2), (1, 1)))
    gy = lambda y, x: sum(wx * (p[y + 3, x + 2 + dx] - p[y + 1, x + 2 + dx]) for dx, wx in ((-1, 1), (0, 2), (1, 1)))
    refl = lambda v, n: -v if v < 0 else (2 * n - 2 - v if v >= n else v)
    a = b = c = 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            y, x = refl(0 + dy, 9), refl(0 + dx, 11)
            a, b, c = a + gx(y, x) ** 2, b + gx(y, x) * gy(y, x), c + gy(y, x) ** 2
    s = (1 / (4 * 3 * 255.0)) ** 2
    assert np.isclose(Rm[0, 0], (a * c - b * b) * s * s - 0.04 * ((a + c) * s) ** 2, rtol=1e-12)
    assert np.isclose(apc[0, 0], (a + c) * s, rtol=1e-12)


# ---------------------------------------------------------------- one cornerSubPix iteration
@pytest.mark.parametrize("w,h", [(91, 93), (181, 95), (333, 251)])
def test_corner_subpix_one_iteration(oracle_mod, w, h):
    """max_iter = 1 on the image's corners moved off the pixel grid (getRectSubPix keeps the
    fraction away from 0) and on points near every border, within flow_ref.subpix_step's bound;
    points with a condition factor over 2^10 are skipped, at most 10% of them."""
    img = fs.pair(w, h)[0]
    corners = oracle_mod.good_features(img) + np.float32([0.37, 0.61])
    edge = fs.subpix_edge_points(w, h) + np.float32([0.13, 0.29])
    pts = np.concatenate([corners, edge]).astype(np.float32)
    got = oracle_mod.corner_subpix(img, pts, max_iter=1)
    skipped, worst = 0, 0.0
    for p, g in zip(pts, got):
        new, bound, kappa = R.subpix_step(img, p)
        if not kappa <= KAPPA_MAX or np.abs(new - p).max() > 9.0:      # ill-conditioned, or near the reset rule
            skipped += 1
            continue
        err = np.abs(g.astype(np.float64) - new).max()
        worst = max(worst, err / bound)
        assert err <= bound, (w, h, p, g, new, bound, kappa)
    assert skipped <= SKIP_CAP * len(pts), (skipped, len(pts))
    print("subpix %dx%d: %d points, %d skipped, worst error / bound %.3g" % (w, h, len(pts), skipped, worst))


# ---------------------------------------------------------------- one LK step
@pytest.mark.parametrize("win", fs.WINS)
@pytest.mark.parametrize("w,h", [(45, 45), (91, 93), (181, 95)])
def test_lk_one_step(oracle_mod, w, h, win):
    """max_level 0, max_count 1: next - prev is one Gauss-Newton step from exact integer sums
    (flow_ref.lk_step), on the image's corners and the directed border points of
    flow_shapes.lk_directed.  Status agrees with the model's range and minimum-eigenvalue tests
    unless the model's value is within 2^-20 of the threshold; the step agrees within the bound,
    points with a condition factor over 2^10 skipped (at most 10%)."""
    prev, cur = fs.pair(w, h)
    pts, nnat, names, levels, want = fs.lk_points(oracle_mod, prev, win, 0)
    nx, st = oracle_mod.lk_pyr(prev, cur, pts, win=win, max_level=0, max_count=1)
    deriv = R.scharr(prev)
    skipped = compared = border = 0
    tracked = 0
    for i, (p, q, s) in enumerate(zip(pts, nx, st)):
        m = R.lk_step(prev, cur, p, win, deriv)
        if not m["in_range"]:
            assert s == 0, (p, "outside the range test")
            continue
        near = lambda v, t: abs(v - t) <= 2.0 ** -20 * t
        if near(m["min_eig"], R.MIN_EIG_THRESHOLD) or near(m["D"], R.FLT_EPSILON):
            continue
        if m["min_eig"] < R.MIN_EIG_THRESHOLD or m["D"] < R.FLT_EPSILON:
            assert s == 0, (p, m["min_eig"], m["D"])
            continue
        if m["factor"] > KAPPA_MAX:
            skipped += 1
            continue
        step = np.array(m["step"])
        end = p.astype(np.float64) + step - m["hw"]             # the result's own range test
        edge = [end[0] + win, end[0] - w, end[1] + win, end[1] - h]
        if min(abs(e - round(e)) for e in edge) <= m["bound"] and min(abs(e) for e in edge) < 1:
            continue
        inr = not (np.floor(end[0]) < -win or np.floor(end[0]) >= w or np.floor(end[1]) < -win or np.floor(end[1]) >= h)
        assert s == int(inr), (p, end, s)
        err = np.abs((q.astype(np.float64) - p.astype(np.float64)) - step).max()
        assert err <= m["bound"], (w, h, win, i, p, q, step, err, m["bound"], m["factor"])
        compared += 1
        tracked += int(s)
        border += i >= nnat
    assert skipped <= SKIP_CAP * len(pts), (skipped, len(pts))
    assert compared >= len(pts) // 3 and tracked >= 5 and (win < 15 or border >= 4), (compared, tracked, border, len(pts))


# ---------------------------------------------------------------- the 7-point solver
def seven_point_sets():
    """Float32 pairs: projections of random 3-D points into two cameras (exact epipolar geometry
    up to the float32 rounding of the points), with and without a pixel of noise."""
    rng = np.random.default_rng(12)
    sets = []
    for i in range(120):
        X = np.concatenate([rng.uniform(-2, 2, (7, 2)), rng.uniform(3, 9, (7, 1))], 1)
        ang = rng.uniform(-0.2, 0.2, 3)
        cx, cy, cz = np.cos(ang)
        sx, sy, sz = np.sin(ang)
        Rm = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
              np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
        t = rng.uniform(-0.5, 0.5, 3)
        K = np.array([[525.0, 0, 320], [0, 525.0, 240], [0, 0, 1]])
        a = (K @ X.T).T
        b = (K @ (Rm @ X.T + t[:, None])).T
        m1, m2 = a[:, :2] / a[:, 2:], b[:, :2] / b[:, 2:]
        if i % 2:
            m2 = m2 + rng.normal(0, 1.0, m2.shape)
        sets.append((np.ascontiguousarray(m1, np.float32), np.ascontiguousarray(m2, np.float32)))
    return sets


def test_seven_point(oracle_mod):
    """Every F of oc_run7point satisfies x2^T F x1 = 0 on its seven pairs and det F = 0, both to 1e-6
    relative to |F| and the points' norms (double against double: an algebra error would be O(1));
    and it returns as many F as the model's cubic has real roots, unless the model's discriminant
    is within 1e-9 (relative) of zero."""
    lib = oracle_mod.lib()
    counted = three = 0
    for m1, m2 in seven_point_sets():
        F = np.zeros(27, np.float64)
        n = lib.oc_run7point(oracle_mod.ptr(m1), oracle_mod.ptr(m2), oracle_mod.ptr(F))
        assert 1 <= n <= 3
        for k in range(n):
            r, d = R.epipolar_residuals(F[9 * k:9 * k + 9].reshape(3, 3), m1, m2)
            assert r.max() <= 1e-6 and d <= 1e-6, (k, r, d)
        Fs, nreal, disc = R.seven_point(m1, m2)
        for Fm in Fs:                                   # the model meets its own definition
            r, d = R.epipolar_residuals(Fm, m1, m2)
            assert r.max() <= 1e-9 and d <= 1e-9
        if abs(disc) > 1e-9:
            assert n == nreal == len(Fs), (n, nreal, len(Fs), disc)
            counted += 1
            three += n == 3
    assert counted >= 100 and three >= 10 and counted - three >= 10, (counted, three)
