"""The CPU oracle's flow stages (oracle/orb_oracle.c: goodFeaturesToTrack, cornerSubPix,
calcOpticalFlowPyrLK, run7Point) against the independent numpy model of tests/flow_ref.py.  The
bounds and their derivations are in flow_ref's docstrings; each test asserts the precondition its
comparison rests on (separated decisions, or a capped share of ill-conditioned points), on the
model alone."""
import ctypes as C

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


# ---------------------------------------------------------------- findFundamentalMat's loops
import fm_sets as S                                      # noqa: E402

_runs = {}


def model_run(oracle_mod, name):
    """(F, trace) of the model on a directed set, computed once."""
    if name not in _runs:
        tr = {}
        F = R.find_fundamental(*S.get(name), solver=S.oracle_solver(oracle_mod), trace=tr)
        _runs[name] = (F, tr)
    return _runs[name]


def same_F(a, b):
    return (a is None) == (b is None) and (a is None or np.array_equal(a.view(np.uint64), b.view(np.uint64)))


def same_tail(got, ref, tag):
    (tm, st, F, nf), (rtm, rst, rF, rnf) = got, ref
    assert np.array_equal(st, rst) and nf == rnf, (tag, nf, rnf)
    assert same_F(F, rF), (tag, F, rF)
    assert (tm is None) == (rtm is None), tag
    if tm is not None:
        assert np.array_equal(tm.view(np.uint32), rtm.view(np.uint32)), (tag, len(tm), len(rtm))


@pytest.mark.parametrize("name", list(S.SETS))
def test_find_fundamental_model_equals_oracle(oracle_mod, name):
    """The model's loops around the oracle's 7-point models against oc_find_fundamental: the same
    emptiness and F bit for bit, on every directed set; and the two tails on a flat image pair."""
    m1, m2 = S.get(name)
    assert S.inside(m1).all() and S.inside(m2).all()
    F, tr = model_run(oracle_mod, name)
    assert same_F(F, oracle_mod.find_fundamental(m1, m2)), (name, tr["winner"], tr["fragile"])
    prev, cur = S.flat_pair()
    st = np.ones(len(m1), np.uint8)
    got = R.moving_tail(prev, cur, m1, m2, st, solver=S.oracle_solver(oracle_mod))
    same_tail(got, oracle_mod.moving_tail(prev, cur, m1, m2, st), name)
    assert same_F(got[2], F) and got[3] == len(m1)


@pytest.mark.parametrize("name", list(S.thin_cases()))
def test_moving_tail_model_equals_oracle_thinned(oracle_mod, name):
    """Pairs removed by state, by the SAD check and by the edge rule: model against oracle, each
    thinned call against the call on its survivors alone, and T_M capacities of 0 and |T_M| - 1."""
    prev, cur, p, q, s = S.thin_cases()[name]
    solver = S.oracle_solver(oracle_mod)
    tr = {}
    got = R.moving_tail(prev, cur, p, q, s, solver=solver, trace=tr)
    ref = oracle_mod.moving_tail(prev, cur, p, q, s)
    same_tail(got, ref, name)
    k = ref[1] != 0
    assert ref[3] == k.sum() and (name != "sad_block" or 15 <= k.sum() < len(p) - 15)
    alone = oracle_mod.moving_tail(prev, cur, p[k], q[k], np.ones(k.sum(), np.uint8))
    assert same_F(ref[2], alone[2]) and alone[1].all()
    if ref[0] is not None:
        assert np.array_equal(ref[0], alone[0])
        nt = len(ref[0])
        assert tr["n_tm"] == nt and (name in ("keep7", "keep8") or nt >= 2)
        for cap in (0, nt - 1):
            if cap < 0:
                continue
            capped = R.moving_tail(prev, cur, p, q, s, tm_cap=cap, solver=solver)
            ont, otm = S.oracle_tail_capped(oracle_mod, prev, cur, p, q, s, cap)
            assert ont == nt and len(capped[0]) == cap and np.array_equal(capped[0], otm[:cap])
            assert (otm[cap:] == -7.0).all()


def test_directed_sets_reach_their_branches(oracle_mod):
    """What every directed set is for, on the model's trace alone."""
    T = {n: model_run(oracle_mod, n) for n in S.SETS}
    its = lambda n: T[n][1]["iterations"]
    retries = lambda n: sum(i["retries"] for i in its(n))
    counts = lambda n: [i["nmodels"] for i in its(n)]
    updates = lambda n: [u for i in its(n) for u in i["niters"]]
    for n in ("none", "six"):
        assert T[n][0] is None and T[n][1]["branch"] == "few"
    assert counts("seven_one_root") == [1] and counts("seven_three_roots") == [3] and counts("seven_repeated") == [0]
    assert T["seven_one_root"][0] is not None and T["seven_three_roots"][0] is not None and T["seven_repeated"][0] is None
    # LMedS: 300 iterations; the final count is exactly 7 on four sets and 8 and 14 on others
    for n in ("clean8", "clean9", "clean14", "noisy8", "noisy9", "noisy12", "noisy14", "random12", "line7_of_12"):
        assert T[n][1]["branch"] == "lmeds" and T[n][1]["ran"] == 300 and T[n][0] is not None, n
    assert [T[n][1]["good"] for n in ("noisy8", "noisy9", "clean14", "noisy14")] == [7, 7, 14, 8]
    # clean RANSAC: no outlier left after iteration 0, one iteration; two acceptances in it on five sets
    for n in ("clean15", "clean16", "clean40", "clean129", "clean300", "clean1024", "shift45"):
        tr = T[n][1]
        assert tr["branch"] == "ransac" and tr["ran"] == 1 and tr["niters"] == 0 and tr["good"] == len(S.get(n)[0]), n
    assert [len(its(n)[0]["niters"]) for n in ("clean15", "clean16", "clean40", "clean129", "clean300", "clean1024")] == \
        [2, 2, 1, 2, 2, 2]
    assert T["shift45"][1]["winner"] == (0, 0) and updates("shift45") == [0]     # the first model, accepted once
    # stops inside a chunk of 32 whose draws were made, at its end, and one iteration into the next
    assert (T["noisy15"][1]["ran"], T["noisy16"][1]["ran"]) == (162, 121)
    assert T["chunk_boundary"][1]["ran"] == 32 and T["chunk_plus_one"][1]["ran"] == 65
    assert T["chunk_plus_one"][1]["niters"] == 54          # lowered below the iterations already run
    for n in ("noisy40", "noisy129", "noisy300", "noisy1024"):
        assert T[n][1]["ran"] == 1000 and 5 <= len(updates(n)) <= 11 and T[n][0] is not None, n
    # subsets that cannot be drawn: the iteration-0 exit, also on a set that has a drawable subset
    for n, att in (("collinear20", 10000), ("five_points20", 10000), ("collinear12", 1000), ("rare_subset14", 1000)):
        assert T[n][0] is None and T[n][1]["ran"] == 1 and retries(n) == att and T[n][1]["not_found"], n
    late = T["rare_subset14_late"][1]                       # not found at iteration 58: the loop stops and keeps its model
    assert late["not_found"] and late["ran"] == 59 and its("rare_subset14_late")[58]["subset"] is None
    assert T["rare_subset14_late"][0] is not None and late["winner"][0] < 58
    # redraws between good draws
    assert retries("line14_of_24") > 1000 and T["line14_of_24"][1]["ran"] == 1000 and retries("line7_of_12") > 300
    assert max(i["retries"] for i in its("line14_of_24")) < 100
    # the solver's 0 and -1: skipped hypotheses, then a model that fits every pair
    assert counts("identity20") == [0, -1, 3] and T["identity20"][1]["niters"] == 0
    for n in ("random30", "random12"):
        assert T[n][0] is not None and T[n][1]["good"] in (7, 8, 9), n
    assert len(updates("random30")) >= 3


def test_directed_sets_are_not_all_fragile(oracle_mod):
    """Every branch has a set whose winner does not hang on the last bit of an error, and no
    iteration-count update lies within 1e-6 of a tie (log from libm against the oracle's fdlibm)."""
    solid = {}
    for n in S.SETS:
        tr = model_run(oracle_mod, n)[1]
        assert all(h >= 1e-6 for h in tr["halves"]), (n, min(tr["halves"]))
        assert tr["nonfinite"] == 0, n
        if not tr["fragile"]:
            solid.setdefault(tr["branch"], []).append(n)
    assert {"few", "seven", "lmeds", "ransac"} <= set(solid), solid
    for group in (("noisy8", "noisy14", "clean14"), ("noisy15", "noisy16"), ("noisy40", "noisy1024"),
                  ("chunk_boundary", "chunk_plus_one"), ("line14_of_24", "identity20", "rare_subset14")):
        assert any(n in solid["lmeds"] + solid["ransac"] for n in group), group


def test_update_iters_rule(oracle_mod):
    """RANSACUpdateNumIters: the model (math.log, pow) against the oracle (fdlibm log, a product)
    for every inlier count of seven set sizes and three running maxima."""
    lib = oracle_mod.lib()
    total = skipped = 0
    for n in (15, 16, 40, 129, 300, 1000, 1024):
        for good in range(7, n + 1):
            for mx in (1000, 300, 37):
                halves = []
                want = R.update_iters(0.99, (n - good) / n, mx, halves)
                total += 1
                if halves and halves[0] < 1e-6:
                    skipped += 1
                    continue
                got = lib.oc_ransac_update_iters(C.c_double(0.99), C.c_double((n - good) / n), mx)
                assert got == want, (n, good, mx, got, want)
    assert skipped < 0.01 * total, (skipped, total)
    assert R.update_iters(0.99, 0.45, 1000) == 300 and R.update_iters(0.99, 0.0, 1000) == 0


# mutation -> the directed case that notices it: (set, arguments of find_fundamental) or a tail case
MUTATION_CASES = {
    "accept_gt_max_good": ("random30", dict(thr=1e-14)),    # no model scores 7 at that threshold; some score 1..6
    "retry_not_counted": ("rare_subset14", {}),
    "collinear_all_triples": ("line14_of_24", {}),
    "collinear_first_six": ("line14_of_24", {}),
    "median_low": ("noisy14", {}),
    "no_min_three": ("noisy9", dict(conf=0.01)),            # update(0.01, 0.45, 1000) = 1
    "good_gt_7": ("noisy8", {}),
    "d_lt_1": ("tail", "keep129"),
    "edge_off_by_one": ("tail", "edges"),
}


@pytest.mark.parametrize("mut", R.MUTATIONS)
def test_every_mutation_is_noticed(oracle_mod, mut):
    """Each wrong reading of OpenCV changes F, its emptiness, T_M or the state on a named directed
    case, on which the unmutated model equals the oracle."""
    solver = S.oracle_solver(oracle_mod)
    name, arg = MUTATION_CASES[mut]
    if name == "tail":
        prev, cur, p, q, s = S.thin_cases()[arg]
        ref = R.moving_tail(prev, cur, p, q, s, solver=solver)
        same_tail(ref, oracle_mod.moving_tail(prev, cur, p, q, s), arg)
        bad = R.moving_tail(prev, cur, p, q, s, solver=solver, mut={mut})
        assert not (np.array_equal(ref[1], bad[1]) and same_F(ref[2], bad[2]) and np.array_equal(ref[0], bad[0]))
        return
    m1, m2 = S.get(name)
    ref = R.find_fundamental(m1, m2, solver=solver, **arg)
    assert same_F(ref, oracle_mod.find_fundamental(m1, m2, **arg)), name
    assert not same_F(ref, R.find_fundamental(m1, m2, solver=solver, mut={mut}, **arg)), (mut, name)


def test_find_fundamental_with_the_svd_solver():
    """The default solver (the module's SVD 7-point models): a clean scene's F has every pair on
    its epipolar line."""
    m1, m2 = S.get("clean40")
    F = R.find_fundamental(m1, m2)
    assert F is not None and R.epipolar_residuals(F, m1, m2)[0].max() < 1e-6
