"""The dynamic-box decision, the mask lookup, the blur flag, GrabImageRGBD's conversions and
UndistortKeyPoints twice: the oracle's C restatement against the plain model of tests/frame_ref.py
on the directed cases that tests/test_gpu_frame_directed.py runs on the device (no GPU here).

First the model is pinned by itself on cases worked by hand; then every case must reach the branch
it is named after, on the model's trace alone; then the oracle is compared with the model on every
case; then one-line mutants of the model must each change the result of a directed case."""
import numpy as np
import pytest

import frame_ref as R
from coeb_front import synth

F32 = np.float32
DYN = {c.name: c for c in R.dyn_cases()}
BLUR = {c.name: c for c in R.blur_cases()}
NS = (1, 255, 256, 257)


# ------------------------------------------------------------------ the model by itself
def test_model_laplacian_3x3_by_hand():
    """crop          REFLECT_101 neighbours (up + down + left + right - 4 c)
       10 12 10      (0,0): 20+20+12+12-40 = 24   (0,1): 30+30+10+10-48 = 32   (0,2) = (0,0) = 24
       20 30 20      (1,0): 10+10+30+30-80 = 0    (1,1): 12+12+20+20-120 = -56 -> 0   (1,2) = 0
       10 12 10      row 2 = row 0
    S = 2 * (24 + 32 + 24) = 160, N = 9, mean 17.78: sharp.  BORDER_REFLECT repeats the edge pixel
    instead ((0,0): 10+20+10+12-40 = 12), abs counts the 56."""
    crop = np.array([[10, 12, 10], [20, 30, 20], [10, 12, 10]], np.uint8)
    img = np.full((7, 9), 255, np.uint8)
    img[2:5, 4:7] = crop
    assert R.blur_flag(img, [4, 2, 7, 5]) == (0, 160, 9, 160 * (1. / 9))
    assert R.blur_flag(img, [4.9, 2.9, 7.95, 5.95])[1:3] == (160, 9)          # Rect(4, 2, 3, 3) again
    assert R.blur_flag(img, [4, 2, 7, 5], mut={"abs"})[1] == 160 + 56
    # REFLECT: (0,0) 12, (0,1) 12+30+10+10-48 = 14, (1,0) 10+10+20+30-80 = -10, (1,1) -56
    assert R.blur_flag(img, [4, 2, 7, 5], mut={"border_reflect"})[1] == 2 * (12 + 14 + 12)
    assert R.blur_flag(np.full((5, 5), 9, np.uint8), [0, 0, 5, 5])[:3] == (1, 0, 25)
    assert R.blur_flag(img, [4, 2, 5, 3])[:3] == (1, 0, 1)                       # one pixel: its own neighbour
    assert [R.border(p, 4) for p in range(-3, 7)] == [3, 2, 1, 0, 1, 2, 3, 2, 1, 0]
    assert [R.border(p, 4, "reflect") for p in range(-3, 7)] == [2, 1, 0, 0, 1, 2, 3, 3, 2, 1]
    assert [R.border(p, 2) for p in (-1, 0, 1, 2)] == [1, 0, 1, 0] and R.border(-1, 1) == R.border(1, 1) == 0
    for bad in ([4, 2, 4.5, 5], [-1, 0, 3, 3], [5, 2, 10, 5], [6, 2, 4, 5], [np.nan, 0, 3, 3]):
        with pytest.raises(ValueError):
            R.blur_flag(img, bad)


def test_model_two_boxes_four_points_by_hand():
    """A = (10, 10, 110, 130): Rect(10, 10, 100, 120), area 12000.  B = (200.5, 50, 261, 99.5):
    Rect(200, 50, 60, 49), area 60.5 * 49.5 = 2994.75, fill columns 200..260, rows 50..98.
    T_M = (10.9, 10.2) -> (10, 10) in A; (109.9, 129.9) -> (109, 129) in A; (260.2, 60) -> column
    260 is past B's Rect (200..259); (259.9, 98.9) -> (259, 98) in B.

         after point    0      1        2      3       left with
    A    count          1      2 -> 20000 > 12000: marked, break       layer 1, count 2, broke at 1
    B    count          0      0        0      1 -> 10000 > 2994.75    layer 1, count 1, broke at 3

    With T_M cut to its first point: A has 1 (10000 > 12000 is false), B has 0; blur = (1, 1)
    marks A by layer 2 and leaves B."""
    boxes = [[10, 10, 110, 130], [200.5, 50, 261, 99.5]]
    tm = [[10.9, 10.2], [109.9, 129.9], [260.2, 60], [259.9, 98.9]]
    d = R.dyn_decide(boxes, tm, [0, 0])
    assert d.mark == [True, True] and d.count == [2, 1] and d.layer == [1, 1] and d.broke_at == [1, 3]
    assert float(d.area) == 12000 + 2994.75 and d.area_flag == 0
    assert d.rects == [(10, 10, 110, 130), (200, 50, 261, 99)]
    want = np.ones((480, 640), np.uint8)
    want[10:130, 10:110] = 0
    want[50:99, 200:261] = 0
    assert np.array_equal(d.mask, want) and np.array_equal(R.rasterise(d.rects, 2), want)
    d = R.dyn_decide(boxes, tm[:1], [1, 1])
    assert d.mark == [True, False] and d.count == [1, 0] and d.layer == [2, 0] and d.broke_at == [-1, -1]
    assert R.dyn_decide(boxes, tm[:1], [0, 1]).mark == [False, False]
    # the lookup: the float product, clamped, truncated
    m = want
    assert R.masked(m, 109.99, 129.99) and not R.masked(m, 110.0, 129.0) and not R.masked(m, 109.0, 130.0)
    assert R.masked(m, 7.0, 7.0, 1.44) and not R.masked(m, 6.9, 7.0, 1.44)        # 10.08 / 9.936
    edge = np.ones((480, 640), np.uint8)
    edge[479, 639] = 0
    assert R.masked(edge, 638.5, 478.5, 1.2) and R.masked(edge, 1000.0, 479.0) and not R.masked(edge, 638.9, 479.0)
    for bad in (dict(boxes=[[600, 10, 641, 20]]), dict(boxes=[[-1, 10, 5, 20]]), dict(boxes=[[50, 10, 40, 20]]),
                dict(tm=[[640.0, 5]]), dict(tm=[[5, -1.0]]), dict(tm=[[np.nan, 5]]), dict(boxes=[[0, 0, np.nan, 5]])):
        with pytest.raises(ValueError):
            R.dyn_decide(bad.get("boxes", boxes[:1]), bad.get("tm", tm[:1]), [0])


def test_model_conversions_by_hand():
    px = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [1, 1, 1], [3, 0, 0]]], np.uint8)
    # 255 * 4899 + 8192 = 1257437 -> 76; 255 * 9617 + 8192 -> 150; 255 * 1868 + 8192 -> 29; 3 * 4899 + 8192 = 22889 -> 1
    assert R.to_gray(px, 1).tolist() == [[76, 150, 29, 255, 1, 1]]
    assert R.to_gray(px, 0).tolist() == [[29, 150, 76, 255, 1, 0]]
    rgba = np.concatenate([px, np.full((1, 6, 1), 200, np.uint8)], axis=2)
    assert np.array_equal(R.to_gray(rgba, 1), R.to_gray(px, 1))
    assert R.to_gray(px[..., 0], 0) is not px and np.array_equal(R.to_gray(px[..., 0], 0), px[..., 0])
    t = R.gray_edge_triples().astype(np.int64)
    v = t[:, 0] * 4899 + t[:, 1] * 9617 + t[:, 2] * 1868 + 8192
    assert (v[:12] % 16384 == 16383).all() and (v[12:] % 16384 == 0).all()
    d16 = np.array([[0, 1, 5000, 65535]], np.uint16)
    assert np.array_equal(R.depth_to_float(d16, 1.0), d16.astype(F32))             # 16U always converts
    assert np.array_equal(R.depth_to_float(d16, 1 / 5000.0), d16.astype(F32) * F32(1 / 5000.0))
    d32 = np.array([0x7fc12345, 0x3f800000, 0x00000001], np.uint32).view(F32).reshape(1, 3)
    for f, conv in zip(R.DEPTH_FACTORS, (False, True, True, False, False, True, False, True)):
        assert R.depth_converts(np.float32, f) == conv, f
        out = R.depth_to_float(d32, f)
        assert np.array_equal(out.view(np.uint32), d32.view(np.uint32)) == (not conv), f


# ------------------------------------------------------------------ undistortion by itself
def five_iteration_bound(x, y, K, dist):
    """A priori bound, from the coefficients alone, on what five fixed-point iterations leave at
    (x, y): q^5 * d.  q bounds the map's contraction over radii up to 1.1 times the point's --
    2 s |f'(s)| / f(s) for the radial factor f(s) = 1 + k1 s + k2 s^2 + k3 s^3, s = r^2, plus
    6 max|p| r / f for the tangential terms' derivatives -- and d the starting error in px, the
    distortion's own size r |f - 1| + 3 max|p| s."""
    fx, fy, cx, cy = K
    k1, k2, p1, p2, k3 = dist
    r = 1.1 * float(np.hypot((x - cx) / fx, (y - cy) / fy))
    s = np.linspace(0.0, r * r, 400)
    f = 1 + k1 * s + k2 * s * s + k3 * s ** 3
    fp = k1 + 2 * k2 * s + 3 * k3 * s * s
    pm = max(abs(p1), abs(p2))
    q = float((2 * s * np.abs(fp) / f).max() + 6 * pm * r / f.min())
    d = (r * float(np.abs(f - 1).max()) + 3 * pm * r * r) * max(fx, fy)
    return q ** 5 * d


def test_model_undistort_round_trip_tum1():
    """undistort, then the forward model, returns the input to within 1e-6 px -- at the points of
    the fixed set (principal point, corners, 7 x 5 grid) where five iterations can get that far:
    those whose a-priori bound five_iteration_bound is <= 1e-6.  The definition has no convergence
    test, and towards the corners of 640 x 480 TUM1's five iterations stop 1e-4 .. 1e-1 px short
    (0.102 px at (639, 0), 0.080 px at (0, 0)); that is the reference's result, not an error of
    the model, and test_model_undistort_is_five_iterations pins it.  Every figure is printed."""
    K, dist = R.DIST["tum1"]
    checked = []
    for x, y in R.undistort_points(40, K[2], K[3]):
        u, v = R.undistort(x, y, *K, dist)
        xd, yd = R.distort(u, v, *K, dist)
        err = max(abs(xd - float(x)), abs(yd - float(y)))
        bound = five_iteration_bound(float(x), float(y), K, dist)
        print("round trip (%7.2f, %7.2f): %.3e px, a-priori bound %.3e" % (x, y, err, bound))
        if bound <= 1e-6:
            assert err <= 1e-6, (x, y, err)
            checked.append((x > K[2], y > K[3]))
    assert len(checked) >= 12 and len(set(checked)) == 4, checked


def test_model_undistort_is_five_iterations():
    """k1 alone, strong: x_{j+1} = x0 / (1 + k1 r_j^2) written out five times is the model; the
    converged inverse (200 iterations, a fixed point to 1e-12) is somewhere else."""
    K = R.TUM1_K
    dist = (0.9, 0.0, 0.0, 0.0, 0.0)
    fx, fy, cx, cy = [float(F32(v)) for v in K]
    k1 = float(F32(0.9))
    x, y = F32(600.0), F32(440.0)
    x0, y0 = (float(x) - cx) / fx, (float(y) - cy) / fy
    xn, yn = x0, y0
    for _ in range(5):
        s = 1.0 / (1.0 + k1 * (xn * xn + yn * yn))
        xn, yn = x0 * s, y0 * s
    got = R.undistort(x, y, *K, dist)
    assert abs(got[0] - (xn * fx + cx)) < 1e-9 and abs(got[1] - (yn * fy + cy)) < 1e-9
    conv = R.undistort(x, y, *K, dist, iters=200)
    assert np.allclose(conv, R.undistort(x, y, *K, dist, iters=201), rtol=0, atol=1e-9)
    back = R.distort(*conv, *K, dist)
    assert abs(back[0] - 600.0) < 1e-6 and abs(back[1] - 440.0) < 1e-6
    assert abs(got[0] - conv[0]) > 0.5, (got, conv)
    # the directed strong set does not converge either, and four iterations are not five
    K, strong = R.DIST["strong"]
    a, b, c = [R.undistort(639, 479, *K, strong, iters=n) for n in (4, 5, 200)]
    assert abs(a[0] - b[0]) > 1e-2 and abs(b[0] - c[0]) > 1e-2 and np.isfinite([a, b, c]).all()
    assert np.abs(R.undistort_model(R.undistort_records(257, K[2], K[3]), K, strong)).max() <= 640


def test_tie_rule():
    lo = F32(100.0)
    hi = np.nextafter(lo, F32(np.inf))
    mid = (float(lo) + float(hi)) / 2
    assert R.check_rounded([lo], [mid - 1e-6]) == 0
    assert R.check_rounded([hi], [mid + 5e-10]) == 0 and R.check_rounded([lo], [mid + 5e-10]) == 1
    assert R.check_rounded([hi], [mid - 5e-10]) == 1
    for got, want in ((hi, mid - 2e-9), (lo, mid + 2e-9), (np.nextafter(hi, F32(np.inf)), mid + 5e-10)):
        with pytest.raises(AssertionError):
            R.check_rounded([got], [want])


# ------------------------------------------------------------------ the cases reach their branches
def test_dyn_scenarios_reach_their_branches():
    for c in DYN.values():
        R.check_dyn_want(c, R.dyn_decide(c.boxes, c.tm, c.blur))
    # the float32 sum in box order: the same three boxes the other way round, and in float64
    a, b = DYN["area_big_then_small"], DYN["area_small_then_big"]
    assert sorted(map(tuple, a.boxes.tolist())) == sorted(map(tuple, b.boxes.tolist()))
    assert sum(float(F32(F32(x[2] - x[0]) * F32(x[3] - x[1]))) for x in a.boxes) > 200000
    # column 299 of the fractional box: filled, though outside the Rect
    m = R.dyn_decide(*DYN["frac_fill_past_rect"][1:4]).mask
    assert m[60, 299] == 0 and m[60, 300] == 1 and m[60, 100] == 0 and m[60, 99] == 1
    assert R.rect_of(DYN["frac_fill_past_rect"].boxes[0]) == (100, 50, 199, 100)
    assert len(DYN["sixteen_marked"].boxes) == 16


def test_blur_scenarios_reach_their_branches():
    """Each crop gives the flag it was built for; each crop with a surround would give the other
    flag to a Laplacian that read the image; the 4.2 cases sit where they are named.

    S * (1. / N) against S / N at the rational 4.2 (S, N) = (21, 5), (42, 10), (210, 50): both forms
    give the double 4.2 itself (4.20000000000000017763568394002504646778106689453125), so
    `< 4.2` is false for either: the same side, and the form is not decided by these three.  The
    first N at which the forms part is 425 (S = 1785): S * (1. / N), the form of cv::mean's source
    and of the model, is below 4.2 (flag 1), S / N is not.  Case n425_exact holds the oracle and the
    kernel to the model's form; that OpenCV's binary computes this form stays unpinned."""
    for c in BLUR.values():
        flag, S, N, mean = R.blur_flag(c.gray, c.box)
        assert flag == c.want_flag, (c.name, S, N, mean)
        whole = N == c.gray.size
        if not whole and N > 1 and c.want_flag == 1:
            assert R.blur_flag(c.gray, c.box, mut={"read_image"})[0] == 0, c.name
    sizes = {c.name: R.blur_flag(c.gray, c.box)[1:3] for c in BLUR.values()}
    assert sizes["1x1"][1] == 1 and sizes["2x2_below"][1] == 4 and sizes["3x3_below"][1] == 9
    assert sizes["whole_image_below"] == (3225, 768) and sizes["whole_image_above"] == (3226, 768)
    assert sizes["over_1024_below"] == (4384, 1044) and sizes["over_1024_above"] == (4385, 1044)
    assert sizes["interior_frac"] == sizes["interior"]
    for n in (5, 10, 50):
        S, N = sizes["n%d_exact" % n]
        assert (S, N) == (42 * n // 10, n) and 10 * S == 42 * N
        assert S * (1. / N) == 4.2 and S / N == 4.2                      # the same side: not below
        assert sizes["n%d_below" % n] == (S - 1, N) and sizes["n%d_above" % n] == (S + 1, N)
    first = [N for N in range(5, 430, 5) if (42 * N // 10 * (1. / N) < 4.2) != (42 * N // 10 / N < 4.2)]
    assert first == [425] and sizes["n425_exact"] == (1785, 425)
    assert 1785 * (1. / 425) < 4.2 and 1785 / 425 == 4.2 and BLUR["n425_exact"].want_flag == 1


def test_conversion_scenarios_reach_their_branches():
    for w, h in R.SINGLE_SIZES + R.BATCH_SIZES:
        for ch in (3, 4):
            img = R.image_for(w, h, ch, w * h + ch).reshape(-1, ch).astype(np.int64)
            v = (img[:, 0] * 4899 + img[:, 1] * 9617 + img[:, 2] * 1868 + 8192) % 16384
            assert (v == 0).any() or (v == 16383).any() or w * h < 2
    npix = [w * h for w, h in R.BATCH_SIZES]
    assert [n % 16 == 0 for n in npix] == [False, False, True, True, True, True]
    assert npix[3] == 4096 and npix[4] == 4096 + 4 * 64 and npix[5] == 4096 + 4 * 16


# ------------------------------------------------------------------ oracle against model
@pytest.fixture(scope="module")
def ex(oracle_mod):
    return oracle_mod.Extractor()


@pytest.fixture(scope="module")
def textured(ex):
    fr = synth.make_frames(640, 480, 1, seed=1234)[0]
    return fr, ex.extract(fr)


def assert_filtered(got, plain, keep, tag):
    assert len(got["kps"]) == len(keep), (tag, len(got["kps"]), len(keep))
    assert np.array_equal(got["kps"], plain["kps"][keep]), tag
    assert np.array_equal(got["desc"], plain["desc"][keep]), tag


@pytest.mark.parametrize("name", sorted(DYN))
def test_oracle_dyn_case(ex, textured, name):
    """area_flag equal; and, the oracle not exporting its mask, the property that stands for it:
    with area_flag 0 the masked extraction is the plain one filtered by the model's mask
    (CheckMovingKeyPoints_finall is a pure filter, ORBextractor.cc:1204-1207)."""
    c = DYN[name]
    fr, plain = textured
    d = R.dyn_decide(c.boxes, c.tm, c.blur)
    got = ex.extract(fr, c.boxes, c.tm, c.blur, debug=True)
    assert got["area_flag"] == d.area_flag, name
    if d.area_flag == 0:
        assert_filtered(got, plain, R.keep_of(d.mask, plain["kps"]), name)


def test_oracle_cull_boundaries(ex, textured):
    fr, plain = textured
    boxes, tm, blur = R.cull_boxes(plain["kps"])
    cls = R.cull_classes(plain["kps"], boxes)
    assert (cls >= 3).all(), cls.tolist()
    d = R.dyn_decide(boxes, tm, blur)
    assert all(d.mark) and d.area_flag == 0 and len(d.rects) == 16
    keep = R.keep_of(d.mask, plain["kps"])
    assert len(plain["kps"]) - len(keep) >= 50
    assert_filtered(ex.extract(fr, boxes, tm, blur), plain, keep, "cull")


def test_oracle_blur_cases(oracle_mod):
    for c in BLUR.values():
        flag, S, N, mean = R.blur_flag(c.gray, c.box)
        f, m = oracle_mod.blur_flags(c.gray, c.box.reshape(1, 4))
        assert (int(f[0]), float(m[0])) == (flag, mean), (c.name, S, N)


def test_oracle_conversions(oracle_mod):
    for w, h in R.SINGLE_SIZES + R.BATCH_SIZES:
        for ch in (1, 3, 4):
            img = R.image_for(w, h, ch, w * h + ch)
            for order in (1, 0):
                assert np.array_equal(oracle_mod.image_to_gray(img, order), R.to_gray(img, order)), (w, h, ch, order)
        for dt in (np.uint16, np.float32):
            dep = R.depth_for(w, h, dt, w + h)
            for f in R.DEPTH_FACTORS:
                got = oracle_mod.depth_to_float(dep, F32(f))
                assert np.array_equal(got.view(np.uint32), R.depth_to_float(dep, f).view(np.uint32)), (w, h, dt, f)


@pytest.mark.parametrize("name", sorted(R.DIST))
def test_oracle_undistort(oracle_mod, name):
    """The tie rule, and the fixed inputs need no exemption from the oracle."""
    K, dist = R.DIST[name]
    for n in NS:
        kps = R.undistort_records(n, K[2], K[3])
        out = oracle_mod.undistort_keypoints(kps, *K, dist)
        assert R.check_undistorted(out, kps, K, dist, (name, n)) == 0


# ------------------------------------------------------------------ mutants
def _dyn_result(mut):
    return [(d.mask.tobytes(), d.area_flag) for d in (R.dyn_decide(c.boxes, c.tm, c.blur, mut=mut) for c in DYN.values())]


def _blur_result(mut):
    return [R.blur_flag(c.gray, c.box, mut=mut)[0] for c in BLUR.values()]


def _gray_result(mut):
    return [R.to_gray(R.image_for(w, h, ch, w * h + ch), order, mut=mut).tobytes()
            for w, h in R.SINGLE_SIZES for ch in (3, 4) for order in (1, 0)]


def _undistort_result(iters):
    out = []
    for name, (K, dist) in sorted(R.DIST.items()):
        kps = R.undistort_records(40, K[2], K[3])
        out.append([tuple(F32(v) for v in R.undistort(x, y, *K, dist, iters=iters)) for x, y in zip(kps["x"], kps["y"])])
    return out


MUTANTS = [("layer1_ge", _dyn_result, "one_in_100x100"), ("area_ge", _dyn_result, "area_200000"),
           ("fill_rect", _dyn_result, "frac_fill_past_rect"), ("tm_round", _dyn_result, "frac_fill_past_rect"),
           ("layer2_no_size", _dyn_result, "blur1_no_point"), ("border_reflect", _blur_result, None),
           ("abs", _blur_result, None), ("mean_le", _blur_result, "n5_exact"), ("swap_rb", _gray_result, None),
           ("no_round", _gray_result, None)]


@pytest.mark.parametrize("mut,run,case", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutant_changes_a_directed_case(mut, run, case):
    """Each one-line change of the model changes what a directed case computes -- the mask or the
    area flag, the blur flag (not only S), the gray bytes -- so the kernel tests, which see only
    those, would catch the same change in a kernel; where a case is named, that case does."""
    good, bad = run(frozenset()), run(frozenset([mut]))
    diff = [i for i in range(len(good)) if good[i] != bad[i]]
    assert diff, mut
    if case is not None:
        names = list(DYN) if run is _dyn_result else list(BLUR)
        assert names.index(case) in diff, (mut, [names[i] for i in diff])


def test_mutant_four_iterations():
    good, bad = _undistort_result(5), _undistort_result(4)
    assert sum(g != b for g, b in zip(good, bad)) >= 4          # every set but the copy
