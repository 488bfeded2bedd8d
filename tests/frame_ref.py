"""Plain numpy / Python model of the dynamic-box decision, the mask lookup, the Frame blur flag,
GrabImageRGBD's input conversions and UndistortKeyPoints, written from the reference's text
(src/ORBextractor.cc, src/Frame.cc, src/Tracking.cc) and OpenCV 3.4's definitions -- not from
oracle/orb_oracle.c and not from the kernels -- plus the directed cases that
tests/test_frame_ref.py (oracle against model, no GPU) and tests/test_gpu_frame_directed.py
(kernels against model) share.

Where the reference's arithmetic is float the model uses np.float32, sums are exact Python ints,
everything else is float64.  `mut` names one-line changes of the model (the mutants of
test_frame_ref.py); the empty set is the model.

Inputs to which the reference's text gives no meaning raise ValueError: a box whose Rect or fill
range leaves the image (Mat::operator()(Rect) asserts; the fill loop writes outside `mask`), a
negative extent, a T_M point whose truncated coordinates are outside the image (mask_mark.ptr reads
outside the Mat), NaN.  What the build does with those is its own convention, tested elsewhere."""
import collections

import numpy as np

F32 = np.float32
W0, H0 = 640, 480          # the reference hard-codes Mat::ones(480, 640) (ORBextractor.cc:1103, 1123)


def itrunc(v):
    """C's float -> int conversion of a finite value: towards zero."""
    v = float(v)
    if v != v:
        raise ValueError("NaN")
    return int(v)


def rect_of(box):
    """cv::Rect(int(xmin), int(ymin), int(xmax - xmin), int(ymax - ymin)) with the differences in
    float (ORBextractor.cc:1124, Frame.cc:173): (x, y, w, h)."""
    xmin, ymin, xmax, ymax = [F32(v) for v in box]
    return itrunc(xmin), itrunc(ymin), itrunc(F32(xmax - xmin)), itrunc(F32(ymax - ymin))


# ---------------------------------------------------------------- dynamic boxes
Dyn = collections.namedtuple("Dyn", "mask mark count area area_flag rects layer broke_at")


def dyn_decide(boxes, tm, blur, W=W0, H=H0, mut=frozenset()):
    """The box loop of ORBextractor::operator() (ORBextractor.cc:1101-1195).

    mask   uint8 H x W, 1 with 0 over every marked box's fill range (:1152-1159, :1172-1178)
    mark   per box: marked by either layer
    count  per box: box_keypoint.size() when the box was left (at the `break` for layer 1)
    area   float32: area_box of the marked boxes summed in box order (:1150, :1179)
    area_flag  area > 200000 (:1192)
    rects  the fill ranges (x0, y0, x1, y1) of the marked boxes whose range is not empty, in box order
    layer  per box 0 / 1 / 2; broke_at: per box the T_M index of the `break`, or -1
    """
    boxes = np.asarray(boxes, F32).reshape(-1, 4)
    tm = np.asarray(tm, F32).reshape(-1, 2)
    blur = np.asarray(blur, np.int64).reshape(-1)
    if np.isnan(boxes).any() or np.isnan(tm).any():
        raise ValueError("NaN")
    if len(blur) != len(boxes):
        raise ValueError("blur_flag[box_id] is read for every box (:1168)")
    mask = np.ones((H, W), np.uint8)                                       # :1103
    area = F32(0)                                                          # :1101
    mark, count, rects, layer, broke = [], [], [], [], []
    pts = []
    for x, y in tm:                                                        # ptr<uchar>(int row, int col) of :1139
        if "tm_round" in mut:
            px, py = int(np.floor(float(x) + 0.5)), int(np.floor(float(y) + 0.5))
        else:
            px, py = itrunc(x), itrunc(y)
        if not (0 <= px < W and 0 <= py < H):
            if "tm_round" in mut:
                pts.append(None)                                           # the mutant's own misses
                continue
            raise ValueError("T_M outside the image")
        pts.append((px, py))
    for b in range(len(boxes)):
        xmin, ymin, xmax, ymax = boxes[b]                                  # :1119-1122
        rx, ry, rw, rh = rect_of(boxes[b])                                 # :1124
        if rw < 0 or rh < 0 or xmax < xmin or ymax < ymin:
            raise ValueError("negative extent")
        fx0, fy0, fx1, fy1 = itrunc(xmin), itrunc(ymin), itrunc(xmax), itrunc(ymax)
        if rx < 0 or ry < 0 or rx + rw > W or ry + rh > H or fx1 > W or fy1 > H:
            raise ValueError("box outside the image")
        mask_mark = np.ones((H, W), np.uint8)                              # :1123
        mask_mark[ry:ry + rh, rx:rx + rw] = 0
        area_box = F32(F32(xmax - xmin) * F32(ymax - ymin))                # :1126
        n, marked, lay, brk = 0, False, 0, -1
        for t, p in enumerate(pts):                                        # :1137
            if p is not None and mask_mark[p[1], p[0]] == 0:               # :1139
                n += 1
            lhs = F32(n * 10000)                                           # size_t -> float for the comparison
            if (lhs >= area_box) if "layer1_ge" in mut else (lhs > area_box):   # :1145
                marked, lay, brk = True, 1, t
                break                                                      # :1160
        if not marked:
            second = blur[b] == 1 if "layer2_no_size" in mut else (blur[b] == 1 and n > 0)
            if second:                                                     # :1168
                marked, lay = True, 2
        if marked:
            area = F32(area + area_box)                                    # :1150 / :1179
            if "fill_rect" in mut:
                fx1, fy1 = rx + rw, ry + rh
            for i in range(fx0, fx1):                                      # :1152-1158 / :1172-1178
                mask[fy0:fy1, i] = 0
            if fx1 > fx0 and fy1 > fy0:
                rects.append((fx0, fy0, fx1, fy1))
        mark.append(marked)
        count.append(n)
        layer.append(lay)
        broke.append(brk)
    flag = bool(area >= F32(200000)) if "area_ge" in mut else bool(area > F32(200000))    # :1192
    return Dyn(mask, mark, count, area, int(flag), rects, layer, broke)


def masked(mask, x, y, scale=1.0):
    """CheckMovingKeyPoints(_finall)'s lookup (ORBextractor.cc:1391-1397, 1426-1440): the float
    product pt * scale, each coordinate >= cols - 1 / rows - 1 set to it, then ptr<uchar>(int, int).
    True where the keypoint is erased."""
    h, w = mask.shape
    sx, sy = F32(F32(x) * F32(scale)), F32(F32(y) * F32(scale))
    if sx >= w - 1:
        sx = F32(w - 1)
    if sy >= h - 1:
        sy = F32(h - 1)
    ix, iy = itrunc(sx), itrunc(sy)
    if ix < 0 or iy < 0:
        raise ValueError("keypoint left of / above the image")
    return mask[iy, ix] == 0


def keep_of(mask, kps):
    """Indices of the keypoint records (level-0 coordinates) that _finall keeps."""
    return np.array([i for i in range(len(kps)) if not masked(mask, kps["x"][i], kps["y"][i], 1.0)], np.int64)


def rasterise(rects, nrect, W=W0, H=H0):
    """The mask a list of (x0, y0, x1, y1) rectangles stands for."""
    m = np.ones((H, W), np.uint8)
    for x0, y0, x1, y1 in list(rects)[:nrect]:
        m[y0:y1, x0:x1] = 0
    return m


# ---------------------------------------------------------------- blur flag
def border(p, n, kind="reflect101"):
    """cv::borderInterpolate: BORDER_REFLECT_101 gfedcb|abcdefgh|gfedcba (a single element maps
    to itself), BORDER_REFLECT fedcba|abcdefgh|hgfedcb."""
    if n == 1:
        return 0
    d = 1 if kind == "reflect101" else 0
    while p < 0 or p >= n:
        p = -p - 1 + d if p < 0 else n - 1 - (p - n) - d
    return p


def blur_flag(gray, box, mut=frozenset()):
    """Frame.cc:173 and detect_laplacian (:905-913) for one box: (flag, S, N, mean).  The crop is
    cloned, so cv::Laplacian(ksize 1: [0 1 0; 1 -4 1; 0 1 0], BORDER_DEFAULT = REFLECT_101) sees
    nothing of the image round it; CV_16U saturates negative responses to 0 (cv::abs then changes
    nothing); cv::mean is sum * (1. / count) in double; flag = mean < 4.2 (:189)."""
    gray = np.asarray(gray, np.uint8)
    H, W = gray.shape
    if np.isnan(np.asarray(box, F32)).any():
        raise ValueError("NaN")
    rx, ry, rw, rh = rect_of(box)
    if rw <= 0 or rh <= 0 or rx < 0 or ry < 0 or rx + rw > W or ry + rh > H:
        raise ValueError("Rect outside the image or empty")
    c = gray[ry:ry + rh, rx:rx + rw].astype(np.int64)
    kind = "reflect" if "border_reflect" in mut else "reflect101"
    S = 0
    for y in range(rh):
        ym, yp = border(y - 1, rh, kind), border(y + 1, rh, kind)
        for x in range(rw):
            xm, xp = border(x - 1, rw, kind), border(x + 1, rw, kind)
            if "read_image" in mut:             # not a mutant of the reference: what a filter on the uncropped image sees
                g = lambda yy, xx: int(gray[border(ry + yy, H), border(rx + xx, W)])
                lap = g(y - 1, x) + g(y + 1, x) + g(y, x - 1) + g(y, x + 1) - 4 * g(y, x)
            else:
                lap = int(c[ym, x] + c[yp, x] + c[y, xm] + c[y, xp] - 4 * c[y, x])
            S += abs(lap) if "abs" in mut else min(max(lap, 0), 65535)
    N = rw * rh
    mean = float(S) * (1. / float(N))
    flag = mean <= 4.2 if "mean_le" in mut else mean < 4.2
    return int(flag), S, N, mean


def lap_sum(c):
    """S of a crop, vectorised (used to build crops with a chosen S; blur_flag is the model)."""
    c = np.asarray(c, np.int64)
    h, w = c.shape
    ym = [border(y - 1, h) for y in range(h)]
    yp = [border(y + 1, h) for y in range(h)]
    xm = [border(x - 1, w) for x in range(w)]
    xp = [border(x + 1, w) for x in range(w)]
    lap = c[ym] + c[yp] + c[:, xm] + c[:, xp] - 4 * c
    return int(np.maximum(lap, 0).sum())


# ---------------------------------------------------------------- conversions
R2Y, G2Y, B2Y, YUV_SHIFT = 4899, 9617, 1868, 14          # OpenCV 3.4 color.cpp, 8-bit RGB2Gray


def to_gray(img, rgb_order=1, mut=frozenset()):
    """Tracking.cc:212-225: a 1-channel image is used as it is, 3 / 4 channels go through cvtColor
    RGB2GRAY / BGR2GRAY / RGBA2GRAY / BGRA2GRAY (alpha ignored): 8-bit fixed point
    (R * 4899 + G * 9617 + B * 1868 + (1 << 13)) >> 14."""
    img = np.asarray(img, np.uint8)
    if img.ndim == 2:
        return img.copy()
    if img.shape[2] not in (3, 4):
        raise ValueError("channels")
    a = img.astype(np.int64)
    first, third = a[..., 0], a[..., 2]
    r, b = (first, third) if rgb_order else (third, first)
    if "swap_rb" in mut:
        r, b = b, r
    v = r * R2Y + a[..., 1] * G2Y + b * B2Y
    if "no_round" not in mut:
        v = v + (1 << (YUV_SHIFT - 1))
    return (v >> YUV_SHIFT).astype(np.uint8)


def depth_converts(dtype, factor):
    """Tracking.cc:227: fabs(mDepthMapFactor - 1.0f) > 1e-5 || type != CV_32F.  The difference is a
    float, the comparison a double's."""
    return abs(float(F32(F32(factor) - F32(1.0)))) > 1e-5 or np.dtype(dtype) != np.dtype(np.float32)


def depth_to_float(depth, factor):
    """Tracking.cc:227-228: convertTo(CV_32F, mDepthMapFactor), dst = src * alpha + beta in float
    with beta = 0, unless the map is 32F already and the factor is 1 to within 1e-5: then the map
    passes through untouched, bit for bit."""
    depth = np.asarray(depth)
    if depth.dtype not in (np.dtype(np.uint16), np.dtype(np.float32)):
        raise ValueError("depth type")
    if not depth_converts(depth.dtype, factor):
        return depth.copy()
    with np.errstate(all="ignore"):
        return (depth.astype(F32) * F32(factor) + F32(0)).astype(F32)


# ---------------------------------------------------------------- undistortion
def undistort(x, y, fx, fy, cx, cy, dist5, iters=5):
    """cv::undistortPoints(mat, mat, mK, mDistCoef, Mat(), mK) as Frame::UndistortKeyPoints calls it
    (Frame.cc:597), for one point, after cvUndistortPointsInternal of OpenCV 3.4: normalise, five
    fixed-point iterations of the inverse Brown model (no convergence test), project with P = mK.
    float64 throughout; returns float64 -- the float the reference stores is its rounding."""
    fx, fy, cx, cy = float(F32(fx)), float(F32(fy)), float(F32(cx)), float(F32(cy))       # mK is CV_32F
    k1, k2, p1, p2, k3 = [float(F32(v)) for v in dist5]                                   # mDistCoef too
    x0 = (float(F32(x)) - cx) / fx
    y0 = (float(F32(y)) - cy) / fy
    xn, yn = x0, y0
    for _ in range(iters):
        r2 = xn * xn + yn * yn
        icdist = 1.0 / (1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2)
        dx = 2.0 * p1 * xn * yn + p2 * (r2 + 2.0 * xn * xn)
        dy = p1 * (r2 + 2.0 * yn * yn) + 2.0 * p2 * xn * yn
        xn = (x0 - dx) * icdist
        yn = (y0 - dy) * icdist
    return xn * fx + cx, yn * fy + cy


def distort(u, v, fx, fy, cx, cy, dist5):
    """The forward Brown model (OpenCV's projectPoints convention) on an undistorted pixel."""
    fx, fy, cx, cy = float(F32(fx)), float(F32(fy)), float(F32(cx)), float(F32(cy))
    k1, k2, p1, p2, k3 = [float(F32(c)) for c in dist5]
    x, y = (u - cx) / fx, (v - cy) / fy
    r2 = x * x + y * y
    rad = 1.0 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return xd * fx + cx, yd * fy + cy


TIE_EPS = 1e-9      # px: ~200 double operations at coordinates <= 640 err by ~1.4e-11; two orders of margin
TIE_CAP = 0.01      # of a case's points


def check_rounded(got, want64, tag=""):
    """The tie rule: got (float32 values) must be the rounding of want64 (the model's float64),
    except where want64 lies within TIE_EPS of the midpoint of two adjacent float32: there either
    neighbour passes.  Returns the number of values that used the exemption."""
    got = np.asarray(got, F32).reshape(-1)
    want64 = np.asarray(want64, np.float64).reshape(-1)
    assert len(got) == len(want64), tag
    used = 0
    for i in range(len(got)):
        r = F32(want64[i])
        if got[i] == r:
            continue
        other = np.nextafter(r, F32(np.inf) if want64[i] > float(r) else F32(-np.inf))
        mid = (float(r) + float(other)) / 2.0
        assert got[i] == other and abs(want64[i] - mid) <= TIE_EPS, (tag, i, float(got[i]), want64[i], float(r))
        used += 1
    return used


# ================================================================ directed cases
# ---- dynamic decision (640 x 480)
DynCase = collections.namedtuple("DynCase", "name boxes tm blur want")
# want: dict of what the model's trace must show for the case to reach its branch


def _dc(name, boxes, tm, blur, **want):
    return DynCase(name, np.asarray(boxes, F32).reshape(-1, 4), np.asarray(tm, F32).reshape(-1, 2),
                   np.asarray(blur, np.int32).reshape(-1), want)


S_A = [10, 10, 11.0078125, 11]          # area 1 + 2^-7 exactly
S_B = [20, 10, 21.0078125, 11]
BIG = [0, 0, 542, 369]                  # 542 * 369 = 199998


def dyn_cases():
    c = []
    b100 = [100, 100, 200, 200]
    c.append(_dc("one_in_100x100", [b100], [[150, 150]], [0], mark=[False], count=[1], layer=[0], flag=0))
    c.append(_dc("two_in_100x100", [b100], [[150, 150], [160.5, 170.25]], [0], mark=[True], count=[2], layer=[1],
                 broke=[1], flag=0))
    c.append(_dc("one_in_100x99", [[100, 100, 200, 199]], [[150, 150]], [0], mark=[True], count=[1], layer=[1],
                 broke=[0], flag=0))
    # 100 x 150: marked at the second point; two more inside follow the break
    c.append(_dc("points_after_break", [[100, 100, 200, 250]], [[110, 110], [120, 120], [130, 130], [140, 140]], [0],
                 mark=[True], count=[2], layer=[1], broke=[1], flag=0))
    c.append(_dc("tm_empty", [b100, [300, 100, 400, 150]], [], [1, 1], mark=[False, False], count=[0, 0],
                 layer=[0, 0], flag=0))
    b200 = [100, 100, 300, 300]
    c.append(_dc("blur1_one_point", [b200], [[150, 150]], [1], mark=[True], count=[1], layer=[2], flag=0))
    c.append(_dc("blur1_no_point", [b200], [[350, 150]], [1], mark=[False], count=[0], layer=[0], flag=0))
    c.append(_dc("blur0_one_point", [b200], [[150, 150]], [0], mark=[False], count=[1], layer=[0], flag=0))
    c.append(_dc("area_200000", [[0, 0, 500, 400]], [[5, 5]], [1], mark=[True], layer=[2], area=200000.0, flag=0))
    c.append(_dc("area_200400", [[0, 0, 501, 400]], [[5, 5]], [1], mark=[True], layer=[2], area=200400.0, flag=1))
    c.append(_dc("two_400x300", [[100, 100, 500, 400]] * 2, [[150, 150]], [1, 1], mark=[True, True], layer=[2, 2],
                 area=240000.0, flag=1))
    # 199998 + (1 + 2^-7) + (1 + 2^-7): each float sum is a tie that rounds to even, 200000 -> flag 0;
    # (1 + 2^-7) + (1 + 2^-7) + 199998 = 200000.015625 exactly -> flag 1.  In float64 both are 1.
    pts = [[10.5, 10.5], [20.5, 10.5]]
    c.append(_dc("area_big_then_small", [BIG, S_A, S_B], pts, [1, 0, 0], mark=[True] * 3, layer=[2, 1, 1],
                 area=200000.0, flag=0))
    c.append(_dc("area_small_then_big", [S_A, S_B, BIG], pts, [0, 0, 1], mark=[True] * 3, layer=[1, 1, 2],
                 area=200000.015625, flag=1))
    # Rect(100, 50, int(199.7) = 199, 100) ends at column 298; the fill runs to (int)300.4 - 1 = 299
    frac = [100.7, 50, 300.4, 150]
    c.append(_dc("frac_point_past_rect", [frac], [[299.5, 60]], [1], mark=[False], count=[0], layer=[0], flag=0))
    c.append(_dc("frac_fill_past_rect", [frac], [[298.6, 60.9]], [1], mark=[True], count=[1], layer=[2], flag=0,
                 rects=[(100, 50, 300, 150)]))
    c.append(_dc("tm_minus_half", [[0, 0, 50, 50]], [[-0.5, -0.5]], [0], mark=[True], count=[1], layer=[1], flag=0))
    c.append(_dc("zero_width", [[100, 100, 100, 200], [300.2, 100, 300.9, 200]], [[100.5, 150], [300.5, 150]], [1, 1],
                 mark=[False, False], count=[0, 0], layer=[0, 0], flag=0))
    grid = [[40 + 150 * (i % 4), 30 + 110 * (i // 4), 70 + 150 * (i % 4), 60 + 110 * (i // 4)] for i in range(16)]
    c.append(_dc("sixteen_marked", grid, [[g[0] + 15, g[1] + 15] for g in grid], [0] * 16, mark=[True] * 16,
                 layer=[1] * 16, broke=list(range(16)), flag=0, nrect=16))
    # marked and unmarked boxes interleaved: the rectangles keep the box order, without gaps
    c.append(_dc("mixed_order", [[400, 300, 460, 360], b200, [10, 10, 60, 40], [500, 20, 620, 200], [300, 400, 330, 470]],
                 [[520, 30], [20, 20], [310, 410], [420, 310]], [0, 0, 0, 1, 0],
                 mark=[True, False, True, True, True], layer=[1, 0, 1, 2, 1], flag=0, nrect=4))
    return c


def check_dyn_want(case, d):
    """The case reaches its branch: the model's trace shows what the case is named after."""
    w = case.want
    for key, got in (("mark", d.mark), ("count", d.count), ("layer", d.layer), ("broke", d.broke_at)):
        if key in w:
            assert list(got) == list(w[key]), (case.name, key, got)
    if "area" in w:
        assert float(d.area) == w["area"], (case.name, float(d.area))
    if "rects" in w:
        assert d.rects == w["rects"], (case.name, d.rects)
    if "nrect" in w:
        assert len(d.rects) == w["nrect"], case.name
    assert d.area_flag == w["flag"], (case.name, float(d.area))


def device_dyn(raw):
    """DynMask as debug_read("dyn") returns it: (area_flag, nrect, rects[16][4])."""
    v = np.asarray(raw).view(np.int32)
    return int(v[0]), int(v[1]), [tuple(int(q) for q in v[2 + 4 * i:6 + 4 * i]) for i in range(16)]


# ---- cull boundaries
CLASSES = ("x==xmin", "x==xmax-1", "x==xmax", "y==ymin", "y==ymax-1", "y==ymax")


def cull_classes(kps, boxes):
    """counts[group][class]: keypoints of octave 0 (group 0) / octaves >= 1 (group 1) whose
    truncated coordinate sits on a box edge while the other coordinate is inside that box."""
    out = np.zeros((2, 6), np.int64)
    ix, iy = kps["x"].astype(np.int64), kps["y"].astype(np.int64)
    g = (kps["octave"] > 0).astype(np.int64)
    for xmin, ymin, xmax, ymax in np.asarray(boxes, F32):
        x0, y0, x1, y1 = int(xmin), int(ymin), int(xmax), int(ymax)
        iny, inx = (iy >= y0) & (iy < y1), (ix >= x0) & (ix < x1)
        for k, sel in enumerate((iny & (ix == x0), iny & (ix == x1 - 1), iny & (ix == x1),
                                 inx & (iy == y0), inx & (iy == y1 - 1), inx & (iy == y1))):
            for grp in (0, 1):
                out[grp, k] += int((sel & (g == grp)).sum())
    return out


def cull_boxes(kps, W=W0, H=H0, need=3):
    """16 disjoint boxes whose edges are taken from the keypoints' own coordinates: eight 225-row
    boxes in the upper half, one per 80-column slot, choose their x edges, eight 76-column boxes in
    the lower half choose their y edges; each at most 40 wide / high so that the marked area stays
    below 200000.  Greedy over the slots for the classes still short of `need`.  Fractional box
    coordinates, one T_M point inside each box and blur_flag 1 (marked by layer 1 or 2).
    Returns (boxes, tm, blur)."""
    ix, iy = kps["x"].astype(np.int64), kps["y"].astype(np.int64)
    g = (kps["octave"] > 0).astype(np.int64)
    rem = np.full((2, 6), need, np.int64)
    boxes = []
    for axis in (0, 1):
        for s in range(8):
            if axis == 0:
                lo, hi, o0, o1 = 80 * s + 2, 80 * s + 78, 10, 235
                sel = (iy >= o0) & (iy < o1)
                pos, n = ix, W
            else:
                lo, hi, o0, o1 = 245, 470, 80 * s + 2, 80 * s + 78     # the y boxes share the rows, not the columns
                sel = (ix >= o0) & (ix < o1)
                pos, n = iy, H
            hist = np.stack([np.bincount(pos[sel & (g == grp)], minlength=n + 1) for grp in (0, 1)])
            best, pick = -1, None
            for a in range(lo, hi - 2):
                for b in range(a + 2, min(a + 41, hi)):
                    gain = sum(min(rem[grp, 3 * axis + k], hist[grp, c])
                               for grp in (0, 1) for k, c in enumerate((a, b - 1, b)))
                    if gain > best:
                        best, pick = gain, (a, b)
            a, b = pick
            for grp in (0, 1):
                for k, c in enumerate((a, b - 1, b)):
                    rem[grp, 3 * axis + k] = max(0, rem[grp, 3 * axis + k] - hist[grp, c])
            boxes.append([a + 0.3, o0, b + 0.6, o1] if axis == 0 else [o0, a + 0.3, o1, b + 0.6])
    boxes = np.asarray(boxes, F32)
    tm = np.stack([(boxes[:, 0] + boxes[:, 2]) / 2, (boxes[:, 1] + boxes[:, 3]) / 2], axis=1).astype(F32)
    return boxes, tm, np.ones(len(boxes), np.int32)


# ---- blur flags
BlurCase = collections.namedtuple("BlurCase", "name gray box want_flag")


def crop_with_sum(w, h, S, seed):
    """A w x h crop of values near 100 whose saturated Laplacian sums to S exactly: seeded hill
    climb on single-pixel +-1 steps."""
    rng = np.random.default_rng(seed)
    c = np.full((h, w), 100, np.int64)
    cur = lap_sum(c)
    for _ in range(200000):
        if cur == S:
            return c.astype(np.uint8)
        y, x = int(rng.integers(h)), int(rng.integers(w))
        step = 1 if rng.integers(2) else -1
        c[y, x] += step
        new = lap_sum(c)
        if abs(new - S) <= abs(cur - S) and 60 <= c[y, x] <= 140:
            cur = new
        else:
            c[y, x] -= step
    raise AssertionError("no crop with S = %d" % S)


def _embed(crop, W, H, x, y, surround=255):
    g = np.full((H, W), surround, np.uint8)
    g[y:y + crop.shape[0], x:x + crop.shape[1]] = crop
    return g


def blur_cases():
    """(name, image, box, the flag the case is built for).  Every crop that is not the whole image
    is surrounded by 255: a Laplacian that read the image instead of reflecting at the crop's edge
    would see differences of ~150 there."""
    c = []
    add = lambda name, crop, W, H, x, y, flag, frac=(0.0, 0.0, 0.0, 0.0): c.append(BlurCase(
        name, _embed(crop, W, H, x, y),
        np.array([x + frac[0], y + frac[1], x + crop.shape[1] + frac[2], y + crop.shape[0] + frac[3]], F32), flag))
    one = np.array([[77]], np.uint8)
    add("1x1", one, 32, 24, 13, 9, 1)
    add("1xN_sharp", np.array([[100, 130, 90, 140, 95, 120, 100]], np.uint8).T, 32, 24, 5, 3, 0)     # w 1, h 7
    add("Nx1_sharp", np.array([[100, 130, 90, 140, 95, 120, 100]], np.uint8), 32, 24, 5, 3, 0)       # w 7, h 1
    add("1xN_flat", crop_with_sum(1, 7, 29, 11), 32, 24, 20, 10, 1)                                  # 29 / 7 = 4.14
    add("Nx1_flat", crop_with_sum(7, 1, 29, 12), 32, 24, 20, 10, 1)
    add("2x2_below", crop_with_sum(2, 2, 16, 13), 32, 24, 7, 7, 1)                                   # 4.0
    add("2x2_above", crop_with_sum(2, 2, 18, 14), 32, 24, 7, 7, 0)                                   # 4.5
    add("3x3_below", crop_with_sum(3, 3, 37, 15), 32, 24, 7, 7, 1)                                   # 4.11
    add("3x3_above", crop_with_sum(3, 3, 38, 16), 32, 24, 7, 7, 0)                                   # 4.22
    soft = crop_with_sum(6, 5, 125, 17)                                                              # 4.17
    for name, x, y in (("corner_tl", 0, 0), ("corner_tr", 26, 0), ("corner_bl", 0, 19), ("corner_br", 26, 19),
                       ("interior", 11, 8)):
        add(name, soft, 32, 24, x, y, 1)
    # Rect(int(11.7), int(8.2), int(6.2), int(5.7)): the same crop from a fractional box
    add("interior_frac", soft, 32, 24, 11, 8, 1, frac=(0.7, 0.2, 0.9, 0.9))
    add("whole_image_below", crop_with_sum(32, 24, 3225, 18), 32, 24, 0, 0, 1)     # 768 px: 3225.6 is the threshold
    add("whole_image_above", crop_with_sum(32, 24, 3226, 19), 32, 24, 0, 0, 0)
    add("over_1024_below", crop_with_sum(36, 29, 4384, 20), 40, 30, 2, 1, 1)       # 1044 px: 4384.8
    add("over_1024_above", crop_with_sum(36, 29, 4385, 21), 40, 30, 2, 1, 0)
    for n, (w, h) in ((5, (5, 1)), (10, (2, 5)), (50, (10, 5))):
        s42 = 42 * n // 10
        add("n%d_below" % n, crop_with_sum(w, h, s42 - 1, 30 + n), 32, 24, 9, 6, 1)
        add("n%d_exact" % n, crop_with_sum(w, h, s42, 31 + n), 32, 24, 9, 6, 0)
        add("n%d_above" % n, crop_with_sum(w, h, s42 + 1, 32 + n), 32, 24, 9, 6, 0)
    # the smallest N at which the two forms of the mean part at the rational 4.2: 1785 * (1. / 425) is
    # the double below 4.2 (flag 1, cv::mean's form), 1785 / 425 is 4.2 (flag 0)
    add("n425_exact", crop_with_sum(25, 17, 1785, 40), 32, 24, 4, 3, 1)
    return c


# ---- conversions
def gray_edge_triples(count=12):
    """(c0, c1, c2) byte triples in RGB order whose weighted sum + 8192 is k * 16384 - 1 (first
    half) or k * 16384 (second half): the two sides of the rounding step."""
    lo, hi = [], []
    g, r = np.meshgrid(np.arange(256), np.arange(256))
    for b in range(3, 256, 7):
        v = r * R2Y + g * G2Y + b * B2Y + 8192
        for want, out in ((16383, lo), (0, hi)):
            rr, gg = np.nonzero(v % 16384 == want)
            for i in range(len(rr)):
                if len(out) < count:
                    out.append((int(r[rr[i], gg[i]]), int(g[rr[i], gg[i]]), b))
    assert len(lo) == count and len(hi) == count
    return np.array(lo + hi, np.uint8)


def image_for(w, h, ch, seed):
    """Random image with the rounding-edge triples written over its first pixels (both channel
    orders: a triple and its reverse)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w) if ch == 1 else (h, w, ch), dtype=np.uint8)
    if ch >= 3:
        t = gray_edge_triples()
        t = np.concatenate([t, t[:, ::-1]])
        flat = img.reshape(-1, ch)
        n = min(len(t), len(flat))
        flat[:n, :3] = t[:n]
    return img


def depth_for(w, h, dtype, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.dtype(np.uint16):
        d = rng.integers(0, 65536, (h, w)).astype(np.uint16)
        d.reshape(-1)[:3] = [0, 65535, 5000][:d.size]
        return d
    d = (rng.random((h, w)) * 8).astype(F32)
    special = np.array([0x7fc12345, 0xffc00001, 0x7f800000, 0x00000001, 0x3f800000], np.uint32).view(F32)
    n = min(len(special), d.size)
    d.reshape(-1)[:n] = special[:n]
    return d


# factors on both sides of |factor - 1| > 1e-5 in float: 1 -+ k * ulp
DEPTH_FACTORS = (1.0, 1.0 / 5000.0, 0.5, 1.0 + 5e-6, float(F32(1) + F32(83 * 2.0 ** -23)),
                 float(F32(1) + F32(84 * 2.0 ** -23)), float(F32(1) - F32(167 * 2.0 ** -24)),
                 float(F32(1) - F32(168 * 2.0 ** -24)))
SINGLE_SIZES = ((1, 1), (63, 3), (64, 4), (65, 5))
BATCH_SIZES = ((4, 1), (12, 3), (4, 4), (64, 64), (68, 64), (64, 65))


# ---- undistortion
TUM1_K = (517.306408, 516.469215, 318.643040, 255.313989)
TUM2_K = (520.908620, 521.007327, 325.141442, 249.701764)
DIST = dict(tum1=(TUM1_K, (0.262383, -0.953104, -0.005358, 0.002628, 1.163314)),
            tum2_k3_0=(TUM2_K, (0.231222, -0.784899, -0.003257, -0.000105, 0.0)),
            negative_k1=(TUM1_K, (-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0)),
            strong=(TUM1_K, (0.9, 0.5, 0.02, -0.015, 0.3)),
            k1_zero=(TUM1_K, (0.0, -0.953104, -0.005358, 0.002628, 1.163314)))
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])


def undistort_points(n, cx, cy):
    """n fixed points inside 640 x 480: the principal point, the image corners, a 7 x 5 grid, then
    a fixed pseudo-random fill."""
    pts = [(cx, cy), (0, 0), (639, 0), (0, 479), (639, 479)]
    pts += [(20 + 100 * i, 15 + 112.5 * j) for j in range(5) for i in range(7)]
    rng = np.random.default_rng(77)
    fill = rng.random((max(0, n - len(pts)), 2)) * [639, 479]
    return np.asarray((pts + fill.tolist())[:n], F32)


def undistort_records(n, cx, cy):
    """Keypoint records at undistort_points with every other field carrying bits that a copy must
    keep: NaN payloads, -0, infinities, class_id -1, negative octaves."""
    p = undistort_points(n, cx, cy)
    k = np.zeros(n, KP_DTYPE)
    k["x"], k["y"] = p[:, 0], p[:, 1]
    bits = np.array([0x7fc12345, 0xffc00001, 0x80000000, 0x7f800000, 0x41f80000, 0x00000001], np.uint32).view(F32)
    i = np.arange(n)
    k["size"], k["angle"], k["response"] = bits[i % 6], bits[(i + 1) % 6], bits[(i + 3) % 6]
    k["octave"] = (i % 9) - 1
    k["class_id"] = -1
    k["class_id"][::5] = 0x7fffffff
    return k


def undistort_model(kps, K, dist):
    return np.array([undistort(x, y, *K, dist) for x, y in zip(kps["x"], kps["y"])], np.float64).reshape(-1, 2)


def check_undistorted(out, kps, K, dist, tag):
    """out against the model under the tie rule, the other five fields bit for bit; dist[0] == 0 is
    a copy (Frame.cc:581-585).  Returns the number of exemptions used."""
    raw = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(len(a), 28)
    assert np.array_equal(raw(out)[:, 8:], raw(kps)[:, 8:]), (tag, "fields other than the point")
    if F32(dist[0]) == 0:
        assert np.array_equal(raw(out), raw(kps)), (tag, "dist[0] == 0 copies")
        return 0
    m = undistort_model(kps, K, dist)
    used = check_rounded(np.stack([out["x"], out["y"]], axis=1), m, tag)
    assert used <= TIE_CAP * len(kps), (tag, used)
    return used
