"""A numpy restatement of the stages of Frame::ProcessMovingObject from OpenCV's published
definitions, in exact integers and float64, to hold the C oracle (oracle/orb_oracle.c) against.
The oracle and its HIP twin were written from one reading of OpenCV; this model is written
separately and in another shape (whole-image convolutions and window gathers instead of per-pixel
loops), so that a sign or border error the two share does not pass unseen.  tests/test_flow_ref.py
runs the comparisons; every bound below is stated in the model's own quantities.

u = 2^-24 is the float32 unit roundoff throughout.

findFundamentalMat's sampling loops are modelled too (find_fundamental, moving_tail below): the
RNG, getSubset and its retry rule, the last-point collinearity test, RANSACUpdateNumIters, the
RANSAC acceptance scan and the LMedS median, sigma and inlier rule, from ptsetreg.cpp and
fundam.cpp.  The 7-point models themselves are passed in (the tests pass the oracle's run7Point,
which test_seven_point holds against the SVD model seven_point), so the loops are compared bit for
bit: the same models scored by the same float32 errors give the same winner.

Still not reached or pinned: "subset not found" after iteration 0 is reached in LMedS only (1000
attempts, fm_sets.rare_subset); under RANSAC's 10000 attempts no input found produces it.  An
LMedS result dropped for fewer than 7 inliers and a non-finite error were not found either: a
model fits its own seven points.  Parity with a real OpenCV build stays unpinned, as OpenCV is
absent here.
"""
import math
from fractions import Fraction

import numpy as np

U = 2.0 ** -24


def pad101(a, n=1):
    return np.pad(a, n, mode="reflect")                 # BORDER_REFLECT_101


def conv_sep(a, ky, kx):
    """Valid correlation of a 2-D integer array with the separable kernel ky (x) kx (3 taps each)."""
    a = a.astype(np.int64)
    t = ky[0] * a[:-2] + ky[1] * a[1:-1] + ky[2] * a[2:]
    return kx[0] * t[:, :-2] + kx[1] * t[:, 1:-1] + kx[2] * t[:, 2:]


# ============================================================ Harris / goodFeaturesToTrack
def harris(img, k=0.04):
    """cornerHarris(blockSize 3, ksize 3, k) on an 8-bit image with BORDER_REFLECT_101: Sobel 3x3
    derivatives scaled by 1 / (4 * 3 * 255), the 3x3 box sums a, b, c of dx^2, dx dy, dy^2
    (the box over the reflected derivative images) and R = a c - b^2 - k (a + c)^2.
    Returns (R float64, a + c float64).  The box sums are exact integers and R is formed from
    them in integers (k as a fraction), so equal corners give equal R.

    The oracle's response is float32.  Its rounding: dx, dy carry one rounding each and their
    products one more (relative 3u); a box sum adds four deep, so a and c (non-negative terms) are
    within 7u relative and b within 7u (a + c) / 2 absolute; then with a c <= (a + c)^2 / 4 and
    |b| <= (a + c) / 2: a c is within 3.75u (a + c)^2, b^2 within 3.75u (a + c)^2, their difference
    rounds by 0.25u (a + c)^2, k (a + c)^2 (in double from a float sum within 8u) moves by
    16 k u (a + c)^2 = 0.64u (a + c)^2 and the last rounding by 0.25u (a + c)^2: under
    9u (a + c)^2.  The bound used is the round figure above it, 64u = 2^-18:
    |R_oracle - R_model| <= 2^-18 (a + c)^2  (harris_bound)."""
    p = pad101(img.astype(np.int64), 1)
    gx = conv_sep(p, (1, 2, 1), (-1, 0, 1))
    gy = conv_sep(p, (-1, 0, 1), (1, 2, 1))
    box = lambda m: conv_sep(pad101(m, 1), (1, 1, 1), (1, 1, 1))
    a, b, c = box(gx * gx), box(gx * gy), box(gy * gy)
    kf = Fraction(str(k))
    num = kf.denominator * (a * c - b * b) - kf.numerator * (a + c) * (a + c)      # < 2^63 for 8-bit images
    s2 = (1.0 / (4.0 * 3.0 * 255.0)) ** 2
    return num.astype(np.float64) * (s2 * s2 / kf.denominator), (a + c).astype(np.float64) * s2


def harris_bound(apc):
    return 2.0 ** -18 * apc * apc


def max3(a, fill=-np.inf):
    """Largest of the 8 neighbours of every pixel."""
    p = np.pad(a, 1, mode="constant", constant_values=fill)
    h, w = a.shape
    return np.max([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3) if (dy, dx) != (1, 1)], axis=0)


def good_features(img, max_corners=1000, quality=0.01, min_distance=8.0, k=0.04, check=False):
    """goodFeaturesToTrack(img, maxCorners, quality, minDistance, noArray(), 3, true, k): threshold
    at quality * max R, the 3x3 maxima off the border, sorted by (R, pixel index) descending, then
    taken greedily while no corner already taken within the 3x3 cells around (cells of
    round(minDistance)) is closer than minDistance.  (n, 2) float64.

    check=True also returns whether the input separates the decisions from the oracle's rounding:
    consecutive sorted candidates, every pixel against the threshold, and every pixel above the
    threshold against its largest neighbour differ by more than twice the Harris bound (the larger
    of the two pixels' bounds; the threshold's is quality times the bound at the image maximum)."""
    R, apc = harris(img, k)
    h, w = R.shape
    thr = R.max() * quality
    nb = max3(R)
    inner = np.zeros_like(R, bool)
    inner[1:-1, 1:-1] = True
    cand = inner & (R > thr) & (R >= nb)
    ys, xs = np.nonzero(cand)
    order = np.lexsort((ys * w + xs, R[ys, xs]))[::-1]
    ys, xs = ys[order], xs[order]
    cell = int(np.rint(min_distance))
    grid, out = {}, []
    for x, y in zip(xs.tolist(), ys.tolist()):
        if max_corners > 0 and len(out) >= max_corners:
            break
        cx, cy = x // cell, y // cell
        near = [q for gy in (cy - 1, cy, cy + 1) for gx in (cx - 1, cx, cx + 1) for q in grid.get((gx, gy), ())]
        if any((x - qx) ** 2 + (y - qy) ** 2 < min_distance * min_distance for qx, qy in near):
            continue
        grid.setdefault((cx, cy), []).append((x, y))
        out.append((x, y))
    out = np.array(out, np.float64).reshape(-1, 2)
    if not check:
        return out
    bound = harris_bound(apc)
    b = bound[ys, xs]
    v = R[ys, xs]
    ok = bool(np.all(v[:-1] - v[1:] > 2 * np.maximum(b[:-1], b[1:]))) if len(v) > 1 else True
    ty, tx = np.unravel_index(np.argmax(R), R.shape)
    bthr = quality * bound[ty, tx] + U * abs(thr)
    ok = ok and bool(np.all(np.abs(R - thr) > 2 * np.maximum(bound, bthr)))
    above = inner & (R > thr)
    ok = ok and bool(np.all((np.abs(R - nb) > 2 * np.maximum(bound, max3(bound, 0.0)))[above]))
    # a border pixel may hold the image maximum; it only sets the threshold
    return out, ok


# ============================================================ one cornerSubPix iteration
def bilinear_replicate(img, x, y):
    """getRectSubPix's sample of an 8-bit image at real (x, y): bilinear, edges replicated."""
    h, w = img.shape
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    ax, ay = x - x0, y - y0
    cx = lambda v: np.clip(v, 0, w - 1)
    cy = lambda v: np.clip(v, 0, h - 1)
    I = img.astype(np.float64)
    return ((1 - ax) * (1 - ay) * I[cy(y0), cx(x0)] + ax * (1 - ay) * I[cy(y0), cx(x0 + 1)] +
            (1 - ax) * ay * I[cy(y0 + 1), cx(x0)] + ax * ay * I[cy(y0 + 1), cx(x0 + 1)])


SUBPIX_SAMPLE_ERR = 255.0 * 16 * U


def subpix_step(img, pt, win=10):
    """One iteration of cornerSubPix(img, pt, Size(win, win), Size(-1, -1)): the (2 win + 3)^2
    window of bilinear samples around pt, central differences gx, gy on its inner (2 win + 1)^2,
    the weights exp(-(i / win)^2) exp(-(j / win)^2), the sums a = S w gx^2, b = S w gx gy,
    c = S w gy^2, bb1 = S w (gx^2 px + gx gy py), bb2 = S w (gx gy px + gy^2 py) and
    pt + [[c, -b], [-b, a]] (bb1, bb2) / (a c - b^2).  Returns (new point, bound, factor).

    The bound.  The oracle's samples are float32: the position, the four weights, their products
    with the pixels and the sums round at most 16 times on values up to 255, e_s = 255 * 16u.  A
    central difference is then within e_g = 2 e_s + 255u <= 3 e_s, the weights (expf products)
    within 3u relative, and the sums run in double.  With G = |gx| or |gy| at a pixel, each product
    gx^2, gx gy, gy^2 moves by at most d = w ((|gx| + |gy|) e_g + e_g^2) + 3u w |product|, so
    da, db, dc <= S d  and  dbb1, dbb2 <= S d (|px| + |py|).  For x = N / det with N = c bb1 - b bb2
    (and likewise the other row), det = a c - b^2:
        dN <= dc |bb1| + (c + dc) dbb1 + db |bb2| + (|b| + db) dbb2
        ddet <= a dc + c da + da dc + 2 |b| db + db^2  <=  2 rho kappa |det| + ...,
    kappa = (a c + b^2) / |a c - b^2| the condition factor and rho the largest relative error of
    a, b, c; and exactly |N' / det' - N / det| <= (dN + |x| ddet) / (|det| - ddet).  The result
    rounds to float32 once more: + 2u |pt|.  Points with kappa > 2^10 are skipped by the test."""
    n = 2 * win + 3
    off = np.arange(n, dtype=np.float64) - (n - 1) / 2
    X, Y = np.meshgrid(float(pt[0]) + off, float(pt[1]) + off)
    S = bilinear_replicate(img, X, Y)
    gx = S[1:-1, 2:] - S[1:-1, :-2]
    gy = S[2:, 1:-1] - S[:-2, 1:-1]
    r = np.arange(-win, win + 1, dtype=np.float64)
    e = np.exp(-(r / win) ** 2)
    wgt = e[:, None] * e[None, :]
    px, py = np.meshgrid(r, r)
    a, b, c = (wgt * gx * gx).sum(), (wgt * gx * gy).sum(), (wgt * gy * gy).sum()
    bb1 = (wgt * (gx * gx * px + gx * gy * py)).sum()
    bb2 = (wgt * (gx * gy * px + gy * gy * py)).sum()
    det = a * c - b * b
    dx, dy = (c * bb1 - b * bb2) / det, (a * bb2 - b * bb1) / det
    eg = 3 * SUBPIX_SAMPLE_ERR
    G = np.abs(gx) + np.abs(gy)
    d = wgt * (G * eg + eg * eg) + 3 * U * wgt * G * G
    dabc = d.sum()
    dbb = (d * (np.abs(px) + np.abs(py))).sum()
    ddet = a * dabc + c * dabc + dabc * dabc + 2 * abs(b) * dabc + dabc * dabc
    kappa = (a * c + b * b) / abs(det) if det != 0 else np.inf
    if not abs(det) > 2 * ddet:
        return np.array([pt[0] + dx, pt[1] + dy]), np.inf, np.inf
    dN1 = dabc * abs(bb1) + (c + dabc) * dbb + dabc * abs(bb2) + (abs(b) + dabc) * dbb
    dN2 = dabc * abs(bb2) + (a + dabc) * dbb + dabc * abs(bb1) + (abs(b) + dabc) * dbb
    bound = max((dN1 + abs(dx) * ddet) / (abs(det) - ddet), (dN2 + abs(dy) * ddet) / (abs(det) - ddet))
    bound += 2 * U * (max(abs(float(pt[0])), abs(float(pt[1]))) + abs(dx) + abs(dy))
    return np.array([float(pt[0]) + dx, float(pt[1]) + dy]), bound, kappa


# ============================================================ one LK step
def scharr(img):
    """calcScharrDeriv: (dx, dy) = ([3 10 3]^T (x) [-1 0 1], [-1 0 1]^T (x) [3 10 3]), REFLECT_101."""
    p = pad101(img.astype(np.int64), 1)
    return conv_sep(p, (3, 10, 3), (-1, 0, 1)), conv_sep(p, (-1, 0, 1), (3, 10, 3))


def lk_weights(a, b):
    """The four bilinear weights in 1/16384, from float32 fractions as lkpyramid.cpp rounds them."""
    a, b, one, s = np.float32(a), np.float32(b), np.float32(1), np.float32(16384)
    w00 = int(np.rint((one - a) * (one - b) * s))
    w01 = int(np.rint(a * (one - b) * s))
    w10 = int(np.rint((one - a) * b * s))
    return w00, w01, w10, 16384 - w00 - w01 - w10


def window(plane, x0, y0, win, mode):
    """The (win + 1)^2 block of an integer plane at (x0, y0): "reflect" pads by REFLECT_101 (the
    image), "zero" by zeros (the derivatives).  win + 1 < the plane's size and x0 >= -win."""
    h, w = plane.shape
    n = win + 1
    p = np.pad(plane, n, mode="reflect") if mode == "reflect" else np.pad(plane, n, mode="constant")
    return p[y0 + n:y0 + 2 * n, x0 + n:x0 + 2 * n]


def taps(block, wts, shift):
    w00, w01, w10, w11 = wts
    v = block[:-1, :-1] * w00 + block[:-1, 1:] * w01 + block[1:, :-1] * w10 + block[1:, 1:] * w11
    return (v + (1 << (shift - 1))) >> shift


MIN_EIG_THRESHOLD = float(np.float32(1e-4))
FLT_EPSILON = 2.0 ** -23


def lk_step(prev, cur, pt, win, deriv=None):
    """calcOpticalFlowPyrLK(prev, cur, pt, Size(win, win), maxLevel 0, TermCriteria(COUNT, 1)): one
    Gauss-Newton step on the single level.  The window origin is pt - (win - 1) / 2 in float32;
    its integer part places the window, its fraction gives the weights; the patch of prev is
    descaled by 9 bits and its Scharr derivatives by 14 (zero outside the image, the image
    itself reflected); A11, A12, A22 = S gx^2, S gx gy, S gy^2 and b1, b2 = S (J - I) gx, S (J - I) gy
    over the window are exact integers (scaled by 2^-20 in OpenCV), and the step is
        dx = (A12 b2 - A22 b1) / D,  dy = (A12 b1 - A11 b2) / D,  D = A11 A22 - A12^2.
    Returns a dict: in_range (the window passes the range test), step (dx, dy) or None, min_eig,
    D (both in OpenCV's 2^-20 units), bound, factor.

    The bound.  OpenCV converts each integer sum to float32 (u relative), multiplies and subtracts
    in float32: a product of two such sums is within 3u, so the numerator is within
    3u (|A12 b2| + |A22 b1|) + u |N| and D within 3u (A11 A22 + A12^2) + u |D| = (3 kappa + 1) u |D|,
    kappa = (A11 A22 + A12^2) / |D| the condition factor; 1 / D and its product with N round
    once each.  So |d(dx)| <= 1.01 (4u (|A12 b2| + |A22 b1|) / |D| + (3 kappa + 3) u |dx|), and the
    point takes three more float32 roundings (pt - hw, + dx, + hw): + 4u (|pt| + |dx| + hw)."""
    h, w = prev.shape
    hw = np.float32(win - 1) * np.float32(0.5)
    fx, fy = np.float32(pt[0]) - hw, np.float32(pt[1]) - hw
    ix, iy = int(np.floor(fx)), int(np.floor(fy))
    res = dict(in_range=not (ix < -win or ix >= w or iy < -win or iy >= h), step=None, min_eig=None, D=None,
               bound=None, factor=None, hw=float(hw))
    if not res["in_range"]:
        return res
    wts = lk_weights(fx - np.float32(ix), fy - np.float32(iy))
    dxi, dyi = deriv if deriv is not None else scharr(prev)
    I = taps(window(prev.astype(np.int64), ix, iy, win, "reflect"), wts, 9)
    J = taps(window(cur.astype(np.int64), ix, iy, win, "reflect"), wts, 9)
    gx = taps(window(dxi, ix, iy, win, "zero"), wts, 14)
    gy = taps(window(dyi, ix, iy, win, "zero"), wts, 14)
    A11, A12, A22 = int((gx * gx).sum()), int((gx * gy).sum()), int((gy * gy).sum())
    b1, b2 = int(((J - I) * gx).sum()), int(((J - I) * gy).sum())
    s = 2.0 ** -20
    D = (A11 * A22 - A12 * A12) * s * s
    res["D"] = D
    res["min_eig"] = ((A22 + A11) * s - np.sqrt(float((A11 - A22) ** 2 + 4 * A12 * A12)) * s) / (2 * win * win)
    if A11 * A22 - A12 * A12 == 0:
        return res
    det = A11 * A22 - A12 * A12
    dx, dy = (A12 * b2 - A22 * b1) / det, (A12 * b1 - A11 * b2) / det
    kappa = (A11 * A22 + A12 * A12) / abs(det)
    bx = 1.01 * (4 * U * (abs(A12 * b2) + abs(A22 * b1)) / abs(det) + (3 * kappa + 3) * U * abs(dx))
    by = 1.01 * (4 * U * (abs(A12 * b1) + abs(A11 * b2)) / abs(det) + (3 * kappa + 3) * U * abs(dy))
    far = max(abs(float(pt[0])), abs(float(pt[1]))) + max(abs(dx), abs(dy)) + float(hw)
    res.update(step=(dx, dy), factor=kappa, bound=max(bx, by) + 4 * U * far)
    return res


# ============================================================ the 7-point solver
def seven_point(m1, m2):
    """The 7-point algorithm: the two-dimensional null space of the 7x9 system x2^T F x1 = 0 by
    numpy.linalg.svd, then det(l F1 + (1 - l) F2) = 0, a cubic in l whose coefficients come from
    four values of the determinant, its roots by numpy.roots.  Returns (list of 3x3 F, number of
    real roots, relative discriminant): the discriminant over the sum of its terms' magnitudes,
    so a value near zero tells that the root count hangs on rounding."""
    m1, m2 = np.asarray(m1, np.float64), np.asarray(m2, np.float64)
    x1, y1, x2, y2 = m1[:, 0], m1[:, 1], m2[:, 0], m2[:, 1]
    A = np.stack([x2 * x1, x2 * y1, x2, y2 * x1, y2 * y1, y2, x1, y1, np.ones(7)], 1)
    vt = np.linalg.svd(A)[2]
    F1, F2 = vt[7].reshape(3, 3), vt[8].reshape(3, 3)
    ls = np.array([-1.0, 0.0, 1.0, 2.0])
    dets = np.array([np.linalg.det(l * F1 + (1 - l) * F2) for l in ls])
    c = np.linalg.solve(np.vander(ls, 4), dets)                 # c[0] l^3 + c[1] l^2 + c[2] l + c[3]
    a, b, cc, d = c
    terms = [18 * a * b * cc * d, -4 * b ** 3 * d, b * b * cc * cc, -4 * a * cc ** 3, -27 * a * a * d * d]
    disc = sum(terms) / max(sum(abs(t) for t in terms), 1e-300)
    roots = np.roots(c)
    real = [r.real for r in roots if abs(r.imag) <= 1e-7 * max(1.0, abs(r))]
    Fs = [l * F1 + (1 - l) * F2 for l in real]
    return Fs, (3 if disc > 0 else 1), disc


def epipolar_residuals(F, m1, m2):
    """|x2^T F x1| / (|F| |x1| |x2|) per pair, and |det F| / |F|^3 (Frobenius norm, homogeneous points)."""
    m1, m2 = np.asarray(m1, np.float64), np.asarray(m2, np.float64)
    h1 = np.concatenate([m1, np.ones((len(m1), 1))], 1)
    h2 = np.concatenate([m2, np.ones((len(m2), 1))], 1)
    nF = np.linalg.norm(F)
    r = np.abs(np.einsum("ni,ij,nj->n", h2, F, h1)) / (nF * np.linalg.norm(h1, axis=1) * np.linalg.norm(h2, axis=1))
    return r, abs(np.linalg.det(F)) / nF ** 3


# ============================================================ findFundamentalMat's sampling loops
# the decisions a reading of OpenCV can get wrong, each switchable (find_fundamental / moving_tail
# `mut`), so that tests/test_flow_ref.py can show that a directed set notices every one of them
MUTATIONS = ("accept_gt_max_good",        # RANSAC accepts on good > max_good, without the floor of 6
             "retry_not_counted",         # a collinear redraw does not count towards maxAttempts
             "collinear_all_triples",     # every triple of the subset instead of those with the 7th point
             "collinear_first_six",       # the test stops one point short: triples with the 6th point
             "median_low",                # element (n - 1) // 2 of the sorted errors
             "no_min_three",              # LMedS without max(niters, 3)
             "good_gt_7",                 # LMedS keeps its model on good > 7
             "d_lt_1",                    # T_M takes d < 1 in place of not (d <= 1)
             "edge_off_by_one")           # the upper edge bound admits n - edge
DBL_MIN, DBL_MAX, DBL_EPSILON = 2.0 ** -1022, float(np.finfo(np.float64).max), 2.0 ** -52


class Rng:
    """cv::RNG((uint64)-1): multiply-with-carry on a 64-bit state, the output its low 32 bits."""

    def __init__(self):
        self.state = 2 ** 64 - 1

    def __call__(self):
        self.state = (self.state & 0xffffffff) * 4164903690 + (self.state >> 32)      # < 2^64: no wrap to model
        return self.state & 0xffffffff


def update_iters(p, ep, max_iters, halves=None):
    """RANSACUpdateNumIters(p, ep, 7, max_iters) = round(log(1 - p) / log(1 - (1 - ep)^7)), capped at
    max_iters, 0 when no outlier is left.  `halves` collects |frac(num / denom) - 1/2|, the distance
    of the rounded quotient from a tie: the oracle takes its log from fdlibm, this one from libm."""
    p, ep = min(max(p, 0.0), 1.0), min(max(ep, 0.0), 1.0)
    num = max(1.0 - p, DBL_MIN)
    denom = 1.0 - (1.0 - ep) ** 7
    if denom < DBL_MIN:
        return 0
    num, denom = math.log(num), math.log(denom)
    if denom >= 0 or -num >= max_iters * -denom:
        return max_iters
    q = num / denom
    if halves is not None:
        halves.append(abs(q - math.floor(q) - 0.5))
    return round(q)                                             # cvRound: ties to even, as Python's


def collinear(s, mut=frozenset()):
    """haveCollinearPoints on a (7, 2) float32 subset: a triple with the last point is collinear when
    |dx2 dy1 - dy2 dx1| <= FLT_EPSILON (|dx1| + |dy1| + |dx2| + |dy2|), the differences taken in
    float32 and widened."""
    lasts = range(2, 7) if "collinear_all_triples" in mut else (5,) if "collinear_first_six" in mut else (6,)
    for i in lasts:
        d = (s[:i] - s[i]).astype(np.float64).tolist()
        for j in range(i):
            dx1, dy1 = d[j]
            for k in range(j):
                dx2, dy2 = d[k]
                if abs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (abs(dx1) + abs(dy1) + abs(dx2) + abs(dy2)):
                    return True
    return False


def get_subset(m1, m2, rng, max_attempts, mut=frozenset()):
    """getSubset: seven distinct indices rng() % n (a repeated index is drawn again); a subset with a
    collinear triple on either side costs one attempt and is drawn afresh.  (indices or None after
    max_attempts, number of redraws)."""
    n, attempts, retries = len(m1), 0, 0
    while attempts < max_attempts and retries < 50 * max_attempts:      # the second bound ends the mutated form
        idx = []
        while len(idx) < 7:
            i = rng() % n
            if i not in idx:
                idx.append(i)
        if not (collinear(m1[idx], mut) or collinear(m2[idx], mut)):
            return idx, retries
        retries += 1
        attempts += "retry_not_counted" not in mut
    return None, retries


def fm_errors(F, m1, m2, dtype=np.float64):
    """FMEstimatorCallback::computeError: the larger of the two squared point-to-epipolar-line
    distances, every operation elementwise in `dtype` and in OpenCV's written order, rounded once
    to float32."""
    f = [dtype(v) for v in np.asarray(F, np.float64).ravel()]
    x1, y1, x2, y2 = m1[:, 0].astype(dtype), m1[:, 1].astype(dtype), m2[:, 0].astype(dtype), m2[:, 1].astype(dtype)
    one = dtype(1)
    with np.errstate(all="ignore"):
        a = f[0] * x1 + f[1] * y1 + f[2]
        b = f[3] * x1 + f[4] * y1 + f[5]
        c = f[6] * x1 + f[7] * y1 + f[8]
        s2 = one / (a * a + b * b)
        d2 = x2 * a + y2 * b + c
        a = f[0] * x2 + f[3] * y2 + f[6]
        b = f[1] * x2 + f[4] * y2 + f[7]
        c = f[2] * x2 + f[5] * y2 + f[8]
        s1 = one / (a * a + b * b)
        d1 = x1 * a + y1 * b + c
        e1, e2 = d1 * d1 * s1, d2 * d2 * s2
        return np.where(e1 < e2, e2, e1).astype(np.float32)             # std::max(e1, e2)


def svd_solver(s1, s2):
    """The module's own 7-point models in the solver interface, scaled to F33 = 1."""
    Fs = seven_point(s1, s2)[0]
    return len(Fs), [F / F[2, 2] if abs(F[2, 2]) > DBL_EPSILON else F for F in Fs]


def _fm_run(m1, m2, thr, conf, solver, mut, dtype):
    n = len(m1)
    info = dict(branch="few" if n < 7 else "seven" if n == 7 else "lmeds" if n < 15 else "ransac", iterations=[],
                winner=None, nonfinite=0, halves=[], niters=None, ran=0, good=None, not_found=False)
    if n < 7:
        return None, info
    if n == 7:
        cnt, models = solver(m1, m2)
        info["iterations"].append(dict(subset=list(range(7)), retries=0, nmodels=cnt, scores=[], niters=[]))
        if cnt <= 0:
            return None, info
        info["winner"] = (0, 0)
        return np.array(models[0], np.float64).reshape(3, 3), info
    ransac = n >= 15
    rng, best = Rng(), None
    if ransac:
        niters, max_good, t = 1000, 0, np.float32(thr * thr)
    else:
        niters = update_iters(conf, 0.45, 1000, info["halves"])
        niters = niters if "no_min_three" in mut else max(niters, 3)
        min_med = DBL_MAX
    it = 0
    while it < niters:
        idx, retries = get_subset(m1, m2, rng, 10000 if ransac else 1000, mut)
        rec = dict(subset=idx, retries=retries, nmodels=None, scores=[], niters=[])
        info["iterations"].append(rec)
        if idx is None:
            info["not_found"] = True
            if it == 0:
                info["niters"], info["ran"] = niters, 1
                return None, info
            break
        cnt, models = solver(m1[idx], m2[idx])
        rec["nmodels"] = cnt
        for k in range(max(cnt, 0)):
            e = fm_errors(models[k], m1, m2, dtype)
            info["nonfinite"] += int(np.count_nonzero(~np.isfinite(e)))
            if ransac:
                good = int(np.count_nonzero(e <= t))
                rec["scores"].append(good)
                if good > max(max_good, 0 if "accept_gt_max_good" in mut else 6):
                    best, max_good, info["winner"] = np.array(models[k], np.float64).reshape(3, 3), good, (it, k)
                    niters = update_iters(conf, (n - good) / n, niters, info["halves"])
                    rec["niters"].append(niters)
            else:
                med = float(np.sort(e)[(n - 1) // 2 if "median_low" in mut else n // 2])
                rec["scores"].append(med)
                if med < min_med:
                    best, min_med, info["winner"] = np.array(models[k], np.float64).reshape(3, 3), med, (it, k)
        it += 1
    info["niters"], info["ran"] = niters, len(info["iterations"])
    if ransac:
        info["good"] = max_good
        return (best if max_good > 0 else None), info
    if not min_med < DBL_MAX:
        return None, info
    sigma = max(2.5 * 1.4826 * (1 + 5.0 / (n - 7)) * math.sqrt(min_med), 0.001)
    e = fm_errors(best, m1, m2, dtype)
    info["good"] = int(np.count_nonzero(e <= np.float32(sigma * sigma)))
    ok = info["good"] > 7 if "good_gt_7" in mut else info["good"] >= 7
    return (best if ok else None), info


def find_fundamental(m1, m2, thr=0.1, conf=0.99, solver=svd_solver, mut=frozenset(), trace=None):
    """cv::findFundamentalMat(m1, m2, FM_RANSAC, thr, conf) on float32 pairs: 3x3 float64 or None.
    n < 7: empty.  n == 7: the solver's first model.  8 <= n <= 14: LMedS, max(update(conf, 0.45,
    1000), 3) iterations, the model with the strictly smallest median (element n // 2 of the sorted
    float32 errors), kept when at least 7 errors are <= float32(sigma^2),
    sigma = max(2.5 * 1.4826 (1 + 5 / (n - 7)) sqrt(median), 0.001).  n >= 15: RANSAC, 1000
    iterations, every model of a subset scored in order against float32(thr^2), accepted on
    good > max(max_good, 6), the iteration count updated on every acceptance.  A subset that cannot
    be drawn ends the loop, with an empty result at iteration 0.

    solver(s1, s2) -> (count, models).  `trace` (a dict) receives the branch, per iteration the
    subset, the redraws, the model count, every model's good count or median and the iteration
    count after each update; the winner (iteration, model), the final good count, niters, the
    iterations run, the number of non-finite errors, the distances of the update quotients from a
    half-integer, and `fragile`: the winner or the verdict changes when the errors are computed in
    np.longdouble, so the set hangs on the last bit of a float32 error."""
    m1 = np.ascontiguousarray(m1, np.float32).reshape(-1, 2)
    m2 = np.ascontiguousarray(m2, np.float32).reshape(-1, 2)
    mut = frozenset(mut)
    assert mut <= set(MUTATIONS), mut
    F, info = _fm_run(m1, m2, thr, conf, solver, mut, np.float64)
    if trace is not None:
        F2, info2 = _fm_run(m1, m2, thr, conf, solver, mut, np.longdouble)
        info["fragile"] = info2["winner"] != info["winner"] or (F2 is None) != (F is None)
        trace.update(info)
    return F


def moving_tail(prev, cur, pxy, nxy, state, edge=5, limit=2120.0, tm_cap=None, solver=svd_solver, mut=frozenset(),
                trace=None):
    """The tail of Frame::ProcessMovingObject on tracked pairs: a pair stays when its state is set,
    its C-truncated coordinates lie in [edge, n - edge) on both sides and the 3x3 SAD around them
    is at most `limit`; findFundamentalMat on the survivors in order; T_M takes the current point of
    every survivor whose distance d to its epipolar line is not (d <= 1).
    (T_M or None, state, F or None, number of survivors); with tm_cap, T_M is cut to it and the
    full count goes to trace["n_tm"]."""
    mut = frozenset(mut)
    h, w = prev.shape
    p = np.ascontiguousarray(pxy, np.float32).reshape(-1, 2)
    q = np.ascontiguousarray(nxy, np.float32).reshape(-1, 2)
    keep = np.asarray(state).reshape(-1) != 0
    tp, tq = np.trunc(p).astype(np.int64), np.trunc(q).astype(np.int64)
    over = 1 if "edge_off_by_one" in mut else 0
    for t in (tp, tq):
        keep = keep & (t[:, 0] >= edge) & (t[:, 0] < w - edge + over) & (t[:, 1] >= edge) & (t[:, 1] < h - edge + over)
    o = np.arange(-1, 2)
    win = lambda img, t: img.astype(np.int64)[t[:, 1, None, None] + o[None, :, None], t[:, 0, None, None] + o[None, None, :]]
    sad = np.abs(win(prev, tp[keep]) - win(cur, tq[keep])).sum(axis=(1, 2))         # exact integers
    keep[np.nonzero(keep)[0][sad > limit]] = False
    m1, m2 = p[keep], q[keep]
    F = find_fundamental(m1, m2, 0.1, 0.99, solver, mut, trace)
    st = keep.astype(np.uint8)
    if F is None:
        return None, st, None, len(m1)
    f = F.ravel()
    px, py, qx, qy = (v.astype(np.float64) for v in (m1[:, 0], m1[:, 1], m2[:, 0], m2[:, 1]))
    with np.errstate(all="ignore"):
        A = f[0] * px + f[1] * py + f[2]
        B = f[3] * px + f[4] * py + f[5]
        Cc = f[6] * px + f[7] * py + f[8]
        d = np.abs(A * qx + B * qy + Cc) / np.sqrt(A * A + B * B)
        tm = m2[d < 1] if "d_lt_1" in mut else m2[~(d <= 1)]
    if trace is not None:
        trace["n_tm"] = len(tm)
    return (tm if tm_cap is None else tm[:tm_cap]).copy(), st, F, len(m1)
