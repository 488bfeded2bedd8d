"""Shapes, images and directed points shared by tests/test_gpu_flow_shapes.py (HIP against the
oracle), tests/test_oracle_kat.py (the same coverage conditions on the oracle alone) and
tests/test_flow_ref.py (the oracle against the numpy model of tests/flow_ref.py).

The LK points are computed with calcOpticalFlowPyrLK's own float32 arithmetic: a level-0
coordinate p has its level-l window origin at floor(p * 2^-l - hw), hw = (win - 1) / 2, and
`window_origin` restates exactly that, so every builder checks that the window it wants is the
window the kernel and the oracle will use."""
import numpy as np

from coeb_front import synth

# LK level byte sizes mod 4 at win 22, max_level 5: 32x32 (0), 45x45 (1, 1; level 1 is 23x23, one
# inside window), 46x47 (2, 0), 91x93 (3, 2, 0), 181x95 (3, 0, 0), 333x251 (3, 2, 0, 0),
# 427x321 (3, 2, 3, 2)
SIZES = ((32, 32), (45, 45), (46, 47), (91, 93), (181, 95), (333, 251), (427, 321))
LEVEL_BYTES_MOD4 = {(32, 32): [0], (45, 45): [1, 1], (46, 47): [2, 0], (91, 93): [3, 2, 0], (181, 95): [3, 0, 0],
                    (333, 251): [3, 2, 0, 0], (427, 321): [3, 2, 3, 2]}
WINS = (3, 7, 15, 21, 22)
MAX_LEVELS = (0, 3, 5, 7)
LK_MAX_LEVELS = 8                                   # kLkMaxLevels of csrc/coeb_flow.hip
SEED = 7


def pair(w, h, seed=SEED):
    """(prev, cur) of synth.make_frames at the size."""
    fr = synth.make_frames(w, h, 2, seed=seed)
    return fr[0], fr[1]


def lk_level_sizes(w, h, win, max_level):
    """The levels buildOpticalFlowPyramid keeps: a halved level no larger than the window ends it."""
    out = [(w, h)]
    for _ in range(max_level):
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= win or h <= win:
            break
        out.append((w, h))
    return out


def half_win(win):
    return np.float32(win - 1) * np.float32(0.5)


def window_origin(p, level, win):
    """floor(p * 2^-level - hw) in float32, as k_lk and oc_lk_pyr compute ipx / ipy."""
    return int(np.floor(np.float32(p) * np.float32(1.0 / (1 << level)) - half_win(win)))


def point_for(ip, frac, level, win):
    """The level-0 coordinate whose level-`level` window origin is ip + frac (frac in [0, 1))."""
    p = np.float32((np.float32(ip + frac) + half_win(win)) * np.float32(1 << level))
    assert window_origin(p, level, win) == ip, (ip, frac, level, win, p)
    return p


# names of the directed points of one level, in the order lk_directed emits them
DIRECTED = ("last_inside", "past_last_x", "past_last_y", "past_last_xy", "first_inside", "minus_one_x", "minus_one_y",
            "minus_win", "minus_win_1")


def lk_directed(w, h, win, max_level):
    """The directed points of every kept level and of the image: (points (n, 2) f32, names, levels,
    wanted (ipx, ipy)).  Per level l of size (lw, lh), with fractions .25 in x and .5 in y:
    the last window that is still inside (ipx = lw - win - 1, ipy = lh - win - 1: its +1 column and
    row are the level's last), the windows one pixel further in x, in y and in both (the reflect
    path), the first inside window (0, 0), the windows at ipx = -1 and at ipy = -1, the window at
    ipx = -win (the last one the range test keeps) and at ipx = -win - 1 (rejected at that level).
    Then (w - 1, h - 1) and two points outside the image (level -1)."""
    pts, names, levels, want = [], [], [], []
    for l, (lw, lh) in enumerate(lk_level_sizes(w, h, win, max_level)):
        lx, ly = lw - win - 1, lh - win - 1
        assert lx >= 0 and ly >= 0
        for name, (ix, iy) in zip(DIRECTED, ((lx, ly), (lx + 1, ly), (lx, ly + 1), (lx + 1, ly + 1), (0, 0), (-1, 0),
                                             (0, -1), (-win, ly // 2), (-win - 1, ly // 2))):
            pts.append((point_for(ix, 0.25, l, win), point_for(iy, 0.5, l, win)))
            names.append(name)
            levels.append(l)
            want.append((ix, iy))
    for name, p in (("image_corner", (w - 1, h - 1)), ("outside_right", (w + 40, 20)), ("outside_above", (h // 2, -3 - win))):
        pts.append(p)
        names.append(name)
        levels.append(-1)
        want.append((0, 0))
    return np.array(pts, np.float32), names, np.array(levels), np.array(want, np.int64)


def is_inside(ipx, ipy, lw, lh, win):
    """k_lk's `inside`: the window and its +1 column and row lie in the level."""
    return ipx >= 0 and ipy >= 0 and ipx + win < lw and ipy + win < lh


def lk_points(oracle_mod, prev, win, max_level):
    """The oracle's subpix corners of prev followed by the directed points: (points, number of
    natural corners, names, levels, wanted origins of the directed ones)."""
    corners = oracle_mod.corner_subpix(prev, oracle_mod.good_features(prev))
    d, names, levels, want = lk_directed(prev.shape[1], prev.shape[0], win, max_level)
    return np.concatenate([corners, d]).astype(np.float32), len(corners), names, levels, want


def assert_lk_coverage(w, h, win, max_level, nnat, names, levels, want, status):
    """What the LK grid must reach, judged on the oracle's status alone."""
    sizes = lk_level_sizes(w, h, win, max_level)
    dst = status[nnat:]
    for i, (name, l, (ix, iy)) in enumerate(zip(names, levels, want)):
        if l < 0:
            continue
        lw, lh = sizes[l]
        assert is_inside(ix, iy, lw, lh, win) == (name in ("last_inside", "first_inside")), (name, l, ix, iy, lw, lh)
        if l == 0 and name == "minus_win_1":
            assert dst[i] == 0, (w, h, win, max_level)               # rejected by the range test
    assert dst[names.index("outside_right")] == 0 and dst[names.index("outside_above")] == 0
    assert 9 <= nnat <= 76, (w, h, nnat)
    if win >= 15:
        # the level-0 last inside window and its neighbour past the edge are both tracked
        assert names[0] == "last_inside" and levels[0] == 0 and names[3] == "past_last_xy"
        assert dst[0] == 1 and dst[3] == 1, (w, h, win, max_level, dst[:4])
    else:
        assert 2 * int(status[:nnat].sum()) >= nnat, (w, h, win, max_level, int(status[:nnat].sum()), nnat)


def lk_grid(w, h):
    """(win, max_level) pairs of the grid that the entry accepts at this size."""
    return [(win, ml) for win in WINS for ml in MAX_LEVELS if len(lk_level_sizes(w, h, win, ml)) <= LK_MAX_LEVELS]


# ---- goodFeaturesToTrack
GF_MIN_DISTANCE = (1.0, 3.0, 7.5, 8.5, 20.0)       # lrint gives cells 1, 3, 8, 8, 20
GF_QUALITY = (0.01, 0.5)
GF_MAX_CORNERS = (1, 1024)


def gf_border_points(w, h):
    return [(x, y) for y in (1, h // 2, h - 2) for x in (1, w // 2, w - 2) if (x, y) != (w // 2, h // 2)]


def gf_border_image(w=48, h=40):
    """Single bright pixels whose Harris maxima sit on the first and last candidate rows and
    columns (1 and w - 2, 1 and h - 2), in the four corners and along each side, and a weaker one
    in the middle of the image."""
    img = np.full((h, w), 20, np.uint8)
    for x, y in gf_border_points(w, h):
        img[y, x] = 250
    img[h // 2, w // 2] = 120
    return img


def gf_ragged_images():
    """Widths that leave 1, 2 and 3 columns over k_gf_response's four-column groups."""
    base = synth.make_frames(64, 48, 1, seed=SEED)[0]
    return [np.ascontiguousarray(base[:33 + i, :36 + i]) for i in (1, 2, 3)]


# ---- cornerSubPix
SUBPIX_MARGIN = 14                                  # k_subpix_order's interior / border split


def subpix_edge_points(w, h):
    """Points at exactly 14.0 px (interior) and 13.99 px (border) from each image edge, and the
    same in each corner."""
    m = float(SUBPIX_MARGIN)
    lo, hi = (m, m - 0.01), lambda n: (n - 1 - m, n - 1 - m + 0.01)
    pts = []
    for v in lo:
        pts += [(v, h / 2), (w / 2, v)]
    for vx, vy in zip(hi(w), hi(h)):
        pts += [(vx, h / 2), (w / 2, vy)]
    for vx in lo + hi(w):
        for vy in lo + hi(h):
            pts.append((vx, vy))
    return np.array(pts, np.float32)


def subpix_is_interior(pts, w, h):
    m = np.float32(SUBPIX_MARGIN)
    return ((pts[:, 0] >= m) & (pts[:, 0] <= np.float32(w - 1 - SUBPIX_MARGIN)) & (pts[:, 1] >= m) &
            (pts[:, 1] <= np.float32(h - 1 - SUBPIX_MARGIN)))


def subpix_wander_image():
    return pair(181, 95)[0]


def subpix_wander_points(oracle_mod, img, nreset=24):
    """Start points in the 8 px band along the image edges, judged on the oracle: (points the
    iteration carries out of the image, where it stops; the first `nreset` points that moved by more
    than the window and were put back to their start -- the result equals the start although one
    iteration alone moves the point)."""
    h, w = img.shape
    ys, xs = np.mgrid[0:h, 0:w]
    band = (xs < 8) | (xs >= w - 8) | (ys < 8) | (ys >= h - 8)
    pts = np.stack([xs[band], ys[band]], 1).astype(np.float32) + np.float32(0.25)
    end = oracle_mod.corner_subpix(img, pts)
    one = oracle_mod.corner_subpix(img, pts, max_iter=1)
    out = (end[:, 0] < 0) | (end[:, 0] >= w) | (end[:, 1] < 0) | (end[:, 1] >= h)
    reset = (end == pts).all(1) & (one != pts).any(1)
    return pts[out], pts[reset][:nreset]


# ---- the MovingTail: SAD limit and image edge
SAD_LIMIT = 2120


def sad_pair(w, h, rng_seed=3):
    """A textured pair with hand-made 3x3 patches: point i of `exact` has a SAD of exactly 2120
    (kept), point i of `over` 2121 (dropped).  Returns (prev, cur, prev points, next points, SADs)."""
    prev, cur = (a.copy() for a in pair(w, h))
    pp, nn, sad = [], [], []
    k = 0
    for want in (SAD_LIMIT, SAD_LIMIT + 1, SAD_LIMIT, SAD_LIMIT + 1):
        x1, y1 = 12 + 9 * k, 10 + 5 * k
        x2, y2 = x1 + 2, y1 + 1
        k += 1
        prev[y1 - 1:y1 + 2, x1 - 1:x1 + 2] = 255
        cur[y2 - 1:y2 + 2, x2 - 1:x2 + 2] = 0
        cur[y2, x2] = 255 - (want - 8 * 255)                        # 8 * 255 + (want - 2040)
        pp.append((x1 + 0.5, y1 + 0.25))
        nn.append((x2 + 0.75, y2 + 0.5))
        sad.append(want)
    return prev, cur, np.array(pp, np.float32), np.array(nn, np.float32), np.array(sad)


def sad_of(prev, cur, p, q):
    x1, y1, x2, y2 = int(p[0]), int(p[1]), int(q[0]), int(q[1])
    a = prev[y1 - 1:y1 + 2, x1 - 1:x1 + 2].astype(np.int64)
    b = cur[y2 - 1:y2 + 2, x2 - 1:x2 + 2].astype(np.int64)
    return int(np.abs(a - b).sum())


def tail_edge_points(w, h):
    """Pairs whose truncated coordinate is 4 (dropped), 5 (kept), n - 6 (kept) or n - 5 (dropped)
    in x or in y, of the previous or of the next point, the other three coordinates mid-image:
    (prev points, next points, kept by the edge rule)."""
    pp, nn, keep = [], [], []
    for which in range(4):                                  # prev x, prev y, next x, next y
        n = w if which % 2 == 0 else h
        for v, ok in ((4.75, False), (5.25, True), (n - 6 + 0.5, True), (n - 5 + 0.125, False)):
            c = [w / 2 + 0.5, h / 2 + 0.25, w / 2 + 1.5, h / 2 - 0.25]
            c[which] = v
            pp.append(c[:2])
            nn.append(c[2:])
            keep.append(ok)
    return np.array(pp, np.float32), np.array(nn, np.float32), np.array(keep)
