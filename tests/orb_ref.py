"""A numpy model of the ORB extractor's per-level work, and directed small frames.

Written from the reference's text -- IC_Angle and computeOrbDescriptor (src/ORBextractor.cc:80-156),
the constructor's umax (:461-476), the FAST cell loop of ComputeKeyPointsOctTree (:795-860) and the
descriptor loop with the level-0 scaling of operator() (:1300-1340) -- and from the OpenCV
definitions tabulated in DESIGN.md s2.1, not from oracle/orb_oracle.c nor from the kernels:
tests/test_orb_ref.py compares the oracle with it and tests/test_gpu_orb_directed.py the kernels,
so that a mistake the oracle and the kernels share does not pass.

What is deliberately different from the oracle's restatement:
  * FAST-9/16 is its definition, evaluated over the 16 rotations of a 9-pixel arc for the whole
    level at once (the oracle restates OpenCV's FAST_t loop, the kernel a min/max doubling);
  * the disc of IC_Angle is a boolean mask built from umax, the moments are integer sums over it,
    and the angle is float64 atan2 (the value under test is the fastAtan2 polynomial);
  * the blur runs on an np.pad(mode="reflect") copy in integers;
  * rBRIEF takes the keypoint's float32 angle as given and rotates in float64; a test whose sample
    coordinate comes within UNDECIDED_EPS of a half-integer is returned as undecided, not compared.

The second half builds the directed frames shared by the CPU and the GPU test, and `kernel_view`,
which restates from DESIGN.md s4.2 / s4.4 the few launch quantities (slab layout, lanes per row,
corner-list capacity, survivor entries) the regime assertions are about.
"""
import math
import os
import re

import numpy as np

import octree_ref as OT
from octree_ref import f32, fast_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF_PATCH_SIZE = 15
PATCH_SIZE = 31
EDGE_THRESHOLD = 19
UNDECIDED_EPS = 1e-4
# largest |fastAtan2 - float64 atan2| in degrees (tests/test_orb_ref.py::test_angle_bound measures it),
# and the bound on |extractor's angle - model's|: twice that, for directions the sweep did not hit
ANGLE_MEASURED = 0.00956
ANGLE_BOUND = 2 * ANGLE_MEASURED

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

# the 16-pixel Bresenham circle of radius 3 as (dx, dy), in OpenCV's order (only contiguity matters)
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2),
        (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


# ------------------------------------------------------------------ resize (moved from test_oracle_kat.py)
def _py_resize_linear(src, dw, dh):
    """numpy restatement of OpenCV 3.4 resize INTER_LINEAR 8U on x86-64 (imgproc resize.cpp):
    11-bit coefficient tables, exact horizontal pass, vertical pass with the SSE2 rounding of
    VResizeLinearVec_32s8u up to its last column and FixedPtCast<int,uchar,22> after it."""
    sh, sw = src.shape
    sx_scale, sy_scale = 1.0 / (dw / sw), 1.0 / (dh / sh)

    def tab(n, scale, limit):
        ofs, c0, c1, xmax = [], [], [], n
        for d in range(n):
            f = np.float32((d + 0.5) * scale - 0.5)
            s = int(np.floor(f))
            f = np.float32(f - np.float32(s))
            if limit:
                if s < 0:
                    f, s = np.float32(0), 0
                if s + 1 >= sw:
                    xmax = min(xmax, d)
                    if s >= sw - 1:
                        f, s = np.float32(0), sw - 1
            ofs.append(s)
            c0.append(int(np.rint(np.float32(np.float32(1) - f) * np.float32(2048))))     # cvRound, half even
            c1.append(int(np.rint(np.float32(f) * np.float32(2048))))
        return np.array(ofs), np.array(c0), np.array(c1), xmax
    xofs, a0, a1, xmax = tab(dw, sx_scale, True)
    yofs, b0, b1, _ = tab(dh, sy_scale, False)
    x = (dw // 16) * 16 if dw >= 16 else 0
    while x < dw - 4:
        x += 4
    out = np.zeros((dh, dw), np.uint8)
    s = src.astype(np.int64)
    for dy in range(dh):
        r0 = min(max(yofs[dy], 0), sh - 1)
        r1 = min(max(yofs[dy] + 1, 0), sh - 1)
        h = []
        for r in (r0, r1):
            row = s[r]
            hx = np.where(np.arange(dw) < xmax, row[xofs] * a0 + row[np.minimum(xofs + 1, sw - 1)] * a1, row[xofs] * 2048)
            h.append(hx)
        simd = (((h[0] >> 4) * b0[dy]) >> 16) + (((h[1] >> 4) * b1[dy]) >> 16)
        simd = (simd + 2) >> 2
        exact = (h[0] * b0[dy] + h[1] * b1[dy] + (1 << 21)) >> 22
        v = np.where(np.arange(dw) < x, simd, exact)
        out[dy] = np.clip(v, 0, 255)
    return out


# ------------------------------------------------------------------ constructor tables (:418-477)
def pattern():
    """bit_pattern_31_ as (512, 2) ints (x, y), from the committed table"""
    txt = open(os.path.join(ROOT, "data", "orb_bit_pattern_31.inc")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return np.array([int(v) for v in re.findall(r"-?\d+", txt)], np.int64).reshape(512, 2)


def cv_round(v):
    """cvRound: nearest, halves to even"""
    return int(np.rint(v))


def make_umax():
    """:461-476"""
    umax = [0] * (HALF_PATCH_SIZE + 2)
    vmax = int(math.floor(f32(f32(HALF_PATCH_SIZE * f32(math.sqrt(2.0))) / 2) + 1))
    vmin = int(math.ceil(f32(f32(HALF_PATCH_SIZE * f32(math.sqrt(2.0))) / 2)))
    hp2 = float(HALF_PATCH_SIZE * HALF_PATCH_SIZE)
    for v in range(vmax + 1):
        umax[v] = cv_round(math.sqrt(hp2 - v * v))
    v0 = 0
    for v in range(HALF_PATCH_SIZE, vmin - 1, -1):
        while umax[v0] == umax[v0 + 1]:
            v0 += 1
        umax[v] = v0
        v0 += 1
    return umax[:HALF_PATCH_SIZE + 1]


def disc_mask(umax=None):
    """(31, 31) bool, [v + 15, u + 15]: |u| <= umax[|v|], the pixels IC_Angle sums (:87-104)"""
    umax = make_umax() if umax is None else umax
    v = np.abs(np.arange(-HALF_PATCH_SIZE, HALF_PATCH_SIZE + 1))
    u = np.abs(np.arange(-HALF_PATCH_SIZE, HALF_PATCH_SIZE + 1))
    return u[None, :] <= np.array(umax)[v][:, None]


class Tables:
    """mvScaleFactor, mvInvScaleFactor, mnFeaturesPerLevel (:422-453); scaleFactor is a double member
    initialised from the float argument"""

    def __init__(self, nfeatures, scale, nlevels):
        sf = float(np.float32(scale))
        self.nlevels = nlevels
        self.scale = [1.0]
        for _ in range(1, nlevels):
            self.scale.append(f32(self.scale[-1] * sf))
        self.inv_scale = [f32(1.0 / s) for s in self.scale]
        factor = f32(1.0 / sf)
        nd = f32(f32(nfeatures * f32(1 - factor)) / f32(1 - f32(math.pow(factor, nlevels))))
        self.nfeat, tot = [], 0
        for _ in range(nlevels - 1):
            self.nfeat.append(cv_round(nd))
            tot += self.nfeat[-1]
            nd = f32(nd * factor)
        self.nfeat.append(max(nfeatures - tot, 0))

    def level_size(self, w, h, l):
        """:1348-1349"""
        return cv_round(f32(float(w) * self.inv_scale[l])), cv_round(f32(float(h) * self.inv_scale[l]))


def pyramid(img, tab):
    """ComputePyramid (:1344-1367): level l resized from level l - 1"""
    h, w = img.shape
    out = [np.ascontiguousarray(img, np.uint8)]
    for l in range(1, tab.nlevels):
        lw, lh = tab.level_size(w, h, l)
        out.append(_py_resize_linear(out[-1], lw, lh))
    return out


# ------------------------------------------------------------------ FAST-9/16
def fast_strength(img):
    """M[y, x]: the largest t + 1 at which (x, y) is a FAST-9/16 corner, 0 where it never is and on
    the 3-px border.  Corner at t <=> some 9 contiguous ring pixels are all > v + t or all < v - t
    <=> for some rotation the smallest of the arc's (ring - v), or of its (v - ring), exceeds t."""
    a = img.astype(np.int32)
    h, w = a.shape
    M = np.zeros((h, w), np.int32)
    if h < 7 or w < 7:
        return M
    v = a[3:h - 3, 3:w - 3]
    d = np.stack([a[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - v for dx, dy in RING])       # ring - v
    best = np.zeros_like(v)
    for s in range(16):
        arc = d[[(s + j) % 16 for j in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(axis=0), (-arc).min(axis=0)))     # bright arc, dark arc
    M[3:h - 3, 3:w - 3] = best
    return M


def fast_roi(M, t):
    """cv::FAST(roi, keys, t, nonmaxSuppression = true) on a ROI whose strengths are M (the ROI's own
    slice of fast_strength: a ring never leaves the ROI inside its 3-px inset).  Score M - 1 where
    M > t, else 0; a corner is kept iff its score is strictly above its 8 neighbours' (outside the
    inset: 0).  Returns (xs, ys, score) in raster order, ROI coordinates."""
    h, w = M.shape
    S = np.zeros((h, w), np.int32)
    if h >= 7 and w >= 7:
        inner = M[3:h - 3, 3:w - 3]
        S[3:h - 3, 3:w - 3] = np.where(inner > t, inner - 1, 0)
    P = np.pad(S, 1)
    keep = S > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= S > P[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    ys, xs = np.nonzero(keep)
    return xs, ys, S[ys, xs]


def level_cells(w, h):
    """the cells ComputeKeyPointsOctTree visits on a w x h level (:811-829), row-major:
    (i, j, x0, y0, x1, y1), the ROI being rows y0..y1-1 and columns x0..x1-1"""
    nCols, nRows, wCell, hCell, maxBX, maxBY = fast_grid(w, h)
    out = []
    for i in range(nRows):
        iniY = 16 + i * hCell
        if iniY >= maxBY - 3:
            continue
        maxY = min(iniY + hCell + 6, maxBY)
        for j in range(nCols):
            iniX = 16 + j * wCell
            if iniX >= maxBX - 6:
                continue
            out.append((i, j, iniX, iniY, min(iniX + wCell + 6, maxBX), maxY))
    return out


def level_candidates(lvl, ini_th, min_th, per_level_fallback=False):
    """vToDistributeKeys of one level (:811-850): per visited cell a dict(i, j, roi, th, xs, ys, score,
    ncorn_min) with keys relative to (16, 16) (ROI coordinates plus the cell's offset, :844-845), th
    the threshold that produced them (None for an empty cell) and ncorn_min the cell window's
    corners at min_th before NMS.  per_level_fallback is the mutant the tests must catch."""
    h, w = lvl.shape
    _, _, wCell, hCell, _, _ = fast_grid(w, h)
    M = fast_strength(lvl)
    cells = []
    for i, j, x0, y0, x1, y1 in level_cells(w, h):
        Mc = M[y0:y1, x0:x1].copy()
        # the ROI's own inset: strengths of pixels within 3 px of the ROI edge do not exist
        Mi = np.zeros_like(Mc)
        Mi[3:-3, 3:-3] = Mc[3:-3, 3:-3]
        res = {}
        for t in (ini_th, min_th):
            res[t] = fast_roi(Mi, t)
        cells.append(dict(i=i, j=j, roi=(x0, y0, x1, y1), res=res, ncorn_min=int((Mi > min_th).sum())))
    any_ini = any(len(c["res"][ini_th][0]) for c in cells)
    for c in cells:
        if per_level_fallback:
            t = ini_th if any_ini else min_th
        else:
            t = ini_th if len(c["res"][ini_th][0]) else min_th
        xs, ys, sc = c.pop("res")[t]
        c["th"] = t if len(xs) else None
        c["xs"], c["ys"], c["score"] = xs + c["j"] * wCell, ys + c["i"] * hCell, sc
    return cells


def flatten(cells):
    """the cells' keys as one list in the reference's order: (xs, ys, score) int lists"""
    xs = [int(v) for c in cells for v in c["xs"]]
    ys = [int(v) for c in cells for v in c["ys"]]
    sc = [int(v) for c in cells for v in c["score"]]
    return xs, ys, sc


# ------------------------------------------------------------------ IC_Angle
def ic_moments(lvl, x, y, mask=None):
    """(m01, m10) of IC_Angle (:80-104): exact integer sums of v I and u I over the disc"""
    mask = disc_mask() if mask is None else mask
    p = lvl[y - 15:y + 16, x - 15:x + 16].astype(np.int64) * mask
    r = np.arange(-15, 16)
    return int((p * r[:, None]).sum()), int((p * r[None, :]).sum())


def ic_angle(m01, m10):
    """the angle fastAtan2 approximates: degrees in [0, 360), float64"""
    return math.degrees(math.atan2(m01, m10)) % 360.0


def angle_diff(a, b):
    """|a - b| modulo 360"""
    return abs((float(a) - float(b) + 180.0) % 360.0 - 180.0)


# ------------------------------------------------------------------ blur
GAUSS_Q8 = np.array([18, 34, 48, 56, 48, 34, 18], np.int64)


def blur7(lvl):
    """GaussianBlur(7x7, sigma 2, BORDER_REFLECT_101) (:1318) as DESIGN.md s2.1 defines it: Q8 kernel,
    horizontal sums kept whole, vertical Q16 sum, (acc + 2^15) >> 16"""
    h, w = lvl.shape
    p = np.pad(lvl.astype(np.int64), 3, mode="reflect")
    hs = sum(GAUSS_Q8[k] * p[:, k:k + w] for k in range(7))
    acc = sum(GAUSS_Q8[k] * hs[k:k + h, :] for k in range(7))
    return ((acc + (1 << 15)) >> 16).astype(np.uint8)


# ------------------------------------------------------------------ rBRIEF
FACTOR_PI = float(np.float32(math.pi / np.float32(180.0)))      # (float)(CV_PI / 180.f)


def round_half_even(v):
    return np.rint(v).astype(np.int64)


def round_half_away(v):
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def brief(blurred, x, y, angle, pat=None, rnd=round_half_even, le=False, sincos=None):
    """computeOrbDescriptor (:110-156) at (x, y) of a blurred level for the float32 `angle` in degrees:
    (desc uint8[32], undecided bool[256]).  angle * factorPI is one float32 product; sin, cos and the
    rotated coordinates are float64.  rnd / le are the mutants the tests must catch; sincos = (sin,
    cos) replaces the angle's own (hand-worked cases with coordinates exactly on half-integers)."""
    pat = pattern() if pat is None else pat
    ang = float(np.float32(np.float32(angle) * np.float32(FACTOR_PI)))
    a, b = (math.cos(ang), math.sin(ang)) if sincos is None else (sincos[1], sincos[0])
    px, py = pat[:, 0].astype(np.float64), pat[:, 1].astype(np.float64)
    fr = px * b + py * a
    fc = px * a - py * b
    und = (np.abs(np.abs(fr - np.floor(fr)) - 0.5) < UNDECIDED_EPS) | (np.abs(np.abs(fc - np.floor(fc)) - 0.5) < UNDECIDED_EPS)
    val = blurred[y + rnd(fr), x + rnd(fc)].astype(np.int64)
    t0, t1 = val[0::2], val[1::2]
    bits = (t0 <= t1) if le else (t0 < t1)
    desc = np.packbits(bits.astype(np.uint8), bitorder="little")
    return desc, und[0::2] | und[1::2]


def unpack_bits(desc):
    """(n, 32) uint8 -> (n, 256) bits, bit k of byte i at 8 i + k"""
    return np.unpackbits(np.ascontiguousarray(desc, np.uint8), axis=-1, bitorder="little")


# ------------------------------------------------------------------ the extractor
def extract(img, nfeatures=1000, scale=1.2, nlevels=8, ini_th=20, min_th=7, angles=None, **mut):
    """operator() without boxes (:1199-1337).  Returns a dict:
      kps        KP_DTYPE records; `angle` holds the float64 atan2 angle rounded to float32
      angle64    the same in float64
      m01, m10   each keypoint's moments
      lx, ly     its integer position on its level
      desc, und  descriptors (n, 32) and undecided bits (n, 256), rotated by `angles` (float32, one
                 per keypoint: the extractor under test's own) or, when None, by kps["angle"]
      cells      per level the level_candidates list
      levels, blurred   the pyramid and its blurred copy
    mut: per_level_fallback, rnd, le (see level_candidates and brief)."""
    tab = Tables(nfeatures, scale, nlevels)
    pyr = pyramid(img, tab)
    mask = disc_mask()
    pat = pattern()
    recs, m01s, m10s, lxs, lys, a64, cells_all = [], [], [], [], [], [], []
    for l, lvl in enumerate(pyr):
        h, w = lvl.shape
        cells = level_candidates(lvl, ini_th, min_th, mut.get("per_level_fallback", False))
        cells_all.append(cells)
        xs, ys, sc = flatten(cells)
        kept = OT.distribute(xs, ys, sc, 16, w - 16, 16, h - 16, tab.nfeat[l])[0] if xs else []
        size = float(int(f32(PATCH_SIZE * tab.scale[l])))
        for k in kept:
            x, y = xs[k] + 16, ys[k] + 16
            m01, m10 = ic_moments(lvl, x, y, mask)
            ang = ic_angle(m01, m10)
            fx, fy = (float(x), float(y)) if l == 0 else (f32(x * tab.scale[l]), f32(y * tab.scale[l]))
            recs.append((fx, fy, size, ang, float(sc[k]), l, -1))
            m01s.append(m01), m10s.append(m10), lxs.append(x), lys.append(y), a64.append(ang)
    kps = np.array(recs, KP_DTYPE) if recs else np.zeros(0, KP_DTYPE)
    blurred = [blur7(lvl) for lvl in pyr]
    n = len(kps)
    use = kps["angle"] if angles is None else np.asarray(angles, np.float32)
    desc = np.zeros((n, 32), np.uint8)
    und = np.zeros((n, 256), bool)
    if len(use) == n:
        for i in range(n):
            desc[i], und[i] = brief(blurred[kps["octave"][i]], lxs[i], lys[i], use[i], pat,
                                    mut.get("rnd", round_half_even), mut.get("le", False))
    return dict(kps=kps, angle64=np.array(a64), m01=np.array(m01s, np.int64), m10=np.array(m10s, np.int64),
                lx=np.array(lxs, np.int64), ly=np.array(lys, np.int64), desc=desc, und=und, cells=cells_all,
                levels=pyr, blurred=blurred, tab=tab)


# ------------------------------------------------------------------ what the kernels make of a frame
FAST_CORNERS = 256       # k_fast's corner list: a cell with more corners at minTh takes the whole-window NMS
FAST_ENTRIES = 128       # its pre-test entry list, drained when a further pass of 64 lanes could overflow it


def kernel_view(w, h, tab):
    """DESIGN.md s4.2 in numbers, per level the visited cells' (ww, wh, ngrp, rows per pass) and for
    the plan the slab row bytes: 96 when every ROI is at most 46 wide, else 72."""
    levels, max_rw = [], 0
    for l in range(tab.nlevels):
        lw, lh = tab.level_size(w, h, l)
        cells = []
        for i, j, x0, y0, x1, y1 in level_cells(lw, lh):
            ww, wh = x1 - x0 - 6, y1 - y0 - 6
            ngrp = (ww + 3) >> 2
            cells.append(dict(i=i, j=j, ww=ww, wh=wh, ngrp=ngrp, rows_per_pass=4 if ngrp > 8 else 8))
            max_rw = max(max_rw, x1 - x0)
        levels.append(dict(w=lw, h=lh, cells=cells))
    return dict(levels=levels, row_bytes=96 if max_rw <= 46 else 72, max_roi_w=max_rw)


def entries_before_last_pass(lvl, cell, kv_cell, min_th):
    """A lower bound of k_fast's pre-test entries (groups of 4 window columns of one row with a
    survivor) before the cell's last pass: every corner at min_th survives the pre-test."""
    x0, y0, x1, y1 = cell["roi"]
    M = fast_strength(lvl)[y0 + 3:y1 - 3, x0 + 3:x1 - 3] > min_th
    rpp = kv_cell["rows_per_pass"]
    last = (M.shape[0] - 1) // rpp * rpp
    M = M[:last]
    pad = (-M.shape[1]) % 4
    G = np.pad(M, ((0, 0), (0, pad))).reshape(M.shape[0], -1, 4).any(axis=2)
    return int(G.sum())


# ------------------------------------------------------------------ directed frames
class Frame:
    """One test frame: image, extractor parameters (scale 1.2, thresholds 20 / 7 throughout), and
    `regime`, the name tests/test_orb_ref.py::check_regime asserts; `info` carries what the builder
    knows (patch centres and the like)."""

    def __init__(self, name, regime, img, nlevels, nfeatures=1000, **info):
        self.name, self.regime, self.img, self.nlevels, self.nfeatures, self.info = name, regime, img, nlevels, nfeatures, info
        self.h, self.w = img.shape

    def model(self, angles=None, **mut):
        return extract(self.img, self.nfeatures, 1.2, self.nlevels, 20, 7, angles=angles, **mut)


def flat(w, h, v=100):
    return np.full((h, w), v, np.uint8)


def faint_noise(w, h, seed, base=100, amp=6):
    """base + [0, amp]: no pixel pair differs by more than amp < minThFAST, so nothing here is a
    corner, yet moments and blurred comparisons are not all ties"""
    return (base + np.random.default_rng(seed).integers(0, amp + 1, (h, w))).astype(np.uint8)


def arcs_frame():
    """Arcs of exactly 8 and exactly 9 ring pixels 40 above (bright) or below (dark) a flat 100,
    from every start index: the centre is a corner (M = 40) iff the arc has 9."""
    img = flat(160, 120)
    centres = []
    p = 0
    for sense in (40, -40):
        for n in (8, 9):
            for s in range(16):
                cx, cy = 24 + 10 * (p % 12), 24 + 10 * (p // 12)
                for k in range(n):
                    dx, dy = RING[(s + k) % 16]
                    img[cy + dy, cx + dx] = 100 + sense
                centres.append((cx, cy, n, s, sense))
                p += 1
    return Frame("arcs_8_and_9", "arcs", img, 1, centres=centres)


def thresholds_frame():
    """Lone pixels d above a flat background have M = d.  Level 0 of 160 x 120 has 4 x 2 cells of
    32 x 44 detected pixels from (19, 19); one case per cell."""
    img = flat(160, 120)
    dots = {(0, 0): [(30, 30, 7)], (0, 1): [(62, 30, 8)], (0, 2): [(94, 30, 20)], (0, 3): [(126, 30, 21)],
            (1, 0): [(30, 70, 21), (40, 80, 20)], (1, 1): [(62, 70, 20), (72, 80, 8)],
            (1, 2): [(94, 70, 60), (95, 70, 15)], (1, 3): [(126, 70, 60), (127, 71, 20), (135, 90, 21)]}
    for cell in dots.values():
        for x, y, d in cell:
            img[y, x] = 100 + d
    # per cell: (threshold that produced the keys, [(x, y, score)])
    expect = {(0, 0): (None, []), (0, 1): (7, [(62, 30, 7)]), (0, 2): (7, [(94, 30, 19)]), (0, 3): (20, [(126, 30, 20)]),
              (1, 0): (20, [(30, 70, 20)]), (1, 1): (7, [(62, 70, 19), (72, 80, 7)]), (1, 2): (20, [(94, 70, 59)]),
              (1, 3): (20, [(126, 70, 59), (135, 90, 20)])}
    return Frame("threshold_equalities", "thresholds", img, 1, expect=expect)


def saturation_frame():
    """255 on 0 and 0 on 255: M = 255 in the dark and in the bright sense"""
    img = np.zeros((120, 160), np.uint8)
    img[:, 80:] = 255
    pts = [(30, 30), (60, 50), (40, 90), (19, 19), (100, 30), (130, 60), (110, 95), (140, 100)]
    for x, y in pts:
        img[y, x] = 255 - img[y, x]
    return Frame("saturation", "saturation", img, 1, points=pts)


def nms_ties_frame():
    """Adjacent corners of equal strength (pixels 50 above a flat 100: M = 50 each)."""
    img = flat(160, 120)
    groups = dict(row_pair=[(30, 30), (31, 30)], col_pair=[(62, 30), (62, 31)], diag_pair=[(30, 80), (31, 81)],
                  triple=[(126, 80), (127, 80), (128, 80)], pair_and_weak=[(62, 80), (63, 80)],
                  across_columns=[(114, 40), (115, 40)], across_rows=[(100, 62), (100, 63)])
    for g in groups.values():
        for x, y in g:
            img[y, x] = 150
    img[95, 75] = 110           # the weak corner of cell (1, 1): only the minTh pass finds it
    return Frame("nms_ties", "nms_ties", img, 1, groups=groups)


# the noise cell of corner_count_frame: pixels of the cell's ROI, in raster order, that are noise (the
# rest of the ROI is flat), found with the model for 255, 256 and 257 corners at minTh before NMS
CORNER_COUNT_FILL = {255: 739, 256: 740, 257: 744}


def corner_count_frame(n, fill=None):
    """160 x 120, two levels.  Level 0's cell (0, 1) (window columns 51..82, rows 19..62) holds uniform
    noise in the first `fill` pixels, in raster order, of columns 54..85 x rows 16..65 and has
    exactly n corners at minTh in its window; cell (0, 0) next to it (window up to column 50, rings
    up to 53) is flat and has none; the other cells hold lone dots."""
    img = flat(160, 120, 128)
    rng = np.random.default_rng(77)
    noise = rng.integers(0, 256, (50, 32), dtype=np.uint8)
    fill = CORNER_COUNT_FILL[n] if fill is None else fill
    roi = img[16:66, 54:86].reshape(-1).copy()
    roi[:fill] = noise.reshape(-1)[:fill]
    img[16:66, 54:86] = roi.reshape(50, 32)
    for x, y in ((100, 30), (130, 50), (30, 80), (60, 90), (100, 75), (125, 95)):
        img[y, x] = 255
    return Frame("corners_%d" % n, "corner_count", img, 2, n=n)


def noise_frame(name, regime, w, h, nlevels, seed, **info):
    return Frame(name, regime, np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8), nlevels, **info)


def count_frame(n):
    """64 x 64, one level: n pixels 100 above faint noise are the frame's n keypoints"""
    img = faint_noise(64, 64, 300 + n)
    pts = [(20 + 6 * (k % 5), 20 + 6 * (k // 5)) for k in range(n)]
    for x, y in pts:
        img[y, x] = 230
    return Frame("keypoints_%d" % n, "count", img, 1, n=n, points=pts)


def halfplane_patch(nx, ny, lo=0, hi=255, r=16):
    """(2r+1)^2 patch: hi where nx u + ny v >= 0, else lo, the centre halfway: the centre sees 9
    contiguous ring pixels of `hi` (the 7 strictly inside the half-plane and the 2 on its edge)"""
    u = np.arange(-r, r + 1)
    p = np.where(nx * u[None, :] + ny * u[:, None] >= 0, hi, lo).astype(np.uint8)
    p[r, r] = (lo + hi + 1) // 2
    return p


MOMENT_TILES = [("zero", None, 0.0), ("east", (1, 0), 0.0), ("west", (-1, 0), 180.0), ("south", (0, 1), 90.0),
                ("north", (0, -1), 270.0), ("se", (1, 1), 45.0), ("sw", (-1, 1), 135.0), ("nw", (-1, -1), 225.0),
                ("ne", (1, -1), 315.0), ("zero_dark", None, 0.0), ("east_weak", (1, 0), 0.0), ("west_mid", (-1, 0), 180.0)]


def moments_frame():
    """160 x 120, one level: twelve 33 x 33 tiles on 128, each around one FAST corner whose disc
    has the moments its name says (image y grows downwards: `south` is m01 > 0, 90 degrees)."""
    img = flat(160, 120, 128)
    centres = {}
    for k, (name, n, ang) in enumerate(MOMENT_TILES):
        cx, cy = 24 + 37 * (k % 4), 22 + 37 * (k // 4)
        if name == "zero":
            p = flat(33, 33, 60)
            p[16, 16] = 200
        elif name == "zero_dark":
            p = flat(33, 33, 255)
            p[16, 16] = 0
        elif name == "east_weak":
            p = halfplane_patch(*n, lo=100, hi=140)          # M = 20: a corner at minTh only
        elif name == "west_mid":
            p = halfplane_patch(*n, lo=50, hi=200)
        else:
            p = halfplane_patch(*n)
        img[cy - 16:cy + 17, cx - 16:cx + 17] = p
        centres[name] = (cx, cy, ang)
    return Frame("moments", "moments", img, 1, centres=centres)


def span_frame():
    """128 x 96, three levels, three pixels on faint noise: a handful of keypoints on every level, so
    the first wave of 8 spans levels"""
    img = faint_noise(128, 96, 41)
    for x, y in ((40, 40), (80, 50), (60, 70)):
        img[y - 1:y + 1, x - 1:x + 1] = 255
    for x, y in ((30, 60), (100, 30)):         # corners at minTh only, alone in their cells; gone on level 1
        img[y, x] = 115
    return Frame("wave_spans_levels", "span", img, 3)


_FRAMES = None


def frames():
    """Every directed frame, by name."""
    global _FRAMES
    if _FRAMES is None:
        out = [arcs_frame(), thresholds_frame(), saturation_frame(), nms_ties_frame(), moments_frame(), span_frame()]
        out += [corner_count_frame(n) for n in (255, 256, 257)]
        out += [count_frame(n) for n in (0, 1, 7, 8, 9, 17)]
        # 160 x 120 x 3: every ROI <= 46 wide (96-byte slab rows); windows 26, 27, 32, 33, 34, 40 wide
        out.append(noise_frame("noise_160x120_L3", "noise96", 160, 120, 3, 5))
        # 128 x 96 x 3: level 2 is 89 x 67, one cell with a 57-px ROI (72-byte slab rows)
        out.append(noise_frame("noise_128x96_L3", "noise72", 128, 96, 3, 6))
        # level 1 is 91 x 62: the widest single-cell level (ROI 59); and 62 x 62: the narrowest (ROI 30)
        out.append(noise_frame("single_cell_91", "single91", 109, 74, 2, 7))
        out.append(noise_frame("single_cell_62", "single62", 74, 74, 2, 8))
        _FRAMES = {f.name: f for f in out}
    return _FRAMES


def random_frames():
    """A few undirected small frames: smooth texture with some contrast, ragged sizes."""
    out = []
    for k, (w, h, L) in enumerate(((97, 71, 1), (141, 100, 2), (157, 117, 3))):
        rng = np.random.default_rng(900 + k)
        g = rng.integers(0, 256, (h // 4 + 2, w // 4 + 2)).astype(np.float64)
        g = np.kron(g, np.ones((4, 4)))[:h, :w]
        g = (g + np.roll(g, 1, 0) + np.roll(g, 1, 1) + np.roll(g, (1, 1), (0, 1))) / 4 + rng.integers(0, 12, (h, w))
        out.append(Frame("random_%dx%d_L%d" % (w, h, L), "random", np.clip(g, 0, 255).astype(np.uint8), L))
    return out
