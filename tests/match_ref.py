"""Literal Python models of the three projection searches, their traces, and directed scenes.

Models (written from the reference's text and DESIGN.md s2.1's canonical float forms, not from
the oracle's C restatement; tests/test_match_ref.py and tests/test_oracle_kat.py compare the two,
so that each pins the other):
  py_search_by_projection  ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono)  ORBmatcher.cc:1329-1471
  py_search_local_map      ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>, th)     ORBmatcher.cc:44-129
  py_search_keyframe       ORBmatcher::SearchByProjection(Frame&, KeyFrame*, set, th, dist)  ORBmatcher.cc:1473-1600
with Frame::AssignFeaturesToGrid / PosInGrid (Frame.cc:396-411, 553-568) and GetFeaturesInArea
(:503-551) shared by the three (Grid).

A trace (trace_frame, trace_local, trace_keyframe) says what the device kernels of
coeb_match.hip would meet on an input: the candidate list of every query (the candidates that
pass the filters which do not depend on earlier queries, in enumeration order), and a simulation
of DESIGN.md s4.5's Jacobi claim fixpoint on those lists with the kernel's sweep count.

The second half builds scenes by hand (Layout): current keypoints and queries at chosen pixels
with chosen Hamming distances, for all three matchers from one description.  scenes(cams) is the
list shared by tests/test_match_ref.py (CPU: models against the oracle, and every scene reaches the
regime it is named after) and tests/test_gpu_match_scenes.py.

Float arithmetic: numpy float32 scalars give the float32 result of one +, -, * or / exactly; a
fused multiply-add is evaluated in double (the product of two float32 is exact there).
"""
import math

import numpy as np

f32, f64 = np.float32, np.float64
COLS, ROWS = 64, 48
TH_HIGH = 100
HISTO_LENGTH = 30
K_CQ = 64            # coeb_match_dev.hpp kCQ: a candidate list's capacity
K_MAX_ITER = 64      # coeb_match.hip kMaxIter
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())


def c_round(v):
    """round(float), half away from zero"""
    v = float(v)
    return int(math.copysign(math.floor(abs(v) + 0.5), v))


class Grid:
    """Frame::AssignFeaturesToGrid and GetFeaturesInArea over one frame's keypoints."""

    def __init__(self, cam, kps):
        self.cam, self.kps = cam, kps
        self.x = [f32(v) for v in kps["x"]]
        self.y = [f32(v) for v in kps["y"]]
        self.oct = [int(v) for v in kps["octave"]]
        self.cells = [[[] for _ in range(ROWS)] for _ in range(COLS)]
        self.off_grid = 0
        minx, miny, gw, gh = f32(cam.min_x), f32(cam.min_y), f32(cam.grid_inv_w), f32(cam.grid_inv_h)
        for i in range(len(kps)):
            px = c_round((self.x[i] - minx) * gw)            # PosInGrid
            py = c_round((self.y[i] - miny) * gh)
            if 0 <= px < COLS and 0 <= py < ROWS:
                self.cells[px][py].append(i)
            else:
                self.off_grid += 1

    def window(self, x, y, r):
        """(x0, x1, y0, y1) of GetFeaturesInArea's cell range, or None when it misses the grid"""
        cam = self.cam
        x, y, r = f32(x), f32(y), f32(r)
        minx, miny, gw, gh = f32(cam.min_x), f32(cam.min_y), f32(cam.grid_inv_w), f32(cam.grid_inv_h)
        x0 = max(0, math.floor(float((x - minx - r) * gw)))
        if x0 >= COLS:
            return None
        x1 = min(COLS - 1, math.ceil(float((x - minx + r) * gw)))
        if x1 < 0:
            return None
        y0 = max(0, math.floor(float((y - miny - r) * gh)))
        if y0 >= ROWS:
            return None
        y1 = min(ROWS - 1, math.ceil(float((y - miny + r) * gh)))
        if y1 < 0:
            return None
        return x0, x1, y0, y1

    def in_area(self, x, y, r, minL, maxL):
        out = []
        w = self.window(x, y, r)
        if w is None:
            return out
        x, y, r = f32(x), f32(y), f32(r)
        chk = minL > 0 or maxL >= 0
        for ix in range(w[0], w[1] + 1):
            for iy in range(w[2], w[3] + 1):
                for j in self.cells[ix][iy]:
                    if chk and (self.oct[j] < minL or (maxL >= 0 and self.oct[j] > maxL)):
                        continue
                    if abs(self.x[j] - x) < r and abs(self.y[j] - y) < r:
                        out.append(j)
        return out


def _project(cam, T, X):
    """x3Dc = Rcw * x3Dw + tcw as cv::Mat's small gemm rounds it (float products summed left to
    right, the translation added in double), invzc, and u, v with the fused multiply-add of the
    reference binary.  Returns (u, v, invzc)."""
    p3 = []
    for k in range(3):
        t = f32(T[k, 0] * X[0]) + f32(T[k, 1] * X[1])
        t = f32(t + f32(T[k, 2] * X[2]))
        p3.append(f32(f64(t) + f64(T[k, 3])))
    invz = f32(1.0 / f64(p3[2]))
    u = f32(f64(f32(f32(cam.fx) * p3[0])) * f64(invz) + f64(f32(cam.cx)))
    v = f32(f64(f32(f32(cam.fy) * p3[1])) * f64(invz) + f64(f32(cam.cy)))
    return u, v, invz


def _cam_centre(T):
    """twc = -Rcw^T * tcw, accumulated in double"""
    out = []
    for k in range(3):
        s = f64(T[0, k]) * f64(T[0, 3]) + f64(T[1, k]) * f64(T[1, 3])
        s = s + f64(T[2, k]) * f64(T[2, 3])
        out.append(f32(s * -1.0))
    return out


def rot_bin(a_query, a_cur):
    rot = f32(f32(a_query) - f32(a_cur))
    if rot < 0:
        rot = f32(rot + f32(360.0))
    b = c_round(f32(rot * f32(1.0 / HISTO_LENGTH)))
    return 0 if b == HISTO_LENGTH else b


def three_maxima(h):
    """ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:1602-1643)"""
    m1 = m2 = m3 = 0
    i1 = i2 = i3 = -1
    for i in range(len(h)):
        if h[i] > m1:
            m3, m2, m1, i3, i2, i1 = m2, m1, h[i], i2, i1, i
        elif h[i] > m2:
            m3, m2, i3, i2 = m2, h[i], i2, i
        elif h[i] > m3:
            m3, i3 = h[i], i
    if m2 < f32(0.1) * f32(m1):
        i2 = i3 = -1
    elif m3 < f32(0.1) * f32(m1):
        i3 = -1
    return i1, i2, i3


def _rotation_filter(match, hist, nm):
    h = [0] * HISTO_LENGTH
    for _, b in hist:
        h[b] += 1
    keep = three_maxima(h)
    for bi, b in hist:
        if b not in keep:
            match[bi] = -1
            nm -= 1
    return nm, h


# ---------------------------------------------------------------- the windows of each search
def _frame_windows(cam, last, Tc, Tl, th, bmono):
    """Per LastFrame point: None, or (u, v, radius, minL, maxL, ur) (ORBmatcher.cc:1339-1391)."""
    Tc, Tl = np.asarray(Tc, f32), np.asarray(Tl, f32)
    twc = _cam_centre(Tc)
    tlc2 = f32(Tl[2, 0] * twc[0]) + f32(Tl[2, 1] * twc[1])
    tlc2 = f32(tlc2 + f32(Tl[2, 2] * twc[2]))
    tlc2 = f32(f64(tlc2) + f64(Tl[2, 3]))
    fwd = bool(tlc2 > f32(cam.mb)) and not bmono
    bwd = bool(-tlc2 > f32(cam.mb)) and not bmono
    out = []
    for i in range(len(last["has_mp"])):
        out.append(None)
        if not last["has_mp"][i] or last["outlier"][i]:
            continue
        u, v, invz = _project(cam, Tc, last["xw"][i].astype(f32))
        if invz < 0:
            continue
        if u < f32(cam.min_x) or u > f32(cam.max_x) or v < f32(cam.min_y) or v > f32(cam.max_y):
            continue
        o = int(last["keys_un"]["octave"][i])
        r = f32(f32(th) * f32(cam.scale[o]))
        lv = (o, -1) if fwd else (0, o) if bwd else (o - 1, o + 1)
        ur = f32(f64(-f32(cam.bf)) * f64(invz) + f64(u))             # u - mbf * invzc, fused
        out[-1] = (u, v, r, lv[0], lv[1], ur)
    return out


def _local_windows(cam, mp, th):
    """Per local-map point: None, or (u, v, radius, minL, maxL, ur) (ORBmatcher.cc:48-78)."""
    out = []
    for q in range(len(mp["in_view"])):
        out.append(None)
        if not mp["in_view"][q]:
            continue
        lvl = int(mp["level"][q])
        r = f32(2.5) if f32(mp["view_cos"][q]) > f32(0.998) else f32(4.0)     # RadiusByViewingCos
        if th != 1.0:
            r = f32(r * f32(th))
        out[-1] = (f32(mp["proj_x"][q]), f32(mp["proj_y"][q]), f32(r * f32(cam.scale[lvl])), lvl - 1, lvl,
                   f32(mp["proj_xr"][q]))
    return out


def _kf_windows(cam, kf, T, th):
    """Per KeyFrame point: None, or (u, v, radius, minL, maxL, None) (ORBmatcher.cc:1489-1536)."""
    T = np.asarray(T, f32)
    Ow = _cam_centre(T)
    log_sf = f32(math.log(f64(f32(cam.scale[1]))))
    out = []
    for q in range(len(kf["valid"])):
        out.append(None)
        if not kf["valid"][q]:
            continue
        X = kf["world_pos"][q].astype(f32)
        u, v, _ = _project(cam, T, X)
        if u < f32(cam.min_x) or u > f32(cam.max_x) or v < f32(cam.min_y) or v > f32(cam.max_y):
            continue
        d = [f32(X[k] - Ow[k]) for k in range(3)]
        ss = 0.0
        for k in range(3):
            ss += f64(d[k]) * f64(d[k])
        dist3 = f32(math.sqrt(ss))
        if dist3 < f32(f32(0.8) * f32(kf["min_distance"][q])) or dist3 > f32(f32(1.2) * f32(kf["max_distance"][q])):
            continue
        ratio = f32(f32(kf["max_distance"][q]) / dist3)
        lvl = int(math.ceil(f32(f32(math.log(f64(ratio))) / log_sf)))        # MapPoint::PredictScale
        lvl = min(max(lvl, 0), cam.nlevels - 1)
        out[-1] = (u, v, f32(f32(th) * f32(cam.scale[lvl])), lvl - 1, lvl + 1, None)
    return out


def _stereo_ok(w, ur_i):
    """ORBmatcher.cc:1408-1414 / :90-95: the right-image coordinate within the radius"""
    return not (ur_i > 0 and abs(f32(w[5] - f32(ur_i))) > w[2])


# ---------------------------------------------------------------- the three literal loops
def py_search_by_projection(cam, kps, desc, ur, last, Tc, Tl, th, bmono, check_ori):
    g = Grid(cam, kps)
    owner = [-1] * len(kps)
    hist = []
    nm = 0
    for i, w in enumerate(_frame_windows(cam, last, Tc, Tl, th, bmono)):
        if w is None:
            continue
        best, bi = 256, -1
        for i2 in g.in_area(*w[:5]):
            if owner[i2] >= 0 and last["mp_nobs"][owner[i2]] > 0:
                continue
            if not _stereo_ok(w, ur[i2]):
                continue
            d = hamming(last["mp_desc"][i], desc[i2])
            if d < best:
                best, bi = d, i2
        if best <= TH_HIGH:
            owner[bi] = i
            nm += 1
            if check_ori:
                hist.append((bi, rot_bin(last["keys_un"]["angle"][i], kps["angle"][bi])))
    if check_ori:
        nm, _ = _rotation_filter(owner, hist, nm)
    return nm, np.array(owner, np.int32)


def py_search_local_map(cam, kps, desc, ur, cur_obs, mp, th, nnratio):
    g = Grid(cam, kps)
    holder = list(cur_obs)
    match = [-1] * len(kps)
    nm = 0
    for q, w in enumerate(_local_windows(cam, mp, th)):
        if w is None:
            continue
        best, bl, best2, bl2, bi = 256, -1, 256, -1, -1
        for idx in g.in_area(*w[:5]):
            if holder[idx] > 0:
                continue
            if not _stereo_ok(w, ur[idx]):
                continue
            d = hamming(mp["descriptor"][q], desc[idx])
            if d < best:
                best2, bl2, best, bl, bi = best, bl, d, g.oct[idx], idx
            elif d < best2:
                bl2, best2 = g.oct[idx], d
        if best <= TH_HIGH:
            if bl == bl2 and f32(best) > f32(nnratio) * f32(best2):
                continue
            match[bi] = q
            holder[bi] = int(mp["observations"][q])
            nm += 1
    return nm, np.array(match, np.int32)


def py_search_keyframe(cam, kps, desc, cur_has, kf, T, th, orb_dist, check_ori):
    g = Grid(cam, kps)
    taken = [bool(h) for h in cur_has]
    match = [-1] * len(kps)
    hist = []
    nm = 0
    for q, w in enumerate(_kf_windows(cam, kf, T, th)):
        if w is None:
            continue
        best, bi = 256, -1
        for j in g.in_area(*w[:5]):
            if taken[j]:
                continue
            d = hamming(kf["descriptor"][q], desc[j])
            if d < best:
                best, bi = d, j
        if best <= orb_dist:
            taken[bi] = True
            match[bi] = q
            nm += 1
            if check_ori:
                hist.append((bi, rot_bin(kf["angle"][q], kps["angle"][bi])))
    if check_ori:
        nm, _ = _rotation_filter(match, hist, nm)
    return nm, np.array(match, np.int32)


# ---------------------------------------------------------------- traces
def _pick_first_min(cands):
    """first strict minimum of (dist) in list order; cands: [(pos, idx, dist, oct)]"""
    best, bi = 256, -1
    for _, idx, d, _ in cands:
        if d < best:
            best, bi = d, idx
    return bi


def _pick_local(nnratio):
    def pick(cands):
        best, bl, best2, bl2, bi = 256, -1, 256, -1, -1
        for _, idx, d, o in cands:
            if d < best:
                best2, bl2, best, bl, bi = best, bl, d, o, idx
            elif d < best2:
                bl2, best2 = o, d
        if best <= TH_HIGH and not (bl == bl2 and f32(best) > f32(nnratio) * f32(best2)):
            return bi
        return -1
    return pick


def _trace(g, wins, lists, blocks, pick):
    """lists[q]: None (no window) or [(idx, dist, oct)] in enumeration order; blocks[q]: q's
    assignment keeps later queries off its keypoint.  Simulates coeb_match.hip's fixpoint: sweep
    `it` recomputes every query against owner[c] = the least blocking p with res_p = c of the
    sweep before (none in sweep 0); a candidate is open to q when owner[c] >= q.  The kernel counts
    the sweep that changes nothing, gives up when sweep kMaxIter still changed something (path 3),
    and does not sweep at all when a list overflows kCQ (path 2)."""
    nq = len(lists)
    ent = [None if l is None else [(p, c[0], c[1], c[2]) for p, c in enumerate(l)] for l in lists]
    res = [-1] * nq
    owner = {}
    total = 0
    while True:
        new = [-1 if e is None else pick([c for c in e if owner.get(c[1], nq) >= q]) for q, e in enumerate(ent)]
        total += 1
        changed = total == 1 or new != res
        res = new
        if not changed:
            break
        owner = {}
        for q, r in enumerate(res):
            if r >= 0 and blocks[q] and owner.get(r, nq) > q:
                owner[r] = q
    counts = [-1 if l is None else len(l) for l in lists]
    max_count = max([c for c in counts] + [0])
    overflow = max_count > K_CQ
    converged = total <= K_MAX_ITER + 1
    ties = 0
    win_pos = [-1] * nq
    for q, e in enumerate(ent):
        if e is None or res[q] < 0:
            continue
        free = [c for c in e if owner.get(c[1], nq) >= q]
        w = [c for c in free if c[1] == res[q]][0]
        win_pos[q] = w[0]
        if any(c[1] != w[1] and c[2] == w[2] for c in free):
            ties += 1
    spans = [None if w is None else g.window(w[0], w[1], w[2]) for w in wins]
    return dict(counts=counts, max_count=max_count, res=res,
                sweeps=0 if overflow else min(total, K_MAX_ITER + 1),
                path=2 if overflow else 0 if converged else 3,
                ties=ties, win_pos=win_pos,
                pos_ge={k: sum(1 for p in win_pos if p >= k) for k in (8, 12, 16)},
                win_cols=[None if s is None else s[1] - s[0] + 1 for s in spans],
                win_rows=[None if s is None else s[3] - s[2] + 1 for s in spans],
                off_grid=g.off_grid)


def _hist_of(res, angle_q, kps):
    h = [0] * HISTO_LENGTH
    for q, r in enumerate(res):
        if r >= 0:
            h[rot_bin(angle_q[q], kps["angle"][r])] += 1
    return h


def trace_frame(cam, kps, desc, ur, last, Tc, Tl, th, bmono, check_ori=True):
    """k_match's lists: window, levels, stereo check, dist <= TH_HIGH"""
    g = Grid(cam, kps)
    wins = _frame_windows(cam, last, Tc, Tl, th, bmono)
    lists = []
    for i, w in enumerate(wins):
        if w is None:
            lists.append(None)
            continue
        l = []
        for i2 in g.in_area(*w[:5]):
            if _stereo_ok(w, ur[i2]):
                d = hamming(last["mp_desc"][i], desc[i2])
                if d <= TH_HIGH:
                    l.append((i2, d, g.oct[i2]))
        lists.append(l)
    t = _trace(g, wins, lists, [n > 0 for n in last["mp_nobs"]], _pick_first_min)
    t["hist"] = _hist_of(t["res"], last["keys_un"]["angle"], kps)
    return t


def trace_local(cam, kps, desc, ur, cur_obs, mp, th, nnratio):
    """k_match_local's lists: window, levels, entry holders with Observations() > 0, stereo
    check; every candidate counts, whatever its distance"""
    g = Grid(cam, kps)
    wins = _local_windows(cam, mp, th)
    lists = []
    for q, w in enumerate(wins):
        if w is None:
            lists.append(None)
            continue
        lists.append([(i2, hamming(mp["descriptor"][q], desc[i2]), g.oct[i2]) for i2 in g.in_area(*w[:5])
                      if cur_obs[i2] <= 0 and _stereo_ok(w, ur[i2])])
    return _trace(g, wins, lists, [n > 0 for n in mp["observations"]], _pick_local(nnratio))


def trace_keyframe(cam, kps, desc, cur_has, kf, T, th, orb_dist, check_ori=True):
    """k_match_kf's lists: window, levels, entry holders, dist <= ORBdist; every query blocks"""
    g = Grid(cam, kps)
    wins = _kf_windows(cam, kf, T, th)
    lists = []
    for q, w in enumerate(wins):
        if w is None:
            lists.append(None)
            continue
        l = []
        for i2 in g.in_area(*w[:5]):
            if not cur_has[i2]:
                d = hamming(kf["descriptor"][q], desc[i2])
                if d <= orb_dist:
                    l.append((i2, d, g.oct[i2]))
        lists.append(l)
    t = _trace(g, wins, lists, [True] * len(wins), _pick_first_min)
    t["hist"] = _hist_of(t["res"], kf["angle"], kps)
    return t


# ================================================================ scenes
def lead_bits(d):
    """A descriptor with its first d bits set: Hamming distance |a - b| between two of them."""
    out = np.zeros(32, np.uint8)
    out[: d // 8] = 255
    if d % 8:
        out[d // 8] = (1 << (d % 8)) - 1
    return out


def below(v):
    return np.nextafter(f32(v), f32(-np.inf))


def above(v):
    return np.nextafter(f32(v), f32(np.inf))


class Layout:
    """Current keypoints and queries by pixel, for the three matchers at once.

    A query meant for pixel (u, v) is the world point ((u - cx) z / fx, (v - cy) z / fy, z) at
    z = 1 under the identity pose; .pix(q) is where the models' projection then puts it (within
    float32 rounding of (u, v)), and the local-map form is given exactly that pixel, so the three
    matchers see one geometry.  Scenes that place a keypoint at an exact offset from a query take
    the offset from .pix()."""

    def __init__(self, cam):
        self.cam = cam
        self.k = []
        self.q = []

    def kp(self, x, y, bits=0, octave=0, angle=0.0, ur=-1.0, held=0):
        self.k.append(dict(x=f32(x), y=f32(y), desc=lead_bits(bits), octave=octave, angle=f32(angle), ur=f32(ur),
                           held=held))
        return len(self.k) - 1

    def query(self, u, v, bits=0, level=0, angle=0.0, nobs=1, valid=1, raw=False):
        """raw: the pixel is given to the local-map search as it is (it may lie off the image);
        the other two searches then get an invalid point."""
        cam = self.cam
        if raw:
            X, pu, pv, valid_p = np.array([0, 0, 1], f32), f32(u), f32(v), 0
        else:
            X = np.array([f32(f32(f32(u) - f32(cam.cx)) / f32(cam.fx)), f32(f32(f32(v) - f32(cam.cy)) / f32(cam.fy)), 1], f32)
            pu, pv, _ = _project(cam, np.eye(4, dtype=f32), X)
            valid_p = valid
        self.q.append(dict(X=X, u=pu, v=pv, desc=lead_bits(bits), level=level, angle=f32(angle), nobs=nobs,
                           valid=valid, valid_p=valid_p))
        return len(self.q) - 1

    def pix(self, q):
        return self.q[q]["u"], self.q[q]["v"]

    def shuffle_keypoints(self, seed):
        """Reorder the keypoints so that index order differs from the order they were placed in."""
        order = np.random.default_rng(seed).permutation(len(self.k))
        self.k = [self.k[i] for i in order]

    # ---- the current frame
    def cur(self):
        n = len(self.k)
        kps = np.zeros(n, KP_DTYPE)
        for f in ("x", "y", "angle", "octave"):
            kps[f] = [k[f] for k in self.k]
        kps["size"] = 31
        desc = np.stack([k["desc"] for k in self.k]) if n else np.zeros((0, 32), np.uint8)
        ur = np.array([k["ur"] for k in self.k], f32)
        held = np.array([k["held"] for k in self.k], np.int32)
        return kps, np.ascontiguousarray(desc), ur, held

    def _qdesc(self):
        return np.ascontiguousarray(np.stack([q["desc"] for q in self.q])) if self.q else np.zeros((0, 32), np.uint8)

    # ---- SearchByProjection(CurrentFrame, LastFrame): identity poses
    def frame(self):
        kps, desc, ur, _ = self.cur()
        m = len(self.q)
        lk = np.zeros(m, KP_DTYPE)
        lk["octave"] = [q["level"] for q in self.q]
        lk["angle"] = [q["angle"] for q in self.q]
        last = dict(has_mp=np.array([q["valid_p"] for q in self.q], np.uint8), outlier=np.zeros(m, np.uint8),
                    xw=np.array([q["X"] for q in self.q], f32).reshape(m, 3), mp_desc=self._qdesc(),
                    mp_nobs=np.array([q["nobs"] for q in self.q], np.int32), keys_un=lk)
        return dict(kps=kps, desc=desc, ur=ur, last=last, Tc=np.eye(4, dtype=f32), Tl=np.eye(4, dtype=f32))

    # ---- SearchByProjection(F, vpMapPoints): isInFrustum's outputs given directly
    def local(self):
        kps, desc, ur, held = self.cur()
        cam = self.cam
        m = len(self.q)
        px = np.array([q["u"] for q in self.q], f32)
        mp = dict(in_view=np.array([q["valid"] for q in self.q], np.uint8), proj_x=px,
                  proj_y=np.array([q["v"] for q in self.q], f32),
                  # u - mbf * invz at z = 1, as the frame search forms it
                  proj_xr=np.array([f32(f64(-f32(cam.bf)) + f64(u)) for u in px], f32),
                  level=np.array([q["level"] for q in self.q], np.int32), view_cos=np.ones(m, f32),
                  descriptor=self._qdesc(), observations=np.array([q["nobs"] for q in self.q], np.int32))
        return dict(kps=kps, desc=desc, ur=ur, cur_obs=np.where(held > 0, held, -1).astype(np.int32), mp=mp)

    # ---- SearchByProjection(CurrentFrame, pKF): identity pose, PredictScale = the query's level
    def keyframe(self):
        kps, desc, _, held = self.cur()
        m = len(self.q)
        xw = np.array([q["X"] for q in self.q], f32).reshape(m, 3)
        dist = np.sqrt((xw.astype(f64) ** 2).sum(1))
        lv = np.array([q["level"] for q in self.q], f64)
        # level 0: max distance under the point's (ratio < 1, clamped); level L: ratio 1.2^(L - 0.5)
        maxd = np.where(lv > 0, dist * f64(f32(self.cam.scale[1])) ** (lv - 0.5), dist * 0.9).astype(f32)
        kf = dict(valid=np.array([q["valid_p"] for q in self.q], np.uint8), world_pos=xw, descriptor=self._qdesc(),
                  max_distance=maxd, min_distance=(maxd * f32(0.1)).astype(f32),
                  angle=np.array([q["angle"] for q in self.q], f32))
        return dict(kps=kps, desc=desc, cur_has=(held > 0).astype(np.uint8), kf=kf, T=np.eye(4, dtype=f32))


class Scene:
    """One call of one matcher.  matcher: "frame" | "local" | "kf"; inputs: the matcher's arrays;
    kw: th, bmono / nnratio / orb_dist, check_ori; camera: None or "inside" (chain_util's bounded
    camera); expect: what the trace must show (test_match_scenes_reach_their_regimes); seq: the
    scene is run once more on the forced sequential path."""

    def __init__(self, name, matcher, inputs, kw, expect, camera=None, seq=False):
        self.name, self.matcher, self.inputs, self.kw = name, matcher, inputs, kw
        self.expect, self.camera, self.seq = expect, camera, seq
        self._trace = None
        self._model = None

    def __repr__(self):
        return self.name

    def trace(self, cam):
        if self._trace is None:
            i, k = self.inputs, self.kw
            if self.matcher == "frame":
                self._trace = trace_frame(cam, i["kps"], i["desc"], i["ur"], i["last"], i["Tc"], i["Tl"], k["th"],
                                          k["bmono"], k["check_ori"])
            elif self.matcher == "local":
                self._trace = trace_local(cam, i["kps"], i["desc"], i["ur"], i["cur_obs"], i["mp"], k["th"], k["nnratio"])
            else:
                self._trace = trace_keyframe(cam, i["kps"], i["desc"], i["cur_has"], i["kf"], i["T"], k["th"],
                                             k["orb_dist"], k["check_ori"])
        return self._trace

    def model(self, cam):
        if self._model is None:
            i, k = self.inputs, self.kw
            if self.matcher == "frame":
                self._model = py_search_by_projection(cam, i["kps"], i["desc"], i["ur"], i["last"], i["Tc"], i["Tl"],
                                                      k["th"], k["bmono"], k["check_ori"])
            elif self.matcher == "local":
                self._model = py_search_local_map(cam, i["kps"], i["desc"], i["ur"], i["cur_obs"], i["mp"], k["th"],
                                                  k["nnratio"])
            else:
                self._model = py_search_keyframe(cam, i["kps"], i["desc"], i["cur_has"], i["kf"], i["T"], k["th"],
                                                 k["orb_dist"], k["check_ori"])
        return self._model

    def oracle(self, O, cam):
        i, k = self.inputs, self.kw
        if self.matcher == "frame":
            return O.search_by_projection(cam, i["kps"], i["desc"], i["ur"], i["last"], i["Tc"], i["Tl"], k["th"],
                                          k["bmono"], k["check_ori"])
        if self.matcher == "local":
            return O.search_local_map(cam, i["kps"], i["desc"], i["ur"], i["cur_obs"], i["mp"], k["th"], k["nnratio"])
        return O.search_keyframe(cam, i["kps"], i["desc"], i["cur_has"], i["kf"], i["T"], k["th"], k["orb_dist"],
                                 k["check_ori"])


MATCHERS = ("frame", "local", "kf")


def _three(name, lay, r, expect, camera=None, seq=False, check_ori=False, nnratio=1.0, orb_dist=100, only=MATCHERS,
           expect_by=None):
    """The layout as one scene per matcher with window radius r at level 0: th = r for the frame
    and KeyFrame searches, th = r / 2.5 for the local map (RadiusByViewingCos = 2.5 at cos 1)."""
    out = []
    for m in only:
        e = dict(expect)
        e.update((expect_by or {}).get(m, {}))
        if m == "frame":
            out.append(Scene(name + "-frame", m, lay.frame(), dict(th=float(r), bmono=True, check_ori=check_ori), e,
                             camera, seq))
        elif m == "local":
            out.append(Scene(name + "-local", m, lay.local(), dict(th=float(r) / 2.5, nnratio=nnratio), e, camera, seq))
        else:
            out.append(Scene(name + "-kf", m, lay.keyframe(), dict(th=float(r), orb_dist=orb_dist, check_ori=check_ori),
                             e, camera, seq))
    return out


# ---- claim chains
CHAIN_K = (1, 8, 63, 64, 65, 66, 100)


def chain_layout(cam, K, break_every=0):
    """Keypoints c_0..c_K on a line 4 px apart, descriptors alternating E (no bit) and O (30 bits).
    Query q_0 sees c_0 alone and takes it.  Query q_k (k >= 1) sits between c_{k-1} and c_k, sees
    those two (radius 2.5) and is nearer in Hamming distance to c_{k-1} (10 against 20), which
    q_{k-1} holds: every query moves on by one, and the Jacobi fixpoint resolves one link per
    sweep.  break_every = 3: every third query has Observations() = 0 and blocks nobody."""
    lay = Layout(cam)
    for j in range(K + 1):
        lay.kp(100 + 4 * j, 200, bits=30 * (j & 1))
    lay.query(99, 200, bits=10)
    for k in range(1, K + 1):
        lay.query(100 + 4 * k - 2, 200, bits=10 if (k - 1) % 2 == 0 else 20,
                  nobs=0 if break_every and k % break_every == break_every - 1 else 1)
    return lay


def chain_scenes(cam):
    out = []
    for K in CHAIN_K:
        # sweep 0 sends every query to its favourite, sweeps 1..K move q_1..q_K on in turn, sweep
        # K + 1 changes nothing: K + 2 sweeps, and the kernel allows kMaxIter + 1 = 65
        e = dict(max_count=2, sweeps=min(K + 2, K_MAX_ITER + 1), path=0 if K + 2 <= K_MAX_ITER + 1 else 3,
                 nmatch=K + 1)
        out += _three("chain%d" % K, chain_layout(cam, K), 2.5, e, seq=True)
    # the chain broken at q_2: q_1 and q_2 move on, q_3 shares c_2 with q_2 (which blocks nobody), the rest
    # keep their favourites: 3 changing sweeps and the still one
    e = dict(max_count=2, sweeps=4, path=0)
    out += _three("chain100-broken", chain_layout(cam, 100, 3), 2.5, e, seq=True, only=("frame", "local"))
    return out


# ---- list lengths
LIST_M = (1, 7, 8, 9, 11, 12, 13, 15, 16, 17, 63, 64, 65)


def _threshold_windows(lay, thr):
    """Two more windows, far from the rest, with one candidate each: at distance thr (taken) and
    thr + 1 (not taken)."""
    lay.kp(100, 400, bits=thr)
    lay.query(100, 400)
    lay.kp(140, 400, bits=thr + 1)
    lay.query(140, 400)


def list_layout(cam, m, equal, hi, lo, extra=()):
    """m keypoints of one grid cell in one window of radius 5 (list order = index order).
    equal=False: distances hi, ..., hi, lo: the only minimum is the last entry.
    equal=True: all distances 0, and m - 1 earlier queries with the same window take the first
    m - 1 keypoints one after another: the last query's answer is entry m - 1 after m - 1 blocks.
    extra: distances of further keypoints in the window, first in index order."""
    lay = Layout(cam)
    for d in extra:
        lay.kp(304.5, 204.5, bits=d)
    for j in range(m):
        lay.kp(300 + 0.5 * (j % 8), 200 + 0.5 * (j // 8), bits=0 if equal else (lo if j == m - 1 else hi))
    for _ in range(m if equal else 1):
        lay.query(302, 202)
    _threshold_windows(lay, hi)
    return lay


def list_scenes(cam):
    out = []
    for m in LIST_M:
        path = 2 if m > K_CQ else 0
        for matcher, hi, lo in (("frame", 100, 50), ("local", 100, 50), ("kf", 50, 40)):
            # k_match and k_match_kf keep a candidate up to TH_HIGH / ORBdist only: one just above it, and
            # thirty more at m = 64, leave the list at m entries.  k_match_local keeps every candidate.
            extra = () if matcher == "local" else (hi + 1,) + (tuple(range(hi + 1, hi + 31)) if m == 64 else ())
            e = dict(max_count=m, path=path, sweeps=0 if path else 2, win_pos_last=m - 1, nmatch=2)
            out += _three("list%d-last" % m, list_layout(cam, m, False, hi, lo, extra), 5.0, e, seq=True,
                          orb_dist=hi, only=(matcher,))
            # equal distances: sweep t sends the queries t.. to keypoint t; the last moves in sweep m - 1 and
            # sweep m is still: m + 1 sweeps (65 at m = 64, the most the kernel allows)
            e = dict(max_count=m, path=path, sweeps=0 if path else m + 1, win_pos_last=m - 1, nmatch=m + 1,
                     min_ties=1 if m > 1 else 0)
            out += _three("list%d-equal" % m, list_layout(cam, m, True, hi, lo, extra), 5.0, e, seq=True,
                          orb_dist=hi, only=(matcher,))
    return out


# ---- query counts
NQ = (1023, 1024, 1025, 2047, 2048, 2049)


def nq_layout(cam, nq, n):
    """n current keypoints on a 12-px lattice, nq queries.  Even queries sit on a keypoint of their
    own (one-entry list), odd ones between lattice points (empty list).  The last three queries share
    a window over three keypoints A, B, C at distances 0, 10, 20 from each of them: they take A, B
    and C in turn, a blocking chain across the last three query indices."""
    lay = Layout(cam)
    pos = [(6 + 12 * (j % 52), 6 + 12 * (j // 52)) for j in range(n - 3)]
    for x, y in pos:
        lay.kp(x, y)
    for i in range(nq - 3):
        x, y = pos[i // 2]
        lay.query(x + (6 if i & 1 else 0), y + (6 if i & 1 else 0))
    for j in range(3):
        lay.kp(632 + 0.5 * j, 474, bits=10 * j)
    for _ in range(3):
        lay.query(632.5, 474)
    return lay


def nq_scenes(cam):
    # launch_match takes 512 threads per pair when the staged form fits half a CU:
    #   lds_form: full = 12304 (grid CSR) + 56 * n4 (sort, owner, float4 + 32-byte descriptor per
    #   keypoint) + 8 * q4 (res, qn); 512 threads <=> full + 256 <= 81920.
    #   n = 1000, nq <= 1025 (q4 = 1028): 12304 + 56000 + 8224 = 76528 -> 512 threads: register heads
    #     for queries < 2 * 512 = 1024, the late-queries loop from query 1024.
    #   n = 2000, nq <= 2049 (q4 = 2052): 12304 + 112000 + 16416 = 140720 <= 163584 (staged), > 81664
    #     -> 1024 threads: late queries from 2 * 1024 = 2048.
    # k_match_local and k_match_kf run 1024 threads on one frame whatever its size (late queries from 2048).
    out = []
    for nq in NQ:
        n = 1000 if nq < 2000 else 2000
        # sweep 0: all three on A; sweep 1: two on B; sweep 2: one on C; sweep 3 still
        e = dict(max_count=3, sweeps=4, path=0, nmatch=(nq - 3 + 1) // 2 + 3, n=n, nq=nq)
        out += _three("nq%d" % nq, nq_layout(cam, nq, n), 2.5, e)
    return out


def lds_bytes(n, nq):
    """coeb_match.hip match_lds_bytes of the staged form"""
    n4, q4 = (n + 3) & ~3, (nq + 3) & ~3
    return (((COLS * ROWS + 1) * 4 + 15) & ~15) + 56 * n4 + 8 * q4


# ---- enumeration order
ORDER_R = {1: 2.5, 4: 12.5, 5: 17.5, 8: 32.5, 9: 37.5}      # window columns -> radius (see order_layout)


def order_layout(cam, cols, seed):
    """Identical descriptors everywhere: a query takes the first open candidate of its list, so the
    result is the enumeration order itself (ix outer, iy inner, index order inside a cell).  Windows
    of radius ORDER_R[cols] whose left edge falls a quarter into a cell span `cols` columns
    (floor((u - r) / 10) .. ceil((u + r) / 10)); a one-column window exists only clipped at the right
    border.  Each window holds up to 40 keypoints, two to a position, placed at random and then
    shuffled, and six queries that take six of them in turn; a second window at the bottom border
    is clipped to fewer rows."""
    rng = np.random.default_rng(seed)
    r = ORDER_R[cols]
    lay = Layout(cam)
    if cols == 1:
        centres = [(636.0, 240.0), (636.0, 473.0)]               # the second: one row as well (row 47)
    else:
        # the second window is clipped at the bottom border: 2 rows (cols 4), 3 rows (cols 5)
        centres = [(302.5 + r, 202.5 + r), (102.5 + r, {4: 478.0, 5: 470.0}.get(cols, 480.0 - r))]
    for cu, cv in centres:
        npos = 6 if cols == 1 else 20
        for _ in range(npos):
            x = min(rng.uniform(cu - r + 0.2, cu + r - 0.2), 634.8)
            y = min(rng.uniform(cv - r + 0.2, cv + r - 0.2), 474.8)
            lay.kp(x, y)
            lay.kp(x + 0.05, y - 0.05 if y > 1 else y)
        for _ in range(6):
            lay.query(cu, cv)
    lay.shuffle_keypoints(seed)
    return lay


def cell_layout(cam, seed):
    """One grid cell with 64 keypoints, all in a window (a 64-entry list out of one cell), and one
    with 200 of which 50 lie in the window of its queries; indices shuffled.  Eight queries each."""
    rng = np.random.default_rng(seed)
    lay = Layout(cam)
    for _ in range(64):
        lay.kp(rng.uniform(296, 304), rng.uniform(196, 204))
    for _ in range(8):
        lay.query(300, 200)
    for j in range(200):
        lay.kp(rng.uniform(504.2, 504.9) if j < 50 else rng.uniform(495.1, 503.8), rng.uniform(196, 204))
    for _ in range(8):
        lay.query(509, 200)
    lay.shuffle_keypoints(seed)
    return lay


def order_scenes(cam):
    out = []
    for cols, r in ORDER_R.items():
        e = dict(path=0, min_ties=10, win_cols=cols, nmatch=12, max_count_le=K_CQ)
        out += _three("order-c%d" % cols, order_layout(cam, cols, 40 + cols), r, e)
    e = dict(path=0, min_ties=14, max_count=64, nmatch=16, cell_sizes=(64, 200))
    out += _three("order-cells", cell_layout(cam, 7), 5.0, e)
    return out


# ---- grid and window edges
EDGE_X = [5 + 10 * i for i in range(63)] + [634.9, 635, 639]
EDGE_Y = [5 + 10 * i for i in range(47)] + [474.9, 475, 479]


def edge_layout(cam):
    """Keypoints on the cell borders (x = 5, 15, ..: PosInGrid rounds half away from zero) and past
    the last column and row (x >= 635 rounds to column 64, y >= 475 to row 48: off the grid), a query
    on each; windows centred at the four corners and the mid-edges; keypoints at distance exactly
    r from a query in u and in v (the reference tests fabs(dist) < r) and one float32 step inside;
    uR error exactly at the radius (kept: er > radius drops) and one step above; for the local map
    (which takes any pixel) windows partly and wholly off the image."""
    lay = Layout(cam)
    for i, x in enumerate(EDGE_X):
        y = EDGE_Y[(7 * i) % len(EDGE_Y)]
        lay.kp(x, y, bits=i % 5)
        lay.query(x, y)
    for i, y in enumerate(EDGE_Y):
        x = EDGE_X[(11 * i + 3) % len(EDGE_X)]
        lay.kp(x, y, bits=i % 3)
        lay.query(x, y)
    for u, v in ((0, 0), (640, 0), (0, 480), (640, 480), (320, 0), (320, 480), (0, 240), (640, 240)):
        lay.kp(min(max(u, 1.5), 634.5) , min(max(v, 1.5), 474.5), bits=1)
        lay.query(u, v)
    r = f32(5.0)
    for j, (du, dv) in enumerate(((1, 0), (-1, 0), (0, 1), (0, -1))):
        q = lay.query(300 + 40 * j, 150)
        u, v = lay.pix(q)
        xe, ye = f32(u + du * r), f32(v + dv * r)
        assert abs(f32(xe - u)) == (r if du else 0) and abs(f32(ye - v)) == (r if dv else 0)
        lay.kp(xe, ye, bits=3)                                    # at r: outside
        q = lay.query(300 + 40 * j, 180)
        u, v = lay.pix(q)
        xe = below(u + r) if du > 0 else above(u - r) if du < 0 else u
        ye = below(v + r) if dv > 0 else above(v - r) if dv < 0 else v
        lay.kp(xe, ye, bits=3)                                    # one step inside
    for j, step in enumerate((0, 1, -1)):
        q = lay.query(400 + 30 * j, 300)
        u, v = lay.pix(q)
        urq = f32(f64(-f32(cam.bf)) + f64(u))
        ur = f32(urq - r)
        assert f32(urq - ur) == r
        ur = below(ur) if step > 0 else above(ur) if step < 0 else ur   # er = r + ulp / r - ulp
        lay.kp(u, v, bits=2, ur=ur)
    for u, v in ((-2, 100), (-50, 100), (700, 100), (300, -2), (300, -60), (300, 540), (641.5, 200), (300, 481.5)):
        lay.kp(min(max(u, 0.5), 634.0), min(max(v, 0.5), 474.0), bits=4)
        lay.query(u, v, raw=True)
    return lay


def edge_scenes(cams):
    out = []
    lay = edge_layout(cams[None])
    # x in {635, 639} (2 + their share of the second loop) and y in {475, 479} leave the grid
    off = sum(1 for k in lay.k if k["x"] >= 635 or k["y"] >= 475)
    e = dict(path=0, off_grid=off, min_off_grid=4, nmatch_min=100)
    out += _three("edges", lay, 5.0, e)
    # the same pixels under image bounds inside the image: keypoints left of min_x - half a cell or above
    # min_y - half a cell round to a negative cell, queries outside the bounds are rejected
    cam_b = cams["inside"]
    lay = edge_layout(cam_b)
    hw, hh = 0.5 / cam_b.grid_inv_w, 0.5 / cam_b.grid_inv_h
    off_min = sum(1 for k in lay.k if k["x"] < cam_b.min_x - hw - 0.01 or k["y"] < cam_b.min_y - hh - 0.01
                  or k["x"] > cam_b.max_x or k["y"] > cam_b.max_y)
    e = dict(path=0, min_off_grid=max(off_min, 20), nmatch_min=60)
    out += _three("edges-bounded", lay, 5.0, e, camera="inside")
    return out


# ---- rotation filter
def rot_layout(cam, rots):
    """One isolated keypoint and query per entry of rots = [(query angle, keypoint angle)]."""
    lay = Layout(cam)
    for j, (aq, ak) in enumerate(rots):
        x, y = 20 + 20 * (j % 30), 100 + 20 * (j // 30)
        lay.kp(x, y, angle=ak)
        lay.query(x, y, angle=aq)
    return lay


def _bin_members(b, n):
    """n (query angle, keypoint angle) pairs inside bin b: rot = 30 b + a few degrees"""
    return [(30.0 * b + 3.0 + 0.5 * j + 17.0, 17.0) for j in range(n)]


ROT_SHAPES = {
    # name: (pairs, histogram as {bin: count}, matches kept)
    "one-bin": (_bin_members(4, 12), {4: 12}, 12),
    "two-maxima": (_bin_members(3, 5) + _bin_members(9, 5) + _bin_members(1, 2) + _bin_members(20, 1),
                   {3: 5, 9: 5, 1: 2, 20: 1}, 12),
    # max2 = 1 against 0.1f * max1 = 1.0f: not smaller, both small bins stay; the fourth goes
    "ten-percent": (_bin_members(6, 10) + _bin_members(2, 1) + _bin_members(8, 1) + _bin_members(12, 1),
                    {6: 10, 2: 1, 8: 1, 12: 1}, 12),
    "three-equal": (_bin_members(5, 4) + _bin_members(7, 4) + _bin_members(11, 4) + _bin_members(15, 2),
                    {5: 4, 7: 4, 11: 4, 15: 2}, 12),
    # rot 14.99 / 15 / 15.01 (round(rot / 30) at a half bin), 345 (11.5), -20 and -0.25 before the + 360
    # wrap (bins 11 and 30 -> 0), beside ten in bin 3
    "half-bins": ([(14.99, 0.0), (15.0, 0.0), (15.01, 0.0), (345.0, 0.0), (10.0, 30.0), (0.0, 0.25)]
                  + _bin_members(3, 10), None, None),
}


def rot_scenes(cam):
    out = []
    for name, (pairs, hist, kept) in ROT_SHAPES.items():
        for ori in (True, False):
            e = dict(path=0, nmatch=(kept if ori else len(pairs)) if hist else None)
            if hist:
                e["hist"] = hist
            else:
                e["hist_bins_min"] = 4
            out += _three("rot-%s-%s" % (name, "on" if ori else "off"), rot_layout(cam, pairs), 2.5, e, check_ori=ori,
                          only=("frame", "kf"))
    return out


# ---- k_match_local's ratio test
def ratio_layout(cam):
    """Isolated windows (radius 5 at level 0), each one case of ORBmatcher.cc:97-121; .cases lists
    (name, query) for the expectations."""
    lay = Layout(cam)
    cases = []

    def win(name, cands, level=0, y=100):
        x = 30 + 40 * len(cases)
        q = lay.query(x, y, level=level)
        for j, c in enumerate(cands):
            lay.kp(x - 1 + j, y, bits=c[0], octave=c[1], held=c[2] if len(c) > 2 else 0)
        cases.append((name, q))

    win("40-50-one-level", [(40, 0), (50, 0)])           # bestDist == 0.8 * bestDist2: kept at 0.8
    win("30-50-one-level", [(30, 0), (50, 0)])           # bestDist == 0.6 * bestDist2 in exact arithmetic
    win("41-50-one-level", [(41, 0), (50, 0)])           # rejected at 0.8
    win("41-50-two-levels", [(41, 1), (50, 0)], level=1)  # no ratio test across levels
    win("best-100", [(100, 0)])
    win("best-101", [(101, 0)])
    win("second-held", [(41, 0), (45, 0, 2)])            # the second best holds a MapPoint with observations
    win("second-free", [(41, 0), (45, 0)])
    win("second-held-no-obs", [(41, 0), (45, 0, 0)])     # held, Observations() = 0: still a candidate
    win("level0", [(10, 0), (5, 1)])                     # window levels [-1, 0]: the octave-1 keypoint is out
    win("level7", [(10, 7), (12, 6), (5, 5)], level=7)   # window levels [6, 7]
    lay.cases = cases
    return lay


def ratio_scenes(cam):
    out = []
    lay = ratio_layout(cam)
    want = {0.8: {"40-50-one-level": 1, "30-50-one-level": 1, "41-50-one-level": 0, "41-50-two-levels": 1, "best-100": 1, "best-101": 0,
                  "second-held": 1, "second-free": 0, "second-held-no-obs": 0, "level0": 1, "level7": 1},
            # float(0.6) * 50 rounds to the float above 30: 30 is not greater, the match stays
            0.6: {"40-50-one-level": 0, "30-50-one-level": 1, "41-50-one-level": 0, "41-50-two-levels": 1, "best-100": 1, "best-101": 0,
                  "second-held": 1, "second-free": 0}}
    for ratio in (0.8, 0.6):
        e = dict(path=0, matched={q: want[ratio][name] for name, q in lay.cases if name in want[ratio]})
        out.append(Scene("ratio-%.1f-local" % ratio, "local", lay.local(), dict(th=2.0, nnratio=ratio), e))
    return out


def scenes(cams):
    """cams: {None: the 640x480 TUM camera, "inside": chain_util.BOUNDS_INSIDE's} (oracle Camera
    structs, or anything with their fields)."""
    cam = cams[None]
    return (chain_scenes(cam) + list_scenes(cam) + nq_scenes(cam) + order_scenes(cam) + edge_scenes(cams)
            + rot_scenes(cam) + ratio_scenes(cam))
