"""Tracking::TrackWithMotionModel on one frame as the CPU references compose it (no GPU):
Tracking::UpdateLastFrame's visual-odometry points (src/Tracking.cc:878-930, the sort and the loop
with its break written out literally; Frame::UnprojectStereo in numpy with the float forms of
DESIGN.md s2.1), ORBmatcher::SearchByProjection with the 2*th retry (oracle.search_by_projection),
Optimizer::PoseOptimization (oracle.pose_optimization) and the discard loop of :966-985 written
out literally.  Plus the scenes the TrackWithMotionModel tests share: no images, only points in
front of a camera, their projections and their descriptors."""
import functools

import numpy as np

import chain_util as cu
import coeb_front as cf
import oracle as O

TH, MIN_MATCHES, TH_DEPTH = 15.0, 20, 3.2           # RGB-D th (:948), `if (nmatches < 20)`, about 40 baselines
W, H = 640, 480
INTR = cu.TUM                                       # fx, fy, cx, cy, bf
# current x last sizes of the GPU test; MAIN is the scene most preconditions are asserted on.  The
# last pair is the largest coeb_match_lastframe takes: 4095 current keypoints, and the last-frame
# points that still fit the matcher's LDS beside them (match_lastframe_fits of csrc/coeb_match.hip:
# the unstaged match_lds_bytes and 512 bytes for k_match's static LDS within the CU's 160 KB).
MAIN = (300, 300)


def match_lds_bytes(n, q):
    return (((64 * 48 + 1) * 4 + 15) & ~15) + 2 * ((n + 3) & ~3) * 4 + 2 * ((q + 3) & ~3) * 4


LAST_MAX = ((160 * 1024 - 512 - match_lds_bytes(4095, 0)) // 8) // 4 * 4
SIZES = ((0, 0), (0, 5), (5, 0), (1, 1), (63, 65), (64, 64), (65, 63), (255, 257), MAIN, (1000, 1000), (4095, LAST_MAX))


@functools.lru_cache(maxsize=None)
def extractor():
    return O.Extractor()


@functools.lru_cache(maxsize=None)
def cameras(bounded=False):
    """(oracle Camera, coeb_front.Camera): ComputeImageBounds of an undistorted image, or bounds
    other than (0, w, 0, h)."""
    return cu.cameras(O, extractor(), W, H, INTR, cu.BOUNDS_INSIDE if bounded else None)


def pose(rx, ry, rz, t):
    """Tcw (float32 4x4) of a rotation by the three small angles and the translation t."""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T.astype(np.float32)


def project(T, xw):
    """Pixel position and depth of world points under Tcw (float64)."""
    Pc = np.asarray(xw, np.float64) @ T[:3, :3].astype(np.float64).T + T[:3, 3].astype(np.float64)
    fx, fy, cx, cy, _ = INTR
    return fx * Pc[:, 0] / Pc[:, 2] + cx, fy * Pc[:, 1] / Pc[:, 2] + cy, Pc[:, 2]


# ---- UpdateLastFrame ----
def twc_of(Tcw):
    """[mRwc | mOw] (float32 3x4) as Frame::UpdatePoseMatrices forms them: mRwc = mRcw.t(), mOw =
    -mRcw.t() * mtcw, a float product accumulated in double and scaled by -1 (GEMM_1_T)."""
    T = np.ascontiguousarray(Tcw, np.float32).reshape(4, 4)
    M = np.zeros((3, 4), np.float32)
    for k in range(3):
        s = np.float64(T[0, k]) * np.float64(T[0, 3]) + np.float64(T[1, k]) * np.float64(T[1, 3])
        s = s + np.float64(T[2, k]) * np.float64(T[2, 3])
        M[k, :3] = T[:3, k]
        M[k, 3] = np.float32(s * -1.0)
    return M


def unproject_stereo(kps, depth, Tcw, intr=INTR):
    """Frame::UnprojectStereo (Frame.cc:844-858) of every keypoint (rows of depth <= 0 are not
    meaningful): x3Dc = (((u - cx) z) invfx, ((v - cy) z) invfy, z) in float, then mRwc * x3Dc +
    mOw as cv::Mat computes it: the products summed in float, the addend added in double."""
    f32 = np.float32
    z = np.asarray(depth, f32)
    invfx, invfy = f32(1.0) / f32(intr[0]), f32(1.0) / f32(intr[1])
    with np.errstate(invalid="ignore", over="ignore"):
        x = ((kps["x"].astype(f32) - f32(intr[2])) * z) * invfx
        y = ((kps["y"].astype(f32) - f32(intr[3])) * z) * invfy
        M = twc_of(Tcw)
        out = np.zeros((len(z), 3), f32)
        for k in range(3):
            v = (M[k, 0] * x + M[k, 1] * y).astype(f32)
            v = (v + M[k, 2] * z).astype(f32)
            out[:, k] = (v.astype(np.float64) + np.float64(M[k, 3])).astype(f32)
    return out


def visited_loop(depth, th_depth):
    """The keypoints UpdateLastFrame's loop reaches, in its order (:880-930, literally)."""
    vDepthIdx = []
    for i in range(len(depth)):
        z = np.float32(depth[i])
        if z > 0:
            vDepthIdx.append((float(z), i))
    vDepthIdx.sort()
    out = []
    nPoints = 0
    for j in range(len(vDepthIdx)):
        out.append(vDepthIdx[j][1])
        nPoints += 1                                # both branches of bCreateNew count
        if vDepthIdx[j][0] > np.float32(th_depth) and nPoints > 100:
            break
    return out


def visited_closed_form(depth, th_depth):
    """The same set from ranks: with M entries of depth > 0, c of them not farther than th_depth,
    the entries of rank (from 0) <= max(c, 100)."""
    z = np.asarray(depth, np.float32)
    with np.errstate(invalid="ignore"):
        ok = z > 0
        idx = np.flatnonzero(ok)
        order = idx[np.lexsort((idx, z[idx]))]
        c = int((ok & ~(z > np.float32(th_depth))).sum())
    return [int(i) for i in order[:max(c, 100) + 1]]


def update_last_frame(last, depth, descriptors, th_depth, Tcw_last, intr=INTR):
    """-> (the last-frame dict after UpdateLastFrame, created u8[n], created_pos f32[n, 3] (zero
    where nothing was created))."""
    n = len(last["has_mp"])
    out = {k: np.array(v, copy=True) for k, v in last.items()}
    created, cpos = np.zeros(n, np.uint8), np.zeros((n, 3), np.float32)
    x3D = unproject_stereo(last["keys_un"], depth, Tcw_last, intr)
    for i in visited_loop(depth, th_depth):
        if not last["has_mp"][i] or last["mp_nobs"][i] < 1:
            out["has_mp"][i] = 1
            out["xw"][i] = x3D[i]
            out["mp_desc"][i] = descriptors[i]
            out["mp_nobs"][i] = 0
            created[i] = 1
            cpos[i] = x3D[i]
    return out, created, cpos


# ---- the discard loop ----
def discard_loop(match, outlier, last_obs, nmatches):
    """Tracking.cc:966-985, literally.  match: mvpMapPoints as last-frame slots (-1: NULL).
    -> (mvpMapPoints afterwards, discarded slot per keypoint, nmatches, nmatchesMap)"""
    mvp = np.array(match, np.int32)
    discarded = np.full(len(mvp), -1, np.int32)
    nmatchesMap = 0
    for i in range(len(mvp)):
        if mvp[i] >= 0:
            if outlier[i]:
                discarded[i] = mvp[i]               # pMP->mbTrackInView = false; pMP->mnLastFrameSeen = mnId
                mvp[i] = -1                         # mvpMapPoints[i] = NULL; mvbOutlier[i] = false
                nmatches -= 1
            elif last_obs[mvp[i]] > 0:
                nmatchesMap += 1
    return mvp, discarded, nmatches, nmatchesMap


def reference(sc, check_orientation=True, min_matches=MIN_MATCHES, th=TH, bmono=False, vo=True, bounded=False):
    """Every output of coeb_track_motion_model on scene sc, plus match_search (the last search's
    assignments before the discard), nmatches_first (the first search's return), retried and the
    last frame as the search saw it."""
    cam_o = cameras(bounded)[0]
    last = sc["last"]
    n, nl = len(sc["kps"]), len(last["has_mp"])
    created = cpos = None
    if vo:
        last, created, cpos = update_last_frame(last, sc["depth"], sc["last_desc"], sc["th_depth"], sc["Tcw_last"])
    if nl:
        nm, match = O.search_by_projection(cam_o, sc["kps"], sc["desc"], sc["ur"], last, sc["Tcw"], sc["Tcw_last"], th,
                                           bmono, check_orientation)
    else:
        nm, match = 0, np.full(n, -1, np.int32)
    first, retried = nm, False
    if nm < min_matches and nl:                     # :954-958
        nm, match = O.search_by_projection(cam_o, sc["kps"], sc["desc"], sc["ur"], last, sc["Tcw"], sc["Tcw_last"],
                                           2 * th, bmono, check_orientation)
        retried = True
    match = np.asarray(match, np.int32).copy()
    res = dict(match_search=match.copy(), nmatches_search=nm, nmatches_first=first, retried=retried, last=last,
               created=created, created_pos=cpos)
    if nm < min_matches or n == 0:                  # :960
        res.update(match=match, discarded=np.full(n, -1, np.int32), Tcw=sc["Tcw"].copy(), ninliers_pose=0, nmatches=nm,
                   nmatches_map=0, outlier=np.zeros(n, np.uint8))
        return res
    has = (match >= 0).astype(np.uint8)
    xw = last["xw"][np.maximum(match, 0)] if nl else np.zeros((n, 3), np.float32)
    nin, T, outl = O.pose_optimization(sc["kps"], has, xw, sc["ur"], sc["isg"], *INTR, sc["Tcw"])
    outl = np.where(has > 0, outl, 0).astype(np.uint8)
    mvp, disc, nmk, nmap = discard_loop(match, outl, last["mp_nobs"], nm)
    res.update(match=mvp, discarded=disc, Tcw=T, ninliers_pose=nin, nmatches=nmk, nmatches_map=nmap, outlier=outl)
    return res


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---- scenes ----
T_LAST = pose(0.02, -0.03, 0.015, (0.05, -0.04, 0.08))


def depth_case(name, n, rng, z):
    """The mvDepth of a last frame of n keypoints whose true depths are z: `holes` knocks out a
    fifth (0 / negative / NaN), the others are the directed sets of the visit rule."""
    d = np.array(z, np.float32)
    if name == "holes":
        r = rng.random(n)
        d[r < 0.07] = 0.0
        d[(r >= 0.07) & (r < 0.14)] = -1.0
        d[(r >= 0.14) & (r < 0.2)] = np.nan
    elif name == "all_far":                         # c = 0: the 101 closest, whatever their depth
        d += np.float32(TH_DEPTH)
    elif name == "all_close":                       # c = M: every keypoint
        d = (d * np.float32(0.3)).astype(np.float32)
    elif name == "ties":                            # equal depths decided by index, one exactly at th_depth
        d = np.round(d * 2) / 2
        d[: n // 3] = np.float32(TH_DEPTH)
    elif name == "none":
        d[:] = -1.0
    else:
        raise KeyError(name)
    return d.astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(n_cur, n_last, seed=3, shared=0.8, shift=0.004, octave0=False, displaced=0.1, mono=0.3, odd_angle=0.08,
          no_point=0.35, depth="holes", random_desc=False, dups=0):
    """n_last last-frame keypoints under T_LAST, each the image of a world point; the current
    frame sees `shared` of min(n_cur, n_last) of them from a pose a few centimetres on
    (descriptors with 0..6 bits flipped, the angle kept but for `odd_angle` of them), the rest of
    its keypoints are distractors.  `no_point` of the last-frame slots hold no MapPoint (only the
    visual-odometry step can give them one), the others hold one with Observations() in 0..3,
    `displaced` of them off by centimetres (the optimiser flags them) and a few marked mvbOutlier.
    The predicted pose is the true one turned by `shift` radians about y (2 px at 0.004; 0.043
    puts every projection about 22 px off: outside th at octave 0, inside 2*th).  random_desc:
    the current descriptors are unrelated (no search finds 20).  dups: the last `dups` of the n_last
    slots are copies of slots the current frame sees, whose own points nobody observes: both are
    assigned to the one keypoint, the search counts two and the keypoint holds the later one."""
    rng = np.random.default_rng(1000 * seed + 7 * n_cur + n_last)
    n_all, n_last = n_last, n_last - dups
    fx, fy, cx, cy, bf = INTR
    f32 = np.float32
    lk = np.zeros(n_last, cf.KEYPOINT_DTYPE)
    lk["x"], lk["y"] = rng.uniform(40, W - 40, n_last), rng.uniform(40, H - 40, n_last)
    lk["size"], lk["response"], lk["class_id"] = 31.0, 50.0, -1
    lk["octave"] = 0 if octave0 else rng.integers(0, 8, n_last)
    lk["angle"] = rng.uniform(0.0, 360.0, n_last)
    z = rng.uniform(0.8, 8.0, n_last).astype(f32)
    xw = unproject_stereo(lk, z, T_LAST)            # where UnprojectStereo puts them: a created point is consistent
    last_desc = rng.integers(0, 256, (n_last, 32)).astype(np.uint8)
    T_true = (pose(0.004, -0.006, 0.003, (0.02, -0.015, 0.03)).astype(np.float64) @ T_LAST.astype(np.float64)).astype(f32)
    m = int(round(shared * min(n_cur, n_last))) if min(n_cur, n_last) > 2 else min(n_cur, n_last)
    src = rng.permutation(n_last)[:m]
    u, v, zc = project(T_true, xw[src])
    u, v = u + rng.normal(0, 0.4, m), v + rng.normal(0, 0.4, m)
    nd = n_cur - m
    kps = np.zeros(n_cur, cf.KEYPOINT_DTYPE)
    kps["x"] = np.concatenate([u, rng.uniform(20, W - 20, nd)])
    kps["y"] = np.concatenate([v, rng.uniform(20, H - 20, nd)])
    kps["size"], kps["response"], kps["class_id"] = 31.0, 50.0, -1
    kps["octave"] = np.concatenate([lk["octave"][src], np.zeros(nd, np.int64) if octave0 else rng.integers(0, 8, nd)])
    turn = np.where(rng.random(m) < odd_angle, rng.uniform(60.0, 330.0, m), rng.normal(0, 2.0, m))
    kps["angle"] = np.concatenate([np.mod(lk["angle"][src].astype(np.float64) - turn, 360.0), rng.uniform(0, 360, nd)])
    zz = np.concatenate([zc, rng.uniform(0.8, 8.0, nd)])
    ur = (kps["x"].astype(np.float64) - bf / zz).astype(f32)
    ur[rng.random(n_cur) < mono] = -1.0
    desc = np.concatenate([last_desc[src], rng.integers(0, 256, (nd, 32)).astype(np.uint8)])
    for i in range(m):
        for b in rng.integers(0, 256, int(rng.integers(0, 7))):
            desc[i, b >> 3] ^= np.uint8(1 << (b & 7))
    if random_desc:
        desc = rng.integers(0, 256, (n_cur, 32)).astype(np.uint8)
    order = rng.permutation(n_cur)
    kps, ur, desc = kps[order], ur[order], desc[order]
    has = (rng.random(n_last) >= no_point).astype(np.uint8)
    nobs = rng.choice(np.array([0, 1, 2, 3], np.int32), n_last, p=[0.25, 0.25, 0.3, 0.2]).astype(np.int32)
    bad = (rng.random(n_last) < displaced) & (has > 0)
    xw_map = xw.copy()
    xw_map[bad] += rng.normal(0, 0.06, (int(bad.sum()), 3)).astype(f32)     # ~10 px: inside the window, past chi2
    # a MapPoint's descriptor is its own (GetDescriptor), not the keypoint's: a quarter differ by a few bits
    mp_desc = last_desc.copy()
    for i in np.flatnonzero(rng.random(n_last) < 0.25):
        for b in rng.integers(0, 256, 3):
            mp_desc[i, b >> 3] ^= np.uint8(1 << (b & 7))
    last = dict(has_mp=has, outlier=(rng.random(n_last) < 0.04).astype(np.uint8), xw=np.ascontiguousarray(xw_map),
                mp_desc=mp_desc, mp_nobs=nobs, keys_un=np.ascontiguousarray(lk))
    zdep = depth_case(depth, n_last, rng, z)
    if dups:
        o = src[:dups]
        last["has_mp"][o], last["mp_nobs"][o], last["outlier"][o], last["xw"][o] = 1, 0, 0, xw[o]
        last = {k: np.ascontiguousarray(np.concatenate([v, v[o]])) for k, v in last.items()}
        last["mp_nobs"][n_last:] = 2
        last_desc, zdep = np.concatenate([last_desc, last_desc[o]]), np.concatenate([zdep, zdep[o]])
    assert len(zdep) == n_all
    Tcw = (pose(0.0, shift, 0.0, (0.0, 0.0, 0.0)).astype(np.float64) @ T_true.astype(np.float64)).astype(f32)
    isg = np.array(list(extractor().p.inv_sigma2), f32)
    return dict(kps=np.ascontiguousarray(kps), desc=np.ascontiguousarray(desc), ur=np.ascontiguousarray(ur), last=last,
                last_desc=last_desc, depth=zdep, th_depth=TH_DEPTH, Tcw=np.ascontiguousarray(Tcw),
                Tcw_last=T_LAST.copy(), isg=isg, intr=INTR)


def sized(n_cur, n_last):
    return scene(n_cur, n_last)


def retry_scene():
    """The first search finds fewer than 20, the retry with 2*th at least 20."""
    return scene(300, 300, seed=5, shift=0.043, octave0=True)


def lost_scene():
    """Neither search finds 20: the call stops at the gate."""
    return scene(300, 300, seed=6, random_desc=True)


def dup_scene():
    """Twelve keypoints are assigned two last-frame points each: SearchByProjection's return counts
    24 for them, and nmatches ends above the number of keypoints that hold a point."""
    return scene(200, 212, seed=8, dups=12)


def few_scene():
    """Two keypoints showing the last frame's two points: fewer than 3 edges."""
    return scene(2, 2, seed=9, displaced=0.0, odd_angle=0.0, no_point=0.0, mono=0.0)


def directed_depth(n, c, seed=1, ties=False, special=False):
    """A depth set for the visit rule: n keypoints, c of them closer than TH_DEPTH and the rest
    farther, in random slots.  ties: depths on a quarter-metre lattice (equal depths, decided by
    index) with a few exactly TH_DEPTH, which count as close.  special: a few slots 0, negative,
    NaN and +inf (the first three are no entries; +inf is the farthest entry)."""
    rng = np.random.default_rng(77 * seed + 13 * n + c)
    d = np.concatenate([rng.uniform(0.5, 3.1, min(c, n)), rng.uniform(3.3, 9.0, max(n - c, 0))]).astype(np.float32)
    d = d[rng.permutation(n)] if n else d
    if ties:
        d = (np.round(d * 4) / 4).astype(np.float32)
        d[rng.random(n) < 0.05] = np.float32(TH_DEPTH)
    if special and n:
        k = rng.permutation(n)[: min(n, 8)]
        d[k] = np.resize(np.array([0.0, -2.0, np.nan, np.inf], np.float32), len(k))
    return d


# (keypoints with depth > 0, close ones): M = 0, 1, 99, 100, 101, 102, 300; c below, at and above 100
VISIT_CASES = ((0, 0), (1, 0), (1, 1), (99, 0), (99, 50), (99, 99), (100, 0), (100, 99), (100, 100), (101, 0), (101, 100),
               (101, 101), (102, 0), (102, 99), (102, 100), (102, 101), (102, 102), (300, 0), (300, 40), (300, 99), (300, 100),
               (300, 101), (300, 180), (300, 300))


def with_depth(sc, depth):
    """sc with another mvDepth.  A slot of depth +inf holds an observed point, so that nothing is
    unprojected from it (inf - inf: a NaN whose sign is the adder's choice)."""
    out = dict(sc)
    out["depth"] = np.ascontiguousarray(depth, np.float32)
    inf = np.isinf(out["depth"])
    if inf.any():
        last = {k: v.copy() for k, v in sc["last"].items()}
        last["has_mp"][inf] = 1
        last["mp_nobs"][inf] = 2
        out["last"] = last
    return out


def frames(sc):
    """(the current Frame at the predicted pose, the last Frame with its map_points) for Context.track_with_motion_model"""
    la = sc["last"]
    cur = cf.Frame(sc["kps"], sc["desc"], sc["ur"], Tcw=sc["Tcw"])
    lf = cf.Frame(la["keys_un"], sc["last_desc"], Tcw=sc["Tcw_last"], outlier=la["outlier"],
                  map_points=dict(world_pos=la["xw"], descriptor=la["mp_desc"], observations=la["mp_nobs"], valid=la["has_mp"]))
    return cur, lf
