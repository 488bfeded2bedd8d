"""Tracking::TrackLocalMap on one frame as the CPU oracle composes it (no GPU): Frame::isInFrustum
per valid local-map point (oc_is_in_frustum), ORBmatcher::SearchByProjection(F, vpLocalMapPoints,
th) (oracle.search_local_map), the merge of the search's points with the MapPoints the keypoints
entered with (as oracle.track_frame does), Optimizer::PoseOptimization and mnMatchesInliers
(Tracking.cc:996-1047, 1222-1272).  Plus the scene the single-frame TrackLocalMap tests share.

oracle.py does not wrap oc_is_in_frustum: its ctypes signature is declared here."""
import ctypes as C
import functools

import numpy as np

import chain_util as cu
import oracle as O
from coeb_front import synth

COS_LIMIT, TH, NNRATIO = 0.5, 3.0, 0.8
FIELDS = (("in_view", np.uint8), ("proj_x", np.float32), ("proj_y", np.float32), ("proj_xr", np.float32),
          ("level", np.int32), ("view_cos", np.float32))
POINT_FIELDS = ("valid", "world_pos", "normal", "max_distance", "min_distance", "descriptor", "observations")
# camera centres the points' normals look at: the current camera's neighbourhood (cos ~ 1, above
# RadiusByViewingCos's 0.998), then views further and further to the side, past cos_limit
CENTRES = np.array([[0.0, 0.0, 0.0], [0.9, 0.0, 0.0], [0.0, -2.6, 0.3], [4.5, 0.5, 0.5]], np.float32)


def _frustum_fn():
    f = O.lib().oc_is_in_frustum
    f.restype = C.c_int
    f.argtypes = [C.POINTER(O.Camera), C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float,
                  C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_int32),
                  C.POINTER(C.c_float)]
    return f


def frustum(cam_o, Tcw, pts, cos_limit=COS_LIMIT):
    """isInFrustum(pMP, cos_limit) over the valid points of pts (dict of POINT_FIELDS arrays):
    the FIELDS arrays (zeros where not in view) and "n_to_match"."""
    f = _frustum_fn()
    n = len(pts["valid"])
    out = {k: np.zeros(n, dt) for k, dt in FIELDS}
    T = np.ascontiguousarray(Tcw, np.float32)
    xw = np.ascontiguousarray(pts["world_pos"], np.float32).reshape(n, 3)
    nr = np.ascontiguousarray(pts["normal"], np.float32).reshape(n, 3)
    u, v, ur, vc, lvl = C.c_float(), C.c_float(), C.c_float(), C.c_float(), C.c_int32()
    for q in range(n):
        if not pts["valid"][q]:
            continue
        P, Pn = xw[q].copy(), nr[q].copy()
        if f(C.byref(cam_o), O.ptr(T), O.ptr(P), O.ptr(Pn), float(pts["max_distance"][q]), float(pts["min_distance"][q]),
             cos_limit, C.byref(u), C.byref(v), C.byref(ur), C.byref(lvl), C.byref(vc)):
            out["in_view"][q] = 1
            out["proj_x"][q], out["proj_y"][q], out["proj_xr"][q] = u.value, v.value, ur.value
            out["level"][q], out["view_cos"][q] = lvl.value, vc.value
    out["n_to_match"] = int(out["in_view"].sum())
    return out


def search(cam_o, sc, fields, cur_obs, th=TH, nnratio=NNRATIO):
    """SearchLocalPoints' matcher call: (nmatches, match); skipped when nothing is in view."""
    n = len(sc["kps"])
    if fields["n_to_match"] == 0:                   # Tracking.cc:1261
        return 0, np.full(n, -1, np.int32)
    mp = {k: fields[k] for k, _ in FIELDS}
    mp.update(descriptor=sc["pts"]["descriptor"], observations=sc["pts"]["observations"])
    cobs = np.full(n, -1, np.int32) if cur_obs is None else cur_obs
    if len(mp["in_view"]) == 0:
        return 0, np.full(n, -1, np.int32)
    return O.search_local_map(cam_o, sc["kps"], sc["desc"], sc["ur"], cobs, mp, th, nnratio)


def reference(sc, only_tracking=False, cos_limit=COS_LIMIT, th=TH, nnratio=NNRATIO, cur_obs="scene"):
    """Every output of coeb_track_local_map on scene sc, from the oracle."""
    cam_o = sc["cam_o"]
    n = len(sc["kps"])
    cur_obs = sc["cur_obs"] if isinstance(cur_obs, str) else cur_obs
    cobs = np.full(n, -1, np.int32) if cur_obs is None else np.asarray(cur_obs, np.int32)
    fields = frustum(cam_o, sc["Tcw"], sc["pts"], cos_limit)
    nl, lmatch = search(cam_o, sc, fields, cobs, th, nnratio)
    hit = lmatch >= 0
    has2 = (hit | (cobs >= 0)).astype(np.uint8)                                      # oracle.track_frame's merge
    pw = sc["pts"]["world_pos"].reshape(-1, 3)
    xw2 = np.where(hit[:, None], pw[np.maximum(lmatch, 0)] if len(pw) else 0, sc["cur_xw"]).astype(np.float32)
    obs2 = np.where(hit, sc["pts"]["observations"][np.maximum(lmatch, 0)] if len(pw) else 0, cobs).astype(np.int32)
    fx, fy, cx, cy, bf = sc["intr"]
    nin, T, outl = O.pose_optimization(sc["kps"], has2, xw2, sc["ur"], sc["isg"], fx, fy, cx, cy, bf, sc["Tcw"])
    outl = np.where(has2 > 0, outl, 0).astype(np.uint8)
    inl = (has2 > 0) & (outl == 0) & ((obs2 > 0) | bool(only_tracking))
    res = dict(fields)
    res.update(match=lmatch, nlocal=nl, has2=has2, obs2=obs2, xw2=xw2, Tcw=T, outlier=outl, ninliers_pose=nin,
               nmatches_inliers=int(inl.sum()))
    return res


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


# ---- the scene ----
def _dist(P, c):
    return np.sqrt(((P.astype(np.float64) - c.astype(np.float64)) ** 2).sum(1))


def make_points(xw, desc, octave, rng, n_distract, scale, invalid_frac=0.1, far_frac=0.06, near_frac=0.06):
    """vpLocalMapPoints: the map points xw plus n_distract random ones all around the camera.  Each
    normal points from one of CENTRES at the point and the distance range is UpdateNormalAndDepth's
    from that centre (as synth.make_keyframe_points: |x| * scale[octave], jittered 10 %), a
    fraction pushed out of the invariance range on each side."""
    n = len(xw)
    dx = rng.uniform(-3.0, 3.0, (n_distract, 3)).astype(np.float32)
    dx[:, 2] = rng.uniform(-1.5, 6.0, n_distract)
    P = np.concatenate([np.asarray(xw, np.float32).reshape(-1, 3), dx]).astype(np.float32)
    m = len(P)
    oct_all = np.concatenate([np.asarray(octave, np.int64), rng.integers(0, len(scale), n_distract)])
    k = rng.choice(len(CENTRES), m, p=[0.55, 0.2, 0.15, 0.1])
    d = P.astype(np.float64) - CENTRES[k].astype(np.float64)
    nd = np.sqrt((d ** 2).sum(1))
    normal = (d / nd[:, None]).astype(np.float32)
    dist0 = _dist(P, CENTRES[0])                     # about the current camera's distance
    maxd = (dist0 * scale[np.clip(oct_all, 0, len(scale) - 1)] * rng.uniform(0.9, 1.1, m)).astype(np.float32)
    r = rng.random(m)
    maxd[r < far_frac] *= np.float32(0.3)            # dist > 1.2 max
    maxd[r > 1 - near_frac] *= np.float32(9.0)       # dist < 0.8 min
    mind = (maxd / scale[-1]).astype(np.float32)
    order = rng.permutation(m)
    pts = dict(valid=(rng.random(m) >= invalid_frac).astype(np.uint8), world_pos=P, normal=normal, max_distance=maxd,
               min_distance=mind,
               descriptor=np.concatenate([np.asarray(desc, np.uint8).reshape(-1, 32),
                                          rng.integers(0, 256, (n_distract, 32)).astype(np.uint8)]),
               observations=rng.choice(np.array([0, 1, 2, 3], np.int32), m, p=[0.3, 0.2, 0.3, 0.2]).astype(np.int32))
    return {k_: np.ascontiguousarray(v[order]) for k_, v in pts.items()}


def camera_distance(Tcw, P):
    """dist of isInFrustum in the reference's float forms: |P - mOw|, mOw = -Rcw^T tcw."""
    T = np.asarray(Tcw, np.float32).astype(np.float64)
    Ow = (-(T[:3, :3].T @ T[:3, 3])).astype(np.float32)
    PO = (np.asarray(P, np.float32) - Ow).astype(np.float32)
    return np.sqrt((PO.astype(np.float64) ** 2).sum(-1)).astype(np.float32)


def unclamped_level(maxd, dist, log_sf):
    """MapPoint::PredictScale before its clamp (MapPoint.cc:410)."""
    ratio = (np.asarray(maxd, np.float32) / np.asarray(dist, np.float32)).astype(np.float32)
    return np.ceil(np.log(ratio.astype(np.float64)).astype(np.float32) / np.float32(log_sf)).astype(np.int64)


@functools.lru_cache(maxsize=None)
def extractor():
    return O.Extractor()


@functools.lru_cache(maxsize=None)
def scene(w=640, h=480, bounds=None, seed=11, n_distract=1000):
    """One extracted frame (frame 1 of a synthetic pair) against a local map made of frame 0's
    MapPoints and distractors.  Tcw: the pair's motion with a rotation added, so projections sit
    a few pixels off the keypoints.  Entry MapPoints on about half the keypoints (Observations()
    in {0, 1, 2}; a tenth of them displaced, for the optimiser to reject)."""
    ex = extractor()
    rng = np.random.default_rng(seed)
    intr = cu.TUM if (w, h) == (640, 480) else cu.intrinsics(w, h)
    if bounds is None:
        bounds = tuple(b * s for b, s in zip(cu.BOUNDS_INSIDE, (w / 640.0, w / 640.0, h / 480.0, h / 480.0)))
    cam_o, cam = cu.cameras(O, ex, w, h, intr, bounds)
    fr = synth.make_frames(w, h, 2, seed=1000 + seed)
    r0, r1 = ex.extract(fr[0]), ex.extract(fr[1])
    depth = synth.make_depth(w, h)
    last = O.mapframe_from_extraction(r0["kps"], r0["desc"], depth, *intr)
    ur, dep = O.stereo_from_rgbd(r1["kps"], depth, intr[4])
    scale = np.array(list(ex.p.scale)[:ex.nlevels], np.float32)
    has = last["has_mp"] > 0
    pts = make_points(last["xw"][has], last["mp_desc"][has], last["keys_un"]["octave"][has], rng, n_distract, scale)
    tm = (synth.SHIFT[0] * synth.DEPTH_Z / intr[0], synth.SHIFT[1] * synth.DEPTH_Z / intr[1], 0.0)
    Tcw = synth.rotated_pose(0.35, axis=1, t=(tm[0] + 0.004, tm[1] - 0.003, tm[2] + 0.006))
    # a few points at the far edge of the invariance range: dist <= 1.2f * max by the last float,
    # where PredictScale's ceil(log(ratio) / log(1.2f)) reaches -1
    edge = np.flatnonzero((pts["valid"] > 0) & (np.abs(pts["normal"][:, 2]) > 0.9))[:48]
    d = camera_distance(Tcw, pts["world_pos"][edge])
    mx = (d / np.float32(1.2)).astype(np.float32)
    for _ in range(4):
        low = d > np.float32(1.2) * mx
        mx = np.where(low, np.nextafter(mx, np.float32(np.inf)), mx).astype(np.float32)
    pts["max_distance"][edge] = mx
    pts["min_distance"][edge] = (mx / scale[-1]).astype(np.float32)
    n = len(r1["kps"])
    kp = r1["kps"]
    # entry MapPoints: the keypoint's own back-projection, in the world of frame 0
    z = np.where(dep > 0, dep, np.float32(synth.DEPTH_Z)).astype(np.float32)
    xc = np.stack([(kp["x"] - np.float32(intr[2])) * z / np.float32(intr[0]),
                   (kp["y"] - np.float32(intr[3])) * z / np.float32(intr[1]), z], axis=1).astype(np.float32)
    cur_xw = (xc - np.array(tm, np.float32)).astype(np.float32)
    held = rng.random(n) < 0.5
    cur_obs = np.where(held, rng.integers(0, 3, n), -1).astype(np.int32)
    bad = held & (rng.random(n) < 0.1)
    cur_xw[bad] += rng.normal(0, 0.25, (int(bad.sum()), 3)).astype(np.float32)
    isg = np.array(list(ex.p.inv_sigma2), np.float32)
    return dict(w=w, h=h, intr=intr, bounds=bounds, cam_o=cam_o, cam=cam, kps=np.ascontiguousarray(kp),
                desc=np.ascontiguousarray(r1["desc"]), ur=np.ascontiguousarray(ur, np.float32), Tcw=Tcw, pts=pts,
                cur_obs=cur_obs, cur_xw=np.ascontiguousarray(cur_xw), isg=isg, scale=scale,
                log_sf=float(np.float32(np.log(np.float64(np.float32(1.2))))))


def with_points(sc, pts):
    out = dict(sc)
    out["pts"] = pts
    return out


def first_points(sc, m):
    """sc with the first m local-map points only."""
    return with_points(sc, {k: np.ascontiguousarray(v[:m]) for k, v in sc["pts"].items()})


def first_keypoints(sc, n):
    out = dict(sc)
    for k in ("kps", "desc", "ur", "cur_obs", "cur_xw"):
        out[k] = np.ascontiguousarray(sc[k][:n])
    return out
