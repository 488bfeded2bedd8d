"""Helpers shared by the tests of the device-batch tracking chain (BASELINE configs[4]).

_chain_oracle runs the chain frame by frame on the CPU oracle, _check_chain compares a
BatchPipeline's results with it bit for bit.  The scenario_* functions build the inputs of
tests/test_gpu_batch_depth.py (per-frame depth with holes, degenerate neighbours, nobs = 0,
rotated predictions, raw 16U depth), and the coverage_* functions count, from the ORACLE's
results alone, the branches each scenario exists to reach; tests/test_oracle_kat.py asserts the
same floors without a GPU, so a change to synth or to the oracle that empties a scenario fails
there first.  The scenario builders take any frame size and the oracle chain any camera
(cameras(): scaled intrinsics, image bounds): tests/test_gpu_chain_shapes.py runs the chain at
ragged sizes and under the bounds of a distorted camera.
"""
import numpy as np

from coeb_front import synth

W, H, F = 640, 480, 8
SEED = 4242
KCAP = 1064                       # the batch's keypoint slots per frame at 640x480, 1000 features: the chain's stride
TUM = (synth.TUM_FX, synth.TUM_FY, synth.TUM_CX, synth.TUM_CY, synth.TUM_BF)


def intrinsics(w, h):
    """(fx, fy, cx, cy, bf) of a w x h camera: TUM's scaled by w / 640 and h / 480 (bf by w / 640),
    rounded to float32 once so the oracle and the device get the same bits."""
    sx, sy = w / 640.0, h / 480.0
    return tuple(float(np.float32(v)) for v in (synth.TUM_FX * sx, synth.TUM_FY * sy, synth.TUM_CX * sx,
                                                synth.TUM_CY * sy, synth.TUM_BF * sx))


def cameras(oracle_mod, ex, w, h, intr=None, bounds=None):
    """(oracle Camera, coeb_front.Camera) of a w x h image with intrinsics intr (default:
    intrinsics(w, h)) and image bounds (min_x, max_x, min_y, max_y) (default: ComputeImageBounds
    of an undistorted image, (0, w, 0, h)).  The oracle's grid inverses are the library's
    expression (coeb_capi.hip, Frame.cc:233-234) on the float32 bounds."""
    import coeb_front
    intr = intrinsics(w, h) if intr is None else intr
    cam_o = oracle_mod.camera(ex, w, h, *intr)
    if bounds is None:
        return cam_o, coeb_front.make_camera(*intr, w, h)
    b = [np.float32(v) for v in bounds]
    cam_o.min_x, cam_o.max_x, cam_o.min_y, cam_o.max_y = (float(v) for v in b)
    cam_o.grid_inv_w = float(np.float32(64) / (b[1] - b[0]))
    cam_o.grid_inv_h = float(np.float32(48) / (b[3] - b[2]))
    return cam_o, coeb_front.Camera(*intr, *(float(v) for v in b))


def _chain_oracle(oracle_mod, ex, frames, boxes, Tpred, stride, isg, nkf=2, depth=None, nobs=2, intr=TUM,
                  bounds=None):
    """The configs[4] loop frame by frame on the oracle: Frame ctor (T_M from the previous frame,
    blur flags, masked extraction) when boxes is given, else the plain extraction; then
    track_frame (motion model + TrackLocalMap).  depth: (F, H, W) float32, frame f's own map
    for its ComputeStereoFromRGBD and its LastFrame snapshot (default: the constant plane);
    nobs: Observations() of every MapPoint.  res[f] also carries what the checks and the
    coverage counts need: "ur" / "kp_depth" (mvuRight / mvDepth of frame f), "kf1" / "kf2" (the
    snapshots of frames f-1 / f-2 the local map was built from, kf2 None where there is none),
    "T_last" (the pose that places kf2 in kf1's frame).  With boxes, ext[f] also carries the
    Frame constructor's "tm" (T_M, None where findFundamentalMat gave an empty Mat) and "blur".
    intr / bounds: the camera (cameras())."""
    F, H, W = frames.shape
    fx, fy, cx, cy, bf = intr
    if depth is None:
        depth = np.broadcast_to(synth.make_depth(W, H), (F, H, W))
    cam_o = cameras(oracle_mod, ex, W, H, intr, bounds)[0]
    ext, res = [], [None]
    for f in range(F):
        if boxes is None:
            ext.append(ex.extract(frames[f]))
            continue
        if f == 0:
            tm0, bl = np.zeros((0, 2), np.float32), np.zeros(len(boxes[0]), np.int32)
        else:
            tm0 = oracle_mod.process_moving_object(frames[f - 1], frames[f])
            bl, _ = oracle_mod.blur_flags(frames[f], boxes[f])
        tm = np.zeros((0, 2), np.float32) if tm0 is None else tm0
        ext.append(ex.extract(frames[f], boxes[f], tm, bl))
        ext[f].update(tm=tm0, blur=bl)
    mfs = [oracle_mod.mapframe_from_extraction(e["kps"], e["desc"], depth[f], *intr, nobs=nobs)
           for f, e in enumerate(ext)]
    for f in range(1, F):
        ur, dep = oracle_mod.stereo_from_rgbd(ext[f]["kps"], depth[f], bf)
        prev2 = mfs[f - 2] if (nkf >= 2 and f >= 2) else None
        T_last = res[f - 1]["T1"] if f >= 2 else np.eye(4, dtype=np.float32)
        r = oracle_mod.track_frame(cam_o, isg, ext[f], ur, mfs[f - 1], prev2, Tpred[f], T_last, stride, nobs=nobs,
                                   fx=fx, fy=fy, cx=cx, cy=cy, bf=bf)
        r.update(ur=ur, kp_depth=dep, kf1=mfs[f - 1], kf2=prev2, T_last=T_last)
        res.append(r)
    return ext, res


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_chain(bp, ext, res, F):
    out, matches, nms = bp.results()
    T1, nin1, outl1 = bp.pose_results()
    tr = bp.track_results()
    states = []
    for f in range(1, F):
        r = res[f]
        n = len(ext[f]["kps"])
        assert np.array_equal(out[f][1], ext[f]["desc"]), f
        # k_prep: mvuRight / mvDepth of every keypoint from frame f's own depth map
        ur = bp.ctx.debug_read("u_right", f).view(np.float32)[:n]
        dep = bp.ctx.debug_read("kp_depth", f).view(np.float32)[:n]
        bad = np.nonzero(_bits(ur) != _bits(r["ur"]))[0]
        assert len(bad) == 0, ("u_right", f, len(bad), ur[bad[:4]], r["ur"][bad[:4]])
        bad = np.nonzero(_bits(dep) != _bits(r["kp_depth"]))[0]
        assert len(bad) == 0, ("kp_depth", f, len(bad), dep[bad[:4]], r["kp_depth"][bad[:4]])
        assert nms[f] == r["nmatches"] and np.array_equal(matches[f], r["match"]), f
        assert np.array_equal(T1[f].view(np.uint32), r["T1"].view(np.uint32)), f
        assert nin1[f] == r["nin1"], f
        if "outlier1" in r:                                     # the first optimisation ran
            m = r["match"] >= 0
            assert np.array_equal(outl1[f][m], r["outlier1"][m]), ("outlier1", f)
        assert tr["state"][f] == r["state"], (f, tr["state"][f], r["state"])
        states.append(r["state"])
        if r["nmatches"] >= 20:
            assert tr["nmatches_map"][f] == r["nmatches_map"], f
        if r["state"] == 0:
            assert tr["ninliers"][f] == 0 and np.array_equal(tr["T"][f].view(np.uint32), r["T1"].view(np.uint32)), f
            continue
        assert tr["nlocal"][f] == r["nlocal"], (f, tr["nlocal"][f], r["nlocal"])
        assert np.array_equal(tr["local_match"][f], r["local_match"]), f
        assert tr["ninliers"][f] == r["ninliers"], (f, tr["ninliers"][f], r["ninliers"])
        assert np.array_equal(tr["T"][f].view(np.uint32), r["T"].view(np.uint32)), f
        h2 = r["has2"] > 0
        assert np.array_equal(tr["outlier"][f][h2], r["outlier"][h2]), f
    return states, tr


# ------------------------------------------------------------------ scenarios (default 640x480, F = 8)
def _motion_pose(w, h):
    """synth.motion_pose() for the intrinsics of a w x h image (the same bits at 640x480)."""
    return synth.motion_pose(fx=synth.TUM_FX * (w / 640.0), fy=synth.TUM_FY * (h / 480.0))


def scenario_holes(w=W, h=H, F=F):
    """Per-frame depth surfaces with 30 % of the 16x16 tiles knocked out (0 / NaN / negative)."""
    return dict(frames=synth.make_frames(w, h, F, seed=SEED), boxes=None, depth=synth.depth_sequence(w, h, F),
                Tcw=np.stack([_motion_pose(w, h)] * F), nobs=2)


def scenario_degenerate(w=W, h=H, F=F):
    """The holes input with frame 3's depth all holes and frame 5 a constant image (0 keypoints)."""
    s = scenario_holes(w, h, F)
    s["depth"][3] = 0.0
    s["frames"][5] = 128
    return s


def scenario_nobs_zero(w=W, h=H, F=F):
    s = scenario_holes(w, h, F)
    s["nobs"] = 0
    return s


def scenario_perturbed(w=W, h=H, F=F):
    s = scenario_holes(w, h, F)
    s["Tcw"] = synth.perturbed_poses(F)
    return s


def scenario_grab_rgbd(w=W, h=H, F=F):
    """The whole GrabImageRGBD loop's input: RGB images, raw 16U depth with holes as 0, YOLO
    boxes.  "depth" is the float map the device's own conversion must produce."""
    frames, boxes = synth.tracking_sequence(w, h, F)
    rgb, _ = synth.rgbd_from_gray(frames)
    u16, depth = synth.raw_depth_u16(synth.depth_sequence(w, h, F))
    return dict(frames=frames, boxes=[boxes[f][None, :] for f in range(F)], depth=depth,
                Tcw=np.stack([_motion_pose(w, h)] * F), nobs=2, rgb=rgb, depth_u16=u16)


def scenario_frame_ctor(w=W, h=H, F=F, seed=3):
    """The RGB-D Frame constructor's input: synth.moving_object_sequence with two YOLO boxes per
    frame, the moving object's (cut at the image edge, as a detector reports it) and a static one
    on the first near panel; the constant depth plane."""
    frames, obj = synth.moving_object_sequence(w, h, F, seed=seed)
    edge = np.float32([w, h, w, h])
    boxes = [np.stack([np.minimum(obj[f], edge), np.float32([40, 40, 160, 140])]) for f in range(F)]
    return dict(frames=frames, boxes=boxes, depth=None, Tcw=np.stack([_motion_pose(w, h)] * F), nobs=2)


def run_oracle(oracle_mod, ex, s, stride, isg, nkf=2, intr=TUM, bounds=None):
    return _chain_oracle(oracle_mod, ex, s["frames"], s["boxes"], s["Tcw"], stride, isg, nkf=nkf, depth=s["depth"],
                         nobs=s["nobs"], intr=intr, bounds=bounds)


# ------------------------------------------------------------------ coverage, from oracle results only
def coverage_edges(r):
    """(monocular, stereo) edges of the first PoseOptimization of oracle frame result r:
    matched keypoints with mvuRight < 0 / >= 0 (Optimizer.cc:287)."""
    m = r["match"] >= 0
    return int((m & (r["ur"] < 0)).sum()), int((m & ~(r["ur"] < 0)).sum())


def coverage_lastframe_holes(r):
    """LastFrame keypoints without a MapPoint (depth <= 0 or NaN)."""
    return int((r["kf1"]["has_mp"] == 0).sum())


def coverage_frustum(r, stride):
    """Over the local map's existing slots of oracle frame result r (a keypoint of KeyFrame f-2
    or f-1 with a MapPoint, not matched by the motion model): (slots isInFrustum rejected,
    in-view points whose predicted level is not their source keypoint's octave)."""
    lm = r["local_map"]
    exists = np.zeros(2 * stride, bool)
    octave = np.zeros(2 * stride, np.int32)
    for base, kf in ((0, r["kf2"]), (stride, r["kf1"])):
        if kf is None:
            continue
        n = len(kf["has_mp"])
        exists[base:base + n] = kf["has_mp"] > 0
        octave[base:base + n] = kf["keys_un"]["octave"]
    exists[stride + r["match"][r["match"] >= 0]] = False          # mnLastFrameSeen (Tracking.cc:979, 1249)
    inv = lm["in_view"] > 0
    assert not (inv & ~exists).any()                                # a point in view comes from an existing slot
    return int((exists & ~inv).sum()), int((inv & (lm["level"] != octave)).sum())


def coverage_real_outliers(res):
    """Some frame whose second optimisation flags a held MapPoint as outlier."""
    return any(((r["outlier"] > 0) & (r["has2"] > 0)).any() for r in res[1:] if r["state"] > 0)


def scenario_lost_neighbours(w=W, h=H, F=F):
    """The holes input with frames 2, 4 and 6 lost on predictions that are wrong but not absurd.
    A lost frame's pose is what the motion model left (the prediction, or a PoseOptimization
    over a few dozen wrong matches that keeps under 10 inliers), and that pose places KeyFrame
    f-2 in the next frame's local map: the only way an existing, unseen slot leaves the frustum
    in this chain (a tracked frame's optimised pose follows the 2-px image motion, and keypoints
    keep 16 px from the border).  With the predictions as poses, frame 3 sees KeyFrame 1 tilted by 75 degrees about its centre (view
    angle), frame 5 sees KeyFrame 3 turned 20 degrees and pushed 0.8 m away (image bounds, beyond
    1.2 max distance), frame 7 sees KeyFrame 5 pulled 0.9 m nearer (inside 0.8 min distance)."""
    s = scenario_holes(w, h, F)
    tilt = synth.rotated_pose(75.0, axis=1, t=(0, 0, 0))
    c = np.array([0, 0, synth.DEPTH_Z], np.float32)
    tilt[:3, 3] = c - tilt[:3, :3] @ c
    s["Tcw"][2] = tilt
    s["Tcw"][4] = synth.rotated_pose(20.0, axis=1, t=(0, 0, 0.8))
    s["Tcw"][6] = synth.rotated_pose(10.0, axis=0, t=(0, 0, -0.9))
    return s


LOST_STATES = [2, 0, 2, 0, 2, 0, 2]


def coverage_rejections(r, stride):
    """Which test of Frame::isInFrustum (Frame.cc:445-501) turned away each existing, unseen
    local-map slot the oracle left out of view in frame result r, recomputed in float64 from the
    oracle's own inputs in the reference's order: behind the camera, image bounds, beyond
    1.2 max / inside 0.8 min distance, view cosine < 0.5."""
    n = dict(behind=0, bounds=0, far=0, near=0, view=0)
    lm = r["local_map"]
    T = r["T1"].astype(np.float64)
    Oc = -T[:3, :3].T @ T[:3, 3]
    sc = 1.2 ** np.arange(8)
    fx, fy, cx, cy, _ = TUM
    for base, kf, Tl in ((0, r["kf2"], r["T_last"].astype(np.float64)), (stride, r["kf1"], np.eye(4))):
        if kf is None:
            continue
        cnt = len(kf["has_mp"])
        exists = kf["has_mp"] > 0
        if base:
            exists[r["match"][r["match"] >= 0]] = False
        rej = exists & (lm["in_view"][base:base + cnt] == 0)
        P = kf["xw"][rej].astype(np.float64) @ Tl[:3, :3].T + Tl[:3, 3]
        d = P - Tl[:3, 3]
        nd = np.linalg.norm(d, axis=1)
        maxd = nd * sc[kf["keys_un"]["octave"][rej]]
        mind = maxd / sc[7]
        Pc = P @ T[:3, :3].T + T[:3, 3]
        z = np.where(Pc[:, 2] > 0, Pc[:, 2], 1.0)
        u, v = fx * Pc[:, 0] / z + cx, fy * Pc[:, 1] / z + cy
        dist = np.linalg.norm(P - Oc, axis=1)
        cos = ((P - Oc) * d).sum(1) / (dist * nd)
        left = np.ones(len(P), bool)
        for name, hit in (("behind", Pc[:, 2] < 0), ("bounds", (u < 0) | (u > W) | (v < 0) | (v > H)),
                          ("far", dist > 1.2 * maxd), ("near", dist < 0.8 * mind), ("view", cos < 0.5)):
            n[name] += int((left & hit).sum())
            left &= ~hit
    return n


def assert_coverage_lost_neighbours(res, stride):
    assert [r["state"] for r in res[1:]] == LOST_STATES
    n = dict(behind=0, bounds=0, far=0, near=0, view=0)
    for f in (3, 5, 7):
        assert coverage_frustum(res[f], stride)[0] >= 20, f
        assert res[f]["local_map"]["in_view"][:stride].sum() >= 20, f    # and KeyFrame f-2 still contributes
        for k, v in coverage_rejections(res[f], stride).items():
            n[k] += v
    assert min(n["bounds"], n["far"], n["near"], n["view"]) >= 20, n


DEGENERATE_STATES = [2, 2, 2, 0, 0, 0, 2]


def assert_coverage_holes(res):
    for f in range(1, len(res)):
        mono, stereo = coverage_edges(res[f])
        assert mono >= 50 and stereo >= 50, (f, mono, stereo)
        assert coverage_lastframe_holes(res[f]) >= 100, f
        assert res[f]["state"] == 2, (f, res[f]["state"])


def assert_coverage_degenerate(ext, res):
    assert [r["state"] for r in res[1:]] == DEGENERATE_STATES
    mono, stereo = coverage_edges(res[3])
    assert mono >= 50 and stereo == 0, (mono, stereo)              # optimised on monocular edges alone
    assert res[4]["nmatches"] == 0 and not res[4]["kf1"]["has_mp"].any()
    assert len(ext[5]["kps"]) == 0 and res[5]["nmatches"] == 0
    assert len(res[6]["kf1"]["has_mp"]) == 0 and len(ext[6]["kps"]) > 0
    assert len(res[7]["kf2"]["has_mp"]) == 0 and res[7]["nlocal"] > 0
    for f in (4, 5, 6):                                             # lost: the pose stays the prediction
        assert res[f]["nin1"] == 0 and "outlier1" not in res[f]


def assert_coverage_nobs_zero(res, Tcw):
    for f in range(1, F):
        r = res[f]
        assert r["nmatches"] >= 20 and r["nin1"] > 0, (f, r["nmatches"], r["nin1"])
        assert r["nmatches_map"] == 0 and r["state"] == 0 and r["nlocal"] == 0, f
        assert np.array_equal(_bits(r["T"]), _bits(r["T1"])), f
        assert not np.array_equal(_bits(r["T1"]), _bits(Tcw[f])), f  # the first optimisation did run


def assert_coverage_perturbed(res, stride):
    assert [r["state"] for r in res[1:]] == [2] * (F - 1)
    # No floor on rejected slots here: with every frame tracked the optimised poses follow the
    # 2-px image motion whatever the prediction was, and no existing, unseen slot can leave the
    # frustum (the oracle rejects 0).  scenario_lost_neighbours carries that floor.
    for f in range(2, F):
        _, releveled = coverage_frustum(res[f], stride)
        assert releveled >= 20, (f, releveled)


def assert_coverage_grab(res):
    states = [r["state"] for r in res[1:]]
    assert states.count(2) >= F - 2, states
    assert coverage_real_outliers(res)
    for f in range(1, F):
        if res[f]["state"] == 2:
            mono, _ = coverage_edges(res[f])
            assert mono >= 50, (f, mono)


# ------------------------------------------------------------------ other frame sizes, other image bounds
# tests/test_gpu_chain_shapes.py: the chain with per-frame offsets that are no multiple of 4
# (427 * 321 = 3 mod 4: frame bases on all four byte alignments; 333 * 251 odd, pitch 333) and
# with the image bounds a distorted camera gives (inside the image: keypoints fall off the grid;
# outside: the grid is coarser than the image).
SHAPES_F = 6
RAGGED_SIZES = ((427, 321), (333, 251))
BOUNDS_INSIDE = (37.5, 598.25, 29.75, 455.5)
BOUNDS_OUTSIDE = (-14.6, 655.3, -11.2, 492.7)
BOUNDED = ((640, 480, BOUNDS_INSIDE, True), (640, 480, BOUNDS_OUTSIDE, False),
           (427, 321, (25.5, 399.25, 19.75, 300.5), True))       # (w, h, bounds, bounds inside the image)


def coverage_off_grid(cam_o, kps):
    """Keypoints for which Frame::PosInGrid fails (Frame.cc:553-568), in the oracle's float32
    expression (orb_oracle.c, oc_grid_build): roundf((x - min) * grid_inv) outside the grid."""
    f32 = np.float32

    def cell(v, lo, inv):
        g = ((v.astype(f32) - f32(lo)) * f32(inv)).astype(np.float64)          # float32 product, held exactly
        return np.copysign(np.floor(np.abs(g) + 0.5), g)                       # roundf: halves away from zero
    px = cell(kps["x"], cam_o.min_x, cam_o.grid_inv_w)
    py = cell(kps["y"], cam_o.min_y, cam_o.grid_inv_h)
    return int(((px < 0) | (px >= 64) | (py < 0) | (py >= 48)).sum())


def assert_coverage_ragged(res):
    """Every frame tracked on a full motion-model match and with local-map matches of its own."""
    for f in range(1, len(res)):
        r = res[f]
        assert r["state"] == 2 and r["nmatches"] >= 300 and r["nlocal"] >= 5, (f, r["state"], r["nmatches"], r["nlocal"])


def assert_coverage_frame_ctor(ext, boxes):
    """At least 3 pairs with a non-empty T_M, and T_M points inside some box (the mask path
    removes keypoints)."""
    tms = [e["tm"] for e in ext[1:]]
    assert sum(t is not None and len(t) > 0 for t in tms) >= 3, [None if t is None else len(t) for t in tms]
    inside = 0
    for f in range(1, len(ext)):
        t = ext[f]["tm"]
        if t is None:
            continue
        x, y = t[:, 0].astype(np.int32), t[:, 1].astype(np.int32)
        for b in boxes[f]:
            inside += int(((x >= int(b[0])) & (x < int(b[2])) & (y >= int(b[1])) & (y < int(b[3]))).sum())
    assert inside > 0


def assert_coverage_bounds(cam_o, ext, res, res_default, inside):
    """The bounds change the oracle's matches in some frame (a device that ignored them fails),
    and bounds inside the image leave >= 10 keypoints of some frame off the grid."""
    assert any(res[f]["nmatches"] != res_default[f]["nmatches"] for f in range(1, len(res))), \
        [r["nmatches"] for r in res[1:]]
    if inside:
        off = [coverage_off_grid(cam_o, e["kps"]) for e in ext]
        assert max(off) >= 10, off


def matcher_pair(oracle_mod, ex):
    """The single-frame matchers' scene: frame 1's extraction and mvuRight, frame 0 as LastFrame."""
    fr = synth.make_frames(640, 480, 2, seed=77)
    r0, r1 = ex.extract(fr[0]), ex.extract(fr[1])
    depth = synth.make_depth(640, 480)
    last = oracle_mod.mapframe_from_extraction(r0["kps"], r0["desc"], depth, *TUM)
    ur1, _ = oracle_mod.stereo_from_rgbd(r1["kps"], depth, synth.TUM_BF)
    return r1, ur1, last


def matcher_scene(last, seed=0):
    """(local map, KeyFrame points) over matcher_pair's LastFrame, as tests/test_gpu_parity.py
    builds them for test_localmap_matches_oracle / test_keyframe_matches_oracle."""
    mp = synth.make_local_map(last["xw"], last["mp_desc"], last["keys_un"]["octave"], synth.motion_pose(), 640, 480,
                              seed=seed)
    kf = synth.make_keyframe_points(last["xw"], last["mp_desc"], last["keys_un"]["octave"], last["keys_un"]["angle"],
                                    seed=seed)
    kf["valid"][:len(last["has_mp"])] &= last["has_mp"]
    return mp, kf


def oracle_matchers(oracle_mod, cam_o, r1, ur1, last, mp, kf):
    """(nmatches, match) of the three single-frame matchers on the oracle with camera cam_o."""
    Tc, I4 = synth.motion_pose(), np.eye(4, dtype=np.float32)
    n = len(r1["kps"])
    return (oracle_mod.search_by_projection(cam_o, r1["kps"], r1["desc"], ur1, last, Tc, I4, 15.0),
            oracle_mod.search_local_map(cam_o, r1["kps"], r1["desc"], ur1, np.full(n, -1, np.int32), mp, 3.0, 0.8),
            oracle_mod.search_keyframe(cam_o, r1["kps"], r1["desc"], np.zeros(n, np.uint8), kf, Tc, 10.0, 100, True))


def assert_coverage_matchers(bounded, default):
    """Each matcher's oracle result under the bounded camera differs from the default camera's."""
    for name, (nb, mb), (nd, md) in zip(("lastframe", "localmap", "keyframe"), bounded, default):
        assert nb > 20 and not np.array_equal(mb, md), (name, nb, nd)
