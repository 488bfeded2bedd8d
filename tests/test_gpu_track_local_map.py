"""coeb_search_local_points / coeb_track_local_map (MI355X only): Frame::isInFrustum, the local-map
projection search, PoseOptimization and mnMatchesInliers in one call, every output bit for bit
against the CPU composition of tests/tlm_ref.py, at the scene's sizes, around k_frustum's wave
(64) and workgroup (256) edges, with empty inputs, against the three-step sequence the fused call
replaces, and at the argument checks."""
import ctypes as C
import functools

import numpy as np
import pytest

import coeb_front as cf
import oracle as O
import tlm_ref as R

pytestmark = pytest.mark.gpu

COEB_OK, COEB_EINVAL, COEB_ERANGE = 0, -22, -34          # include/coeb_front.h
SMALL = (333, 251, 400)
SCENES = ((640, 480, 1000), SMALL)


def scene(w, h, nd):
    return R.scene(w, h, n_distract=nd)


@functools.lru_cache(maxsize=None)
def scene_ref(w, h, nd, only_tracking):
    return R.reference(scene(w, h, nd), only_tracking)


def frame(sc):
    return cf.Frame(sc["kps"], sc["desc"], sc["ur"], Tcw=sc["Tcw"])


def points(sc):
    return cf.LocalPoints(*[sc["pts"][k] for k in R.POINT_FIELDS])


def track(ctx, sc, only_tracking=False, cur_obs="scene", cos_limit=R.COS_LIMIT):
    cobs = sc["cur_obs"] if isinstance(cur_obs, str) else cur_obs
    return cf.track_local_map(ctx, sc["cam"], frame(sc), cobs, sc["cur_xw"], points(sc), cos_limit, R.TH, R.NNRATIO,
                              only_tracking)


def assert_search(got, want, tag=""):
    for k, _ in R.FIELDS:
        assert np.array_equal(R.bits(got[k]), R.bits(want[k])), (tag, k)
    assert got["n_to_match"] == want["n_to_match"], (tag, got["n_to_match"], want["n_to_match"])
    assert np.array_equal(got["match"], want["match"]), tag


def assert_track(got, want, tag=""):
    assert_search(got, want, tag)
    assert got["nlocal"] == want["nlocal"], (tag, got["nlocal"], want["nlocal"])
    assert np.array_equal(R.bits(got["Tcw"]), R.bits(want["Tcw"])), (tag, got["Tcw"], want["Tcw"])
    assert np.array_equal(got["outlier"], want["outlier"]), tag
    assert (got["ninliers_pose"], got["nmatches_inliers"]) == (want["ninliers_pose"], want["nmatches_inliers"]), tag


@pytest.mark.parametrize("only_tracking", [False, True])
@pytest.mark.parametrize("w,h,nd", SCENES)
def test_track_local_map_matches_reference(ctx, w, h, nd, only_tracking):
    sc, want = scene(w, h, nd), scene_ref(w, h, nd, only_tracking)
    assert want["n_to_match"] >= 200 and want["nlocal"] >= 100 and want["outlier"].any()
    assert_track(track(ctx, sc, only_tracking), want)
    path = np.zeros(2, np.int32)
    ctx.check(cf.lib().coeb_debug_read(ctx.h, b"search_path", 0, path.ctypes.data, 8, None))
    assert path[0] == 0, path                              # the parallel claims converged


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 257])
def test_local_map_sizes(ctx, m):
    sc = scene(*SMALL)
    pts = {k: v[:m].copy() for k, v in sc["pts"].items()}
    pts["valid"][:] = 1
    if m > 1:
        pts["valid"][m // 2] = 0                            # one invalid point inside
    sub = R.with_points(sc, pts)
    want = R.reference(sub)
    if m >= 63:
        assert want["n_to_match"] >= 10 and want["nlocal"] >= 3
    assert_track(track(ctx, sub), want, m)


def test_last_point_of_a_wave_and_of_a_workgroup_in_view(ctx):
    """Points 63, 64, 255 and 256 are the only valid ones and all in view: nToMatch counts across
    k_frustum's wave and workgroup edges."""
    sc = scene(*SMALL)
    iv = np.flatnonzero(scene_ref(*SMALL, False)["in_view"])[:4]
    pts = {k: v[:257].copy() for k, v in sc["pts"].items()}
    pts["valid"][:] = 0
    for q, src in zip((63, 64, 255, 256), iv):
        for k in pts:
            pts[k][q] = sc["pts"][k][src]
    sub = R.with_points(sc, pts)
    want = R.reference(sub)
    assert want["n_to_match"] == 4 and list(np.flatnonzero(want["in_view"])) == [63, 64, 255, 256]
    assert_track(track(ctx, sub), want)


def test_no_keypoints(ctx):
    sub = R.first_keypoints(scene(*SMALL), 0)
    want = R.reference(sub)
    assert want["n_to_match"] >= 200 and want["nlocal"] == 0 and want["ninliers_pose"] == 0
    got = track(ctx, sub)
    assert_track(got, want)
    assert np.array_equal(R.bits(got["Tcw"]), R.bits(sub["Tcw"]))


@pytest.mark.parametrize("how", ["all_invalid", "cos_limit"])
def test_nothing_in_view_still_optimises_the_entry_points(ctx, how):
    sc = scene(*SMALL)
    cos = R.COS_LIMIT
    if how == "all_invalid":
        pts = dict(sc["pts"])
        pts["valid"] = np.zeros_like(pts["valid"])
        sc = R.with_points(sc, pts)
    else:
        cos = 1.5                                           # no cosine reaches it
    want = R.reference(sc, cos_limit=cos)
    assert want["n_to_match"] == 0 and want["nlocal"] == 0 and want["ninliers_pose"] >= 30
    assert not np.array_equal(want["Tcw"], sc["Tcw"])
    assert_track(track(ctx, sc, cos_limit=cos), want, how)


def test_fewer_than_three_edges_leave_the_pose(ctx):
    """No entry MapPoints and two matched local-map points with Observations() == 0: the optimiser
    returns 0 with the pose untouched, and nothing counts as a tracked inlier."""
    sc = scene(*SMALL)
    full = R.reference(sc, cur_obs=None)
    take = np.unique(full["match"][full["match"] >= 0])[:2]
    pts = {k: v[take].copy() for k, v in sc["pts"].items()}
    pts["observations"][:] = 0
    sub = R.with_points(sc, pts)
    want = R.reference(sub, cur_obs=None)
    assert 1 <= want["nlocal"] < 3 and want["has2"].sum() == want["nlocal"]
    assert want["ninliers_pose"] == 0 and want["nmatches_inliers"] == 0 and not want["outlier"].any()
    assert np.array_equal(R.bits(want["Tcw"]), R.bits(sc["Tcw"]))
    assert_track(track(ctx, sub, cur_obs=None), want)
    assert R.reference(sub, True, cur_obs=None)["nmatches_inliers"] == want["nlocal"]
    assert track(ctx, sub, True, cur_obs=None)["nmatches_inliers"] == want["nlocal"]


@pytest.mark.parametrize("w,h,nd", SCENES)
def test_null_cur_observations(ctx, w, h, nd):
    sc = scene(w, h, nd)
    want = R.reference(sc, cur_obs=None)
    assert want["nlocal"] > scene_ref(w, h, nd, False)["nlocal"]       # held keypoints are free now
    assert_track(track(ctx, sc, cur_obs=None), want)


@pytest.mark.parametrize("w,h,nd", SCENES)
def test_search_local_points_is_the_first_half(ctx, w, h, nd):
    sc, want = scene(w, h, nd), scene_ref(w, h, nd, False)
    got = cf.search_local_points(ctx, sc["cam"], frame(sc), sc["cur_obs"], points(sc), R.COS_LIMIT, R.TH, R.NNRATIO)
    assert_search(got, want)
    assert got["nmatches"] == want["nlocal"]
    bare = cf.search_local_points(ctx, sc["cam"], frame(sc), sc["cur_obs"], points(sc), R.COS_LIMIT, R.TH, R.NNRATIO,
                                  track_fields=False)
    assert np.array_equal(bare["match"], want["match"]) and bare["n_to_match"] == want["n_to_match"]


@pytest.mark.parametrize("w,h,nd", SCENES)
def test_equals_the_three_step_sequence(ctx, w, h, nd):
    """Host isInFrustum (the oracle's), coeb_match_localmap and coeb_pose_optimization on the same
    inputs give what the one call gives."""
    sc = scene(w, h, nd)
    fields = R.frustum(sc["cam_o"], sc["Tcw"], sc["pts"])
    F = frame(sc)
    n = F.N
    F.mvpMapPointObs = sc["cur_obs"].copy()
    F.mvpMapPoints = np.where(sc["cur_obs"] >= 0, 1000000 + np.arange(n), -1).astype(np.int32)
    lm = cf.LocalMap(*[fields[k] for k, _ in R.FIELDS], sc["pts"]["descriptor"], sc["pts"]["observations"])
    nlocal = cf.ORBmatcher(R.NNRATIO, ctx=ctx).SearchByProjection(F, lm, R.TH, camera=sc["cam"])
    hit = (F.mvpMapPoints >= 0) & (F.mvpMapPoints < 1000000)
    F.mvMapPointPos = np.where(hit[:, None], sc["pts"]["world_pos"][np.where(hit, F.mvpMapPoints, 0)],
                               sc["cur_xw"]).astype(np.float32)
    nin = cf.Optimizer.PoseOptimization(F, sc["cam"], ctx)
    got = track(ctx, sc)
    assert got["nlocal"] == nlocal and got["ninliers_pose"] == nin
    assert np.array_equal(np.where(hit, F.mvpMapPoints, -1), got["match"])
    assert np.array_equal(R.bits(got["Tcw"]), R.bits(F.mTcw))
    held = F.mvpMapPoints >= 0
    assert np.array_equal(got["outlier"][held], np.asarray(F.mvbOutlier)[held]) and not got["outlier"][~held].any()
    for k, _ in R.FIELDS:
        assert np.array_equal(R.bits(got[k]), R.bits(fields[k])), k


# ---- argument checks ----
SENT = 0x5A


def raw_track(ctx, sc, pts, search_only=False, drop=None):
    """The C entry point with sentinel-filled outputs: (rc, every output array / scalar)."""
    n, nq = len(sc["kps"]), len(pts["valid"])
    arrs = {k: np.ascontiguousarray(pts[k]) for k in R.POINT_FIELDS}
    ptr = {k: (None if k == drop else C.c_void_p(a.ctypes.data)) for k, a in arrs.items()}
    lp = cf.LocalPointsC(nq, *[ptr[k] for k in R.POINT_FIELDS])
    cur = cf.CurFrameC(n, C.c_void_p(sc["kps"].ctypes.data), C.c_void_p(sc["desc"].ctypes.data),
                       C.c_void_p(sc["ur"].ctypes.data))
    out = {k: np.full(max(nq, 1), SENT, dt) for k, dt in R.FIELDS}
    tf = cf.TrackFieldsC(*[C.c_void_p(out[k].ctypes.data) for k, _ in R.FIELDS])
    out.update(match=np.full(max(n, 1), SENT, np.int32), outlier=np.full(max(n, 1), SENT, np.uint8),
               T=sc["Tcw"].copy())
    cnt = [C.c_int(SENT) for _ in range(4)]
    L = cf.lib()
    if search_only:
        rc = L.coeb_search_local_points(ctx.h, C.byref(sc["cam"]), C.byref(cur), sc["cur_obs"].ctypes.data,
                                        out["T"].ctypes.data, C.byref(lp), R.COS_LIMIT, R.TH, R.NNRATIO, C.byref(tf),
                                        out["match"].ctypes.data, C.byref(cnt[0]), C.byref(cnt[1]))
    else:
        rc = L.coeb_track_local_map(ctx.h, C.byref(sc["cam"]), C.byref(cur), sc["cur_obs"].ctypes.data,
                                    sc["cur_xw"].ctypes.data, out["T"].ctypes.data, C.byref(lp), R.COS_LIMIT, R.TH,
                                    R.NNRATIO, 0, C.byref(tf), out["match"].ctypes.data, out["outlier"].ctypes.data,
                                    *[C.byref(c) for c in cnt])
    out["counts"] = [c.value for c in cnt]
    return rc, out


def untouched(sc, out):
    ok = all((out[k] == np.array(SENT, dt)).all() for k, dt in R.FIELDS)
    return (ok and (out["match"] == SENT).all() and (out["outlier"] == SENT).all() and out["counts"] == [SENT] * 4
            and np.array_equal(R.bits(out["T"]), R.bits(sc["Tcw"])))


BAD_POINTS = (("world_pos", np.nan), ("world_pos", np.inf), ("normal", np.nan), ("normal", -np.inf),
              ("min_distance", 0.0), ("min_distance", -1.0), ("min_distance", np.nan), ("max_distance", np.inf),
              ("max_distance", np.nan), ("max_distance", "below_min"))


@pytest.mark.parametrize("search_only", [False, True])
def test_invalid_arguments_write_nothing(ctx, search_only):
    sc = R.first_points(scene(*SMALL), 300)
    q = int(np.flatnonzero(sc["pts"]["valid"])[7])
    for field, value in BAD_POINTS:
        pts = {k: v.copy() for k, v in sc["pts"].items()}
        v = pts["min_distance"][q] * np.float32(0.5) if isinstance(value, str) else value
        if pts[field].ndim == 2:
            pts[field][q, 1] = v
        else:
            pts[field][q] = v
        rc, out = raw_track(ctx, sc, pts, search_only)
        assert rc == COEB_EINVAL and untouched(sc, out), (field, value, rc)
        pts["valid"][q] = 0                                 # the same values on an invalid point are never read
        rc, out = raw_track(ctx, sc, pts, search_only)
        assert rc == COEB_OK, (field, value, rc)
    for drop in R.POINT_FIELDS:
        rc, out = raw_track(ctx, sc, sc["pts"], search_only, drop=drop)
        assert rc == COEB_EINVAL and untouched(sc, out), drop
    # the context still works, and gives the reference's answer
    assert_track(track(ctx, sc), R.reference(sc))


def test_local_map_past_the_lds_budget(ctx):
    """8 keypoints and 20000 points need more on-chip memory than a workgroup has:
    coeb_match_localmap refuses with COEB_ERANGE, and so do the fused calls, with nothing written."""
    sc = R.first_keypoints(scene(*SMALL), 8)
    nq = 20000
    z = np.zeros(nq, np.float32)
    none, zi, zd = np.zeros(nq, np.uint8), np.zeros(nq, np.int32), np.zeros((nq, 32), np.uint8)
    lm = cf.LocalMapC(nq, *[C.c_void_p(a.ctypes.data) for a in (none, z, z, z, zi, z, zd, zi)])
    cur = cf.CurFrameC(8, C.c_void_p(sc["kps"].ctypes.data), C.c_void_p(sc["desc"].ctypes.data),
                       C.c_void_p(sc["ur"].ctypes.data))
    m, nm = np.zeros(8, np.int32), C.c_int()
    rc = cf.lib().coeb_match_localmap(ctx.h, C.byref(sc["cam"]), C.byref(cur), None, C.byref(lm), R.TH, R.NNRATIO,
                                      m.ctypes.data, C.byref(nm))
    assert rc == COEB_ERANGE
    pts = dict(valid=np.zeros(nq, np.uint8), world_pos=np.zeros((nq, 3), np.float32), normal=np.zeros((nq, 3), np.float32),
               max_distance=z, min_distance=z, descriptor=np.zeros((nq, 32), np.uint8), observations=np.zeros(nq, np.int32))
    for search_only in (False, True):
        rc, out = raw_track(ctx, sc, pts, search_only)
        assert rc == COEB_ERANGE and untouched(sc, out), (search_only, rc)
    assert b"LDS budget" in cf.lib().coeb_last_error(ctx.h)
    assert_track(track(ctx, sc), R.reference(sc))
