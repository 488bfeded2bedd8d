"""coeb_track_motion_model (MI355X only): UpdateLastFrame's visual-odometry points, SearchByProjection
with the 2*th retry, the nmatches gate, PoseOptimization and the outlier discard of
Tracking::TrackWithMotionModel in one call, every output bit for bit against the CPU composition of
tests/twmm_ref.py: at sizes around the kernels' wave (64) and workgroup (256) edges, empty, 1000 x
1000 and the largest pair the matcher takes; with both orientation settings, bMono, a bounded
camera; at the three retry cases, both sides of the gate and with fewer than three edges; on the
directed depth sets of the visit rule; against the existing calls composed; at the argument checks;
with the context's buffers reused; and the launch chain."""
import ctypes as C
import functools

import numpy as np
import pytest

import coeb_front as cf
import twmm_ref as R

pytestmark = pytest.mark.gpu

COEB_OK, COEB_EINVAL, COEB_ERANGE = 0, -22, -34     # include/coeb_front.h
COUNTS = ("nmatches_search", "ninliers_pose", "nmatches", "nmatches_map")


@functools.lru_cache(maxsize=None)
def sized_ref(n_cur, n_last, check_ori=True, min_matches=R.MIN_MATCHES, bmono=False, vo=True, bounded=False):
    return R.reference(R.sized(n_cur, n_last), check_ori, min_matches, bmono=bmono, vo=vo, bounded=bounded)


def run(c, sc, check_ori=True, min_matches=R.MIN_MATCHES, bmono=False, vo=True, bounded=False, th=R.TH):
    cur, lf = R.frames(sc)
    return c.track_with_motion_model(R.cameras(bounded)[1], cur, lf, th, bmono, check_ori, min_matches,
                                     depth=sc["depth"] if vo else None, th_depth=sc["th_depth"] if vo else None)


def assert_same(got, want, tag=""):
    for k in ("match", "discarded", "outlier"):
        assert np.array_equal(got[k], want[k]), (tag, k, got[k], want[k])
    assert [got[k] for k in COUNTS] == [want[k] for k in COUNTS], (tag, [got[k] for k in COUNTS], [want[k] for k in COUNTS])
    assert np.array_equal(R.bits(got["Tcw"]), R.bits(want["Tcw"])), (tag, got["Tcw"], want["Tcw"])
    if want["created"] is None:
        assert got["created"] is None and got["created_pos"] is None, tag
    else:
        assert np.array_equal(got["created"], want["created"]), (tag, np.flatnonzero(got["created"] != want["created"]))
        assert np.array_equal(R.bits(got["created_pos"]), R.bits(want["created_pos"])), tag


@pytest.mark.parametrize("check_ori", [True, False])
@pytest.mark.parametrize("n_cur,n_last", R.SIZES)
def test_matches_reference(ctx, n_cur, n_last, check_ori):
    sc, want = R.sized(n_cur, n_last), sized_ref(n_cur, n_last, check_ori)
    assert_same(run(ctx, sc, check_ori), want, (n_cur, n_last))


@pytest.mark.parametrize("n_cur,n_last", [(5, 0), (65, 63), R.MAIN])
def test_slam_mode_creates_nothing(ctx, n_cur, n_last):
    assert_same(run(ctx, R.sized(n_cur, n_last), vo=False), sized_ref(n_cur, n_last, vo=False), (n_cur, n_last))


@pytest.mark.parametrize("bmono", [False, True])
@pytest.mark.parametrize("bounded", [False, True])
def test_mono_and_bounded_camera(ctx, bmono, bounded):
    sc = R.sized(*R.MAIN)
    assert_same(run(ctx, sc, bmono=bmono, bounded=bounded), sized_ref(*R.MAIN, bmono=bmono, bounded=bounded), (bmono, bounded))


def test_retry_cases(ctx):
    """First search enough (no retry); first short and the retry enough; both short (the gate)."""
    first = run(ctx, R.sized(*R.MAIN))
    assert_same(first, sized_ref(*R.MAIN))
    sc = R.retry_scene()
    want = R.reference(sc)
    assert want["retried"] and want["nmatches_search"] >= R.MIN_MATCHES > want["nmatches_first"]
    assert_same(run(ctx, sc), want, "retry")
    sc = R.lost_scene()
    want = R.reference(sc)
    got = run(ctx, sc)
    assert_same(got, want, "lost")
    assert np.array_equal(R.bits(got["Tcw"]), R.bits(sc["Tcw"])) and got["ninliers_pose"] == 0
    assert (got["discarded"] == -1).all() and not got["outlier"].any() and got["nmatches_map"] == 0


def test_nmatches_counts_assignments(ctx):
    """Keypoints that two last-frame points were assigned to: nmatches is the search's return less
    the discards, above the number of keypoints that hold a point; on both sides of the gate."""
    sc = R.dup_scene()
    for vo in (True, False):
        want = R.reference(sc, vo=vo)
        assert want["nmatches"] > int((want["match"] >= 0).sum())
        assert_same(run(ctx, sc, vo=vo), want, vo)
        stops = R.reference(sc, min_matches=1000, vo=vo)
        assert stops["nmatches"] == stops["nmatches_search"] > int((stops["match"] >= 0).sum())
        assert_same(run(ctx, sc, min_matches=1000, vo=vo), stops, vo)


def test_gate(ctx):
    sc = R.sized(*R.MAIN)
    nms = sized_ref(*R.MAIN)["nmatches_search"]
    assert_same(run(ctx, sc, min_matches=nms), sized_ref(*R.MAIN, True, nms))     # min_matches = nmatches still runs
    stops = run(ctx, sc, min_matches=nms + 200)                                    # the retry finds no 200 more
    want = sized_ref(*R.MAIN, True, nms + 200)
    assert want["retried"] and want["nmatches_search"] < nms + 200
    assert_same(stops, want)
    assert np.array_equal(R.bits(stops["Tcw"]), R.bits(sc["Tcw"])) and stops["ninliers_pose"] == 0
    assert np.array_equal(stops["match"], want["match_search"]) and (stops["discarded"] == -1).all()
    assert stops["nmatches"] == stops["nmatches_search"] and stops["nmatches_map"] == 0


@pytest.mark.parametrize("min_matches", [0, 2])
def test_fewer_than_three_edges_leave_the_pose(ctx, min_matches):
    sc = R.few_scene()
    want = R.reference(sc, True, min_matches)
    assert want["nmatches_search"] == 2
    got = run(ctx, sc, min_matches=min_matches)
    assert_same(got, want)
    assert np.array_equal(R.bits(got["Tcw"]), R.bits(sc["Tcw"])) and got["ninliers_pose"] == 0 and got["nmatches"] == 2


# ---- the visual-odometry step on the directed depth sets ----
@pytest.mark.parametrize("n_last", [99, 100, 101, 102, 255, 256, 257])
def test_directed_depth_sets(ctx, n_last):
    """Every (M, c) of the visit rule that fits n_last keypoints, M < n_last padded with slots of
    no depth; plain, with ties and with the special values."""
    base = R.scene(120, n_last, seed=31)
    cases = [(M, c) for M, c in R.VISIT_CASES if M <= n_last] + [(n_last, 0), (n_last, 100), (n_last, n_last)]
    for k, (M, c) in enumerate(cases):
        d = np.full(n_last, -1.0, np.float32)
        slots = np.random.default_rng(5 * n_last + k).permutation(n_last)[:M]
        d[slots] = R.directed_depth(M, c, seed=k, ties=k % 3 == 1, special=k % 3 == 2)
        sc = R.with_depth(base, d)
        want = R.reference(sc)
        got = run(ctx, sc)
        assert_same(got, want, (n_last, M, c))
        assert got["created"].sum() <= min(M, max(c, 100) + 1)


# ---- against the existing calls ----
def composed(c, sc, check_ori, min_matches, th=R.TH, bmono=False):
    """TrackWithMotionModel stitched from coeb_match_lastframe (once or twice) and
    coeb_pose_optimization, with the gather, the gate and the discard loop on the host (SLAM mode:
    no existing call creates points)."""
    cam = R.cameras()[1]
    cur, lf = R.frames(sc)
    matcher = cf.ORBmatcher(0.9, check_ori, ctx=c)
    nm = matcher.SearchByProjection(cur, lf, th, bmono, cam)
    if nm < min_matches:
        nm = matcher.SearchByProjection(cur, lf, 2 * th, bmono, cam)
    match = cur.mvpMapPoints.copy()
    n = cur.N
    if nm < min_matches:
        return dict(match=match, discarded=np.full(n, -1, np.int32), outlier=np.zeros(n, np.uint8), Tcw=sc["Tcw"],
                    nmatches_search=nm, ninliers_pose=0, nmatches=nm, nmatches_map=0, created=None, created_pos=None)
    cur.mvMapPointPos = sc["last"]["xw"][np.maximum(match, 0)]
    nin = cf.Optimizer.PoseOptimization(cur, cam, c)
    outl = np.where(match >= 0, np.asarray(cur.mvbOutlier), 0).astype(np.uint8)
    mvp, disc, nmk, nmap = R.discard_loop(match, outl, sc["last"]["mp_nobs"], nm)
    return dict(match=mvp, discarded=disc, outlier=outl, Tcw=cur.mTcw, nmatches_search=nm, ninliers_pose=nin,
                nmatches=nmk, nmatches_map=nmap, created=None, created_pos=None)


def test_equals_the_existing_calls_composed(ctx):
    for sc, tag in ((R.sized(63, 65), "63x65"), (R.sized(*R.MAIN), "main"), (R.retry_scene(), "retry"),
                    (R.lost_scene(), "lost"), (R.dup_scene(), "dup")):
        for check_ori in (True, False):
            assert_same(run(ctx, sc, check_ori, vo=False), composed(ctx, sc, check_ori, R.MIN_MATCHES), (tag, check_ori))


# ---- argument checks ----
SENT = 0x5A


def raw(c, sc, kps=None, last_kps=None, drop=None, n_cur=None, n_last=None, vo=True):
    """The C entry point with sentinel-filled outputs: (rc, every output array / scalar).
    n_cur / n_last override the sizes passed (the arrays stay as long as the scene's)."""
    kps = sc["kps"] if kps is None else kps
    la = sc["last"]
    lk = la["keys_un"] if last_kps is None else last_kps
    n = len(kps) if n_cur is None else n_cur
    nl = len(lk) if n_last is None else n_last
    arrs = dict(keys=kps, desc=sc["desc"], ur=sc["ur"], has=la["has_mp"], outl=la["outlier"], xw=la["xw"], mpd=la["mp_desc"],
                obs=np.ascontiguousarray(la["mp_nobs"], np.int32), lkeys=lk, depth=sc["depth"], vdesc=sc["last_desc"],
                Tl=sc["Tcw_last"])
    p = {k: (None if k == drop else C.c_void_p(a.ctypes.data)) for k, a in arrs.items()}
    cur = cf.CurFrameC(n, p["keys"], p["desc"], p["ur"])
    lf = cf.LastFrameC(nl, p["has"], p["outl"], p["xw"], p["mpd"], p["obs"], p["lkeys"])
    m, ml = max(len(kps), 1), max(len(lk), 1)
    out = dict(match=np.full(m, SENT, np.int32), discarded=np.full(m, SENT, np.int32), outlier=np.full(m, SENT, np.uint8),
               created=np.full(ml, SENT, np.uint8), created_pos=np.full((ml, 3), float(SENT), np.float32), T=sc["Tcw"].copy())
    vp = cf.VoPointsC(p["depth"], p["vdesc"], sc["th_depth"], out["created"].ctypes.data, out["created_pos"].ctypes.data)
    cnt = [C.c_int(SENT) for _ in range(4)]
    rc = cf.lib().coeb_track_motion_model(
        c.h, None if drop == "cam" else C.byref(R.cameras()[1]), C.byref(cur), C.byref(lf), C.byref(vp) if vo else None,
        p["Tl"], None if drop == "T" else out["T"].ctypes.data, R.TH, 0, 1, R.MIN_MATCHES,
        None if drop == "match" else out["match"].ctypes.data, out["discarded"].ctypes.data, out["outlier"].ctypes.data,
        *[C.byref(x) for x in cnt])
    out["counts"] = [x.value for x in cnt]
    return rc, out


def untouched(sc, out):
    return (all((out[k] == SENT).all() for k in ("match", "discarded", "outlier", "created", "created_pos"))
            and out["counts"] == [SENT] * 4 and np.array_equal(R.bits(out["T"]), R.bits(sc["Tcw"])))


def test_invalid_arguments_write_nothing(ctx):
    sc, want = R.sized(*R.MAIN), sized_ref(*R.MAIN)
    for kw in (dict(n_cur=4096), dict(n_cur=-1), dict(n_last=-1), dict(n_last=cf.VO_MAX_LAST + 1)):
        rc, out = raw(ctx, sc, **kw)
        assert rc == COEB_EINVAL and untouched(sc, out), kw
    # one last-frame keypoint more than the matcher's LDS takes beside 4095: refused by size alone
    rc, out = raw(ctx, sc, n_cur=R.SIZES[-1][0], n_last=R.SIZES[-1][1] + 1)
    assert rc == COEB_ERANGE and untouched(sc, out)
    for octave in (8, -1):                                         # outside the 8-level pyramid, on either frame
        kps = sc["kps"].copy()
        kps["octave"][int(np.flatnonzero(want["match"] >= 0)[3])] = octave
        rc, out = raw(ctx, sc, kps=kps)
        assert rc == COEB_EINVAL and untouched(sc, out), octave
        lk = sc["last"]["keys_un"].copy()
        lk["octave"][int(np.flatnonzero(want["created"])[0])] = octave      # a slot only the device gives a point
        rc, out = raw(ctx, sc, last_kps=lk)
        assert rc == COEB_EINVAL and untouched(sc, out), octave
    for drop in ("keys", "desc", "ur", "has", "outl", "xw", "mpd", "obs", "lkeys", "depth", "vdesc", "Tl", "T", "cam", "match"):
        rc, out = raw(ctx, sc, drop=drop)
        assert rc == COEB_EINVAL and untouched(sc, out), drop
    # the context still works, and gives the reference's answer
    rc, out = raw(ctx, sc)
    assert rc == COEB_OK and out["counts"] == [want[k] for k in COUNTS]
    for k in ("match", "discarded", "outlier", "created"):
        assert np.array_equal(out[k], want[k]), k
    assert np.array_equal(R.bits(out["T"]), R.bits(want["Tcw"]))
    made = want["created"] > 0                                      # positions are written where created only
    assert np.array_equal(R.bits(out["created_pos"][made]), R.bits(want["created_pos"][made]))
    assert (out["created_pos"][~made] == float(SENT)).all()
    rc, out = raw(ctx, sc, vo=False)
    assert rc == COEB_OK and (out["created"] == SENT).all() and out["counts"] == [sized_ref(*R.MAIN, vo=False)[k] for k in COUNTS]


def test_buffers_are_reused_across_calls_and_entry_points(ctx):
    """300 x 300, then 5 x 0, 65 x 63 and 1000 x 1000, then 300 x 300 again on one context, a
    coeb_track_local_map and a coeb_track_reference_keyframe on their own scenes in between."""
    import tlm_ref as L
    import trk_ref as K
    assert_same(run(ctx, R.sized(*R.MAIN)), sized_ref(*R.MAIN), "first")
    assert_same(run(ctx, R.sized(5, 0)), sized_ref(5, 0), "small")
    lsc = L.scene(333, 251, n_distract=400)
    lwant = L.reference(lsc)
    got = cf.track_local_map(ctx, lsc["cam"], cf.Frame(lsc["kps"], lsc["desc"], lsc["ur"], Tcw=lsc["Tcw"]), lsc["cur_obs"],
                             lsc["cur_xw"], cf.LocalPoints(*[lsc["pts"][k] for k in L.POINT_FIELDS]), L.COS_LIMIT, L.TH,
                             L.NNRATIO, False)
    assert np.array_equal(got["match"], lwant["match"]) and np.array_equal(L.bits(got["Tcw"]), L.bits(lwant["Tcw"]))
    assert_same(run(ctx, R.sized(65, 63), False), sized_ref(65, 63, False), "65x63")
    ksc = K.sized(*K.MAIN)
    v = cf.Vocabulary.from_arrays(*ksc["voc_args"])
    ctx.set_vocabulary(v)
    v.close()
    kgot = ctx.track_reference_keyframe(ksc["cam"], K.frame(ksc), K.bow_keyframe(ksc), ksc["kf"]["xw"], ksc["kf"]["obs"],
                                        levelsup=ksc["levelsup"], nnratio=K.NNRATIO, min_matches=K.MIN_MATCHES)
    kwant = K.reference(ksc)
    assert np.array_equal(kgot["match"], kwant["match"]) and np.array_equal(K.bits(kgot["Tcw"]), K.bits(kwant["Tcw"]))
    assert_same(run(ctx, R.sized(1000, 1000)), sized_ref(1000, 1000), "grown")
    assert_same(run(ctx, R.sized(*R.MAIN), vo=False), sized_ref(*R.MAIN, vo=False), "again, SLAM mode")
    assert_same(run(ctx, R.sized(*R.MAIN)), sized_ref(*R.MAIN), "again")


def test_launch_chain(ctx):
    sc = R.sized(*R.MAIN)
    ctx.profile(True)
    try:
        ctx.profile_reset()
        assert_same(run(ctx, sc), sized_ref(*R.MAIN))
        prof = ctx.profile_read()
        ctx.profile_reset()
        assert_same(run(ctx, sc, vo=False), sized_ref(*R.MAIN, vo=False))
        slam = ctx.profile_read()
    finally:
        ctx.profile(False)
    chain = {"k_vo_points", "k_match_lists", "k_match", "k_trk_pose_prep", "k_pose", "k_mm_tail"}
    for k in chain:
        assert k in prof and prof[k][1] == 1, (k, prof)
    assert all(v[1] == 0 for k, v in prof.items() if k not in chain), prof      # nothing else was launched
    assert slam.get("k_vo_points", (0, 0))[1] == 0 and slam["k_match"][1] == 1 and slam["k_pose"][1] == 1
