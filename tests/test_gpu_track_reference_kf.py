"""coeb_track_reference_keyframe (MI355X only): Frame::ComputeBoW, SearchByBoW, the nmatches gate,
PoseOptimization and the outlier discard of Tracking::TrackReferenceKeyFrame in one call, every
output bit for bit against the CPU composition of tests/trk_ref.py: at sizes around the kernels'
wave (64) edge, empty, the main 300 x 300 scene and the 4095 limit, against the three existing
calls composed, at the gate, with fewer than three edges, with the node ids given, at the
argument checks, with the context's buffers reused, and the launch chain."""
import ctypes as C
import functools

import numpy as np
import pytest

import coeb_front as cf
import trk_ref as R

pytestmark = pytest.mark.gpu

COEB_OK, COEB_EINVAL = 0, -22                       # include/coeb_front.h
COUNTS = ("nmatches_bow", "ninliers_pose", "nmatches", "nmatches_map")


@functools.lru_cache(maxsize=None)
def sized_ref(n_cur, n_kf, check_ori, min_matches=R.MIN_MATCHES):
    return R.reference(R.sized(n_cur, n_kf), check_ori, min_matches)


@pytest.fixture
def voc_ctx(ctx):
    """The session context with a scene's vocabulary set (set_vocabulary replaces the tables)."""
    def use(sc, c=ctx):
        v = cf.Vocabulary.from_arrays(*sc["voc_args"])
        c.set_vocabulary(v)
        v.close()
        return c
    return use


def run(c, sc, check_ori=True, min_matches=R.MIN_MATCHES, node=None):
    return c.track_reference_keyframe(sc["cam"], R.frame(sc), R.bow_keyframe(sc), sc["kf"]["xw"], sc["kf"]["obs"],
                                      cur_node_id=node, levelsup=sc["levelsup"], nnratio=R.NNRATIO,
                                      check_orientation=check_ori, min_matches=min_matches)


def assert_same(got, want, tag="", bow=True):
    if bow:
        for k in ("word", "node"):
            assert np.array_equal(got[k], want[k]), (tag, k)
        assert np.array_equal(got["weight"].view(np.uint64), want["weight"].view(np.uint64)), tag
    for k in ("match", "discarded"):
        assert np.array_equal(got[k], want[k]), (tag, k, got[k], want[k])
    assert [got[k] for k in COUNTS] == [want[k] for k in COUNTS], (tag, [got[k] for k in COUNTS], [want[k] for k in COUNTS])
    assert np.array_equal(R.bits(got["Tcw"]), R.bits(want["Tcw"])), (tag, got["Tcw"], want["Tcw"])


@pytest.mark.parametrize("check_ori", [True, False])
@pytest.mark.parametrize("n_cur,n_kf", R.SIZES)
def test_matches_reference(voc_ctx, n_cur, n_kf, check_ori):
    sc, want = R.sized(n_cur, n_kf), sized_ref(n_cur, n_kf, check_ori)
    assert_same(run(voc_ctx(sc), sc, check_ori), want, (n_cur, n_kf))


def composed(c, sc, check_ori, min_matches):
    """TrackReferenceKeyFrame stitched from coeb_bow_transform, coeb_match_bow and
    coeb_pose_optimization, with the gate and the discard loop on the host."""
    F = R.frame(sc)
    F.ComputeBoW(c, sc["levelsup"])
    nmb = cf.ORBmatcher(R.NNRATIO, check_ori, ctx=c).SearchByBoW(R.bow_keyframe(sc), F)
    match = F.mvpMapPoints.copy()
    res = dict(word=F.mBowWord, node=F.mFeatNode, weight=F.mBowWeight, nmatches_bow=nmb)
    if nmb < min_matches:
        res.update(match=match, discarded=np.full(F.N, -1, np.int32), Tcw=sc["Tcw"], ninliers_pose=0, nmatches=nmb,
                   nmatches_map=0)
        return res
    F.mvMapPointPos = sc["kf"]["xw"][np.maximum(match, 0)] if len(sc["kf"]["xw"]) else np.zeros((F.N, 3), np.float32)
    nin = cf.Optimizer.PoseOptimization(F, sc["cam"], c)
    outl = np.where(match >= 0, np.asarray(F.mvbOutlier), 0)
    mvp, disc, nm, nmap = R.discard_loop(match, outl, sc["kf"]["obs"], nmb)
    res.update(match=mvp, discarded=disc, Tcw=F.mTcw, ninliers_pose=nin, nmatches=nm, nmatches_map=nmap)
    return res


@pytest.mark.parametrize("n_cur,n_kf", [(63, 65), R.MAIN, (5, 0)])
def test_equals_the_three_calls_composed(voc_ctx, n_cur, n_kf):
    sc = R.sized(n_cur, n_kf)
    c = voc_ctx(sc)
    for check_ori in (True, False):
        assert_same(run(c, sc, check_ori), composed(c, sc, check_ori, R.MIN_MATCHES), (n_cur, n_kf, check_ori))


def test_gate(voc_ctx):
    sc = R.sized(*R.MAIN)
    c = voc_ctx(sc)
    nmb = sized_ref(*R.MAIN, True)["nmatches_bow"]
    runs = run(c, sc, True, nmb)
    assert_same(runs, sized_ref(*R.MAIN, True, nmb))
    assert_same(runs, sized_ref(*R.MAIN, True))                    # min_matches = nmatches_bow still runs
    stops = run(c, sc, True, nmb + 1)
    want = sized_ref(*R.MAIN, True, nmb + 1)
    assert_same(stops, want)
    assert np.array_equal(R.bits(stops["Tcw"]), R.bits(sc["Tcw"])) and stops["ninliers_pose"] == 0
    assert np.array_equal(stops["match"], want["match_bow"]) and (stops["discarded"] == -1).all()
    assert stops["nmatches"] == nmb and stops["nmatches_map"] == 0


def test_fewer_than_three_edges_leave_the_pose(voc_ctx):
    sc = R.two_matches()
    want = R.reference(sc, True, 0)
    assert want["nmatches_bow"] == 2
    got = run(voc_ctx(sc), sc, True, 0)
    assert_same(got, want)
    assert np.array_equal(R.bits(got["Tcw"]), R.bits(sc["Tcw"])) and got["ninliers_pose"] == 0 and got["nmatches"] == 2


def test_precomputed_node_ids_need_no_vocabulary():
    """A fresh context without a vocabulary: with the frame's node ids given the results are the
    computed path's, and word / node / weight stay as the caller filled them."""
    sc, want = R.sized(*R.MAIN), sized_ref(*R.MAIN, True)
    c = cf.Context(max_width=640, max_height=480, max_batch=1)
    try:
        assert_same(run(c, sc, node=want["node"]), want, bow=False)
        rc, out = raw(c, sc, node=want["node"])
        assert rc == COEB_OK
        assert (out["word"] == SENT).all() and (out["node"] == SENT).all() and (out["weight"] == float(SENT)).all()
        assert np.array_equal(out["match"], want["match"]) and out["counts"] == [want[k] for k in COUNTS]
        empty = R.sized(0, 5)
        assert_same(run(c, empty, node=np.zeros(0, np.int32)), sized_ref(0, 5, True), bow=False)
    finally:
        c.close()


# ---- argument checks ----
SENT = 0x5A


def raw(c, sc, node=None, kps=None, drop=None, n_cur=None, n_kf=None):
    """The C entry point with sentinel-filled outputs: (rc, every output array / scalar).
    n_cur / n_kf override the sizes passed (the arrays stay as long as the scene's)."""
    kps = sc["kps"] if kps is None else kps
    n = len(kps) if n_cur is None else n_cur
    kf = sc["kf"]
    nq = len(kf["valid"]) if n_kf is None else n_kf
    cur = cf.CurFrameC(n, C.c_void_p(kps.ctypes.data), C.c_void_p(sc["desc"].ctypes.data), C.c_void_p(sc["ur"].ctypes.data))
    arrs = dict(valid=kf["valid"], desc=kf["desc"], node=np.ascontiguousarray(kf["node"], np.int32), angle=kf["angle"],
                xw=kf["xw"], obs=np.ascontiguousarray(kf["obs"], np.int32))
    ptr = {k: (None if k == drop else C.c_void_p(a.ctypes.data)) for k, a in arrs.items()}
    kc = cf.RefKeyFrameC(cf.BowKeyFrameC(nq, ptr["valid"], ptr["desc"], ptr["node"], ptr["angle"]), ptr["xw"], ptr["obs"])
    m = max(len(kps), n, 1)
    out = dict(word=np.full(m, SENT, np.int32), node=np.full(m, SENT, np.int32), weight=np.full(m, float(SENT)),
               match=np.full(m, SENT, np.int32), discarded=np.full(m, SENT, np.int32), T=sc["Tcw"].copy())
    cnt = [C.c_int(SENT) for _ in range(4)]
    nd = None if node is None else np.ascontiguousarray(node, np.int32)
    rc = cf.lib().coeb_track_reference_keyframe(
        c.h, C.byref(sc["cam"]), C.byref(cur), None if nd is None else C.c_void_p(nd.ctypes.data), sc["levelsup"],
        C.byref(kc), out["T"].ctypes.data, R.NNRATIO, 1, R.MIN_MATCHES, out["word"].ctypes.data, out["node"].ctypes.data,
        out["weight"].ctypes.data, out["match"].ctypes.data, out["discarded"].ctypes.data, *[C.byref(x) for x in cnt])
    out["counts"] = [x.value for x in cnt]
    for k in ("word", "node", "weight", "match", "discarded"):
        out[k] = out[k][:len(kps)]
    return rc, out


def untouched(sc, out):
    return (all((out[k] == SENT).all() for k in ("word", "node", "weight", "match", "discarded"))
            and out["counts"] == [SENT] * 4 and np.array_equal(R.bits(out["T"]), R.bits(sc["Tcw"])))


def test_invalid_arguments_write_nothing(voc_ctx):
    sc, want = R.sized(*R.MAIN), sized_ref(*R.MAIN, True)
    fresh = cf.Context(max_width=640, max_height=480, max_batch=1)
    try:
        rc, out = raw(fresh, sc)                                    # NULL cur_node_id without a vocabulary
        assert rc == COEB_EINVAL and untouched(sc, out) and b"no vocabulary" in cf.lib().coeb_last_error(fresh.h)
    finally:
        fresh.close()
    c = voc_ctx(sc)
    for kw in (dict(n_cur=4096), dict(n_kf=4096), dict(n_cur=-1), dict(n_kf=-1)):
        rc, out = raw(c, sc, **kw)
        assert rc == COEB_EINVAL and untouched(sc, out), kw
    kps = sc["kps"].copy()
    i = int(np.flatnonzero(want["match"] >= 0)[3])
    kps["octave"][i] = 8                                            # a matched keypoint outside the 8-level pyramid
    rc, out = raw(c, sc, kps=kps)
    assert rc == COEB_EINVAL and untouched(sc, out)
    kps["octave"][i] = -1
    assert raw(c, sc, kps=kps)[0] == COEB_EINVAL
    for drop in ("xw", "obs", "valid", "desc", "node", "angle"):
        rc, out = raw(c, sc, drop=drop)
        assert rc == COEB_EINVAL and untouched(sc, out), drop
    # the context still works, and gives the reference's answer
    rc, out = raw(c, sc)
    assert rc == COEB_OK and np.array_equal(out["match"], want["match"]) and out["counts"] == [want[k] for k in COUNTS]
    assert np.array_equal(out["discarded"], want["discarded"]) and np.array_equal(R.bits(out["T"]), R.bits(want["Tcw"]))
    assert_same(run(c, sc), want)


def test_buffers_are_reused_across_calls_and_entry_points(voc_ctx):
    """300 x 300, then 5 x 0, then 300 x 300 again on one context, a coeb_match_bow and a
    coeb_track_local_map on their own scenes in between: every result equals its reference."""
    import tlm_ref as L
    main, small, bow_sc = R.sized(*R.MAIN), R.sized(5, 0), R.sized(63, 65)
    lsc = L.scene(333, 251, n_distract=400)
    lwant = L.reference(lsc)
    c = voc_ctx(main)
    assert_same(run(c, main), sized_ref(*R.MAIN, True), "first")
    F = R.frame(bow_sc)
    F.mFeatNode = bow_sc["bow"]["node"]
    nm = cf.ORBmatcher(R.NNRATIO, True, ctx=c).SearchByBoW(R.bow_keyframe(bow_sc), F)
    assert nm == sized_ref(63, 65, True)["nmatches_bow"] and np.array_equal(F.mvpMapPoints, sized_ref(63, 65, True)["match_bow"])
    assert_same(run(voc_ctx(small), small), sized_ref(5, 0, True), "small")
    got = cf.track_local_map(c, lsc["cam"], cf.Frame(lsc["kps"], lsc["desc"], lsc["ur"], Tcw=lsc["Tcw"]), lsc["cur_obs"],
                             lsc["cur_xw"], cf.LocalPoints(*[lsc["pts"][k] for k in L.POINT_FIELDS]), L.COS_LIMIT, L.TH,
                             L.NNRATIO, False)
    assert np.array_equal(got["match"], lwant["match"]) and np.array_equal(L.bits(got["Tcw"]), L.bits(lwant["Tcw"]))
    assert got["nmatches_inliers"] == lwant["nmatches_inliers"] and np.array_equal(got["outlier"], lwant["outlier"])
    assert_same(run(voc_ctx(main), main, False), sized_ref(*R.MAIN, False), "again")


def test_launch_chain(voc_ctx):
    sc = R.sized(*R.MAIN)
    c = voc_ctx(sc)
    c.profile(True)
    try:
        c.profile_reset()
        assert_same(run(c, sc), sized_ref(*R.MAIN, True))
        prof = c.profile_read()
    finally:
        c.profile(False)
    for k in ("k_bow_transform", "k_bow_csr", "k_match_bow", "k_bow_rot", "k_trk_pose_prep", "k_pose", "k_trk_tail"):
        assert k in prof and prof[k][1] == 1, (k, prof)
    chain = {"k_bow_transform", "k_bow_csr", "k_match_bow", "k_bow_rot", "k_trk_pose_prep", "k_pose", "k_trk_tail"}
    assert all(v[1] == 0 for k, v in prof.items() if k not in chain), prof     # nothing else was launched
