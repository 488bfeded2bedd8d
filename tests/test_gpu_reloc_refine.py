"""coeb_reloc_refine (MI355X only): the relocalisation refinement of one round of PnP hypotheses in
one call, every output bit for bit against the CPU composition of tests/reloc_ref.py: at sizes
around the kernels' wave (64) and workgroup (256) edges, empty sides and 1000 x 1000, with 1, 2 and
16 hypotheses whose KeyFrames differ in size (one of them empty); on every directed scene of
tests/test_reloc_ref.py alone and mixed in one call; against the existing calls composed; with both
orientation settings, a bounded camera and a monocular frame; at the argument checks; with the
context's buffers reused between entry points; and the launch chain."""
import ctypes as C

import numpy as np
import pytest

import coeb_front as cf
import reloc_ref as R

pytestmark = pytest.mark.gpu

COEB_OK, COEB_EINVAL, COEB_ERANGE = 0, -22, -34     # include/coeb_front.h
DEFAULT = (R.MIN_GOOD, R.LOW_GOOD, R.ENOUGH_GOOD)


def run(c, fr, hyps, th=DEFAULT, check_ori=True, bounded=False):
    return c.reloc_refine(R.cameras(bounded)[1], R.cur_frame(fr), [R.hyp_args(h) for h in hyps], R.TH1, R.ORB1, R.TH2,
                          R.ORB2, check_ori, *th)


def refs_of(fr, hyps, th=DEFAULT, check_ori=True, bounded=False):
    return [R.reference(fr, h, check_orientation=check_ori, min_good=th[0], low_good=th[1], enough_good=th[2],
                        bounded=bounded) for h in hyps]


def assert_same(got, refs, th=DEFAULT, tag=""):
    assert len(got["stage"]) == len(refs)
    for h, r in enumerate(refs):
        for k in R.COUNTS:
            assert int(got[k][h]) == r[k], (tag, h, k, [int(got[q][h]) for q in R.COUNTS], [r[q] for q in R.COUNTS])
        assert np.array_equal(got["match"][h], r["match"]), (tag, h, np.flatnonzero(got["match"][h] != r["match"]))
        assert np.array_equal(got["outlier"][h], r["outlier"]), (tag, h, np.flatnonzero(got["outlier"][h] != r["outlier"]))
        assert np.array_equal(R.bits(got["Tcw"][h]), R.bits(r["Tcw"])), (tag, h, got["Tcw"][h], r["Tcw"])
    assert got["first_good"] == R.first_good(refs, th[2]), (tag, got["first_good"], [r["ngood"] for r in refs])


def sized_hyps(n_cur, n_kf, nhyp):
    """nhyp KeyFrames of different sizes over one frame: n_kf, none at all, then smaller ones."""
    sizes = [n_kf, 0] + [max(n_kf - (37 * h) % 101, 0) for h in range(2, 16)]
    return [R.hypothesis(n_cur, k, seed=h + 1) for h, k in enumerate(sizes[:nhyp])]


@pytest.mark.parametrize("nhyp", [1, 2, 16])
@pytest.mark.parametrize("n_cur,n_kf", R.SIZES)
def test_matches_reference(ctx, n_cur, n_kf, nhyp):
    fr, hyps = R.frame(n_cur), sized_hyps(n_cur, n_kf, nhyp)
    th = R.thresholds_for(fr, hyps[0])
    refs = refs_of(fr, hyps, th)
    if min(n_cur, n_kf) >= 63:
        assert refs[0]["stage"] == 5                            # the whole chain runs
    assert_same(run(ctx, fr, hyps, th), refs, th, (n_cur, n_kf, nhyp))


@pytest.mark.parametrize("check_ori", [True, False])
@pytest.mark.parametrize("tag", [d[0] for d in R.directed()])
def test_directed_scene_alone(ctx, tag, check_ori):
    fr, hyp, th, stage = R.directed_case(tag)
    ref = R.directed_ref(tag, check_ori)
    if check_ori:
        assert ref["stage"] == stage
    assert_same(run(ctx, fr, [hyp], th, check_ori), [ref], th, tag)


@pytest.mark.parametrize("order,first", [(("few", "short", "rich", "thin", "mid", "wide"), 2),
                                         (("rich", "few", "mid", "short", "wide", "thin"), 0),
                                         (("few", "short", "thin", "mid"), -1),
                                         (("few", "mid", "short", "thin") * 3 + ("mid", "few", "wide", "rich"), 14)])
def test_directed_scenes_mixed(ctx, order, first):
    """The reference's thresholds over one frame: neighbouring hypotheses end in different stages,
    and the first good one is a middle index, index 0 or none."""
    fr = R.base(order[0])[0]
    hyps = [R.base(name)[1] for name in order]
    refs = refs_of(fr, hyps)
    stages = [r["stage"] for r in refs]
    assert all(a != b for a, b in zip(stages, stages[1:])) and R.first_good(refs) == first, stages
    got = run(ctx, fr, hyps)
    assert_same(got, refs, DEFAULT, order)
    assert got["first_good"] == first


def composed(c, fr, hyp, th=DEFAULT, check_ori=True):
    """One hypothesis stitched from coeb_pose_optimization (up to three times) and coeb_match_keyframe
    (up to twice) with the entry, discard, merge and gate loops on the host."""
    cam = R.cameras()[1]
    min_good, low_good, enough_good = th
    k = hyp["kf"]
    kp, n = R.hyp_args(hyp)[0], len(fr["kps"])
    F = cf.Frame(fr["kps"], fr["desc"], fr["ur"], Tcw=hyp["Tcw"])
    matcher2 = cf.ORBmatcher(0.9, check_ori, ctx=c)
    F.mvpMapPoints = np.where(hyp["inlier"] > 0, hyp["match"], -1).astype(np.int32)
    sFound = set(int(q) for q in F.mvpMapPoints[F.mvpMapPoints >= 0])
    state = dict(written=np.zeros(n, bool))

    def optimise():
        F.mvMapPointPos = k["world_pos"][np.maximum(F.mvpMapPoints, 0)] if len(k["valid"]) else np.zeros((n, 3), np.float32)
        state["written"] = F.mvpMapPoints >= 0
        return cf.Optimizer.PoseOptimization(F, cam, c)

    def discard():
        F.mvpMapPoints = np.where(np.asarray(F.mvbOutlier) > 0, -1, F.mvpMapPoints).astype(np.int32)

    def result(stage, nGood, a1=0, a2=0):
        return dict(match=F.mvpMapPoints, outlier=np.where(state["written"], F.mvbOutlier, 0).astype(np.uint8), Tcw=F.mTcw,
                    ngood=nGood, nadditional1=a1, nadditional2=a2, stage=stage)

    nGood = optimise()
    if nGood < min_good:
        return result(0, nGood)
    discard()
    if nGood >= enough_good:
        return result(1, nGood)
    a1 = matcher2.SearchByProjection(F, kp, sFound, R.TH1, R.ORB1, cam)
    if a1 + nGood < enough_good:
        return result(2, nGood, a1)
    nGood = optimise()
    if not (low_good < nGood < enough_good):
        return result(3, nGood, a1)
    sFound = set(int(q) for q in F.mvpMapPoints[F.mvpMapPoints >= 0])
    a2 = matcher2.SearchByProjection(F, kp, sFound, R.TH2, R.ORB2, cam)
    if nGood + a2 < enough_good:
        return result(4, nGood, a1, a2)
    nGood = optimise()
    discard()
    return result(5, nGood, a1, a2)


def test_equals_the_existing_calls_composed(ctx):
    for name in R.BASES:
        fr, hyp = R.base(name)
        for check_ori in (True, False):
            assert_same(run(ctx, fr, [hyp], DEFAULT, check_ori), [composed(ctx, fr, hyp, DEFAULT, check_ori)], DEFAULT,
                        (name, check_ori))
    fr, hyps = R.frame(255), sized_hyps(255, 257, 4)
    th = R.thresholds_for(fr, hyps[0])
    assert_same(run(ctx, fr, hyps, th), [composed(ctx, fr, h, th) for h in hyps], th, "255x257")


def test_bounded_camera(ctx):
    fr, hyps = R.frame(300), sized_hyps(300, 300, 3)
    th = R.thresholds_for(fr, hyps[0], bounded=True)
    plain, bounded = refs_of(fr, hyps, th), refs_of(fr, hyps, th, bounded=True)
    assert any(not np.array_equal(a["match"], b["match"]) for a, b in zip(plain, bounded))     # the bounds matter
    assert_same(run(ctx, fr, hyps, th, bounded=True), bounded, th, "bounded")


def test_monocular_frame(ctx):
    """u_right < 0 on every keypoint: monocular edges only."""
    fr = R.frame(300, mono=1.0)
    assert (fr["ur"] < 0).all()
    hyps = [R.hypothesis(300, k, seed=s, mono=1.0) for s, k in ((1, 300), (2, 257))]
    th = R.thresholds_for(fr, hyps[0])
    refs = refs_of(fr, hyps, th)
    assert refs[0]["stage"] == 5
    assert_same(run(ctx, fr, hyps, th), refs, th, "mono")


# ---- argument checks ----
SENT = 0x5A


def raw(c, fr, hyps, nhyp=None, n_cur=None, drop=None, kps=None, edit=None, th=DEFAULT):
    """The C entry point with sentinel-filled outputs: (rc, outputs).  n_cur / nhyp override the
    sizes passed; drop names a pointer passed as NULL; edit(h, fields) changes hypothesis h's
    (match, inlier, kf_n) before the call."""
    kps = fr["kps"] if kps is None else kps
    n = len(kps) if n_cur is None else n_cur
    H = len(hyps)
    keep = []
    hy = (cf.RelocHypothesisC * H)()
    for h, hp in enumerate(hyps):
        k = hp["kf"]
        f = dict(match=hp["match"].copy(), inlier=hp["inlier"].copy(), kf_n=len(k["valid"]))
        if edit:
            edit(h, f)
        arrs = [np.ascontiguousarray(k[name]) for name, _ in (("valid", 0), ("world_pos", 0), ("descriptor", 0),
                                                              ("max_distance", 0), ("min_distance", 0), ("angle", 0))]
        keep.append((f, arrs))
        ptrs = [None if drop == "kf_" + nm else C.c_void_p(a.ctypes.data)
                for nm, a in zip(("valid", "world_pos", "descriptor", "max_distance", "min_distance", "angle"), arrs)]
        hy[h].kf = cf.KeyFramePointsC(f["kf_n"], *ptrs)
        hy[h].match = None if drop == "match_in" else f["match"].ctypes.data
        hy[h].inlier = None if drop == "inlier" else f["inlier"].ctypes.data
        C.memmove(hy[h].Tcw, np.ascontiguousarray(hp["Tcw"], np.float32).ctypes.data, 64)
    p = dict(keys=kps, desc=fr["desc"], ur=fr["ur"])
    p = {k: (None if k == drop else C.c_void_p(a.ctypes.data)) for k, a in p.items()}
    cur = cf.CurFrameC(n, p["keys"], p["desc"], p["ur"])
    m = max(len(kps), 1) * H
    out = dict(match=np.full(m, SENT, np.int32), outlier=np.full(m, SENT, np.uint8))
    for k in ("ngood", "nadditional1", "nadditional2", "stage"):
        out[k] = np.full(H, SENT, np.int32)
    first = C.c_int(SENT)
    op = {k: (None if k == drop else C.c_void_p(a.ctypes.data)) for k, a in out.items()}
    rc = cf.lib().coeb_reloc_refine(
        c.h, None if drop == "cam" else C.byref(R.cameras()[1]), None if drop == "cur" else C.byref(cur),
        None if drop == "hyp" else hy, H if nhyp is None else nhyp, R.TH1, R.ORB1, R.TH2, R.ORB2, 1, *th,
        op["match"], op["outlier"], op["ngood"], op["nadditional1"], op["nadditional2"], op["stage"],
        None if drop == "first" else C.byref(first))
    out["first_good"] = first.value
    out["Tcw"] = np.array([list(hy[h].Tcw) for h in range(H)], np.float32).reshape(H, 4, 4)
    return rc, out


def untouched(hyps, out):
    return (all((out[k] == SENT).all() for k in ("match", "outlier", "ngood", "nadditional1", "nadditional2", "stage"))
            and out["first_good"] == SENT
            and all(np.array_equal(R.bits(out["Tcw"][h]), R.bits(hp["Tcw"])) for h, hp in enumerate(hyps)))


def test_invalid_arguments_write_nothing(ctx):
    fr = R.frame(300)
    hyps = [R.base("mid")[1], R.base("wide")[1]]
    refs = refs_of(fr, hyps)
    for kw in (dict(n_cur=4096), dict(n_cur=-1), dict(nhyp=0), dict(nhyp=-1), dict(nhyp=cf.RELOC_MAX_HYP + 1)):
        rc, out = raw(ctx, fr, hyps, **kw)
        assert rc == COEB_EINVAL and untouched(hyps, out), kw

    def neg_kf(h, f):
        if h == 1:
            f["kf_n"] = -1

    def match_past(h, f):
        if h == 1:
            f["match"][int(np.flatnonzero(f["match"] < 0)[0])] = f["kf_n"]

    def match_below(h, f):
        if h == 0:
            f["match"][5] = -2

    def inlier_without(h, f):
        if h == 1:
            f["inlier"][int(np.flatnonzero(f["match"] < 0)[0])] = 1

    for edit in (neg_kf, match_past, match_below, inlier_without):
        rc, out = raw(ctx, fr, hyps, edit=edit)
        assert rc == COEB_EINVAL and untouched(hyps, out), edit.__name__
    for octave in (8, -1):                                         # outside the 8-level pyramid, on a keypoint no hypothesis matched
        kps = fr["kps"].copy()
        free = np.flatnonzero((hyps[0]["match"] < 0) & (hyps[1]["match"] < 0))
        kps["octave"][int(free[0])] = octave
        rc, out = raw(ctx, fr, hyps, kps=kps)
        assert rc == COEB_EINVAL and untouched(hyps, out), octave
    for drop in ("keys", "desc", "ur", "cam", "cur", "hyp", "match", "ngood", "nadditional1", "nadditional2", "stage", "first",
                 "match_in", "inlier", "kf_valid", "kf_world_pos", "kf_descriptor", "kf_max_distance", "kf_min_distance",
                 "kf_angle"):
        rc, out = raw(ctx, fr, hyps, drop=drop)
        assert rc == COEB_EINVAL and untouched(hyps, out), drop
    # the context still works, and gives the reference's answer; flags are written only where an optimisation saw a point
    rc, out = raw(ctx, fr, hyps)
    assert rc == COEB_OK and out["first_good"] == R.first_good(refs)
    n = len(fr["kps"])
    for h, r in enumerate(refs):
        assert [int(out[k][h]) for k in R.COUNTS] == [r[k] for k in R.COUNTS]
        assert np.array_equal(out["match"][h * n:(h + 1) * n], r["match"])
        fl = out["outlier"][h * n:(h + 1) * n]
        assert np.array_equal(fl[r["written"]], r["outlier"][r["written"]]) and (fl[~r["written"]] == SENT).all()
        assert np.array_equal(R.bits(out["Tcw"][h]), R.bits(r["Tcw"]))
    rc, out = raw(ctx, fr, hyps, drop="outlier")                   # outlier_out may be NULL
    assert rc == COEB_OK and [int(v) for v in out["stage"]] == [r["stage"] for r in refs]


def test_lds_budget_is_refused_on_the_host(ctx):
    """4095 keypoints beside a KeyFrame of 60000 points: COEB_ERANGE by size alone, nothing launched."""
    n, kn = 4095, 60000
    fr = R.frame(n)
    kf = dict(valid=np.zeros(kn, np.uint8), world_pos=np.zeros((kn, 3), np.float32), descriptor=np.zeros((kn, 32), np.uint8),
              max_distance=np.ones(kn, np.float32), min_distance=np.ones(kn, np.float32), angle=np.zeros(kn, np.float32))
    big = dict(kf=kf, match=np.full(n, -1, np.int32), inlier=np.zeros(n, np.uint8), Tcw=R.T_TRUE.copy())
    hyps = [R.hypothesis(n, 300, seed=3), big]
    ctx.profile(True)
    try:
        ctx.profile_reset()
        rc, out = raw(ctx, fr, hyps)
        prof = ctx.profile_read()
    finally:
        ctx.profile(False)
    assert rc == COEB_ERANGE and untouched(hyps, out)
    assert all(v[1] == 0 for v in prof.values()), prof


def test_empty_frame_is_ok(ctx):
    fr = R.frame(0)
    hyps = [R.hypothesis(0, 5, seed=1), R.hypothesis(0, 0, seed=2)]
    rc, out = raw(ctx, fr, hyps)
    assert rc == COEB_OK and out["first_good"] == -1
    assert all((out[k] == 0).all() for k in ("ngood", "nadditional1", "nadditional2", "stage"))
    assert all(np.array_equal(R.bits(out["Tcw"][h]), R.bits(hp["Tcw"])) for h, hp in enumerate(hyps))


# ---- the context's buffers, and the single search ----
def keyframe_search(c, fr, hyp, th=R.TH1, orb_dist=R.ORB1):
    F = cf.Frame(fr["kps"], fr["desc"], fr["ur"], Tcw=hyp["Tcw"])
    nm = cf.ORBmatcher(0.9, True, ctx=c).SearchByProjection(F, R.hyp_args(hyp)[0], set(), th, orb_dist, R.cameras()[1])
    return nm, F.mvpMapPoints.copy()


def test_single_search_is_unchanged_around_a_call(ctx):
    fr, hyp = R.base("wide")
    want_nm, want_m = R.O.search_keyframe(R.cameras()[0], fr["kps"], fr["desc"], None, hyp["kf"], hyp["Tcw"], R.TH1, R.ORB1, True)
    before = keyframe_search(ctx, fr, hyp)
    hyps = sized_hyps(300, 300, 16)
    th = R.thresholds_for(fr, hyps[0])
    assert_same(run(ctx, fr, hyps, th), refs_of(fr, hyps, th), th)
    after = keyframe_search(ctx, fr, hyp)
    assert before[0] == after[0] == want_nm and np.array_equal(before[1], after[1]) and np.array_equal(before[1], want_m)
    assert tuple(ctx.debug_read("search_path").view(np.int32)[:1]) == (0,)


def test_buffers_are_reused_across_calls_and_entry_points(ctx):
    """300 x 300 x 2, then 5 x 0, 65 x 63 x 16 and 1000 x 1000 x 2, then 300 x 300 again on one context, a
    coeb_match_keyframe, a coeb_track_motion_model and a coeb_track_local_map on their own scenes in between."""
    import tlm_ref as L
    import twmm_ref as M

    def one(n_cur, n_kf, nhyp, tag):
        fr, hyps = R.frame(n_cur), sized_hyps(n_cur, n_kf, nhyp)
        th = R.thresholds_for(fr, hyps[0])
        assert_same(run(ctx, fr, hyps, th), refs_of(fr, hyps, th), th, tag)

    one(300, 300, 2, "first")
    one(5, 0, 1, "small")
    fr, hyp = R.base("rich")
    nm, m = keyframe_search(ctx, fr, hyp)
    want = R.O.search_keyframe(R.cameras()[0], fr["kps"], fr["desc"], None, hyp["kf"], hyp["Tcw"], R.TH1, R.ORB1, True)
    assert nm == want[0] and np.array_equal(m, want[1])
    one(65, 63, 16, "65x63")
    msc = M.sized(*M.MAIN)
    cur, lf = M.frames(msc)
    mgot = ctx.track_with_motion_model(M.cameras()[1], cur, lf, M.TH, False, True, M.MIN_MATCHES, depth=msc["depth"],
                                       th_depth=msc["th_depth"])
    mwant = M.reference(msc)
    assert np.array_equal(mgot["match"], mwant["match"]) and np.array_equal(M.bits(mgot["Tcw"]), M.bits(mwant["Tcw"]))
    one(1000, 1000, 2, "grown")
    lsc = L.scene(333, 251, n_distract=400)
    lwant = L.reference(lsc)
    got = cf.track_local_map(ctx, lsc["cam"], cf.Frame(lsc["kps"], lsc["desc"], lsc["ur"], Tcw=lsc["Tcw"]), lsc["cur_obs"],
                             lsc["cur_xw"], cf.LocalPoints(*[lsc["pts"][k] for k in L.POINT_FIELDS]), L.COS_LIMIT, L.TH,
                             L.NNRATIO, False)
    assert np.array_equal(got["match"], lwant["match"]) and np.array_equal(L.bits(got["Tcw"]), L.bits(lwant["Tcw"]))
    one(300, 300, 2, "again")


def test_launch_chain(ctx):
    fr, hyps = R.frame(300), sized_hyps(300, 300, 4)
    th = R.thresholds_for(fr, hyps[0])
    ctx.profile(True)
    try:
        ctx.profile_reset()
        assert_same(run(ctx, fr, hyps, th), refs_of(fr, hyps, th), th)
        prof = ctx.profile_read()
    finally:
        ctx.profile(False)
    chain = dict(k_rr_enter=1, k_pose=3, k_rr_after1=1, k_match_kf=2, k_rr_merge=2, k_rr_after2=1, k_rr_tail=1)
    for k, cnt in chain.items():
        assert k in prof and prof[k][1] == cnt, (k, prof)
    assert all(v[1] == 0 for k, v in prof.items() if k not in chain), prof      # nothing else was launched
