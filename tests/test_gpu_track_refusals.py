"""The refusals of the nine single-frame tracking calls (MI355X only, as every call takes a context):
code, message and precedence, through the raw C entry points.  Every case returns from a host-side
check before anything is launched, with the caller's outputs as they were.  The expected strings
are the ones the library carried before its staging code was shared between the calls; the
precedence differs between the calls (coeb_track_local_map tests octaves before the LDS budget,
coeb_track_motion_model the budget first, coeb_reloc_refine every hypothesis's arrays before the
octaves), which the double faults at the end of each group pin."""
import ctypes as C

import numpy as np
import pytest

import coeb_front as cf

pytestmark = pytest.mark.gpu

EINVAL, ERANGE = -22, -34                           # include/coeb_front.h
SENT = 0x5A
CAP = 4096          # every array holds at least this many elements: a size that slipped past its check reads inside them
NLEVELS = 8         # the session context's pyramid
BIG = dict(n=8, nq=20000)                           # test_gpu_track_local_map.py's LDS-budget shape
CAM = cf.make_camera(500.0, 500.0, 320.0, 240.0, 40.0, 640, 480)
# coeb_match_* and coeb_pose_optimization zero their count once the pointers are there; the fused calls write nothing
ZEROES_COUNT = ("coeb_match_lastframe", "coeb_match_localmap", "coeb_match_keyframe", "coeb_pose_optimization")


def vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def keypoints(cap, octave):
    k = np.zeros(cap, cf.KEYPOINT_DTYPE)
    k["octave"] = octave
    return k


def struct(cls, prefix, n, arrays, m):
    """cls(n, arrays...) with the array m["drop"] names ("<prefix>.<field>") passed as NULL."""
    return cls(n, *[None if prefix + "." + k == m.get("drop") else vp(a) for k, a in arrays.items()])


def cam(m):
    return None if m.get("null") else C.byref(CAM)


def cur_frame(m):
    n = m.get("n", 1)
    cap = max(CAP, n)
    a = dict(keys_un=keypoints(cap, m.get("octave", 0)), descriptors=np.zeros((cap, 32), np.uint8),
             u_right=np.full(cap, -1, np.float32))
    return a, struct(cf.CurFrameC, "cur", n, a, m), cap


def last_frame(m):
    nl = m.get("nq", 1)
    cap = max(CAP, nl)
    a = dict(has_mappoint=np.ones(cap, np.uint8), outlier=np.zeros(cap, np.uint8), world_pos=np.zeros((cap, 3), np.float32),
             mp_descriptor=np.zeros((cap, 32), np.uint8), mp_observations=np.ones(cap, np.int32),
             keys_un=keypoints(cap, m.get("octave2", 0)))
    return a, struct(cf.LastFrameC, "last", nl, a, m)


def keyframe_points(m):
    nq = m.get("nq", 1)
    cap = max(CAP, nq)
    a = dict(valid=np.ones(cap, np.uint8), world_pos=np.zeros((cap, 3), np.float32), descriptor=np.zeros((cap, 32), np.uint8),
             max_distance=np.full(cap, 10, np.float32), min_distance=np.full(cap, 1, np.float32), angle=np.zeros(cap, np.float32))
    return a, struct(cf.KeyFramePointsC, "kf", nq, a, m)


def sent(n, dt=np.int32):
    return np.full(n, SENT, dt)


def pose():
    return np.eye(4, dtype=np.float32)


def counts(k):
    return [C.c_int(SENT) for _ in range(k)]


def coeb_match_lastframe(ctx, m):
    ca, cu, cap = cur_frame(m)
    la, last = last_frame(m)
    T, match, cnt = pose(), sent(cap), counts(1)
    rc = cf.lib().coeb_match_lastframe(ctx.h, cam(m), C.byref(cu), C.byref(last), vp(T), vp(T), 15.0, 0, 1, vp(match),
                                       C.byref(cnt[0]))
    return rc, [match], cnt, [T]


def coeb_match_localmap(ctx, m):
    ca, cu, cap = cur_frame(m)
    nq = m.get("nq", 1)
    capq = max(CAP, nq)
    z = np.zeros(capq, np.float32)
    a = dict(in_view=np.ones(capq, np.uint8), proj_x=z, proj_y=z, proj_xr=z, level=np.full(capq, m.get("octave2", 0), np.int32),
             view_cos=z, descriptor=np.zeros((capq, 32), np.uint8), observations=np.ones(capq, np.int32))
    mp = struct(cf.LocalMapC, "mp", nq, a, m)
    match, cnt = sent(cap), counts(1)
    rc = cf.lib().coeb_match_localmap(ctx.h, cam(m), C.byref(cu), None, C.byref(mp), 3.0, 0.8, vp(match), C.byref(cnt[0]))
    return rc, [match], cnt, []


def coeb_match_keyframe(ctx, m):
    ca, cu, cap = cur_frame(m)
    ka, kf = keyframe_points(m)
    T, match, cnt = pose(), sent(cap), counts(1)
    rc = cf.lib().coeb_match_keyframe(ctx.h, cam(m), C.byref(cu), None, C.byref(kf), vp(T), 10.0, 100, 1, vp(match),
                                      C.byref(cnt[0]))
    return rc, [match], cnt, [T]


def coeb_pose_optimization(ctx, m):
    n = m.get("n", 1)
    cap = max(CAP, n)
    a = dict(has_mappoint=np.ones(cap, np.uint8), world_pos=np.ones((cap, 3), np.float32), keys_un=keypoints(cap, m.get("octave", 0)),
             u_right=np.full(cap, -1, np.float32))
    fr = struct(cf.PoseFrameC, "fr", n, a, m)
    T, outl, cnt = pose(), sent(cap, np.uint8), counts(1)
    rc = cf.lib().coeb_pose_optimization(ctx.h, cam(m), C.byref(fr), vp(T), vp(outl), C.byref(cnt[0]))
    return rc, [outl], cnt, [T]


def local_points(m):
    nq = m.get("nq", 1)
    cap = max(CAP, nq)
    a = dict(valid=np.zeros(cap, np.uint8), world_pos=np.zeros((cap, 3), np.float32), normal=np.zeros((cap, 3), np.float32),
             max_distance=np.zeros(cap, np.float32), min_distance=np.zeros(cap, np.float32),
             descriptor=np.zeros((cap, 32), np.uint8), observations=np.zeros(cap, np.int32))
    fields = [sent(cap, dt) for dt in (np.uint8, np.float32, np.float32, np.float32, np.int32, np.float32)]
    return a, struct(cf.LocalPointsC, "mp", nq, a, m), fields, cf.TrackFieldsC(*[vp(f) for f in fields])


def coeb_search_local_points(ctx, m):
    ca, cu, cap = cur_frame(m)
    pa, lp, fields, tf = local_points(m)
    T, match, cnt = pose(), sent(cap), counts(2)
    rc = cf.lib().coeb_search_local_points(ctx.h, cam(m), C.byref(cu), None, vp(T), C.byref(lp), 0.5, 3.0, 0.8, C.byref(tf),
                                           vp(match), *[C.byref(c) for c in cnt])
    return rc, [match] + fields, cnt, [T]


def coeb_track_local_map(ctx, m):
    ca, cu, cap = cur_frame(m)
    pa, lp, fields, tf = local_points(m)
    T, match, outl, cnt = pose(), sent(cap), sent(cap, np.uint8), counts(4)
    rc = cf.lib().coeb_track_local_map(ctx.h, cam(m), C.byref(cu), None, None, vp(T), C.byref(lp), 0.5, 3.0, 0.8, 0,
                                       C.byref(tf), vp(match), vp(outl), *[C.byref(c) for c in cnt])
    return rc, [match, outl] + fields, cnt, [T]


def coeb_track_reference_keyframe(ctx, m):
    ca, cu, cap = cur_frame(m)
    nq = m.get("nq", 1)
    capq = max(CAP, nq)
    ba = dict(valid=np.ones(capq, np.uint8), descriptor=np.zeros((capq, 32), np.uint8), node_id=np.zeros(capq, np.int32),
              angle=np.zeros(capq, np.float32))
    ra = dict(world_pos=np.zeros((capq, 3), np.float32), observations=np.ones(capq, np.int32))
    kf = cf.RefKeyFrameC(struct(cf.BowKeyFrameC, "kf", nq, ba, m),
                         *[None if "kf." + k == m.get("drop") else vp(a) for k, a in ra.items()])
    node = np.zeros(cap, np.int32)                  # the frame's node ids given: no vocabulary needed
    T, cnt = pose(), counts(4)
    outs = [sent(cap), sent(cap), np.full(cap, float(SENT)), sent(cap), sent(cap)]      # word, node, weight, match, discarded
    rc = cf.lib().coeb_track_reference_keyframe(ctx.h, cam(m), C.byref(cu), vp(node), 0, C.byref(kf), vp(T), 0.7, 1, 15,
                                                *[vp(o) for o in outs], *[C.byref(c) for c in cnt])
    return rc, outs, cnt, [T]


def coeb_track_motion_model(ctx, m):
    ca, cu, cap = cur_frame(m)
    la, last = last_frame(m)
    T, cnt = pose(), counts(4)
    outs = [sent(cap), sent(cap), sent(cap, np.uint8)]                                  # match, discarded, outlier
    rc = cf.lib().coeb_track_motion_model(ctx.h, cam(m), C.byref(cu), C.byref(last), None, vp(pose()), vp(T), 15.0, 0, 1, 20,
                                          *[vp(o) for o in outs], *[C.byref(c) for c in cnt])
    return rc, outs, cnt, [T]


def coeb_reloc_refine(ctx, m):
    ca, cu, cap = cur_frame(m)
    ka, kf = keyframe_points(m)
    ha = dict(match=np.full(cap, -1, np.int32), inlier=np.zeros(cap, np.uint8))
    ha["match"][0] = m.get("match0", -1)
    hyp = (cf.RelocHypothesisC * 1)()
    hyp[0].kf = kf
    hyp[0].match, hyp[0].inlier = [None if "hyp." + k == m.get("drop") else a.ctypes.data for k, a in ha.items()]
    hyp[0].Tcw[:] = pose().ravel().tolist()
    outs = [sent(cap), sent(cap, np.uint8), sent(1), sent(1), sent(1), sent(1)]    # match, outlier, ngood, nadd1, nadd2, stage
    cnt = counts(1)
    rc = cf.lib().coeb_reloc_refine(ctx.h, cam(m), C.byref(cu), hyp, m.get("nhyp", 1), 10.0, 100, 3.0, 64, 1, 10, 30, 50,
                                    *[vp(o) for o in outs], C.byref(cnt[0]))
    return rc, outs, cnt, [np.array(hyp[0].Tcw[:], np.float32).reshape(4, 4)]


def group(entry, who, rows):
    """who: the prefix the call puts in front of a message ("" where it has none)."""
    return [pytest.param(entry, m, code, msg.replace("@", who), id="%s-%s" % (entry.__name__, tag)) for tag, m, code, msg in rows]


OCT = dict(octave=NLEVELS)
CASES = (
    group(coeb_match_lastframe, "coeb_match_lastframe", [
        ("null", dict(null=1), EINVAL, "@: invalid arguments"),
        ("negative", dict(n=-1), EINVAL, "negative frame size"),
        ("negative-last", dict(nq=-1), EINVAL, "negative frame size"),
        ("4096", dict(n=4096), EINVAL, "more than 4095 current keypoints"),
        ("missing-cur", dict(drop="cur.descriptors"), EINVAL, "@: missing current-frame arrays"),
        ("missing-last", dict(drop="last.world_pos"), EINVAL, "@: missing LastFrame arrays"),
        ("octave", dict(octave2=NLEVELS), EINVAL, "@: LastFrame keypoint octave outside the pyramid"),
        ("lds", BIG, ERANGE, "@: the two frames exceed the LDS budget"),
        ("octave+lds", dict(BIG, octave2=NLEVELS), EINVAL, "@: LastFrame keypoint octave outside the pyramid")])
    + group(coeb_match_localmap, "coeb_match_localmap", [
        ("null", dict(null=1), EINVAL, "@: invalid arguments"),
        ("negative", dict(n=-1), EINVAL, "negative frame / local map size"),
        ("negative-map", dict(nq=-1), EINVAL, "negative frame / local map size"),
        ("4096", dict(n=4096), EINVAL, "more than 4095 current keypoints"),
        ("missing-cur", dict(drop="cur.u_right"), EINVAL, "@: missing current-frame arrays"),
        ("missing-map", dict(drop="mp.level"), EINVAL, "@: missing local-map arrays"),
        ("level", dict(octave2=NLEVELS), EINVAL, "@: predicted level outside the pyramid")])
    + group(coeb_match_keyframe, "coeb_match_keyframe", [
        ("null", dict(null=1), EINVAL, "@: invalid arguments"),
        ("negative", dict(n=-1), EINVAL, "negative frame / keyframe size"),
        ("negative-kf", dict(nq=-1), EINVAL, "negative frame / keyframe size"),
        ("4096", dict(n=4096), EINVAL, "more than 4095 current keypoints"),
        ("missing-cur", dict(drop="cur.descriptors"), EINVAL, "@: missing current-frame arrays"),
        ("missing-kf", dict(drop="kf.angle"), EINVAL, "@: missing keyframe arrays"),
        ("lds", BIG, ERANGE, "@: frame and keyframe exceed the LDS budget")])
    + group(coeb_pose_optimization, "coeb_pose_optimization", [      # no keypoint limit of its own: no 4096 case
        ("null", dict(null=1), EINVAL, "@: invalid arguments"),
        ("negative", dict(n=-1), EINVAL, "negative frame size"),
        ("missing", dict(drop="fr.world_pos"), EINVAL, "@: missing frame arrays"),
        ("octave", OCT, EINVAL, "@: keypoint octave outside the pyramid")])
    + [c for entry in (coeb_search_local_points, coeb_track_local_map) for c in group(entry, entry.__name__, [
        ("null", dict(null=1), EINVAL, "@: invalid arguments"),
        ("negative", dict(n=-1), EINVAL, "@: negative frame / local map size"),
        ("negative-map", dict(nq=-1), EINVAL, "@: negative frame / local map size"),
        ("4096", dict(n=4096), EINVAL, "@: more than 4095 current keypoints"),
        ("missing-cur", dict(drop="cur.descriptors"), EINVAL, "@: missing current-frame arrays"),
        ("missing-map", dict(drop="mp.normal"), EINVAL, "@: missing local-map arrays"),
        ("octave", OCT, EINVAL, "@: keypoint octave outside the pyramid"),
        ("lds", BIG, ERANGE, "@: frame and local map exceed the LDS budget"),
        ("octave+lds", dict(BIG, **OCT), EINVAL, "@: keypoint octave outside the pyramid")])]
    + group(coeb_track_reference_keyframe, "coeb_track_reference_keyframe", [
        ("null", dict(null=1), EINVAL, "@: invalid arguments"),
        ("negative", dict(n=-1), EINVAL, "@: negative frame / keyframe size"),
        ("negative-kf", dict(nq=-1), EINVAL, "@: negative frame / keyframe size"),
        ("4096", dict(n=4096), EINVAL, "@: more than 4095 features"),
        ("4096-kf", dict(nq=4096), EINVAL, "@: more than 4095 features"),
        ("missing-cur", dict(drop="cur.descriptors"), EINVAL, "@: missing current-frame arrays"),
        ("missing-kf", dict(drop="kf.observations"), EINVAL, "@: missing keyframe arrays"),
        ("octave", OCT, EINVAL, "@: keypoint octave outside the pyramid")])
    + group(coeb_track_motion_model, "coeb_track_motion_model", [
        ("null", dict(null=1), EINVAL, "@: invalid arguments"),
        ("negative", dict(n=-1), EINVAL, "@: negative frame size"),
        ("negative-last", dict(nq=-1), EINVAL, "@: negative frame size"),
        ("4096", dict(n=4096), EINVAL, "@: more than 4095 current keypoints"),
        ("missing-cur", dict(drop="cur.u_right"), EINVAL, "@: missing current-frame arrays"),
        ("missing-last", dict(drop="last.outlier"), EINVAL, "@: missing LastFrame arrays"),
        ("octave", OCT, EINVAL, "@: keypoint octave outside the pyramid"),
        ("octave-last", dict(octave2=NLEVELS), EINVAL, "@: LastFrame keypoint octave outside the pyramid"),
        ("both-octaves", dict(OCT, octave2=NLEVELS), EINVAL, "@: keypoint octave outside the pyramid"),
        ("lds", BIG, ERANGE, "@: the two frames exceed the LDS budget"),
        ("octave+lds", dict(BIG, **OCT), ERANGE, "@: the two frames exceed the LDS budget")])
    + group(coeb_reloc_refine, "coeb_reloc_refine", [
        ("null", dict(null=1), EINVAL, "@: invalid arguments"),
        ("nhyp", dict(nhyp=0), EINVAL, "@: nhyp outside 1..COEB_RELOC_MAX_HYP"),
        ("negative", dict(n=-1), EINVAL, "@: negative frame size"),
        ("negative-kf", dict(nq=-1), EINVAL, "@: negative keyframe size"),
        ("4096", dict(n=4096), EINVAL, "@: more than 4095 current keypoints"),
        ("missing-cur", dict(drop="cur.u_right"), EINVAL, "@: missing current-frame arrays"),
        ("missing-kf", dict(drop="kf.valid"), EINVAL, "@: missing keyframe arrays"),
        ("missing-match", dict(drop="hyp.match"), EINVAL, "@: missing match / inlier arrays"),
        ("match", dict(match0=1), EINVAL, "@: match outside [-1, kf.n)"),
        ("octave", OCT, EINVAL, "@: keypoint octave outside the pyramid"),
        ("lds", BIG, ERANGE, "@: frame and keyframe exceed the LDS budget"),
        ("match+octave", dict(OCT, match0=1), EINVAL, "@: match outside [-1, kf.n)"),
        ("octave+lds", dict(BIG, **OCT), EINVAL, "@: keypoint octave outside the pyramid")]))


@pytest.mark.parametrize("entry,m,code,msg", CASES)
def test_refusal(ctx, entry, m, code, msg):
    rc, outs, cnt, poses = entry(ctx, m)
    got = cf.lib().coeb_last_error(ctx.h).decode()
    assert rc == code and got == msg, (rc, got)
    for o in outs:
        assert (o == o.dtype.type(SENT)).all()
    zeroed = entry.__name__ in ZEROES_COUNT and not m.get("null")
    assert [c.value for c in cnt] == [0 if zeroed else SENT] * len(cnt)
    for T in poses:
        assert np.array_equal(T.view(np.uint32), pose().view(np.uint32))
