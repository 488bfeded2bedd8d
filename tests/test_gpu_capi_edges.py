"""The single-frame C-ABI the way the C++ adapters call it (adapter/ORBextractor.h passes
image.step[0], adapter/Frame_coeb.h imgray.step[0]): strided inputs, null and short output
arrays, the LK window at the last inside position of every pyramid level, and the reference's
adaptive extractor sequence (Tracking.cc:426-466).  Every comparison is bit-exact against the
oracle run on np.ascontiguousarray(view); floats are compared as their bit patterns.  The calls
go through coeb_front.lib() with ctypes, since the Python wrappers hide the arguments under test
(MI355X only)."""
import ctypes as C
import time

import numpy as np
import pytest

import coeb_front as cf
from coeb_front import KEYPOINT_DTYPE, synth
from test_gpu_parity import assert_same, keyframe_both, localmap_both, match_both

pytestmark = pytest.mark.gpu

COEB_OK, COEB_EINVAL, COEB_ERANGE = 0, -22, -34          # include/coeb_front.h
SENTINEL = 0xA5


def bits(a):
    """Float arrays as their bit patterns (NaN == NaN, -0 != +0)."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(a, b, tag):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, (tag, a.shape, b.shape)
    bad = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0] if len(a) else []
    assert len(bad) == 0, (tag, len(bad), a[bad[:3]], b[bad[:3]])


def in_parent(img, stride, fill):
    """img as a view of a (rows, stride) parent whose other bytes are `fill` (a value, or
    "garbage": random bytes)."""
    h, w = img.shape
    if isinstance(fill, str):
        parent = np.random.default_rng(stride).integers(0, 256, (h, stride)).astype(img.dtype)
    else:
        parent = np.full((h, stride), fill, img.dtype)
    parent[:, :w] = img
    view = parent[:, :w]
    assert view.strides[0] == stride * img.itemsize and not view.flags["C_CONTIGUOUS"]
    return view


def raw_extract(ctx, view, stride, dyn=None, cap=None, want_kps=True, want_desc=True):
    """coeb_extract on the view's own memory with row pitch `stride`: (rc, n, kps, desc), the
    output arrays pre-filled with SENTINEL over the context's whole capacity."""
    h, w = view.shape
    full = ctx.max_keypoints(w, h)
    kps = np.frombuffer(bytes([SENTINEL]) * (28 * full), KEYPOINT_DTYPE).copy()
    desc = np.full((full, 32), SENTINEL, np.uint8)
    boxes, tm, blur = dyn if dyn is not None else (None, None, None)
    n = C.c_int(-1)
    rc = cf.lib().coeb_extract(ctx.h, view.ctypes.data, w, h, stride,
                               None if boxes is None else boxes.ctypes.data, 0 if boxes is None else len(boxes),
                               None if tm is None else tm.ctypes.data, 0 if tm is None else len(tm),
                               None if blur is None else blur.ctypes.data, 0 if blur is None else len(blur),
                               kps.ctypes.data if want_kps else None, desc.ctypes.data if want_desc else None,
                               full if cap is None else cap, C.byref(n))
    return rc, n.value, kps, desc


def kp_bytes(k):
    return np.ascontiguousarray(k).view(np.uint8).reshape(len(k), 28)


def untouched(kps, desc, first):
    """Rows at or after `first` still hold the sentinel."""
    return bool((kp_bytes(kps)[first:] == SENTINEL).all() and (desc[first:] == SENTINEL).all())


def expect_exact(rc, n, kps, desc, ref, tag):
    assert rc == COEB_OK, (tag, rc)
    assert_same(kps[:n], desc[:n], ref["kps"], ref["desc"], tag)
    assert np.array_equal(kp_bytes(kps[:n]), kp_bytes(ref["kps"])), tag
    assert untouched(kps, desc, n), tag


@pytest.fixture(scope="module")
def ex(oracle_mod):
    return oracle_mod.Extractor()


# ------------------------------------------------------------------ 1. coeb_extract, strided input
def strided_views(case, fill):
    """(view, stride) of the issue's three cases, everything outside the view = fill."""
    fr = synth.make_frames(640, 480, 1, seed=1000 + ord(case))[0]
    if case == "a":                         # odd stride
        return in_parent(fr, 649, fill), 649
    if case == "b":
        return in_parent(fr, 704, fill), 704
    parent = np.full((480, 640), fill, np.uint8)         # c: ROI at (3, 5), misaligned base, stride 640
    parent[5:245, 3:323] = fr[5:245, 3:323]
    return parent[5:245, 3:323], 640


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_extract_strided(ctx, ex, case):
    ref = {}
    for fill in (0, 255):
        view, stride = strided_views(case, fill)
        h, w = view.shape
        assert view.strides == (stride, 1) and (case != "c" or view.ctypes.data % 4 != 0)
        for name, dyn in (("plain", None), ("dyn", synth.dynamic_inputs(w, h))):
            if name not in ref:             # the oracle on the contiguous copy, once per case
                ref[name] = ex.extract(np.ascontiguousarray(view), *(dyn or ()))
                assert len(ref[name]["kps"]) > 100
            rc, n, kps, desc = raw_extract(ctx, view, stride, dyn)
            expect_exact(rc, n, kps, desc, ref[name], "%s %s pad %d" % (case, name, fill))


def test_extract_stride_below_width_rejected(ctx, ex):
    fr = synth.make_frames(640, 480, 1, seed=1000)[0]
    rc, n, kps, desc = raw_extract(ctx, fr, 639)
    assert rc == COEB_EINVAL and n == 0 and untouched(kps, desc, 0)
    rc, n, kps, desc = raw_extract(ctx, fr, 640)        # no sticky state
    expect_exact(rc, n, kps, desc, ex.extract(fr), "after EINVAL")


# ------------------------------------------------------------------ 2. output arrays and cap
@pytest.fixture(scope="module")
def frame31(ex):
    fr = synth.make_frames(640, 480, 1, seed=31)[0]
    ref = ex.extract(fr)
    assert 900 <= len(ref["kps"]) <= 1100              # 1000 for this frame
    return fr, ref


@pytest.mark.parametrize("want_kps,want_desc", [(False, True), (True, False), (False, False)])
def test_extract_null_outputs(ctx, frame31, want_kps, want_desc):
    """One array null: nothing is packed behind the kernels (guess = 0) and the other array comes
    by the second device-to-host round trip."""
    fr, ref = frame31
    n_ref = len(ref["kps"])
    other = synth.make_frames(640, 480, 1, seed=32)[0]      # the staging buffer holds another frame's records
    assert raw_extract(ctx, other, 640)[0] == COEB_OK
    rc, n, kps, desc = raw_extract(ctx, fr, 640, want_kps=want_kps, want_desc=want_desc)
    assert rc == COEB_OK and n == n_ref
    if want_kps:
        assert np.array_equal(kp_bytes(kps[:n]), kp_bytes(ref["kps"]))
    if want_desc:
        assert np.array_equal(desc[:n], ref["desc"])
    assert untouched(kps, desc, n)
    rc, n, kps, desc = raw_extract(ctx, fr, 640)
    expect_exact(rc, n, kps, desc, ref, "after a null-array call")


@pytest.mark.parametrize("short", ["n-1", "1", "0"])
def test_extract_small_cap(ctx, frame31, short):
    """cap < n: COEB_ERANGE, *n_out = n, and the first cap records are still delivered."""
    fr, ref = frame31
    n_ref = len(ref["kps"])
    cap = {"n-1": n_ref - 1, "1": 1, "0": 0}[short]
    rc, n, kps, desc = raw_extract(ctx, fr, 640, cap=cap)
    assert rc == COEB_ERANGE and n == n_ref, (rc, n)
    assert np.array_equal(kp_bytes(kps[:cap]), kp_bytes(ref["kps"][:cap]))
    assert np.array_equal(desc[:cap], ref["desc"][:cap])
    assert untouched(kps, desc, cap)
    rc, n, kps, desc = raw_extract(ctx, fr, 640)
    expect_exact(rc, n, kps, desc, ref, "after ERANGE")


def test_frame_rgbd_and_extract_alternate_on_one_context(frame31):
    """coeb_frame_rgbd and coeb_extract share the page-locked buffer's layout and the enqueue of the
    frame: alternated on one context (with and without boxes / T_M, the one-array second round
    trip, a short cap), each call returns what a fresh context returns for it."""
    W, H = 640, 480
    fr_a, fr_b = synth.make_frames(W, H, 2, seed=77)
    fr_c, ref_c = frame31
    depth = synth.make_depth(W, H)
    cam = cf.make_camera(synth.TUM_FX, synth.TUM_FY, synth.TUM_CX, synth.TUM_CY, synth.TUM_BF, W, H)
    dyn = synth.dynamic_inputs(W, H)
    cap = len(ref_c["kps"]) // 2

    def rgbd(c):
        return c.frame_rgbd(fr_a, depth, cam, dist=(0.2624, -0.9531, -0.0054, 0.0026, 1.1633), boxes=dyn[0], tm=dyn[1],
                            blur=dyn[2])

    calls = [rgbd,
             lambda c: raw_extract(c, fr_b, W, want_kps=False),          # desc_out only: fetched by the second copy
             lambda c: raw_extract(c, fr_c, W, dyn, cap=cap),            # COEB_ERANGE, the first cap records
             rgbd]
    want = []
    for call in calls[:3]:
        c = cf.Context(max_width=W, max_height=H, max_batch=1)
        try:
            want.append(call(c))
        finally:
            c.close()
    want.append(want[0])
    c = cf.Context(max_width=W, max_height=H, max_batch=1)
    try:
        got = [call(c) for call in calls]
    finally:
        c.close()
    for i in (0, 3):
        assert len(got[i]["kps"]) > 100
        for name in ("kps", "kps_un", "desc", "u_right", "depth"):
            a, b = got[i][name], want[i][name]
            if name.startswith("kps"):
                a, b = kp_bytes(a), kp_bytes(b)
            same_bits(a, b, "call %d %s" % (i, name))
    for i in (1, 2):
        (rc, n, kps, desc), (rc_w, n_w, kps_w, desc_w) = got[i], want[i]
        assert (rc, n) == (rc_w, n_w), (i, rc, n, rc_w, n_w)
        assert np.array_equal(kp_bytes(kps), kp_bytes(kps_w)) and np.array_equal(desc, desc_w), i
    rc, n, kps, desc = got[1]
    assert rc == COEB_OK and n > 100 and (kp_bytes(kps) == SENTINEL).all() and (desc[:n] != SENTINEL).any()
    assert (desc[n:] == SENTINEL).all()
    rc, n, kps, desc = got[2]
    assert rc == COEB_ERANGE and n > cap and untouched(kps, desc, cap)
    assert (kp_bytes(kps[:cap]) != SENTINEL).any() and (desc[:cap] != SENTINEL).any()


# ------------------------------------------------------------------ 3. coeb_stereo_from_rgbd
def raw_stereo(ctx, kps, n, depth_view, w, h, dstride):
    ur = np.full(max(n, 1), np.float32(7.5))
    dd = np.full(max(n, 1), np.float32(7.5))
    rc = cf.lib().coeb_stereo_from_rgbd(ctx.h, kps.ctypes.data if kps is not None else None, n,
                                        depth_view.ctypes.data if depth_view is not None else None, w, h, dstride,
                                        C.c_float(synth.TUM_BF), ur.ctypes.data if kps is not None else None,
                                        dd.ctypes.data if kps is not None else None)
    return rc, ur[:n], dd[:n]


def test_stereo_from_rgbd_strided_depth(ctx, oracle_mod, frame31):
    W, H = 640, 480
    _, ref = frame31
    hand = np.zeros(12, KEYPOINT_DTYPE)
    pos = [(0, 0), (W - 1, H - 1), (W - 1, 0), (0, H - 1),                       # the corners
           (0.25, 100.5), (W - 0.25, 100.5), (300.5, 0.25), (300.5, H - 0.25),  # just inside each border
           (W - 1.001, H - 1.001), (0.999, 0.999), (W - 0.5, H - 0.5), (0.5, H - 0.5)]
    hand["x"], hand["y"] = np.float32([p[0] for p in pos]), np.float32([p[1] for p in pos])
    assert (hand["x"] < W).all() and (hand["y"] < H).all()
    kps = np.concatenate([ref["kps"].astype(KEYPOINT_DTYPE), hand])
    rng = np.random.default_rng(3)
    depth = (0.5 + 7 * rng.random((H, W))).astype(np.float32)      # every pixel its own value
    specials = np.float32([0, -1, np.nan, np.inf, 1e-30])
    for i, k in enumerate(kps[::17]):                               # under every 17th keypoint
        depth[int(k["y"]), int(k["x"])] = specials[i % 5]
    for i, k in enumerate(hand[:5]):
        depth[int(k["y"]), int(k["x"])] = specials[i]
    view = in_parent(depth, 647, np.float32(np.nan))
    ur_ref, dep_ref = oracle_mod.stereo_from_rgbd(kps, np.ascontiguousarray(view), synth.TUM_BF)
    # the special depths are met: <= 0 and NaN give (-1, -1), +inf gives uR = x, 1e-30 a huge disparity
    assert (dep_ref == -1).sum() >= len(kps[::17]) // 3 and np.isinf(dep_ref).any() and (dep_ref == specials[4]).any()
    assert not np.isnan(ur_ref).any() and not np.isnan(dep_ref).any()
    rc, ur, dd = raw_stereo(ctx, kps, len(kps), view, W, H, 647)
    assert rc == COEB_OK
    same_bits(ur, ur_ref, "uR")
    same_bits(dd, dep_ref, "depth")
    assert raw_stereo(ctx, None, 0, None, W, H, W)[0] == COEB_OK
    assert raw_stereo(ctx, kps, len(kps), view, W, H, W - 1)[0] == COEB_EINVAL
    rc, ur, dd = raw_stereo(ctx, kps, len(kps), view, W, H, 647)   # no sticky state
    assert rc == COEB_OK
    same_bits(ur, ur_ref, "uR again")
    same_bits(dd, dep_ref, "depth again")


# ------------------------------------------------------------------ 4. flow and frame helpers, strided
CROP_X0, CROP_Y0, CROP_W, CROP_H, CROP_STRIDE = 121, 97, 320, 240, 329


@pytest.fixture(scope="module")
def crop(oracle_mod):
    """A 320x240 crop of moving_object_pair(640, 480, 0) inside (240, 329) parents with garbage
    padding, and the oracle's stages on the contiguous crop: 181 corners, |T_M| = 30."""
    prev, cur, _ = synth.moving_object_pair(640, 480, 0)
    sl = (slice(CROP_Y0, CROP_Y0 + CROP_H), slice(CROP_X0, CROP_X0 + CROP_W))
    p, c = np.ascontiguousarray(prev[sl]), np.ascontiguousarray(cur[sl])
    r = dict(p=p, c=c, pv=in_parent(p, CROP_STRIDE, "garbage"), cv=in_parent(c, CROP_STRIDE, "garbage"))
    r["gf"] = oracle_mod.good_features(p)
    r["sp"] = oracle_mod.corner_subpix(p, r["gf"])
    r["nx"], r["st"] = oracle_mod.lk_pyr(p, c, r["sp"])
    r["tail"] = oracle_mod.moving_tail(p, c, r["sp"], r["nx"], r["st"])
    r["tm"] = oracle_mod.process_moving_object(p, c)
    assert len(r["gf"]) >= 30 and r["tm"] is not None and len(r["tm"]) > 0, (len(r["gf"]), r["tm"])
    return r


def test_good_features_strided(ctx, crop):
    out = np.zeros((1000, 2), np.float32)
    n = C.c_int(0)
    ctx.check(cf.lib().coeb_good_features(ctx.h, crop["pv"].ctypes.data, CROP_W, CROP_H, CROP_STRIDE, 1000, 0.01, 8.0,
                                          0.04, out.ctypes.data, 1000, C.byref(n)))
    same_bits(out[:n.value], crop["gf"], "goodFeaturesToTrack")
    rc = cf.lib().coeb_good_features(ctx.h, crop["pv"].ctypes.data, CROP_W, CROP_H, CROP_W - 1, 1000, 0.01, 8.0, 0.04,
                                     out.ctypes.data, 1000, C.byref(n))
    assert rc == COEB_EINVAL


def test_corner_subpix_strided(ctx, crop):
    xy = crop["gf"].copy()
    ctx.check(cf.lib().coeb_corner_subpix(ctx.h, crop["pv"].ctypes.data, CROP_W, CROP_H, CROP_STRIDE, xy.ctypes.data,
                                          len(xy), 10, 20, 0.03))
    same_bits(xy, crop["sp"], "cornerSubPix")


def test_lk_strided(ctx, crop):
    pts = crop["sp"]
    nx = np.zeros_like(pts)
    st = np.zeros(len(pts), np.uint8)
    ctx.check(cf.lib().coeb_optical_flow_pyr_lk(ctx.h, crop["pv"].ctypes.data, crop["cv"].ctypes.data, CROP_W, CROP_H,
                                                CROP_STRIDE, pts.ctypes.data, len(pts), 22, 5, 20, 0.01,
                                                nx.ctypes.data, st.ctypes.data))
    assert crop["st"].sum() >= 30
    same_bits(st, crop["st"], "LK status")
    same_bits(nx[crop["st"] == 1], crop["nx"][crop["st"] == 1], "LK next")


def test_moving_tail_strided(ctx, crop):
    pts, nx = crop["sp"], crop["nx"]
    st = crop["st"].copy()
    rtm, rst, rF, rnf = crop["tail"]
    tm = np.zeros((len(pts), 2), np.float32)
    F = np.zeros(9, np.float64)
    nt, nf = C.c_int(0), C.c_int(0)
    ctx.check(cf.lib().coeb_moving_tail(ctx.h, crop["pv"].ctypes.data, crop["cv"].ctypes.data, CROP_W, CROP_H,
                                        CROP_STRIDE, pts.ctypes.data, nx.ctypes.data, st.ctypes.data, len(pts),
                                        tm.ctypes.data, len(tm), C.byref(nt), F.ctypes.data, C.byref(nf)))
    assert rF is not None and len(rtm) > 0
    same_bits(st, rst, "state after the SAD check")
    assert nf.value == rnf and nt.value == len(rtm)
    same_bits(F.reshape(3, 3), rF, "F")
    same_bits(tm[:nt.value], rtm, "T_M")


def flow_debug_arrays():
    a = dict(corners_raw=np.zeros((1000, 2), np.float32), corners=np.zeros((1000, 2), np.float32),
             ncorners=np.zeros(1, np.int32), next_pts=np.zeros((1000, 2), np.float32), status=np.zeros(1000, np.uint8),
             state=np.zeros(1000, np.uint8), F=np.zeros(9, np.float64), nf=np.zeros(1, np.int32))
    return a, cf.FlowDebug(**{k: C.c_void_p(v.ctypes.data) for k, v in a.items()})


def check_pmo(crop, tm, nt, a, tag):
    """T_M and the stage outputs of a whole ProcessMovingObject call against the oracle's."""
    assert nt == len(crop["tm"]), (tag, nt)
    same_bits(tm[:nt], crop["tm"], tag + " T_M")
    n = int(a["ncorners"][0])
    assert n == len(crop["gf"]), tag
    same_bits(a["corners_raw"][:n], crop["gf"], tag + " gf")
    same_bits(a["corners"][:n], crop["sp"], tag + " subpix")
    same_bits(a["status"][:n], crop["st"], tag + " LK status")
    ok = crop["st"] == 1
    same_bits(a["next_pts"][:n][ok], crop["nx"][ok], tag + " LK next")
    same_bits(a["state"][:n], crop["tail"][1], tag + " state")
    same_bits(a["F"].reshape(3, 3), crop["tail"][2], tag + " F")
    assert int(a["nf"][0]) == crop["tail"][3], tag


def test_moving_object_points_strided_host_and_device(ctx, crop):
    """coeb_moving_object_points on the strided host views, and coeb_moving_object_points_device
    on frames uploaded with pitch 384 > width: both equal the oracle (hence each other)."""
    L = cf.lib()
    tm = np.zeros((1024, 2), np.float32)
    nt = C.c_int(0)
    a, dbg = flow_debug_arrays()
    ctx.check(L.coeb_moving_object_points(ctx.h, crop["pv"].ctypes.data, crop["cv"].ctypes.data, CROP_W, CROP_H,
                                          CROP_STRIDE, tm.ctypes.data, len(tm), C.byref(nt), C.byref(dbg)))
    check_pmo(crop, tm, nt.value, a, "host")
    host_tm = tm[:nt.value].copy()
    pitch = 384
    dp = ctx.upload(np.ascontiguousarray(in_parent(crop["p"], pitch, "garbage").base))
    dc = ctx.upload(np.ascontiguousarray(in_parent(crop["c"], pitch, "garbage").base))
    try:
        tm2 = np.zeros((1024, 2), np.float32)
        nt2 = C.c_int(0)
        a2, dbg2 = flow_debug_arrays()
        ctx.check(L.coeb_moving_object_points_device(ctx.h, C.c_void_p(dp.ptr), C.c_void_p(dc.ptr), CROP_W, CROP_H, pitch,
                                                     tm2.ctypes.data, len(tm2), C.byref(nt2), C.byref(dbg2)))
        check_pmo(crop, tm2, nt2.value, a2, "device")
        same_bits(tm2[:nt2.value], host_tm, "device vs host")
        rc = L.coeb_moving_object_points_device(ctx.h, C.c_void_p(dp.ptr), C.c_void_p(dc.ptr), CROP_W, CROP_H, CROP_W - 1,
                                                tm2.ctypes.data, len(tm2), C.byref(nt2), None)
        assert rc == COEB_EINVAL
    finally:
        dp.free()
        dc.free()


def test_blur_flags_strided(ctx, oracle_mod, crop):
    """The boxes of test_blur_flags scaled to the 320x240 crop."""
    sm = crop["p"].copy()
    sm[50:150, 100:160] = 90            # flat region -> blurred -> flag 1
    boxes = np.array([[100, 50, 160, 150], [5.25, 10.25, 100.1, 200.35], [315, 235, 320, 240], [0, 0, 1, 1],
                      [-2.5, 0, 5, 5]], np.float32)
    ref, _ = oracle_mod.blur_flags(sm, boxes)
    view = in_parent(sm, CROP_STRIDE, "garbage")
    out = np.full(len(boxes), -7, np.int32)
    ctx.check(cf.lib().coeb_blur_flags(ctx.h, view.ctypes.data, CROP_W, CROP_H, CROP_STRIDE, boxes.ctypes.data,
                                       len(boxes), out.ctypes.data))
    assert np.array_equal(out, ref) and ref[0] == 1, (out, ref)


# ------------------------------------------------------------------ 5. LK at the last inside window
WIN, HALF = 22, np.float32(10.5)


def lk_level_sizes(w, h, max_level=5):
    """The levels calcOpticalFlowPyrLK uses: pyrDown halves until a level is no larger than the window."""
    out = [(w, h)]
    for _ in range(max_level):
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= WIN or h <= WIN:
            break
        out.append((w, h))
    return out


def window_origin(p, level):
    """ipx (or ipy) of the level-`level` window of a level-0 coordinate p: floor(p / 2^L - 10.5),
    in float32 as the kernel and the reference compute it."""
    return np.floor(np.float32(p) * np.float32(1.0 / (1 << level)) - HALF).astype(np.int64)


def edge_points(w, h):
    """Per level and level corner, windows whose origin is the first (0) / last (l - 23) one with
    the whole window and its +1 neighbours inside, at fractional parts 0, 0.25, 0.999 -- and the
    same moved one level pixel outward along x and along y (the reflect path).  Returns
    (points (n, 2) f32, level, wanted (ipx, ipy))."""
    pts, lev, want = [], [], []
    for L, (lw, lh) in enumerate(lk_level_sizes(w, h)):
        for ix, sx in ((0, -1), (lw - WIN - 1, 1)):
            for iy, sy in ((0, -1), (lh - WIN - 1, 1)):
                for frac in (0.0, 0.25, 0.999):
                    for ox, oy in ((0, 0), (sx, 0), (0, sy)):
                        x = np.float32((np.float32(ix + ox + frac) + HALF) * (1 << L))
                        y = np.float32((np.float32(iy + oy + frac) + HALF) * (1 << L))
                        pts.append((x, y))
                        lev.append(L)
                        want.append((ix + ox, iy + oy))
    return np.array(pts, np.float32), np.array(lev), np.array(want, np.int64)


def lk_pair(w, h):
    """A synth pair of any size: a crop of two 640x480 frames (texture everywhere)."""
    fr = synth.make_frames(640, 480, 2, seed=1003)
    x0, y0 = (0, 0) if (w, h) == (640, 480) else (7, 11)
    return np.ascontiguousarray(fr[0][y0:y0 + h, x0:x0 + w]), np.ascontiguousarray(fr[1][y0:y0 + h, x0:x0 + w])


# 321x243: odd level widths; 322x243: even widths whose level sizes are still no multiple of 4;
# 46x46: level 1 is 23x23, one window that is the first and the last inside one; 61x46: odd at
# both levels, the second 31x23
@pytest.mark.parametrize("w,h", [(640, 480), (321, 243), (322, 243), (46, 46), (61, 46)])
def test_lk_last_inside_window(ctx, oracle_mod, w, h):
    """Levels whose byte size is no multiple of 4 (321x243, 322x243, 61x46, 46x46's 23x23 level)
    once lost their last pixels under the bottom right window to the buffer range check."""
    prev, cur = lk_pair(w, h)
    pts, lev, want = edge_points(w, h)
    sizes = lk_level_sizes(w, h)
    assert len(sizes) == {(640, 480): 5, (321, 243): 4, (322, 243): 4, (46, 46): 2, (61, 46): 2}[(w, h)]
    inside = np.zeros(len(pts), bool)
    for i, (p, L, wt) in enumerate(zip(pts, lev, want)):
        got = (window_origin(p[0], L), window_origin(p[1], L))
        assert got == tuple(wt), (p, L, got, wt)               # the intended window is hit
        lw, lh = sizes[L]
        inside[i] = got[0] >= 0 and got[1] >= 0 and got[0] + WIN < lw and got[1] + WIN < lh
    assert inside.sum() * 3 == len(pts)                        # two of three took a step out
    rnx, rst = oracle_mod.lk_pyr(prev, cur, pts)
    assert (rst[inside] == 1).sum() >= 6 and (rst[~inside] == 1).sum() >= 6, (rst[inside].sum(), rst[~inside].sum())
    runs = []
    for before in (255, 0):            # whatever the calls before left in the flow scratch
        flat = np.full((h, w), before, np.uint8)
        cf.CalcOpticalFlowPyrLK(ctx, flat, flat, pts[:4])
        # a same-size call writes the same regions as the call under test; a slightly larger frame
        # lays its levels over the bytes that follow this size's frames and levels
        big = np.full((h + 16, w + 16), before, np.uint8)
        cf.CalcOpticalFlowPyrLK(ctx, big, big, pts[:4])
        nx, st = cf.CalcOpticalFlowPyrLK(ctx, prev, cur, pts)
        same_bits(st, rst, "status after %d" % before)
        same_bits(nx[rst == 1], rnx[rst == 1], "next after %d" % before)
        runs.append((nx, st))
    same_bits(runs[0][1], runs[1][1], "status, 255 vs 0 before")
    same_bits(runs[0][0][rst == 1], runs[1][0][rst == 1], "next, 255 vs 0 before")


# ------------------------------------------------------------------ 6. the adaptive extractor sequence
def test_adaptive_nfeatures_sequence(oracle_mod):
    """Tracking.cc:426-466 steps nFeatures 1000 -> 1500 -> 2000 and back and constructs a new
    ORBextractor each time: a new context per frame, each frame exact against an oracle Extractor
    of that nfeatures, and SearchByProjection between consecutive frames (extracted by different
    contexts) exact too."""
    steps = [1000, 1500, 2000, 2000, 1000]
    fr = synth.make_frames(640, 480, len(steps), seed=606)
    depth = synth.make_depth(640, 480)
    Tc, Tl = synth.motion_pose(), np.eye(4, dtype=np.float32)
    prev_ref, create_s = None, []
    for i, nf in enumerate(steps):
        exo = oracle_mod.Extractor(nf, 1.2, 8, 20, 7)
        t0 = time.perf_counter()
        c = cf.Context(nf, 1.2, 8, 20, 7, max_width=640, max_height=480)
        create_s.append(time.perf_counter() - t0)
        try:
            r = exo.extract(fr[i])
            assert len(r["kps"]) > 0.9 * nf, (nf, len(r["kps"]))
            rc, n, kps, desc = raw_extract(c, fr[i], 640)
            expect_exact(rc, n, kps, desc, r, "frame %d nfeatures %d" % (i, nf))
            if prev_ref is not None:
                last = oracle_mod.mapframe_from_extraction(prev_ref["kps"], prev_ref["desc"], depth, synth.TUM_FX,
                                                           synth.TUM_FY, synth.TUM_CX, synth.TUM_CY, synth.TUM_BF)
                ur, _ = oracle_mod.stereo_from_rgbd(r["kps"], depth, synth.TUM_BF)
                assert match_both(c, oracle_mod, exo, r["kps"], r["desc"], ur, last, Tc, Tl) > 100
            prev_ref = r
        finally:
            c.close()
    print("coeb_create, cold contexts: %s s" % ["%.3f" % t for t in create_s])


# ------------------------------------------------------------------ 7. BatchPipeline.frame() guard
def test_pipeline_frame_without_match_raises():
    from coeb_front.pipeline import BatchPipeline
    bp = BatchPipeline(640, 480, 2)
    try:
        bp.load(synth.make_frames(640, 480, 2, seed=5))
        bp.run(match=False)
        bp.synchronize()
        assert len(bp.frame(0)["kps"]) > 500
        with pytest.raises(ValueError):
            bp.frame(1)
    finally:
        bp.close()


# ------------------------------------------------------------------ 8. call order of the batch entry points
def test_batch_call_order_guards():
    """The call-order checks of the device-batch entry points, on one 320x240 context with
    max_batch = 2: each refusal is a host-side argument check that returns before any launch, and
    asking for results that do not exist yet changes nothing about what the next call may do."""
    from coeb_front.pipeline import BatchPipeline
    F, W, H = 2, 320, 240
    bp = BatchPipeline(W, H, F)
    c = bp.ctx

    def refused(text, fn, *args):
        with pytest.raises(cf.CoebError) as e:
            fn(*args)
        assert text in str(e.value), str(e.value)

    try:
        bp.load(synth.make_frames(W, H, F, seed=77), Tcw=np.stack([np.eye(4, dtype=np.float32), synth.motion_pose()]))
        c.extract_batch_device(bp.gray.ptr, F, W, H)
        assert c.batch_match_results() == (None, None)
        refused("must follow", c.pose_batch_device, bp.cam, F, bp.dTcw.ptr)      # the read above made no match
        refused("no batch pose yet", c.batch_pose_results)
        refused("no batch TrackLocalMap yet", c.batch_track_results)
        refused("no frame batch yet", c.batch_frame_results, F)
        refused("rc=%d" % COEB_EINVAL, c.debug_read, "search_path")
        c.match_batch_device_tcw(bp.depth.ptr, F, W, H, bp.cam, bp.dTcw.ptr)
        m, n = c.batch_match_results()
        assert m and n
        refused("must follow", c.track_local_map_batch_device, bp.cam, F)
        c.pose_batch_device(bp.cam, F, bp.dTcw.ptr)
        assert all(c.batch_pose_results())
        c.track_local_map_batch_device(bp.cam, F)
        refused("already run", c.track_local_map_batch_device, bp.cam, F)
        assert all(c.batch_track_results())
        c.synchronize()
    finally:
        bp.close()


# ------------------------------------------------------------------ 9. the matchers' unstaged forms
GRID_CELLS, LDS_BUDGET, CUR_MAX, N_SECOND = 64 * 48, 160 * 1024, 4095, 64


def match_lds_bytes(n, q, lds_cur):
    """match_lds_bytes of csrc/coeb_match.hip: the LDS of one matcher workgroup with n current
    keypoints and q second-side points, with or without the current frame staged."""
    n4, q4 = (n + 3) & ~3, (q + 3) & ~3
    return (((GRID_CELLS + 1) * 4 + 15) & ~15) + 2 * n4 * 4 + 2 * q4 * 4 + (n4 * (16 + 32) if lds_cur else 0)


def smallest_unstaged_n(q):
    """The fewest current keypoints at which the launchers can no longer stage the frame."""
    n = next(n for n in range(1, CUR_MAX + 1) if match_lds_bytes(n, q, True) + 256 > LDS_BUDGET)
    assert match_lds_bytes(n - 1, q, True) + 256 <= LDS_BUDGET < match_lds_bytes(n, q, True) + 256
    assert match_lds_bytes(n, q, False) + 256 <= LDS_BUDGET and n <= CUR_MAX
    return n


@pytest.fixture(scope="module")
def crowded_frame(oracle_mod):
    """A synthetic current frame with just too many keypoints for the staged matcher forms (by
    shape, the only way k_match_lists<false> + k_match<false>, k_match_local<false> and
    k_match_kf<false> run): keypoints spread over 640x480 with random descriptors, and a second
    side of N_SECOND points that are its first N_SECOND keypoints seen from the identity pose
    with a few descriptor bits flipped."""
    n = smallest_unstaged_n(N_SECOND)
    rng = np.random.default_rng(2693)
    k = np.zeros(n, KEYPOINT_DTYPE)
    k["x"] = rng.uniform(16, 640 - 16, n).astype(np.float32)
    k["y"] = rng.uniform(16, 480 - 16, n).astype(np.float32)
    k["octave"] = rng.integers(0, 8, n)
    k["size"] = (31 * np.float32(1.2) ** k["octave"]).astype(np.float32)
    k["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    k["response"] = rng.uniform(20, 200, n).astype(np.float32)
    k["class_id"] = -1
    d = rng.integers(0, 256, (n, 32)).astype(np.uint8)
    depth = synth.make_depth(640, 480)
    ur, _ = oracle_mod.stereo_from_rgbd(k, depth, synth.TUM_BF)
    d2 = d[:N_SECOND].copy()
    for row in d2:                                       # 6 of 256 bits differ: far below TH_HIGH = 100
        for b in rng.choice(256, 6, replace=False):
            row[b >> 3] ^= np.uint8(1 << (b & 7))
    second = oracle_mod.mapframe_from_extraction(k[:N_SECOND], d2, depth, synth.TUM_FX, synth.TUM_FY, synth.TUM_CX,
                                                 synth.TUM_CY, synth.TUM_BF)
    return k, d, ur, second


def test_match_lastframe_unstaged_form(ctx, oracle_mod, ex, crowded_frame):
    k, d, ur, last = crowded_frame
    nm = match_both(ctx, oracle_mod, ex, k, d, ur, last, synth.motion_pose(), np.eye(4, dtype=np.float32))
    assert nm >= N_SECOND // 2, nm


def test_match_localmap_unstaged_form(ctx, oracle_mod, ex, crowded_frame):
    k, d, ur, last = crowded_frame
    mp = synth.make_local_map(last["xw"], last["mp_desc"], last["keys_un"]["octave"], synth.motion_pose(), 640, 480,
                              seed=1, dup_frac=0.0, n_distract=0)
    assert len(mp["in_view"]) == N_SECOND
    assert localmap_both(ctx, oracle_mod, ex, k, d, ur, None, mp, th=5.0) >= N_SECOND // 4


def test_match_keyframe_unstaged_form(ctx, oracle_mod, ex, crowded_frame):
    k, d, _, last = crowded_frame
    kf = synth.make_keyframe_points(last["xw"], last["mp_desc"], last["keys_un"]["octave"], last["keys_un"]["angle"],
                                    seed=1, n_distract=0)
    assert len(kf["valid"]) == N_SECOND
    assert keyframe_both(ctx, oracle_mod, ex, k, d, None, kf, synth.motion_pose()) >= N_SECOND // 4


def assert_holders_unmatched(m_ref, held, nm):
    """m_ref: the oracle's mvpMapPoints, which the device result equals index for index."""
    assert not np.any((m_ref >= 0) & held), np.nonzero((m_ref >= 0) & held)[0][:8]
    assert nm == int(np.sum(m_ref >= 0)) and nm >= N_SECOND // 8, nm


def test_match_localmap_unstaged_holders(ctx, oracle_mod, ex, crowded_frame):
    """k_match_local<false> with entry holders: the staged form marks them while staging, the
    unstaged form tests cur_obs per candidate.  Half of the true matches are held."""
    k, d, ur, last = crowded_frame
    mp = synth.make_local_map(last["xw"], last["mp_desc"], last["keys_un"]["octave"], synth.motion_pose(), 640, 480,
                              seed=1, dup_frac=0.0, n_distract=0)
    obs = np.random.default_rng(41).choice(np.array([-1, 0, 2], np.int32), len(k))
    obs[:N_SECOND:2] = 2
    nm = localmap_both(ctx, oracle_mod, ex, k, d, ur, obs, mp, th=5.0)
    cam_o = oracle_mod.camera(ex, 640, 480, synth.TUM_FX, synth.TUM_FY, synth.TUM_CX, synth.TUM_CY, synth.TUM_BF)
    _, m_ref = oracle_mod.search_local_map(cam_o, k, d, ur, obs, mp, 5.0, 0.8)
    assert_holders_unmatched(m_ref, obs > 0, nm)


def test_match_keyframe_unstaged_holders(ctx, oracle_mod, ex, crowded_frame):
    """k_match_kf<false> with entry holders (cur_has): half of the true matches and a tenth of
    the other keypoints already hold a MapPoint."""
    k, d, _, last = crowded_frame
    kf = synth.make_keyframe_points(last["xw"], last["mp_desc"], last["keys_un"]["octave"], last["keys_un"]["angle"],
                                    seed=1, n_distract=0)
    has = (np.random.default_rng(43).random(len(k)) < 0.1).astype(np.uint8)
    has[:N_SECOND:2] = 1
    Tcw = synth.motion_pose()
    nm = keyframe_both(ctx, oracle_mod, ex, k, d, has, kf, Tcw)
    cam_o = oracle_mod.camera(ex, 640, 480, synth.TUM_FX, synth.TUM_FY, synth.TUM_CX, synth.TUM_CY, synth.TUM_BF)
    _, m_ref = oracle_mod.search_keyframe(cam_o, k, d, has, kf, Tcw, 10.0, 100, True)
    assert_holders_unmatched(m_ref, has > 0, nm)
