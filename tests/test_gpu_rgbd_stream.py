"""coeb_rgbd_stream_frame: the RGB-D Frame constructor (src/Frame.cc:157-223) on a stream of
frames, one call per frame, the previous frame's state on the device.

Every comparison is bit-exact (floats as their bit patterns): T_M and its count, the blur flags, the
28-byte keypoint records, the descriptors, kp_un, u_right, depth and gray.  The references are
tests/stream_ref.py (the oracle composed frame by frame; its preconditions are asserted by
tests/test_stream_ref.py on the CPU) and the existing calls composed on the same context
(coeb_moving_object_points -> coeb_blur_flags -> coeb_frame_rgbd).  MI355X only."""
import ctypes as C

import numpy as np
import pytest

import coeb_front as cf
from coeb_front import KEYPOINT_DTYPE, synth
import stream_ref as R

pytestmark = pytest.mark.gpu

COEB_OK, COEB_EINVAL, COEB_ERANGE = 0, -22, -34
SENTINEL = 0xA5
FIELDS = ("kps", "kps_un", "desc", "u_right", "depth")


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), -1) if len(a) else np.zeros((0, 0), np.uint8)


def same(got, ref, tag=""):
    """every output of a stream frame against a reference dict, bit for bit"""
    assert got["n_tm"] == ref["n_tm"], (tag, got["n_tm"], ref["n_tm"])
    assert np.array_equal(raw(got["tm"]), raw(ref["tm"])), (tag, "tm")
    assert np.array_equal(got["blur"], ref["blur"]), (tag, got["blur"], ref["blur"])
    assert bool(got["first"]) == bool(ref["first"]), (tag, "first")
    assert len(got["kps"]) == len(ref["kps"]), (tag, len(got["kps"]), len(ref["kps"]))
    for k in FIELDS:
        g = got[k] if got[k] is not None else np.zeros((0, 32), np.uint8)
        assert np.array_equal(raw(g), raw(ref[k])), (tag, k)


def cam_for(w, h):
    fx, fy, cx, cy = R.camera_params(w, h)
    return cf.make_camera(fx, fy, cx, cy, R.BF, w, h)


def scale_of(depth):
    return R.U16_SCALE if depth.dtype == np.uint16 else 1.0


@pytest.fixture(scope="module")
def small_ctx():
    c = cf.Context(*R.SEQUENCES["small"]["orb"], max_width=160, max_height=120)
    yield c
    c.close()


def ctx_of(name, ctx, small_ctx):
    return small_ctx if name == "small" else ctx


def run_sequence(c, name, kind="f32", shadow=True, frames=None):
    s = R.SEQUENCES[name]
    fr, boxes = R.sequence(name)
    depth = R.depth_map(s["w"], s["h"], kind)
    cam = cam_for(s["w"], s["h"])
    st = cf.RGBDStream(c, shadow=shadow)
    try:
        return [st.frame(fr[f], depth, cam, dist=R.TUM1, boxes=boxes[f], depth_scale=scale_of(depth))
                for f in (range(s["n"]) if frames is None else frames)]
    finally:
        st.close()


# ------------------------------------------------------------------ 1. against the oracle composition
@pytest.mark.parametrize("kind", ["f32", "u16"])
@pytest.mark.parametrize("name", ["vga", "odd", "small"])
def test_matches_reference(ctx, small_ctx, oracle_mod, name, kind):
    ref = R.sequence_ref(name, kind)
    got = run_sequence(ctx_of(name, ctx, small_ctx), name, kind)
    fr, _ = R.sequence(name)
    for f, (g, r) in enumerate(zip(got, ref)):
        same(g, r, (name, kind, f))
        assert np.array_equal(g["gray"], fr[f]), f          # a 1-channel image is mImGray itself


# ------------------------------------------------------------------ 2. against the three calls it replaces
def composed(c, prev, cur, boxes, depth, cam):
    """coeb_moving_object_points -> coeb_blur_flags -> coeb_frame_rgbd on context c"""
    if prev is None:
        tm, n_tm, blur = None, 0, np.zeros(len(boxes), np.int32)
    else:
        tm = cf.ProcessMovingObject(c, prev, cur)
        n_tm = -1 if tm is None else len(tm)
        blur = np.full(len(boxes), -7, np.int32)
        b = np.ascontiguousarray(boxes, np.float32)
        cur_c = np.ascontiguousarray(cur)
        c.check(cf.lib().coeb_blur_flags(c.h, cur_c.ctypes.data, cur.shape[1], cur.shape[0], cur.shape[1], b.ctypes.data,
                                         len(b), blur.ctypes.data))
    r = c.frame_rgbd(cur, depth, cam, dist=R.TUM1, boxes=boxes, tm=tm if tm is not None and len(tm) else None, blur=blur,
                     depth_scale=scale_of(depth))
    r.update(tm=np.zeros((0, 2), np.float32) if tm is None else tm, n_tm=n_tm, blur=blur, first=prev is None)
    return r


@pytest.mark.parametrize("name,kind", [("vga", "u16"), ("odd", "f32")])
def test_matches_composed_calls_on_the_same_context(ctx, name, kind):
    """The stream frames alternate with the composed calls on ONE context: equal results, and the
    composed calls (which rewrite the context's flow scratch, stage and extraction buffers between
    two stream frames) leave the stream's state alone."""
    s = R.SEQUENCES[name]
    fr, boxes = R.sequence(name)
    depth = R.depth_map(s["w"], s["h"], kind)
    cam = cam_for(s["w"], s["h"])
    st = cf.RGBDStream(ctx)
    try:
        for f in range(s["n"]):
            got = st.frame(fr[f], depth, cam, dist=R.TUM1, boxes=boxes[f], depth_scale=scale_of(depth))
            ref = composed(ctx, fr[f - 1] if f else None, fr[f], boxes[f], depth, cam)
            same(got, ref, (name, f))
    finally:
        st.close()


# ------------------------------------------------------------------ 3. shadow against no shadow, two streams on one context
def test_shadow_equals_no_shadow_two_streams_alternating(ctx, oracle_mod):
    """Two streams on one context, fed alternately: one with the shadow stream on the "odd"
    sequence, one without on the same sequence one frame behind.  Each equals the reference, so
    they equal each other and neither sees the other's frames."""
    name = "odd"
    s = R.SEQUENCES[name]
    fr, boxes = R.sequence(name)
    ref = R.sequence_ref(name)
    depth = R.depth_map(s["w"], s["h"])
    cam = cam_for(s["w"], s["h"])
    a, b = cf.RGBDStream(ctx, shadow=True), cf.RGBDStream(ctx, shadow=False)
    try:
        for f in range(s["n"] + 1):
            if f < s["n"]:
                same(a.frame(fr[f], depth, cam, dist=R.TUM1, boxes=boxes[f]), ref[f], ("shadow", f))
            if f >= 1:
                same(b.frame(fr[f - 1], depth, cam, dist=R.TUM1, boxes=boxes[f - 1]), ref[f - 1], ("no shadow", f - 1))
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------ 4. colour input, strides, no boxes
@pytest.mark.parametrize("rgb_order", [True, False])
def test_colour_input_matches_preprocess_gray(ctx, oracle_mod, rgb_order):
    """3-channel 333 x 251 frames (a 3-byte pixel pitch meets every alignment at that width): the
    gray level the stream makes is coeb_rgbd_preprocess's, and everything downstream is the
    reference's on those gray frames."""
    s = R.SEQUENCES["odd"]
    fr, boxes = R.sequence("odd")
    depth = R.depth_map(s["w"], s["h"])
    cam = cam_for(s["w"], s["h"])
    col = [np.stack([fr[f], 255 - fr[f] // 2, np.roll(fr[f], 1, axis=1)], axis=2) for f in range(3)]
    gray = [cf.GrabImageRGBD(ctx, c, mbRGB=rgb_order)[0] for c in col]
    assert not np.array_equal(gray[0], cf.GrabImageRGBD(ctx, col[0], mbRGB=not rgb_order)[0])
    st = cf.RGBDStream(ctx)
    try:
        for f in range(3):
            got = st.frame(col[f], depth, cam, dist=R.TUM1, boxes=boxes[f], rgb_order=rgb_order)
            assert np.array_equal(got["gray"], gray[f]), f
            same(got, R.frame_ref(gray[f - 1] if f else None, gray[f], boxes[f], depth), (rgb_order, f))
    finally:
        st.close()


def test_strided_rows_and_no_boxes(ctx, oracle_mod):
    s = R.SEQUENCES["odd"]
    fr, _ = R.sequence("odd")
    w, h = s["w"], s["h"]
    depth = R.depth_map(w, h, "u16")
    wide_d = np.full((h, w + 11), 77, np.uint16)
    wide_d[:, :w] = depth
    cam = cam_for(w, h)
    st = cf.RGBDStream(ctx)
    try:
        for f in range(3):
            wide = np.full((h, w + 13), 200, np.uint8)
            wide[:, :w] = fr[f]
            got = st.frame(wide[:, :w], wide_d[:, :w], cam, dist=R.TUM1, boxes=None, depth_scale=R.U16_SCALE)
            ref = R.frame_ref(fr[f - 1] if f else None, fr[f], None, depth)
            same(got, ref, f)
            assert len(got["blur"]) == 0 and np.array_equal(got["gray"], fr[f])
    finally:
        st.close()


# ------------------------------------------------------------------ 5. the stream's state
def test_reset_in_mid_sequence(ctx, oracle_mod):
    s = R.SEQUENCES["odd"]
    fr, boxes = R.sequence("odd")
    ref = R.sequence_ref("odd")
    depth = R.depth_map(s["w"], s["h"])
    cam = cam_for(s["w"], s["h"])
    st = cf.RGBDStream(ctx)
    try:
        for f in (0, 1):
            same(st.frame(fr[f], depth, cam, dist=R.TUM1, boxes=boxes[f]), ref[f], f)
        st.reset()
        got = st.frame(fr[2], depth, cam, dist=R.TUM1, boxes=boxes[2])
        assert got["first"] and got["n_tm"] == 0 and len(got["tm"]) == 0 and not got["blur"].any()
        same(got, R.frame_ref(None, fr[2], boxes[2], depth), "after reset")
        assert ref[2]["n_tm"] > 0                                   # without the reset it would have had T_M
        same(st.frame(fr[3], depth, cam, dist=R.TUM1, boxes=boxes[3]), ref[3], "pairs with the first frame")
    finally:
        st.close()


def test_flat_pair_gives_minus_one(small_ctx, oracle_mod):
    a, b = R.flat_pair()
    box = np.float32([[10, 10, 60, 60]])
    depth = R.depth_map(a.shape[1], a.shape[0])
    cam = cam_for(a.shape[1], a.shape[0])
    orb = R.SEQUENCES["small"]["orb"]
    st = cf.RGBDStream(small_ctx)
    try:
        st.frame(a, depth, cam, dist=R.TUM1, boxes=box)
        got = st.frame(b, depth, cam, dist=R.TUM1, boxes=box)
        assert got["n_tm"] == -1 and len(got["tm"]) == 0 and list(got["blur"]) == [1]
        same(got, R.frame_ref(a, b, box, depth, orb=orb), "flat")
        plain = small_ctx.frame_rgbd(b, depth, cam, dist=R.TUM1)      # the unmasked extraction
        for k in FIELDS:
            g = got[k] if got[k] is not None else np.zeros((0, 32), np.uint8)
            p = plain[k] if plain[k] is not None else np.zeros((0, 32), np.uint8)
            assert np.array_equal(raw(g), raw(p)), k
        # the stream carries on: a textured frame after the flat one pairs with it
        fr, boxes = R.sequence("small")
        got = st.frame(fr[0], depth, cam, dist=R.TUM1, boxes=boxes[0])
        same(got, R.frame_ref(b, fr[0], boxes[0], depth, orb=orb), "after flat")
    finally:
        st.close()


def raw_frame(st, c, img, depth, cam, boxes, cap=None, null=(), w=None, h=None):
    """coeb_rgbd_stream_frame on sentinel-filled outputs: (rc, out struct, arrays)"""
    hh, ww = img.shape[:2]
    w, h = ww if w is None else w, hh if h is None else h
    full = c.max_keypoints(ww, hh)
    o = dict(kps=np.frombuffer(bytes([SENTINEL]) * (28 * full), KEYPOINT_DTYPE).copy(),
             kps_un=np.frombuffer(bytes([SENTINEL]) * (28 * full), KEYPOINT_DTYPE).copy(),
             desc=np.full((full, 32), SENTINEL, np.uint8), u_right=np.full(full, SENTINEL, np.uint8).repeat(4).view(np.float32),
             depth=np.full(full, SENTINEL, np.uint8).repeat(4).view(np.float32),
             tm=np.full(1024 * 8, SENTINEL, np.uint8).view(np.float32).reshape(1024, 2),
             blur=np.full(16 * 4, SENTINEL, np.uint8).view(np.int32), gray=np.full((hh, ww), SENTINEL, np.uint8))
    p = lambda k: None if k in null else o[k].ctypes.data
    out = cf.RgbdStreamOutC(p("tm"), 1024, -99, p("blur"), p("gray"), ww, p("kps"), p("kps_un"), p("desc"), p("u_right"),
                            p("depth"), full if cap is None else cap, -99, -99)
    d5 = np.asarray(R.TUM1, np.float32)
    b = None if boxes is None else np.ascontiguousarray(boxes, np.float32)
    rc = cf.lib().coeb_rgbd_stream_frame(st.h, img.ctypes.data, img.strides[0], 1, 1, w, h,
                                         None if "map" in null else depth.ctypes.data, depth.strides[0],
                                         cf.DEPTH_F32, C.c_float(1.0), C.byref(cam), d5.ctypes.data,
                                         None if b is None else b.ctypes.data, 0 if b is None else len(b), C.byref(out))
    return rc, out, o


def untouched(out, o):
    return (out.n, out.n_tm, out.first) == (-99, -99, -99) and all((raw(o[k]) == SENTINEL).all() for k in o)


def test_size_change_and_bad_arguments_write_nothing(ctx, oracle_mod):
    s = R.SEQUENCES["odd"]
    fr, boxes = R.sequence("odd")
    ref = R.sequence_ref("odd")
    depth = R.depth_map(s["w"], s["h"])
    cam = cam_for(s["w"], s["h"])
    other, _ = R.sequence("vga")
    st = cf.RGBDStream(ctx)
    try:
        for f in (0, 1):
            st.frame(fr[f], depth, cam, dist=R.TUM1, boxes=boxes[f])
        # another size without a reset
        rc, out, o = raw_frame(st, ctx, np.ascontiguousarray(other[0]), R.depth_map(640, 480), cam_for(640, 480), None)
        assert rc == COEB_EINVAL and untouched(out, o)
        # bad arguments: no depth map, a missing required output, too many boxes, a clipped row
        img = np.ascontiguousarray(fr[2])
        for kw in (dict(null=("map",)), dict(null=("kps",)), dict(null=("desc",)), dict(null=("tm",)), dict(w=s["w"] + 1)):
            rc, out, o = raw_frame(st, ctx, img, depth, cam, boxes[2], **kw)
            assert rc == COEB_EINVAL and untouched(out, o), kw
        rc, out, o = raw_frame(st, ctx, img, depth, cam, np.zeros((17, 4), np.float32))
        assert rc == COEB_EINVAL and untouched(out, o)
        # the next correct frame still pairs with the old predecessor
        same(st.frame(fr[2], depth, cam, dist=R.TUM1, boxes=boxes[2]), ref[2], "after refusals")
        # after a reset any size is taken
        st.reset()
        vb = R.sequence("vga")[1]
        for f in (0, 1):
            got = st.frame(other[f], R.depth_map(640, 480), cam_for(640, 480), dist=R.TUM1, boxes=vb[f])
            same(got, R.sequence_ref("vga")[f], ("other size", f))
    finally:
        st.close()


def test_short_cap_is_erange_with_the_first_records(ctx, oracle_mod):
    s = R.SEQUENCES["odd"]
    fr, boxes = R.sequence("odd")
    ref = R.sequence_ref("odd")
    depth = R.depth_map(s["w"], s["h"])
    cam = cam_for(s["w"], s["h"])
    st = cf.RGBDStream(ctx)
    try:
        st.frame(fr[0], depth, cam, dist=R.TUM1, boxes=boxes[0])
        rc, out, o = raw_frame(st, ctx, np.ascontiguousarray(fr[1]), depth, cam, boxes[1], cap=10)
        assert rc == COEB_ERANGE and out.n == len(ref[1]["kps"]) and out.n_tm == ref[1]["n_tm"] and out.first == 0
        for k in FIELDS:
            assert np.array_equal(raw(o[k])[:10], raw(ref[1][k])[:10]), k
            assert (raw(o[k])[10:] == SENTINEL).all(), k
        assert np.array_equal(raw(o["tm"][:out.n_tm]), raw(ref[1]["tm"]))
        # the frame was taken: the next one pairs with it
        same(st.frame(fr[2], depth, cam, dist=R.TUM1, boxes=boxes[2]), ref[2], "after ERANGE")
    finally:
        st.close()


# ------------------------------------------------------------------ 6. other calls between two stream frames
def test_other_calls_between_frames_leave_the_stream_alone(ctx, oracle_mod):
    """coeb_moving_object_points on other images (it rewrites the context's flow scratch), coeb_extract
    and a 3-frame coeb_frame_batch_device between the stream's frames, for both forms."""
    fr, boxes = R.sequence("vga")
    ref = R.sequence_ref("vga")
    depth = R.depth_map(640, 480)
    cam = cam_for(640, 480)
    noise = synth.make_frames(640, 480, 3, seed=77)
    dbatch = ctx.upload(noise)
    for shadow in (True, False):
        st = cf.RGBDStream(ctx, shadow=shadow)
        try:
            for f in range(4):
                same(st.frame(fr[f], depth, cam, dist=R.TUM1, boxes=boxes[f]), ref[f], (shadow, f))
                cf.ProcessMovingObject(ctx, noise[0], noise[1])
                ctx.extract(noise[2])
                ctx.frame_batch_device(dbatch.ptr, 3, 640, 480)
                ctx.synchronize()
        finally:
            st.close()
    dbatch.free()


# ------------------------------------------------------------------ 7. the launch chain
@pytest.mark.parametrize("shadow", [True, False])
def test_launch_chain_per_call(ctx, shadow):
    """Per call f >= 1: one launch each of the corner kernels, k_sharr, k_lk and k_fm, and one
    k_pyr_down per LK level above 0 -- the pyramid of ONE frame (coeb_moving_object_points builds
    both frames' in as many launches, twice the workgroups)."""
    fr, boxes = R.sequence("vga")
    depth = R.depth_map(640, 480)
    cam = cam_for(640, 480)
    levels = 5                                              # 640 x 480, window 22: 320, 160, 80, 40 above level 0
    st = cf.RGBDStream(ctx, shadow=shadow)
    ctx.profile(True)
    try:
        st.frame(fr[0], depth, cam, dist=R.TUM1, boxes=boxes[0])
        st.frame(fr[1], depth, cam, dist=R.TUM1, boxes=boxes[1])
        # from here every call has a predecessor before it and the corner work of one frame in it
        # or behind it; count two calls and halve
        ctx.synchronize()
        ctx.profile_reset()
        for f in (2, 3):
            st.frame(fr[f], depth, cam, dist=R.TUM1, boxes=boxes[f])
        st.close()                                          # joins the shadow work
        st = None
        prof = ctx.profile_read()
        for k in ("k_gf_response", "k_gf_candidates", "k_gf_select", "k_subpix", "k_sharr", "k_lk", "k_fm", "k_blur_flags",
                  "k_frame_tail"):
            assert prof[k][1] == 2, (k, prof.get(k))
        assert prof["k_pyr_down"][1] == 2 * (levels - 1), prof["k_pyr_down"]
        assert "k_rgbd" not in prof
    finally:
        ctx.profile(False)
        if st is not None:
            st.close()
