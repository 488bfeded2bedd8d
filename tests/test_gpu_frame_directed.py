"""k_dynmask and masked_out, k_blur_flags, k_rgbd / k_rgbd_batch / k_rgbd_batch16 and
undistort_point on the directed cases of tests/frame_ref.py, against the independent model
(MI355X only).

tests/test_frame_ref.py (no GPU) asserts that every case reaches the branch it is named after and
that the oracle agrees with the model.  Here the device's mask rectangles (debug_read("dyn")) are
rasterised and compared with the model's mask pixel for pixel, the masked extraction must be the
model's filter of the device's own unmasked one (single frame, coeb_frame_rgbd and a batch of
three), and the blur flags, gray bytes, depth floats and undistorted points must be the model's --
the last under the tie rule of frame_ref.check_rounded."""
import ctypes as C

import numpy as np
import pytest

import coeb_front as cf
import frame_ref as R
from coeb_front import synth

pytestmark = pytest.mark.gpu

F32 = np.float32
DYN = {c.name: c for c in R.dyn_cases()}
BLUR = {c.name: c for c in R.blur_cases()}
W, H = 640, 480
SENT = 0xA5


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


def check_device_dyn(c, d, tag, f=0):
    flag, nrect, rects = R.device_dyn(c.debug_read("dyn", f))
    assert flag == d.area_flag, (tag, flag, float(d.area))
    assert nrect == len(d.rects) and rects[:nrect] == d.rects, (tag, nrect, rects[:nrect], d.rects)
    assert np.array_equal(R.rasterise(rects, nrect), d.mask), tag


# ------------------------------------------------------------------ the decision
@pytest.mark.parametrize("name", sorted(DYN))
def test_dyn_decision(ctx, name):
    c = DYN[name]
    d = R.dyn_decide(c.boxes, c.tm, c.blur)
    R.check_dyn_want(c, d)
    k, _ = ctx.extract(np.full((H, W), 128, np.uint8), c.boxes, c.tm, c.blur)
    assert len(k) == 0
    check_device_dyn(ctx, d, name)


# ------------------------------------------------------------------ the cull
@pytest.fixture(scope="module")
def textured(oracle_mod):
    fr = synth.make_frames(W, H, 3, seed=1234)
    ex = oracle_mod.Extractor()
    return fr, [ex.extract(fr[f]) for f in (0, 2)]


def cull_inputs(plain_kps):
    boxes, tm, blur = R.cull_boxes(plain_kps)
    cls = R.cull_classes(plain_kps, boxes)
    assert (cls >= 3).all(), cls.tolist()                    # on the unmasked oracle output
    d = R.dyn_decide(boxes, tm, blur)
    assert all(d.mark) and d.area_flag == 0 and len(d.rects) == 16
    return boxes, tm, blur, d


def test_cull_boundaries_single_frame(ctx, textured):
    fr, plain = textured
    boxes, tm, blur, d = cull_inputs(plain[0]["kps"])
    k0, d0 = ctx.extract(fr[0])
    k0, d0 = k0.copy(), d0.copy()
    keep = R.keep_of(d.mask, k0)
    assert len(k0) - len(keep) >= 50
    k, dd = ctx.extract(fr[0], boxes, tm, blur)
    assert np.array_equal(raw(k), raw(k0[keep])) and np.array_equal(dd, d0[keep])
    check_device_dyn(ctx, d, "cull")
    # the same through the fused Frame constructor
    cam = cf.make_camera(*R.TUM1_K, synth.TUM_BF, W, H)
    depth = (1 + 0.001 * np.arange(W)[None, :] + 0.0007 * np.arange(H)[:, None]).astype(F32)
    dist = R.DIST["tum1"][1]
    r0 = {k_: (None if v is None else v.copy()) for k_, v in ctx.frame_rgbd(fr[0], depth, cam, dist).items()}
    assert np.array_equal(raw(r0["kps"]), raw(k0))
    r = ctx.frame_rgbd(fr[0], depth, cam, dist, boxes, tm, blur)
    for key in ("kps", "kps_un", "desc", "u_right", "depth"):
        assert np.array_equal(raw(r[key]), raw(r0[key][keep])), key
    check_device_dyn(ctx, d, "cull frame_rgbd")


def test_cull_boundaries_batch_with_an_empty_frame(textured):
    """coeb_extract_batch_device takes per-frame boxes and T_M from the host: F = 3, the middle
    frame without any."""
    from coeb_front.pipeline import BatchPipeline
    fr, plain = textured
    dyn = [cull_inputs(plain[0]["kps"]), None, cull_inputs(plain[1]["kps"])]
    bp = BatchPipeline(W, H, 3)
    try:
        bp.load(fr)
        bp.run(match=False)
        bp.synchronize()
        base, _, _ = bp.results()
        bp.load(fr, dyn=[(None, None, None) if v is None else v[:3] for v in dyn])
        bp.run(match=False)
        bp.synchronize()
        out, _, _ = bp.results()
        for f in range(3):
            if dyn[f] is None:
                d = R.dyn_decide(np.zeros((0, 4)), np.zeros((0, 2)), [])
            else:
                d = dyn[f][3]
            keep = R.keep_of(d.mask, base[f][0])
            assert (len(keep) == len(base[f][0])) == (dyn[f] is None)
            assert np.array_equal(raw(out[f][0]), raw(base[f][0][keep])), f
            assert np.array_equal(out[f][1], base[f][1][keep]), f
            check_device_dyn(bp.ctx, d, "batch frame %d" % f, f)
    finally:
        bp.close()


# ------------------------------------------------------------------ blur flags
def test_blur_flags(ctx):
    """The flag of every case is the model's, on host rows 5 bytes further apart than the image is
    wide (the padding holds 0, the surround 255).  The cases at the rational 4.2 are described in
    test_frame_ref.test_blur_scenarios_reach_their_branches."""
    for c in BLUR.values():
        h, w = c.gray.shape
        buf = np.zeros((h, w + 5), np.uint8)
        buf[:, :w] = c.gray
        flag = R.blur_flag(c.gray, c.box)[0]
        assert flag == c.want_flag
        out = np.full(1, -7, np.int32)
        box = np.ascontiguousarray(c.box, F32)
        ctx.check(cf.lib().coeb_blur_flags(ctx.h, buf.ctypes.data, w, h, w + 5, box.ctypes.data, 1, out.ctypes.data))
        assert int(out[0]) == flag, (c.name, int(out[0]), R.blur_flag(c.gray, c.box))
    # all the 32 x 24 cases of one image size in one call: one workgroup per box
    same = [c for c in BLUR.values() if c.gray.shape == (24, 32) and c.name.startswith("corner")]
    assert len(same) == 4 and all(np.array_equal(c.gray[c.gray != 255], same[0].gray[same[0].gray != 255]) for c in same)
    img = np.minimum.reduce([c.gray for c in same])
    boxes = np.ascontiguousarray(np.stack([c.box for c in same]), F32)
    out = np.full(4, -7, np.int32)
    ctx.check(cf.lib().coeb_blur_flags(ctx.h, img.ctypes.data, 32, 24, 32, boxes.ctypes.data, 4, out.ctypes.data))
    assert out.tolist() == [R.blur_flag(img, b)[0] for b in boxes] == [1, 1, 1, 1]


# ------------------------------------------------------------------ conversions
@pytest.mark.parametrize("w,h", R.SINGLE_SIZES)
def test_rgbd_preprocess_single(ctx, w, h):
    L = cf.lib()
    for ch in (1, 3, 4):
        img = R.image_for(w, h, ch, w * h + ch)
        stride = ch * w + 5
        buf = np.full((h, stride), SENT, np.uint8)
        buf[:, :ch * w] = img.reshape(h, ch * w)
        for order in (1, 0):
            gray = np.full((h, w), SENT, np.uint8)
            ctx.check(L.coeb_rgbd_preprocess(ctx.h, buf.ctypes.data, stride, ch, order, None, 0, 0, C.c_float(1.0), w, h,
                                             gray.ctypes.data, None))
            assert np.array_equal(gray, R.to_gray(img, order)), (ch, order)
    for dt, code, nb in ((np.uint16, cf.DEPTH_U16, 2), (np.float32, cf.DEPTH_F32, 4)):
        dep = R.depth_for(w, h, dt, w + h)
        stride = nb * (w + 3)
        buf = np.full((h, stride), SENT, np.uint8)
        buf[:, :nb * w] = dep.view(np.uint8).reshape(h, nb * w)
        for f in R.DEPTH_FACTORS:
            out = np.full((h, w), -7, F32)
            ctx.check(L.coeb_rgbd_preprocess(ctx.h, None, 0, 1, 1, buf.ctypes.data, stride, code, C.c_float(f), w, h,
                                             None, out.ctypes.data))
            assert np.array_equal(out.view(np.uint32), R.depth_to_float(dep, f).view(np.uint32)), (dt, f)
    # image and depth in one call
    img, dep = R.image_for(w, h, 3, 5), R.depth_for(w, h, np.uint16, 6)
    gray, out = np.zeros((h, w), np.uint8), np.zeros((h, w), F32)
    ctx.check(L.coeb_rgbd_preprocess(ctx.h, img.ctypes.data, 3 * w, 3, 0, dep.ctypes.data, 2 * w, cf.DEPTH_U16,
                                     C.c_float(1 / 5000.0), w, h, gray.ctypes.data, out.ctypes.data))
    assert np.array_equal(gray, R.to_gray(img, 0)) and np.array_equal(out, R.depth_to_float(dep, 1 / 5000.0))


def run_batch(ctx, img, order, dep, fac, F, w, h, img_off=0, gray_off=0):
    """coeb_rgbd_preprocess_batch_device on fresh device buffers, the image read from and the gray
    written to base + offset; outputs pre-filled with SENT.  Returns (gray bytes, depth bytes) of
    the whole output buffers."""
    npix = w * h
    slack = 256
    bufs = []
    pi = pg = pd = po = 0
    ch = 1
    if img is not None:
        ch = 1 if img.ndim == 3 else img.shape[3]
        di = ctx.alloc(img.nbytes + slack)
        di.write(img, img_off)
        dg = ctx.upload(np.full(F * npix + slack, SENT, np.uint8))
        bufs += [di, dg]
        pi, pg = di.ptr + img_off, dg.ptr + gray_off
    dt = cf.DEPTH_U16
    if dep is not None:
        dt = cf.DEPTH_U16 if dep.dtype == np.uint16 else cf.DEPTH_F32
        dd = ctx.upload(dep)
        do = ctx.upload(np.full(4 * F * npix + slack, SENT, np.uint8))
        bufs += [dd, do]
        pd, po = dd.ptr, do.ptr
    try:
        ctx.rgbd_preprocess_batch_device(pi, ch, order, pd, dt, float(F32(fac)), F, w, h, pg, po)
        ctx.synchronize()
        return (bufs[1].read() if img is not None else None), (bufs[-1].read() if dep is not None else None)
    finally:
        for b in bufs:
            b.free()


def check_batch(ctx, w, h, ch, order, dt, fac, img_off=0, gray_off=0, F=3):
    npix = w * h
    img = None if ch == 0 else np.stack([R.image_for(w, h, ch, 100 * f + ch) for f in range(F)])
    dep = None if dt is None else np.stack([R.depth_for(w, h, dt, 7 * f + 1) for f in range(F)])
    g, d = run_batch(ctx, img, order, dep, fac, F, w, h, img_off, gray_off)
    tag = (w, h, ch, order, dt, fac, img_off, gray_off)
    if img is not None:
        want = np.stack([R.to_gray(img[f], order) for f in range(F)]).reshape(-1)
        assert np.array_equal(g[gray_off:gray_off + F * npix], want), tag
        assert (g[:gray_off] == SENT).all() and (g[gray_off + F * npix:] == SENT).all(), tag
    if dep is not None:
        want = np.stack([R.depth_to_float(dep[f], fac) for f in range(F)]).reshape(-1)
        assert np.array_equal(d[:4 * F * npix].view(np.uint32), want.view(np.uint32)), tag
        assert (d[4 * F * npix:] == SENT).all(), tag


@pytest.mark.parametrize("w,h", R.BATCH_SIZES)
def test_rgbd_preprocess_batch(ctx, w, h):
    """Every channel instance with 16U depth, depth alone (16U scaled, 32F scaled and passed
    through), image alone; W x H puts the frame on one lane (4 x 4), one whole 4096-pixel block,
    a second block of 64 lanes (68 x 64) or 16 lanes (64 x 65), or off the 16-pixel kernel
    altogether (4 x 1, 12 x 3)."""
    for ch, order in ((1, 1), (3, 1), (3, 0), (4, 1), (4, 0)):
        check_batch(ctx, w, h, ch, order, np.uint16, 1 / 5000.0)
    check_batch(ctx, w, h, 0, 1, np.uint16, 1 / 5000.0)
    check_batch(ctx, w, h, 0, 1, np.float32, 0.5)
    check_batch(ctx, w, h, 0, 1, np.float32, 1.0)
    check_batch(ctx, w, h, 3, 1, None, 1.0)
    check_batch(ctx, w, h, 4, 0, np.float32, R.DEPTH_FACTORS[5])


def test_rgbd_preprocess_batch_pointer_offsets(ctx):
    """64 x 64 would take the 16-pixel kernel: an image or gray pointer 4 bytes off a 16-byte
    boundary sends it to the 4-pixel one, 16 bytes off leaves it there."""
    for ch in (1, 3, 4):
        for img_off, gray_off in ((4, 0), (0, 4), (4, 4), (16, 16), (12, 8)):
            check_batch(ctx, 64, 64, ch, 1, np.uint16, 1 / 5000.0, img_off, gray_off)
            check_batch(ctx, 68, 64, ch, 0, None, 1.0, img_off, gray_off)


# ------------------------------------------------------------------ undistortion
@pytest.mark.parametrize("name", sorted(R.DIST))
def test_undistort(ctx, name):
    K, dist = R.DIST[name]
    cam = cf.make_camera(*K, synth.TUM_BF, W, H)
    for n in (1, 255, 256, 257):
        kps = R.undistort_records(n, K[2], K[3])
        out = cf.UndistortKeyPoints(ctx, kps, cam, dist)
        R.check_undistorted(out, kps, K, dist, (name, n))
