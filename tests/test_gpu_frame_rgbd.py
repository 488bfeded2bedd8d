"""coeb_frame_rgbd: the RGB-D Frame constructor's tail (src/Frame.cc:214-223) in one call.

The reference of every comparison is the oracle composition: O.extract, O.undistort_keypoints,
then the depth looked up at the RAW keypoint and uRight = kps_un.x - bf / d in float32
(Frame.cc:829-839).  Every comparison is bit-exact (floats as their bit patterns).  Each case is
one 640x480 frame.  The calls that need it go through coeb_front.lib() with ctypes, since the
Python wrapper hides the arguments under test (MI355X only)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import coeb_front as cf
from coeb_front import KEYPOINT_DTYPE, synth
from test_gpu_capi_edges import (COEB_EINVAL, COEB_ERANGE, COEB_OK, SENTINEL, bits, in_parent, kp_bytes, raw_extract,
                                 raw_stereo, same_bits)
from conftest import ROOT

pytestmark = pytest.mark.gpu

W, H = 640, 480
# TUM1 (freiburg1) calibration: the intrinsics of tests/test_gpu_parity.py::test_undistort_keypoints
FX, FY, CX, CY = 517.306408, 516.469215, 318.643040, 255.313989
TUM1 = (0.262383, -0.953104, -0.005358, 0.002628, 1.163314)
BF = synth.TUM_BF


def compose(kps, kps_un, depth):
    """ComputeStereoFromRGBD as Frame.cc:829-839 writes it: d at the raw keypoint, uRight from
    the undistorted x, IEEE float32 division and subtraction."""
    d = np.ascontiguousarray(depth, np.float32)[kps["y"].astype(np.int32), kps["x"].astype(np.int32)]
    with np.errstate(all="ignore"):
        pos = d > 0                                             # false for NaN
        ur = np.where(pos, kps_un["x"] - np.float32(BF) / d, np.float32(-1)).astype(np.float32)
    return ur, np.where(pos, d, np.float32(-1)).astype(np.float32)


def sentinel_outputs(full):
    return dict(kps=np.frombuffer(bytes([SENTINEL]) * (28 * full), KEYPOINT_DTYPE).copy(),
                kps_un=np.frombuffer(bytes([SENTINEL]) * (28 * full), KEYPOINT_DTYPE).copy(),
                desc=np.full((full, 32), SENTINEL, np.uint8),
                u_right=np.frombuffer(bytes([SENTINEL]) * (4 * full), np.float32).copy(),
                depth=np.frombuffer(bytes([SENTINEL]) * (4 * full), np.float32).copy())


def out_bytes(o, name):
    a = o[name]
    return kp_bytes(a) if a.dtype == KEYPOINT_DTYPE else np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)


def untouched(o, first, names=("kps", "kps_un", "desc", "u_right", "depth")):
    return all(bool((out_bytes(o, k)[first:] == SENTINEL).all()) for k in names)


def raw_frame(ctx, gray, stride, depth, dstride, cam, dist=None, dyn=None, cap=None, scale=1.0, w=W, h=H, dtype=None,
              null=(), n_ptr=True):
    """coeb_frame_rgbd on the arrays' own memory: (rc, n, outputs), the outputs pre-filled with
    SENTINEL over the context's whole capacity.  null: names of output arrays passed as NULL."""
    full = ctx.max_keypoints(W, H)
    o = sentinel_outputs(full)
    boxes, tm, blur = dyn if dyn is not None else (None, None, None)
    d5 = None if dist is None else np.asarray(dist, np.float32)
    if dtype is None:
        dtype = cf.DEPTH_U16 if depth is not None and depth.dtype == np.uint16 else cf.DEPTH_F32
    n = C.c_int(-1)
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = cf.lib().coeb_frame_rgbd(ctx.h, ptr(gray), w, h, stride, ptr(depth), dstride, dtype, C.c_float(scale),
                                  C.byref(cam) if cam is not None else None, ptr(d5),
                                  ptr(boxes), 0 if boxes is None else len(boxes), ptr(tm), 0 if tm is None else len(tm),
                                  ptr(blur), 0 if blur is None else len(blur),
                                  *[None if k in null else o[k].ctypes.data for k in ("kps", "kps_un", "desc", "u_right", "depth")],
                                  full if cap is None else cap, C.byref(n) if n_ptr else None)
    return rc, n.value, o


def expect(o, n, ref, m=None, tag="", skip=()):
    """The first m (default n) entries of all five outputs equal the reference dict's, the rest
    still hold the sentinel."""
    m = n if m is None else m
    for k in ("kps", "kps_un", "desc", "u_right", "depth"):
        if k in skip:
            assert untouched(o, 0, (k,)), (tag, k)
            continue
        assert np.array_equal(out_bytes(o, k)[:m], out_bytes(ref, k)[:m]), (tag, k)
        assert untouched(o, m, (k,)), (tag, k)


@pytest.fixture(scope="module")
def ex(oracle_mod):
    return oracle_mod.Extractor()


@pytest.fixture(scope="module")
def cam():
    return cf.make_camera(FX, FY, CX, CY, BF, W, H)


def make_depth_map():
    """Every pixel its own value, with one hole of each class the reference's `d > 0` rejects."""
    yy, xx = np.mgrid[0:H, 0:W]
    depth = (1 + 0.001 * xx + 0.0007 * yy).astype(np.float32)
    depth[40:200, 30:250] = 0
    depth[220:330, 330:520] = -1.5
    depth[300:420, 40:200] = np.nan
    return depth


@pytest.fixture(scope="module")
def case1(oracle_mod, ex):
    """Frame 31 with the TUM1 calibration and the holed depth map: the oracle composition, and
    the preconditions that make the case mean something, on the oracle's output alone."""
    fr = synth.make_frames(W, H, 1, seed=31)[0]
    r = ex.extract(fr)
    kps = r["kps"].astype(KEYPOINT_DTYPE)
    kun = oracle_mod.undistort_keypoints(kps, FX, FY, CX, CY, TUM1)
    depth = make_depth_map()
    ur, dep = compose(kps, kun, depth)
    d_raw = depth[kps["y"].astype(np.int32), kps["x"].astype(np.int32)]
    moved = (np.trunc(kun["x"]) != np.trunc(kps["x"])) | (np.trunc(kun["y"]) != np.trunc(kps["y"]))
    assert moved.sum() >= 100, moved.sum()
    assert (d_raw == 0).sum() >= 30 and (d_raw < 0).sum() >= 30 and np.isnan(d_raw).sum() >= 30, \
        ((d_raw == 0).sum(), (d_raw < 0).sum(), np.isnan(d_raw).sum())
    assert (dep > 0).sum() >= 500 and ((dep == -1) == ~(d_raw > 0)).all()
    assert not np.isnan(ur).any() and ((ur == -1) == (dep == -1)).all()
    return dict(fr=fr, kps=kps, kps_un=kun, desc=r["desc"], u_right=ur, depth=dep, map=depth)


# ------------------------------------------------------------------ 1. parity with a distorted calibration
def test_parity_distorted_calibration(ctx, oracle_mod, cam, case1):
    ref = case1
    got = ctx.frame_rgbd(ref["fr"], ref["map"], cam, dist=TUM1)
    n = len(ref["kps"])
    assert len(got["kps"]) == n
    for k in ("kps", "kps_un", "desc", "u_right", "depth"):
        assert np.array_equal(out_bytes(got, k), out_bytes(ref, k)), k
    # what no sequence of the older calls gives: coeb_stereo_from_rgbd takes ONE keypoint array.
    # With the raw keys its x term is the raw x ...
    rc, ur_raw, dep_raw = raw_stereo(ctx, ref["kps"], n, ref["map"], W, H, W)
    assert rc == COEB_OK
    same_bits(dep_raw, ref["depth"], "depth on the raw keys")
    assert (bits(ur_raw) != bits(got["u_right"])).sum() >= 100
    # ... and with the undistorted keys the lookup pixel is the undistorted one.  Only keys whose
    # undistorted position is still inside the image are handed over (the call reads the map there).
    kun = ref["kps_un"]
    inside = (kun["x"] >= 0) & (kun["x"] < W) & (kun["y"] >= 0) & (kun["y"] < H)
    assert inside.sum() >= 500
    sub = np.ascontiguousarray(kun[inside])
    ur_o, dep_o = oracle_mod.stereo_from_rgbd(sub, ref["map"], BF)
    assert (bits(ur_o) != bits(ref["u_right"][inside])).sum() >= 50 and (bits(dep_o) != bits(ref["depth"][inside])).sum() >= 50
    rc, ur_un, dep_un = raw_stereo(ctx, sub, len(sub), ref["map"], W, H, W)
    assert rc == COEB_OK
    same_bits(ur_un, ur_o, "uR on the undistorted keys")
    assert (bits(ur_un) != bits(got["u_right"][inside])).sum() >= 50
    assert (bits(dep_un) != bits(got["depth"][inside])).sum() >= 50


# ------------------------------------------------------------------ 2. equivalences
@pytest.mark.parametrize("dist", [None, (0.0, 0.5, 0.1, 0.1, 0.1)])
def test_no_distortion_equals_separate_calls(ctx, oracle_mod, cam, case1, dist):
    """dist NULL, or dist[0] == 0 with the other coefficients set (Frame.cc:581-585): mvKeysUn is
    a copy, and the call equals coeb_extract followed by coeb_stereo_from_rgbd."""
    fr, depth = case1["fr"], case1["map"]
    rc, n, o = raw_frame(ctx, fr, W, depth, 4 * W, cam, dist)
    assert rc == COEB_OK and n == len(case1["kps"])
    rc, n2, kps, desc = raw_extract(ctx, fr, W)
    assert rc == COEB_OK and n2 == n
    assert np.array_equal(kp_bytes(o["kps"][:n]), kp_bytes(kps[:n])) and np.array_equal(o["desc"][:n], desc[:n])
    assert np.array_equal(kp_bytes(o["kps_un"][:n]), kp_bytes(o["kps"][:n]))
    rc, ur, dep = raw_stereo(ctx, kps, n, depth, W, H, W)
    assert rc == COEB_OK
    same_bits(o["u_right"][:n], ur, "uR")
    same_bits(o["depth"][:n], dep, "depth")
    ur_o, dep_o = oracle_mod.stereo_from_rgbd(case1["kps"], depth, BF)    # and the reference's own form agrees
    same_bits(ur, ur_o, "oracle uR")
    same_bits(compose(case1["kps"], case1["kps"], depth)[0], ur_o, "composition vs oracle")
    assert untouched(o, n)


def test_depth_types_and_scale(ctx, oracle_mod, cam, case1):
    """16U depth converted under the keypoints only equals a 32F map converted beforehand
    (Tracking.cc:227), a 32F map with scale 1 is read unchanged, and one with another scale is
    multiplied."""
    fr = case1["fr"]
    rng = np.random.default_rng(5)
    d16 = rng.integers(0, 65536, (H, W)).astype(np.uint16)
    d16[100:200, 100:300] = 0
    scale = np.float32(1.0 / 5000.0)
    pre = oracle_mod.depth_to_float(d16, scale)
    ur, dep = compose(case1["kps"], case1["kps_un"], pre)
    ref = dict(case1, u_right=ur, depth=dep)
    assert (dep == -1).sum() >= 10 and (dep > 0).sum() >= 500
    rc, n, o = raw_frame(ctx, fr, W, d16, 2 * W, cam, TUM1, scale=scale)
    assert rc == COEB_OK
    expect(o, n, ref, tag="16U")
    rc, n, o = raw_frame(ctx, fr, W, pre, 4 * W, cam, TUM1, scale=1.0)
    assert rc == COEB_OK
    expect(o, n, ref, tag="32F pre-converted")
    # pass-through: the depth values come back as the map holds them
    m = case1["map"]
    rc, n, o = raw_frame(ctx, fr, W, m, 4 * W, cam, TUM1, scale=1.0)
    assert rc == COEB_OK
    expect(o, n, case1, tag="32F scale 1")
    d_raw = m[case1["kps"]["y"].astype(np.int32), case1["kps"]["x"].astype(np.int32)]
    pos = d_raw > 0
    same_bits(o["depth"][:n][pos], d_raw[pos], "pass-through")
    # a 32F map with a scale that is not 1 is converted: float product per value
    half = oracle_mod.depth_to_float(m, 0.5)
    ur, dep = compose(case1["kps"], case1["kps_un"], half)
    rc, n, o = raw_frame(ctx, fr, W, m, 4 * W, cam, TUM1, scale=0.5)
    assert rc == COEB_OK
    expect(o, n, dict(case1, u_right=ur, depth=dep), tag="32F scale 0.5")


# ------------------------------------------------------------------ 3. edges
@pytest.mark.parametrize("fill", [0, 255])
def test_strided_gray_and_depth(ctx, cam, case1, fill):
    gray = in_parent(case1["fr"], 649, fill)
    depth = in_parent(case1["map"], 647, np.float32(np.nan) if fill else np.float32(9.0))
    rc, n, o = raw_frame(ctx, gray, 649, depth, 4 * 647, cam, TUM1)
    assert rc == COEB_OK
    expect(o, n, case1, tag="strided, pad %d" % fill)
    d16 = (np.clip(np.nan_to_num(case1["map"], nan=0.0), 0, 60) * 1000).astype(np.uint16)    # the holes read 0
    ur, dep = compose(case1["kps"], case1["kps_un"], d16.astype(np.float32) * np.float32(0.001))
    rc, n, o = raw_frame(ctx, gray, 649, in_parent(d16, 645, 0xFFFF if fill else 0), 2 * 645, cam, TUM1,
                         scale=np.float32(0.001))
    assert rc == COEB_OK
    expect(o, n, dict(case1, u_right=ur, depth=dep), tag="strided 16U, pad %d" % fill)


def test_boxes_tm_blur(ctx, oracle_mod, ex, cam, case1):
    """The dynamic-object mask inputs: the masked keypoint set is O.extract's with the same arguments."""
    dyn = synth.dynamic_inputs(W, H)
    r = ex.extract(case1["fr"], *dyn)
    kps = r["kps"].astype(KEYPOINT_DTYPE)
    assert 100 < len(kps) and kps.tobytes() != case1["kps"].tobytes()
    kun = oracle_mod.undistort_keypoints(kps, FX, FY, CX, CY, TUM1)
    ur, dep = compose(kps, kun, case1["map"])
    rc, n, o = raw_frame(ctx, case1["fr"], W, case1["map"], 4 * W, cam, TUM1, dyn=dyn)
    assert rc == COEB_OK and n == len(kps)
    expect(o, n, dict(kps=kps, kps_un=kun, desc=r["desc"], u_right=ur, depth=dep), tag="dyn")
    got = ctx.frame_rgbd(case1["fr"], case1["map"], cam, dist=TUM1, boxes=dyn[0], tm=dyn[1], blur=dyn[2])
    assert np.array_equal(kp_bytes(got["kps_un"]), kp_bytes(kun)) and np.array_equal(bits(got["u_right"]), bits(ur))


@pytest.mark.parametrize("short", ["n-1", "1", "0"])
def test_small_cap(ctx, cam, case1, short):
    """cap < n: COEB_ERANGE, *n_out = n, the first cap entries of all five outputs delivered."""
    n_ref = len(case1["kps"])
    cap = {"n-1": n_ref - 1, "1": 1, "0": 0}[short]
    rc, n, o = raw_frame(ctx, case1["fr"], W, case1["map"], 4 * W, cam, TUM1, cap=cap)
    assert rc == COEB_ERANGE and n == n_ref, (rc, n)
    expect(o, n, case1, m=cap, tag="cap %d" % cap)
    rc, n, o = raw_frame(ctx, case1["fr"], W, case1["map"], 4 * W, cam, TUM1)
    assert rc == COEB_OK
    expect(o, n, case1, tag="after ERANGE")


def test_null_kp_un_and_empty_image(ctx, cam, case1):
    rc, n, o = raw_frame(ctx, case1["fr"], W, case1["map"], 4 * W, cam, TUM1, null=("kps_un",))
    assert rc == COEB_OK and n == len(case1["kps"])
    expect(o, n, case1, tag="kp_un_out NULL", skip=("kps_un",))
    # an empty image: COEB_OK, *n_out = 0, nothing written (ORBextractor.cc:1096-1097) -- before
    # any other argument is looked at
    for kw in (dict(w=0), dict(h=0), dict(gray=None)):
        gray = kw.pop("gray", case1["fr"])
        rc, n, o = raw_frame(ctx, gray, W, case1["map"], 4 * W, cam, TUM1, **kw)
        assert rc == COEB_OK and n == 0 and untouched(o, 0), kw
    rc, n, o = raw_frame(ctx, None, W, None, 0, None, None, dtype=7, null=("kps", "desc", "u_right", "depth"))
    assert rc == COEB_OK and n == 0
    got = ctx.frame_rgbd(np.zeros((0, 0), np.uint8), np.zeros((0, 0), np.float32), cam)
    assert len(got["kps"]) == 0 and got["desc"] is None and len(got["u_right"]) == 0


def test_einval_cases_leave_no_trace(ctx, cam, case1):
    fr, m = case1["fr"], case1["map"]
    good = dict(gray=fr, stride=W, depth=m, dstride=4 * W, cam=cam, dist=TUM1)
    boxes = np.array([[10, 10, 50, 50]], np.float32)
    many = np.tile(boxes, (17, 1))
    cases = {
        "stride < width": dict(stride=W - 1),
        "null depth": dict(depth=None, dtype=cf.DEPTH_F32),
        "depth_stride < one 32F row": dict(dstride=4 * W - 1),
        "depth_stride < one 16U row": dict(depth=m.view(np.uint16)[:, :W].copy(), dstride=2 * W - 1),
        "depth_type 2": dict(dtype=2),
        "depth_type -1": dict(dtype=-1),
        "null camera": dict(cam=None),
        "17 boxes": dict(dyn=(many, None, None)),
        "null kp_out": dict(null=("kps",)),
        "null desc_out": dict(null=("desc",)),
        "null u_right_out": dict(null=("u_right",)),
        "null depth_out": dict(null=("depth",)),
    }
    for tag, kw in cases.items():
        rc, n, o = raw_frame(ctx, **dict(good, **kw))
        assert rc == COEB_EINVAL and n == 0, (tag, rc, n)
        assert untouched(o, 0), tag
        assert cf.lib().coeb_last_error(ctx.h).decode().startswith("coeb_frame_rgbd"), tag
    assert raw_frame(ctx, n_ptr=False, **good)[0] == COEB_EINVAL
    # negative counts and a null array with a count, as coeb_extract refuses them
    L = cf.lib()
    full = ctx.max_keypoints(W, H)
    for nbox, ntm, nblur, bp, tp in ((-1, 0, 0, None, None), (0, -1, 0, None, None), (0, 0, -1, None, None),
                                     (1, 0, 0, None, None), (0, 1, 0, None, None)):
        o = sentinel_outputs(full)
        n = C.c_int(-1)
        rc = L.coeb_frame_rgbd(ctx.h, fr.ctypes.data, W, H, W, m.ctypes.data, 4 * W, cf.DEPTH_F32, C.c_float(1.0),
                               C.byref(cam), None, bp, nbox, tp, ntm, None, nblur, o["kps"].ctypes.data,
                               o["kps_un"].ctypes.data, o["desc"].ctypes.data, o["u_right"].ctypes.data,
                               o["depth"].ctypes.data, full, C.byref(n))
        assert rc == COEB_EINVAL and n.value == 0 and untouched(o, 0), (nbox, ntm, nblur)
    rc, n, o = raw_frame(ctx, **good)                    # no sticky state: the next good call is exact
    assert rc == COEB_OK
    expect(o, n, case1, tag="after the EINVAL cases")


def test_interleaved_with_extract_and_debug_read(ctx, oracle_mod, ex, cam, case1):
    """coeb_extract and coeb_frame_rgbd share the context's page-locked buffer: each after the
    other, on different frames, is exact; and the context holds the frame as after coeb_extract."""
    other = synth.make_frames(W, H, 1, seed=32)[0]
    r2 = ex.extract(other)
    k2 = r2["kps"].astype(KEYPOINT_DTYPE)
    kun2 = oracle_mod.undistort_keypoints(k2, FX, FY, CX, CY, TUM1)
    ur2, dep2 = compose(k2, kun2, case1["map"])
    ref2 = dict(kps=k2, kps_un=kun2, desc=r2["desc"], u_right=ur2, depth=dep2)
    rc, n, o = raw_frame(ctx, case1["fr"], W, case1["map"], 4 * W, cam, TUM1)
    assert rc == COEB_OK
    expect(o, n, case1, tag="frame 31")
    lvl_frame = ctx.debug_read("lvl_n")
    rc, n, kps, desc = raw_extract(ctx, other, W)                                # extract after frame_rgbd
    assert rc == COEB_OK and n == len(k2)
    assert np.array_equal(kp_bytes(kps[:n]), kp_bytes(k2)) and np.array_equal(desc[:n], r2["desc"])
    rc, n, o = raw_frame(ctx, other, W, case1["map"], 4 * W, cam, TUM1)          # frame_rgbd after extract
    assert rc == COEB_OK
    expect(o, n, ref2, tag="frame 32")
    rc, n, kps, desc = raw_extract(ctx, case1["fr"], W)
    assert rc == COEB_OK and np.array_equal(kp_bytes(kps[:n]), kp_bytes(case1["kps"]))
    lvl_extract = ctx.debug_read("lvl_n")
    assert len(lvl_frame) > 0 and np.array_equal(lvl_frame, lvl_extract)


# ------------------------------------------------------------------ 5. the C++ adapter
def test_adapter_frame_rgbd(tmp_path, case1):
    """coeb::FrameRGBD (adapter/Frame_coeb.h) over ORBextractor::ExtractRGBD, from C++ with a
    reference-shaped Frame: tests/adapter_shim/frame_rgbd_exec.cpp, compiled here against the
    shim headers and the in-tree library."""
    shim = os.path.join(ROOT, "tests", "adapter_shim")
    libdir = os.path.join(ROOT, "coeb-slam_amd", "lib")
    exe = str(tmp_path / "frame_rgbd_exec")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-I", shim, "-I", os.path.join(ROOT, "coeb-slam_amd", "adapter"),
           "-I", os.path.join(ROOT, "include"), os.path.join(shim, "frame_rgbd_exec.cpp"), "-o", exe,
           "-L", libdir, "-lcoeb_front", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    d = str(tmp_path)

    def put(name, a):
        np.ascontiguousarray(a).tofile(os.path.join(d, name))
    put("size.i32", np.array([W, H], np.int32))
    put("frame.u8", case1["fr"])
    put("depth.f32", case1["map"])
    put("cam.f32", np.array([FX, FY, CX, CY, BF], np.float32))
    put("dist.f32", np.array(TUM1, np.float32))
    out = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr

    def get(name, dtype):
        return np.fromfile(os.path.join(d, name), dtype)
    n = len(case1["kps"])
    assert int(get("n.i32", np.int32)[0]) == n
    got = dict(kps=get("kps.bin", np.uint8).view(KEYPOINT_DTYPE), kps_un=get("kps_un.bin", np.uint8).view(KEYPOINT_DTYPE),
               desc=get("desc.u8", np.uint8).reshape(-1, 32), u_right=get("ur.f32", np.float32),
               depth=get("dep.f32", np.float32))
    for k in ("kps", "kps_un", "desc", "u_right", "depth"):
        assert len(got[k]) == n and np.array_equal(out_bytes(got, k), out_bytes(case1, k)), k
    checks = dict(l.split() for l in open(os.path.join(d, "checks.txt")))
    assert checks == {"empty_untouched": "1", "flat_released": "1"}, checks
