"""coeb::FrameRGBDStream (adapter/Frame_coeb.h over ORBextractor::ExtractRGBDStream) from C++ with a
reference-shaped Frame: tests/adapter_shim/frame_stream_exec.cpp, compiled here against the shim
headers and the in-tree library (the compile needs no GPU), then run on the 640x480 sequence of
tests/stream_ref.py.  Four frames in a row must equal the reference bit for bit; then the lifetime
rules a tracking thread depends on: coeb::FrameStreamReset (Tracking::Reset) and a frame handed to
another extractor (the adaptive nFeatures switch) both make the next frame a first frame, and an
empty image leaves outputs and stream alone."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from coeb_front import KEYPOINT_DTYPE
import stream_ref as R
from conftest import ROOT

SHIM = os.path.join(ROOT, "tests", "adapter_shim")
LIBDIR = os.path.join(ROOT, "coeb-slam_amd", "lib")
INCLUDES = ["-I", SHIM, "-I", os.path.join(ROOT, "coeb-slam_amd", "adapter"), "-I", os.path.join(ROOT, "include")]
FIELDS = ("kps", "kps_un", "desc", "u_right", "depth")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_frame_stream_adapter_compiles():
    cmd = ["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Werror"] + INCLUDES + [os.path.join(SHIM, "frame_stream_exec.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def raw(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(len(a), -1) if len(a) else np.zeros((0, 0), np.uint8)


@pytest.mark.gpu
def test_frame_stream_adapter_runs_against_library(tmp_path, oracle_mod):
    exe = str(tmp_path / "frame_stream_exec")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Werror"] + INCLUDES + [os.path.join(SHIM, "frame_stream_exec.cpp"), "-o", exe,
           "-L", LIBDIR, "-lcoeb_front", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    s = R.SEQUENCES["vga"]
    w, h = s["w"], s["h"]
    fr, boxes = R.sequence("vga")
    depth = R.depth_map(w, h)
    d = str(tmp_path)

    def put(name, a):
        np.ascontiguousarray(a).tofile(os.path.join(d, name))
    put("size.i32", np.array([w, h, s["n"], 2], np.int32))
    put("frames.u8", fr)
    put("depth.f32", depth)
    put("cam.f32", np.array(R.camera_params(w, h) + (R.BF,), np.float32))
    put("dist.f32", np.array(R.TUM1, np.float32))
    put("boxes.f32", np.stack(boxes).astype(np.float32))
    out = subprocess.run([exe, d], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr

    def get(tag):
        g = lambda name, dtype: np.fromfile(os.path.join(d, tag + "." + name), dtype)
        return dict(kps=g("kps.bin", np.uint8).view(KEYPOINT_DTYPE), kps_un=g("kps_un.bin", np.uint8).view(KEYPOINT_DTYPE),
                    desc=g("desc.u8", np.uint8).reshape(-1, 32), u_right=g("ur.f32", np.float32), depth=g("dep.f32", np.float32),
                    tm=g("tm.f32", np.float32).reshape(-1, 2), blur=g("blur.i32", np.int32), n=int(g("n.i32", np.int32)[0]))

    def same(tag, ref):
        got = get(tag)
        assert got["n"] == len(ref["kps"]), (tag, got["n"], len(ref["kps"]))
        assert np.array_equal(raw(got["tm"]), raw(ref["tm"])), (tag, "tm", len(got["tm"]), len(ref["tm"]))
        assert np.array_equal(got["blur"], ref["blur"]), (tag, got["blur"], ref["blur"])
        for k in FIELDS:
            assert np.array_equal(raw(got[k]), raw(ref[k])), (tag, k)

    ref = R.sequence_ref("vga")
    for f in range(4):                                          # four frames in a row
        same("f%d" % f, ref[f])
    assert sum(len(ref[f]["tm"]) for f in range(1, 4)) > 0
    # Tracking::Reset: frame 4 is a first frame, frame 5 pairs with it
    first4 = R.frame_ref(None, fr[4], boxes[4], depth)
    assert len(ref[4]["tm"]) > 0 and len(first4["tm"]) == 0
    same("r4", first4)
    same("r5", ref[5])
    # the extractor switch: the other extractor's frame is a first frame, and so is the next one of the first
    same("b4", R.frame_ref(None, fr[4], boxes[4], depth, orb=(1500, 1.2, 8, 20, 7)))
    same("s5", R.frame_ref(None, fr[5], boxes[5], depth))
    checks = dict(l.split() for l in open(os.path.join(d, "checks.txt")))
    assert checks == {"empty_untouched": "1"}, checks
