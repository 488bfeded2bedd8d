"""coeb_rgbd_stream_frame without a GPU: the host part of the entry point (argument checks, the
page-locked layout of a call, the slot layout and arithmetic of the stream's device memory:
csrc/coeb_rgbd_stream_host.hpp) as a stand-alone program under ASan + UBSan -- layouts for 32x32,
333x251 with 3 channels, 640x480 and 1280x960, 16U and 32F depth, with 0, 1 and 64 boxes -- and the
Python mirror's declaration of the new entry points.  COEB_MAX_BOXES is 16, so 64 boxes exceed the
ABI's limit: the program checks that the argument check refuses them (as it refuses 17) and that the
layout, whose head is sized for COEB_MAX_BOXES, does not depend on the count; only 0, 1 and 16 boxes
are ever written into a head."""
import ctypes
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_host_part_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "rgbd_stream_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "coeb-slam_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "rgbd_stream_host_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_library_exports_and_mirror_declares_the_stream():
    import coeb_front
    names = ["coeb_rgbd_stream_create", "coeb_rgbd_stream_destroy", "coeb_rgbd_stream_reset", "coeb_rgbd_stream_frame"]
    L = ctypes.CDLL(coeb_front.LIB_PATH)
    for nm in names:
        assert nm in coeb_front.ABI_SYMBOLS and hasattr(L, nm), nm
    assert len(coeb_front.lib().coeb_rgbd_stream_frame.argtypes) == 16       # the header's parameter list
    # coeb_rgbd_stream_out as the header lays it out on LP64
    o = coeb_front.RgbdStreamOutC
    assert [f[0] for f in o._fields_] == ["tm_xy", "tm_cap", "n_tm", "blur_flag", "gray", "gray_stride", "kp", "kp_un",
                                          "desc", "u_right", "depth", "cap", "n", "first"]
    assert ctypes.sizeof(o) == 96 and o.blur_flag.offset == 16 and o.cap.offset == 80 and o.first.offset == 88
    assert coeb_front.STREAM_NO_SHADOW == 1
    for m in ("frame", "reset", "close"):
        assert callable(getattr(coeb_front.RGBDStream, m))
