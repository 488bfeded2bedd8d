"""coeb_frame_rgbd without a GPU: the host part of the entry point (argument check, page-locked
buffer layout, row staging: csrc/coeb_single_frame_host.hpp) as a stand-alone program under
ASan + UBSan, the C++ adapter (ORBextractor::ExtractRGBD, coeb::FrameRGBD) as a compile check
against the OpenCV stand-in, and the Python mirror's declaration of the entry point."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SHIM = os.path.join(ROOT, "tests", "adapter_shim")
INCLUDES = ["-I", SHIM, "-I", os.path.join(ROOT, "coeb-slam_amd", "adapter"), "-I", os.path.join(ROOT, "include")]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_host_part_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "frame_rgbd_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "coeb-slam_amd", "csrc"),
           os.path.join(ROOT, "tests", "host", "frame_rgbd_host_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_frame_rgbd_adapter_compiles():
    cmd = ["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Werror"] + INCLUDES + [os.path.join(SHIM, "frame_rgbd_exec.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_exports_and_mirror_declares_frame_rgbd():
    import coeb_front
    assert "coeb_frame_rgbd" in coeb_front.ABI_SYMBOLS
    L = ctypes.CDLL(coeb_front.LIB_PATH)
    assert hasattr(L, "coeb_frame_rgbd")
    assert len(coeb_front.lib().coeb_frame_rgbd.argtypes) == 24          # the header's parameter list
    sig = inspect.signature(coeb_front.Context.frame_rgbd)
    assert list(sig.parameters) == ["self", "gray", "depth", "cam", "dist", "boxes", "tm", "blur", "depth_scale"]
    assert sig.parameters["depth_scale"].default == 1.0 and sig.parameters["dist"].default is None
