"""The TrackWithMotionModel drop-in adapter (adapter/Tracking_coeb.h) run by the shim program
(tests/adapter_shim/trackmm_exec.cpp) over Frame / MapPoint types that record what is done to
them, in SLAM mode and in localisation mode: mvpMapPoints, mvbOutlier, the pose, the return value,
mbVO, mbTrackInView / mnLastFrameSeen on exactly the discarded MapPoints, and the temporary
MapPoints in mLastFrame and mlpTemporalPoints must be what the CPU reference says
(tests/twmm_ref.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import twmm_ref as R
from conftest import ROOT

SHIM = os.path.join(ROOT, "tests", "adapter_shim")
INCLUDES = ["-I", SHIM, "-I", os.path.join(ROOT, "coeb-slam_amd", "adapter"), "-I", os.path.join(ROOT, "include")]
FRAME_ID = 23


def mat_product(a, b):
    """The shim's cv::Mat product: row by column, summed in float in order."""
    c = np.zeros((4, 4), np.float32)
    for r in range(4):
        for k in range(4):
            s = np.float32(0)
            for j in range(4):
                s = np.float32(s + np.float32(a[r, j] * b[j, k]))
            c[r, k] = s
    return c


def adapter_scene():
    """The main scene with its predicted pose written as mVelocity * mLastFrame.mTcw."""
    sc = dict(R.sized(*R.MAIN))
    V = (sc["Tcw"].astype(np.float64) @ np.linalg.inv(sc["Tcw_last"].astype(np.float64))).astype(np.float32)
    sc["Tcw"] = mat_product(V, sc["Tcw_last"])
    return sc, V


def test_adapter_scene_has_what_it_is_for():
    sc, V = adapter_scene()
    assert np.abs(sc["Tcw"] - R.sized(*R.MAIN)["Tcw"]).max() < 1e-5 and np.abs(V - np.eye(4)).max() > 0.01
    loc, slam = R.reference(sc), R.reference(sc, vo=False)
    for want in (loc, slam):
        assert want["nmatches_search"] >= 20 and (want["discarded"] >= 0).sum() >= 3 and want["nmatches_map"] >= 10
    assert loc["created"].sum() >= 20 and loc["nmatches"] > 20
    # a keypoint ends up holding a temporary point, and a replaced slot held an unobserved one before
    assert loc["created"][loc["match"][loc["match"] >= 0]].any()
    assert ((loc["created"] > 0) & (sc["last"]["has_mp"] > 0)).any()


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_trackmm_adapter_compiles():
    cmd = ["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Werror"] + INCLUDES + [os.path.join(SHIM, "trackmm_tu.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("localisation", [0, 1])
def test_trackmm_adapter_runs_against_library(tmp_path, localisation):
    lib_dir = os.path.join(ROOT, "coeb-slam_amd", "lib")
    exe = str(tmp_path / "trackmm_exec")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Werror"] + INCLUDES + [
        os.path.join(SHIM, "trackmm_exec.cpp"), "-o", exe, "-L", lib_dir, "-lcoeb_front", "-Wl,-rpath," + lib_dir,
        "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sc, V = adapter_scene()
    want = R.reference(sc, vo=bool(localisation))
    la = sc["last"]
    n, nl = len(sc["kps"]), len(la["has_mp"])
    cam = np.array(list(sc["intr"]) + [0.0, float(R.W), 0.0, float(R.H)], np.float32)
    for name, a in (("cam.f32", cam), ("V.f32", V), ("T_last.f32", sc["Tcw_last"]),
                    ("flags.i32", np.array([localisation, FRAME_ID], np.int32)),
                    ("thdepth.f32", np.array([sc["th_depth"]], np.float32)), ("kps.bin", sc["kps"]), ("desc.u8", sc["desc"]),
                    ("ur.f32", sc["ur"]), ("l_kps.bin", la["keys_un"]), ("l_desc.u8", sc["last_desc"]),
                    ("l_depth.f32", sc["depth"]), ("l_outl.u8", la["outlier"]), ("l_has.u8", la["has_mp"]),
                    ("l_xw.f32", la["xw"]), ("l_mpdesc.u8", la["mp_desc"]), ("l_obs.i32", np.asarray(la["mp_nobs"], np.int32))):
        np.ascontiguousarray(a).tofile(str(tmp_path / name))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr

    def got(name, dt):
        return np.fromfile(str(tmp_path / name), dt)

    assert np.array_equal(got("mvp.i32", np.int32), want["match"])
    # mvbOutlier: false on every matched keypoint, kept or discarded (:977); the others keep their initial true
    assert np.array_equal(got("outl.u8", np.uint8), (want["match_search"] < 0).astype(np.uint8))
    assert np.array_equal(got("T_out.f32", np.uint32), R.bits(want["Tcw"]).ravel())
    if localisation:
        ret, vo = int(want["nmatches"] > 20), int(want["nmatches_map"] < 10)
    else:
        ret, vo = int(want["nmatches_map"] >= 10), 1                # mbVO left as it was
    assert list(got("ret.i32", np.int32)) == [ret, want["nmatches_map"], vo]
    has_after = want["last"]["has_mp"] > 0
    gone = np.zeros(nl, bool)
    gone[want["discarded"][want["discarded"] >= 0]] = True
    assert np.array_equal(got("mp_inview.u8", np.uint8), np.where(has_after, (~gone).astype(np.uint8), 2))
    assert np.array_equal(got("mp_seen.i32", np.int32), np.where(has_after, np.where(gone, FRAME_ID, FRAME_ID - 1), -1))
    created = want["created"] if localisation else np.zeros(nl, np.uint8)
    assert np.array_equal(got("mp_new.u8", np.uint8), created)
    # mlpTemporalPoints: the created slots in the order of UpdateLastFrame's depth sort, each at its position
    order = [i for i in R.visited_loop(sc["depth"], sc["th_depth"]) if created[i]]
    assert list(got("tmp_slot.i32", np.int32)) == order and len(order) == int(created.sum())
    if localisation:
        assert np.array_equal(got("tmp_pos.f32", np.uint32).reshape(-1, 3), R.bits(want["created_pos"][order]))
