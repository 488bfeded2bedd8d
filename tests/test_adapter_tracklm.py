"""The Tracking drop-in adapter (adapter/Tracking_coeb.h) run by the shim program
(tests/adapter_shim/tracklm_exec.cpp) over Frame / MapPoint types that record what is done to
them: mvpMapPoints, mvbOutlier, the pose, the mnVisible / mnFound increments, mbTrackInView with
the mTrack* fields and the return value must be what the CPU reference says (tests/tlm_ref.py),
with bad and already-seen points in the local map and bad entry MapPoints on the frame."""
import os
import subprocess

import numpy as np
import pytest

import tlm_ref as R
from conftest import ROOT

SHIM = os.path.join(ROOT, "tests", "adapter_shim")
INCLUDES = ["-I", SHIM, "-I", os.path.join(ROOT, "coeb-slam_amd", "adapter"), "-I", os.path.join(ROOT, "include")]
FRAME_ID = 17


def adapter_scene():
    """The 333 x 251 scene; its invalid points become bad (odd index) or seen in this frame (even),
    and every 9th entry MapPoint is bad, which the adapter resets to NULL before the snapshot."""
    sc = R.scene(333, 251, n_distract=400)
    valid = sc["pts"]["valid"] > 0
    kind = np.where(valid, 0, 1 + (np.arange(len(valid)) % 2 == 0)).astype(np.uint8)
    cur_bad = ((sc["cur_obs"] >= 0) & (np.arange(len(sc["cur_obs"])) % 9 == 0)).astype(np.uint8)
    eff = dict(sc)
    eff["cur_obs"] = np.where(cur_bad > 0, -1, sc["cur_obs"]).astype(np.int32)
    return sc, eff, kind, cur_bad


def test_adapter_scene_has_what_it_is_for():
    sc, eff, kind, cur_bad = adapter_scene()
    assert (kind == 1).sum() >= 5 and (kind == 2).sum() >= 5 and cur_bad.sum() >= 5
    want = R.reference(eff)
    assert want["nlocal"] >= 100 and want["outlier"].any()
    assert ((eff["cur_obs"] >= 0) & (want["match"] < 0)).sum() >= 50


@pytest.mark.gpu
@pytest.mark.parametrize("only_tracking", [0, 1])
def test_tracking_adapter_runs_against_library(tmp_path, only_tracking):
    lib_dir = os.path.join(ROOT, "coeb-slam_amd", "lib")
    exe = str(tmp_path / "tracklm_exec")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Werror"] + INCLUDES + [
        os.path.join(SHIM, "tracklm_exec.cpp"), "-o", exe, "-L", lib_dir, "-lcoeb_front", "-Wl,-rpath," + lib_dir,
        "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    sc, eff, kind, cur_bad = adapter_scene()
    p = sc["pts"]
    cam = np.array(list(sc["intr"]) + list(sc["bounds"]), np.float32)
    for name, a in (("cam.f32", cam), ("T.f32", sc["Tcw"]), ("flags.i32", np.array([only_tracking, FRAME_ID], np.int32)),
                    ("kps.bin", sc["kps"]), ("desc.u8", sc["desc"]), ("ur.f32", sc["ur"]), ("cur_obs.i32", sc["cur_obs"]),
                    ("cur_xw.f32", sc["cur_xw"]), ("cur_bad.u8", cur_bad), ("p_kind.u8", kind), ("p_xw.f32", p["world_pos"]),
                    ("p_normal.f32", p["normal"]), ("p_maxd.f32", p["max_distance"]), ("p_mind.f32", p["min_distance"]),
                    ("p_desc.u8", p["descriptor"]), ("p_obs.i32", p["observations"])):
        np.ascontiguousarray(a).tofile(str(tmp_path / name))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr

    def got(name, dt):
        return np.fromfile(str(tmp_path / name), dt)

    want = R.reference(eff, bool(only_tracking))
    n, nq = len(sc["kps"]), len(kind)
    held = np.where(want["match"] >= 0, want["match"], np.where(eff["cur_obs"] >= 0, 1000000 + np.arange(n), -1))
    assert np.array_equal(got("mvp.i32", np.int32), held)
    assert np.array_equal(got("outl.u8", np.uint8), want["outlier"])
    assert np.array_equal(got("T_out.f32", np.uint32), R.bits(want["Tcw"]).ravel())
    assert got("ret.i32", np.int32)[0] == want["nmatches_inliers"]
    iv = want["in_view"] > 0
    # mbTrackInView: isInFrustum's verdict on the valid points, untouched (true) on the others
    assert np.array_equal(got("p_inview.u8", np.uint8), np.where(kind == 0, iv, 1))
    f = got("p_fields.f32", np.float32).reshape(nq, 5)
    for j, k in enumerate(("proj_x", "proj_y", "proj_xr", "view_cos")):
        assert np.array_equal(R.bits(f[iv, j]), R.bits(want[k][iv])), k
    assert np.array_equal(f[iv, 4], want["level"][iv].astype(np.float32)) and (f[~iv] == -1).all()
    assert np.array_equal(got("p_visible.i32", np.int32), iv.astype(np.int32))
    inl = (want["has2"] > 0) & (want["outlier"] == 0)
    pfound = np.bincount(want["match"][inl & (want["match"] >= 0)], minlength=nq)
    assert np.array_equal(got("p_found.i32", np.int32), pfound)
    live = eff["cur_obs"] >= 0                               # entry MapPoints that are not bad
    assert np.array_equal(got("e_visible.i32", np.int32), live.astype(np.int32))
    assert np.array_equal(got("e_found.i32", np.int32), (inl & (want["match"] < 0)).astype(np.int32))
    assert np.array_equal(got("e_inview.u8", np.uint8), (~live).astype(np.uint8))
    assert np.array_equal(got("e_seen.i32", np.int32), np.where(live, FRAME_ID, np.where(sc["cur_obs"] >= 0, FRAME_ID - 1, 0)))
    # SearchLocalPoints alone
    assert np.array_equal(got("s_mvp.i32", np.int32), held)
    assert got("s_ret.i32", np.int32)[0] == want["n_to_match"]
    assert np.array_equal(got("s_p_visible.i32", np.int32), iv.astype(np.int32))
