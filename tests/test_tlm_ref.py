"""The single-frame TrackLocalMap reference (tests/tlm_ref.py) and its scene, without a GPU: the
scene takes every exit of Frame::isInFrustum and every branch of the merge, asserted on the
oracle's own result; one point is worked by hand; the adapter (adapter/Tracking_coeb.h)
compiles against reference-shaped types and the header declares both entry points."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle as O
import tlm_ref as R
from conftest import ROOT

SHIM = os.path.join(ROOT, "tests", "adapter_shim")
INCLUDES = ["-I", SHIM, "-I", os.path.join(ROOT, "coeb-slam_amd", "adapter"), "-I", os.path.join(ROOT, "include")]
SCENES = ((640, 480, 1000), (333, 251, 400))


def exits(sc):
    """The exit of isInFrustum each valid point takes, by a float64 restatement with a margin
    (points within the margin of a test are left unclassified): name -> bool[n]."""
    p = sc["pts"]
    T = sc["Tcw"].astype(np.float64)
    P = p["world_pos"].astype(np.float64)
    Pc = P @ T[:3, :3].T + T[:3, 3]
    fx, fy, cx, cy, _ = sc["intr"]
    z = np.where(np.abs(Pc[:, 2]) > 1e-9, Pc[:, 2], 1e-9)
    u, v = fx * Pc[:, 0] / z + cx, fy * Pc[:, 1] / z + cy
    x0, x1, y0, y1 = sc["bounds"]
    d = R.camera_distance(sc["Tcw"], p["world_pos"]).astype(np.float64)
    Ow = -(T[:3, :3].T @ T[:3, 3])
    cos = ((P - Ow) * p["normal"].astype(np.float64)).sum(1) / np.maximum(d, 1e-9)
    m, left = 1e-3, p["valid"] > 0
    out = {}
    for name, hit, keep in (("behind", Pc[:, 2] < -m, Pc[:, 2] > m), ("left", u < x0 - m, u > x0 + m),
                            ("right", u > x1 + m, u < x1 - m), ("above", v < y0 - m, v > y0 + m),
                            ("below", v > y1 + m, v < y1 - m),
                            ("near", d < 0.8 * p["min_distance"] * (1 - m), d > 0.8 * p["min_distance"] * (1 + m)),
                            ("far", d > 1.2 * p["max_distance"] * (1 + m), d < 1.2 * p["max_distance"] * (1 - m)),
                            ("cos", cos < R.COS_LIMIT - m, cos > R.COS_LIMIT + m)):
        out[name] = left & hit
        left = left & keep
    out["inside"] = left
    return out


@pytest.mark.parametrize("w,h,nd", SCENES)
def test_scene_has_what_it_is_for(w, h, nd):
    sc = R.scene(w, h, n_distract=nd)
    r = R.reference(sc)
    iv = r["in_view"] > 0
    assert sc["bounds"] != (0.0, float(w), 0.0, float(h))
    ex = exits(sc)
    for name in ("behind", "left", "right", "above", "below", "near", "far", "cos"):
        assert ex[name].sum() >= 5 and not iv[ex[name]].any(), (name, int(ex[name].sum()))
    assert iv[ex["inside"]].all() and not iv[sc["pts"]["valid"] == 0].any()
    # PredictScale's clamp, both ends
    s = R.unclamped_level(sc["pts"]["max_distance"], R.camera_distance(sc["Tcw"], sc["pts"]["world_pos"]), sc["log_sf"])
    assert (s[iv] < 0).any() and (s[iv] >= 8).any()
    assert np.array_equal(r["level"][iv], np.clip(s[iv], 0, 7))
    assert (r["view_cos"][iv] > 0.998).sum() >= 20 and (r["view_cos"][iv] <= 0.998).sum() >= 20
    assert r["n_to_match"] >= 200 and r["nlocal"] >= 100
    co = sc["cur_obs"]
    assert ((co >= 0) & (r["match"] < 0)).sum() >= 50                     # keypoints that keep their entry point
    assert ((co == 0) & (r["match"] >= 0)).sum() >= 1                     # an unobserved entry point replaced
    assert (sc["pts"]["observations"] == 0).any() and set(np.unique(co)) == {-1, 0, 1, 2}
    assert r["outlier"].sum() >= 1 and r["ninliers_pose"] >= 30
    assert not np.array_equal(r["Tcw"], sc["Tcw"])
    assert ((r["has2"] > 0) & (r["outlier"] == 0) & (r["obs2"] == 0)).sum() >= 1
    assert R.reference(sc, only_tracking=True)["nmatches_inliers"] > r["nmatches_inliers"] > 0


def test_reference_skips_the_search_with_nothing_in_view():
    sc = R.scene(333, 251, n_distract=400)
    pts = dict(sc["pts"])
    pts["valid"] = np.zeros_like(pts["valid"])
    r = R.reference(R.with_points(sc, pts))
    assert r["n_to_match"] == 0 and r["nlocal"] == 0 and (r["match"] == -1).all()
    assert r["ninliers_pose"] > 0 and np.array_equal(r["has2"] > 0, sc["cur_obs"] >= 0)   # the pose still runs


def test_hand_worked_point():
    """fx = fy = 500, cx = 320, cy = 240, bf = 40; Tcw = [I | (0.5, -0.25, 2)], P = (0.5, 0.75, 2):
    Pc = (1, 0.5, 4), invz = 0.25, u = 500 * 1 * 0.25 + 320 = 445, v = 500 * 0.5 * 0.25 + 240 =
    302.5, ur = 445 - 40 * 0.25 = 435.  mOw = (-0.5, 0.25, -2), PO = (1, 0.5, 4), dist =
    sqrt(17.25) = 4.1533117f; Pn = (0, 0, 1): viewCos = 4 / 4.1533117 = 0.96308684f.
    mfMaxDistance = 8: ratio 1.9261737, log(ratio) / log(1.2f) = 3.595.. -> level 4."""
    cam_o = O.camera(R.extractor(), 640, 480, 500.0, 500.0, 320.0, 240.0, 40.0)
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = (0.5, -0.25, 2.0)

    def run(maxd, mind, normal=(0, 0, 1), cos_limit=0.5):
        pts = dict(valid=np.ones(1, np.uint8), world_pos=np.array([[0.5, 0.75, 2.0]], np.float32),
                   normal=np.array([normal], np.float32), max_distance=np.array([maxd], np.float32),
                   min_distance=np.array([mind], np.float32))
        return R.frustum(cam_o, T, pts, cos_limit)

    r = run(8.0, 8.0 / 3.5831808)
    assert r["in_view"][0] == 1 and r["n_to_match"] == 1
    assert r["proj_x"][0] == np.float32(445.0) and r["proj_y"][0] == np.float32(302.5)
    assert r["proj_xr"][0] == np.float32(435.0) and r["level"][0] == 4
    assert r["view_cos"][0] == np.float32(0.96308684)
    assert run(8.0, 8.0 / 3.5831808, cos_limit=0.97)["in_view"][0] == 0
    assert run(3.4, 1.0)["in_view"][0] == 0                     # 1.2 * 3.4 = 4.08 < dist
    assert run(30.0, 5.2)["in_view"][0] == 0                    # 0.8 * 5.2 = 4.16 > dist
    assert run(30.0, 5.1)["level"][0] == 7                      # ratio 7.2: ceil(10.8) clamped to nlevels - 1
    assert run(8.0, 1.0, normal=(0, 0, -1))["in_view"][0] == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_tracking_adapter_compiles():
    cmd = ["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Werror"] + INCLUDES + [os.path.join(SHIM, "tracklm_tu.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_header_declares_both_entry_points():
    txt = open(os.path.join(ROOT, "include", "coeb_front.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("coeb_search_local_points", "coeb_track_local_map"):
        assert re.search(r"\bint\s+%s\s*\(" % name, txt), name
    assert "coeb_local_points;" in txt and "coeb_track_fields;" in txt
    import coeb_front
    assert {"coeb_search_local_points", "coeb_track_local_map"} <= set(coeb_front.ABI_SYMBOLS)
