"""bench.py --dump-outputs on the device: the arrays a plain run writes are what the oracle computes
for the sampled frames of the bench's own synthetic input, and two runs with the same arguments
write the same arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, d):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dump-outputs", str(d)] + args
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=110, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_is_reproducible_and_matches_oracle(tmp_path, oracle_mod):
    """Config A, 9 matched frames as two pipelines (5 + 4, a halo frame each), 3 timed steps."""
    O = oracle_mod
    from coeb_front import synth
    args = ["--steps", "3", "--warmup", "1", "--batch", "9", "--pipelines", "2"]
    rec, a = _run(args, tmp_path / "a")
    rec_b, b = _run(args, tmp_path / "b")
    assert rec["steps"] == 3 and rec["ms_per_step"] > 0 and "cpu_baseline" not in rec and rec["roofline"] is None
    assert set(a) == set(b) == {"frame_index", "keypoint_count", "match_count", "keypoints", "descriptors", "matches"}
    for n in a:
        assert a[n].dtype in (np.float32, np.float64) and np.array_equal(a[n], b[n]), n
    assert a["frame_index"].tolist() == list(range(1, 10))            # fewer than the sample size: every counted frame
    cfg = bench.CONFIGS["A"]
    w, h = cfg["w"], cfg["h"]
    frames = synth.make_frames(w, h, 10, seed=1000, first=0)
    ex = O.Extractor(cfg["nfeatures"], 1.2, 8, 20, 7)
    cam = O.camera(ex, w, h, synth.TUM_FX, synth.TUM_FY, synth.TUM_CX, synth.TUM_CY, synth.TUM_BF)
    depth = synth.make_depth(w, h)
    Tc, I4 = synth.motion_pose(), np.eye(4, dtype=np.float32)
    ref = [ex.extract(f) for f in frames]
    row = 0
    for i, g in enumerate(a["frame_index"].astype(int)):
        r, prev = ref[g], ref[g - 1]
        n = len(r["kps"])
        assert a["keypoint_count"][i] == n
        kp = a["keypoints"][row:row + n]
        for j, name in enumerate(r["kps"].dtype.names):
            assert np.array_equal(kp[:, j], r["kps"][name].astype(np.float32)), (g, name)
        assert np.array_equal(a["descriptors"][row:row + n], r["desc"].astype(np.float32)), g
        last = O.mapframe_from_extraction(prev["kps"], prev["desc"], depth, synth.TUM_FX, synth.TUM_FY, synth.TUM_CX,
                                          synth.TUM_CY, synth.TUM_BF)
        ur, _ = O.stereo_from_rgbd(r["kps"], depth, synth.TUM_BF)
        nm, m = O.search_by_projection(cam, r["kps"], r["desc"], ur, last, Tc, I4, 15.0)
        if nm < 20:
            nm, m = O.search_by_projection(cam, r["kps"], r["desc"], ur, last, Tc, I4, 30.0)
        assert a["match_count"][i] == nm and np.array_equal(a["matches"][row:row + n], m.astype(np.float32)), g
        row += n
    assert row == len(a["keypoints"])


def test_dump_config_d_records(tmp_path):
    """Config D adds the tracking records, one row per sampled frame / keypoint."""
    rec, a = _run(["--config", "D", "--steps", "2", "--warmup", "1", "--batch", "6", "--pipelines", "2"], tmp_path / "d")
    n = int(a["keypoint_count"].sum())
    assert a["frame_index"].tolist() == list(range(1, 7)) and n > 0
    assert a["pose"].shape == a["pose_motion_model"].shape == (6, 4, 4) and np.isfinite(a["pose"]).all()
    assert a["local_matches"].shape == a["outliers"].shape == a["matches"].shape == (n,)
    assert set(a["state"].tolist()) <= {0.0, 1.0, 2.0} and set(np.unique(a["outliers"]).tolist()) <= {0.0, 1.0}
    want = np.where((a["match_count"] < 20) | (a["matches_map"] < 10), 0, np.where(a["inliers"] >= 30, 2, 1))
    assert np.array_equal(a["state"], want)
    assert rec["tracking"]["frames"] == 3
