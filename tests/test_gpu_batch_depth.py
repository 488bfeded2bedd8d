"""The device-batch tracking chain (coeb_extract_batch_device / coeb_frame_batch_device ->
coeb_match_batch_device* -> coeb_pose_batch_device -> coeb_track_local_map_batch_device) under
the input it exists for: a depth map per frame with 20-30 % holes, predicted poses that are not
one shared translation, frames without keypoints or without MapPoints inside the batch, and
nobs = 0 (MI355X only).

Every test compares the whole chain with the oracle bit for bit (chain_util._check_chain:
descriptors, mvuRight / mvDepth out of k_prep, matches, both poses as uint32, inlier counts,
nmatchesMap, local-map matches, both optimisations' outlier flags, state), then asserts the
coverage condition that is the reason for its scenario.  Those conditions are computed from the
ORACLE's results (chain_util.assert_coverage_*), never from device output, so none can pass
because a kernel is wrong; tests/test_oracle_kat.py asserts the same conditions without a GPU.
All scenarios are 640x480, F = 8, with the image bounds of an undistorted image: frame sizes
whose per-frame offsets are no multiple of 4 and other image bounds are
tests/test_gpu_chain_shapes.py's business, bench-size batches tests/test_gpu_bench_scale.py's.
"""
import numpy as np
import pytest

import chain_util as cu
from chain_util import F, H, W

pytestmark = pytest.mark.gpu

_scenarios, _chains = {}, {}


@pytest.fixture(scope="module")
def ex(oracle_mod):
    return oracle_mod.Extractor()


def scenario(name):
    if name not in _scenarios:
        _scenarios[name] = getattr(cu, "scenario_" + name)()
    return _scenarios[name]


def oracle_chain(oracle_mod, ex, name, nkf, stride):
    """(extractions, per-frame oracle results) of a scenario, computed once per module and shared.
    stride: the batch's keypoint slots per frame, which number the local map's slots."""
    key = (name, nkf, stride)
    if key not in _chains:
        isg = np.array(ex.p.inv_sigma2[:8], np.float32)
        _chains[key] = cu.run_oracle(oracle_mod, ex, scenario(name), stride, isg, nkf=nkf)
    return _chains[key]


def pipeline(ex):
    from coeb_front.pipeline import BatchPipeline
    bp = BatchPipeline(W, H, F)
    assert np.array_equal(np.array(bp.ctx.tables().inv_sigma2[:8], np.float32),
                          np.array(ex.p.inv_sigma2[:8], np.float32))
    return bp


def run_checked(bp, oracle_mod, ex, name, **kw):
    """One step, synchronised (coeb_synchronize fails on a capacity error word), then the whole
    chain against the oracle.  Returns (ext, res, stride, states, device track results)."""
    bp.run(**kw)
    bp.synchronize()
    stride = bp.ctx.batch_results()[3]
    ext, res = oracle_chain(oracle_mod, ex, name, kw.get("nkf", 2), stride)
    states, tr = cu._check_chain(bp, ext, res, F)
    return ext, res, stride, states, tr


@pytest.mark.parametrize("nkf", [2, 1])
def test_chain_depth_holes(oracle_mod, ex, nkf):
    """Per-frame depth surfaces with holes: every frame's first PoseOptimization mixes
    monocular (mvuRight < 0) and stereo edges, every LastFrame has keypoints without a
    MapPoint, every frame is tracked."""
    s = scenario("holes")
    bp = pipeline(ex)
    try:
        bp.load(s["frames"], depth=s["depth"], Tcw=s["Tcw"])
        ext, res, _, states, tr = run_checked(bp, oracle_mod, ex, "holes", track=True, nkf=nkf)
        cu.assert_coverage_holes(res)
        assert states == [2] * (F - 1)
        # pipelined: three back-to-back steps leave the single-step results
        for _ in range(3):
            bp.run(track=True, nkf=nkf)
        bp.synchronize()
        tr2 = bp.track_results()
        assert tr2["ninliers"] == tr["ninliers"] and tr2["nlocal"] == tr["nlocal"]
        assert np.array_equal(tr2["T"][1:].view(np.uint32), tr["T"][1:].view(np.uint32))
        cu._check_chain(bp, ext, res, F)
    finally:
        bp.close()


def test_chain_degenerate_neighbours(oracle_mod, ex):
    """Frame 3's own depth is all holes (optimised on monocular edges alone), so frame 4 meets
    a LastFrame without MapPoints; frame 5 is a constant image (0 keypoints), so frame 6 meets
    an empty LastFrame and frame 7 an empty KeyFrame f-2."""
    s = scenario("degenerate")
    bp = pipeline(ex)
    try:
        bp.load(s["frames"], depth=s["depth"], Tcw=s["Tcw"])
        ext, res, _, states, tr = run_checked(bp, oracle_mod, ex, "degenerate", track=True)
        cu.assert_coverage_degenerate(ext, res)
        assert states == cu.DEGENERATE_STATES
        out, matches, nms = bp.results()
        assert len(out[5][0]) == 0 and nms[4:7] == [0, 0, 0]
        for f in (4, 5, 6):                                      # lost: the pose is the prediction
            assert np.array_equal(tr["T"][f].view(np.uint32), s["Tcw"][f].view(np.uint32)), f
    finally:
        bp.close()


def test_chain_nobs_zero(oracle_mod, ex):
    """Observations() == 0 on every MapPoint: the matcher skips no claim, the first
    PoseOptimization runs, nmatchesMap stays 0 and TrackLocalMap must not run."""
    s = scenario("nobs_zero")
    bp = pipeline(ex)
    try:
        bp.load(s["frames"], depth=s["depth"], Tcw=s["Tcw"])
        ext, res, _, states, tr = run_checked(bp, oracle_mod, ex, "nobs_zero", track=True, nobs=0)
        cu.assert_coverage_nobs_zero(res, s["Tcw"])
        assert states == [0] * (F - 1)
        T1, _, _ = bp.pose_results()
        for f in range(1, F):
            assert tr["nmatches_map"][f] == res[f]["nmatches_map"] == 0, f
            assert tr["nlocal"][f] == res[f]["nlocal"] == 0, (f, tr["nlocal"][f])
            assert np.array_equal(tr["local_match"][f], res[f]["local_match"]), f
            assert np.array_equal(tr["T"][f].view(np.uint32), T1[f].view(np.uint32)), f
    finally:
        bp.close()


def test_chain_perturbed_poses(oracle_mod, ex):
    """A different full-rank predicted pose per frame (rotations about x and y, z translations
    both ways): every projection uses its own frame's rotation, and the local map's predicted
    levels leave the source keypoints' octaves.  The host-pose entry point
    (coeb_match_batch_device) must give the same matches as the device-pose one."""
    s = scenario("perturbed")
    bp = pipeline(ex)
    try:
        bp.load(s["frames"], depth=s["depth"], Tcw=s["Tcw"])
        ext, res, stride, states, _ = run_checked(bp, oracle_mod, ex, "perturbed", track=True)
        cu.assert_coverage_perturbed(res, stride)
        assert states == [2] * (F - 1)
        bp.ctx.match_batch_device(bp.depth.ptr, F, W, H, bp.cam, s["Tcw"])
        bp.synchronize()
        _, matches, nms = bp.results()
        for f in range(1, F):
            assert nms[f] == res[f]["nmatches"] and np.array_equal(matches[f], res[f]["match"]), f
    finally:
        bp.close()


def test_chain_lost_neighbours_reach_frustum_rejections(oracle_mod, ex):
    """Frames 2, 4 and 6 are lost on moderately wrong predictions, so the frames after them
    place KeyFrame f-2 by a wrong pose: isInFrustum turns slots away at the image bounds, at both
    ends of the distance range and on the view angle, while other KeyFrame f-2 points stay in
    view.  The lost frames' PoseOptimization runs on a few dozen wrong matches."""
    s = scenario("lost_neighbours")
    bp = pipeline(ex)
    try:
        bp.load(s["frames"], depth=s["depth"], Tcw=s["Tcw"])
        ext, res, stride, states, _ = run_checked(bp, oracle_mod, ex, "lost_neighbours", track=True)
        cu.assert_coverage_lost_neighbours(res, stride)
        assert states == cu.LOST_STATES
    finally:
        bp.close()


def test_grab_rgbd_loop_raw_depth_holes(oracle_mod, ex):
    """The whole GrabImageRGBD loop (bench config D's path) on RGB images and raw 16U depth
    whose holes are stored as 0: conversion, Frame constructor with boxes, motion model and
    TrackLocalMap, against the oracle chain over the converted float depth."""
    s = scenario("grab_rgbd")
    bp = pipeline(ex)
    try:
        bp.load_rgbd(s["rgb"], s["depth_u16"], 1.0 / 5000.0, Tcw=s["Tcw"])
        bp.set_frame_boxes(s["boxes"])
        ext, res, _, states, _ = run_checked(bp, oracle_mod, ex, "grab_rgbd", rgbd=True, frame=True, track=True)
        cu.assert_coverage_grab(res)
        assert states.count(2) >= F - 2, states
        dep = bp.ctx.download(bp.depth.ptr, 4 * F * H * W, np.float32).reshape(F, H, W)
        assert np.array_equal(dep.view(np.uint32), s["depth"].view(np.uint32))
    finally:
        bp.close()
