"""The device-batch tracking chain off 640x480 and off the default image bounds (MI355X only).

tests/test_gpu_batch_depth.py runs the chain at one geometry: 640x480 frames, whose bases in the
packed batch are 256-byte aligned and whose LK levels are whole dwords, and the image bounds of
an undistorted image, inside which every keypoint has a grid cell.  Here the same bit-for-bit
comparison (chain_util._check_chain) runs

  * at 427x321 (427 * 321 = 3 mod 4: the six frame bases fall on all four byte alignments) and
    333x251 (odd too, pitch 333): pmo_batch's pair stride w * h under k_gf_response, k_subpix,
    k_pyr_down, k_sharr, k_lk and k_fm, k_prep's depth at f * w * h floats with pitch w, and the
    extraction of a batch whose frames are not dword aligned;
  * with the image bounds a distorted camera gives: inside the image (keypoints fail PosInGrid in
    the matchers' phase 0, search windows start past the last grid column, projections are
    rejected at min_x / max_x) and outside it (the grid inverse is not 64 / w).

F = 6 everywhere.  Every coverage condition is computed from the ORACLE's results
(chain_util.assert_coverage_*), never from device output; tests/test_oracle_kat.py asserts the
same conditions without a GPU.  The raw RGB-D conversion is not run at the ragged sizes:
coeb_rgbd_preprocess_batch_device takes widths that are a multiple of 4 only, and
test_rgbd_preprocess_batch_matches_oracle covers it.
"""
import numpy as np
import pytest

import chain_util as cu
from test_gpu_parity import keyframe_both, localmap_both, match_both

pytestmark = pytest.mark.gpu

F = cu.SHAPES_F
_oracle = {}


@pytest.fixture(scope="module")
def ex(oracle_mod):
    return oracle_mod.Extractor()


def scenario(name, w, h):
    key = (name, w, h)
    if key not in _oracle:
        _oracle[key] = getattr(cu, "scenario_" + name)(w, h, F)
    return _oracle[key]


def oracle_chain(oracle_mod, ex, name, w, h, bounds, stride):
    """(extractions, per-frame oracle results) of a scenario under a camera, computed once."""
    key = (name, w, h, bounds, stride)
    if key not in _oracle:
        isg = np.array(ex.p.inv_sigma2[:8], np.float32)
        _oracle[key] = cu.run_oracle(oracle_mod, ex, scenario(name, w, h), stride, isg, intr=cu.intrinsics(w, h),
                                     bounds=bounds)
    return _oracle[key]


def pipeline(oracle_mod, ex, w, h, bounds=None):
    from coeb_front.pipeline import BatchPipeline
    cam_o, cam = cu.cameras(oracle_mod, ex, w, h, bounds=bounds)
    bp = BatchPipeline(w, h, F, camera=cam)
    assert np.array_equal(np.array(bp.ctx.tables().inv_sigma2[:8], np.float32), np.array(ex.p.inv_sigma2[:8], np.float32))
    return bp, cam_o


def run_checked(bp, oracle_mod, ex, name, w, h, bounds=None, **kw):
    """One step, synchronised, then the whole chain against the oracle."""
    bp.run(track=True, **kw)
    bp.synchronize()
    stride = bp.ctx.batch_results()[3]
    ext, res = oracle_chain(oracle_mod, ex, name, w, h, bounds, stride)
    states, tr = cu._check_chain(bp, ext, res, F)
    return ext, res, stride, states, tr


@pytest.mark.parametrize("w,h", cu.RAGGED_SIZES)
def test_chain_ragged_sizes(oracle_mod, ex, w, h):
    """The holes chain with frames w * h bytes apart, w * h odd: every frame tracked on >= 300
    motion-model matches and >= 5 local-map matches, single step and three steps back to back."""
    s = scenario("holes", w, h)
    bp, _ = pipeline(oracle_mod, ex, w, h)
    try:
        bp.load(s["frames"], depth=s["depth"], Tcw=s["Tcw"])
        ext, res, _, states, tr = run_checked(bp, oracle_mod, ex, "holes", w, h, nkf=2)
        cu.assert_coverage_ragged(res)
        assert states == [2] * (F - 1)
        for _ in range(3):
            bp.run(track=True, nkf=2)
        bp.synchronize()
        tr2 = bp.track_results()
        assert tr2["ninliers"] == tr["ninliers"] and tr2["nlocal"] == tr["nlocal"]
        assert np.array_equal(tr2["T"][1:].view(np.uint32), tr["T"][1:].view(np.uint32))
        cu._check_chain(bp, ext, res, F)
    finally:
        bp.close()


def test_frame_ctor_ragged_size(oracle_mod, ex):
    """The whole loop with the RGB-D Frame constructor at 427x321: per frame T_M (None versus
    empty included), the blur flags and every field of the masked extraction against the oracle
    run frame by frame, then the chain.  >= 3 pairs have a non-empty T_M and T_M points lie
    inside a box, so the mask removes keypoints."""
    w, h = cu.RAGGED_SIZES[0]
    s = scenario("frame_ctor", w, h)
    nb = len(s["boxes"][0])
    bp, _ = pipeline(oracle_mod, ex, w, h)
    try:
        bp.load(s["frames"], Tcw=s["Tcw"])
        bp.set_frame_boxes(s["boxes"])
        bp.run(frame=True, track=True)
        bp.synchronize()
        stride = bp.ctx.batch_results()[3]
        ext, res = oracle_chain(oracle_mod, ex, "frame_ctor", w, h, None, stride)
        cu.assert_coverage_frame_ctor(ext, s["boxes"])
        out, _, _ = bp.results()
        tms, flags = bp.ctx.batch_frame_results(F, nb * F)
        for f in range(F):
            e = ext[f]
            if e["tm"] is None:
                assert tms[f] is None, f
            else:
                assert tms[f] is not None and np.array_equal(tms[f], e["tm"]), f
            assert np.array_equal(flags[nb * f:nb * f + nb], e["blur"]), f
            for name in e["kps"].dtype.names:
                assert np.array_equal(out[f][0][name], e["kps"][name]), (f, name)
            assert np.array_equal(out[f][1], e["desc"]), f
        cu._check_chain(bp, ext, res, F)
    finally:
        bp.close()


@pytest.mark.parametrize("w,h,bounds,inside", cu.BOUNDED)
def test_chain_image_bounds(oracle_mod, ex, w, h, bounds, inside):
    """The holes chain under a camera whose image bounds are not (0, w, 0, h).  The oracle's
    matches differ from the default-bounds run of the same input, so a device that ignored the
    bounds, or took the grid inverse from the image size, fails; bounds inside the image leave
    >= 10 keypoints of some frame without a grid cell."""
    s = scenario("holes", w, h)
    bp, cam_o = pipeline(oracle_mod, ex, w, h, bounds)
    try:
        bp.load(s["frames"], depth=s["depth"], Tcw=s["Tcw"])
        ext, res, stride, states, _ = run_checked(bp, oracle_mod, ex, "holes", w, h, bounds, nkf=2)
        _, res_default = oracle_chain(oracle_mod, ex, "holes", w, h, None, stride)
        cu.assert_coverage_bounds(cam_o, ext, res, res_default, inside)
    finally:
        bp.close()


def test_single_frame_matchers_image_bounds(ctx, oracle_mod, ex):
    """coeb_match_lastframe, coeb_match_localmap and coeb_match_keyframe, one call each, with the
    640x480 camera whose bounds lie inside the image; each oracle result differs from the
    default camera's."""
    r1, ur1, last = cu.matcher_pair(oracle_mod, ex)
    mp, kf = cu.matcher_scene(last)
    cams = cu.cameras(oracle_mod, ex, 640, 480, cu.TUM, cu.BOUNDS_INSIDE)
    default = cu.oracle_matchers(oracle_mod, cu.cameras(oracle_mod, ex, 640, 480, cu.TUM)[0], r1, ur1, last, mp, kf)
    cu.assert_coverage_matchers(cu.oracle_matchers(oracle_mod, cams[0], r1, ur1, last, mp, kf), default)
    Tc = cu.synth.motion_pose()
    match_both(ctx, oracle_mod, ex, r1["kps"], r1["desc"], ur1, last, Tc, np.eye(4, dtype=np.float32), cams=cams)
    localmap_both(ctx, oracle_mod, ex, r1["kps"], r1["desc"], ur1, None, mp, cams=cams)
    keyframe_both(ctx, oracle_mod, ex, r1["kps"], r1["desc"], None, kf, Tc, cams=cams)
