"""The reference of the streaming RGB-D Frame constructor (tests/stream_ref.py) on the CPU: the
conditions tests/test_gpu_rgbd_stream.py leans on, checked on the oracle's output alone."""
import numpy as np
import pytest

import stream_ref as R


@pytest.mark.parametrize("name", sorted(R.SEQUENCES))
def test_sequence_exercises_the_mask(oracle_mod, name):
    frames, boxes = R.sequence(name)
    ref = R.sequence_ref(name)
    s = R.SEQUENCES[name]
    assert frames.shape == (s["n"], s["h"], s["w"])
    # the object's box stays inside every frame
    for b in boxes:
        assert b[0, 0] >= 0 and b[0, 1] >= 0 and b[0, 2] <= s["w"] and b[0, 3] <= s["h"], b[0]
    # frame 0 is a first frame: no T_M, flags 0 (Frame.cc:205-209)
    assert ref[0]["first"] and ref[0]["n_tm"] == 0 and not ref[0]["blur"].any()
    assert not any(r["first"] for r in ref[1:])
    # at least one frame with a non-empty T_M ...
    assert max(r["n_tm"] for r in ref) > 0, [r["n_tm"] for r in ref]
    # ... and one whose masked extraction differs from the unmasked one
    ex = R.extractor(s["orb"])
    differs = 0
    for f in range(1, s["n"]):
        plain = ex.extract(frames[f])
        if len(plain["kps"]) != len(ref[f]["kps"]) or not np.array_equal(plain["desc"], ref[f]["desc"]):
            differs += 1
    assert differs >= 1
    assert all(len(r["kps"]) >= 100 for r in ref)


def test_both_blur_flags_occur(oracle_mod):
    flags = np.concatenate([r["blur"] for r in R.sequence_ref("small")[1:]])
    assert (flags == 1).any() and (flags == 0).any(), flags
    # per box: the object's is sharp, the static one lies on a smooth stretch
    for r in R.sequence_ref("small")[1:]:
        assert list(r["blur"]) == [0, 1]


def test_flat_pair_has_no_fundamental_matrix(oracle_mod):
    a, b = R.flat_pair()
    assert R.moving_points(a, b) is None
    box = np.float32([[10, 10, 60, 60]])
    depth = R.depth_map(a.shape[1], a.shape[0])
    orb = R.SEQUENCES["small"]["orb"]
    r = R.frame_ref(a, b, box, depth, orb=orb)
    assert r["n_tm"] == -1 and len(r["tm"]) == 0 and list(r["blur"]) == [1]
    # extracted without T_M: the same records as the unmasked extraction
    plain = R.extractor(orb).extract(b)
    assert np.array_equal(plain["desc"], r["desc"]) and len(plain["kps"]) == len(r["kps"])


def test_depth_maps_hold_every_hole_class(oracle_mod):
    for name, s in R.SEQUENCES.items():
        d = R.depth_map(s["w"], s["h"])
        assert (d == 0).any() and (d < 0).any() and np.isnan(d).any() and (d > 0).any()
        u = R.depth_map(s["w"], s["h"], "u16")
        assert u.dtype == np.uint16 and (u == 0).any() and (u > 0).any()
        # the holes reach keypoints: -1 entries beside valid ones in the reference
        for kind in ("f32", "u16"):
            dep = np.concatenate([r["depth"] for r in R.sequence_ref(name, kind)])
            assert (dep == -1).sum() >= 10 and (dep > 0).sum() >= 100, (name, kind)
        r = R.sequence_ref(name)[1]
        assert ((r["u_right"] == -1) == (r["depth"] == -1)).all()
