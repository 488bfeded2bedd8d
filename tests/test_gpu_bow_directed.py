"""The bag-of-words kernels on the directed inputs of tests/bow_cases.py (MI355X only): the
vocabulary walk on every child count, tie and depth edge (k_bow_transform), the feature-vector
CSR on hand-made node arrays (k_bow_csr) and SearchByBoW on scenes that sit on the list-length,
lane, acceptance, claim-chain and rotation edges (k_match_bow / bow_match_node, k_bow_rot), also
through the fused coeb_track_reference_keyframe.  Everything is integer and has to equal
tests/bow_ref.py; tests/test_bow_cases.py shows without a GPU that each case reaches its edge."""
import numpy as np
import pytest

import bow_cases as B

pytestmark = pytest.mark.gpu


@pytest.fixture
def voc_ctx(ctx):
    from coeb_front import Vocabulary

    def use(name):
        v = Vocabulary.from_arrays(*B.voc_args(name))
        ctx.set_vocabulary(v)
        v.close()
        return ctx
    return use


@pytest.mark.parametrize("name", B.transform_names())
def test_transform_case(voc_ctx, name):
    voc, desc, levelsup = B.transform_case(name)
    want = B.transform_ref(name)
    got = voc_ctx(voc).bow_transform(desc, levelsup)
    for key in ("word", "node", "fv_node", "fv_off", "fv_idx", "weight"):
        assert np.array_equal(got[key], want[key]), key


def _frame(m):
    from coeb_front import Frame, KEYPOINT_DTYPE
    keys = np.zeros(len(m["cur_desc"]), KEYPOINT_DTYPE)
    keys["angle"] = m["cur_angle"]
    F = Frame(keys, m["cur_desc"])
    F.mFeatNode = np.ascontiguousarray(m["cur_node"], np.int32)
    return F


def _keyframe(m):
    from coeb_front import BowKeyFrame
    return BowKeyFrame(m["valid"], m["kf_desc"], m["kf_node"], m["kf_angle"])


@pytest.mark.parametrize("name,nnratio,check_ori", B.MATCH_RUNS, ids=lambda v: str(v))
def test_search_by_bow_scene(ctx, name, nnratio, check_ori):
    from coeb_front import ORBmatcher
    m = B.scene(name)
    want, want_nm, _, _ = B.match_ref(name, nnratio, check_ori)
    F = _frame(m)
    nm = ORBmatcher(nnratio, check_ori, ctx=ctx).SearchByBoW(_keyframe(m), F)
    assert nm == want_nm
    assert np.array_equal(F.mvpMapPoints, want)


@pytest.mark.parametrize("name,nnratio,check_ori", B.FUSED_RUNS, ids=lambda v: str(v))
def test_fused_call_takes_the_same_walk(ctx, name, nnratio, check_ori):
    """coeb_track_reference_keyframe with the node ids given and a gate no scene passes: what it
    returns is SearchByBoW's result."""
    from coeb_front import make_camera
    m = B.scene(name)
    want, want_nm, _, _ = B.match_ref(name, nnratio, check_ori)
    nkf = len(m["valid"])
    r = ctx.track_reference_keyframe(make_camera(500.0, 500.0, 320.0, 240.0, 40.0, 640, 480), _frame(m), _keyframe(m),
                                     np.zeros((nkf, 3), np.float32), np.ones(nkf, np.int32), cur_node_id=m["cur_node"],
                                     nnratio=nnratio, check_orientation=check_ori, min_matches=1 << 20)
    assert r["nmatches_bow"] == want_nm and r["ninliers_pose"] == 0
    assert np.array_equal(r["match"], want) and (r["discarded"] == -1).all()
