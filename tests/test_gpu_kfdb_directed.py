"""The device keyframe database on the directed inputs of tests/bow_cases.py (MI355X only):
coeb_kfdb_query on keyframes whose words and common words sit on the 64-word blocks of
k_kfdb_common / k_kfdb_score, on both sides of minCommonWords, on every arrangement of scored
waves in a workgroup, on a score whose float32 bits depend on the order of the double sum, and
through growth, erase, reuse and clear from one slot; coeb_match_bow_kfdb (k_match_bow_db) on a
scene whose result depends on skipping an invalid KeyFrame feature inside the walk.  Everything
has to equal tests/kfdb_ref.py / tests/bow_ref.py, the score as float32 bits."""
import numpy as np
import pytest

import bow_cases as B

pytestmark = pytest.mark.gpu


def _same(got, want):
    for key in ("max_common", "min_common"):
        assert got[key] == want[key], key
    for key in ("common", "order"):
        assert np.array_equal(got[key], want[key]), key
    assert got["score"].dtype == np.float32 and np.array_equal(got["score"].view(np.uint32), want["score"].view(np.uint32))


def _bow(b):
    keys = sorted(b)
    return np.array(keys, np.int32), np.array([b[k] for k in keys], np.float64)


@pytest.mark.parametrize("name", B.query_names())
def test_query_case(ctx, name):
    from coeb_front import KeyFrameDatabase
    slots, ops = B.query_case(name)
    want = B.query_ref(name)
    db = KeyFrameDatabase(ctx, max_features=B.MAXF, initial_slots=slots)
    none = np.zeros(0, np.int32)
    try:
        for i, (op, w) in enumerate(zip(ops, want)):
            if op[0] == "add":
                assert db.add(np.zeros((0, 32), np.uint8), none, np.zeros(0, np.float32), *_bow(op[1])) == w, i
            elif op[0] == "erase":
                db.erase(op[1])
            elif op[0] == "clear":
                db.clear()
            else:
                assert db.size()[1] == len(w["common"]), i
                _same(db.query(*_bow(op[1])), w)
    finally:
        db.close()


@pytest.fixture(scope="module")
def scene_db(ctx):
    from coeb_front import KeyFrameDatabase
    kfs, _, _, _ = B.db_scene()
    db = KeyFrameDatabase(ctx, max_features=B.MAXF, initial_slots=1)
    w, val = np.array([3], np.int32), np.array([1.0])
    assert [db.add(kf["desc"], kf["node"], kf["angle"], w, val) for kf in kfs] == [0, 1, 2]
    yield db
    db.close()


@pytest.mark.parametrize("check_ori", [True, False])
@pytest.mark.parametrize("nnratio", [0.75, 0.6])
@pytest.mark.parametrize("which", ["main", "one", "most"])
def test_candidates(scene_db, which, nnratio, check_ori):
    from coeb_front import Frame, KEYPOINT_DTYPE
    _, cur, cands, _ = B.db_scene()
    want = B.db_match_ref(which, nnratio, check_ori)
    keys = np.zeros(len(cur["desc"]), KEYPOINT_DTYPE)
    keys["angle"] = cur["angle"]
    F = Frame(keys, cur["desc"])
    F.mFeatNode = np.ascontiguousarray(cur["node"], np.int32)
    got, nm = scene_db.SearchByBoW([s for s, _ in cands[which]], [v for _, v in cands[which]], F, nnratio, check_ori)
    assert got.shape == (len(want), len(cur["desc"]))
    for j, w in enumerate(want):
        assert nm[j] == w[1], j
        assert np.array_equal(got[j], w[0]), j
