"""SearchForTriangulation over the device keyframe database on a random scene (MI355X only):
6 keyframes of 300 features over a k = 10, L = 4 vocabulary, about half of the features with
MapPoints, stereo and mono mixed, for only_stereo x check_orientation against tests/tri_ref.py;
the refusals; geometry through slab growth, erase and reuse; and the database's other calls
unchanged by set_geometry."""
import functools

import numpy as np
import pytest

import bow_ref as R
import tri_cases as C
import tri_ref as T
from test_gpu_tri_directed import load

pytestmark = pytest.mark.gpu
NKF, N, NBASE = 6, 300, 260


@functools.lru_cache(maxsize=None)
def scene():
    """260 scene points (descriptor, image point, angle); 40 of them share their descriptor with
    another (equal distances inside a node).  A keyframe sees a random 300 of them (with repeats),
    each with up to 14 flipped bits, its point moved by up to a few pixels along y (the epipolar
    lines are close to y2 = y1) and its angle by a few degrees, plus 30 whole-bin outliers."""
    rng = np.random.RandomState(77)
    voc = R.Voc(*R.random_voc(10, 4, seed=9, zero_weight=0.05))
    base_d = rng.randint(0, 256, (NBASE, 32)).astype(np.uint8)
    base_d[220:] = base_d[:40]
    base_xy = np.stack([rng.uniform(20, 620, NBASE), rng.uniform(20, 460, NBASE)], 1)
    base_a = rng.uniform(0, 360, NBASE)
    kfs = []
    for k in range(NKF):
        src = rng.randint(0, NBASE, N)
        d = np.unpackbits(base_d[src], axis=1)
        for i in range(N):
            d[i, rng.choice(256, rng.randint(0, 15), replace=False)] ^= 1
        d = np.packbits(d, axis=1)
        xy = base_xy[src] + np.stack([rng.uniform(-30, 30, N), rng.choice([0.0, 0.5, 1.5, 2.5, 6.0], N)], 1)
        ang = (base_a[src] + 40.0 * k + rng.uniform(-6, 6, N)) % 360.0
        out = rng.choice(N, 30, replace=False)
        ang[out] = (ang[out] + rng.choice([60.0, 120.0, 200.0], 30)) % 360.0
        stereo = rng.rand(N) < 0.5
        node = np.array([voc.transform(x, 3)[2] if voc.transform(x, 3)[1] > 0 else -1 for x in d], np.int32)
        kfs.append(dict(desc=d, node=node, x=xy[:, 0].astype(np.float32), y=xy[:, 1].astype(np.float32),
                        octave=rng.randint(0, 8, N).astype(np.int32), angle=ang.astype(np.float32),
                        u_right=np.where(stereo, xy[:, 0] - 4.0, -1.0).astype(np.float32),
                        has_mp=(rng.rand(N) < 0.5).astype(np.uint8)))
    slots2 = [1, 2, 3, 4, 5]
    F12 = np.array([C.LINE_Y + rng.uniform(-1, 1, (3, 3)) * [[1e-5, 1e-5, 1e-3]] * 3 for _ in slots2], np.float32)
    # the epipole next to a mono feature of the neighbour
    epi = []
    for s in slots2:
        i = int(np.flatnonzero(kfs[s]["u_right"] < 0)[7])
        epi.append((kfs[s]["x"][i] + 3.0, kfs[s]["y"][i] + 1.0))
    return dict(kfs=kfs, slot1=0, slots2=slots2, F12=F12, epipole=np.array(epi, np.float32), only_stereo=False,
                check_ori=True, mutants=())


@functools.lru_cache(maxsize=None)
def scene_ref(only_stereo, check_ori):
    return C.reference(scene(), only_stereo=only_stereo, check_ori=check_ori)


@pytest.fixture(scope="module")
def scene_db(ctx):
    """One slot to begin with: the slabs double three times while keyframes with geometry are in them."""
    from coeb_front import KeyFrameDatabase
    db = KeyFrameDatabase(ctx, max_features=N, initial_slots=1)
    assert load(db, scene()["kfs"]) == list(range(NKF))
    yield db
    db.close()


def _search(db, c, only_stereo, check_ori, slot1=None, slots2=None):
    slot1 = c["slot1"] if slot1 is None else slot1
    slots2 = c["slots2"] if slots2 is None else slots2
    return db.search_for_triangulation(slot1, c["kfs"][c["slot1"]]["has_mp"], slots2,
                                       [c["kfs"][s]["has_mp"] for s in c["slots2"]], c["F12"], c["epipole"], only_stereo,
                                       check_ori)


def test_scene_exercises_the_rules():
    """Properties of the model's own result."""
    c = scene()
    k1, tr = c["kfs"][0], []
    for j, s2 in enumerate(c["slots2"]):
        T.search_for_triangulation(k1, c["kfs"][s2], k1["has_mp"], c["kfs"][s2]["has_mp"], c["F12"][j], c["epipole"][j],
                                   C.SCALE, C.SIGMA2, False, False, trace=tr)
    what = [w for _, _, w in tr]
    assert what.count("accepted") >= 100 and what.count("line") >= 30 and what.count("epipole") >= 1
    assert what.count("has_mp") >= 1000
    plain, ori = scene_ref(False, False), scene_ref(False, True)
    assert plain[1].min() >= 10 and 0 < (plain[1] - ori[1]).sum() and ori[1].min() >= 8
    assert 0 < scene_ref(True, False)[1].sum() < plain[1].sum()


@pytest.mark.parametrize("check_ori", [False, True])
@pytest.mark.parametrize("only_stereo", [False, True])
def test_random_scene(scene_db, only_stereo, check_ori):
    want, want_nm = scene_ref(only_stereo, check_ori)
    got, nm = _search(scene_db, scene(), only_stereo, check_ori)
    assert nm.tolist() == want_nm.tolist()
    assert np.array_equal(got, want)


def test_one_neighbour_calls_equal_the_batched_call(scene_db):
    c = scene()
    want, want_nm = scene_ref(False, True)
    for j, s2 in enumerate(c["slots2"]):
        got, nm = scene_db.search_for_triangulation(0, c["kfs"][0]["has_mp"], [s2], [c["kfs"][s2]["has_mp"]],
                                                    c["F12"][j:j + 1], c["epipole"][j:j + 1], False, True)
        assert nm.tolist() == [want_nm[j]] and np.array_equal(got[0], want[j])


def test_refusals(ctx, scene_db):
    from coeb_front import CoebError, KeyFrameDatabase
    c = scene()
    kf = c["kfs"][0]
    db = KeyFrameDatabase(ctx, max_features=N, initial_slots=2)
    try:
        s0, s1 = load(db, c["kfs"][:2])
        s2 = db.add(kf["desc"], kf["node"], kf["angle"], np.zeros(0, np.int32), np.zeros(0))      # no geometry
        args = (c["F12"][:1], c["epipole"][:1], False, True)
        with pytest.raises(CoebError, match="geometry"):
            db.search_for_triangulation(s0, kf["has_mp"], [s2], [kf["has_mp"]], *args)
        with pytest.raises(CoebError, match="geometry"):
            db.search_for_triangulation(s2, kf["has_mp"], [s1], [c["kfs"][1]["has_mp"]], *args)
        db.erase(s1)
        with pytest.raises(CoebError, match="no keyframe"):
            db.search_for_triangulation(s0, kf["has_mp"], [s1], [c["kfs"][1]["has_mp"]], *args)
        with pytest.raises(CoebError, match="no keyframe"):
            db.search_for_triangulation(s0, kf["has_mp"], [7], [c["kfs"][1]["has_mp"]], *args)
        from coeb_front import KEYPOINT_DTYPE
        keys = np.zeros(N, KEYPOINT_DTYPE)
        with pytest.raises(CoebError, match="no keyframe"):
            db.set_geometry(s1, keys, kf["u_right"])
        with pytest.raises(CoebError, match="0..32"):
            db.search_for_triangulation(s0, kf["has_mp"], [s0] * 33, [kf["has_mp"]] * 33, np.zeros((33, 9)),
                                        np.zeros((33, 2)), False, True)
        # an octave outside the pyramid
        keys["octave"][N - 1] = C.NLEVELS
        with pytest.raises(CoebError, match="octave"):
            db.set_geometry(s2, keys, kf["u_right"])
        # nnb == 0: fine, nothing to write
        got, nm = db.search_for_triangulation(s0, kf["has_mp"], [], [], np.zeros((0, 9)), np.zeros((0, 2)), False, True)
        assert got.shape == (0, N) and len(nm) == 0
    finally:
        db.close()


def test_erase_and_reuse_need_geometry_again(ctx):
    from coeb_front import CoebError, KeyFrameDatabase
    c = scene()
    db = KeyFrameDatabase(ctx, max_features=N, initial_slots=1)
    try:
        assert load(db, c["kfs"][:3]) == [0, 1, 2]
        db.erase(1)
        kf = c["kfs"][4]
        assert db.add(kf["desc"], kf["node"], kf["angle"], np.zeros(0, np.int32), np.zeros(0)) == 1
        args = (c["F12"][3:4], c["epipole"][3:4], False, True)
        with pytest.raises(CoebError, match="geometry"):
            db.search_for_triangulation(0, c["kfs"][0]["has_mp"], [1], [kf["has_mp"]], *args)
        from coeb_front import KEYPOINT_DTYPE
        keys = np.zeros(N, KEYPOINT_DTYPE)
        keys["x"], keys["y"], keys["octave"] = kf["x"], kf["y"], kf["octave"]
        wrong = keys.copy()
        wrong["y"] += 50.0
        db.set_geometry(1, wrong, kf["u_right"])
        got, nm = db.search_for_triangulation(0, c["kfs"][0]["has_mp"], [1], [kf["has_mp"]], *args)
        assert nm[0] < scene_ref(False, True)[1][3]
        db.set_geometry(1, keys, kf["u_right"])             # a second call replaces the data
        got, nm = db.search_for_triangulation(0, c["kfs"][0]["has_mp"], [1], [kf["has_mp"]], *args)
        assert nm[0] == scene_ref(False, True)[1][3] and np.array_equal(got[0], scene_ref(False, True)[0][3])
        db.clear()
        assert load(db, c["kfs"][:1]) == [0]
        with pytest.raises(CoebError, match="no keyframe"):
            db.search_for_triangulation(0, c["kfs"][0]["has_mp"], [1], [kf["has_mp"]], *args)
    finally:
        db.close()


def test_other_calls_unchanged_by_set_geometry(ctx):
    """coeb_kfdb_query and coeb_match_bow_kfdb before and after set_geometry on the same database."""
    from coeb_front import Frame, KEYPOINT_DTYPE, KeyFrameDatabase
    c = scene()
    rng = np.random.RandomState(3)
    db = KeyFrameDatabase(ctx, max_features=N, initial_slots=1)
    try:
        bows = []
        for kf in c["kfs"]:
            w = np.unique(rng.randint(0, 400, 120)).astype(np.int32)
            v = rng.uniform(0.1, 1.0, len(w))
            bows.append((w, v / v.sum()))
            db.add(kf["desc"], kf["node"], kf["angle"], *bows[-1])
        cur = c["kfs"][0]
        keys = np.zeros(N, KEYPOINT_DTYPE)
        keys["angle"] = cur["angle"]
        F = Frame(keys, cur["desc"])
        F.mFeatNode = cur["node"]
        valids = [1 - kf["has_mp"] for kf in c["kfs"]]

        def both():
            q = db.query(*bows[2])
            m = db.SearchByBoW(list(range(NKF)), valids, F, 0.75, True)
            return q, m

        q0, m0 = both()
        for s, kf in enumerate(c["kfs"]):
            k = np.zeros(N, KEYPOINT_DTYPE)
            k["x"], k["y"], k["octave"] = kf["x"], kf["y"], kf["octave"]
            db.set_geometry(s, k, kf["u_right"])
        _search(db, c, False, True)
        q1, m1 = both()
        assert q0["max_common"] == q1["max_common"] > 0 and q0["min_common"] == q1["min_common"]
        for key in ("common", "order"):
            assert np.array_equal(q0[key], q1[key])
        assert np.array_equal(q0["score"].view(np.uint32), q1["score"].view(np.uint32))
        assert np.array_equal(m0[0], m1[0]) and np.array_equal(m0[1], m1[1]) and m0[1].sum() > 50
    finally:
        db.close()
