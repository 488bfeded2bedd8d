"""coeb_kfdb_create_new_map_points on the seeded random scene of tests/newpts_cases.py (MI355X only): 6 keyframes
of 300 features against tests/newpts_ref.py, the refusals, the stereo data through slab growth from one slot,
erase and reuse, a second call on the same context after one of another size, and the database's other calls
unchanged by set_stereo."""
import numpy as np
import pytest

import newpts_cases as C
from test_gpu_newpts_directed import call, check, load, views_of

pytestmark = pytest.mark.gpu
N = C.NFEAT


@pytest.fixture(scope="module")
def scene_db(ctx):
    """One slot to begin with: the slabs double three times while keyframes with stereo data are in them."""
    from coeb_front import KeyFrameDatabase
    db = KeyFrameDatabase(ctx, max_features=N, initial_slots=1)
    assert load(db, C.random_scene()["kfs"]) == list(range(C.NKF))
    yield db
    db.close()


@pytest.mark.parametrize("only_stereo", [False, True])
def test_random_scene(scene_db, only_stereo):
    check(call(scene_db, C.random_scene(), only_stereo), C.reference(C.random_scene(), only_stereo))


def test_second_call_after_one_of_another_size(scene_db):
    c = C.random_scene()
    want = C.reference(c)
    small = dict(c, slots2=c["slots2"][3:4], F12=c["F12"][3:4], epipole=c["epipole"][3:4])
    got = call(scene_db, small, False)
    assert np.array_equal(got["match"][0], want["match"][3]) and np.array_equal(got["status"][0], want["status"][3])
    assert np.array_equal(got["first_ok"] >= 0, want["status"][3] == 1)
    check(call(scene_db, c, False), want)


def test_refusals(ctx):
    from coeb_front import CoebError, KeyFrameDatabase
    c = C.random_scene()
    kfs = c["kfs"]
    db = KeyFrameDatabase(ctx, max_features=N, initial_slots=2)
    try:
        assert load(db, kfs[:3]) == [0, 1, 2]
        two = dict(c, slots2=[1, 2], F12=c["F12"][:2], epipole=c["epipole"][:2])
        ok = call(db, two, False)
        assert ok["nmatches"].sum() > 50

        def refused(match, **kw):
            with pytest.raises(CoebError, match=match):
                call(db, dict(two, **kw), False)

        refused("repeated", slots2=[1, 1])
        refused("itself", slots2=[1, 0])
        refused("no keyframe", slots2=[1, 4])
        bad = [dict(v) for v in c["views"]]
        bad[2] = dict(bad[2], tcw=np.array([0, np.inf, 0], np.float32))
        refused("not finite", views=bad)
        bad = [dict(v) for v in c["views"]]
        bad[0] = dict(bad[0], invfx=np.float32(np.nan))
        refused("not finite", views=bad)
        with pytest.raises(CoebError, match="0..32"):
            db.create_new_map_points(0, views_of(c, [0])[0], kfs[0]["has_mp"], list(range(1, 34)), views_of(c, [1] * 33),
                                     [kfs[1]["has_mp"]] * 33, np.zeros((33, 9)), np.zeros((33, 2)))
        # a non-finite entry, a stereo feature without depth
        xy = np.stack([kfs[2]["kx"], kfs[2]["ky"]], 1)
        d = kfs[2]["depth"].copy()
        d[5] = np.nan
        with pytest.raises(CoebError, match="not finite"):
            db.set_stereo(2, xy, d)
        check(call(db, two, False), ok)                          # the refused upload changed nothing
        d = kfs[2]["depth"].copy()
        d[int(np.flatnonzero(kfs[2]["u_right"] >= 0)[0])] = 0.0
        db.set_stereo(2, xy, d)
        refused("depth <= 0")
        db.set_stereo(2, xy, kfs[2]["depth"])                    # a second call replaces the data
        check(call(db, two, False), ok)
        # a slot with geometry and without stereo data
        kf = kfs[3]
        from test_gpu_tri_directed import load as load_geometry
        assert load_geometry(db, [dict(kf)]) == [3]
        refused("stereo data", slots2=[1, 3])
        refused("stereo data", slot1=3, slots2=[1, 2])
        with pytest.raises(CoebError, match="no keyframe"):
            db.set_stereo(7, xy, d)
        # nnb == 0: fine, first_ok all -1
        got = db.create_new_map_points(0, views_of(c, [0])[0], kfs[0]["has_mp"], [], np.zeros(0, views_of(c, [0]).dtype), [],
                                       np.zeros((0, 9)), np.zeros((0, 2)))
        assert got["match"].shape == (0, N) and (got["first_ok"] == -1).all() and len(got["nmatches"]) == 0
    finally:
        db.close()


def test_erase_and_reuse_drop_the_stereo_data(ctx):
    from coeb_front import CoebError, KeyFrameDatabase
    from test_gpu_tri_directed import load as load_geometry
    c = C.random_scene()
    kfs = c["kfs"]
    db = KeyFrameDatabase(ctx, max_features=N, initial_slots=1)
    try:
        assert load(db, kfs[:3]) == [0, 1, 2]
        one = dict(c, slots2=[1], F12=c["F12"][:1], epipole=c["epipole"][:1])
        want = call(db, one, False)
        db.erase(1)
        assert load_geometry(db, [dict(kfs[1])]) == [1]          # the slot again, with geometry only
        with pytest.raises(CoebError, match="stereo data"):
            call(db, one, False)
        db.set_stereo(1, np.stack([kfs[1]["kx"], kfs[1]["ky"]], 1), kfs[1]["depth"])
        check(call(db, one, False), want)
        db.clear()
        assert load_geometry(db, [dict(k) for k in kfs[:2]]) == [0, 1]
        with pytest.raises(CoebError, match="stereo data"):
            call(db, one, False)
    finally:
        db.close()


def test_other_calls_unchanged_by_set_stereo(ctx):
    """query, SearchByBoW, search_for_triangulation and fuse_search before and after set_stereo."""
    from coeb_front import Frame, KEYPOINT_DTYPE, KeyFrameDatabase, make_camera
    from test_gpu_tri_directed import load as load_geometry
    c = C.random_scene()
    kfs = c["kfs"]
    rng = np.random.RandomState(3)
    db = KeyFrameDatabase(ctx, max_features=N, initial_slots=1)
    try:
        bows = []
        for kf in kfs:
            w = np.unique(rng.randint(0, 400, 120)).astype(np.int32)
            v = rng.uniform(0.1, 1.0, len(w))
            bows.append((w, v / v.sum()))
            s = db.add(kf["desc"], kf["node"], kf["angle"], *bows[-1])
            keys = np.zeros(N, KEYPOINT_DTYPE)
            keys["x"], keys["y"], keys["octave"] = kf["x"], kf["y"], kf["octave"]
            db.set_geometry(s, keys, kf["u_right"])
        cur = kfs[0]
        keys = np.zeros(N, KEYPOINT_DTYPE)
        F = Frame(keys, cur["desc"])
        F.mFeatNode = cur["node"]
        valids = [1 - kf["has_mp"] for kf in kfs]
        cam = make_camera(C.FX, C.FY, C.CX, C.CY, C.MBF, 640, 480)
        npt = 64
        pts = dict(valid=np.ones(npt, np.uint8), world_pos=rng.uniform(-2, 2, (npt, 3)) + [0, 0, 6.0],
                   normal=np.tile([0, 0, 1.0], (npt, 1)), max_distance=np.full(npt, 20.0), min_distance=np.full(npt, 1.0),
                   descriptor=kfs[1]["desc"][:npt])
        jobs = [dict(slot=s, Rcw=c["views"][s]["Rcw"], tcw=c["views"][s]["tcw"], Ow=c["views"][s]["Ow"]) for s in (1, 2)]

        def all_calls():
            q = db.query(*bows[2])
            m = db.SearchByBoW(list(range(C.NKF)), valids, F, 0.75, True)
            t = db.search_for_triangulation(0, cur["has_mp"], c["slots2"], [kfs[s]["has_mp"] for s in c["slots2"]], c["F12"],
                                            c["epipole"], False, True)
            f = db.fuse_search(cam, pts, jobs)
            return q, m, t, f

        q0, m0, t0, f0 = all_calls()
        for s, kf in enumerate(kfs):
            db.set_stereo(s, np.stack([kf["kx"], kf["ky"]], 1), kf["depth"])
        assert call(db, c, False)["nmatches"].sum() > 100
        q1, m1, t1, f1 = all_calls()
        for key in ("common", "order", "max_common", "min_common"):
            assert np.array_equal(q0[key], q1[key])
        assert np.array_equal(q0["score"].view(np.uint32), q1["score"].view(np.uint32)) and q0["max_common"] > 0
        assert np.array_equal(m0[0], m1[0]) and np.array_equal(m0[1], m1[1])
        assert np.array_equal(t0[0], t1[0]) and np.array_equal(t0[1], t1[1]) and t0[1].sum() > 100
        for a, b in zip(f0[0] + f0[1], f1[0] + f1[1]):
            assert np.array_equal(a, b)
    finally:
        db.close()
