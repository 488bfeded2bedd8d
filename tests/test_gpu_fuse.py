"""The Fuse search over the device keyframe database on a random scene (MI355X only): 6 keyframes of
300 features with true poses, stereo and mono mixed, against tests/fuse_ref.py; a 4095-feature
keyframe for the grid build; the refusals; the grid kept across calls and rebuilt after erase and
reuse, set_geometry, other bounds and slab growth; and the database's other calls unchanged."""
import functools

import numpy as np
import pytest

import fuse_ref as F
from test_gpu_fuse_directed import check_tables, load

pytestmark = pytest.mark.gpu
NKF, N, NP = 6, 300, 320
f32 = np.float32
CAM = F.Cam(fx=517.3, fy=516.5, cx=318.6, cy=255.3, bf=40.0)


def _rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
            np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def make_scene(seed, nkf, n, npts, cam):
    """World points in front of nkf nearby cameras.  A keyframe's features are the projections of the
    points it sees (noise of a pixel or so, some 3 px off), at the octave its distance predicts or one
    next to it, half of them stereo; descriptors are the point's with up to 60 bits flipped."""
    rng = np.random.RandomState(seed)
    X = np.stack([rng.uniform(-2.5, 2.5, npts), rng.uniform(-1.8, 1.8, npts), rng.uniform(3.0, 9.0, npts)], 1)
    desc = rng.randint(0, 256, (npts, 32)).astype(np.uint8)
    maxd = (np.linalg.norm(X, axis=1) * 1.2 ** rng.uniform(-1.5, 6.5, npts)).astype(f32)
    pts = dict(valid=(rng.rand(npts) < 0.95).astype(np.uint8), world_pos=X.astype(f32),
               normal=(-X / np.linalg.norm(X, axis=1)[:, None] * -1).astype(f32), max_distance=maxd,
               min_distance=(maxd / 1.2 ** 7).astype(f32), descriptor=desc)
    kfs, poses = [], []
    for k in range(nkf):
        R = _rot(*rng.uniform(-0.04, 0.04, 3)).astype(f32)
        t = rng.uniform(-0.3, 0.3, 3).astype(f32)
        Ow = (-R.astype(np.float64).T @ t.astype(np.float64)).astype(f32)
        Pc = X @ R.astype(np.float64).T + t
        u, v = cam.fx * Pc[:, 0] / Pc[:, 2] + cam.cx, cam.fy * Pc[:, 1] / Pc[:, 2] + cam.cy
        src = rng.randint(0, npts, n)
        noise = rng.normal(0, 0.7, (n, 2)) + (rng.rand(n, 1) < 0.15) * rng.uniform(-4, 4, (n, 2))
        dist = np.linalg.norm(X[src] - Ow, axis=1)
        lvl = np.clip(np.ceil(np.log(maxd[src] / dist) / np.log(1.2)) - rng.choice([0, 0, 0, 1, 2, -1], n), 0, 7)
        d = np.unpackbits(desc[src], axis=1)
        for i in range(n):
            d[i, rng.choice(256, rng.choice([0, 5, 20, 45, 60]), replace=False)] ^= 1
        x, y = (u[src] + noise[:, 0]).astype(f32), (v[src] + noise[:, 1]).astype(f32)
        stereo = rng.rand(n) < 0.5
        ur = np.where(stereo, x - float(cam.bf) / Pc[src, 2] + rng.normal(0, 0.5, n), -1.0).astype(f32)
        kfs.append(dict(x=x, y=y, octave=lvl.astype(np.int32), u_right=ur, desc=np.packbits(d, axis=1)))
        poses.append((R, t, Ow))
    return dict(cam=cam, kfs=kfs, pts=pts, poses=poses)


@functools.lru_cache(maxsize=None)
def scene():
    return make_scene(11, NKF, N, NP, CAM)


@functools.lru_cache(maxsize=None)
def scene_ref():
    sc, out, traces = scene(), [], []
    for kf, (R, t, Ow) in zip(sc["kfs"], sc["poses"]):
        tr = []
        out.append(F.fuse_search(kf, sc["cam"], R, t, Ow, sc["pts"], 3.0, traces=tr))
        traces += tr
    return out, traces


def jobs(sc, slots, which=None, **kw):
    which = range(len(slots)) if which is None else which
    return [dict(slot=slots[k], Rcw=sc["poses"][k][0], tcw=sc["poses"][k][1], Ow=sc["poses"][k][2], **kw) for k in which]


@pytest.fixture(scope="module")
def scene_db(ctx):
    """One slot to begin with: the slabs double three times."""
    from coeb_front import KeyFrameDatabase
    db = KeyFrameDatabase(ctx, max_features=N, initial_slots=1)
    assert load(db, scene()["kfs"]) == list(range(NKF))
    yield db
    db.close()


def same(got, want):
    return all(np.array_equal(g, w[0]) for g, w in zip(got[0], want)) and \
        all(np.array_equal(g, w[1]) for g, w in zip(got[1], want))


def test_random_scene(ctx, scene_db):
    sc = scene()
    check_tables(ctx, sc["cam"])
    want, _ = scene_ref()
    slots = list(range(NKF))
    assert same(scene_db.fuse_search(sc["cam"].tuple(), sc["pts"], jobs(sc, slots)), want)
    # again (the grids are kept), job by job, and over sub-ranges with skip bytes
    assert same(scene_db.fuse_search(sc["cam"].tuple(), sc["pts"], jobs(sc, slots)), want)
    for k in (0, 5):
        assert same(scene_db.fuse_search(sc["cam"].tuple(), sc["pts"], jobs(sc, slots, [k])), want[k:k + 1])
    skip = (np.arange(100) % 3 == 0).astype(np.uint8)
    gi, gd = scene_db.fuse_search(sc["cam"].tuple(), sc["pts"], jobs(sc, slots, [2], first=50, count=100, skip=skip))
    wi, wd = want[2][0][50:150].copy(), want[2][1][50:150].copy()
    wi[skip == 1], wd[skip == 1] = -1, 256
    assert np.array_equal(gi[0], wi) and np.array_equal(gd[0], wd)


def test_grid_of_4095_features(ctx):
    from coeb_front import KeyFrameDatabase
    sc = make_scene(5, 1, 4095, 300, CAM)
    (R, t, Ow), kf = sc["poses"][0], sc["kfs"][0]
    want = F.fuse_search(kf, sc["cam"], R, t, Ow, sc["pts"], 3.0)
    assert (want[0] >= 0).sum() >= 50
    db = KeyFrameDatabase(ctx, max_features=4095, initial_slots=1)
    try:
        slots = load(db, sc["kfs"])
        assert same(db.fuse_search(sc["cam"].tuple(), sc["pts"], jobs(sc, slots)), [want])
    finally:
        db.close()


def test_refusals(ctx):
    from coeb_front import CoebError, KeyFrameDatabase
    sc = scene()
    cam, pts = sc["cam"].tuple(), sc["pts"]
    db = KeyFrameDatabase(ctx, max_features=N, initial_slots=2)
    try:
        s0, s1 = load(db, sc["kfs"][:2])
        kf = sc["kfs"][2]
        s2 = db.add(kf["desc"], np.full(N, -1, np.int32), np.zeros(N, f32), np.zeros(0, np.int32), np.zeros(0))
        with pytest.raises(CoebError, match="geometry"):
            db.fuse_search(cam, pts, jobs(sc, [s0, s1, s2]))
        db.erase(s1)
        with pytest.raises(CoebError, match="no keyframe"):
            db.fuse_search(cam, pts, jobs(sc, [s0, s1]))
        with pytest.raises(CoebError, match="no keyframe"):
            db.fuse_search(cam, pts, [dict(jobs(sc, [s0])[0], slot=9)])
        with pytest.raises(CoebError, match="no keyframe"):
            db.fuse_search(cam, pts, [dict(jobs(sc, [s0])[0], slot=-1)])
        with pytest.raises(CoebError, match="0..128"):
            db.fuse_search(cam, pts, jobs(sc, [s0]) * 129)
        for first, count in ((0, NP + 1), (NP, 1), (-1, 2), (3, -1)):
            with pytest.raises(CoebError, match="range"):
                db.fuse_search(cam, pts, jobs(sc, [s0], first=first, count=count))
        for key, val, what in (("world_pos", np.nan, "non-finite"), ("normal", np.inf, "non-finite"),
                               ("min_distance", 0.0, "distance range"), ("max_distance", np.inf, "distance range"),
                               ("max_distance", 1e-9, "distance range")):
            bad = {k: v.copy() for k, v in pts.items()}
            i = int(np.flatnonzero(bad["valid"])[3])
            bad[key][i] = val
            with pytest.raises(CoebError, match=what):
                db.fuse_search(cam, bad, jobs(sc, [s0]))
            bad["valid"][i] = 0                                 # the same values on an invalid point are not read
            db.fuse_search(cam, bad, jobs(sc, [s0]))
        with pytest.raises(CoebError, match="bounds"):
            db.fuse_search(cam[:5] + (0.0, 0.0, 0.0, 480.0), pts, jobs(sc, [s0]))
        with pytest.raises(CoebError, match="th"):
            db.fuse_search(cam, pts, jobs(sc, [s0]), th=-1.0)
        with pytest.raises(CoebError, match="pose"):
            db.fuse_search(cam, pts, [dict(jobs(sc, [s0])[0], tcw=[np.nan, 0, 0])])
        from coeb_front import lib
        import ctypes as ct
        assert lib().coeb_kfdb_fuse_search(db.h, None, None, None, 0, ct.c_float(3.0), None, None) == -22   # missing arrays
        # more pairs than COEB_FUSE_MAX_PAIRS: 128 jobs over a list of 8193 invalid points
        big = dict(valid=np.zeros(8193, np.uint8), world_pos=np.zeros((8193, 3), f32), normal=np.zeros((8193, 3), f32),
                   max_distance=np.ones(8193, f32), min_distance=np.ones(8193, f32), descriptor=np.zeros((8193, 32), np.uint8))
        with pytest.raises(CoebError, match="rc=-34"):
            db.fuse_search(cam, big, jobs(sc, [s0]) * 128)
        # nothing to do: fine
        assert db.fuse_search(cam, pts, []) == ([], [])
        gi, gd = db.fuse_search(cam, pts, jobs(sc, [s0, s0], count=0))
        assert [len(a) for a in gi] == [0, 0]
    finally:
        db.close()


def test_grid_is_rebuilt_when_its_inputs_change(ctx):
    from coeb_front import KEYPOINT_DTYPE, KeyFrameDatabase
    sc = scene()
    cam, pts = sc["cam"], sc["pts"]
    want, _ = scene_ref()
    db = KeyFrameDatabase(ctx, max_features=N, initial_slots=1)
    try:
        assert load(db, sc["kfs"][:1]) == [0]
        assert same(db.fuse_search(cam.tuple(), pts, jobs(sc, [0])), want[:1])
        assert load(db, sc["kfs"][1:4]) == [1, 2, 3]            # the slabs grow under the built grid of slot 0
        assert same(db.fuse_search(cam.tuple(), pts, jobs(sc, [0, 1, 2, 3])), want[:4])
        # erase and reuse: slot 1 takes keyframe 4, searched with keyframe 4's pose
        db.erase(1)
        assert load(db, [sc["kfs"][4]]) == [1]
        j = jobs(sc, [0, 0, 0, 0, 1], [4])
        assert same(db.fuse_search(cam.tuple(), pts, j), want[4:5])
        # set_geometry again: every feature moved far away, then back
        kf = sc["kfs"][4]
        keys = np.zeros(N, KEYPOINT_DTYPE)
        keys["x"], keys["y"], keys["octave"] = kf["x"] + 200.0, kf["y"], kf["octave"]
        db.set_geometry(1, keys, kf["u_right"])
        moved = dict(kf, x=(kf["x"] + f32(200.0)).astype(f32))
        R, t, Ow = sc["poses"][4]
        assert same(db.fuse_search(cam.tuple(), pts, j), [F.fuse_search(moved, cam, R, t, Ow, pts, 3.0)])
        keys["x"] = kf["x"]
        db.set_geometry(1, keys, kf["u_right"])
        assert same(db.fuse_search(cam.tuple(), pts, j), want[4:5])
        # other bounds: another grid, other cells, and another IsInImage
        cam2 = F.Cam(fx=517.3, fy=516.5, cx=318.6, cy=255.3, bf=40.0, min_x=100.0, max_x=541.0, min_y=60.0, max_y=401.0)
        w2 = [F.fuse_search(sc["kfs"][k], cam2, *sc["poses"][k], pts, 3.0) for k in (0, 2)]
        assert not np.array_equal(w2[0][1], want[0][1])
        assert same(db.fuse_search(cam2.tuple(), pts, jobs(sc, [0, 0, 2], [0, 2])), w2)
        assert same(db.fuse_search(cam.tuple(), pts, jobs(sc, [0, 0, 2], [0, 2])), [want[0], want[2]])
        db.clear()
        assert load(db, sc["kfs"][5:6]) == [0]
        assert same(db.fuse_search(cam.tuple(), pts, jobs(sc, [0] * 6, [5])), want[5:6])
    finally:
        db.close()


def test_other_calls_unchanged_by_fuse(ctx):
    """query, match_bow_kfdb and search_triangulation before and after fuse calls on the same database."""
    from coeb_front import Frame, KEYPOINT_DTYPE, KeyFrameDatabase
    sc = scene()
    rng = np.random.RandomState(3)
    db = KeyFrameDatabase(ctx, max_features=N, initial_slots=1)
    try:
        bows, nodes = [], []
        for kf in sc["kfs"]:
            w = np.unique(rng.randint(0, 400, 120)).astype(np.int32)
            v = rng.uniform(0.1, 1.0, len(w))
            bows.append((w, v / v.sum()))
            nodes.append(rng.randint(0, 12, N).astype(np.int32))
            s = db.add(kf["desc"], nodes[-1], np.zeros(N, f32), *bows[-1])
            keys = np.zeros(N, KEYPOINT_DTYPE)
            keys["x"], keys["y"], keys["octave"] = kf["x"], kf["y"], kf["octave"]
            db.set_geometry(s, keys, kf["u_right"])
        cur = sc["kfs"][0]
        Fr = Frame(np.zeros(N, KEYPOINT_DTYPE), cur["desc"])
        Fr.mFeatNode = nodes[0]
        valids = [np.ones(N, np.uint8)] * NKF
        F12 = np.array([[[0, 0, 0], [0, 0, -1], [0, 1, 0]]] * 2, f32)
        has = np.zeros(N, np.uint8)

        def others():
            q = db.query(*bows[2])
            m = db.SearchByBoW(list(range(NKF)), valids, Fr, 0.75, True)
            t = db.search_for_triangulation(0, has, [1, 2], [has, has], F12, np.full((2, 2), 5000.0, f32), False, False)
            return q, m, t

        q0, m0, t0 = others()
        want, _ = scene_ref()
        assert same(db.fuse_search(sc["cam"].tuple(), sc["pts"], jobs(sc, list(range(NKF)))), want)
        q1, m1, t1 = others()
        assert same(db.fuse_search(sc["cam"].tuple(), sc["pts"], jobs(sc, list(range(NKF)))), want)
        assert q0["max_common"] == q1["max_common"] > 0 and q0["min_common"] == q1["min_common"]
        for key in ("common", "order"):
            assert np.array_equal(q0[key], q1[key])
        assert np.array_equal(q0["score"].view(np.uint32), q1["score"].view(np.uint32))
        assert np.array_equal(m0[0], m1[0]) and np.array_equal(m0[1], m1[1]) and m0[1].sum() > 20
        assert np.array_equal(t0[0], t1[0]) and np.array_equal(t0[1], t1[1])
    finally:
        db.close()
