"""The host-array calls that keep their inputs and their results in one staged region, at the sizes where
a region's layout can go wrong: coeb_bow_transform, coeb_match_bow, coeb_kfdb_query, coeb_match_bow_kfdb,
coeb_match_localmap and coeb_match_keyframe (MI355X only).  Every result is an integer (or a float32
compared by its bits) and must equal the Python models' (tests/bow_ref.py, tests/kfdb_ref.py,
tests/match_ref.py).

Feature counts of 0, 1, 3, 5 and 17: n, 4 n and 32 n are no multiples of the region's 16-byte step, and
max(n, 1) differs from n.  A count below 4 cannot fill a fourth rotation bin, so "some matches found, some
removed by the rotation filter" is asserted of every case that has at least 5 features on both sides, and
of each family as a whole (test_cases_are_not_trivial, no GPU needed).

Not covered: a raised device error word behind coeb_match_localmap.  The word's only writers the
projection searches can reach are the n >= 4096 guards of their kernels, and the host refuses 4096
keypoints before anything is launched; no existing test raises the word through this call either."""
import ctypes as C
import functools

import numpy as np
import pytest

import bow_ref as R
import kfdb_ref as K
import match_ref as mr
import test_gpu_bow as GB
import test_gpu_kfdb as GK
from chain_util import TUM, cameras

SIZES = (0, 1, 3, 5, 17)
VOC, LEVELSUP = "k3_ragged", 4


# ------------------------------------------------------------------ SearchByBoW inputs
@functools.lru_cache(maxsize=None)
def bow_pair(nq, n, seed=0):
    """A keyframe of nq and a frame of n features in two nodes: frame feature j is keyframe feature
    perm[j] with up to 8 bits flipped (j < min(nq, n)), the others are noise; the rotation between a
    matched pair is 10 + 60 (j % 6) degrees, so five matches fall into five bins; keyframe feature 1 is
    invalid."""
    rng = np.random.RandomState(1000 + 97 * nq + n + seed)
    kf = rng.randint(0, 256, (nq, 32)).astype(np.uint8)
    cur = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    kf_node, cur_node = (np.arange(nq) % 2 + 7).astype(np.int32), np.zeros(n, np.int32)
    kf_angle, cur_angle = np.zeros(nq, np.float32), rng.uniform(0, 360, n).astype(np.float32)
    perm = rng.permutation(nq)
    for j in range(min(nq, n)):
        i = perm[j]
        cur[j] = kf[i]
        for b in rng.choice(256, rng.randint(0, 9), replace=False):
            cur[j, b >> 3] ^= 1 << (b & 7)
        cur_node[j] = kf_node[i]
        kf_angle[i] = 350
        cur_angle[j] = 340 - 60 * (j % 6)
    cur_node[min(nq, n):] = 7
    valid = np.ones(nq, np.uint8)
    valid[1:2] = 0
    return dict(valid=valid, kf_desc=kf, kf_node=kf_node, kf_angle=kf_angle, cur_desc=cur, cur_node=cur_node,
                cur_angle=cur_angle)


def _args(m):
    return (m["valid"], m["kf_desc"], m["kf_node"], m["kf_angle"], m["cur_desc"], m["cur_node"], m["cur_angle"])


@functools.lru_cache(maxsize=None)
def bow_pair_ref(nq, n, check_ori):
    return R.search_by_bow(*_args(bow_pair(nq, n)), 0.75, check_ori)


# ------------------------------------------------------------------ the database's candidates
DB_KFS = (5, 17, 0, 5)                  # features of the keyframes in slots 0..3
CAND_SETS = ((0,), (1,), (0, 1, 3), (1, 2, 0))


@functools.lru_cache(maxsize=None)
def db_case():
    """One frame of 5 features (a match row is 20 bytes) and the keyframes of the slots 0..3: each holds
    near copies of the frame's features at shuffled indices, rotated by 10 + 60 i degrees, the rest noise;
    an odd slot's copy of frame feature 1 is invalid."""
    rng = np.random.RandomState(77)
    cur = dict(cur_desc=rng.randint(0, 256, (5, 32)).astype(np.uint8), cur_node=np.array([7, 8, 7, 8, 7], np.int32),
               cur_angle=(340 - 60 * np.arange(5)).astype(np.float32))
    kfs = []
    for j, nq in enumerate(DB_KFS):
        kf = dict(valid=np.ones(nq, np.uint8), kf_desc=rng.randint(0, 256, (nq, 32)).astype(np.uint8),
                  kf_node=rng.randint(7, 9, nq).astype(np.int32), kf_angle=rng.uniform(0, 360, nq).astype(np.float32))
        perm = rng.permutation(nq)
        for i in range(min(nq, 5)):
            d = cur["cur_desc"][i].copy()
            for b in rng.choice(256, rng.randint(0, 9), replace=False):
                d[b >> 3] ^= 1 << (b & 7)
            kf["kf_desc"][perm[i]], kf["kf_node"][perm[i]], kf["kf_angle"][perm[i]] = d, cur["cur_node"][i], 350
            if i == 1 and j % 2:
                kf["valid"][perm[i]] = 0
        kfs.append(kf)
    return kfs, cur


@functools.lru_cache(maxsize=None)
def db_ref(slots, n_cur, check_ori=True):
    pairs, cur = db_case()
    return [R.search_by_bow(pairs[s]["valid"], pairs[s]["kf_desc"], pairs[s]["kf_node"], pairs[s]["kf_angle"],
                            cur["cur_desc"][:n_cur], cur["cur_node"][:n_cur], cur["cur_angle"][:n_cur], 0.75, check_ori)
            for s in slots]


# ------------------------------------------------------------------ the database's query
QUERIES = {"one": {4: 1.0}, "three": {2: 0.25, 4: 0.5, 9: 0.25}, "foreign": {100: 0.5, 101: 0.5}}


@functools.lru_cache(maxsize=None)
def query_case(nslots):
    """nslots keyframes whose BowVectors share the words 2, 4 and 9 with the queries to different
    degrees; the middle one is erased.  -> (bows, the reference's result per query)"""
    rng = np.random.RandomState(50 + nslots)
    bows = []
    for j in range(nslots):
        words = sorted(set([4] + ([2, 9] if j % 2 == 0 else [9]) + list(rng.randint(10, 40, 3))))
        v = rng.uniform(0.1, 1.0, len(words))
        bows.append(dict(zip(words, v / v.sum())))
    kfs = [K.KeyFrame(j, b) for j, b in enumerate(bows)]
    db = K.Database()
    for kf in kfs:
        db.add(kf)
    db.erase(kfs[nslots // 2])
    slot_of = {j: j for j in range(nslots)}
    # a query's result is read before the next query overwrites the keyframes' mnRelocWords
    return bows, {name: GK._expect(K.detect_reloc(q, db, fid, lambda kf: []), slot_of, nslots)
                  for fid, (name, q) in enumerate(sorted(QUERIES.items()), 1)}


# ------------------------------------------------------------------ the projection searches
def proj_layout(cam, n, nq):
    """Query q at (40 + 30 q, 100); keypoint i one pixel to its right while both exist, further keypoints
    and queries far from everything.  The rotation between a matched pair is 10 + 60 (i % 6) degrees."""
    lay = mr.Layout(cam)
    for q in range(nq):
        lay.query(40 + 30 * q, 100, bits=0, angle=350.0)
    for i in range(n):
        if i < nq:
            u, v = lay.pix(i)
            lay.kp(u + 1, v, bits=1 + i % 4, angle=340.0 - 60 * (i % 6), held=3 if i == 2 else 0)
        else:
            lay.kp(40 + 30 * i, 400, bits=200)
    return mr._three("ragged-%d-%d" % (n, nq), lay, 5, {}, check_ori=True, only=("local", "kf"))


@pytest.fixture(scope="module")
def cams(oracle_mod):
    return cameras(oracle_mod, oracle_mod.Extractor(), 640, 480, TUM)


@pytest.fixture(scope="module")
def proj_scenes(cams):
    """Every (keypoints, points) pair of SIZES for both searches; a scene keeps its model's result."""
    return [s for n in SIZES for nq in SIZES for s in proj_layout(cams[0], n, nq)]


# ------------------------------------------------------------------ the references' own results (no GPU)
def test_cases_are_not_trivial(cams, proj_scenes):
    nm = removed = 0
    for nq in SIZES:
        for n in SIZES:
            _, m, st = bow_pair_ref(nq, n, True)
            nm, removed = nm + m, removed + st["rot_removed"]
            if min(nq, n) >= 5:
                assert m >= 2 and st["rot_removed"] >= 1, (nq, n)
            assert bow_pair_ref(nq, n, False)[1] == m + st["rot_removed"]
    assert nm >= 20 and removed >= 10
    for slots in CAND_SETS:
        want = db_ref(slots, 5)
        assert sum(w[1] for w in want) >= 2 and sum(w[2]["rot_removed"] for w in want) >= 1, slots
        assert all(w[1] == 0 for s, w in zip(slots, want) if DB_KFS[s] == 0)
    for ns in (1, 3, 5):
        _, want = query_case(ns)
        assert not want["foreign"]["common"].any() and len(want["foreign"]["order"]) == 0
        if ns > 1:
            assert want["one"]["max_common"] == 1 and want["three"]["max_common"] == 3
            assert (want["three"]["score"] >= 0).any() and (want["three"]["score"] < 0).any()
            assert want["three"]["common"][ns // 2] == 0                    # the erased slot
        else:
            assert not want["three"]["common"].any()
    by = {m: [s.model(cams[0]) for s in proj_scenes if s.matcher == m] for m in ("local", "kf")}
    assert sum(r[0] for r in by["local"]) >= 20 and sum(r[0] for r in by["kf"]) >= 20
    # the keyframe search's rotation filter removed some: without it the same scenes match more
    plain = sum(mr.py_search_keyframe(cams[0], s.inputs["kps"], s.inputs["desc"], s.inputs["cur_has"], s.inputs["kf"],
                                      s.inputs["T"], s.kw["th"], s.kw["orb_dist"], False)[0]
                for s in proj_scenes if s.matcher == "kf")
    assert plain >= sum(r[0] for r in by["kf"]) + 10


# ------------------------------------------------------------------ on the device
def _frame(desc, node, angle):
    from coeb_front import Frame, KEYPOINT_DTYPE
    keys = np.zeros(len(desc), KEYPOINT_DTYPE)
    keys["angle"] = angle
    F = Frame(keys, desc)
    F.mFeatNode = np.ascontiguousarray(node, np.int32)
    return F


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_match_bow_ragged(ctx, n):
    for nq in SIZES:
        for check_ori in (True, False):
            want, want_nm, _ = bow_pair_ref(nq, n, check_ori)
            got, nm = GB._gpu_match(ctx, *_args(bow_pair(nq, n)), 0.75, check_ori)
            assert nm == want_nm and len(got) == n and np.array_equal(got, want), (nq, n, check_ori)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_bow_transform_ragged(ctx, n):
    from coeb_front import Vocabulary, lib
    c, v = ctx, Vocabulary.from_arrays(*GB.voc_case(VOC)[0])
    c.set_vocabulary(v)
    v.close()
    desc = np.ascontiguousarray(GB.desc_case(VOC)[:n])
    want = GB.bow_ref_case(VOC, LEVELSUP, n)
    GB._check_transform(c.bow_transform(desc, LEVELSUP), want)
    # without the feature-vector outputs, and with the ids alone
    m = max(n, 1)
    word, node, weight = np.full(m, -7, np.int32), np.full(m, -7, np.int32), np.full(m, -7.0)
    vp = lambda a: C.c_void_p(a.ctypes.data)                            # noqa: E731
    for outs in ((word, node, weight), (word, None, None)):
        rc = lib().coeb_bow_transform(c.h, vp(desc) if n else None, n, LEVELSUP, *[None if o is None else vp(o) for o in outs],
                                      None, None, None, 0, None)
        assert rc == 0
    assert np.array_equal(word[:n], want["word"]) and np.array_equal(node[:n], want["node"])
    assert np.array_equal(weight[:n], want["weight"])
    assert (word[n:] == -7).all() and (node[n:] == -7).all() and (weight[n:] == -7).all()


@pytest.fixture(scope="module")
def small_db(ctx):
    from coeb_front import KeyFrameDatabase
    pairs, _ = db_case()
    db = KeyFrameDatabase(ctx, max_features=32, initial_slots=1)
    w, val = np.array([1, 7], np.int32), np.array([0.25, 0.75])
    assert [db.add(p["kf_desc"], p["kf_node"], p["kf_angle"], w, val) for p in pairs] == list(range(len(pairs)))
    yield db
    db.close()


@pytest.mark.gpu
@pytest.mark.parametrize("slots", CAND_SETS + ((0, 1, 2),))
def test_match_bow_kfdb_ragged(small_db, slots):
    pairs, cur = db_case()
    for n_cur in ((5, 0) if slots == (0, 1, 2) else (5,)):
        want = db_ref(slots, n_cur)
        F = _frame(cur["cur_desc"][:n_cur], cur["cur_node"][:n_cur], cur["cur_angle"][:n_cur])
        got, nm = small_db.SearchByBoW(list(slots), [pairs[s]["valid"] for s in slots], F, 0.75, True)
        assert got.shape == (len(slots), n_cur)
        for j, w in enumerate(want):
            assert nm[j] == w[1] and np.array_equal(got[j], w[0]), (slots, n_cur, j)


@pytest.mark.gpu
@pytest.mark.parametrize("nslots", [1, 3, 5])
def test_kfdb_query_ragged(ctx, nslots):
    from coeb_front import KeyFrameDatabase
    bows, want = query_case(nslots)
    db = KeyFrameDatabase(ctx, max_features=8, initial_slots=1)
    try:
        for b in bows:
            words = sorted(b)
            db.add(np.zeros((1, 32), np.uint8), [0], [0.0], np.array(words, np.int32), np.array([b[w] for w in words]))
        db.erase(nslots // 2)
        assert db.size() == (nslots - 1, nslots)
        for name, q in QUERIES.items():
            words = sorted(q)
            GK._same(db.query(np.array(words, np.int32), np.array([q[w] for w in words])), want[name])
    finally:
        db.close()


@pytest.mark.gpu
def test_results_larger_than_the_page_locked_minimum():
    """70 candidates of 4095 features against a 4095-feature frame as the first call of a fresh context:
    the match rows and counts take 70 * 4096 * 4 bytes = 1.15 MB, more than the page-locked buffer's 1 MiB
    minimum, the inputs 0.45 MB.  Every row must be what coeb_match_bow gives on a second context; a small
    call on the first context follows."""
    from coeb_front import Context, KeyFrameDatabase
    N, NC = 4095, 70
    rng = np.random.RandomState(9)
    desc = rng.randint(0, 256, (N, 32)).astype(np.uint8)
    node = rng.randint(0, 900, N).astype(np.int32)
    angle = rng.uniform(0, 360, N).astype(np.float32)
    perm = rng.permutation(N)
    cur = desc[perm].copy()
    cur[:, 0] ^= 1
    words, vals = np.array([1], np.int32), np.array([1.0])
    valids = [(rng.rand(N) < 0.5 + 0.005 * j).astype(np.uint8) for j in range(NC)]
    a, b = Context(max_width=640, max_height=480, max_batch=1), Context(max_width=640, max_height=480, max_batch=1)
    try:
        db = KeyFrameDatabase(a, max_features=N, initial_slots=1)
        assert db.add(desc, node, angle, words, vals) == 0
        cur_node = node[perm]                                           # a frame feature lies in its source's node
        got, nm = db.SearchByBoW([0] * NC, valids, _frame(cur, cur_node, angle), 0.75, True)
        assert nm.min() >= 100 and len({int(x) for x in nm}) >= 10
        for j in range(NC):
            row, n1 = GB._gpu_match(b, valids[j], desc, node, angle, cur, cur_node, angle, 0.75, True)
            assert n1 == nm[j] and np.array_equal(row, got[j]), j
        small = bow_pair(5, 5)
        row, n1 = GB._gpu_match(a, *_args(small), 0.75, True)
        assert n1 == bow_pair_ref(5, 5, True)[1] and np.array_equal(row, bow_pair_ref(5, 5, True)[0])
        db.close()
    finally:
        a.close()
        b.close()


def _gpu_scene(ctx, cam, s):
    import coeb_front
    i, k = s.inputs, s.kw
    if s.matcher == "local":
        F = coeb_front.Frame(i["kps"], i["desc"], i["ur"])
        F.mvpMapPointObs = i["cur_obs"].copy()
        mp = i["mp"]
        lm = coeb_front.LocalMap(mp["in_view"], mp["proj_x"], mp["proj_y"], mp["proj_xr"], mp["level"], mp["view_cos"],
                                 mp["descriptor"], mp["observations"])
        return coeb_front.ORBmatcher(k["nnratio"], ctx=ctx).SearchByProjection(F, lm, k["th"], camera=cam), F.mvpMapPoints
    F = coeb_front.Frame(i["kps"], i["desc"], Tcw=i["T"])
    F.mvpMapPoints = np.where(i["cur_has"] > 0, 10 ** 6, -1).astype(np.int32)
    kf = i["kf"]
    kp = coeb_front.KeyFramePoints(kf["valid"], kf["world_pos"], kf["descriptor"], kf["max_distance"], kf["min_distance"],
                                   kf["angle"])
    nm = coeb_front.ORBmatcher(0.75, k["check_ori"], ctx=ctx).SearchByProjection(F, kp, set(), k["th"], k["orb_dist"], cam)
    return nm, np.where(F.mvpMapPoints == 10 ** 6, -1, F.mvpMapPoints)


@pytest.mark.gpu
@pytest.mark.parametrize("matcher", ["local", "kf"])
def test_projection_searches_ragged(ctx, cams, proj_scenes, matcher):
    for s in proj_scenes:
        if s.matcher == matcher:
            want_nm, want = s.model(cams[0])
            nm, got = _gpu_scene(ctx, cams[1], s)
            assert nm == want_nm and np.array_equal(got, want), s.name
