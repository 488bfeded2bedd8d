"""The device keyframe database against the CPU restatement (tests/kfdb_ref.py, tests/bow_ref.py):
coeb_kfdb_query (common words, list order, the word threshold, L1 scores bit for bit as float32),
the slot lifecycle (growth, erase, reuse, clear) and coeb_match_bow_kfdb (every candidate's row
equal to SearchByBoW's reference).  References are computed once per module."""
import ctypes as C
import functools

import numpy as np
import pytest

import bow_ref as R
import kfdb_ref as K

EINVAL = -22
NKF, NFEAT, MAXF = 48, 300, 1000
ERASED = (0, 5, 17, 30, 47)


# ------------------------------------------------------------------ the query
@functools.lru_cache(maxsize=None)
def query_case():
    """A vocabulary of 10 000 words (k = 10, L = 4) and 48 keyframes of 300 features.  Features are
    given their words directly (weight: the word's, node: its ancestor two levels up), the frame's
    from words below 5000:
      kf 0            the frame's own features                              (score 1)
      kf 1..5         85..97 % of the frame's words, the rest foreign        (common > min_common)
      kf 6            exactly min_common of the frame's words                (the strict >)
      kf 7..39        1..60 % of the frame's words                           (0 < common <= min_common)
      kf 40           300 features of one frame word                         (nw = 1)
      kf 41..47       foreign words only                                     (common = 0)"""
    k, L, parent, is_leaf, _, weight = R.random_voc(10, 4, seed=41)
    leaf_nodes = [i + 1 for i in range(len(parent)) if is_leaf[i]]
    assert len(leaf_nodes) == 10000

    def features(words):
        words = np.asarray(words, np.int32)
        nodes = np.array([parent[parent[leaf_nodes[w] - 1] - 1] for w in words], np.int32)
        return words, np.array([weight[leaf_nodes[w] - 1] for w in words]), nodes

    rng = np.random.RandomState(43)
    f_words = rng.randint(0, 5000, NFEAT)
    f_set = np.unique(f_words)
    foreign = lambda m: rng.randint(5000, 10000, m)                     # noqa: E731
    min_common = int(np.float32(len(f_set)) * np.float32(0.8))
    kfs = [f_words.copy()]
    for frac in (0.97, 0.94, 0.91, 0.88, 0.85):
        keep = rng.rand(NFEAT) < frac
        kfs.append(np.where(keep, f_words, foreign(NFEAT)))
    kfs.append(np.concatenate([f_set[-min_common:], foreign(NFEAT - min_common)]))
    for i in range(33):
        m = max(1, int(NFEAT * 0.6 * (i + 1) / 33))
        kfs.append(np.concatenate([rng.choice(f_words, m), foreign(NFEAT - m)]))
    kfs.append(np.full(NFEAT, f_set[3]))
    for _ in range(7):
        kfs.append(foreign(NFEAT))
    assert len(kfs) == NKF
    out = []
    for words in [f_words] + kfs:
        w, wt, nd = features(words)
        bv = K.bow_vector(w, wt, nd)
        keys = sorted(bv)
        out.append(dict(word=np.array(keys, np.int32), value=np.array([bv[x] for x in keys]), bow=bv, node=nd,
                        desc=rng.randint(0, 256, (NFEAT, 32)).astype(np.uint8),
                        angle=rng.uniform(0, 360, NFEAT).astype(np.float32)))
    return out[0], out[1:]


def _expect(r, slot_of, nslots):
    """The query's outputs from detect_reloc's result; slot_of: KeyFrame id -> slot."""
    common, score = np.zeros(nslots, np.int32), np.full(nslots, -1, np.float32)
    for kf in r["sharing"]:
        common[slot_of[kf.id]] = kf.reloc_words
    for s, kf in r["scored"]:
        score[slot_of[kf.id]] = s
    return dict(common=common, score=score, order=np.array([slot_of[kf.id] for kf in r["sharing"]], np.int32),
                max_common=r["max_common"], min_common=r["min_common"])


def _same(got, want):
    for key in ("max_common", "min_common"):
        assert got[key] == want[key], key
    for key in ("common", "order"):
        assert np.array_equal(got[key], want[key]), key
    assert got["score"].dtype == np.float32 and np.array_equal(got["score"].view(np.uint32), want["score"].view(np.uint32))


@functools.lru_cache(maxsize=None)
def query_ref():
    """The reference's results through the lifecycle: all 48, after 5 erasures, after 2 re-adds."""
    F, kfs = query_case()
    ref_kfs = [K.KeyFrame(i, kf["bow"]) for i, kf in enumerate(kfs)]
    db = K.Database()
    for kf in ref_kfs:
        db.add(kf)
    none = lambda kf: []                                                # noqa: E731
    full = K.detect_reloc(F["bow"], db, 1, none)
    for i in ERASED:
        db.erase(ref_kfs[i])
    erased = K.detect_reloc(F["bow"], db, 2, none)
    for i in (17, 0):
        db.add(ref_kfs[i])
    readded = K.detect_reloc(F["bow"], db, 3, none)
    return [dict(r, words=[kf.reloc_words for kf in r["sharing"]], ids=[kf.id for kf in r["sharing"]])
            for r in (full, erased, readded)]


def test_query_case_has_what_it_is_for():
    """Properties of the reference's own result (no GPU)."""
    F, kfs = query_case()
    full, erased, readded = query_ref()
    mn = full["min_common"]
    words = dict(zip(full["ids"], full["words"]))
    assert sum(w > mn for w in words.values()) >= 3
    assert sum(0 < w <= mn for w in words.values()) >= 3
    assert NKF - len(words) >= 2
    assert mn in words.values() and words[6] == mn
    first = [min(set(F["bow"]) & set(kfs[i]["bow"])) for i in full["ids"]]
    assert first == sorted(first) and len(set(first)) < len(first)       # equal first words: insertion decides
    assert np.float32(1.0) in [s for s, _ in full["scored"]] and len(kfs[40]["word"]) == 1 and words[40] == 1
    assert full["max_common"] == len(F["word"])
    assert not set(erased["ids"]) & set(ERASED)
    # the re-added keyframes took the slots 0 and 5 but come last among those that start at the same word
    ids = readded["ids"]
    assert first[0] == first[1] and ids.index(17) > ids.index(1) and ids.index(0) > ids.index(17)
    assert ids.index(0) == max(i for i, kf in enumerate(ids) if min(set(F["bow"]) & set(kfs[kf]["bow"])) == first[0])


def _add(db, kf):
    return db.add(kf["desc"], kf["node"], kf["angle"], kf["word"], kf["value"])


@pytest.mark.gpu
def test_query_and_lifecycle(ctx):
    from coeb_front import CoebError, KeyFrameDatabase
    F, kfs = query_case()
    full, erased, readded = query_ref()
    db = KeyFrameDatabase(ctx, max_features=MAXF, initial_slots=4)      # 48 adds: the storage doubles 4 times
    try:
        assert db.size() == (0, 0) and len(db.query(F["word"], F["value"])["order"]) == 0
        assert [_add(db, kf) for kf in kfs] == list(range(NKF)) and db.size() == (NKF, NKF)
        _same(db.query(F["word"], F["value"]), _expect(full, {i: i for i in range(NKF)}, NKF))
        for i in ERASED:
            db.erase(i)
        assert db.size() == (NKF - 5, NKF)
        _same(db.query(F["word"], F["value"]), _expect(erased, {i: i for i in range(NKF)}, NKF))
        with pytest.raises(CoebError):
            db.erase(5)                                                 # already empty
        assert [_add(db, kfs[17]), _add(db, kfs[0])] == [0, 5]          # lowest free slot first
        slot_of = {i: i for i in range(NKF)}
        slot_of[17], slot_of[0] = 0, 5
        _same(db.query(F["word"], F["value"]), _expect(readded, slot_of, NKF))
        # an empty query; a query of one word; bad arguments
        q = db.query(np.zeros(0, np.int32), np.zeros(0))
        assert len(q["order"]) == 0 and q["max_common"] == 0 and not q["common"].any() and (q["score"] == -1).all()
        with pytest.raises(CoebError, match="max_features"):
            db.query(np.arange(MAXF + 1, dtype=np.int32), np.ones(MAXF + 1))
        with pytest.raises(CoebError, match="max_features"):
            db.add(np.zeros((1, 32), np.uint8), [3], [0.0], np.arange(MAXF + 1), np.ones(MAXF + 1))
        with pytest.raises(CoebError, match="max_features"):
            db.add(np.zeros((MAXF + 1, 32), np.uint8), np.zeros(MAXF + 1), np.zeros(MAXF + 1), [1], [1.0])
        for bad in ([4, 4, 9], [9, 4], [-1, 3]):
            with pytest.raises(CoebError, match="ascending"):
                db.add(np.zeros((1, 32), np.uint8), [3], [0.0], bad, np.ones(len(bad)))
        assert db.size() == (NKF - 3, NKF)
        db.clear()
        assert db.size() == (0, 0)
        q = db.query(F["word"], F["value"])
        assert len(q["order"]) == 0 and q["max_common"] == 0 and q["min_common"] == 0
        assert _add(db, kfs[40]) == 0                                   # usable after clear
        q = db.query(F["word"], F["value"])
        assert list(q["order"]) == [0] and list(q["common"]) == [1] and (q["max_common"], q["min_common"]) == (1, 0)
        assert q["score"][0] == np.float32(K.l1_score(F["bow"], kfs[40]["bow"]))
    finally:
        db.close()


# ------------------------------------------------------------------ the batched matcher
@functools.lru_cache(maxsize=None)
def cand_case(name, n_cur):
    """The KeyFrame / frame pair of tests/test_gpu_bow.py as a frame of n_cur features and the
    candidates (keyframe features [a, b), valid mask): 1000, 500, 64, 1 and 0 features, the first
    listed twice and once more with every feature valid, 500 others with an all-zero mask."""
    import test_gpu_bow as G
    m = G.match_case(name)
    kfs = [(0, 1000), (0, 500), (0, 64), (0, 1), (0, 0), (500, 1000)]   # database keyframes, by slot
    v = m["valid"]
    cands = [(0, v), (1, v[:500]), (2, v[:64]), (3, np.ones(1, np.uint8)), (4, v[:0]), (0, v), (0, np.ones(1000, np.uint8)),
             (5, np.zeros(500, np.uint8))]
    cur = dict(desc=m["cur_desc"][:n_cur], node=m["cur_node"][:n_cur], angle=m["cur_angle"][:n_cur])
    return m, kfs, cands, cur


@functools.lru_cache(maxsize=None)
def cand_ref(name, n_cur, nnratio, check_ori):
    m, kfs, cands, cur = cand_case(name, n_cur)
    out = []
    for slot, valid in cands:
        a, b = kfs[slot]
        out.append(R.search_by_bow(valid, m["kf_desc"][a:b], m["kf_node"][a:b], m["kf_angle"][a:b], cur["desc"],
                                   cur["node"], cur["angle"], nnratio, check_ori))
    return out


@pytest.fixture(scope="module")
def match_db(ctx):
    """name -> (database holding the six keyframes of cand_case(name), its slots)"""
    from coeb_front import KeyFrameDatabase
    made = {}

    def get(name):
        if name not in made:
            m, kfs, _, _ = cand_case(name, 1000)
            db = KeyFrameDatabase(ctx, max_features=MAXF, initial_slots=2)
            w, val = np.array([1, 7], np.int32), np.array([0.25, 0.75])
            slots = [db.add(m["kf_desc"][a:b], m["kf_node"][a:b], m["kf_angle"][a:b], w, val) for a, b in kfs]
            assert slots == list(range(6))
            made[name] = db
        return made[name]
    yield get
    for db in made.values():
        db.close()


def _frame(cur):
    from coeb_front import Frame, KEYPOINT_DTYPE
    keys = np.zeros(len(cur["desc"]), KEYPOINT_DTYPE)
    keys["angle"] = cur["angle"]
    F = Frame(keys, cur["desc"])
    F.mFeatNode = np.ascontiguousarray(cur["node"], np.int32)
    return F


@pytest.mark.gpu
@pytest.mark.parametrize("name,n_cur,nnratio,check_ori",
                         [(nm, 1000, r, o) for nm in ("k10", "k2") for r in (0.75, 0.6) for o in (False, True)] +
                         [("k10", 65, 0.75, True), ("k2", 65, 0.75, True)])
def test_candidates_match_reference(match_db, name, n_cur, nnratio, check_ori):
    m, kfs, cands, cur = cand_case(name, n_cur)
    want = cand_ref(name, n_cur, nnratio, check_ori)
    # the inputs exercise what the case is for (properties of the reference's own result)
    if n_cur == 1000:
        assert sum(w[1] for w in want) >= 100 and sum(w[2]["claim_dependency"] for w in want) >= 1
        if check_ori:
            assert sum(w[2]["rot_removed"] for w in want) >= 1
        if name == "k2":
            sizes = np.bincount(m["cur_node"][m["cur_node"] >= 0])
            assert (sizes > 400).sum() == 2            # longer than a wave and than the LDS tile of 128
    else:
        assert sum(w[1] for w in want) >= 10           # 65 frame features: one wave and one lane more
    # no features / no valid feature: nothing; the same slot with another mask: another result
    assert want[4][1] == 0 and want[7][1] == 0 and not np.array_equal(want[6][0], want[0][0])
    got, nm = match_db(name).SearchByBoW([s for s, _ in cands], [v for _, v in cands], _frame(cur), nnratio, check_ori)
    assert got.shape == (len(cands), n_cur)
    for j, w in enumerate(want):
        assert nm[j] == w[1], j
        assert np.array_equal(got[j], w[0]), j
    assert np.array_equal(got[0], got[5]) and nm[0] == nm[5]           # a slot listed twice


@pytest.mark.gpu
def test_candidate_edges(ctx, match_db):
    from coeb_front import BowFrameC, CoebError, KeyFrameDatabase, lib
    m, kfs, cands, cur = cand_case("k10", 1000)
    db = match_db("k10")
    F = _frame(cur)
    got, nm = db.SearchByBoW([], [], F)                                 # ncand = 0
    assert got.shape == (0, 1000) and len(nm) == 0
    with pytest.raises(CoebError, match="256"):
        db.SearchByBoW([3] * 257, [np.ones(1, np.uint8)] * 257, F)
    got, nm = db.SearchByBoW([3] * 256, [np.ones(1, np.uint8)] * 256, F)
    want = R.search_by_bow(np.ones(1, np.uint8), m["kf_desc"][:1], m["kf_node"][:1], m["kf_angle"][:1], cur["desc"],
                           cur["node"], cur["angle"], 0.75, True)
    assert (nm == want[1]).all() and (got == want[0]).all()
    # an empty frame
    got, nm = db.SearchByBoW([0, 4], [m["valid"], m["valid"][:0]], _frame({k: v[:0] for k, v in cur.items()}))
    assert got.shape == (2, 0) and list(nm) == [0, 0]
    # an erased slot, and slots out of range, among the candidates: COEB_EINVAL, outputs untouched
    own = KeyFrameDatabase(ctx, max_features=64, initial_slots=1)
    try:
        w, val = np.array([2], np.int32), np.array([1.0])
        for _ in range(3):
            own.add(m["kf_desc"][:64], m["kf_node"][:64], m["kf_angle"][:64], w, val)
        own.erase(1)
        node = np.ascontiguousarray(cur["node"], np.int32)
        fc = BowFrameC(1000, *[C.c_void_p(a.ctypes.data) for a in (cur["desc"], node, cur["angle"])])
        valid = np.ones(64, np.uint8)
        for slots in ([0, 1, 2], [0, 3], [-1]):
            out, nmo = np.full((3, 1000), -9, np.int32), np.full(3, -9, np.int32)
            sl = np.array(slots, np.int32)
            vp = (C.c_void_p * 3)(*[valid.ctypes.data] * 3)
            rc = lib().coeb_match_bow_kfdb(own.h, sl.ctypes.data, len(slots), vp, C.byref(fc), 0.75, 1, out.ctypes.data,
                                           nmo.ctypes.data)
            assert rc == EINVAL and (out == -9).all() and (nmo == -9).all()
        got, nm = own.SearchByBoW([0, 2], [valid, valid], F)
        assert np.array_equal(got[0], got[1]) and nm[0] == nm[1]
    finally:
        own.close()
