"""Bag-of-words front end on the GPU against the CPU reference (tests/bow_ref.py): k_bow_transform
and the feature-vector CSR (coeb_bow_transform, coeb_bow_batch_device) and SearchByBoW
(coeb_match_bow).  Everything is integer: word ids, node ids, the CSR, the matches and their
count must be identical.  The references are computed once per module."""
import functools

import numpy as np
import pytest

import bow_ref as R
from bow_cases import depths as _depths


@functools.lru_cache(maxsize=None)
def voc_case(name):
    """-> (args of the vocabulary, reference Voc, levelsup)"""
    if name == "k10":
        args = R.random_voc(10, 3, seed=5)
        assert len(args[2]) == 1110
        return args, R.Voc(*args), 1
    if name == "k3_ragged":
        args = R.random_voc(3, 6, seed=8, ragged=True, zero_weight=0.1)
        return args, R.Voc(*args), 4
    if name == "k20":
        args = R.random_voc(20, 2, seed=9)
        return args, R.Voc(*args), 1
    if name == "k2":
        args = R.random_voc(2, 2, seed=10)
        return args, R.Voc(*args), 1
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def desc_case(name):
    args, ref, _ = voc_case(name)
    rng = np.random.RandomState(21)
    d = rng.randint(0, 256, (1000, 32)).astype(np.uint8)
    copies = args[4][rng.choice(len(args[4]), 50, replace=len(args[4]) < 50)]      # exact node descriptors: distance 0
    return np.concatenate([d, copies])


@functools.lru_cache(maxsize=None)
def bow_ref_case(name, levelsup, n):
    _, ref, _ = voc_case(name)
    return R.compute_bow(ref, desc_case(name)[:n], levelsup)


@pytest.fixture
def voc_ctx(ctx):
    """The session context with a vocabulary set by name (set_vocabulary replaces the tables)."""
    from coeb_front import Vocabulary

    def use(name):
        v = Vocabulary.from_arrays(*voc_case(name)[0])
        ctx.set_vocabulary(v)
        v.close()                      # the context keeps nothing of it
        return ctx
    return use


def _check_transform(got, want):
    for key in ("word", "node", "fv_node", "fv_off", "fv_idx"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(got["weight"], want["weight"])


@pytest.mark.gpu
def test_transform_before_set_vocabulary_is_an_error():
    from coeb_front import CoebError, Context
    c = Context(max_width=640, max_height=480, max_batch=1)
    try:
        with pytest.raises(CoebError, match="no vocabulary"):
            c.bow_transform(np.zeros((4, 32), np.uint8))
        with pytest.raises(CoebError, match="no vocabulary"):
            c.bow_batch_device(4)
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["k10", "k3_ragged", "k20"])
def test_transform_matches_reference(voc_ctx, name):
    c = voc_ctx(name)
    _, ref, levelsup = voc_case(name)
    n = len(desc_case(name))
    want = bow_ref_case(name, levelsup, n)
    _check_transform(c.bow_transform(desc_case(name), levelsup), want)
    if name == "k3_ragged":
        # the inputs reach what the case is for: leaves at depth 2 = nid_level (nid is the leaf),
        # nodes with one child, words of weight 0
        leaves = [ref.word_node[w] for w in want["word"]]
        depth = _depths(ref)
        assert any(depth[nd] == 2 and want["node"][i] == nd for i, nd in enumerate(leaves))
        assert (want["node"] < 0).sum() > 10 and min(len(ch) for ch in ref.children if ch) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name,levelsup", [("k10", 3), ("k10", 7), ("k20", 2), ("k10", 0), ("k3_ragged", 2)])
def test_transform_levelsup_edges(voc_ctx, name, levelsup):
    c = voc_ctx(name)
    want = bow_ref_case(name, levelsup, 200)
    ref = voc_case(name)[1]
    if levelsup >= ref.L:
        assert set(want["node"]) == {0} and list(want["fv_node"]) == [0]
    if name == "k3_ragged":            # leaves above nid_level = 4: nid is defined as that leaf
        depth = _depths(ref)
        leaves = [ref.word_node[w] for w in want["word"]]
        assert any(depth[nd] < ref.L - levelsup and want["node"][i] == nd for i, nd in enumerate(leaves))
    _check_transform(c.bow_transform(desc_case(name)[:200], levelsup), want)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_transform_small_counts(voc_ctx, n):
    c = voc_ctx("k3_ragged")
    got = c.bow_transform(desc_case("k3_ragged")[:n], 4)
    _check_transform(got, bow_ref_case("k3_ragged", 4, n))
    assert len(got["word"]) == n and len(got["fv_off"]) == len(got["fv_node"]) + 1


@pytest.mark.gpu
def test_batch_transform_matches_single_frame(voc_ctx):
    from coeb_front import synth
    c = voc_ctx("k10")
    w, h, F = 640, 480, 3
    frames = np.stack(synth.make_frames(w, h, F, seed=1200))
    frames[1] = 128                                  # a flat frame: no keypoints
    dg = c.upload(frames)
    try:
        c.extract_batch_device(dg.ptr, F, w, h)
        c.bow_batch_device(1)
        d_kps, d_desc, d_counts, kcap = c.batch_results()
        counts = c.download(d_counts, F * 4, np.int32)
        desc = c.download(d_desc, F * kcap * 32).reshape(F, kcap, 32)
        d_word, d_node = c.batch_bow_results()
        word = c.download(d_word, F * kcap * 4, np.int32).reshape(F, kcap)
        node = c.download(d_node, F * kcap * 4, np.int32).reshape(F, kcap)
    finally:
        dg.free()
    assert counts[1] == 0 and counts[0] > 100 and counts[2] > 100
    for f in range(F):
        single = c.bow_transform(desc[f, :counts[f]], 1)
        assert np.array_equal(word[f, :counts[f]], single["word"])
        assert np.array_equal(node[f, :counts[f]], single["node"])
        assert (word[f, counts[f]:] == -1).all() and (node[f, counts[f]:] == -1).all()
    # ... and the single-frame call against the reference on real descriptors
    ref = voc_case("k10")[1]
    want = R.compute_bow(ref, desc[0, :200], 1)
    _check_transform(c.bow_transform(desc[0, :200], 1), want)


# ------------------------------------------------------------------ SearchByBoW
@functools.lru_cache(maxsize=None)
def match_case(name):
    """KeyFrame and frame of 1000 features: the frame's descriptors are a permutation of the
    KeyFrame's with <= 20 flipped bits, 15 % replaced by noise; a third of the KeyFrame's
    descriptors come in families of near copies, so that features compete for the same frame
    feature (claim order, second-best ratio, exact ties).  Angles share one rotation, 10 %
    scattered; 30 % of the KeyFrame features are invalid."""
    _, ref, levelsup = voc_case(name)
    rng = np.random.RandomState(77)
    n = 1000
    kf = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    fam = n // 3
    for i in range(fam):                             # features fam + i and 2 fam + i: near copies of feature i
        src = kf[i]
        for j in (fam + i, 2 * fam + i):
            v = src.copy()
            for b in rng.choice(256, rng.randint(0, 7), replace=False):
                v[b >> 3] ^= 1 << (b & 7)
            kf[j] = v
    perm = rng.permutation(n)
    cur = kf[perm].copy()
    for i in range(n):
        for b in rng.choice(256, rng.randint(0, 21), replace=False):
            cur[i, b >> 3] ^= 1 << (b & 7)
    noise = rng.rand(n) < 0.15
    cur[noise] = rng.randint(0, 256, (int(noise.sum()), 32)).astype(np.uint8)
    kf_angle = rng.uniform(0, 360, n).astype(np.float32)
    cur_angle = np.mod(kf_angle[perm] - np.float32(47.0), 360).astype(np.float32)
    scat = rng.rand(n) < 0.10
    cur_angle[scat] = rng.uniform(0, 360, int(scat.sum())).astype(np.float32)
    cur_angle[cur_angle >= 360] = 0
    valid = (rng.rand(n) >= 0.30).astype(np.uint8)
    kf_node = R.compute_bow(ref, kf, levelsup)["node"]
    cur_node = R.compute_bow(ref, cur, levelsup)["node"]
    return dict(valid=valid, kf_desc=kf, kf_node=kf_node, kf_angle=kf_angle, cur_desc=cur, cur_node=cur_node,
                cur_angle=cur_angle)


@functools.lru_cache(maxsize=None)
def match_ref(name, nnratio, check_ori):
    m = match_case(name)
    return R.search_by_bow(m["valid"], m["kf_desc"], m["kf_node"], m["kf_angle"], m["cur_desc"], m["cur_node"],
                           m["cur_angle"], nnratio, check_ori)


def _gpu_match(ctx, valid, kf_desc, kf_node, kf_angle, cur_desc, cur_node, cur_angle, nnratio, check_ori):
    from coeb_front import BowKeyFrame, Frame, KEYPOINT_DTYPE, ORBmatcher
    keys = np.zeros(len(cur_desc), KEYPOINT_DTYPE)
    keys["angle"] = cur_angle
    F = Frame(keys, cur_desc)
    F.mFeatNode = np.ascontiguousarray(cur_node, np.int32)
    kf = BowKeyFrame(valid, kf_desc, kf_node, kf_angle)
    nm = ORBmatcher(nnratio, check_ori, ctx=ctx).SearchByBoW(kf, F)
    return F.mvpMapPoints, nm


@pytest.mark.gpu
@pytest.mark.parametrize("check_ori", [False, True])
@pytest.mark.parametrize("nnratio", [0.7, 0.6])
@pytest.mark.parametrize("name", ["k10", "k2"])
def test_search_by_bow_matches_reference(ctx, name, nnratio, check_ori):
    m = match_case(name)
    want, want_nm, st = match_ref(name, nnratio, check_ori)
    # the inputs exercise what the case is for (properties of the reference's own result)
    assert want_nm >= 100 and st["claim_dependency"] >= 1 and st["tie_rejected"] >= 1
    if check_ori:
        assert st["rot_removed"] >= 1
    if name == "k2":
        sizes = np.bincount(m["cur_node"][m["cur_node"] >= 0])
        assert (sizes > 400).sum() == 2              # longer than a wave and than the LDS tile of 128
    got, nm = _gpu_match(ctx, m["valid"], m["kf_desc"], m["kf_node"], m["kf_angle"], m["cur_desc"], m["cur_node"],
                         m["cur_angle"], nnratio, check_ori)
    assert nm == want_nm
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_search_by_bow_hand_worked(ctx):
    import test_bow_ref as T
    for check_ori, want, want_nm in ((False, [0, -1, 1, 3, -1, -1, -1, 6], 4), (True, [0, -1, 1, -1, -1, -1, -1, 6], 3)):
        got, nm = _gpu_match(ctx, T.KF_VALID, np.array(T.KF_DESC), T.KF_NODE, T.KF_ANGLE, np.array(T.CUR_DESC),
                             T.CUR_NODE, T.CUR_ANGLE, 0.7, check_ori)
        assert list(got) == want and nm == want_nm


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["empty_kf", "empty_frame", "no_common_node", "all_invalid", "all_minus_one"])
def test_search_by_bow_degenerate(ctx, case):
    m = {k: v[:200].copy() for k, v in match_case("k10").items()}
    if case == "empty_kf":
        for k in ("valid", "kf_desc", "kf_node", "kf_angle"):
            m[k] = m[k][:0]
    elif case == "empty_frame":
        for k in ("cur_desc", "cur_node", "cur_angle"):
            m[k] = m[k][:0]
    elif case == "no_common_node":
        m["cur_node"] = m["cur_node"] + 100000
    elif case == "all_invalid":
        m["valid"][:] = 0
    else:
        m["kf_node"][:] = -1
        m["cur_node"][:] = -1
    args = (m["valid"], m["kf_desc"], m["kf_node"], m["kf_angle"], m["cur_desc"], m["cur_node"], m["cur_angle"])
    want, want_nm, _ = R.search_by_bow(*args, 0.7, True)
    got, nm = _gpu_match(ctx, *args, 0.7, True)
    assert want_nm == 0 and nm == 0 and len(got) == len(want) and (got == -1).all()
