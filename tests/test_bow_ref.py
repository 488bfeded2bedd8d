"""Pins tests/bow_ref.py (the CPU reference of the bag-of-words calls) on a vocabulary and a
SearchByBoW case small enough to work by hand; every expected value below is written out."""
import numpy as np

import bow_ref as R


def D(**bytes_at):
    d = np.zeros(32, np.uint8)
    for k, v in bytes_at.items():
        d[int(k[1:])] = v
    return d


# k = 2, L = 2.  node: 1 (inner, zeros)  2 (inner, 16 bits)  3, 4 under 1   5, 6 under 2
PARENT = [0, 0, 1, 1, 2, 2]
LEAF = [0, 0, 1, 1, 1, 1]
DESC = [D(), D(b0=0xFF, b1=0xFF), D(b31=0x0F), D(b31=0xF0), D(b0=0xFF, b1=0xFF, b2=0xFF), D(b0=0xFF, b1=0xFF, b3=0xFF)]
WEIGHT = [0, 0, 1.0, 2.0, 0.0, 3.0]


def hand_voc():
    return R.Voc(2, 2, PARENT, LEAF, DESC, WEIGHT)


def test_hamming_is_descriptor_distance(oracle_mod):
    rng = np.random.RandomState(1)
    a, b = rng.randint(0, 256, (20, 32)).astype(np.uint8), rng.randint(0, 256, (20, 32)).astype(np.uint8)
    for i in range(20):
        assert int(R.hamming(a[i], b[i])) == oracle_mod.descriptor_distance(a[i], b[i])
    assert list(R.hamming(a[0], b)) == [oracle_mod.descriptor_distance(a[0], b[i]) for i in range(20)]


def test_text_round_trip_and_shape():
    text = R.voc_text(2, 2, PARENT, LEAF, DESC, WEIGHT)
    k, L, parent, leaf, desc, weight = R.parse_text(text)
    assert (k, L, parent, leaf, weight) == (2, 2, PARENT, LEAF, WEIGHT)
    assert np.array_equal(desc, np.array(DESC))
    v = hand_voc()
    assert v.children == [[1, 2], [3, 4], [5, 6], [], [], [], []]
    assert v.word_of == [-1, -1, -1, 0, 1, 2, 3] and v.word_node == [3, 4, 5, 6]
    assert v.slots()[0] == [0, 1, 2, 3, 4, 5, 6]


def test_transform_hand_worked():
    v = hand_voc()
    q0 = D()                                # root: 0 vs 16 -> node 1; leaves 4 vs 4: the tie goes to node 3
    q1 = D(b0=0xFF, b31=0xF0)               # root: 12 vs 12: the tie goes to node 1; leaves 16 vs 8 -> node 4
    q2 = D(b0=0xFF, b1=0xFF, b2=0xFF)       # node 2, then node 5 (distance 0): word 2, weight 0
    q3 = D(b0=0xFF, b1=0xFF, b3=0xFF)       # node 2, then node 6
    assert v.transform(q0, 1) == (0, 1.0, 1)
    assert v.transform(q1, 1) == (1, 2.0, 1)
    assert v.transform(q2, 1) == (2, 0.0, 2)
    assert v.transform(q3, 1) == (3, 3.0, 2)
    assert [v.transform(q, 0)[2] for q in (q0, q1, q2, q3)] == [3, 4, 5, 6]      # nid_level = L: the leaf
    assert [v.transform(q, 2)[2] for q in (q0, q1, q2, q3)] == [0, 0, 0, 0]      # levelsup >= L
    r = R.compute_bow(v, np.array([q0, q1, q2, q3]), 1)
    assert list(r["word"]) == [0, 1, 2, 3] and list(r["weight"]) == [1.0, 2.0, 0.0, 3.0]
    assert list(r["node"]) == [1, 1, -1, 2]                                       # weight 0: not in the feature vector
    assert list(r["fv_node"]) == [1, 2] and list(r["fv_off"]) == [0, 2, 3] and list(r["fv_idx"]) == [0, 1, 3]


def test_leaf_above_nid_level_is_the_nid():
    # k = 2, L = 3: node 1 is a leaf at depth 1, node 2 inner with leaves 3, 4 at depth 2
    v = R.Voc(2, 3, [0, 0, 2, 2], [1, 0, 1, 1], [D(), D(b0=0xFF), D(b0=0xFF, b1=1), D(b0=0xFF, b1=3)], [1, 0, 1, 1])
    assert v.transform(D(), 0) == (0, 1.0, 1)            # nid_level 3, leaf at level 1
    assert v.transform(D(b0=0xFF), 1) == (1, 1.0, 3)     # nid_level 2 reached at the leaf
    assert v.transform(D(b0=0xFF), 2) == (1, 1.0, 2)


# SearchByBoW by hand.  KeyFrame features k0..k6, frame features c0..c7.
KF_NODE = [7, 7, 7, 7, 9, 11, 13]
KF_VALID = [1, 1, 0, 1, 1, 1, 1]
KF_DESC = [D(), D(b0=0x02), D(b0=0x01), D(b0=0xFF, b1=0xFF, b2=0x01), D(), D(b9=1), D(b10=0xFF)]
CUR_NODE = [7, 7, 7, 7, 9, 9, 12, 13]
CUR_DESC = [D(), D(b0=0x01), D(b0=0x03), D(b0=0xFF, b1=0xFF), D(b5=0x01), D(b5=0x02), D(b9=1), D(b10=0xFF)]
KF_ANGLE = [100.0] * 7
CUR_ANGLE = [90.0, 0.0, 40.0, 280.0, 0.0, 0.0, 0.0, 350.0]


def test_search_by_bow_hand_worked():
    # node 7: k0 takes c0 (0 against 1); k1 is as close to c0 (taken) as to c2 and takes c2 (1 against 2);
    #         k2 is invalid (it would have taken c1); k3 takes c3 (1 against 16)
    # node 9: k4 is at distance 1 of both c4 and c5: bestDist1 == bestDist2, rejected
    # nodes 11, 12: on one side only.  node 13: k6 takes c7 (0 against 256)
    m, nm, st = R.search_by_bow(KF_VALID, KF_DESC, KF_NODE, KF_ANGLE, CUR_DESC, CUR_NODE, CUR_ANGLE, 0.7, False)
    assert list(m) == [0, -1, 1, 3, -1, -1, -1, 6] and nm == 4
    assert st == dict(rot_removed=0, claim_dependency=1, tie_rejected=1)
    # rotations 10, 60, 180 (-180 + 360) and 110 (-250 + 360): bins 0, 2, 6, 4, one match each; the
    # three maxima are the first three bins in index order (0, 2, 4), so c3 (bin 6) loses its match
    m, nm, st = R.search_by_bow(KF_VALID, KF_DESC, KF_NODE, KF_ANGLE, CUR_DESC, CUR_NODE, CUR_ANGLE, 0.7, True)
    assert list(m) == [0, -1, 1, -1, -1, -1, -1, 6] and nm == 3 and st["rot_removed"] == 1
    # nnratio 0.4: k1's 1 < 0.4 * 2 still holds, k3 and k6 too; a ratio of 0.5 is not below 1 / 2
    m, nm, _ = R.search_by_bow(KF_VALID, KF_DESC, KF_NODE, KF_ANGLE, CUR_DESC, CUR_NODE, CUR_ANGLE, 0.5, False)
    assert list(m) == [0, -1, -1, 3, -1, -1, -1, 6] and nm == 3


def test_three_maxima():
    assert R.three_maxima([0] * 30) == (-1, -1, -1)
    h = [0] * 30
    h[4], h[7], h[9], h[20] = 50, 4, 30, 6
    assert R.three_maxima(h) == (4, 9, 20)
    h[20] = 4
    assert R.three_maxima(h) == (4, 9, -1)              # max3 = 4 < 0.1 * 50
    h[9] = 4
    assert R.three_maxima(h) == (4, -1, -1)
