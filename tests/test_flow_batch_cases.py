"""The frame lists of tests/flow_batch_cases.py, checked on the oracle alone (no GPU).

tests/test_gpu_flow_batch.py relies on what these lists contain: pairs without corners at the
start, at the end and in a run, a pair at the 1000-corner cap, pairs with a handful of corners,
neighbouring frames whose T_M differ, T_M that changes the extraction.  Every such condition is
asserted here from the oracle's results, so a later change of synth cannot silently empty a
case.  The per-case counts are printed (pytest -s).  The numpy model of the flattened work list
is checked against the plain enumeration of the points, and each wrong reading of it must change
the (pair, point) map on at least one case.
"""
import numpy as np
import pytest

import flow_batch_cases as fc

SMALL = ("mixed", "empty_first", "empty_last", "empty_run", "cap", "two_frames", "one_frame")


def _res(oracle_mod, name):
    nl = fc.ROUND_LEVELS if name == "round" else 8
    return fc.build(name), fc.oracle_case(oracle_mod, fc.build(name), nl)


def _report(name, res):
    n, t = fc.counts(res), fc.tm_counts(res)
    if len(n) > 32:
        busy = np.nonzero(n)[0]
        print("%s: %d pairs, corners %s, |T_M| %s" % (name, len(n), [(int(z), int(n[z])) for z in busy],
                                                       [(f, v) for f, v in enumerate(t) if v > 0]))
    else:
        print("%s: corners %s, |T_M| per frame (-1: None) %s" % (name, n.tolist(), t))


def test_mixed_conditions(oracle_mod):
    case, res = _res(oracle_mod, "mixed")
    _report("mixed", res)
    fr, n, t, roles = case["frames"], fc.counts(res), fc.tm_counts(res), case["roles"]
    assert (case["w"], case["h"]) == fc.MIXED_SIZE and len(fr) == 10
    for z in roles["ordinary"]:
        assert n[z] >= 50 and t[z + 1] > 0, z
    z = roles["to_flat"]
    assert fr[z].std() > 10 and fr[z + 1].std() == 0 and n[z] > 0
    z = roles["from_flat"]
    assert fr[z].std() == 0 and fr[z + 1].std() > 10 and n[z] == 0 and t[z + 1] == -1
    z = roles["many"]
    assert n[z] >= 400 and t[z + 1] == 0
    assert 8 <= n[roles["few"]] <= 15
    assert 1 <= n[roles["fewer"]] <= 7
    z = roles["identical"]
    assert np.array_equal(fr[z], fr[z + 1])
    for f in range(len(t) - 1):
        if t[f] > 0 and t[f + 1] > 0:
            assert abs(t[f] - t[f + 1]) >= 5, (f, t)
    # T_M of a neighbouring slot would change the extraction: >= 3 frames whose own T_M has
    # points inside a box, removes keypoints, and gives another result than T_M of f - 1 or f + 1
    ex, hit = res["ex"], []
    for f in range(1, len(fr)):
        tm, b = res["tm"][f], case["boxes"][f]
        if tm is None or not len(tm) or not len(b):
            continue
        inside = ((tm[:, None, 0] >= b[None, :, 0]) & (tm[:, None, 0] <= b[None, :, 2]) &
                  (tm[:, None, 1] >= b[None, :, 1]) & (tm[:, None, 1] <= b[None, :, 3])).any()
        own = res["ext"][f]
        bare = fc.masked_extract(ex, fr[f], b, None, res["blur"][f])
        others = [fc.masked_extract(ex, fr[f], b, res["tm"][g], res["blur"][f]) for g in (f - 1, f + 1) if g < len(fr)]
        if inside and len(own["kps"]) < len(bare["kps"]) and not any(fc.same_extraction(own, o) for o in others):
            hit.append(f)
    print("mixed: frames whose T_M slot decides the extraction:", hit)
    assert len(hit) >= 3, hit


@pytest.mark.parametrize("name", ["empty_first", "empty_last", "empty_run"])
def test_empty_pair_positions(oracle_mod, name):
    case, res = _res(oracle_mod, name)
    _report(name, res)
    n = fc.counts(res)
    if name == "empty_first":
        assert len(case["frames"]) == 5 and n[0] == 0 and (n[1:] > 0).all()
    elif name == "empty_last":
        assert len(case["frames"]) == 5 and n[-1] == 0 and (n[:-1] > 0).all()
    else:
        # three empty pairs between two others are five pairs: six frames
        assert len(case["frames"]) == 6 and n[0] > 0 and n[4] > 0 and (n[1:4] == 0).all()
    offs = fc.index_offsets(n)
    assert (np.diff(offs) == 0).sum() == (n == 0).sum()          # equal neighbours in offs
    for z in np.nonzero(n == 0)[0]:
        assert res["tm"][z + 1] is None, z


def test_cap_reaches_1000(oracle_mod):
    case, res = _res(oracle_mod, "cap")
    _report("cap", res)
    n = fc.counts(res)
    assert len(case["frames"]) == 3 and n.tolist() == [1000, 1000]
    assert fc.index_offsets(n).tolist() == [0, 1000, 2000]
    assert fc.item_map(fc.index_offsets(n))[:, 1].max() == 999
    # the size is the smallest of its family: one step down the cap is missed
    w = case["w"] - 1
    nz = fc.noise(w, w * 3 // 4, seed=12)
    assert min(len(oracle_mod.good_features(fc.shifted(nz, k))) for k in range(2)) < 1000


def test_two_frames_and_one_frame(oracle_mod):
    case, res = _res(oracle_mod, "two_frames")
    _report("two_frames", res)
    assert len(case["frames"]) == 2 and fc.counts(res)[0] >= 50 and fc.tm_counts(res)[1] > 0
    case, res = _res(oracle_mod, "one_frame")
    _report("one_frame", res)
    assert len(case["frames"]) == 1 and len(res["pairs"]) == 0 and fc.tm_counts(res) == [0]
    assert len(res["ext"][0]["kps"]) > 100


def test_round_crosses_the_second_round_inside_busy_pairs(oracle_mod):
    case, res = _res(oracle_mod, "round")
    _report("round", res)
    n = fc.counts(res)
    assert (case["w"], case["h"]) == fc.ROUND_SIZE and len(case["frames"]) == 1030 and len(n) == 1029
    assert tuple(np.nonzero(n)[0]) == fc.ROUND_BUSY
    assert n[fc.ROUND - 1] > 0 and n[fc.ROUND] > 0            # the round boundary lies inside the busy run
    offs = fc.index_offsets(n)
    assert offs[fc.ROUND] > 0 and offs[-1] == n.sum()
    t = fc.tm_counts(res)
    assert sum(1 for f in range(1022, 1030) if t[f] > 0) >= 2   # T_M past frame 1023 reaches the extraction
    assert sum(1 for e in res["ext"] if len(e["kps"])) >= 5     # of the nine frames that are not flat


def test_index_model_and_wrong_readings(oracle_mod):
    """The binary-search model gives the plain enumeration on every case; each wrong reading
    gives another map on at least one.  No frame list makes goodFeaturesToTrack report -1 (more
    local maxima than a quarter of the pixels), so the negative count stands in a count vector
    of its own: mixed's with the device's overflow marker in one pair."""
    vectors = {}
    for name in SMALL + ("round",):
        vectors[name] = fc.counts(_res(oracle_mod, name)[1])
    neg = vectors["mixed"].copy()
    neg[4] = -1
    vectors["mixed_overflow"] = neg
    for name, n in vectors.items():
        got, want = fc.item_map(fc.index_offsets(n)), fc.expected_map(n)
        assert np.array_equal(got, want), name
    for reading, f in fc.WRONG_READINGS.items():
        apart = [name for name, n in vectors.items()
                 if not np.array_equal(np.asarray(f(n))[:len(fc.expected_map(n))], fc.expected_map(n))
                 or len(f(n)) != len(fc.expected_map(n))]
        print("wrong reading %s: separated by %s" % (reading, apart))
        assert apart, reading
    # which case separates which reading is no accident
    assert not np.array_equal(fc.WRONG_READINGS["nine_bit_index"](vectors["cap"]), fc.expected_map(vectors["cap"]))
    assert not np.array_equal(fc.WRONG_READINGS["round_base_dropped"](vectors["round"]), fc.expected_map(vectors["round"]))
    assert not np.array_equal(fc.WRONG_READINGS["strict_compare"](vectors["empty_run"]), fc.expected_map(vectors["empty_run"]))
