"""The relocalisation refinement's CPU composition (tests/reloc_ref.py, no GPU): the directed scene
list reaches every stage 0-5 with the reference's thresholds and every gate on both sides of its
boundary, and holds the scenes the GPU test needs in order not to pass on an easy list."""
import numpy as np
import pytest

import reloc_ref as R

DIRECTED = R.directed()
TAGS = [d[0] for d in DIRECTED]


@pytest.mark.parametrize("tag", TAGS)
def test_directed_scene_ends_in_its_stage(tag):
    _, _, _, stage = R.directed_case(tag)
    assert R.directed_ref(tag)["stage"] == stage


def test_reference_thresholds_reach_every_stage():
    D = (R.MIN_GOOD, R.LOW_GOOD, R.ENOUGH_GOOD)
    stages = {R.directed_ref(t)["stage"] for t, _, th, _ in DIRECTED if th == D}
    assert stages == {0, 1, 2, 3, 4, 5}


def test_every_gate_on_both_sides_of_its_boundary():
    ref = {t: R.directed_ref(t) for t in TAGS}
    th = {t: d[2] for t, d in zip(TAGS, DIRECTED)}
    first = lambda t: ref[t]["trace"]["ngood"][0]
    second = lambda t: ref[t]["trace"]["ngood"][1]
    # nGood < min_good
    assert first("min_good-1") == th["min_good-1"][0] - 1 and ref["min_good-1"]["stage"] == 0
    assert first("min_good") == th["min_good"][0] and ref["min_good"]["stage"] > 0
    # nGood < enough_good after the first optimisation
    assert first("enough-1@1") == th["enough-1@1"][2] - 1 and ref["enough-1@1"]["stage"] >= 2
    assert first("min_good") == th["min_good"][2] and ref["min_good"]["stage"] == 1
    # nadditional + nGood >= enough_good
    assert ref["sum1-1"]["nadditional1"] + first("sum1-1") == th["sum1-1"][2] - 1 and ref["sum1-1"]["stage"] == 2
    assert ref["sum1"]["nadditional1"] + first("sum1") == th["sum1"][2] and ref["sum1"]["stage"] >= 3
    # low_good < nGood < enough_good at the second optimisation
    assert second("low") == th["low"][1] and ref["low"]["stage"] == 3
    assert second("low+1") == th["low+1"][1] + 1 and ref["low+1"]["stage"] == 4
    assert second("enough@2") == th["enough@2"][2] and ref["enough@2"]["stage"] == 3
    # nGood + nadditional >= enough_good behind the second search
    assert second("low+1") + ref["low+1"]["nadditional2"] == th["low+1"][2] - 1
    assert second("low+1,5") + ref["low+1,5"]["nadditional2"] == th["low+1,5"][2] and ref["low+1,5"]["stage"] == 5


def test_an_outlier_keeps_its_point_through_stage_3():
    """No discard in front of or behind the second optimisation: a flagged keypoint still holds its point."""
    r = R.directed_ref("default-3")
    assert r["stage"] == 3
    kept = (r["outlier"] > 0) & (r["match"] >= 0)
    assert kept.sum() >= 3
    assert r["written"][kept].all()


def test_second_search_sees_another_sfound():
    r = R.directed_ref("default-5")
    f1, f2 = r["trace"]["found1"], r["trace"]["found2"]
    assert f1 - f2, "an inlier the first optimisation discarded stays in the first sFound only"
    assert f2 - f1, "the first search's assignments are in the second sFound only"
    # and the second search does find points the first one was barred from
    fr, hyp, _, _ = R.directed_case("default-5")
    at2, at3 = r["trace"]["held_at"][1], r["trace"]["held_at"][2]
    new = at3[(at3 >= 0) & (at2 < 0)]
    assert len(new) == r["nadditional2"] > 0 and set(new.tolist()) & (f1 - f2)


def test_first_search_assigns_although_the_hypothesis_stops():
    r = R.directed_ref("default-2")
    fr, hyp, _, _ = R.directed_case("default-2")
    assert r["stage"] == 2 and r["nadditional1"] > 0
    entered = np.where(hyp["inlier"] > 0, hyp["match"], -1)
    assigned = (r["match"] >= 0) & (r["match"] != entered)
    assert assigned.sum() == r["nadditional1"]
    assert len(r["trace"]["ngood"]) == 1                       # no second optimisation ran
    assert (~r["written"][assigned & ~(hyp["inlier"] > 0)]).all()     # no optimisation saw those: no flag is reported


def test_stage_0_keeps_the_inlier_points():
    r = R.directed_ref("default-0")
    fr, hyp, _, _ = R.directed_case("default-0")
    assert r["stage"] == 0 and r["ngood"] < R.MIN_GOOD
    assert np.array_equal(r["match"], np.where(hyp["inlier"] > 0, hyp["match"], -1))
    assert (r["outlier"] > 0).any()                            # `continue` skips the discard: flagged and still held


def test_gates_off_takes_every_branch():
    for name in R.BASES:
        t = R.base_trace(name)
        assert all(t[k] >= 0 for k in t)
        assert len(R.reference(*R.base(name), gates=False)["trace"]["ngood"]) == 3


def test_sized_scenes_and_thresholds():
    """The sizes of the GPU test: the composition runs on each (empty sides included), and the
    thresholds chosen for a scene take it past the first gate wherever it has points."""
    for n_cur, n_kf in R.SIZES:
        fr, hyp = R.frame(n_cur), R.sized(n_cur, n_kf)
        assert len(hyp["match"]) == n_cur and len(hyp["kf"]["valid"]) == n_kf
        assert ((hyp["match"] >= -1) & (hyp["match"] < max(n_kf, 1))).all() and (hyp["match"][hyp["inlier"] > 0] >= 0).all()
        mg, lg, eg = R.thresholds_for(fr, hyp)
        r = R.reference(fr, hyp, min_good=mg, low_good=lg, enough_good=eg)
        if min(n_cur, n_kf) >= 63:
            assert r["stage"] == 5, (n_cur, n_kf, r["stage"])
        if n_cur == 0 or n_kf == 0:
            assert r["stage"] == 0 and r["ngood"] == 0


def test_python_mirror_lists_the_call():
    import coeb_front
    assert "coeb_reloc_refine" in coeb_front.ABI_SYMBOLS
    assert len(coeb_front.lib().coeb_reloc_refine.argtypes) == 20        # the header's parameter list
    assert coeb_front.RELOC_MAX_HYP == 16
