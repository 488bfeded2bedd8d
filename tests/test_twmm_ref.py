"""The single-frame TrackWithMotionModel reference (tests/twmm_ref.py) and its scenes, without a
GPU: UpdateLastFrame's visit rule in closed form against the literal loop on directed depth sets,
the numpy UnprojectStereo against the oracle's two forms of it, the shared scenes asserted to reach
the branches the GPU tests need them for, and the header declaring the entry point."""
import os
import re

import numpy as np
import pytest

import chain_util as cu
import oracle as O
import twmm_ref as R
from coeb_front import synth
from conftest import ROOT


# ---- the visit rule ----
@pytest.mark.parametrize("M,c", R.VISIT_CASES)
@pytest.mark.parametrize("ties", [False, True])
def test_visit_rule_closed_form_equals_the_loop(M, c, ties):
    d = R.directed_depth(M, c, ties=ties)
    loop = R.visited_loop(d, R.TH_DEPTH)
    assert loop == R.visited_closed_form(d, R.TH_DEPTH), (M, c, ties)
    cc = int((d <= np.float32(R.TH_DEPTH)).sum())
    assert len(loop) == min(M, max(cc, 100) + 1)
    if not ties:
        assert cc == c


def test_visit_rule_special_depths():
    """0, negative and NaN depths are no entries; +inf is the farthest entry; a depth exactly
    th_depth counts as close; equal depths go by index."""
    for M, c in ((99, 50), (102, 100), (300, 40), (300, 180)):
        d = R.directed_depth(M, c, special=True, ties=True)
        assert np.isnan(d).any() and np.isinf(d).any() and (d == 0).any() and (d < 0).any()
        loop = R.visited_loop(d, R.TH_DEPTH)
        assert loop == R.visited_closed_form(d, R.TH_DEPTH), (M, c)
        with np.errstate(invalid="ignore"):
            assert all(d[i] > 0 for i in loop)
    d = np.full(150, 5.0, np.float32)                   # all equal and far: the first 101 by index
    assert R.visited_loop(d, R.TH_DEPTH) == list(range(101)) == R.visited_closed_form(d, R.TH_DEPTH)
    d = np.full(150, R.TH_DEPTH, np.float32)            # all exactly th_depth: all close, all visited
    assert R.visited_loop(d, R.TH_DEPTH) == list(range(150)) == R.visited_closed_form(d, R.TH_DEPTH)
    d = np.full(150, 5.0, np.float32)
    d[140] = np.float32(R.TH_DEPTH)
    d[7] = np.inf                                       # the one close point first, inf last and not reached
    want = [140] + [i for i in range(150) if i not in (140, 7)][:100]
    assert R.visited_loop(d, R.TH_DEPTH) == want == R.visited_closed_form(d, R.TH_DEPTH)
    assert R.visited_loop(d, np.nan) == R.visited_closed_form(d, np.nan) and len(R.visited_loop(d, np.nan)) == 150


def test_update_last_frame_replaces_unobserved_points_only():
    sc = R.scene(120, 150, seed=21)
    d = R.directed_depth(150, 60, special=True)
    sc = R.with_depth(sc, d)
    last = {k: v.copy() for k, v in sc["last"].items()}
    visited = R.visited_loop(d, R.TH_DEPTH)
    a, b, e = visited[0], visited[1], visited[2]
    last["has_mp"][a], last["mp_nobs"][a], last["outlier"][a] = 1, 0, 1     # nobody observes it: replaced, outlier kept
    last["has_mp"][b], last["mp_nobs"][b] = 1, 1                          # observed: kept
    last["has_mp"][e] = 0                                                  # no point: created
    new, created, cpos = R.update_last_frame(last, d, sc["last_desc"], R.TH_DEPTH, sc["Tcw_last"])
    assert created[a] and created[e] and not created[b]
    assert new["mp_nobs"][a] == 0 and new["has_mp"][a] == 1 and new["outlier"][a] == 1
    assert np.array_equal(new["mp_desc"][a], sc["last_desc"][a]) and np.array_equal(new["xw"][a], cpos[a])
    assert new["mp_nobs"][b] == 1 and np.array_equal(new["xw"][b], last["xw"][b])
    not_visited = np.setdiff1d(np.arange(150), visited)
    assert len(not_visited) and not created[not_visited].any()
    for k in ("has_mp", "mp_nobs", "xw", "mp_desc"):
        assert np.array_equal(new[k][not_visited], last[k][not_visited]), k
    want = np.array([(not last["has_mp"][i]) or last["mp_nobs"][i] < 1 for i in visited])
    assert np.array_equal(created[visited].astype(bool), want) and created.sum() == want.sum()
    assert np.array_equal(new["outlier"], last["outlier"])


# ---- the unprojection ----
@pytest.fixture(scope="module")
def extracted():
    ex = R.extractor()
    r = ex.extract(synth.make_frames(R.W, R.H, 1, seed=1003)[0])
    depth = synth.make_depth(R.W, R.H)
    return r, depth, O.mapframe_from_extraction(r["kps"], r["desc"], depth, *cu.TUM)


def test_unprojection_at_identity_is_the_oracles(extracted):
    r, depth, mf = extracted
    _, dep = O.stereo_from_rgbd(r["kps"], depth, cu.TUM[4])
    has = mf["has_mp"] > 0
    assert has.sum() > 500
    got = R.unproject_stereo(r["kps"], dep, np.eye(4, dtype=np.float32))
    assert np.array_equal(R.bits(got[has]), R.bits(mf["xw"][has]))


def test_unprojection_under_a_pose_is_the_local_maps(extracted):
    """oracle.local_map_build places KF2's points by mRwc * x3Dc + mOw with KF2's Twc given as a
    matrix; with [mRwc | mOw] of T_LAST it is UnprojectStereo under T_LAST."""
    r, depth, mf = extracted
    _, dep = O.stereo_from_rgbd(r["kps"], depth, cu.TUM[4])
    n = len(r["kps"])
    Twc = np.eye(4, dtype=np.float32)
    Twc[:3] = R.twc_of(R.T_LAST)
    assert np.abs(Twc[:3, :3] - np.eye(3)).max() > 0.01 and np.abs(Twc[:3, 3]).min() > 0.01     # a real pose
    lm = O.local_map_build(R.cameras()[0], mf, mf, Twc, None, 2, n, np.eye(4, dtype=np.float32))
    has = mf["has_mp"] > 0
    got = R.unproject_stereo(r["kps"], dep, R.T_LAST)
    assert np.array_equal(R.bits(got[has]), R.bits(lm["xw"][:n][has]))
    # and mOw is the camera centre: Tcw * [mOw, 1] = 0 to float accuracy
    T = R.T_LAST.astype(np.float64)
    assert np.abs(T[:3, :3] @ R.twc_of(R.T_LAST)[:, 3].astype(np.float64) + T[:3, 3]).max() < 1e-7


# ---- the scenes reach their branches ----
def test_main_scene_reaches_its_branches():
    sc = R.sized(*R.MAIN)
    ref = R.reference(sc)
    assert ref["nmatches_first"] >= R.MIN_MATCHES and not ref["retried"]        # first search >= 20
    assert (ref["discarded"] >= 0).sum() >= 1                                   # at least one discard
    kept = ref["match"][ref["match"] >= 0]
    assert (ref["last"]["mp_nobs"][kept] == 0).sum() >= 1                       # a kept match nobody observes
    assert ref["created"][ref["match_search"][ref["match_search"] >= 0]].sum() >= 1     # a created point matched
    assert 0 < ref["nmatches_map"] < ref["nmatches"] < ref["nmatches_search"]
    assert ref["ninliers_pose"] >= 3 and not np.array_equal(R.bits(ref["Tcw"]), R.bits(sc["Tcw"]))
    assert np.array_equal(ref["outlier"] > 0, ref["discarded"] >= 0)
    mono = sc["ur"][ref["match_search"] >= 0] < 0
    assert mono.any() and not mono.all()                                        # both edge kinds
    # SLAM mode on the same scene: nothing is created, fewer points to find
    slam = R.reference(sc, vo=False)
    assert slam["created"] is None and R.MIN_MATCHES <= slam["nmatches_search"] < ref["nmatches_search"]
    # the orientation check matters
    assert not np.array_equal(R.reference(sc, check_orientation=False)["match_search"], ref["match_search"])
    # the last frame has a slot with mvbOutlier that the step replaced: the search still skips it
    rep = (ref["created"] > 0) & (sc["last"]["outlier"] > 0)
    assert rep.any() and not np.isin(np.flatnonzero(rep), ref["match_search"]).any()


def test_retry_and_lost_scenes_reach_their_branches():
    sc = R.retry_scene()
    ref = R.reference(sc)
    assert ref["nmatches_first"] < R.MIN_MATCHES <= ref["nmatches_search"] and ref["retried"]
    assert ref["ninliers_pose"] >= 3
    lost = R.reference(R.lost_scene())
    assert lost["retried"] and lost["nmatches_search"] < R.MIN_MATCHES          # both < 20
    assert lost["ninliers_pose"] == 0 and lost["nmatches"] == lost["nmatches_search"] and lost["nmatches_map"] == 0
    assert (lost["discarded"] == -1).all() and np.array_equal(lost["match"], lost["match_search"])


def test_dup_scene_counts_assignments_not_keypoints():
    sc = R.dup_scene()
    for vo in (True, False):
        ref = R.reference(sc, vo=vo)
        held = int((ref["match_search"] >= 0).sum())
        assert ref["nmatches_search"] >= held + 5 and ref["nmatches_search"] >= R.MIN_MATCHES
        assert ref["nmatches"] == ref["nmatches_search"] - int((ref["discarded"] >= 0).sum()) > int((ref["match"] >= 0).sum())


def test_few_scene_has_fewer_than_three_edges():
    sc = R.few_scene()
    ref = R.reference(sc, min_matches=0)
    assert ref["nmatches_search"] == 2
    assert ref["ninliers_pose"] == 0 and np.array_equal(R.bits(ref["Tcw"]), R.bits(sc["Tcw"])) and ref["nmatches"] == 2


@pytest.mark.parametrize("n_cur,n_last", [s for s in R.SIZES if s[0] <= 1000])
def test_sized_scenes_are_not_empty(n_cur, n_last):
    ref = R.reference(R.sized(n_cur, n_last))
    if min(n_cur, n_last) >= 63:
        assert ref["nmatches_search"] >= R.MIN_MATCHES and ref["created"].sum() > 0, (n_cur, n_last)
    else:
        assert ref["nmatches_search"] < R.MIN_MATCHES


def test_bounded_camera_changes_the_search():
    sc = R.sized(*R.MAIN)
    assert not np.array_equal(R.reference(sc, bounded=True)["match_search"], R.reference(sc)["match_search"])


def test_largest_pair_fits_the_matcher():
    n, q = R.SIZES[-1]
    lds = R.match_lds_bytes
    assert n == 4095 and lds(n, q) + 512 <= 160 * 1024 < lds(n, q + 1) + 512


# ---- the interface ----
def test_header_declares_the_entry_point():
    txt = open(os.path.join(ROOT, "include", "coeb_front.h")).read()
    assert re.search(r"coeb_track_motion_model\s+<-", txt)                     # the table of entry points
    limit = int(re.search(r"#define\s+COEB_VO_MAX_LAST\s+(\d+)", txt).group(1))
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+coeb_track_motion_model\s*\(", txt) and "coeb_vo_points;" in txt
    assert re.search(r"#define\s+COEB_ABI_VERSION\s+3\b", txt)                 # nothing existing changed
    import coeb_front
    assert "coeb_track_motion_model" in coeb_front.ABI_SYMBOLS
    assert hasattr(coeb_front.Context, "track_with_motion_model")
    assert coeb_front.VO_MAX_LAST == limit >= R.SIZES[-1][1]
