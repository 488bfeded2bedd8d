"""The directed matcher scenes (tests/match_ref.py) on the device: k_match (with k_match_lists),
k_match_local and k_match_kf through the single-frame C-ABI against the oracle, count and every
match index exactly.  For the two kernels with a readout the path (0 parallel claims, 2 list
overflow, 3 no convergence) and the number of fixpoint sweeps must be what the Python model's
trace says; k_match has none, its regimes are asserted on the CPU (tests/test_match_ref.py)."""
import numpy as np
import pytest

import match_ref as mr
from chain_util import BOUNDS_INSIDE, TUM, cameras
from test_gpu_parity import keyframe_both, localmap_both, localmap_path, match_both, search_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cam_pairs(oracle_mod):
    ex = oracle_mod.Extractor()
    return ex, {None: cameras(oracle_mod, ex, 640, 480, TUM), "inside": cameras(oracle_mod, ex, 640, 480, TUM, BOUNDS_INSIDE)}


@pytest.fixture(scope="module")
def all_scenes(cam_pairs):
    return mr.scenes({k: v[0] for k, v in cam_pairs[1].items()})


def run_scene(ctx, oracle_mod, cam_pairs, s, forced=False):
    """The scene on the device against the oracle; the path readout against the trace."""
    ex, cams = cam_pairs
    i, k = s.inputs, s.kw
    if s.matcher == "frame":
        match_both(ctx, oracle_mod, ex, i["kps"], i["desc"], i["ur"], i["last"], i["Tc"], i["Tl"], th=k["th"],
                   bmono=k["bmono"], check_ori=k["check_ori"], cams=cams[s.camera])
        return
    if s.matcher == "local":
        localmap_both(ctx, oracle_mod, ex, i["kps"], i["desc"], i["ur"], i["cur_obs"], i["mp"], k["th"], k["nnratio"],
                      cams=cams[s.camera])
        got = localmap_path(ctx)
    else:
        keyframe_both(ctx, oracle_mod, ex, i["kps"], i["desc"], i["cur_has"], i["kf"], i["T"], k["th"], k["orb_dist"],
                      k["check_ori"], cams=cams[s.camera])
        got = search_path(ctx)
    t = s.trace(cams[s.camera][0])
    assert got == ((1, 0) if forced else (t["path"], t["sweeps"])), (s.name, got, t["path"], t["sweeps"])


def group(all_scenes, prefix, matcher):
    out = [s for s in all_scenes if s.name.startswith(prefix) and s.matcher == matcher]
    assert out
    return out


GROUPS = ("chain", "list", "nq", "order", "edges", "rot", "ratio")


@pytest.mark.parametrize("prefix", GROUPS[:-1])
@pytest.mark.parametrize("split", [None, "0", "2"])
def test_lastframe_scenes(ctx, oracle_mod, cam_pairs, all_scenes, monkeypatch, prefix, split):
    """k_match: one pair's lists from 8 k_match_lists workgroups (unset), from k_match itself (0),
    from 2 workgroups."""
    if split is not None:
        monkeypatch.setenv("COEB_MATCH_SPLIT", split)
    for s in group(all_scenes, prefix, "frame"):
        run_scene(ctx, oracle_mod, cam_pairs, s)


@pytest.mark.parametrize("prefix", [g for g in GROUPS if g != "rot"])     # no rotation filter in this search
def test_localmap_scenes(ctx, oracle_mod, cam_pairs, all_scenes, prefix):
    for s in group(all_scenes, prefix, "local"):
        run_scene(ctx, oracle_mod, cam_pairs, s)


@pytest.mark.parametrize("prefix", GROUPS[:-1])
def test_keyframe_scenes(ctx, oracle_mod, cam_pairs, all_scenes, prefix):
    for s in group(all_scenes, prefix, "kf"):
        run_scene(ctx, oracle_mod, cam_pairs, s)


@pytest.mark.parametrize("matcher", mr.MATCHERS)
def test_chain_and_list_scenes_sequential(ctx, oracle_mod, cam_pairs, all_scenes, monkeypatch, matcher):
    """The literal loop of each kernel (COEB_MATCH_SEQUENTIAL) on the chain and list-length scenes."""
    monkeypatch.setenv("COEB_MATCH_SEQUENTIAL", "1")
    ss = [s for s in all_scenes if s.seq and s.matcher == matcher]
    assert len(ss) >= len(mr.CHAIN_K) + 2 * len(mr.LIST_M)
    for s in ss:
        run_scene(ctx, oracle_mod, cam_pairs, s, forced=True)


def test_paths_at_their_boundaries(ctx, oracle_mod, cam_pairs, all_scenes):
    """Path 3 from the first chain that needs more than kMaxIter + 1 sweeps, path 2 from the first
    list over kCQ entries, path 0 just below both, read from the device."""
    by = {s.name: s for s in all_scenes}
    for m, read in (("local", localmap_path), ("kf", search_path)):
        got = []
        for name in ("chain63", "chain64", "list64-last", "list65-last", "list64-equal", "list65-equal"):
            run_scene(ctx, oracle_mod, cam_pairs, by["%s-%s" % (name, m)])
            got.append(read(ctx))
        assert got == [(0, 65), (3, 65), (0, 2), (2, 0), (0, 65), (2, 0)], (m, got)
