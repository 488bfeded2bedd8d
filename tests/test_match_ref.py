"""The directed matcher scenes on the CPU (tests/match_ref.py): the literal Python models against
the C oracle on every scene, and every scene reaches the regime it is named after -- asserted
from the model's trace alone, so that the GPU comparison (tests/test_gpu_match_scenes.py) is known
to cross the kernels' list, sweep and grid boundaries it is meant to cross."""
import numpy as np
import pytest

import match_ref as mr


@pytest.fixture(scope="module")
def cams(oracle_mod):
    import chain_util as cu
    ex = oracle_mod.Extractor()
    return {None: cu.cameras(oracle_mod, ex, 640, 480, cu.TUM)[0],
            "inside": cu.cameras(oracle_mod, ex, 640, 480, cu.TUM, cu.BOUNDS_INSIDE)[0]}


@pytest.fixture(scope="module")
def all_scenes(cams):
    return mr.scenes(cams)


def test_scene_list_covers_the_issue(all_scenes):
    names = {s.name for s in all_scenes}
    for m in mr.MATCHERS:
        for K in mr.CHAIN_K:
            assert "chain%d-%s" % (K, m) in names
        for n in mr.LIST_M:
            assert "list%d-last-%s" % (n, m) in names and "list%d-equal-%s" % (n, m) in names
        for nq in mr.NQ:
            assert "nq%d-%s" % (nq, m) in names
        for c in mr.ORDER_R:
            assert "order-c%d-%s" % (c, m) in names
    assert len(names) == len(all_scenes)


def test_models_match_oracle_on_every_scene(oracle_mod, cams, all_scenes):
    """Oracle and model: the same count and the same match array; and the fixpoint the trace
    simulates ends at the literal loop's assignments (DESIGN.md s4.5's claim)."""
    for s in all_scenes:
        cam = cams[s.camera]
        nm_o, m_o = s.oracle(oracle_mod, cam)
        nm_p, m_p = s.model(cam)
        assert nm_o == nm_p and np.array_equal(m_o, m_p), (s.name, nm_o, nm_p)
        if not s.kw.get("check_ori"):
            t = s.trace(cam)
            last = np.full(len(m_p), -1, np.int32)
            for q, r in enumerate(t["res"]):
                if r >= 0:
                    last[r] = q                       # the last query assigned to a keypoint wins
            assert np.array_equal(last, m_p), s.name
            assert nm_p == sum(1 for r in t["res"] if r >= 0), s.name


def test_match_scenes_reach_their_regimes(cams, all_scenes):
    rows_seen = set()
    for s in all_scenes:
        cam = cams[s.camera]
        t, e = s.trace(cam), s.expect
        nm = s.model(cam)[0]
        name = s.name
        assert t["path"] == e["path"], (name, t["path"], t["sweeps"])
        if "sweeps" in e:
            assert t["sweeps"] == e["sweeps"], (name, t["sweeps"])
        if "max_count" in e:
            assert t["max_count"] == e["max_count"], (name, t["max_count"])
        if "max_count_le" in e:
            assert 0 < t["max_count"] <= e["max_count_le"], (name, t["max_count"])
        if e.get("nmatch") is not None:
            assert nm == e["nmatch"], (name, nm)
        if "nmatch_min" in e:
            assert nm >= e["nmatch_min"], (name, nm)
        if "min_ties" in e:
            assert t["ties"] >= e["min_ties"], (name, t["ties"])
        if "win_pos_last" in e:
            # the query under test is the last of the list window's (two threshold windows follow)
            q = len(t["counts"]) - 3
            assert t["counts"][q] == e["max_count"] and t["win_pos"][q] == e["win_pos_last"], (name, t["win_pos"][q])
            for k in (8, 12, 16):
                assert (t["pos_ge"][k] >= 1) == (e["win_pos_last"] >= k), (name, k)
        if "win_cols" in e:
            assert e["win_cols"] in t["win_cols"], (name, set(t["win_cols"]))
            rows_seen |= {r for r in t["win_rows"] if r is not None}
        if "cell_sizes" in e:
            g = mr.Grid(cam, s.inputs["kps"])
            sizes = sorted(len(c) for col in g.cells for c in col if c)
            assert sizes == sorted(e["cell_sizes"]), (name, sizes)
        if "off_grid" in e:
            assert t["off_grid"] == e["off_grid"], (name, t["off_grid"])
        if "min_off_grid" in e:
            assert t["off_grid"] >= e["min_off_grid"], (name, t["off_grid"])
        if "hist" in e:
            assert {b: c for b, c in enumerate(t["hist"]) if c} == e["hist"], (name, t["hist"])
        if "hist_bins_min" in e:
            assert sum(1 for c in t["hist"] if c) >= e["hist_bins_min"], (name, t["hist"])
        if "matched" in e:
            for q, want in e["matched"].items():
                assert (t["res"][q] >= 0) == bool(want), (name, q)
        if "nq" in e:
            assert len(t["counts"]) == e["nq"] and len(s.inputs["kps"]) == e["n"]
            # the blocking chain ends on the last query, the one past the register-head boundary
            assert t["res"][-1] >= 0 and t["win_pos"][-3:] == [0, 1, 2], (name, t["win_pos"][-3:])
            # launch_match's thread-count rule (match_ref.nq_scenes)
            assert (mr.lds_bytes(e["n"], e["nq"]) + 256 <= 80 * 1024) == (e["nq"] < 2000)
            assert mr.lds_bytes(e["n"], e["nq"]) <= 160 * 1024 - 256 and e["n"] <= 4094
    assert {1, 2, 3} <= rows_seen, rows_seen


def test_chain_paths_at_the_sweep_limit(cams, all_scenes):
    """Path 0 up to K = 63 (65 sweeps, the last one still), path 3 from K = 64; path 2 from a
    65-entry list: the exact boundaries, for the two matchers with a path readout and for k_match."""
    by = {s.name: s for s in all_scenes}
    for m in mr.MATCHERS:
        got = [(by["chain%d-%s" % (K, m)].trace(cams[None])["path"], by["chain%d-%s" % (K, m)].trace(cams[None])["sweeps"])
               for K in (63, 64)]
        assert got == [(0, 65), (3, 65)], (m, got)
        assert [by["list%d-last-%s" % (n, m)].trace(cams[None])["path"] for n in (64, 65)] == [0, 2]
        assert by["list64-equal-%s" % m].trace(cams[None])["sweeps"] == 65
