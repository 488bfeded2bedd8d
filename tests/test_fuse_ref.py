"""tests/fuse_ref.py pinned on a hand-worked case, and tests/fuse_cases.py checked against it: every
wrong reading of fuse_ref.MUTATIONS changes the expected output of a directed case that names it, or
is shown to be equivalent (no GPU)."""
import os
import re

import numpy as np
import pytest

import fuse_cases as C
import fuse_ref as F

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hand_worked_point():
    """fx = 512, the point (1/512, 0, 1): z = 1, invz = 1, u = fma(512, 1/512, 320) = 321, v = 240,
    ur = 321 - 40 = 281; dist3D = sqrt(1 + 2^-18) -> 1.0000019; maxd = 1: ratio < 1, level 0, r = 3.
    Feature 0 at (322, 241): e2 = 1 + 1 = 2 <= 5.99, distance 7.  Feature 1 at (323.5, 240): 2.5 px,
    e2 = 6.25 > 5.99.  Feature 2, stereo at (321, 242) with ur 283: e2 = 0 + 4 + 4 = 8 > 7.8."""
    cam = C.CAM
    kf = C.KF()
    kf.add(322, 241, d=7)
    kf.add(323.5, 240, d=1)
    kf.add(321, 242, ur=283.0, d=1)
    kf = kf.done()
    P = np.array([1.0 / 512, 0, 1], f32)
    z, invz, u, v, ur = F.project(cam, C.I3, C.Z3, P)
    assert (z, invz, u, v, ur) == (1.0, 1.0, 321.0, 240.0, 281.0)
    grid = F.assign_features_to_grid(kf, cam)
    assert grid[32][24] == [0, 1, 2] and sum(len(c) for col in grid for c in col) == 3     # round(32.2), round(32.35), round(32.1)
    assert F.features_in_area(kf, grid, cam, u, v, 3.0) == [0, 1, 2]
    assert F.features_in_area(kf, grid, cam, u, v, 2.5) == [0, 2]             # |323.5 - 321| < 2.5 is false
    tr = {}
    got = F.fuse_point(kf, grid, cam, C.I3, C.Z3, C.Z3, P, P, 1.0, 0.5, C.low(0), 3.0, trace=tr)
    assert got == (0, 7) and tr["mono"] == 2 and tr["stereo"] == 1 and tr["ndist"] == 1
    assert F.predict_scale(cam, 1.0, 1.0000019) == 0 and F.predict_scale(cam, 1.3, 1.0) == 2
    assert F.predict_scale(cam, 100.0, 1.0) == 7


def test_level_tables_are_the_extractor_s():
    assert np.array_equal(C.CAM.scale[:3], np.array([1.0, 1.2, f32(float(f32(1.2)) * float(f32(1.2)))], f32))
    assert C.CAM.inv_sigma2[0] == 1.0 and abs(float(C.CAM.inv_sigma2[1]) - 1 / 1.44) < 1e-6


def test_early_returns():
    """1 and 3 through Fuse (th = 0 next to the far bounds); 2 and 4 only by calling the walk directly,
    since Fuse has u >= min_x, v >= min_y and r >= 0."""
    c = C.case("early_returns")
    tr = []
    C.reference(c, traces=tr)
    assert [t["ret"] for t in tr[0]] == [[1], [3]]
    kf = c["kfs"][0]
    grid = F.assign_features_to_grid(kf, c["cam"])
    for x, y, want in ((-20.0, 100.0, 2), (100.0, -20.0, 4)):
        ret = []
        assert F.features_in_area(kf, grid, c["cam"], x, y, 3.0, ret=ret) == [] and ret == [want]


def test_cases_reach_what_they_name():
    tr = []
    C.reference(C.case("depth"), traces=tr)
    assert [t["why"] for t in tr[0]] == ["z", "image", "image", "image", "compared", "image"]
    tr = []
    C.reference(C.case("image_bounds"), traces=tr)
    assert [t["why"] for t in tr[0]][:4] == ["compared", "image", "compared", "image"] and tr[0][6]["why"] == "image"
    bi, bd = C.expected("range")
    assert bd[0].tolist() == [2, 256, 2, 256, 2, 2]
    assert C.expected("angle")[1][0].tolist() == [2, 256, 256]
    assert C.expected("predict_scale")[0][0].tolist() == [2, 3, 0, 7, 0, 5, 4, 11, 12]
    assert C.expected("window_edge")[0][0].tolist() == [1, 3]
    assert C.expected("grid_edges")[0][0].tolist() == list(range(8))
    assert C.expected("outside_grid")[0][0].tolist() == [1, -1, 4, 5]
    assert C.expected("chi")[0][0].tolist() == [0, -1, 2, -1, -1, 5, -1]
    assert C.expected("ties")[0][0].tolist() == [1, 2, 5]
    bi, bd = C.expected("best_dist")
    assert bi[0].tolist() == [0, -1, -1] and bd[0].tolist() == [50, 51, 256]
    tr = []
    C.reference(C.case("chi"), traces=tr)
    assert sum(t["stereo"] for t in tr[0]) >= 4 and sum(t["mono"] for t in tr[0]) >= 2
    j = C.expected("jobs")
    assert [len(b) for b in j[0]] == [6, 4, 6, 0, 4, 3, 1] and j[0][0][2] == -1 and j[0][1][1] == -1
    assert j[0][5].tolist() != j[0][0][:3].tolist()                 # the second pose moves the projections
    assert len(C.case("jobs_128")["jobs"]) == 128


@pytest.mark.parametrize("mut", F.MUTATIONS)
def test_every_mutation_is_noticed_or_equivalent(mut):
    hit = [n for n in C.names() if mut in C.case(n)["mutants"]]
    if mut in F.EQUIVALENT:
        assert not hit and C.chi_products_disagree(C.CAM) == [] and C.chi_products_disagree(C.CAM_B) == []
        return
    assert hit, "no directed case names " + mut
    for n in hit:
        want, got = C.expected(n), C.reference(C.case(n), {mut})
        assert any(not np.array_equal(a, b) for a, b in zip(want[0] + want[1], got[0] + got[1])), (n, mut)


def test_random_scene_exercises_the_rules():
    """The scene of tests/test_gpu_fuse.py on the model alone: at least a third of the pairs reach the descriptor
    comparison and both chi-square branches occur."""
    from test_gpu_fuse import scene_ref
    want, tr = scene_ref()
    why = [t["why"] for t in tr]
    assert why.count("compared") * 3 >= len(why), {w: why.count(w) for w in set(why)}
    assert sum(t.get("stereo", 0) for t in tr) >= 200 and sum(t.get("mono", 0) for t in tr) >= 200
    assert sum(int((bi >= 0).sum()) for bi, _ in want) >= 200
    assert sum(int(((bd > 50) & (bd < 256)).sum()) for _, bd in want) >= 50
    for w in ("image", "range", "skipped", "filtered"):
        assert why.count(w) >= 1, w


def test_abi():
    txt = open(os.path.join(ROOT, "include", "coeb_front.h")).read()
    assert re.search(r"#define\s+COEB_ABI_VERSION\s+3\b", txt)                 # nothing existing changed
    assert "coeb_kfdb_fuse_search" in txt and re.search(r"#define\s+COEB_FUSE_MAX_JOBS\s+128\b", txt)
    import coeb_front as h
    assert "coeb_kfdb_fuse_search" in h.ABI_SYMBOLS and hasattr(h.KeyFrameDatabase, "fuse_search")
    assert h.FUSE_MAX_JOBS == 128
