"""SearchForTriangulation without a GPU: the CPU restatement (tests/tri_ref.py) pinned on a
hand-worked case, every wrong reading of it shown to change a named directed case
(tests/tri_cases.py), the guard that is equivalent shown to be, and the library's exports.
Nothing here can fail without the feature; tests/test_gpu_tri_directed.py and tests/test_gpu_tri.py do."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import tri_cases as C
import tri_ref as T
from conftest import ROOT

f32 = np.float32
# ---- the hand-worked case ----
# F12 = [[1,0,0],[0,2,0],[3,4,5]], kp1 = (2, 3):
#   a = 2*1 + 3*0 + 3 = 5,  b = 2*0 + 3*2 + 4 = 10,  c = 2*0 + 3*0 + 5 = 5,  den = 25 + 100 = 125
#   kp2 = (4, 0):  num = 20 + 0 + 5 = 25,  dsqr = 625 / 125 = 5     > 3.84 * 1     (octave 0: rejected)
#                                                                   < 3.84 * 1.44  (octave 1: accepted)
#   kp2 = (3, 0):  num = 15 + 0 + 5 = 20,  dsqr = 400 / 125 = 3.2   < 3.84
#   kp2 = (1, -1): num = 5 - 10 + 5 = 0,   dsqr = 0
F_HAND = [[1, 0, 0], [0, 2, 0], [3, 4, 5]]


def _kf(rows):
    k = C.KF()
    for r in rows:
        k.add(*r)
    return k.done()


def test_line_hand_worked():
    assert tuple(float(v) for v in T.epipolar_line(2, 3, F_HAND)) == (5.0, 10.0, 5.0, 125.0)
    assert not T.check_dist_epipolar_line(2, 3, 4, 0, F_HAND, 1.0)
    assert T.check_dist_epipolar_line(2, 3, 4, 0, F_HAND, C.SIGMA2[1])
    assert T.check_dist_epipolar_line(2, 3, 3, 0, F_HAND, 1.0) and T.check_dist_epipolar_line(2, 3, 1, -1, F_HAND, 1.0)
    assert not T.check_dist_epipolar_line(2, 3, 1, -1, np.zeros((3, 3)), 1.0)          # den == 0
    # 6^2 + 8^2 = 100 = 100 * 1: not inside; 100 < 100 * 1.2 at octave 1
    assert not T.near_epipole(0, 0, 6, 8, 1.0) and T.near_epipole(0, 0, 6, 8, C.SCALE[1])
    assert T.near_epipole(1, 1, 7, 8.75, 1.0)                                           # 36 + 60.0625
    assert [T.rot_bin(15, 0), T.rot_bin(0, 30), T.rot_bin(900, 0), T.rot_bin(359.9, 0), T.rot_bin(45, 0)] == \
        [1, 11, 0, 12, 2]
    assert float(C.SCALE[1]) == float(f32(1.2)) and abs(float(C.SIGMA2[7]) - 1.2 ** 14) < 1e-4


def test_search_hand_worked():
    """One node: 10 bits away but off the line, two candidates 20 bits away on it (the last stays),
    51 bits away on it; a node keyframe 2 does not have; a feature with a MapPoint."""
    kf1 = _kf([(3, C.low(0), 2, 3), (4, C.low(0), 2, 3), (3, C.low(0), 2, 3, 0, -1.0, 0.0, 1)])
    kf2 = _kf([(3, C.low(10), 4, 0), (3, C.low(20), 3, 0), (3, C.bits(range(1, 21)), 1, -1), (3, C.low(51), 1, -1),
               (5, C.low(0), 1, -1)])
    trace = []
    m, nm = T.search_for_triangulation(kf1, kf2, kf1["has_mp"], kf2["has_mp"], F_HAND, C.FAR, C.SCALE, C.SIGMA2,
                                       False, False, trace=trace)
    assert m.tolist() == [2, -1, -1] and nm == 1 and T.matched_pairs(m) == [(0, 2)]
    assert trace == [(0, 0, "line"), (0, 1, "accepted"), (0, 2, "accepted"), (0, 3, "dist")]
    # at octave 1 the first candidate passes the line and is the nearest
    kf2["octave"][0] = 1
    m, nm = T.search_for_triangulation(kf1, kf2, kf1["has_mp"], kf2["has_mp"], F_HAND, C.FAR, C.SCALE, C.SIGMA2,
                                       False, False)
    assert m.tolist() == [0, -1, -1] and nm == 1


def test_fmaf_rounds_once():
    rng = np.random.RandomState(5)
    vals = rng.standard_normal((4000, 3)).astype(f32) * f32(8.0)
    vals[::7, 2] = -(vals[::7, 0] * vals[::7, 1])           # cancellation: the product's low bits decide
    for a, b, c in vals:
        exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
        got = T.fmaf(a, b, c)
        lo, hi = np.nextafter(got, f32(-np.inf)), np.nextafter(got, f32(np.inf))
        err = abs(Fraction(float(got)) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact)
        if err == abs(Fraction(float(lo)) - exact) or err == abs(Fraction(float(hi)) - exact):
            assert not got.view(np.uint32) & 1          # a tie goes to the even neighbour
    assert T.fmaf(f32(1 + 2.0 ** -12), f32(1 + 2.0 ** -12), f32(-1)) == f32(2.0 ** -11 + 2.0 ** -24)


@pytest.mark.parametrize("name", C.names())
def test_case_mutants(name):
    c = C.case(name)
    want = C.expected(name)
    for mu in c["mutants"]:
        got = C.reference(c, frozenset([mu]))
        assert not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])), mu
    if "want" in c:                                          # the winners the builder placed
        assert {i: int(want[0][0][i]) for i in c["want"]} == c["want"]
    assert want[1].tolist() == [int((row >= 0).sum()) for row in want[0]]


def test_every_mutant_has_a_case():
    named = {mu for n in C.names() for mu in C.case(n)["mutants"]}
    assert named == set(T.MUTATIONS)


def test_den_guard_is_equivalent():
    """den == 0 -> false: without the guard num * num / 0 is inf or nan and neither is < the bound,
    on every directed case (an all-zero F12 among them) and on lines with a == b == 0 and any c."""
    for n in C.names():
        c = C.case(n)
        got, want = C.reference(c, frozenset(T.EQUIVALENT)), C.expected(n)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), n
    for c22 in (0.0, 1.0, -3.5, np.inf):
        F = np.zeros((3, 3), f32)
        F[2, 2] = c22
        assert T.epipolar_line(4, 5, F)[3] == 0
        assert not T.check_dist_epipolar_line(4, 5, 6, 7, F, 1.0, frozenset(T.EQUIVALENT))
        assert not T.check_dist_epipolar_line(4, 5, 6, 7, F, 1.0)


def test_cases_cover_what_they_are_for():
    traces = {}
    for n in ("epipole", "chi2_bound", "trips_130", "nodes"):
        c = C.case(n)
        k1, tr = c["kfs"][c["slot1"]], []
        for j, s2 in enumerate(c["slots2"]):
            T.search_for_triangulation(k1, c["kfs"][s2], k1["has_mp"], c["kfs"][s2]["has_mp"], c["F12"][j], c["epipole"][j],
                                       C.SCALE, C.SIGMA2, c["only_stereo"], c["check_ori"], trace=tr)
        traces[n] = tr
    assert sum(w == "epipole" for _, _, w in traces["epipole"]) == 2
    assert C.expected("epipole")[0][0].tolist() == [1, 2, 3, 4, 5, -1]
    assert C.expected("chi2_bound")[0].tolist() == [[0, 1], [-1, -1], [-1, 1], [-1, -1]]
    assert max(len(k["node"]) for n in C.names() for k in C.case(n)["kfs"]) <= 200
    assert sorted(len(C.case(n)["slots2"]) for n in C.names())[-1] == 32
    assert sum(w == "accepted" for _, _, w in traces["trips_130"]) == 2 + 4        # C's four tied candidates
    assert C.expected("nodes")[1].tolist() == [3]
    assert (C.expected("nnb32")[1] > 0).sum() >= 12 and C.expected("rotation")[1].tolist() == [16]


def test_library_exports_the_entry_points():
    lib = os.path.join(ROOT, "coeb-slam_amd", "lib", "libcoeb_front.so")
    if not os.path.exists(lib):
        pytest.skip("libcoeb_front.so is not built")
    h = ctypes.CDLL(lib)
    assert hasattr(h, "coeb_kfdb_set_geometry") and hasattr(h, "coeb_kfdb_search_triangulation")
