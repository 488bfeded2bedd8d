"""tests/newpts_ref.py pinned without a device: on a hand-worked pair, against a float64 model of the same loop
body (np.linalg.svd, math.cos / atan2), and by its wrong readings, each of which a named case of
tests/newpts_cases.py has to notice.

Decision rule.  The float64 model records every gate quantity it evaluates with its threshold.  A pair is
DECIDED when each of them is away from its threshold by more than MARGIN_COS = 1e-6 (absolute, for the three
cosine comparisons: a float32 cosine near 1 carries 6e-8, and the canonical parallax bound differs from
cos(2 atan2()) by rounding only) or by more than MARGIN_REL = 1e-3 of the threshold (the depths, the two
reprojection sums, the two ratio products).  On decided pairs the restatement's status has to equal the
model's; the seeded scene leaves at most 5 % of its pairs undecided.  x3D of the decided, accepted pairs is
compared by the largest relative deviation |x - x64| / |x64|, see X3D_MEASURED."""
import math

import numpy as np
import pytest

import newpts_cases as C
import newpts_ref as N
from tri_cases import NLEVELS, SCALE, SIGMA2

f32 = np.float32
MARGIN_COS, MARGIN_REL = 1e-6, 1e-3
# the largest relative deviation of x3D from the float64 model over the decided, accepted pairs of the seeded
# scene (float32 Jacobi rounding at the scene's worst conditioning); the test asserts twice it
X3D_MEASURED = 2.44e-6


def model64(V1, V2, g1, g2, scale, sigma2, rf):
    """-> (status, source, X float64 or None, gates [(quantity, threshold, absolute margin)])"""
    gates = []
    R1, R2 = V1["Rcw"].astype(float).reshape(3, 3), V2["Rcw"].astype(float).reshape(3, 3)
    t1, t2 = V1["tcw"].astype(float), V2["tcw"].astype(float)
    st1, st2 = g1["u_right"] >= 0, g2["u_right"] >= 0
    xn1 = np.array([(float(g1["x"]) - float(V1["cx"])) * float(V1["invfx"]), (float(g1["y"]) - float(V1["cy"])) * float(V1["invfy"]), 1.0])
    xn2 = np.array([(float(g2["x"]) - float(V2["cx"])) * float(V2["invfx"]), (float(g2["y"]) - float(V2["cy"])) * float(V2["invfy"]), 1.0])
    r1, r2 = R1.T @ xn1, R2.T @ xn2
    cos = float(r1 @ r2 / (np.linalg.norm(r1) * np.linalg.norm(r2)))
    cps1 = cps2 = cos + 1
    if st1:
        cps1 = math.cos(2 * math.atan2(float(V1["mb"]) / 2, float(g1["depth"])))
    elif st2:
        cps2 = math.cos(2 * math.atan2(float(V2["mb"]) / 2, float(g2["depth"])))
    cps = min(cps1, cps2)
    gates += [(cos, cps, MARGIN_COS), (cos, 0.0, MARGIN_COS)]
    if not (st1 or st2):
        gates.append((cos, 0.9998, MARGIN_COS))

    def unproject(V, g):
        z = float(g["depth"])
        Pc = np.array([(float(g["kx"]) - float(V["cx"])) * z * float(V["invfx"]), (float(g["ky"]) - float(V["cy"])) * z * float(V["invfy"]), z])
        return V["Rcw"].astype(float).reshape(3, 3).T @ Pc + V["Ow"].astype(float)

    if cos < cps and cos > 0 and (st1 or st2 or cos < 0.9998):
        src = N.SRC_TRI
        T1, T2 = np.hstack([R1, t1[:, None]]), np.hstack([R2, t2[:, None]])
        A = np.array([xn1[0] * T1[2] - T1[0], xn1[1] * T1[2] - T1[1], xn2[0] * T2[2] - T2[0], xn2[1] * T2[2] - T2[1]])
        h = np.linalg.svd(A)[2][3]
        if h[3] == 0:
            return N.W_ZERO, src, None, gates
        X = h[:3] / h[3]
    elif st1 and cps1 < cps2:
        src, X = N.SRC_STEREO1, unproject(V1, g1)
    elif st2 and cps2 < cps1:
        src, X = N.SRC_STEREO2, unproject(V2, g2)
    else:
        return N.LOW_PARALLAX, N.SRC_NONE, None, gates
    z1, z2 = float(R1[2] @ X + t1[2]), float(R2[2] @ X + t2[2])
    depth_scale = max(abs(z1), abs(z2), 1.0)
    gates.append((z1, 0.0, MARGIN_REL * depth_scale))
    if z1 <= 0:
        return N.Z1, src, None, gates
    gates.append((z2, 0.0, MARGIN_REL * depth_scale))
    if z2 <= 0:
        return N.Z2, src, None, gates
    for code, V, R, t, z, g in ((N.REPROJ1, V1, R1, t1, z1, g1), (N.REPROJ2, V2, R2, t2, z2, g2)):
        x, y = float(R[0] @ X + t[0]), float(R[1] @ X + t[1])
        u, v = float(V["fx"]) * x / z + float(V["cx"]), float(V["fy"]) * y / z + float(V["cy"])
        e2 = (u - float(g["x"])) ** 2 + (v - float(g["y"])) ** 2
        k = 5.991
        if g["u_right"] >= 0:
            e2 += (u - float(V1["mbf"]) / z - float(g["u_right"])) ** 2
            k = 7.8
        bound = k * float(sigma2[int(g["octave"])])
        gates.append((e2, bound, MARGIN_REL * bound))
        if e2 > bound:
            return code, src, None, gates
    d1, d2 = np.linalg.norm(X - V1["Ow"].astype(float)), np.linalg.norm(X - V2["Ow"].astype(float))
    if d1 == 0 or d2 == 0:
        return N.ZERO_DIST, src, None, gates
    rd, ro = d2 / d1, float(scale[int(g1["octave"])]) / float(scale[int(g2["octave"])])
    gates += [(rd * rf, ro, MARGIN_REL * ro), (rd, ro * rf, MARGIN_REL * ro * rf)]
    if rd * rf < ro or rd > ro * rf:
        return N.RATIO, src, None, gates
    return N.ACCEPTED, src, X, gates


def decided(gates):
    return all(abs(q - thr) > m for q, thr, m in gates)


def test_hand_worked_pair():
    """Keyframe 1 at the identity, the neighbour 0.5 to its right, the point (0.5, 0.25, 5): u1 = 370, v = 265,
    u2 = 320.  Mono: cosParallaxRays = (0.1 * 0 + 0.05^2 + 1) / (|(.1, .05, 1)| |(0, .05, 1)|) = 0.99503.. < 0.9998,
    the triangulation returns the point, z1 = z2 = 5, both errors 0, dist2 / dist1 = 5.00625 / 5.03115 = 0.99505."""
    V1, V2 = N.view_dict(C.view()), N.view_dict(C.shifted(0.5))
    g1 = dict(x=370.0, y=265.0, u_right=-1.0, octave=0, kx=370.0, ky=265.0, depth=-1.0)
    g2 = dict(g1, x=320.0, kx=320.0)
    tr = {}
    st, src, X = N.new_map_point(V1, V2, g1, g2, SCALE, SIGMA2, C.RATIO_FACTOR, trace=tr)
    assert (st, src) == (N.ACCEPTED, N.SRC_TRI)
    assert abs(float(tr["cos_rays"]) - 1.0025 / math.sqrt(1.0125 * 1.0025)) < 1e-7
    assert np.allclose(X, (0.5, 0.25, 5.0), rtol=2e-5) and abs(float(tr["ratio_dist"]) - 0.995050) < 1e-5
    assert np.array_equal(tr["A"][0], np.array([-1, 0, 0.1, 0], f32)) and np.array_equal(tr["A"][2], np.array([-1, 0, 0, 0.5], f32))
    # the same point through keyframe 1's stereo depth once the neighbour is nearer than mb
    g1s = dict(g1, u_right=370.0 - 8.0, depth=5.0)
    V2n = N.view_dict(C.shifted(0.05))
    st, src, X = N.new_map_point(V1, V2n, g1s, dict(g2, x=365.0), SCALE, SIGMA2, C.RATIO_FACTOR)
    assert (st, src) == (N.ACCEPTED, N.SRC_STEREO1) and np.array_equal(X, np.array([0.5, 0.25, 5.0], f32))


def test_jacobi_null_vector_on_known_matrices():
    rng = np.random.RandomState(1)
    for _ in range(20):
        A = rng.uniform(-1, 1, (4, 4))
        U, s, Vt = np.linalg.svd(A)
        s[3] = 1e-3 * s[2]
        A = (U * s) @ Vt
        sw = []
        h = N.jacobi_null4(A.astype(f32), sw).astype(float)
        assert sw[0] < N.JACOBI_SWEEPS                   # converged by its own test, not by the cap
        assert abs(abs(h @ Vt[3]) - 1.0) < 1e-4 and abs(np.linalg.norm(h) - 1) < 1e-5
    # the last of equal smallest columns wins, and a zero column never rotates
    Z = np.zeros((4, 4), f32)
    Z[0, 1] = Z[1, 2] = 1
    assert np.array_equal(N.jacobi_null4(Z), np.array([0, 0, 0, 1], f32))


def test_parallax_bound_is_the_cosine():
    for mb, d in ((0.08, 0.3), (0.08, 4.0), (0.5, 2.0), (0.08, 40.0), (0.08, 1000.0)):
        assert abs(float(N.stereo_parallax_bound(mb, d)) - math.cos(2 * math.atan2(float(f32(mb)) / 2, float(f32(d))))) < 6e-8


def test_no_float_equals_a_chi2_product():
    """why `>=` at a chi-square bound is an equivalent reading (newpts_ref.EQUIVALENT)"""
    for k in (5.991, 7.8):
        for l in range(NLEVELS):
            bound = k * float(SIGMA2[l])
            assert float(f32(bound)) != bound
    for name in C.names():
        a, b = C.expected(name), C.reference(C.case(name), mut={"chi2_ge"})
        assert all(np.array_equal(a[k], b[k], equal_nan=True) for k in a), name


def test_every_mutation_is_noticed_by_a_named_case():
    seen = set()
    for name in C.names():
        c, want = C.case(name), C.expected(name)
        for m in c["mutants"]:
            got = C.reference(c, mut={m})
            assert not all(np.array_equal(want[k], got[k], equal_nan=True) for k in want), (name, m)
            seen.add(m)
    assert seen == set(N.MUTATIONS)


def test_cases_reach_what_they_are_for():
    st = {n: C.expected(n)["status"] for n in C.names()}
    every = np.concatenate([s.ravel() for s in st.values()])
    assert set(np.unique(every)) == set(range(10))               # every way out of the loop body
    src = np.concatenate([C.expected(n)["source"].ravel() for n in C.names()])
    assert set(np.unique(src)) == {0, 1, 2, 3}
    assert st["w_zero"].tolist() == [[N.W_ZERO]] and st["zero_distance"].tolist() == [[N.ZERO_DIST]]
    # z on 0 and one float below it leave at the depth test; one float above goes on (to the stereo reprojection
    # test, which keyframe 1's u_right fails / to acceptance), as the feature well above does
    assert st["z1"][0].tolist() == [N.Z1, N.REPROJ1, N.Z1, N.REPROJ1]
    assert st["z2"][0].tolist() == [N.Z2, N.ACCEPTED, N.Z2, N.ACCEPTED]
    assert st["zero_distance2"].tolist() == [[N.ZERO_DIST]] and C.expected("zero_distance2")["source"].tolist() == [[N.SRC_STEREO1]]
    assert st["ratio"][0].tolist() == [N.RATIO, N.RATIO, N.ACCEPTED, N.ACCEPTED, N.ACCEPTED, N.RATIO, N.ACCEPTED, N.RATIO]
    assert C.expected("first_ok")["first_ok"].tolist() == [0, 2, 5, -1, 1]
    assert st["shared_idx2"].tolist() == [[1, 1]] and C.expected("shared_idx2")["match"].tolist() == [[0, 0]]
    assert [len(C.case("pairs_%d" % L)["kfs"][0]["node"]) for L in (1, 63, 64, 65, 130)] == [1, 63, 64, 65, 130]
    assert C.expected("pairs_130")["nmatches"].tolist() == [130] and len(C.case("nnb32")["slots2"]) == 32
    par = C.expected("parallax")
    assert par["status"][0, :3].tolist()[0] == N.LOW_PARALLAX and par["source"][0, 2] != par["source"][0, 1]
    assert {1, 2, 3} <= set(par["source"][1:3].ravel().tolist())
    assert par["status"][3, -1] == N.LOW_PARALLAX and par["source"][4, -1] == N.SRC_TRI      # either side of 0.9998
    # only_stereo changes the search, not the loop body
    assert C.expected("pairs_65", True)["nmatches"][0] < C.expected("pairs_65")["nmatches"][0]
    assert max(len(k["node"]) for n in C.names() for k in C.case(n)["kfs"]) <= 200


@pytest.fixture(scope="module")
def scene_vs_model():
    c, r = C.random_scene(), C.reference(C.random_scene())
    V = [N.view_dict(v) for v in c["views"]]
    rows = []
    for j, s2 in enumerate(c["slots2"]):
        for i in np.flatnonzero(r["match"][j] >= 0):
            g1, g2 = N.feature(c["kfs"][0], i), N.feature(c["kfs"][s2], int(r["match"][j, i]))
            st, src, X, gates = model64(V[0], V[s2], g1, g2, SCALE, SIGMA2, float(C.RATIO_FACTOR))
            rows.append((j, i, st, src, X, decided(gates)))
    return r, rows


def test_scene_status_equals_the_float64_model_on_decided_pairs(scene_vs_model):
    r, rows = scene_vs_model
    assert len(rows) >= 400
    undecided = [q for q in rows if not q[5]]
    print("pairs %d, undecided %d" % (len(rows), len(undecided)))
    assert len(undecided) <= 0.05 * len(rows)
    for j, i, st, src, X, ok in rows:
        if ok:
            assert (r["status"][j, i], r["source"][j, i]) == (st, src), (j, i)
    kinds = {q[2] for q in rows if q[5]}
    assert {N.ACCEPTED, N.LOW_PARALLAX} <= kinds and {q[3] for q in rows if q[5]} >= {1, 2, 3}


def test_scene_x3d_against_the_float64_model(scene_vs_model):
    r, rows = scene_vs_model
    dev = [np.linalg.norm(r["x3d"][j, i].astype(float) - X) / np.linalg.norm(X)
           for j, i, st, src, X, ok in rows if ok and st == N.ACCEPTED]
    print("x3D: %d pairs, largest relative deviation %.3g" % (len(dev), max(dev)))
    assert len(dev) >= 300 and max(dev) <= 2 * X3D_MEASURED
