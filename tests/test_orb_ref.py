"""The extractor's per-level work twice: the oracle's C restatement (oc_level_candidates,
oc_ic_angle_moments, oc_gaussian_blur7, oc_orb_descriptor, oc_extract) against the numpy model of
tests/orb_ref.py, and the directed frames of tests/test_gpu_orb_directed.py against the regimes
they are named after (no GPU).

First the model is pinned by itself on cases worked by hand; then the oracle is compared with it on
every directed frame and a few random ones; then one-line mutants of the model must each fail a
named directed frame (MUTANTS: DESIGN.md s2.2 lists which case catches which)."""
import math

import numpy as np
import pytest

import orb_ref as R

FRAMES = R.frames()
RANDOM = {f.name: f for f in R.random_frames()}
ALL = dict(FRAMES, **RANDOM)


# ------------------------------------------------------------------ the model by itself
def ring_patch(n, s, sense, v=100):
    """15 x 15 patch of v with ring pixels s .. s + n - 1 of the centre at v + sense"""
    p = np.full((15, 15), v, np.uint8)
    for k in range(n):
        dx, dy = R.RING[(s + k) % 16]
        p[7 + dy, 7 + dx] = v + sense
    return p


@pytest.mark.parametrize("sense", [40, -40])
def test_model_arcs_of_8_and_9(sense):
    """9 contiguous ring pixels 40 off the centre: corner for t < 40, score 39; 8: never.  Every
    start index, so arcs wrapping ring index 15 -> 0 are included."""
    for s in range(16):
        assert R.fast_strength(ring_patch(9, s, sense))[7, 7] == 40, s
        assert R.fast_strength(ring_patch(8, s, sense))[7, 7] == 0, s
        # 9 pixels that are not contiguous (a gap after the 4th)
        p = ring_patch(4, s, sense)
        q = ring_patch(5, s + 5, sense)
        assert R.fast_strength(np.where(q != 100, q, p))[7, 7] == 0, s
    xs, ys, sc = R.fast_roi(R.fast_strength(ring_patch(9, 13, sense)), 20)
    assert (7, 7, 39) in list(zip(xs.tolist(), ys.tolist(), sc.tolist()))


def test_model_threshold_equalities():
    """A lone pixel d above a flat patch has M = d: a corner at t iff d > t, score d - 1."""
    for t in (7, 20):
        for d, n in ((t, 0), (t + 1, 1)):
            p = np.full((9, 9), 100, np.uint8)
            p[4, 4] = 100 + d
            M = R.fast_strength(p)
            assert M[4, 4] == d and M.sum() == d
            xs, ys, sc = R.fast_roi(M, t)
            assert len(xs) == n and (n == 0 or (xs[0], ys[0], sc[0]) == (4, 4, d - 1))
    # the 3-px inset: a pixel 2 px from the ROI's edge has no strength
    p = np.full((9, 9), 100, np.uint8)
    p[2, 4] = 200
    assert R.fast_strength(p).sum() == 0


def test_model_nms_tie():
    """Equal neighbours suppress each other; a neighbour that is no corner at t scores 0."""
    p = np.full((9, 10), 100, np.uint8)
    p[4, 4] = p[4, 5] = 150
    M = R.fast_strength(p)
    assert M[4, 4] == 50 and M[4, 5] == 50
    assert len(R.fast_roi(M, 20)[0]) == 0 and len(R.fast_roi(M, 7)[0]) == 0
    p[4, 5] = 115                                   # M = 15: a corner at 7, none at 20
    M = R.fast_strength(p)
    assert [v.tolist() for v in R.fast_roi(M, 20)] == [[4], [4], [49]]
    assert [v.tolist() for v in R.fast_roi(M, 7)] == [[4], [4], [49]]
    p[4, 5] = 151                                   # the stronger one wins, at both thresholds
    assert [v.tolist() for v in R.fast_roi(R.fast_strength(p), 20)] == [[5], [4], [50]]


def test_model_disc():
    umax = R.make_umax()
    assert umax == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
    m = R.disc_mask()
    assert m.sum() == sum(2 * umax[abs(v)] + 1 for v in range(-15, 16)) == 749
    assert np.array_equal(m, m.T) and np.array_equal(m, m[::-1]) and np.array_equal(m, m[:, ::-1])
    assert m[0].sum() == 7 and m[15].sum() == 31


def test_model_half_planes():
    """Half-plane images: image x (u) grows to the right and y (v) downwards, so a bright lower half
    is m01 > 0: 90 degrees."""
    u = np.arange(41)
    for name, img, ang in (("right", np.where(u[None, :] > 20, 255, 0) + 0 * u[:, None], 0.0),
                           ("below", np.where(u[:, None] > 20, 255, 0) + 0 * u[None, :], 90.0),
                           ("left", np.where(u[None, :] < 20, 255, 0) + 0 * u[:, None], 180.0),
                           ("above", np.where(u[:, None] < 20, 255, 0) + 0 * u[None, :], 270.0)):
        m01, m10 = R.ic_moments(img.astype(np.uint8), 20, 20)
        assert R.ic_angle(m01, m10) == ang, name
        assert max(abs(m01), abs(m10)) == 255 * sum(sum(range(1, R.make_umax()[abs(v)] + 1)) for v in range(-15, 16))
        assert min(abs(m01), abs(m10)) == 0
    assert R.ic_angle(0, 0) == 0.0


def test_model_descriptor_at_angle_zero():
    """At angle 0 the rotation is the identity: bit k = I(pattern[2k]) < I(pattern[2k + 1])."""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (41, 41), dtype=np.uint8)
    pat = R.pattern()
    desc, und = R.brief(img, 20, 20, np.float32(0.0))
    bits = [int(img[20 + pat[2 * k][1], 20 + pat[2 * k][0]] < img[20 + pat[2 * k + 1][1], 20 + pat[2 * k + 1][0]])
            for k in range(256)]
    assert R.unpack_bits(desc).tolist() == bits and not und.any()
    # 90 degrees: (x, y) -> row x, column -y
    desc90, _ = R.brief(img, 20, 20, np.float32(90.0))
    bits90 = [int(img[20 + pat[2 * k][0], 20 - pat[2 * k][1]] < img[20 + pat[2 * k + 1][0], 20 - pat[2 * k + 1][1]])
              for k in range(256)]
    assert R.unpack_bits(desc90).tolist() == bits90
    # 30 degrees: sin = 0.5 puts odd pattern coordinates on half-integers: undecided
    assert R.brief(img, 20, 20, np.float32(30.0))[1].sum() > 16


def test_model_blur_and_rounding():
    assert R.GAUSS_Q8.sum() == 256
    assert (R.blur7(np.full((9, 12), 77, np.uint8)) == 77).all()
    img = np.zeros((9, 9), np.uint8)
    img[4, 4] = 255
    b = R.blur7(img)
    assert b[4, 4] == (255 * 56 * 56 + 32768) >> 16 and b[4, 1] == (255 * 56 * 18 + 32768) >> 16
    # REFLECT_101 at the corner: pixel (0, 0) sees (1, 1) through offsets (-1, -1), (1, 1), (-1, 1), (1, -1)
    img = np.zeros((9, 9), np.uint8)
    img[1, 1] = 255
    assert R.blur7(img)[0, 0] == (255 * (48 + 48) * (48 + 48) + 32768) >> 16
    assert R.round_half_even(np.array([0.5, 1.5, -0.5, -1.5, 2.5])).tolist() == [0, 2, 0, -2, 2]
    assert R.round_half_away(np.array([0.5, 1.5, -0.5, -1.5, 2.5])).tolist() == [1, 2, -1, -2, 3]


def test_sample_ties_round_to_even(oracle_mod):
    """The one place where cvRound's tie rule shows: at 30 degrees the canonical float sine is exactly
    0.5f, so a pattern point (x, 0) with odd x has the row coordinate x / 2 exactly, in the oracle's
    float fma as in float64.  The model, given that sine and cosine, must give the oracle's bits on
    every test that is decided or an exact tie; rounding ties away from zero instead changes some."""
    s, c = oracle_mod.sincos(float(np.float32(np.float32(30.0) * np.float32(R.FACTOR_PI))))
    assert s == 0.5 and c == float(np.float32(math.sqrt(0.75)))
    pat = R.pattern()
    img = np.random.default_rng(9).integers(0, 256, (41, 41), dtype=np.uint8)
    fr = pat[:, 0] * s + pat[:, 1] * c
    fc = pat[:, 0] * c - pat[:, 1] * s
    tie = ((fr - np.floor(fr) == 0.5) | (fc - np.floor(fc) == 0.5))
    tie = tie[0::2] | tie[1::2]
    assert tie.sum() >= 16 and (pat[:, 1] == 0).sum() >= 8
    ref = R.unpack_bits(oracle_mod.orb_descriptor(img, 20, 20, 30.0, pat))
    desc, und = R.brief(img, 20, 20, np.float32(30.0), sincos=(s, c))
    use = tie | ~und
    assert use.sum() > 240 and np.array_equal(R.unpack_bits(desc)[use], ref[use])
    away, _ = R.brief(img, 20, 20, np.float32(30.0), sincos=(s, c), rnd=R.round_half_away)
    assert not np.array_equal(R.unpack_bits(away)[use], ref[use])


# ------------------------------------------------------------------ oracle against model
class Both:
    """oracle and model results of one frame"""

    def __init__(self, O, fr):
        self.fr = fr
        self.ex = O.Extractor(fr.nfeatures, 1.2, fr.nlevels, 20, 7)
        self.o = self.ex.extract(fr.img, debug=True)
        self.m = fr.model(angles=self.o["kps"]["angle"])
        self.sizes = self.ex.level_sizes(fr.w, fr.h)
        self.olevels = [fr.img] + [self.o["pyramid"][self.o["level_off"][l]:self.o["level_off"][l] + lw * lh].reshape(lh, lw)
                                   for l, (lw, lh) in enumerate(self.sizes) if l > 0]


_both = {}


@pytest.fixture
def both(oracle_mod, request):
    name = request.param
    if name not in _both:
        _both[name] = Both(oracle_mod, ALL[name])
    return _both[name]


def compare_records(kps, desc, m, bound, tag):
    """keypoints and descriptors of an extractor under test against the model `m` (run with that
    extractor's own angles): every field but the angle exact, the angle within `bound` of float64
    atan2 modulo 360, every decided descriptor bit equal.  Returns (undecided bits, worst angle)."""
    assert len(kps) == len(m["kps"]), (tag, len(kps), len(m["kps"]))
    for f in R.KP_DTYPE.names:
        if f != "angle":
            bad = np.nonzero(kps[f] != m["kps"][f])[0]
            assert len(bad) == 0, (tag, f, len(bad), kps[bad[:3]], m["kps"][bad[:3]])
    worst = max([R.angle_diff(a, b) for a, b in zip(kps["angle"], m["angle64"])], default=0.0)
    assert worst <= bound, (tag, "angle", worst, bound)
    if len(kps) == 0:
        return 0, worst
    diff = (R.unpack_bits(desc) != R.unpack_bits(m["desc"])) & ~m["und"]
    assert not diff.any(), (tag, "descriptor bits", int(diff.sum()), np.nonzero(diff.any(axis=1))[0][:5].tolist())
    return int(m["und"].sum()), worst


@pytest.mark.parametrize("both", sorted(ALL), indirect=True)
def test_oracle_equals_model(oracle_mod, both):
    b, O = both, oracle_mod
    assert [l.shape[::-1] for l in b.m["levels"]] == b.sizes
    pat = R.pattern()
    for l, lvl in enumerate(b.olevels):
        assert np.array_equal(lvl, b.m["levels"][l]), ("pyramid level", l)
        assert np.array_equal(O.gaussian_blur7(lvl), b.m["blurred"][l]), ("blurred level", l)
        xs, ys, sc = O.level_candidates(lvl)
        mx, my, ms = R.flatten(b.m["cells"][l])
        assert (xs.tolist(), ys.tolist(), sc.tolist()) == (mx, my, ms), ("candidates of level", l, len(xs), len(mx))
    assert b.o["ncand"] == [sum(len(c["xs"]) for c in cells) for cells in b.m["cells"]]
    compare_records(b.o["kps"], b.o["desc"], b.m, R.ANGLE_BOUND, b.fr.name)
    # the per-keypoint entry points, on the model's levels
    umax = list(b.ex.p.umax)
    for i in range(0, len(b.o["kps"]), max(1, len(b.o["kps"]) // 40)):
        l, x, y = int(b.m["kps"]["octave"][i]), int(b.m["lx"][i]), int(b.m["ly"][i])
        assert O.ic_angle_moments(b.m["levels"][l], x, y, umax) == (b.m["m01"][i], b.m["m10"][i]), i
        assert O.fast_atan2(float(b.m["m01"][i]), float(b.m["m10"][i])) == b.o["kps"]["angle"][i]
        assert np.array_equal(O.orb_descriptor(b.m["blurred"][l], x, y, b.o["kps"]["angle"][i], pat), b.o["desc"][i])


# ------------------------------------------------------------------ regimes
def cell_of(cells, i, j):
    return next(c for c in cells if (c["i"], c["j"]) == (i, j))


def keys_abs(c):
    return [(int(x) + 16, int(y) + 16, int(s)) for x, y, s in zip(c["xs"], c["ys"], c["score"])]


def check_regime(fr, m):
    """what each frame is there to reach, from the model alone"""
    g, info = fr.regime, fr.info
    kv = R.kernel_view(fr.w, fr.h, m["tab"])
    kp = m["kps"]
    at = {(int(x), int(y)): i for i, (x, y, o) in enumerate(zip(m["lx"], m["ly"], kp["octave"])) if o == 0}
    M0 = R.fast_strength(fr.img)
    if g == "arcs":
        assert len(info["centres"]) == 64
        for cx, cy, n, s, sense in info["centres"]:
            assert M0[cy, cx] == (40 if n == 9 else 0), (cx, cy, n, s, sense)
        assert {s for _, _, n, s, _ in info["centres"] if n == 9} == set(range(16))
        cand = {k[:2] for c in m["cells"][0] for k in keys_abs(c)}
        assert all(((cx, cy) in cand) == (n == 9) for cx, cy, n, _, _ in info["centres"])
    elif g == "thresholds":
        for (i, j), (th, keys) in info["expect"].items():
            c = cell_of(m["cells"][0], i, j)
            assert c["th"] == th and keys_abs(c) == keys, ((i, j), c["th"], keys_abs(c))
    elif g == "saturation":
        assert all(M0[y, x] == 255 for x, y in info["points"])
        assert {int(fr.img[y, x]) for x, y in info["points"]} == {0, 255}
        assert sorted(at) == sorted(p for p in info["points"]) and (kp["response"] == 254).all()
    elif g == "nms_ties":
        gr = info["groups"]
        assert all(M0[y, x] == 50 for pts in gr.values() for x, y in pts)
        cells = m["cells"][0]
        for i, j in ((0, 0), (1, 0), (1, 3)):       # only the tie: empty after both passes
            c = cell_of(cells, i, j)
            assert c["th"] is None and c["ncorn_min"] in (2, 3), ((i, j), c)
        c = cell_of(cells, 1, 1)                    # the tie empties the iniTh pass, minTh finds the weak corner
        assert c["th"] == 7 and keys_abs(c) == [(75, 95, 9)] and c["ncorn_min"] == 3
        # a pair split by a cell border: each half is alone in its cell's window
        assert keys_abs(cell_of(cells, 0, 2)) == [(114, 40, 49), (100, 62, 49)]
        assert keys_abs(cell_of(cells, 0, 3)) == [(115, 40, 49)] and keys_abs(cell_of(cells, 1, 2)) == [(100, 63, 49)]
        assert keys_abs(cell_of(cells, 0, 1)) == []
        # five candidates, three keypoints: the octree cannot part adjacent keys (its list stops growing
        # once every node has one non-empty child) and keeps the first of each pair
        assert [(int(x), int(y)) for x, y in zip(kp["x"], kp["y"])] == [(114, 40), (100, 62), (75, 95)]
    elif g == "corner_count":
        cells = m["cells"][0]
        c = cell_of(cells, 0, 1)
        assert c["ncorn_min"] == info["n"] and (info["n"] > R.FAST_CORNERS) == (info["n"] == 257)
        assert cell_of(cells, 0, 0)["ncorn_min"] == 0 and cell_of(cells, 0, 0)["th"] is None
        k = next(k for k in kv["levels"][0]["cells"] if (k["i"], k["j"]) == (0, 1))
        # the entry list is drained in mid-cell: more than 64 entries before the last pass
        assert R.entries_before_last_pass(fr.img, c, k, 7) > R.FAST_ENTRIES - 64
        assert kv["row_bytes"] == 96
    elif g == "count":
        assert len(kp) == info["n"] and sorted(at) == sorted(info["points"])
    elif g == "moments":
        D = 255 * sum(sum(range(1, R.make_umax()[abs(v)] + 1)) for v in range(-15, 16))
        for name, (cx, cy, ang) in info["centres"].items():
            assert (cx, cy) in at, (name, "is no keypoint")
            i = at[(cx, cy)]
            m01, m10 = int(m["m01"][i]), int(m["m10"][i])
            assert m["angle64"][i] == ang, (name, m01, m10, m["angle64"][i])
            if name.startswith("zero"):
                assert m01 == 0 and m10 == 0
            elif name in ("east", "west"):
                assert m01 == 0 and abs(m10) == D
            elif name in ("north", "south"):
                assert m10 == 0 and abs(m01) == D
            elif len(name) == 2:
                assert abs(m01) == abs(m10) > 0
        c = info["centres"]["east_weak"]
        assert M0[c[1], c[0]] == 20 and kp["response"][at[c[:2]]] == 19
    elif g == "span":
        assert kp["octave"].tolist() == [0, 0, 0, 1, 1, 1, 2, 2]          # one wave of k_describe, three levels
    elif g in ("noise96", "noise72", "single91", "single62"):
        assert kv["row_bytes"] == (96 if g in ("noise96", "single62") else 72)
        if g == "single91":
            assert (kv["levels"][1]["w"], len(kv["levels"][1]["cells"]), kv["max_roi_w"]) == (91, 1, 59)
        if g == "single62":
            assert (kv["levels"][1]["w"], len(kv["levels"][1]["cells"]), kv["max_roi_w"]) == (62, 1, 42)
        if g == "noise72":
            assert len(kv["levels"][2]["cells"]) == 1 and 47 <= kv["max_roi_w"] <= 59
        if g == "noise96":
            ww = {c["ww"] for lv in kv["levels"] for c in lv["cells"]}
            assert {w % 4 for w in ww} == {0, 1, 2, 3} and {c["ngrp"] for lv in kv["levels"] for c in lv["cells"]} >= {8, 9}
        if g == "single91":       # width 109: level 0's pitch is no multiple of 16 (k_describe's byte path)
            assert {int(v) for v in (m["lx"][kp["octave"] == 0] - 15) & 15} == set(range(16))
        if g in ("noise96", "noise72"):
            for l, (lw, lh) in enumerate((lv["w"], lv["h"]) for lv in kv["levels"]):
                on = kp["octave"] == l
                x, y = m["lx"][on], m["ly"][on]
                assert {int(v) for v in (x - 15) & 15} == set(range(16)), (l, "alignments")
                assert x.min() == 19 and x.max() == lw - 20 and y.min() == 19 and y.max() == lh - 20, (l, "edges")
                assert {int(v) for v in (y + 18) // 8 - (y - 18) // 8 + 1} == {5, 6}, (l, "tile rows")
    elif g == "random":
        assert len(kp) > 50
    else:
        raise AssertionError("unknown regime " + g)


@pytest.mark.parametrize("both", sorted(ALL), indirect=True)
def test_frames_reach_their_regimes(both):
    check_regime(both.fr, both.m)


def test_frame_set_covers_the_launch_shapes():
    """over the whole set: both slab layouts, level widths 62 and 91, every ww mod 4, ngrp 8 and 9,
    keypoint totals 0, 1, 7, 8, 9, 17"""
    rb, widths, ww, ngrp = set(), set(), set(), set()
    for fr in ALL.values():
        kv = R.kernel_view(fr.w, fr.h, R.Tables(fr.nfeatures, 1.2, fr.nlevels))
        rb.add(kv["row_bytes"])
        for lv in kv["levels"]:
            widths.add(lv["w"])
            ww |= {c["ww"] % 4 for c in lv["cells"]}
            ngrp |= {c["ngrp"] for c in lv["cells"]}
    assert rb == {72, 96} and {62, 91} <= widths and ww == {0, 1, 2, 3} and {8, 9} <= ngrp
    assert min(min(fr.w, fr.h) for fr in ALL.values()) == 64 and max(fr.w for fr in ALL.values()) == 160
    assert {fr.w % 16 == 0 for fr in ALL.values()} == {True, False}       # level-0 vector and byte paths


# ------------------------------------------------------------------ tolerances and caps
def test_angle_bound(oracle_mod):
    """fastAtan2 (the oracle's) against float64 atan2 over 120 001 directions at seven lengths and
    over every directed keypoint's moments: the largest deviation is R.ANGLE_MEASURED, the bound on
    |extractor - model| twice that, and it stays below the 0.02 degrees of test_fast_atan2_properties."""
    worst = 0.0
    n = 120001
    for k in range(n):
        th = 2 * math.pi * k / n
        r = 1000.0 * (1 + k % 7)
        y, x = float(np.float32(r * math.sin(th))), float(np.float32(r * math.cos(th)))
        worst = max(worst, R.angle_diff(oracle_mod.fast_atan2(y, x), R.ic_angle(y, x)))
    for name in sorted(FRAMES):
        if name not in _both:
            _both[name] = Both(oracle_mod, FRAMES[name])
        m = _both[name].m
        for m01, m10 in zip(m["m01"], m["m10"]):
            worst = max(worst, R.angle_diff(oracle_mod.fast_atan2(float(m01), float(m10)), R.ic_angle(m01, m10)))
    print("largest |fastAtan2 - atan2|: %.6f degrees" % worst)
    assert worst <= R.ANGLE_MEASURED
    assert R.ANGLE_BOUND == 2 * R.ANGLE_MEASURED < 0.02


def test_undecided_bits_cap(oracle_mod):
    """At most 1 % of all descriptor bits undecided over the directed and random frames, and no
    keypoint with more than 16 of its 256 (no directed angle has a sine or cosine of 0.5)."""
    und = total = 0
    for name in sorted(ALL):
        if name not in _both:
            _both[name] = Both(oracle_mod, ALL[name])
        u = _both[name].m["und"]
        und += int(u.sum())
        total += u.size
        assert u.size == 0 or u.sum(axis=1).max() <= 16, (name, int(u.sum(axis=1).max()))
    print("undecided bits: %d of %d (%.4f %%)" % (und, total, 100.0 * und / total))
    assert und <= 0.01 * total


# ------------------------------------------------------------------ mutants
def _mutant_nms_ge():
    orig = R.fast_roi

    def fast_roi_ge(M, t):
        h, w = M.shape
        S = np.zeros((h, w), np.int32)
        S[3:h - 3, 3:w - 3] = np.where(M[3:h - 3, 3:w - 3] > t, M[3:h - 3, 3:w - 3] - 1, 0)
        P = np.pad(S, 1)
        keep = S > 0
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dx or dy:
                    keep &= S >= P[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
        ys, xs = np.nonzero(keep)
        return xs, ys, S[ys, xs]
    return "fast_roi", orig, fast_roi_ge


def _mutant_corner_ge():
    orig = R.fast_roi
    return "fast_roi", orig, lambda M, t: orig(M, t - 1)          # M > t - 1 <=> M >= t


def _mutant_umax15():
    orig = R.disc_mask
    return "disc_mask", orig, lambda umax=None: orig(R.make_umax()[:15] + [4])


MUTANTS = [("nms_gt_to_ge", _mutant_nms_ge, {}, "nms_ties"),
           ("corner_gt_to_ge", _mutant_corner_ge, {}, "threshold_equalities"),
           ("umax15_3_to_4", _mutant_umax15, {}, "moments"),
           ("t0_lt_to_le", None, dict(le=True), "keypoints_8"),
           ("fallback_per_level", None, dict(per_level_fallback=True), "threshold_equalities")]


@pytest.mark.parametrize("name,patch,mut,frame", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_mutant_fails_a_named_frame(oracle_mod, monkeypatch, name, patch, mut, frame):
    """Each one-line change of the model makes the oracle-versus-model comparison of the named
    directed frame fail: the frames name the edge a broken extractor would get wrong."""
    fr = FRAMES[frame]
    o = oracle_mod.Extractor(fr.nfeatures, 1.2, fr.nlevels, 20, 7).extract(fr.img, debug=True)
    good = fr.model(angles=o["kps"]["angle"])
    compare_records(o["kps"], o["desc"], good, R.ANGLE_BOUND, frame)
    if patch is not None:
        attr, _, new = patch()
        monkeypatch.setattr(R, attr, new)
    bad = R.extract(fr.img, fr.nfeatures, 1.2, fr.nlevels, 20, 7, angles=o["kps"]["angle"], **mut)
    if name == "umax15_3_to_4":
        # the moments are compared exactly: the half-plane tiles' differ by the two extra pixels' worth
        umax = R.make_umax()
        got = [oracle_mod.ic_angle_moments(fr.img, int(x), int(y), umax) for x, y in zip(good["lx"], good["ly"])]
        assert got == list(zip(good["m01"].tolist(), good["m10"].tolist()))
        assert got != list(zip(bad["m01"].tolist(), bad["m10"].tolist()))
        return
    with pytest.raises(AssertionError):
        compare_records(o["kps"], o["desc"], bad, R.ANGLE_BOUND, frame)
