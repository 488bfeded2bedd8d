"""k_blur_rows' band structure and k_fast's slab layouts against the CPU oracle, bit for bit
(MI355X only).

k_blur_rows gives a wave one band of 32 rows of four 56-column strips: 6 prologue rows, blocks of
8 source rows with a tile flush after each, a last block of 1..7 rows in the last band of a level;
interior bands step a scalar row offset, the first and last band reflect every row index.  The
cases below reach each of these through the extractor:

  size      scale  levels  level heights -> bands (rows of the last band)   widths -> live strips of the last quad
  97 x 71   1.2    1       71 -> 3 (7)                                      97 -> 2
  97 x 71   1.13   2       71 -> 3 (7), 63 -> 2 (31: no interior band)      97 -> 2, 86 -> 2
  233 x 101 1.2    3       101 -> 4 (5), 84 -> 3 (20), 70 -> 3 (6)          233 -> 1, 194 -> 4, 162 -> 3

A level must hold the 30-px FAST grid (width and height >= 62) or the plan is refused, so no
level has a single band (height <= 32); two bands (62..64 rows) is the smallest a plan reaches.
"""
import numpy as np
import pytest

from coeb_front import Context

from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

BLUR_CASES = [(97, 71, 1.2, 1), (97, 71, 1.13, 2), (233, 101, 1.2, 3)]


def level_bands(h, brows=32):
    """(number of bands, rows of the last band) of a level of h rows."""
    n = (h + brows - 1) // brows
    return n, h - (n - 1) * brows


def noise_frames(w, h, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(n)]


def border_frame(w, h, seed):
    """Smooth interior, top 3 and bottom 3 rows alternating 0 / 255 against it: a REFLECT_101 row
    taken from the wrong source row changes the blurred rows 0..2 and h-3..h-1."""
    rng = np.random.default_rng(seed)
    g = (96 + 32 * np.sin(np.arange(w) / 9.0)[None, :] + 24 * np.cos(np.arange(h) / 7.0)[:, None]).astype(np.uint8)
    g = np.ascontiguousarray(g + rng.integers(0, 4, (h, w), dtype=np.uint8))
    for r, v in ((0, 255), (1, 0), (2, 255), (h - 3, 0), (h - 2, 255), (h - 1, 0)):
        g[r, :] = v
    g[1, ::3] = 200
    g[h - 2, ::5] = 30
    return g


def check_blur(c, ex, oracle_mod, gray, tag):
    """Every blurred pixel of every level (and the raw pyramid) against the oracle: the
    comparison of test_gpu_parity.test_blur_pyramid_matches_oracle."""
    h, w = gray.shape
    r = ex.extract(gray, debug=True)
    k, d = c.extract(gray)
    assert_same(k, d, r["kps"], r["desc"], tag)
    blur = c.debug_read("blur")
    pyr = c.debug_read("pyr")
    off = poff = 0
    for l, (lw, lh) in enumerate(ex.level_sizes(w, h)):
        lvl = gray if l == 0 else r["pyramid"][r["level_off"][l]:r["level_off"][l] + lw * lh].reshape(lh, lw)
        if l > 0:
            pp = (lw + 63) // 64 * 64
            gotp = pyr[poff:poff + pp * lh].reshape(lh, pp)[:, :lw]
            assert np.array_equal(gotp, lvl), (tag, "pyramid level", l)
            poff = (poff + pp * lh + 255) // 256 * 256
        ref = oracle_mod.gaussian_blur7(lvl)
        pitch = (lw + 63) // 64 * 64
        got = blur[off:off + pitch * lh].reshape(lh, pitch)[:, :lw]
        bad = np.argwhere(got != ref)
        assert len(bad) == 0, (tag, "level", l, (lw, lh), len(bad), bad[:4].tolist())
        off = (off + pitch * lh + 255) // 256 * 256


@pytest.mark.parametrize("w,h,scale,nlev", BLUR_CASES)
def test_blur_band_structure(oracle_mod, w, h, scale, nlev):
    ex = oracle_mod.Extractor(1000, scale, nlev, 20, 7)
    sizes = ex.level_sizes(w, h)
    bands = [level_bands(lh) for _, lh in sizes]
    # the case reaches what the table in the module docstring says
    if (w, h, nlev) == (97, 71, 2):
        assert bands[1][0] == 2, bands
    else:
        assert all(n >= 3 and 1 <= last <= 7 for n, last in bands[:1]), bands
    if w == 233:
        assert [((lw + 55) // 56 - 1) % 4 + 1 for lw, _ in sizes] == [1, 4, 3]
        assert all(lw % 56 and lw % 16 for lw, _ in sizes)
    c = Context(1000, scale, nlev, 20, 7, max_width=w, max_height=h)
    try:
        for i, g in enumerate(noise_frames(w, h, 2, seed=w * 3 + nlev)):
            check_blur(c, ex, oracle_mod, g, "%dx%d L%d f%d" % (w, h, nlev, i))
    finally:
        c.close()


def test_blur_reflection_rows(oracle_mod):
    w, h = 233, 101
    ex = oracle_mod.Extractor(1000, 1.2, 3, 20, 7)
    c = Context(1000, 1.2, 3, 20, 7, max_width=w, max_height=h)
    try:
        for i in range(2):
            g = border_frame(w, h, seed=i)
            # the border rows do change the reference: a frame with the interior rows reflected
            # into them blurs differently in rows 0..2 and h-3..h-1
            g2 = g.copy()
            g2[:3] = g[3:6]
            g2[h - 3:] = g[h - 6:h - 3]
            b1, b2 = oracle_mod.gaussian_blur7(g), oracle_mod.gaussian_blur7(g2)
            assert (b1[:3] != b2[:3]).any() and (b1[h - 3:] != b2[h - 3:]).any()
            check_blur(c, ex, oracle_mod, g, "reflect f%d" % i)
    finally:
        c.close()


def fast_frame(seed):
    """160 x 120, two levels (every ROI <= 46 wide: the 96-byte slab by default).  Level 0 has
    4 x 2 cells of 32 x 44 detection pixels from (19, 19).  Left half flat (cells with no corner
    even at minThFAST) with single bright pixels on the first / last detection row and column of
    cells (0, 0) and (1, 1); right half noise (more than 256 corners in a cell)."""
    rng = np.random.default_rng(seed)
    g = np.full((120, 160), 60, np.uint8)
    g[:, 84:] = rng.integers(0, 256, (120, 76), dtype=np.uint8)
    for x, y in ((19, 19), (50, 30), (30, 62), (51, 63), (82, 106), (60, 63 + 43)):
        g[y, x] = 255
    return g


def test_fast_both_slab_layouts(oracle_mod, monkeypatch):
    ex = oracle_mod.Extractor(1000, 1.2, 2, 20, 7)
    c = Context(1000, 1.2, 2, 20, 7, max_width=160, max_height=120)
    try:
        for rb in (None, "72"):
            if rb:
                monkeypatch.setenv("COEB_FAST_RB", rb)
            for i in range(2):
                g = fast_frame(seed=11 + i)
                r = ex.extract(g, debug=True)
                k, d = c.extract(g)
                cn = c.debug_read("cand_n").view(np.int32)
                tag = "rb%s f%d" % (rb or "96", i)
                assert int(cn.sum()) == sum(r["ncand"]), (tag, int(cn.sum()), r["ncand"])
                assert (cn == 0).any() and cn.max() > 0, (tag, cn.tolist())
                assert_same(k, d, r["kps"], r["desc"], tag)
    finally:
        c.close()


def test_extract_match_640x480_three_frames(oracle_mod):
    """The bench's plan (640 x 480, 8 levels, 1000 keypoints, extract + SearchByProjection) at
    the smallest batch: 3 frames through the batch pipeline against the oracle."""
    from coeb_front import synth
    from coeb_front.pipeline import BatchPipeline
    ex = oracle_mod.Extractor()
    F = 3
    fr = synth.make_frames(640, 480, F, seed=1000)
    depth = synth.make_depth(640, 480)
    Tc = synth.motion_pose()
    bp = BatchPipeline(640, 480, F)
    try:
        bp.load(fr, Tcw=np.stack([Tc] * F))
        bp.run()
        bp.synchronize()
        out, matches, nms = bp.results()
    finally:
        bp.close()
    refs = [ex.extract(fr[f]) for f in range(F)]
    for f in range(F):
        assert_same(out[f][0], out[f][1], refs[f]["kps"], refs[f]["desc"], "f%d" % f)
    cam_o = oracle_mod.camera(ex, 640, 480, synth.TUM_FX, synth.TUM_FY, synth.TUM_CX, synth.TUM_CY, synth.TUM_BF)
    I4 = np.eye(4, dtype=np.float32)
    for f in range(1, F):
        last = oracle_mod.mapframe_from_extraction(refs[f - 1]["kps"], refs[f - 1]["desc"], depth, synth.TUM_FX,
                                                   synth.TUM_FY, synth.TUM_CX, synth.TUM_CY, synth.TUM_BF)
        ur, _ = oracle_mod.stereo_from_rgbd(refs[f]["kps"], depth, synth.TUM_BF)
        nm_ref, m_ref = oracle_mod.search_by_projection(cam_o, refs[f]["kps"], refs[f]["desc"], ur, last, Tc, I4, 15.0)
        if nm_ref < 20:                                      # Tracking.cc:954-958
            nm_ref, m_ref = oracle_mod.search_by_projection(cam_o, refs[f]["kps"], refs[f]["desc"], ur, last, Tc, I4, 30.0)
        assert nms[f] == nm_ref, (f, nms[f], nm_ref)
        assert np.array_equal(matches[f], m_ref), f
