"""k_fast's pixel pre-test is a filter only: what it admits and the exact arc score rejects must
leave no trace, whatever the number of admitted pixels (MI355X only).

The pre-test keeps a pixel iff, in the dark or in the bright sense, both compass pairs of its ring
(0/8 and 4/12) hold a pixel beyond v -/+ minTh (FILTER_PAIRS = 2, the entry list
holds ENT_CAP = 192 entries and is drained in mid-cell when more than ENT_CAP - 64 are pending).
`survivors` restates that here; every frame asserts on the CPU, before the GPU runs, that it has
the survivor counts and the rejected pixels it is built for, so that a change of the filter depth
cannot silently empty the cases.  Candidates per cell are compared with the numpy model
(tests/orb_ref.py), keypoints and descriptors with the oracle, bit for bit, in both slab layouts.
"""
import numpy as np
import pytest

import orb_ref as R
from test_gpu_orb_directed import check_frame
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

FILTER_PAIRS = 2
PAIR_ORDER = (0, 4, 2, 6, 1, 5, 3, 7)
ENT_CAP = 192
BG = 100


def survivors(img, t, depth=FILTER_PAIRS):
    """bool (h, w): pixels the depth-pair pre-test admits at t (False on the 3-px border)"""
    a = img.astype(np.int32)
    h, w = a.shape
    v = a[3:h - 3, 3:w - 3]
    ring = [a[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in R.RING]
    dark = np.ones_like(v, bool)
    bright = np.ones_like(v, bool)
    for k in PAIR_ORDER[:depth]:
        dark &= np.minimum(ring[k], ring[k + 8]) < v - t
        bright &= np.maximum(ring[k], ring[k + 8]) > v + t
    out = np.zeros((h, w), bool)
    out[3:h - 3, 3:w - 3] = dark | bright
    return out


def windows(w, h):
    """{(i, j): (x0, y0, x1, y1)}: the detection window (ROI minus its 3-px inset) of each cell"""
    return {(i, j): (x0 + 3, y0 + 3, x1 - 3, y1 - 3) for i, j, x0, y0, x1, y1 in R.level_cells(w, h)}


def count_in(S, win):
    x0, y0, x1, y1 = win
    return int(S[y0:y1, x0:x1].sum())


def alternating(img, cx, cy):
    """ring pixels alternately 40 above and 40 below the centre: every opposite pair of an even
    index is bright, so any pair pre-test admits the centre, and no two ring neighbours agree"""
    for k, (dx, dy) in enumerate(R.RING):
        img[cy + dy, cx + dx] = BG + 40 if k % 2 == 0 else BG - 40


def fill_cell(img, win, target, others):
    """Adds, in raster order, units of two bright pixels at (x, y + 3) and (x + 3, y) -- (x, y) then
    passes both compass pairs and has no arc -- and lone bright pixels, to window `win` until it has
    exactly `target` survivors at minTh 7, leaving the counts of the windows `others` as they are."""
    x0, y0, x1, y1 = win
    before = [count_in(survivors(img, 7), o) for o in others]
    for pixels in (((0, 3), (3, 0)), ((0, 0),)):
        for y in range(y0 + 1, y1 - 4, 3 if len(pixels) > 1 else 2):
            for x in range(x0 + 1, x1 - 4, 4 if len(pixels) > 1 else 2):
                if count_in(survivors(img, 7), win) == target:
                    return
                old = [img[y + dy, x + dx] for dx, dy in pixels]
                if any(v != BG for v in old):
                    continue
                for dx, dy in pixels:
                    img[y + dy, x + dx] = BG + 60
                S = survivors(img, 7)
                if count_in(S, win) > target or [count_in(S, o) for o in others] != before:
                    for (dx, dy), v in zip(pixels, old):
                        img[y + dy, x + dx] = v
    assert count_in(survivors(img, 7), win) == target, (win, target)


COUNTS = {(0, 0): 63, (0, 1): 64, (0, 2): 65, (1, 0): 128, (1, 1): 129}


def counts_frame():
    """160 x 120, one level, 4 x 2 cells: five cells with exactly 63, 64, 65, 128 and 129 pre-test
    survivors, cell (0, 3) with the alternating rings (interior, first / last window row and column,
    one with a true corner beside it) and cell (1, 3) of noise, more entries than the list holds."""
    img = np.full((120, 160), BG, np.uint8)
    W = windows(160, 120)
    x0, y0, x1, y1 = W[(0, 3)]
    alt = [(x0, y0), (x1 - 1, y0 + 12), (x0 + 12, y1 - 1), (x0 + 14, y0 + 14), (x0 + 24, y0 + 28)]
    for cx, cy in alt:
        alternating(img, cx, cy)
    corner = (alt[-1][0] + 1, alt[-1][1])
    img[corner[1], corner[0]] = 250
    nx0, ny0, nx1, ny1 = W[(1, 3)]
    img[ny0:ny1, nx0:nx1] = np.random.default_rng(5).integers(0, 256, (ny1 - ny0, nx1 - nx0), dtype=np.uint8)
    for cell, n in COUNTS.items():
        fill_cell(img, W[cell], n, [W[c] for c in W if c != cell])
    return R.Frame("filter_counts", "filter", img, 1, alt=alt, corner=corner)


def wide_frame():
    """97 x 74, one level: cell (0, 0) is 33 columns wide (16 lanes per row, 4 rows per pass) and holds
    noise up to its last four columns and an alternating ring on its last column; cell (0, 1) holds
    alternating rings on its window edges"""
    img = np.full((74, 97), BG, np.uint8)
    W = windows(97, 74)
    assert sorted(W) == [(0, 0), (0, 1)] and W[(0, 0)][2] - W[(0, 0)][0] == 33, W
    x0, y0, x1, y1 = W[(0, 0)]
    img[y0:y1, x0:x1 - 4] = np.random.default_rng(6).integers(0, 256, (y1 - y0, x1 - 4 - x0), dtype=np.uint8)
    alt = [(x1 - 1, y0 + 20)]
    x0, y0, x1, y1 = W[(0, 1)]
    alt += [(x1 - 1, y0), (x0 + 8, y1 - 1), (x0 + 16, y0 + 16)]
    for cx, cy in alt:
        alternating(img, cx, cy)
    img[y0 + 8, x0 + 24] = 250
    return R.Frame("filter_wide", "filter", img, 1, alt=alt)


def entries_before_last_pass(S, win, rows_per_pass):
    """pre-test entries (groups of 4 window columns of a row with a survivor) before the last pass"""
    x0, y0, x1, y1 = win
    M = S[y0:y1, x0:x1]
    M = M[:(M.shape[0] - 1) // rows_per_pass * rows_per_pass]
    G = np.pad(M, ((0, 0), (0, (-M.shape[1]) % 4))).reshape(M.shape[0], -1, 4).any(axis=2)
    return int(G.sum())


def check_preconditions(fr, t=7):
    S, M = survivors(fr.img, t), R.fast_strength(fr.img)
    assert not (~S & (M > t)).any(), "the pre-test is a necessary condition of a corner"
    for cx, cy in fr.info["alt"]:
        assert S[cy, cx] and survivors(fr.img, t, 4)[cy, cx] and M[cy, cx] <= t, (cx, cy, int(M[cy, cx]))
    return S, M


@pytest.fixture(scope="module")
def frames():
    return dict(counts=counts_frame(), wide=wide_frame())


def run(oracle_mod, monkeypatch, fr):
    from coeb_front import Context
    ref = oracle_mod.Extractor(fr.nfeatures, 1.2, fr.nlevels, 20, 7).extract(fr.img)
    c = Context(fr.nfeatures, 1.2, fr.nlevels, 20, 7, max_width=fr.w, max_height=fr.h)
    try:
        check_frame(c, fr, ref, fr.name)
        assert R.kernel_view(fr.w, fr.h, R.Tables(fr.nfeatures, 1.2, fr.nlevels))["row_bytes"] == 96
        monkeypatch.setenv("COEB_FAST_RB", "72")
        check_frame(c, fr, ref, fr.name + " rb72")
    finally:
        c.close()
    return ref


def test_survivor_counts_across_the_list_boundaries(oracle_mod, monkeypatch, frames):
    fr = frames["counts"]
    S, M = check_preconditions(fr)
    W = windows(fr.w, fr.h)
    for cell, n in COUNTS.items():
        assert count_in(S, W[cell]) == n, cell
        assert entries_before_last_pass(S, W[cell], 8) <= ENT_CAP - 64, cell        # drained once, at the end
    assert entries_before_last_pass(S, W[(1, 3)], 8) > ENT_CAP - 64                 # drained in mid-cell
    assert count_in(S, W[(1, 3)]) > 4 * 64
    # the units' centres and the alternating rings are admitted and rejected; the corner beside one stays
    rejected = S & (M <= 7)
    assert all(count_in(rejected, W[cell]) >= n // 3 - 1 for cell, n in COUNTS.items())
    cx, cy = fr.info["corner"]
    assert M[cy, cx] > 20
    ref = run(oracle_mod, monkeypatch, fr)
    keys = {(int(k["x"]), int(k["y"])) for k in ref["kps"]}
    assert not keys & set(fr.info["alt"])
    m = fr.model()
    cell = [c for c in m["cells"][0] if (c["i"], c["j"]) == (0, 3)][0]
    assert (cx - 16, cy - 16) in set(zip(cell["xs"].tolist(), cell["ys"].tolist())), "the true corner keeps its NMS result"


def test_wide_cells_sixteen_lanes_per_row(oracle_mod, monkeypatch, frames):
    fr = frames["wide"]
    S, _ = check_preconditions(fr)
    kv = R.kernel_view(fr.w, fr.h, R.Tables(fr.nfeatures, 1.2, 1))
    assert kv["levels"][0]["cells"][0]["rows_per_pass"] == 4
    assert entries_before_last_pass(S, windows(fr.w, fr.h)[(0, 0)], 4) > ENT_CAP - 64
    run(oracle_mod, monkeypatch, fr)


# one marked box over the left 40 columns: (1040 x 220) px > 200 000, so area_flag and 30 / 10
AREA_BOX = np.array([[-1000.0, -100.0, 40.0, 120.0]], np.float32)
AREA_TM = np.array([[5.0 + (k % 6) * 5, 5.0 + (k // 6) * 20] for k in range(30)], np.float32)


@pytest.mark.parametrize("rb", ["default", "72"])
def test_dynamic_area_thresholds(oracle_mod, monkeypatch, frames, rb):
    from coeb_front import Context
    fr = frames["counts"]
    S, M = check_preconditions(fr, 10)
    W = windows(fr.w, fr.h)
    assert count_in(S, W[(1, 3)]) > 4 * 64 and entries_before_last_pass(S, W[(1, 3)], 8) > ENT_CAP - 64
    assert (S & (M <= 10)).sum() >= 100
    ref = oracle_mod.Extractor(fr.nfeatures, 1.2, 1, 20, 7).extract(fr.img, boxes=AREA_BOX, tm=AREA_TM, debug=True)
    assert ref["area_flag"] == 1
    want = [len(c["xs"]) for c in R.level_candidates(fr.img, 30, 10)]
    if rb == "72":
        monkeypatch.setenv("COEB_FAST_RB", "72")
    c = Context(fr.nfeatures, 1.2, 1, 20, 7, max_width=fr.w, max_height=fr.h)
    try:
        k, d = c.extract(fr.img, boxes=AREA_BOX, tm=AREA_TM)
        assert c.debug_read("cand_n").view(np.int32).tolist() == want
        assert len(k) > 0
        assert_same(k, d, ref["kps"], ref["desc"], "area rb " + rb)
    finally:
        c.close()
