"""The flow kernels (csrc/coeb_flow.hip: Frame::ProcessMovingObject stage by stage) off 640x480 and
off calcOpticalFlowPyrLK's one window and level count (MI355X only).  Every comparison is bit for
bit against the CPU oracle, as in test_gpu_flow.py; the shapes, images and directed points come
from tests/flow_shapes.py, and tests/test_oracle_kat.py asserts on the oracle alone that they
reach what they are meant to reach.

Sizes: 32x32 (the smallest the entries accept) to 427x321, chosen so that the LK level byte sizes
at win 22 cover every residue mod 4 (flow_shapes.SIZES): the last inside window of a level reads
a dword pair that reaches past the level's last pixel, under the buffer resource's limit."""
import ctypes as C

import numpy as np
import pytest

import coeb_front as cf
import flow_shapes as fs

pytestmark = pytest.mark.gpu

COEB_OK, COEB_EINVAL = 0, -22                          # include/coeb_front.h
SIZE_IDS = ["%dx%d" % s for s in fs.SIZES]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(a, b, tag):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, (tag, a.shape, b.shape)
    bad = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0] if len(a) else []
    assert len(bad) == 0, (tag, len(bad), bad[:6], a[bad[:3]], b[bad[:3]])


def in_parent(img, stride):
    """img as a view of a (rows, stride) parent of random bytes."""
    h, w = img.shape
    parent = np.random.default_rng(stride).integers(0, 256, (h, stride)).astype(np.uint8)
    parent[:, :w] = img
    return parent[:, :w]


# ---- the four stage entries through the C ABI, with the row pitch as an argument
def raw_gf(ctx, img, stride, max_corners=1000, quality=0.01, min_distance=8.0):
    h, w = img.shape
    out = np.zeros((max_corners, 2), np.float32)
    n = C.c_int(0)
    rc = cf.lib().coeb_good_features(ctx.h, img.ctypes.data, w, h, stride, max_corners, quality, min_distance, 0.04,
                                     out.ctypes.data, max_corners, C.byref(n))
    return rc, out[:n.value].copy()


def raw_subpix(ctx, img, stride, xy):
    h, w = img.shape
    xy = np.ascontiguousarray(xy, np.float32).copy()
    rc = cf.lib().coeb_corner_subpix(ctx.h, img.ctypes.data, w, h, stride, xy.ctypes.data, len(xy), 10, 20, 0.03)
    return rc, xy


def raw_lk(ctx, prev, cur, stride, xy, win=22, max_level=5, w=None, h=None):
    h = prev.shape[0] if h is None else h
    w = prev.shape[1] if w is None else w
    xy = np.ascontiguousarray(xy, np.float32)
    nx = np.zeros_like(xy)
    st = np.zeros(len(xy), np.uint8)
    rc = cf.lib().coeb_optical_flow_pyr_lk(ctx.h, prev.ctypes.data, cur.ctypes.data, w, h, stride, xy.ctypes.data,
                                           len(xy), win, max_level, 20, 0.01, nx.ctypes.data, st.ctypes.data)
    return rc, nx, st


def raw_tail(ctx, prev, cur, stride, pxy, nxy, state):
    h, w = prev.shape
    pxy, nxy = np.ascontiguousarray(pxy, np.float32), np.ascontiguousarray(nxy, np.float32)
    st = np.ascontiguousarray(state, np.uint8).copy()
    tm = np.zeros((max(len(pxy), 1), 2), np.float32)
    F = np.zeros(9, np.float64)
    nt, nf = C.c_int(0), C.c_int(0)
    rc = cf.lib().coeb_moving_tail(ctx.h, prev.ctypes.data, cur.ctypes.data, w, h, stride, pxy.ctypes.data,
                                   nxy.ctypes.data, st.ctypes.data, len(pxy), tm.ctypes.data, len(tm), C.byref(nt),
                                   F.ctypes.data, C.byref(nf))
    return rc, (None if nt.value < 0 else tm[:nt.value].copy()), st, (None if nt.value < 0 else F.reshape(3, 3)), nf.value


def same_tail(got, ref, tag):
    tm, st, F, nf = got
    rtm, rst, rF, rnf = ref
    same_bits(st, rst, tag + " state")
    assert nf == rnf, (tag, nf, rnf)
    assert (F is None) == (rF is None), tag
    if rF is not None:
        same_bits(F, rF, tag + " F")
        same_bits(tm, rtm, tag + " T_M")


# ---------------------------------------------------------------- 1. the LK grid
@pytest.mark.parametrize("win", fs.WINS)
@pytest.mark.parametrize("w,h", fs.SIZES, ids=SIZE_IDS)
def test_lk_grid(ctx, oracle_mod, w, h, win):
    """win x max_level at every size, on the oracle's corners and the directed points of every kept
    level (flow_shapes.lk_directed): status for all points, positions where the oracle tracks."""
    prev, cur = fs.pair(w, h)
    grid = [ml for wn, ml in fs.lk_grid(w, h) if wn == win]
    assert grid == list(fs.MAX_LEVELS)                  # max_level <= 7 never gives more than 8 levels
    for ml in grid:
        pts, nnat, names, levels, want = fs.lk_points(oracle_mod, prev, win, ml)
        rnx, rst = oracle_mod.lk_pyr(prev, cur, pts, win=win, max_level=ml)
        fs.assert_lk_coverage(w, h, win, ml, nnat, names, levels, want, rst)
        nx, st = cf.CalcOpticalFlowPyrLK(ctx, prev, cur, pts, win=win, max_level=ml)
        tag = "%dx%d win %d max_level %d" % (w, h, win, ml)
        same_bits(st, rst, tag + " status")
        same_bits(nx[rst == 1], rnx[rst == 1], tag + " next")


def test_lk_eight_levels(ctx, oracle_mod):
    """win 3 with max_level 8 at 640x480 keeps 8 levels (the ninth would be 3x2), the most the entry
    takes: down to a 5x4 level."""
    prev, cur = fs.pair(640, 480)
    assert fs.lk_level_sizes(640, 480, 3, 8)[-1] == (5, 4) and len(fs.lk_level_sizes(640, 480, 3, 8)) == 8
    pts, nnat, names, levels, want = fs.lk_points(oracle_mod, prev, 3, 8)
    pts = pts[max(0, nnat - 200):]
    rnx, rst = oracle_mod.lk_pyr(prev, cur, pts, win=3, max_level=8)
    assert rst.sum() >= 50
    nx, st = cf.CalcOpticalFlowPyrLK(ctx, prev, cur, pts, win=3, max_level=8)
    same_bits(st, rst, "status")
    same_bits(nx[rst == 1], rnx[rst == 1], "next")


# ---------------------------------------------------------------- 2. row pitch
@pytest.mark.parametrize("w,h", fs.SIZES, ids=SIZE_IDS)
def test_row_pitch(ctx, oracle_mod, w, h):
    """A host stride of w + 3 and w + 64 (random bytes between the rows) gives what the contiguous
    call gives, for all four stage entries."""
    prev, cur = fs.pair(w, h)
    pts, nnat, names, levels, want = fs.lk_points(oracle_mod, prev, 22, 5)
    rnx, rst = oracle_mod.lk_pyr(prev, cur, pts)
    rc, gf0 = raw_gf(ctx, prev, w)
    assert rc == COEB_OK and len(gf0) == nnat
    _, sp0 = raw_subpix(ctx, prev, w, gf0)
    _, nx0, st0 = raw_lk(ctx, prev, cur, w, pts)
    same_bits(st0, rst, "contiguous status")
    tail0 = raw_tail(ctx, prev, cur, w, pts, rnx, rst)
    assert tail0[0] == COEB_OK
    for stride in (w + 3, w + 64):
        pv, cv = in_parent(prev, stride), in_parent(cur, stride)
        assert pv.strides == (stride, 1)
        rc, gf = raw_gf(ctx, pv, stride)
        assert rc == COEB_OK
        same_bits(gf, gf0, "gf stride %d" % stride)
        rc, sp = raw_subpix(ctx, pv, stride, gf0)
        assert rc == COEB_OK
        same_bits(sp, sp0, "subpix stride %d" % stride)
        rc, nx, st = raw_lk(ctx, pv, cv, stride, pts)
        assert rc == COEB_OK
        same_bits(st, st0, "LK status stride %d" % stride)
        same_bits(nx[st0 == 1], nx0[st0 == 1], "LK next stride %d" % stride)
        got = raw_tail(ctx, pv, cv, stride, pts, rnx, rst)
        assert got[0] == COEB_OK
        same_tail(got[1:], tail0[1:], "tail stride %d" % stride)


# ---------------------------------------------------------------- 3. goodFeaturesToTrack
@pytest.mark.parametrize("w,h", fs.SIZES, ids=SIZE_IDS)
def test_good_features_grid(ctx, oracle_mod, w, h):
    prev, _ = fs.pair(w, h)
    for md in fs.GF_MIN_DISTANCE:
        for q in fs.GF_QUALITY:
            for mc in fs.GF_MAX_CORNERS:
                ref = oracle_mod.good_features(prev, mc, q, md)
                assert len(ref) >= 1
                got = cf.GoodFeaturesToTrack(ctx, prev, max_corners=mc, quality=q, min_distance=md)
                same_bits(got, ref, "%dx%d min_distance %g quality %g max_corners %d" % (w, h, md, q, mc))


def test_good_features_first_and_last_candidates(ctx, oracle_mod):
    """Corners on rows and columns 1 and n - 2, the first and last positions the 3x3 maximum
    test looks at."""
    img = fs.gf_border_image()
    ref = oracle_mod.good_features(img, min_distance=1.0)
    assert sorted(map(tuple, ref[:8].astype(int).tolist())) == sorted(fs.gf_border_points(img.shape[1], img.shape[0]))
    same_bits(cf.GoodFeaturesToTrack(ctx, img, min_distance=1.0), ref, "border")
    same_bits(cf.GoodFeaturesToTrack(ctx, img), oracle_mod.good_features(img), "border min_distance 8")


def test_good_features_ragged_widths(ctx, oracle_mod):
    imgs = fs.gf_ragged_images()
    assert [im.shape[1] % 4 for im in imgs] == [1, 2, 3]
    for im in imgs:
        for md in (1.0, 8.0):
            ref = oracle_mod.good_features(im, min_distance=md)
            assert len(ref) >= 5
            same_bits(cf.GoodFeaturesToTrack(ctx, im, min_distance=md), ref, "width %d" % im.shape[1])


# ---------------------------------------------------------------- 4. cornerSubPix and MovingTail edges
@pytest.mark.parametrize("w,h", fs.SIZES, ids=SIZE_IDS)
def test_corner_subpix_margin(ctx, oracle_mod, w, h):
    """Points at exactly 14.0 and 13.99 px from each edge and in each corner: k_subpix_order's
    interior / border / corner split, in one call so that every queue is used."""
    prev, _ = fs.pair(w, h)
    pts = fs.subpix_edge_points(w, h)
    pts = np.concatenate([pts, oracle_mod.good_features(prev)])
    same_bits(cf.CornerSubPix(ctx, prev, pts), oracle_mod.corner_subpix(prev, pts), "%dx%d" % (w, h))


def test_corner_subpix_leaves_image_and_resets(ctx, oracle_mod):
    img = fs.subpix_wander_image()
    out, reset = fs.subpix_wander_points(oracle_mod, img)
    assert len(out) >= 2 and len(reset) >= 8
    pts = np.concatenate([out, reset])
    same_bits(cf.CornerSubPix(ctx, img, pts), oracle_mod.corner_subpix(img, pts), "wander")


@pytest.mark.parametrize("w,h", [(91, 93), (427, 321)], ids=["91x93", "427x321"])
def test_moving_tail_limits(ctx, oracle_mod, w, h):
    """A 3x3 SAD of exactly 2120 is kept and 2121 dropped; truncated coordinates 4 and n - 5 are
    dropped and 5 and n - 6 kept, for the previous and the next point in x and in y.  The directed
    pairs run alone (fewer than 7 kept: no F) and after the scene's tracked corners."""
    prev, cur, sp, sn, sad = fs.sad_pair(w, h)
    assert [fs.sad_of(prev, cur, p, q) for p, q in zip(sp, sn)] == list(sad)
    ep, en, keep = fs.tail_edge_points(w, h)
    dp, dn = np.concatenate([sp, ep]), np.concatenate([sn, en])
    want = np.concatenate([sad <= fs.SAD_LIMIT, keep])
    corners = oracle_mod.corner_subpix(prev, oracle_mod.good_features(prev))
    cn, cst = oracle_mod.lk_pyr(prev, cur, corners)
    for tag, p, q, s in (("edges alone", ep, en, np.ones(len(ep), np.uint8)),
                         ("sad alone", sp, sn, np.ones(len(sp), np.uint8)),
                         ("with corners", np.concatenate([corners, dp]), np.concatenate([cn, dn]),
                          np.concatenate([cst, np.ones(len(dp), np.uint8)]))):
        ref = oracle_mod.moving_tail(prev, cur, p, q, s)
        if tag == "with corners":
            state = ref[1][len(corners):]
            assert np.array_equal(state[:len(sp)] == 1, want[:len(sp)])
            # the SAD check still applies to the edge pairs that pass the edge rule
            assert not state[len(sp):][~keep].any() and ref[2] is not None
        got = cf.MovingTail(ctx, prev, cur, p, q, s)
        same_tail(got, ref, "%dx%d %s" % (w, h, tag))


# ---------------------------------------------------------------- 5. rejections
def test_rejections_leave_the_context_usable(ctx, oracle_mod):
    """win 2 and 23, a width or height of 31, nine pyramid levels and a stride below the width are
    COEB_EINVAL, and the good call that follows each gives the oracle's result.  Nine levels need
    win 3 with max_level 8 on a frame of at least 1025 pixels a side (1280x960: level 8 is 5x4);
    640x480 keeps eight and is accepted (test_lk_eight_levels)."""
    w, h = 91, 93
    prev, cur = fs.pair(w, h)
    pts, nnat, names, levels, want = fs.lk_points(oracle_mod, prev, 22, 5)
    rnx, rst = oracle_mod.lk_pyr(prev, cur, pts)
    big = np.zeros((960, 1280), np.uint8)
    assert len(fs.lk_level_sizes(1280, 960, 3, 8)) == 9
    bad = [dict(win=2), dict(win=23), dict(w=31), dict(h=31), dict(stride=w - 1), dict(big=True, win=3, max_level=8)]
    for kw in bad:
        if kw.get("big"):
            rc, _, _ = raw_lk(ctx, big, big, 1280, pts[:4], win=3, max_level=8)
        else:
            rc, _, _ = raw_lk(ctx, prev, cur, kw.get("stride", w), pts, win=kw.get("win", 22), w=kw.get("w"), h=kw.get("h"))
        assert rc == COEB_EINVAL, (kw, rc)
        rc, nx, st = raw_lk(ctx, prev, cur, w, pts)
        assert rc == COEB_OK, kw
        same_bits(st, rst, "status after %s" % kw)
        same_bits(nx[rst == 1], rnx[rst == 1], "next after %s" % kw)
    small = np.zeros((31, 64), np.uint8)
    gf_ref = oracle_mod.good_features(prev)
    for call in (lambda: raw_gf(ctx, small, 64)[0], lambda: raw_gf(ctx, small.T.copy(), 31)[0],
                 lambda: raw_gf(ctx, prev, w - 1)[0], lambda: raw_subpix(ctx, prev, w - 1, gf_ref)[0],
                 lambda: raw_subpix(ctx, small, 64, gf_ref[:2])[0],
                 lambda: raw_tail(ctx, prev, cur, w - 1, pts, rnx, rst)[0],
                 lambda: raw_tail(ctx, small, small, 64, pts[:2], rnx[:2], rst[:2])[0]):
        assert call() == COEB_EINVAL
        rc, gf = raw_gf(ctx, prev, w)
        assert rc == COEB_OK
        same_bits(gf, gf_ref, "good features after a rejection")
