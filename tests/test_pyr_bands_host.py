"""k_pyr_rows' band descriptors without a GPU: the PyrBand table make_plan appends to the resize
tables (csrc/coeb_plan.cpp, coeb_plan.hpp), printed by tests/host/pyr_bands_host_main.cpp (built
as a stand-alone program under ASan + UBSan, like tests/test_plan_host.py) and recomputed here in
numpy from the resize definition of the oracle (oc_resize_tables: fy = (float)((dy + 0.5) *
scale_y - 0.5), sy = floor(fy), beta = round((1 - fy) * 2048), round(fy * 2048)).

A band is 8 output rows; its pattern is the sequence sy(oy + r) - sy(oy), r = 0..7.  A band is
generic when a source row is clamped, when it is the level's last, partial band, or when its
sequence is not one of the instantiated patterns; every other band names its pattern.

What the plans of the bench shapes give (asserted below):
  * 640x480 and 1280x960 each use all five instantiated patterns; the other sequences are 1-2 %
    of their bands (the drift of ratios such as 640/533 across a phase) and stay generic;
  * at 640x480 the levels 2..7 each have a generic band (the partial last band: 333, 278, 231,
    193, 161, 134 rows).  Level 1 has none: 480 -> 400 rows is the exact ratio 1.2 with 50 whole
    bands, ten of each pattern, and its last source row 479 is reached without a clamp.  No wave
    of that level runs the per-row body on the GPU (its last strip's waves run the patterns'
    kLast bodies); tests/test_gpu_pyr_bands.py adds shapes whose level 1 has a partial band.

rows_ok (the row form's window test: every column pair's sources within 6 bytes of its aligned
window) is 1 for scale factors up to 2, so 1.2-scale shapes cannot make it 0; 640x480 with 2 levels
at 2.1 does, and every band of that level is generic (row steps of 2 and 3).
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SAN = ["-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
GENERIC = -1
BAND = 8
# (W, H, levels): the bench shapes and the small shapes of tests/test_gpu_pyr_bands.py
SHAPES = [(640, 480, 8), (1280, 960, 8), (333, 251, 8), (172, 130, 5)]


@pytest.fixture(scope="module")
def bands_exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("pyr_bands") / "pyr_bands_host")
    cmd = ["g++", "-std=c++17"] + SAN + ["-I", os.path.join(ROOT, "coeb-slam_amd", "csrc"),
                                         os.path.join(ROOT, "tests", "host", "pyr_bands_host_main.cpp"),
                                         os.path.join(ROOT, "coeb-slam_amd", "csrc", "coeb_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def plan_bands(exe, w, h, nlev, scale=None):
    """(pattern masks, levels): a level is a dict of its geometry and its (nbands, 12) descriptors."""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, str(w), str(h), str(nlev)] + ([repr(scale)] if scale else []), capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    masks, levels = None, []
    for ln in r.stdout.splitlines():
        t = ln.split()
        if t[0] == "patterns":
            masks = [int(v) for v in t[2:]]
            assert len(masks) == int(t[1])
        elif t[0] == "level":
            keys = ("l", "sw", "sh", "sp", "dw", "dh", "pitch", "rows_ok", "nbands")
            levels.append(dict(zip(keys, map(int, t[1:])), bands=[]))
        else:
            assert t[0] == "band" and len(t) == 13
            levels[-1]["bands"].append([int(v) for v in t[1:]])
    for lv in levels:
        lv["bands"] = np.array(lv["bands"], np.int64).reshape(-1, 12)
        assert len(lv["bands"]) == lv["nbands"] == (lv["dh"] + BAND - 1) // BAND
    return masks, levels


def test_scale_above_two_clears_rows_ok_and_every_band_is_generic(bands_exe):
    """640x480, 2 levels: at 2.1 a column pair's window is wider than 6 bytes (rows_ok 0: the
    launch takes the byte form) and the row steps are 2 or 3; at 2.0 rows_ok is still 1 and every
    step is 2.  Neither sequence is a pattern: all bands generic, descriptors as numpy gives them."""
    for scale, rows_ok, steps in ((2.1, 0, {2, 3}), (2.0, 1, {2})):
        masks, levels = plan_bands(bands_exe, 640, 480, 2, scale)
        assert len(levels) == 1
        lv = levels[0]
        assert lv["rows_ok"] == rows_ok, (scale, lv["rows_ok"])
        assert set(check_level(masks, lv)) == {GENERIC}, scale
        sy, _ = resize_rows(lv["sh"], lv["dh"])
        assert set(np.diff(sy).tolist()) == steps, scale


def resize_rows(sh, dh):
    """yofs (unclamped) and the packed beta of cv::resize INTER_LINEAR 8U, dh rows from sh."""
    scale_y = 1.0 / (float(dh) / sh)
    fy = ((np.arange(dh) + 0.5) * scale_y - 0.5).astype(np.float32)
    sy = np.floor(fy).astype(np.int64)
    fy = fy - sy.astype(np.float32)
    b0 = np.rint((np.float32(1) - fy) * np.float32(2048)).astype(np.int64)
    b1 = np.rint(fy * np.float32(2048)).astype(np.int64)
    return sy, (b0 & 0xFFFF) | (b1 << 16)


def mask_sequence(mask):
    """sy(oy + r) - sy(oy), r = 0..7, of a pattern mask (bit i: a step of 2 after row i)."""
    steps = [1 + ((mask >> i) & 1) for i in range(BAND - 1)]
    return [0] + list(np.cumsum(steps))


def resize_simd_end(w):
    x = (w // 16) * 16 if w >= 16 else 0
    while x < w - 4:
        x += 4
    return x


def check_level(masks, lv):
    """Every descriptor of a level against numpy; returns the list of its pattern ids."""
    sh, dh, sp = lv["sh"], lv["dh"], lv["sp"]
    sy, beta = resize_rows(sh, dh)
    seqs = [mask_sequence(m) for m in masks]
    ids = []
    for b, d in enumerate(lv["bands"]):
        oy = b * BAND
        tag = (lv["l"], b)
        partial = oy + BAND > dh
        rows = sy[oy:min(oy + BAND, dh)]
        clamped = bool((rows < 0).any() or (rows + 1 > sh - 1).any())
        seq = list(rows - rows[0])
        want = GENERIC
        if not partial and not clamped and seq in seqs:
            want = seqs.index(seq)
        assert d[0] == want, (tag, d[0], want, seq)
        if d[0] != GENERIC:
            # pattern id <-> sequence, and the 9 + popcount(mask) source rows are inside the level
            assert mask_sequence(masks[d[0]]) == seq, tag
            assert rows[0] >= 0 and rows[0] + 9 + bin(masks[d[0]]).count("1") <= sh, tag
            assert rows[-1] + 1 == rows[0] + 8 + bin(masks[d[0]]).count("1"), tag
        assert d[1] == min(max(int(sy[oy]), 0), sh - 1) * sp, tag
        assert d[2] == oy * lv["pitch"] and d[3] == 0, tag
        nb = min(BAND, dh - oy)
        assert list(d[4:4 + nb]) == list(beta[oy:oy + nb]) and not d[4 + nb:].any(), tag
        ids.append(int(d[0]))
    return ids


@pytest.mark.parametrize("w,h,nlev", SHAPES)
def test_band_descriptors_match_numpy(bands_exe, w, h, nlev):
    masks, levels = plan_bands(bands_exe, w, h, nlev)
    assert len(levels) == nlev - 1 and len(set(masks)) == len(masks)
    for lv in levels:
        ids = check_level(masks, lv)
        if lv["dh"] % BAND:
            assert ids[-1] == GENERIC, lv["l"]


@pytest.mark.parametrize("w,h", [(640, 480), (1280, 960)])
def test_bench_plans_use_every_pattern(bands_exe, w, h):
    """The instantiated list is taken from these two plans: each pattern is used by both, and the
    sequences left generic are a small share of the whole bands."""
    masks, levels = plan_bands(bands_exe, w, h, 8)
    ids = np.concatenate([lv["bands"][:, 0] for lv in levels])
    for p in range(len(masks)):
        assert (ids == p).sum() >= 1, (p, masks[p])
    whole = sum(lv["dh"] // BAND for lv in levels)
    assert (ids != GENERIC).sum() >= 0.95 * whole, ((ids != GENERIC).sum(), whole)


def test_640x480_generic_bands_per_level(bands_exe):
    """Both bodies run in every launch that can have both: levels 2..7 each have a generic band
    beside pattern bands.  Level 1 (400 rows from 480: exactly 1.2, 50 whole bands, no clamp) has
    no generic band by the definition; it is pinned here so that a change of the classification
    shows."""
    masks, levels = plan_bands(bands_exe, 640, 480, 8)
    for lv in levels:
        ids = lv["bands"][:, 0]
        assert (ids != GENERIC).any(), lv["l"]
        if lv["l"] == 1:
            assert lv["dh"] == 400 and (ids != GENERIC).all()
            assert sorted(np.bincount(ids, minlength=len(masks)).tolist()) == [10] * 5
        else:
            assert (ids == GENERIC).sum() >= 1, lv["l"]


def test_small_shapes_reach_the_cases_of_the_gpu_test(bands_exe):
    """What tests/test_gpu_pyr_bands.py says its small shapes provide."""
    _, a = plan_bands(bands_exe, 333, 251, 8)
    _, b = plan_bands(bands_exe, 172, 130, 5)
    # rows_ok is 1 for scale factors up to 2 (1.2-scale shapes cannot make it 0; the 2.1 case
    # above does), so here the byte form is reached through the other condition of the launch:
    # a source pitch that is no multiple of 4.  333x251's level 1 reads the 333-byte-pitch frame.
    assert all(lv["rows_ok"] == 1 for lv in a + b)
    assert a[0]["sp"] == 333 and a[0]["sp"] % 4 != 0 and all(lv["sp"] % 4 == 0 for lv in a[1:])
    # 172x130: every level in the row form, level 1 from a pitch (172) that is no multiple of 64
    assert all(lv["sp"] % 4 == 0 for lv in b) and b[0]["sp"] == 172
    for lv in a[1:] + b:
        # a last strip with tail columns and the edge column (112 = 7 * 16 columns: the edge
        # column without a tail); a partial (generic) last band
        xs = resize_simd_end(lv["dw"])
        assert (xs < lv["dw"] and (lv["dw"] - 1) // 128 == xs // 128) or (lv["dw"] == 112 and xs == 112), lv
        assert lv["dh"] % BAND != 0 and lv["bands"][-1, 0] == GENERIC and (lv["bands"][:, 0] != GENERIC).any(), lv
    # levels narrower than one 128-column strip (every wave holds the edge: pattern bands run
    # the kLast bodies, generic bands pyr_rows_out<*, true>)
    assert [lv["dw"] for lv in a[-2:]] == [112, 93] and [lv["dw"] for lv in b[1:]] == [119, 100, 83]
    # levels of two and three strips, whose first strips run the pattern bodies
    assert [lv["dw"] for lv in a[1:5]] == [231, 193, 161, 134] and b[0]["dw"] == 143
    # a generic band that is not the partial one (a sequence outside the list) inside a level
    assert any((lv["bands"][:-1, 0] == GENERIC).any() for lv in a[1:] + b)
