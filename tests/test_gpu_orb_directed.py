"""k_fast, k_describe, the blur and the level-0 scaling on the directed small frames of
tests/orb_ref.py, against the oracle bit for bit and against the independent numpy model (MI355X
only).

tests/test_orb_ref.py (no GPU) asserts that every frame reaches the regime it is named after and
that the oracle agrees with the model; here `ctx.extract` of each frame must equal the oracle in
every keypoint field and descriptor byte (assert_same), agree with the model under the rules of
test_orb_ref.compare_records (every field but the angle exact, the angle within orb_ref.ANGLE_BOUND
of float64 atan2, every decided descriptor bit), and `cand_n` must equal the model's candidate
count of every cell, so that a failure names the stage and the cell.  Frames whose plan takes the
96-byte slab rows run a second time under COEB_FAST_RB=72."""
import ctypes as C

import numpy as np
import pytest

import orb_ref as R
from test_gpu_parity import assert_same
from test_orb_ref import compare_records

pytestmark = pytest.mark.gpu

FRAMES = dict(R.frames(), **{f.name: f for f in R.random_frames()})


def extract_strided(c, img, stride):
    """coeb_extract on a copy of img whose rows are `stride` bytes apart"""
    import coeb_front as cf
    h, w = img.shape
    buf = np.full(h * stride + 64, 0xA5, np.uint8)
    off = (-buf.ctypes.data) % 64 + 1                   # an odd first-row address as well
    view = np.ndarray((h, w), np.uint8, buf, off, (stride, 1))
    view[:] = img
    cap = c.max_keypoints(w, h)
    kps = np.zeros(cap, cf.KEYPOINT_DTYPE)
    desc = np.zeros((cap, 32), np.uint8)
    n = C.c_int()
    c.check(cf.lib().coeb_extract(c.h, view.ctypes.data, w, h, stride, None, 0, None, 0, None, 0, kps.ctypes.data,
                                  desc.ctypes.data, cap, C.byref(n)))
    return kps[:n.value], (desc[:n.value] if n.value else None)


def check_frame(c, fr, ref, tag, stride=None):
    k, d = c.extract(fr.img) if stride is None else extract_strided(c, fr.img, stride)
    cn = c.debug_read("cand_n").view(np.int32).tolist()
    m = fr.model(angles=k["angle"])
    want = [len(cell["xs"]) for cells in m["cells"] for cell in cells]
    assert cn == want, (tag, "candidates per cell", cn, want)
    assert_same(k, d, ref["kps"], ref["desc"], tag)
    compare_records(k, d if d is not None else np.zeros((0, 32), np.uint8), m, R.ANGLE_BOUND, tag)


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_directed_frame(oracle_mod, monkeypatch, name):
    from coeb_front import Context
    fr = FRAMES[name]
    ref = oracle_mod.Extractor(fr.nfeatures, 1.2, fr.nlevels, 20, 7).extract(fr.img)
    kv = R.kernel_view(fr.w, fr.h, R.Tables(fr.nfeatures, 1.2, fr.nlevels))
    c = Context(fr.nfeatures, 1.2, fr.nlevels, 20, 7, max_width=fr.w, max_height=fr.h)
    try:
        check_frame(c, fr, ref, name)
        if kv["row_bytes"] == 96:
            monkeypatch.setenv("COEB_FAST_RB", "72")
            check_frame(c, fr, ref, name + " rb72")
    finally:
        c.close()


def test_odd_input_stride(oracle_mod):
    """Host rows w + 3 bytes apart from an odd first address, the padding filled with 0xA5: the
    single-frame staging packs them, so the result is the packed frame's.  (On the device level 0
    has pitch w: frames whose width is no multiple of 16 -- 74, 97, 109, 141, 157 -- take
    k_describe's and k_fast's byte and word paths there, 64, 128 and 160 the vector paths.)"""
    from coeb_front import Context
    fr = FRAMES["noise_160x120_L3"]
    ref = oracle_mod.Extractor(fr.nfeatures, 1.2, fr.nlevels, 20, 7).extract(fr.img)
    c = Context(fr.nfeatures, 1.2, fr.nlevels, 20, 7, max_width=fr.w, max_height=fr.h)
    try:
        check_frame(c, fr, ref, "stride %d" % (fr.w + 3), stride=fr.w + 3)
    finally:
        c.close()
