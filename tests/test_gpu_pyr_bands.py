"""k_pyr_rows' pattern bands against the CPU oracle and against k_pyr_level's byte form, every
pixel of every pyramid level of every frame of a batch (MI355X only).

A k_pyr_rows wave owns 8 output rows x 128 columns.  Where its band has one of the instantiated
row patterns (PyrBand, csrc/coeb_plan.hpp) it runs that pattern's body: pyr_rows_pattern<P, false>,
straight-line, where it holds neither tail columns (>= resize_simd_end) nor the level's last
column, and pyr_rows_pattern<P, true> (exact rounding of the tail, guarded stores) in a level's
last strip.  Waves of generic bands run the per-row body pyr_rows_out.  Which level provides which
case (tests/test_pyr_bands_host.py asserts the same on the CPU):

  640 x 480, F = 2    the bench plan: all five patterns in every level; level 1 (400 rows) has
                      only pattern bands, the levels 2..7 a partial last band and (2, 3, 4, 5, 6, 7)
                      a band whose sequence is outside the list
  333 x 251, F = 3    level 1 reads the frame at a 333-byte pitch (no multiple of 4): the byte
                      form runs beside the row form of the levels 2..7 (the pitch is the launch's
                      other condition; rows_ok is 1 for scale factors up to 2, see the last case);
                      heights 209, 174, 145, 121, 101, 84, 70: none a multiple of 8;
                      widths 231, 193, 161, 134: a pattern strip and a last strip with tail and
                      edge columns; 112: one strip, the edge column without a tail; 93: one strip
                      with tail and edge
  172 x 130, F = 3    5 levels, all in the row form; level 1 from a 172-byte source pitch: 143
                      columns = a pattern strip + a 15-column last strip with tail (140..142) and
                      edge; 108 rows = 13 whole bands + 4 rows; the levels 119, 100 and 83 wide
                      are narrower than one strip
  640 x 480, F = 2,   rows_ok is 0 for level 1 (305 x 229; a column pair's window is wider than
  2 levels at 2.1     6 bytes): the launch's rows_ok gate sends it to the byte form although the
                      pitches are aligned; its band table (row steps of 2 and 3) is all generic
"""
import numpy as np
import pytest

from coeb_front import Context

pytestmark = pytest.mark.gpu

CASES = [(640, 480, 8, 1.2, 2), (333, 251, 8, 1.2, 3), (172, 130, 5, 1.2, 3), (640, 480, 2, 2.1, 2)]


def frames_of(w, h, F, seed):
    """Noise over a gradient: every pixel differs from its neighbours, so a wrong source row or
    column, or a wrong beta, changes the output; the frames differ from each other."""
    rng = np.random.default_rng(seed)
    ramp = (np.arange(w)[None, :] * 3 + np.arange(h)[:, None] * 5) % 97
    return np.stack([(rng.integers(0, 160, (h, w)) + ramp).astype(np.uint8) for _ in range(F)])


def read_pyramids(c, frames):
    F, h, w = frames.shape
    dg = c.upload(frames)
    try:
        c.extract_batch_device(dg.ptr, F, w, h)
        c.synchronize()
        return [c.debug_read("pyr", f) for f in range(F)]
    finally:
        dg.free()


@pytest.mark.parametrize("w,h,nlev,scale,F", CASES)
def test_pyramid_rows_form_matches_oracle_and_byte_form(oracle_mod, monkeypatch, w, h, nlev, scale, F):
    ex = oracle_mod.Extractor(1000, scale, nlev, 20, 7)
    frames = frames_of(w, h, F, seed=w + h)
    c = Context(1000, scale, nlev, 20, 7, max_width=w, max_height=h, max_batch=F)
    try:
        monkeypatch.delenv("COEB_PYR_BYTES", raising=False)
        rows = read_pyramids(c, frames)
        monkeypatch.setenv("COEB_PYR_BYTES", "1")
        byts = read_pyramids(c, frames)
    finally:
        c.close()
    sizes = ex.level_sizes(w, h)
    for f in range(F):
        r = ex.extract(frames[f], debug=True)
        poff = 0
        for l, (lw, lh) in enumerate(sizes):
            if l == 0:
                continue
            ref = r["pyramid"][r["level_off"][l]:r["level_off"][l] + lw * lh].reshape(lh, lw)
            pp = (lw + 63) // 64 * 64
            got = rows[f][poff:poff + pp * lh].reshape(lh, pp)[:, :lw]
            gotb = byts[f][poff:poff + pp * lh].reshape(lh, pp)[:, :lw]
            bad = np.argwhere(got != ref)
            assert len(bad) == 0, ("rows form vs oracle", f, l, (lw, lh), len(bad), bad[:4].tolist())
            bad = np.argwhere(got != gotb)
            assert len(bad) == 0, ("rows form vs byte form", f, l, (lw, lh), len(bad), bad[:4].tolist())
            poff = (poff + pp * lh + 255) // 256 * 256
