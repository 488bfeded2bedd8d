"""SearchForTriangulation on the device (k_tri_match, k_tri_rot) over the directed inputs of
tests/tri_cases.py (MI355X only): every entry of match_out and nmatches has to equal the model
(tests/tri_ref.py), under the case's own flags and under the other three combinations of
only_stereo x check_orientation."""
import numpy as np
import pytest

import tri_cases as C

pytestmark = pytest.mark.gpu


def load(db, kfs):
    """The keyframes into an empty database, with their geometry -> their slots."""
    from coeb_front import KEYPOINT_DTYPE
    slots = []
    for kf in kfs:
        n = len(kf["node"])
        s = db.add(kf["desc"], kf["node"], kf["angle"], np.zeros(0, np.int32), np.zeros(0))
        keys = np.zeros(n, KEYPOINT_DTYPE)
        keys["x"], keys["y"], keys["octave"], keys["angle"] = kf["x"], kf["y"], kf["octave"], kf["angle"]
        db.set_geometry(s, keys, kf["u_right"])
        slots.append(s)
    return slots


@pytest.mark.parametrize("name", C.names())
def test_directed_case(ctx, name):
    from coeb_front import KeyFrameDatabase
    t = ctx.tables()
    assert np.array_equal(np.array(t.scale[:C.NLEVELS], np.float32), C.SCALE)
    assert np.array_equal(np.array(t.sigma2[:C.NLEVELS], np.float32), C.SIGMA2)
    c = C.case(name)
    db = KeyFrameDatabase(ctx, max_features=200, initial_slots=2)
    try:
        slots = load(db, c["kfs"])
        assert slots == list(range(len(c["kfs"])))
        k1 = c["kfs"][c["slot1"]]
        for only_stereo, check_ori in ((c["only_stereo"], c["check_ori"]), (not c["only_stereo"], c["check_ori"]),
                                       (c["only_stereo"], not c["check_ori"]), (not c["only_stereo"], not c["check_ori"])):
            want, want_nm = C.reference(c, only_stereo=only_stereo, check_ori=check_ori)
            got, nm = db.search_for_triangulation(c["slot1"], k1["has_mp"], c["slots2"],
                                                  [c["kfs"][s]["has_mp"] for s in c["slots2"]], c["F12"], c["epipole"],
                                                  only_stereo, check_ori)
            assert got.shape == want.shape and got.dtype == np.int32
            assert nm.tolist() == want_nm.tolist(), (only_stereo, check_ori)
            assert np.array_equal(got, want), (only_stereo, check_ori)
    finally:
        db.close()
