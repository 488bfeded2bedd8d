"""coeb_kfdb_create_new_map_points on the device (k_tri_match, k_tri_points) over the directed inputs of
tests/newpts_cases.py (MI355X only): every match_out, status, source and first_ok entry and the bits of every
accepted x3d equal the restatement (tests/newpts_ref.py) for only_stereo 0 and 1, match_out equals
coeb_kfdb_search_triangulation's, and x3d stays untouched where a pair was not accepted."""
import numpy as np
import pytest

import newpts_cases as C
import newpts_ref as N
from test_gpu_tri_directed import load as load_geometry

pytestmark = pytest.mark.gpu


def load(db, kfs):
    """The keyframes into an empty database with geometry and stereo data -> their slots."""
    slots = load_geometry(db, [dict(kf, angle=np.zeros(len(kf["node"]), np.float32)) for kf in kfs])
    for s, kf in zip(slots, kfs):
        db.set_stereo(s, np.stack([kf["kx"], kf["ky"]], 1), kf["depth"])
    return slots


def views_of(c, idx):
    from coeb_front import kf_view
    return np.array([kf_view(**c["views"][i]) for i in idx])


def call(db, c, only_stereo, slot_of=lambda s: s):
    k1 = c["kfs"][c["slot1"]]
    return db.create_new_map_points(slot_of(c["slot1"]), views_of(c, [c["slot1"]])[0], k1["has_mp"],
                                    [slot_of(s) for s in c["slots2"]], views_of(c, c["slots2"]),
                                    [c["kfs"][s]["has_mp"] for s in c["slots2"]], c["F12"], c["epipole"], only_stereo)


def check(got, want):
    for k in ("match", "status", "source", "first_ok", "nmatches"):
        assert np.array_equal(got[k], want[k]), k
    acc = want["status"] == N.ACCEPTED
    assert np.array_equal(got["x3d"][acc].view(np.uint32), want["x3d"][acc].view(np.uint32))
    assert np.isnan(got["x3d"][~acc]).all()             # the binding's initial value: untouched


@pytest.mark.parametrize("name", C.names())
def test_directed_case(ctx, name):
    from coeb_front import KeyFrameDatabase
    t = ctx.tables()
    assert np.array_equal(np.array(t.scale[:8], np.float32), C.SCALE)
    assert np.array_equal(np.array(t.sigma2[:8], np.float32), C.SIGMA2)
    c = C.case(name)
    db = KeyFrameDatabase(ctx, max_features=200, initial_slots=2)
    try:
        assert load(db, c["kfs"]) == list(range(len(c["kfs"])))
        k1 = c["kfs"][c["slot1"]]
        for only_stereo in (False, True):
            got = call(db, c, only_stereo)
            check(got, C.expected(name, only_stereo))
            m, nm = db.search_for_triangulation(c["slot1"], k1["has_mp"], c["slots2"],
                                                [c["kfs"][s]["has_mp"] for s in c["slots2"]], c["F12"], c["epipole"],
                                                only_stereo, False)
            assert np.array_equal(got["match"], m) and np.array_equal(got["nmatches"], nm)
    finally:
        db.close()
