"""The Fuse search on the device (k_fuse_grid, k_fuse) over the directed inputs of tests/fuse_cases.py
(MI355X only): every best_idx and best_dist entry has to equal the model (tests/fuse_ref.py)."""
import numpy as np
import pytest

import fuse_cases as C

pytestmark = pytest.mark.gpu


def load(db, kfs):
    """The keyframes into the database, with their geometry -> their slots."""
    from coeb_front import KEYPOINT_DTYPE
    slots = []
    for kf in kfs:
        n = len(kf["x"])
        s = db.add(kf["desc"], np.full(n, -1, np.int32), np.zeros(n, np.float32), np.zeros(0, np.int32), np.zeros(0))
        keys = np.zeros(n, KEYPOINT_DTYPE)
        keys["x"], keys["y"], keys["octave"] = kf["x"], kf["y"], kf["octave"]
        db.set_geometry(s, keys, kf["u_right"])
        slots.append(s)
    return slots


def jobs_of(c, slots):
    return [dict(slot=slots[j["kf"]], Rcw=j["Rcw"], tcw=j["tcw"], Ow=j["Ow"], first=j["first"], count=j["count"],
                 skip=j["skip"]) for j in c["jobs"]]


def check_tables(ctx, cam):
    t = ctx.tables()
    assert t.nlevels == cam.nlevels
    assert np.array_equal(np.array(t.scale[:cam.nlevels], np.float32), cam.scale)
    assert np.array_equal(np.array(t.inv_sigma2[:cam.nlevels], np.float32), cam.inv_sigma2)


@pytest.mark.parametrize("name", C.names())
def test_directed_case(ctx, name):
    from coeb_front import KeyFrameDatabase
    c = C.case(name)
    check_tables(ctx, c["cam"])
    db = KeyFrameDatabase(ctx, max_features=64, initial_slots=1)
    try:
        slots = load(db, c["kfs"])
        want_i, want_d = C.expected(name)
        for _ in range(2):                                  # the second call finds the grids built
            got_i, got_d = db.fuse_search(c["cam"].tuple(), c["pts"], jobs_of(c, slots), c["th"])
            assert len(got_i) == len(want_i)
            for j in range(len(want_i)):
                assert got_d[j].tolist() == want_d[j].tolist(), j
                assert got_i[j].tolist() == want_i[j].tolist(), j
    finally:
        db.close()
