"""The inputs of tests/test_gpu_overlap_inputs.py, checked on the oracle alone (no GPU).

The GPU tests alternate between the input sets A, B, C and rely on a stale read being visible:
here differs() is asserted for every pair of sets on the frames a GPU test compares with the
oracle (the F = 8 sets whole, under the tracking chain, and the chunk-boundary frames of the
chunked sizes, and the F = 33 sets under the chain, which the GPU tests run over two chunk
streams), together with the floors the GPU tests rely on: >= 100 keypoints and >= 20
motion-model matches on every frame, every frame of a chain tracked (state 2).  make_chunks'
boundaries are pinned by a restatement, so the GPU tests' "first frame of a chunk" indices are
no guesses.
"""
import itertools

import numpy as np
import pytest

import overlap_cases as oc

PAIRS = list(itertools.combinations(oc.NAMES, 2))
STRIDE = 564         # the batch's keypoint slots per frame at 320x240, 500 features (asserted on the device)


def boundary_union():
    fr = set()
    for F, ns in oc.CHUNKED + ((oc.MID_F, 4), (64, 3), (oc.SMALL_F, 1)):
        fr |= set(oc.boundary_frames(F, ns))
    return sorted(fr)


def test_chunk_boundaries():
    want = {(33, 2): [0, 16, 33], (49, 3): [0, 16, 32, 49], (64, 4): [0, 16, 32, 48, 64], (65, 4): [0, 16, 32, 48, 65],
            (31, 4): [0, 31], (48, 4): [0, 16, 32, 48], (8, 4): [0, 8]}
    for (F, ns), b in want.items():
        assert oc.chunks(F, ns) == b, (F, ns)           # oc.chunks: make_chunks restated in three lines
    assert oc.boundary_frames(33, 2) == [0, 15, 16, 32]
    assert oc.boundary_frames(49, 3) == [0, 15, 16, 31, 32, 48]
    assert oc.boundary_frames(64, 4) == [0, 15, 16, 31, 32, 47, 48, 63]
    assert boundary_union() == [0, 7, 15, 16, 20, 21, 31, 32, 41, 42, 47, 48, 63]


def test_sets_share_frames_and_never_repeat():
    """Frame k of a set depends on (set, k) alone, and no two sets share a frame, a depth map or
    (from frame 1 on) a pose."""
    for name in oc.NAMES:
        s, s8 = oc.make_set(name), oc.make_set(name, oc.SMALL_F)
        assert s["frames"].shape == (oc.FMAX, oc.H, oc.W) and s8["frames"].shape == (oc.SMALL_F, oc.H, oc.W)
        assert np.array_equal(s8["frames"], s["frames"][:oc.SMALL_F]) and s8["depth"].tobytes() == s["depth"][:8].tobytes()
        holes = ~(s["depth"] > 0)
        assert 0.15 < holes.mean() < 0.45
    for x, y in PAIRS:
        a, b = oc.make_set(x), oc.make_set(y)
        for f in range(oc.FMAX):
            assert not np.array_equal(a["frames"][f], b["frames"][f])
            assert a["depth"][f].tobytes() != b["depth"][f].tobytes()
            assert a["Tcw"][f].tobytes() != b["Tcw"][f].tobytes()


@pytest.fixture(scope="module")
def boundary_records(oracle_mod):
    return {name: {f: oc.oracle_record(oracle_mod, name, f) for f in boundary_union()} for name in oc.NAMES}


def test_boundary_frames_differ_and_are_full(boundary_records):
    for name, recs in boundary_records.items():
        for f, r in recs.items():
            assert len(r["kps"]) >= 100, (name, f, len(r["kps"]))
            if f:
                assert r["nmatch"] >= 20, (name, f, r["nmatch"])
    for x, y in PAIRS:
        assert oc.differs(boundary_records[x], boundary_records[y]), (x, y)


@pytest.mark.parametrize("F,nkf", [(oc.SMALL_F, 2), (oc.SMALL_F, 1), (33, 2)])
def test_chain_sets_differ_and_are_tracked(oracle_mod, F, nkf):
    """Every (F, nkf) the GPU tests run the tracking chain at: each frame tracked, and each pair
    of sets different in every frame's keypoints, matches, pose and local matches."""
    recs = {}
    for name in oc.NAMES:
        ext, res = oc.oracle_chain(oracle_mod, name, STRIDE, nkf, F)
        recs[name] = oc.chain_records(ext, res)
        for f in range(F):
            assert len(ext[f]["kps"]) >= 100, (name, f)
            if f:
                assert res[f]["nmatches"] >= 20 and res[f]["state"] == 2, (name, f, res[f]["nmatches"], res[f]["state"])
                # the chain's motion-model match is the batch matcher's
                o = oc.oracle_record(oracle_mod, name, f)
                assert o["nmatch"] == res[f]["nmatches"] and np.array_equal(o["match"], res[f]["match"]), (name, f)
    for x, y in PAIRS:
        assert oc.differs(recs[x], recs[y]), (x, y)


def test_differs_notices_one_equal_field(boundary_records):
    """differs() is false as soon as one frame shares its keypoints or its matches."""
    a, b = boundary_records["A"], boundary_records["B"]
    assert not oc.differs(a, a)
    assert oc.differs(a, b)
    for f, rec in ((16, dict(b[16], match=a[16]["match"])), (16, dict(a[16], match=b[16]["match"])), (0, a[0])):
        other = dict(b)
        other[f] = rec
        assert not oc.differs(a, other), f
