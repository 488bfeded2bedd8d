"""The batched moving-object chain on directed heterogeneous batches (MI355X only).

coeb_frame_batch_device computes T_M of every frame through pmo_batch: one launch sequence over
all F - 1 consecutive pairs.  The frame lists of tests/flow_batch_cases.py put pairs without
corners at the start, at the end and in runs, a pair at the 1000-corner cap, pairs of a handful
of corners and neighbours that look nothing alike into one batch, and 1029 pairs into another
(two rounds of k_flow_index); tests/test_flow_batch_cases.py asserts on the oracle alone that
they do.  Here every pair's block of the flow scratch (Context.flow_pair), every frame's T_M,
blur flags and masked extraction are compared with the oracle run pair by pair and frame by
frame.  Every comparison is bit for bit.

Sizes: a default (8-level) context plans no frame under 221x221 (224x208, for one, has a 58-px
level 7), so the small cases run at 221x221; the second, smaller size of the state test needs a context of its
own with 5 levels (163x131); the 96x80 batch of 1030 frames takes a 2-level context.
"""
import numpy as np
import pytest

import coeb_front as cf
import flow_batch_cases as fc

pytestmark = pytest.mark.gpu


def run_case(c, case):
    """One coeb_frame_batch_device over the case's frames; everything the device kept of it."""
    F, w, h = len(case["frames"]), case["w"], case["h"]
    boxes, off = fc.box_arrays(case)
    nbox = int(off[-1])
    gray = c.upload(case["frames"])
    try:
        c.frame_batch_device(gray.ptr, F, w, h, boxes if nbox else None, off if nbox else None)
        c.synchronize()
        tms, flags = c.batch_frame_results(F, nbox)
        kp_ptr, desc_ptr, cnt_ptr, kcap = c.batch_results()
        n = c.download(cnt_ptr, 4 * F, np.int32)
        kps = c.download(kp_ptr, 28 * kcap * F, np.uint8).view(cf.KEYPOINT_DTYPE).reshape(F, kcap)
        desc = c.download(desc_ptr, 32 * kcap * F, np.uint8).reshape(F, kcap, 32)
        ext = [(kps[f, :n[f]].copy(), desc[f, :n[f]].copy()) for f in range(F)]
        if F >= 2:
            pairs = [c.flow_pair(z) for z in range(F - 1)]
            counts = c.debug_read("flow_counts").view(np.int32).reshape(-1, 2)
        else:
            pairs, counts = [], np.zeros((0, 2), np.int32)
    finally:
        c.synchronize()
        gray.free()
    return dict(tm=tms, flags=flags, off=off, ext=ext, pairs=pairs, counts=counts)


def check_flow(got, ref, tag):
    """Every pair's intermediates and every frame's T_M against the oracle."""
    assert len(got["pairs"]) == len(ref["pairs"]) == len(got["counts"]), tag
    for z, (g, r) in enumerate(zip(got["pairs"], ref["pairs"])):
        at = (tag, "pair", z)
        assert g["npts"] == r["npts"] == got["counts"][z, 1], at
        assert np.array_equal(g["corners"], r["corners"]), at
        assert np.array_equal(g["status"], r["status"]), at
        ok = r["status"] == 1
        assert np.array_equal(g["next_pts"][ok], r["next_pts"][ok]), at
        assert np.array_equal(g["state"], r["state"]), at
        assert g["nf"] == r["nf"], at
        if r["F"] is not None:
            assert np.array_equal(g["F"], r["F"]), at
    assert got["tm"][0] is not None and len(got["tm"][0]) == 0, tag
    for f in range(1, len(ref["tm"])):
        g, r = got["tm"][f], ref["tm"][f]
        assert (g is None) == (r is None), (tag, "T_M", f)
        if r is not None:
            assert np.array_equal(g, r), (tag, "T_M", f)


def check_frames(got, ref, tag):
    """Blur flags and every field of the masked extraction of every frame."""
    off = got["off"]
    for f, r in enumerate(ref["ext"]):
        assert np.array_equal(got["flags"][off[f]:off[f + 1]], ref["blur"][f]), (tag, "blur", f)
        k, d = got["ext"][f]
        for name in r["kps"].dtype.names:
            assert np.array_equal(k[name], r["kps"][name]), (tag, f, name)
        assert np.array_equal(d, r["desc"]), (tag, f)


def same_run(a, b, tag):
    """Two runs of one case kept the same bytes of everything the oracle defines."""
    assert np.array_equal(a["counts"], b["counts"]), tag
    for z, (p, q) in enumerate(zip(a["pairs"], b["pairs"])):
        for key in ("npts", "nf"):
            assert p[key] == q[key], (tag, z, key)
        for key in ("corners", "status", "state"):
            assert np.array_equal(p[key], q[key]), (tag, z, key)
        ok = p["status"] == 1
        assert np.array_equal(p["next_pts"][ok], q["next_pts"][ok]), (tag, z)
    for f in range(len(a["tm"])):
        assert (a["tm"][f] is None) == (b["tm"][f] is None), (tag, f)
        if a["tm"][f] is not None:
            assert np.array_equal(a["tm"][f], b["tm"][f]), (tag, f)
        if a["tm"][f] is not None and f:
            assert np.array_equal(a["pairs"][f - 1]["F"], b["pairs"][f - 1]["F"]), (tag, f)
        assert np.array_equal(a["ext"][f][0], b["ext"][f][0]) and np.array_equal(a["ext"][f][1], b["ext"][f][1]), (tag, f)
    assert np.array_equal(a["flags"], b["flags"]), tag


@pytest.mark.parametrize("name", ["mixed", "empty_first", "empty_last", "empty_run", "cap", "two_frames"])
def test_batch_case_matches_oracle(ctx, oracle_mod, name):
    case = fc.build(name)
    ref = fc.oracle_case(oracle_mod, case)
    got = run_case(ctx, case)
    check_flow(got, ref, name)
    check_frames(got, ref, name)


def test_one_frame_has_no_flow(oracle_mod):
    """F = 1 on a context that has run no batch: ntm[0] = 0, the extraction is unmasked, and
    there is no moving-object batch to read."""
    case = fc.build("one_frame")
    ref = fc.oracle_case(oracle_mod, case)
    c = cf.Context(max_width=case["w"], max_height=case["h"], max_batch=2)
    try:
        got = run_case(c, case)
        check_flow(got, ref, "one_frame")
        check_frames(got, ref, "one_frame")
        for what in ("flow_pair", "flow_counts"):
            with pytest.raises(cf.CoebError):
                c.debug_read(what, 0)
    finally:
        c.close()


def test_round_of_1029_pairs(oracle_mod):
    """1030 frames of 96x80: the flattened list spans both rounds of k_flow_index, the second one
    starting inside the non-empty pairs 1022 .. 1026."""
    case = fc.build("round")
    ref = fc.oracle_case(oracle_mod, case, fc.ROUND_LEVELS)
    c = cf.Context(nlevels=fc.ROUND_LEVELS, max_width=case["w"], max_height=case["h"], max_batch=len(case["frames"]))
    try:
        got = run_case(c, case)
        check_flow(got, ref, "round")
        check_frames(got, ref, "round")
    finally:
        c.close()


def _small_context():
    w, h = fc.CAP_SIZE
    return cf.Context(nlevels=fc.SMALL_LEVELS, max_width=w, max_height=h, max_batch=10)


def test_state_across_batches(oracle_mod):
    """cap, empty_run, mixed, mixed at 163x131, mixed again on one context: every run equals the
    oracle and the run of a fresh context, so no count, rmax / nkeys word, T_M slot or scratch
    layout of an earlier batch (more pairs, fewer pairs, larger frames, smaller frames) leaks."""
    steps = [("cap", ()), ("empty_run", ()), ("mixed", ()), ("mixed", fc.SMALL_SIZE), ("mixed", ())]
    c = _small_context()
    try:
        for i, (name, size) in enumerate(steps):
            case = fc.build(name, *size)
            ref = fc.oracle_case(oracle_mod, case, fc.SMALL_LEVELS)
            tag = "%d:%s%s" % (i, name, size)
            got = run_case(c, case)
            check_flow(got, ref, tag)
            check_frames(got, ref, tag)
            fresh = _small_context()
            try:
                same_run(got, run_case(fresh, case), tag)
            finally:
                fresh.close()
    finally:
        c.close()


def test_single_pair_call_retires_the_batch(ctx, oracle_mod):
    """A single-pair call between two batches rewrites the flow scratch: flow_pair and
    flow_counts refuse until the next batch, which then reads right again; a pair index outside
    the batch is refused as well."""
    case = fc.build("empty_run")
    ref = fc.oracle_case(oracle_mod, case)
    check_flow(run_case(ctx, case), ref, "before")
    P = len(case["frames"]) - 1
    for z in (-1, P, P + 1000):
        with pytest.raises(cf.CoebError):
            ctx.flow_pair(z)
    ctx.flow_pair(P - 1)
    tm = cf.ProcessMovingObject(ctx, case["frames"][0], case["frames"][1])
    assert np.array_equal(tm, ref["tm"][1])
    with pytest.raises(cf.CoebError):
        ctx.flow_pair(0)
    with pytest.raises(cf.CoebError):
        ctx.debug_read("flow_counts")
    got = run_case(ctx, case)
    check_flow(got, ref, "after")
    check_frames(got, ref, "after")
