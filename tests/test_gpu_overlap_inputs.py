"""Overlapped batch steps on inputs that change from step to step (MI355X only).

Every other test that runs batch steps back to back runs one input again, so a kernel that
started before its producer, or a buffer overwritten before its reader finished, reads or
leaves the same bytes and passes.  Here consecutive steps run on the input sets A, B, C of
tests/overlap_cases.py, which differ in every frame's keypoints, matches, poses and local-map
matches (asserted on the oracle in tests/test_overlap_cases.py), with no host synchronisation
between steps (overlap_cases.Stepper).  Each comparison is bit for bit against a serial,
synchronised step on the same set (serial_reference) run on ANOTHER context, so the context
under test never holds the right answer before it computes it; the references' first, last
and chunk-boundary frames are compared with the oracle.

What the tests can notice depends on timing: a missing wait shows only when the two streams
actually race.  DESIGN.md s2.2 lists which removed waits these tests caught on the device.
"""
import numpy as np
import pytest

import chain_util as cu
import overlap_cases as oc
from overlap_cases import Stepper, step

pytestmark = pytest.mark.gpu

STREAMS = {8: (1,), 33: (2,), 48: (3,), 49: (3,), 64: (4, 3)}      # the chunkings a batch size runs under


@pytest.fixture(scope="module")
def refs(oracle_mod):
    """refs(F, name, **step_kw): the serial reference of one step, computed once on a context of
    its own per batch size; plain extractions and matches are checked against the oracle."""
    pipes, cache = {}, {}

    def get(F, name, **kw):
        key = (F, name, tuple(sorted(kw.items())))
        if key in cache:
            return cache[key]
        if F not in pipes:
            pipes[F] = oc.open_pipeline(F)
        if kw.get("bow") and not getattr(pipes[F], "ov_voc", False):
            set_vocabulary(pipes[F])
        r = oc.serial_reference(pipes[F], name, **kw)
        if not kw.get("dyn") and not kw.get("boxes"):
            frames = sorted({f for ns in STREAMS[F] for f in oc.boundary_frames(F, ns)})
            oc.assert_oracle_frames(oracle_mod, r, name, frames, "reference F=%d" % F)
        if kw.get("track"):                      # as the oracle's chain (tests/test_overlap_cases.py): every frame tracked,
            assert oc.states(r)[1:] == [2] * (F - 1), (F, name, oc.states(r))      # so no field of it is skipped below
        cache[key] = r
        return r
    yield get
    for p in pipes.values():
        oc.close_pipeline(p)


def set_vocabulary(bp):
    from coeb_front import Vocabulary
    from test_gpu_bow import voc_case
    v = Vocabulary.from_arrays(*voc_case("k10")[0])
    bp.ctx.set_vocabulary(v)
    v.close()
    bp.ov_voc = True


def run_steps(F, steps, streams=None, max_F=None):
    bp = oc.open_pipeline(F, max_F)
    try:
        assert bp.ctx.max_keypoints(oc.W, oc.H) == 564         # the stride tests/test_overlap_cases.py ran the oracle chain with
        if streams:
            bp.ctx.set_batch_streams(streams)
        return Stepper(bp).run(steps)
    finally:
        oc.close_pipeline(bp)


# ------------------------------------------------------------------ 1. chunked steps on alternating inputs
@pytest.mark.parametrize("F,ns", oc.CHUNKED)
def test_chunked_steps_on_alternating_inputs(refs, F, ns):
    """A B C B A over ns chunk streams, every step collected: chunk k's matcher needs chunk
    k-1's k_prep of THIS step (ev_prep), the chunk streams need the context stream's earlier
    work (ev_main), and the downloads need every chunk stream (main_stream)."""
    order = "ABCBA"
    got = run_steps(F, [step(n) for n in order], streams=ns)
    for i, n in enumerate(order):
        oc.assert_step_equal(got[i], refs(F, n), (i, n))


def test_chunked_steps_with_host_poses(refs):
    """The same through coeb_match_batch_device: the poses are copied from host memory on the
    context stream, and the chunk streams' matchers wait for that copy (ev_main)."""
    order = "ABCA"
    got = run_steps(64, [step(n, host_pose=True) for n in order], streams=4)
    for i, n in enumerate(order):
        oc.assert_step_equal(got[i], refs(64, n), (i, n))


# ------------------------------------------------------------------ 2. a fresh context whose first step is chunked
def test_first_step_of_a_fresh_context_is_chunked(refs):
    got = run_steps(64, [step("A")], streams=4)
    oc.assert_step_equal(got[0], refs(64, "A"))


# ------------------------------------------------------------------ 3. write after read across steps
@pytest.mark.parametrize("F,ns", oc.CHUNKED)
def test_next_extraction_waits_for_the_previous_matchers(refs, F, ns):
    """Step i + 1's extraction of chunk k overwrites the keypoints the matcher of chunk k + 1 of
    step i still reads (the `cross` wait on ev_mdone[k + 1]); the matches left behind are step
    i's, the keypoints step i + 1's."""
    got = run_steps(F, [step("A", collect=False), step("B", match=False)], streams=ns)
    oc.assert_extract_equal(got[1], refs(F, "B"), "AB")
    oc.assert_match_equal(got[1], refs(F, "A"), "AB")
    got = run_steps(F, [step("A", collect=False), step("B", collect=False), step("C", match=False)], streams=ns)
    oc.assert_extract_equal(got[2], refs(F, "C"), "ABC")
    oc.assert_match_equal(got[2], refs(F, "B"), "ABC")


# ------------------------------------------------------------------ 4. the schedule changes between steps
def test_stream_count_changes_between_steps(refs):
    order, ns = "ABCA", (4, 3, 1, 4)
    got = run_steps(64, [step(n, streams=s) for n, s in zip(order, ns)])
    for i, n in enumerate(order):
        oc.assert_step_equal(got[i], refs(64, n), (i, n))


@pytest.mark.parametrize("kind", ["dyn", "boxes"])
def test_serial_step_between_chunked_steps(refs, kind):
    """dyn: dynamic boxes and T_M take coeb_extract_batch_device's serial branch; boxes:
    run(frame=True), coeb_frame_batch_device, resets the chunk table.  The chunked step before
    is not collected: the serial step's own joins order it."""
    kw = {kind: True}
    got = run_steps(64, [step("A", collect=False), step("B", **kw), step("C"), step("A", **kw), step("B")], streams=4)
    oc.assert_step_equal(got[1], refs(64, "B", **kw), "B " + kind)
    oc.assert_step_equal(got[2], refs(64, "C"), "C")
    oc.assert_step_equal(got[3], refs(64, "A", **kw), "A " + kind)
    oc.assert_step_equal(got[4], refs(64, "B"), "B")
    if kind == "dyn":                            # the mask removes keypoints (the sets' scenes hold no moving object:
        assert not np.array_equal(refs(64, "B")["counts"], refs(64, "B", **kw)["counts"])      # T_M of "boxes" is empty)


def test_smaller_batch_between_two_full_ones(refs):
    """48 frames between two batches of 64 on a context with max_batch = 64 (batch_frames != F)."""
    got = run_steps(64, [step("A", collect=False), step("B", F=oc.MID_F), step("C"), step("A", F=oc.MID_F, collect=False),
                         step("B")], streams=4)
    oc.assert_step_equal(got[1], refs(oc.MID_F, "B"), "B 48")
    oc.assert_step_equal(got[2], refs(64, "C"), "C 64")
    oc.assert_step_equal(got[4], refs(64, "B"), "B 64")


# ------------------------------------------------------------------ 5. the pose stream under a following step
@pytest.mark.parametrize("F,ns2,nkf", [(8, 1, 2), (8, 1, 1), (33, 2, 2)])
def test_pose_stream_reads_only_its_snapshots(refs, F, ns2, nkf):
    """Step 2 (extract + match on B, over ns2 chunk streams) starts while the pose stream still
    works on step 1 (the tracking chain on A): k_pose, k_tlm_frustum, k_match_local and the
    second k_pose must read their snapshots only.  A collected step on C runs first, so the
    pose buffers hold C's answers, not A's, when step 1 starts."""
    got = run_steps(F, [step("C", track=True, nkf=nkf), step("A", collect=False, track=True, nkf=nkf),
                        step("B", streams=ns2)])
    oc.assert_step_equal(got[0], refs(F, "C", track=True, nkf=nkf), "C")
    a, b = refs(F, "A", track=True, nkf=nkf), refs(F, "B")
    oc.assert_pose_equal(got[2], a, "pose of A")
    oc.assert_track_equal(got[2], a, "track of A")
    oc.assert_extract_equal(got[2], b, "B")
    oc.assert_match_equal(got[2], b, "B")


@pytest.mark.parametrize("F,ns", [(8, 1), (33, 2)])
def test_chain_step_behind_an_uncollected_chain_step(refs, F, ns):
    """Two tracking steps back to back, the first not collected: the second reaches join_pose() at
    the head of coeb_pose_batch_device with the pose stream still pending (every other test
    clears pose_pending first: a collected step and a synchronisation join the pose stream, and
    the step after an uncollected chain step has no pose).  Its memsets and k_track_prep then
    overwrite bp.t_* under the first step's k_pose unless that call waits."""
    got = run_steps(F, [step("C", track=True), step("A", collect=False, track=True), step("B", track=True)], streams=ns)
    oc.assert_step_equal(got[0], refs(F, "C", track=True), "C")
    oc.assert_step_equal(got[2], refs(F, "B", track=True), "B")


# ------------------------------------------------------------------ 6. the tracking chain on alternating inputs
def test_tracking_chain_on_alternating_inputs(refs, oracle_mod):
    """ev_tprep, ev_tlm and the main_stream join before k_track_prep / k_tlm_snapshot.  Every step
    is collected, so join_pose() at the head of coeb_pose_batch_device finds nothing pending here
    (test_chain_step_behind_an_uncollected_chain_step reaches it).  The first step is the
    oracle's chain."""
    F = oc.SMALL_F
    bp = oc.open_pipeline(F)
    try:
        oc.select(bp, "A", F)
        bp.run(track=True)
        bp.synchronize()
        ext, res = oc.oracle_chain(oracle_mod, "A", bp.ctx.batch_results()[3])
        st, _ = cu._check_chain(bp, ext, res, F)
        assert st == [2] * (F - 1)
        bp.ov_F.update(match=F, pose=F, track=F)
        order = "BCAB"
        got = Stepper(bp).run([step(n, track=True) for n in order])
        for i, n in enumerate(order):
            oc.assert_step_equal(got[i], refs(F, n, track=True), (i, n))
    finally:
        oc.close_pipeline(bp)


def test_tracking_chain_behind_chunked_matchers(refs):
    """F = 33 over two chunk streams: chunked extraction and matching feed k_track_prep on the
    context stream."""
    order = "ABCA"
    got = run_steps(33, [step(n, track=True) for n in order], streams=2)
    for i, n in enumerate(order):
        oc.assert_step_equal(got[i], refs(33, n, track=True), (i, n))


# ------------------------------------------------------------------ 7. side-stream modes, pipelines interleaved
@pytest.mark.parametrize("side", ["own", "shared", "eager", "off"])
def test_interleaved_pipelines_side_stream_modes(refs, monkeypatch, side):
    """Two pipelines on one thread, stepped in turn as the benchmark does, swapping their sets in
    round two; collected after round two only."""
    want = {name: refs(oc.SMALL_F, name) for name in ("B", "C")}      # the reference context exists before the modes are set
    monkeypatch.setenv("COEB_SIDE_SHARED", "1" if side == "shared" else "0")
    monkeypatch.setenv("COEB_SIDE_EAGER", "1" if side == "eager" else "0")
    monkeypatch.setenv("COEB_SIDE_STREAM", "0" if side == "off" else "1")
    import ctypes as C
    from coeb_front import HostBuffer, lib
    F = oc.SMALL_F
    bps, bufs = [], []
    try:
        for _ in range(2):
            bps.append(oc.open_pipeline(F))
        K = bps[0].ctx.max_keypoints(oc.W, oc.H)
        for bp in bps:
            bp.ov_F["match"] = F
            for name in oc.NAMES:                # every upload before the first step
                oc.select(bp, name, F)
            bufs.append({k: HostBuffer(n) for k, n in oc.array_sizes(bp, F, False).items()})
        for rnd in (("A", "B"), ("B", "C")):
            for bp, name in zip(bps, rnd):
                oc.enqueue(bp, step(name))
        for bp, hb in zip(bps, bufs):
            ptr = oc.device_arrays(bp, F, False)
            for k, b in hb.items():
                bp.ctx.check(lib().coeb_memcpy_d2h_async(bp.ctx.h, C.c_void_p(b.ptr), C.c_void_p(ptr[k]), b.nbytes))
        for bp in bps:
            bp.synchronize()
        for hb, name in zip(bufs, ("B", "C")):
            oc.assert_step_equal(oc.shaped({k: b.array for k, b in hb.items()}, F, K), want[name], (side, name))
    finally:
        for bp in bps:
            oc.close_pipeline(bp)
        for hb in bufs:
            for b in hb.values():
                b.free()


# ------------------------------------------------------------------ 8. the batch BoW transform behind chunked extraction
def test_bow_transform_behind_chunked_extraction(refs):
    bp = oc.open_pipeline(33)
    try:
        set_vocabulary(bp)
        bp.ctx.set_batch_streams(2)
        got = Stepper(bp).run([step("A", bow=True), step("B", bow=True)])
    finally:
        oc.close_pipeline(bp)
    for g, n in zip(got, "AB"):
        r = refs(33, n, bow=True)
        assert (r["word"][0, :r["counts"][0]] >= 0).all()
        oc.assert_step_equal(g, r, n)
