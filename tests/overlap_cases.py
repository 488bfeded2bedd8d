"""Inputs, references and the step driver of the overlapped-batch tests.

tests/test_overlap_cases.py (CPU) and tests/test_gpu_overlap_inputs.py (MI355X) share this file.
The batch path keeps several HIP streams busy at once (chunk streams, the pose stream, the side
stream); every other test that runs steps back to back feeds each step the same input, so a
consumer that started before its producer would read the previous step's identical bytes.  Here
a step selects one of three input sets A, B, C (frames, per-frame depth with holes, predicted
poses) that differ in every result of every frame (differs(), asserted on the oracle), the
input buffers are uploaded once and never rewritten, and every comparison is exact.

Shape: 320x240, 500 features, 8 levels (level 7 is 89x67, the smallest plan the default scale
takes).  Batch sizes: make_chunks cuts F frames over n = min(streams, F // 16) chunks at
F * k // n: 33 -> (0, 16, 33), 49 -> (0, 16, 32, 49), 64 -> (0, 16, 32, 48, 64); F = 8 never
chunks.  Frame k of a set depends on (set, k) alone, so the sets of every F share their frames
and one oracle result per (set, frame) serves all of them.
"""
import numpy as np

import chain_util as cu
from coeb_front import synth

W, H = 320, 240
NFEATURES = 500
NAMES = ("A", "B", "C")
FMAX = 64
SMALL_F = 8
CHUNKED = ((33, 2), (49, 3), (64, 4))
MID_F = 48                               # the batch run between two of 64 on one context
SEEDS = dict(A=(6100, 910), B=(6200, 920), C=(6300, 930))        # (frames, depth)
POSE_FIRST = dict(B=0, C=5)              # synth.perturbed_poses(first=...); A: the exact image motion
INTR = cu.intrinsics(W, H)


def chunks(F, ns):
    """make_chunks (coeb_capi.hip) restated: the chunk boundaries of F frames over ns streams."""
    n = max(1, min(ns, F // 16))
    return [F * k // n for k in range(n + 1)]


def boundary_frames(F, ns):
    """The first and the last frame and the frames on both sides of every chunk boundary."""
    b = chunks(F, ns)
    return sorted({0, F - 1} | {f for k in b[1:-1] for f in (k - 1, k)})


_sets = {}


def make_set(name, F=FMAX):
    """dict(frames (F, H, W) u8, depth (F, H, W) f32, Tcw (F, 4, 4) f32): the first F frames of set `name`."""
    if name not in _sets:
        fs, ds = SEEDS[name]
        if name == "A":
            Tcw = np.stack([cu._motion_pose(W, H)] * FMAX)
        else:
            Tcw = synth.perturbed_poses(FMAX, first=POSE_FIRST[name])
        _sets[name] = dict(frames=synth.make_frames(W, H, FMAX, seed=fs), depth=synth.depth_sequence(W, H, FMAX, seed=ds),
                           Tcw=np.ascontiguousarray(Tcw, np.float32))
    return {k: v[:F] for k, v in _sets[name].items()}


def dyn_inputs(F):
    """BatchPipeline.dyn of F frames: synth.dynamic_inputs scaled to the shape, the same for every frame."""
    b, t, bl = synth.dynamic_inputs(W, H)
    return (np.concatenate([b] * F), np.arange(F + 1, dtype=np.int32) * len(b), np.concatenate([t] * F),
            np.arange(F + 1, dtype=np.int32) * len(t), np.concatenate([bl] * F))


def frame_boxes(F):
    return [synth.dynamic_inputs(W, H)[0]] * F


# ------------------------------------------------------------------ the oracle, one result per (set, frame)
_ex = {}
_orc = {}


def extractor(oracle_mod):
    if "ex" not in _ex:
        _ex["ex"] = oracle_mod.Extractor(NFEATURES, 1.2, 8, 20, 7)
    return _ex["ex"]


def oracle_extract(oracle_mod, name, f):
    key = ("ext", name, f)
    if key not in _orc:
        _orc[key] = extractor(oracle_mod).extract(make_set(name)["frames"][f])
    return _orc[key]


def oracle_record(oracle_mod, name, f):
    """Frame f of set `name` as the batch computes it: dict(kps, desc) and for f >= 1 (nmatch,
    match) of SearchByProjection against frame f - 1 with the retry at 2 th (Tracking.cc:954-958)."""
    key = ("rec", name, f)
    if key in _orc:
        return _orc[key]
    s = make_set(name)
    r = oracle_extract(oracle_mod, name, f)
    rec = dict(kps=r["kps"], desc=r["desc"])
    if f:
        ex = extractor(oracle_mod)
        rp = oracle_extract(oracle_mod, name, f - 1)
        cam_o = cu.cameras(oracle_mod, ex, W, H)[0]
        last = oracle_mod.mapframe_from_extraction(rp["kps"], rp["desc"], s["depth"][f - 1], *INTR)
        ur, _ = oracle_mod.stereo_from_rgbd(r["kps"], s["depth"][f], INTR[4])
        I4 = np.eye(4, dtype=np.float32)
        nm, m = oracle_mod.search_by_projection(cam_o, r["kps"], r["desc"], ur, last, s["Tcw"][f], I4, 15.0)
        if nm < 20:
            nm, m = oracle_mod.search_by_projection(cam_o, r["kps"], r["desc"], ur, last, s["Tcw"][f], I4, 30.0)
        rec.update(nmatch=nm, match=m)
    _orc[key] = rec
    return rec


def oracle_chain(oracle_mod, name, stride, nkf=2, F=SMALL_F):
    """(ext, res) of chain_util._chain_oracle over the first F frames of set `name`."""
    key = ("chain", name, stride, nkf, F)
    if key not in _orc:
        ex = extractor(oracle_mod)
        s = make_set(name, F)
        isg = np.array(ex.p.inv_sigma2[:8], np.float32)
        _orc[key] = cu._chain_oracle(oracle_mod, ex, s["frames"], None, s["Tcw"], stride, isg, nkf=nkf, depth=s["depth"],
                                     nobs=2, intr=INTR)
    return _orc[key]


def chain_records(ext, res):
    """The oracle chain as per-frame records for differs()."""
    out = {}
    for f, e in enumerate(ext):
        rec = dict(kps=e["kps"], desc=e["desc"])
        if f:
            r = res[f]
            rec.update(nmatch=r["nmatches"], match=r["match"], state=r["state"], T=r["T"])
            if r["state"]:
                rec["local_match"] = r["local_match"]
        out[f] = rec
    return out


def differs(x, y):
    """x, y: {frame: record} of two sets.  True when, over their common frames, every frame's
    keypoint records differ, every frame >= 1 has a different match array, and every frame both
    tracked (state != 0) has a different pose and a different local-match array: a stale read of
    any of them cannot pass for the right answer."""
    common = sorted(set(x) & set(y))
    if not common:
        return False
    for f in common:
        a, b = x[f], y[f]
        if len(a["kps"]) == len(b["kps"]) and a["kps"].tobytes() == b["kps"].tobytes():
            return False
        if "match" in a and "match" in b and np.array_equal(a["match"], b["match"]):
            return False
        if a.get("state") and b.get("state"):
            if np.array_equal(np.asarray(a["T"], np.float32).view(np.uint32), np.asarray(b["T"], np.float32).view(np.uint32)):
                return False
            if np.array_equal(a["local_match"], b["local_match"]):
                return False
    return True


# ------------------------------------------------------------------ device side
def step(name, collect=True, streams=None, F=None, dyn=False, boxes=False, bow=False, host_pose=False, **run_kw):
    """One step of a Stepper: set `name`, BatchPipeline.run(**run_kw).  streams: set_batch_streams
    before it; F: a batch of another size on the same context; dyn: dynamic boxes and T_M;
    boxes: run(frame=True) with boxes; bow: bow_batch_device behind it; host_pose: the matcher
    through coeb_match_batch_device (poses from host memory) instead of the device poses."""
    return dict(name=name, collect=collect, streams=streams, F=F, dyn=dyn, boxes=boxes, bow=bow, host_pose=host_pose,
                kw=run_kw)


def open_pipeline(F, max_F=None):
    """A BatchPipeline of the shape with device-resident input sets (uploaded on first use, once)."""
    import coeb_front
    from coeb_front.pipeline import BatchPipeline
    bp = BatchPipeline(W, H, max_F or F, nfeatures=NFEATURES, camera=coeb_front.make_camera(*INTR, W, H))
    bp.F = bp.ov_base_F = F                      # a step without an F of its own runs ov_base_F frames
    bp.ov_sets = {}
    bp.ov_F = dict(match=0, pose=0, track=0)     # the batch size of the last matcher / pose / TrackLocalMap step
    return bp


def select(bp, name, F):
    """Point the pipeline at set `name` of F frames; no input buffer is ever rewritten."""
    key = (name, F)
    if key not in bp.ov_sets:
        s = make_set(name, F)
        bp.ov_sets[key] = (bp.ctx.upload(s["frames"]), bp.ctx.upload(s["depth"]), bp.ctx.upload(s["Tcw"].reshape(F, 16)),
                           s["Tcw"])
    bp.gray, bp.depth, bp.dTcw, bp.Tcw = bp.ov_sets[key]
    bp.F = F


def close_pipeline(bp):
    bp.gray = bp.depth = bp.dTcw = None
    try:
        bp.ctx.synchronize()
    finally:
        for bufs in bp.ov_sets.values():
            for b in bufs[:3]:
                b.free()
        bp.ov_sets = {}
        bp.close()


def enqueue(bp, st):
    """Enqueue step st; no host synchronisation."""
    F = st["F"] or bp.ov_base_F
    if st["streams"]:
        bp.ctx.set_batch_streams(st["streams"])
    select(bp, st["name"], F)
    kw = dict(st["kw"])
    bp.dyn = dyn_inputs(F) if st["dyn"] else None
    if st["boxes"]:
        bp.set_frame_boxes(frame_boxes(F))
        kw["frame"] = True
    if st["host_pose"]:
        assert not kw
        bp.ctx.extract_batch_device(bp.gray.ptr, F, W, H)
        bp.ctx.match_batch_device(bp.depth.ptr, F, W, H, bp.cam, bp.Tcw)
    else:
        bp.run(**kw)
    bp.dyn = None
    if kw.get("match", True):
        bp.ov_F["match"] = F
        if kw.get("pose") or kw.get("track"):
            bp.ov_F["pose"] = F
            bp.ov_F["track"] = F if kw.get("track") else 0
    if st["bow"]:
        bp.ctx.bow_batch_device(1)
    return F


DTYPES = dict(counts=np.int32, match=np.int32, nmatch=np.int32, pose_T=np.float32, pose_nin=np.int32, trk_T=np.float32,
              trk_nin=np.int32, trk_nmap=np.int32, trk_nloc=np.int32, trk_lm=np.int32, word=np.int32, node=np.int32)


def array_sizes(bp, F, bow):
    """{array: bytes} of every result array the context holds for a batch of F frames."""
    K = bp.ctx.max_keypoints(W, H)
    n = dict(kps=28 * K * F, desc=32 * K * F, counts=4 * F)
    if bp.ov_F["match"] == F:
        n.update(match=4 * K * F, nmatch=4 * F)
    if bp.ov_F["pose"] == F:
        n.update(pose_T=64 * F, pose_nin=4 * F, pose_outl=K * F)
    if bp.ov_F["track"] == F:
        n.update(trk_T=64 * F, trk_nin=4 * F, trk_nmap=4 * F, trk_nloc=4 * F, trk_lm=4 * K * F, trk_outl=K * F)
    if bow:
        n.update(word=4 * K * F, node=4 * K * F)
    return n


def device_arrays(bp, F, bow):
    """{array: device pointer} for array_sizes(); the pose getters join the pose stream."""
    c = bp.ctx
    kp, de, cn, K = c.batch_results()
    assert K == c.max_keypoints(W, H)
    p = dict(kps=kp, desc=de, counts=cn)
    if bp.ov_F["match"] == F:
        p["match"], p["nmatch"] = c.batch_match_results()
    if bp.ov_F["pose"] == F:
        p["pose_T"], p["pose_nin"], p["pose_outl"] = c.batch_pose_results()
    if bp.ov_F["track"] == F:
        p["trk_T"], p["trk_nin"], p["trk_nmap"], p["trk_nloc"], p["trk_lm"], p["trk_outl"] = c.batch_track_results()
    if bow:
        p["word"], p["node"] = c.batch_bow_results()
    assert all(p.values()), p
    return p


def shaped(raw, F, K):
    """Raw result bytes -> dict of arrays: (F, K) records per keypoint slot, (F,) per frame."""
    from coeb_front import KEYPOINT_DTYPE
    out = dict(F=F, K=K)
    for name, a in raw.items():
        a = np.array(a, copy=True).view(np.uint8)
        if name == "kps":
            out[name] = a.view(KEYPOINT_DTYPE).reshape(F, K)
        elif name == "desc":
            out[name] = a.reshape(F, K, 32)
        else:
            a = a.view(DTYPES.get(name, np.uint8))
            out[name] = a.reshape(F, 4, 4) if name.endswith("_T") else a.reshape(F, -1) if a.size != F else a
    return out


def serial_reference(bp, name, **step_kw):
    """One step on set `name` with set_batch_streams(1), synchronised before and after, and
    every result array as host copies (shaped())."""
    st = step(name, **step_kw)
    bp.ctx.set_batch_streams(1)
    bp.ctx.synchronize()
    F = enqueue(bp, st)
    bp.ctx.synchronize()
    ptr, size = device_arrays(bp, F, st["bow"]), array_sizes(bp, F, st["bow"])
    kw = st["kw"]
    made = [k for k in size                      # what this step produced, not what an earlier one left
            if (kw.get("match", True) or k not in ("match", "nmatch"))
            and (kw.get("pose") or kw.get("track") or not k.startswith("pose_"))
            and (kw.get("track") or not k.startswith("trk_"))]
    raw = {k: bp.ctx.download(ptr[k], size[k]) for k in made}
    return shaped(raw, F, bp.ctx.max_keypoints(W, H))


class Stepper:
    """Runs steps with no host synchronisation between them.  Behind every step flagged collect
    it enqueues coeb_memcpy_d2h_async of every result array into page-locked buffers of that
    step's own (allocated before the first step); that call joins the chunk and pose streams, so
    a collected step is fully ordered before the next.  Steps not collected overlap with their
    successor.  One synchronize() at the end."""

    def __init__(self, bp):
        self.bp = bp

    def run(self, steps):
        import ctypes as C
        from coeb_front import HostBuffer, lib
        bp = self.bp
        K = bp.ctx.max_keypoints(W, H)
        big = array_sizes_all(K, max((st["F"] or bp.ov_base_F) for st in steps))
        bufs = [{k: HostBuffer(n) for k, n in big.items()} if st["collect"] else None for st in steps]
        keep = (bp.gray, bp.depth, bp.dTcw, bp.Tcw, bp.F)
        for st in steps:                         # every upload (a synchronous copy) before the first step
            select(bp, st["name"], st["F"] or bp.ov_base_F)
        bp.gray, bp.depth, bp.dTcw, bp.Tcw, bp.F = keep
        got = []
        try:
            for st, hb in zip(steps, bufs):
                F = enqueue(bp, st)
                if hb is None:
                    got.append(None)
                    continue
                ptr, size = device_arrays(bp, F, st["bow"]), array_sizes(bp, F, st["bow"])
                for k, n in size.items():
                    bp.ctx.check(lib().coeb_memcpy_d2h_async(bp.ctx.h, C.c_void_p(hb[k].ptr), C.c_void_p(ptr[k]), n))
                got.append((F, size))
            bp.ctx.synchronize()
            return [None if g is None else shaped({k: hb[k].array[:n] for k, n in g[1].items()}, g[0], K)
                    for g, hb in zip(got, bufs)]
        finally:
            bp.ctx.synchronize()
            for hb in bufs:
                for b in (hb or {}).values():
                    b.free()


def array_sizes_all(K, F):
    return dict(kps=28 * K * F, desc=32 * K * F, counts=4 * F, match=4 * K * F, nmatch=4 * F, pose_T=64 * F, pose_nin=4 * F,
                pose_outl=K * F, trk_T=64 * F, trk_nin=4 * F, trk_nmap=4 * F, trk_nloc=4 * F, trk_lm=4 * K * F,
                trk_outl=K * F, word=4 * K * F, node=4 * K * F)


# ------------------------------------------------------------------ exact comparisons (slots below the frame's count)
def _rows_equal(a, b, counts, tag, first=0):
    for f in range(first, len(counts)):
        n = counts[f]
        assert a[f, :n].tobytes() == b[f, :n].tobytes(), (tag, f)


def assert_extract_equal(got, ref, tag=""):
    assert np.array_equal(got["counts"], ref["counts"]), (tag, "counts", got["counts"], ref["counts"])
    _rows_equal(got["kps"], ref["kps"], ref["counts"], (tag, "kps"))
    _rows_equal(got["desc"], ref["desc"], ref["counts"], (tag, "desc"))


def assert_match_equal(got, ref, tag=""):
    assert np.array_equal(got["nmatch"][1:], ref["nmatch"][1:]), (tag, "nmatch", got["nmatch"], ref["nmatch"])
    _rows_equal(got["match"], ref["match"], ref["counts"], (tag, "match"), 1)


def assert_pose_equal(got, ref, tag=""):
    assert got["pose_T"][1:].tobytes() == ref["pose_T"][1:].tobytes(), (tag, "pose_T")
    assert np.array_equal(got["pose_nin"][1:], ref["pose_nin"][1:]), (tag, "pose_nin")
    _rows_equal(got["pose_outl"], ref["pose_outl"], ref["counts"], (tag, "pose_outl"), 1)


def states(r):
    """The rule of BatchPipeline.track_results()."""
    return [None] + [0 if (r["nmatch"][f] < 20 or r["trk_nmap"][f] < 10) else (2 if r["trk_nin"][f] >= 30 else 1)
                     for f in range(1, r["F"])]


def assert_track_equal(got, ref, tag=""):
    """Every field of track_results(); the local-map search's outputs where the reference ran it
    (state != 0), as chain_util._check_chain compares them."""
    assert got["trk_T"][1:].tobytes() == ref["trk_T"][1:].tobytes(), (tag, "trk_T")
    for k in ("trk_nin", "trk_nmap"):
        assert np.array_equal(got[k][1:], ref[k][1:]), (tag, k, got[k], ref[k])
    st = states(ref)
    for f in range(1, ref["F"]):
        n = ref["counts"][f]
        assert got["trk_outl"][f, :n].tobytes() == ref["trk_outl"][f, :n].tobytes(), (tag, "trk_outl", f)
        if st[f]:
            assert got["trk_nloc"][f] == ref["trk_nloc"][f], (tag, "trk_nloc", f)
            assert got["trk_lm"][f, :n].tobytes() == ref["trk_lm"][f, :n].tobytes(), (tag, "trk_lm", f)


def assert_bow_equal(got, ref, tag=""):
    _rows_equal(got["word"], ref["word"], ref["counts"], (tag, "word"))
    _rows_equal(got["node"], ref["node"], ref["counts"], (tag, "node"))


def assert_step_equal(got, ref, tag=""):
    """Everything the reference step produced."""
    assert_extract_equal(got, ref, tag)
    if "match" in ref:
        assert_match_equal(got, ref, tag)
    if "pose_T" in ref:
        assert_pose_equal(got, ref, tag)
    if "trk_T" in ref:
        assert_track_equal(got, ref, tag)
    if "word" in ref:
        assert_bow_equal(got, ref, tag)


def records(r, frames=None):
    """A shaped() result as per-frame records for differs()."""
    st = states(r) if "trk_T" in r else None
    out = {}
    for f in (range(r["F"]) if frames is None else frames):
        n = r["counts"][f]
        rec = dict(kps=r["kps"][f, :n], desc=r["desc"][f, :n])
        if f and "match" in r:
            rec.update(match=r["match"][f, :n], nmatch=int(r["nmatch"][f]))
        if f and st:
            rec.update(state=st[f], T=r["trk_T"][f], local_match=r["trk_lm"][f, :n])
        out[f] = rec
    return out


def assert_oracle_frames(oracle_mod, ref, name, frames, tag=""):
    """The serial reference's frames against the oracle, so it is not only compared with itself."""
    from coeb_front import KEYPOINT_DTYPE
    for f in frames:
        o = oracle_record(oracle_mod, name, f)
        n = ref["counts"][f]
        assert n == len(o["kps"]), (tag, name, f, n, len(o["kps"]))
        for fld in KEYPOINT_DTYPE.names:
            assert np.array_equal(ref["kps"][f, :n][fld], o["kps"][fld]), (tag, name, f, fld)
        assert np.array_equal(ref["desc"][f, :n], o["desc"]), (tag, name, f)
        if f and "match" in ref:
            assert ref["nmatch"][f] == o["nmatch"] and np.array_equal(ref["match"][f, :n], o["match"]), (tag, name, f)
