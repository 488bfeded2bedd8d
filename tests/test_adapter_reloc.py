"""The Relocalization drop-in adapter (adapter/Tracking_coeb.h) run by the shim program
(tests/adapter_shim/reloc_exec.cpp) over Frame / KeyFrame / MapPoint types and a scripted solver
type that returns canned poses and inlier sets: the frame's mvpMapPoints, mvbOutlier and mTcw, the
return value, vbDiscarded / nCandidates and the number of iterate calls per candidate must be what
the reference's loop (src/Tracking.cc:1477-1568) over the CPU composition (tests/reloc_ref.py) says."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import reloc_ref as R
from conftest import ROOT

SHIM = os.path.join(ROOT, "tests", "adapter_shim")
INCLUDES = ["-I", SHIM, "-I", os.path.join(ROOT, "coeb-slam_amd", "adapter"), "-I", os.path.join(ROOT, "include")]


def few_inliers(hyp, keep=5):
    """hyp with all but `keep` of its inliers dropped: the first optimisation cannot reach 10."""
    out = dict(hyp)
    inl = hyp["inlier"].copy()
    inl[np.flatnonzero(inl)[keep:]] = 0
    out["inlier"] = inl
    return out


def scripts():
    """name -> (candidate base scenes, per candidate the iterate results (bNoMore, hypothesis or None)).
    wins:  two rounds; candidate 1 reaches max iterations without a pose, candidate 3 with one; the
           winner is candidate 2, in the second round, behind a candidate that fails again.
    fails: every candidate runs out of iterations; the frame keeps the last hypothesis refined."""
    few, short, rich, thin = (R.base(n)[1] for n in ("few", "short", "rich", "thin"))
    return dict(
        wins=((few, short, rich, thin),
              ([(0, few), (0, few)], [(1, None)], [(0, few_inliers(rich)), (0, rich)], [(1, thin)])),
        fails=((few, thin), ([(0, few), (1, few_inliers(few, 3))], [(0, thin), (1, None)])))


def reference_loop(fr, cands, script):
    """Tracking.cc:1477-1568 over reloc_ref.reference, every live candidate of a round iterating (as
    the adapter runs it).  -> (ret, state of the frame: candidate, hypothesis, reference result, mvbOutlier;
    calls, discarded, nCandidates).  mvbOutlier starts all true and takes the flags of the hypothesis a
    round leaves in the frame (its winner, else its last) where an optimisation saw a point: elsewhere
    it is stale, as in the reference, whose stale flags are those of every hypothesis in turn."""
    K = len(cands)
    discarded, calls, n_cand = [False] * K, [0] * K, K
    state = None
    outl = np.ones(len(fr["kps"]), np.uint8)
    while n_cand > 0:
        round_ = []
        for i in range(K):
            if discarded[i]:
                continue
            no_more, hyp = script[i][calls[i]]
            calls[i] += 1
            if no_more:
                discarded[i] = True
                n_cand -= 1
            if hyp is not None:
                round_.append((i, hyp))
        for i, hyp in round_:
            state = (i, hyp, R.reference(fr, hyp), outl)
            if state[2]["ngood"] >= R.ENOUGH_GOOD:
                break
        if round_:
            ref = state[2]
            outl[ref["written"]] = ref["outlier"][ref["written"]]
            if ref["ngood"] >= R.ENOUGH_GOOD:
                return True, state, calls, discarded, n_cand
    return False, state, calls, discarded, n_cand


def test_scripts_have_what_they_are_for():
    fr = R.frame(300)
    cands, script = scripts()["wins"]
    ret, (who, hyp, ref, outl), calls, disc, n_cand = reference_loop(fr, cands, script)
    assert ret and who == 2 and calls == [2, 1, 2, 1] and disc == [False, True, False, True] and n_cand == 2
    assert R.reference(fr, script[2][0][1])["stage"] == 0 and ref["stage"] == 1
    cands, script = scripts()["fails"]
    ret, (who, hyp, ref, outl), calls, disc, n_cand = reference_loop(fr, cands, script)
    assert not ret and who == 0 and calls == [2, 2] and disc == [True, True] and n_cand == 0 and ref["stage"] == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_reloc_adapter_compiles():
    cmd = ["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Werror"] + INCLUDES + [os.path.join(SHIM, "reloc_exec.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["wins", "fails"])
def test_reloc_adapter_runs_against_library(tmp_path, name):
    lib_dir = os.path.join(ROOT, "coeb-slam_amd", "lib")
    exe = str(tmp_path / "reloc_exec")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Werror"] + INCLUDES + [
        os.path.join(SHIM, "reloc_exec.cpp"), "-o", exe, "-L", lib_dir, "-lcoeb_front", "-Wl,-rpath," + lib_dir,
        "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    fr = R.frame(300)
    cands, script = scripts()[name]
    n = len(fr["kps"])
    cam = np.array(list(R.INTR) + [0.0, float(R.W), 0.0, float(R.H)], np.float32)
    files = [("cam.f32", cam), ("kps.bin", fr["kps"]), ("desc.u8", fr["desc"]), ("ur.f32", fr["ur"]),
             ("ncand.i32", np.array([len(cands)], np.int32))]
    for c, (hyp, calls) in enumerate(zip(cands, script)):
        k = hyp["kf"]
        # a slot that is not valid is NULL or a bad point; a matched point the KeyFrame no longer holds goes through too
        valid = np.where(k["valid"] > 0, 1, np.where(np.arange(len(k["valid"])) % 2, 2, 0)).astype(np.uint8)
        files += [("kf%d_valid.u8" % c, valid), ("kf%d_xw.f32" % c, k["world_pos"]), ("kf%d_desc.u8" % c, k["descriptor"]),
                  ("kf%d_maxd.f32" % c, k["max_distance"]), ("kf%d_mind.f32" % c, k["min_distance"]),
                  ("kf%d_angle.f32" % c, k["angle"]), ("m%d.i32" % c, hyp["match"]),
                  ("s%d_flags.i32" % c, np.array([[nm, h is not None] for nm, h in calls], np.int32)),
                  ("s%d_T.f32" % c, np.array([np.eye(4) if h is None else h["Tcw"] for _, h in calls], np.float32)),
                  ("s%d_inl.u8" % c, np.array([np.zeros(n) if h is None else h["inlier"] for _, h in calls], np.uint8))]
    for fname, a in files:
        np.ascontiguousarray(a).tofile(str(tmp_path / fname))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr

    def got(fname, dt):
        return np.fromfile(str(tmp_path / fname), dt)

    ret, (who, hyp, ref, outl), calls, disc, n_cand = reference_loop(fr, cands, script)
    assert list(got("ret.i32", np.int32)) == [int(ret), n_cand]
    assert list(got("calls.i32", np.int32)) == calls and list(got("discarded.u8", np.uint8)) == [int(x) for x in disc]
    assert np.array_equal(got("mvp.i32", np.int32), ref["match"])
    assert np.array_equal(got("mvp_kf.i32", np.int32), np.where(ref["match"] >= 0, who, -1))
    assert np.array_equal(got("outl.u8", np.uint8), outl)
    assert np.array_equal(outl[ref["written"]], ref["outlier"][ref["written"]])
    assert np.array_equal(got("T_out.f32", np.uint32), R.bits(ref["Tcw"]).ravel())
