"""Time of the single-frame TrackWithMotionModel on one MI355X: two extracted 640x480 frames
(about 1000 keypoints each), the last frame's MapPoints its own back-projections.
  * one coeb_track_motion_model call (search with the in-kernel retry, gate, pose, discard; one
    synchronisation), in SLAM mode and in localisation mode (a third of the last frame's slots
    emptied, so the visual-odometry step has points to create)
  * against the composition it replaces on the same inputs: coeb_match_lastframe, again with 2*th
    below 20 matches, the host gather of the matched positions, coeb_pose_optimization and the
    host discard loop (numpy, vectorised)
  * the same pair of forms on a scene whose prediction is off, so that the retry fires.
The forms go through ctypes with every argument built beforehand and alternate within every round,
the profiler off; a wall figure is the mean per call of one round, the line gives the median round
and the range, after a warm-up round.  The outputs of the two forms are asserted equal.  The device
times of the kernels come from the library's HIP-event profiler in rounds of their own.

    python tools/twmm_time.py [--rounds 7] [--launches 20] [--out FILE]
    python tools/twmm_time.py --composition-lib OTHER/libcoeb_front.so     (the composition alone, on
        another build of the library, e.g. the parent commit's, through a binding of its own)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in ("coeb-slam_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(HERE, "..", p))

TH, MIN_MATCHES, TH_DEPTH = 15.0, 20, 3.2
KERNELS = ["k_match_lists", "k_match", "k_trk_pose_prep", "k_pose", "k_mm_tail"]


def vp(a):
    return C.c_void_p(a.ctypes.data)


def stat(v):
    return dict(median_us=float(np.median(v)), min_us=float(min(v)), max_us=float(max(v)), rounds=len(v))


def wall_rounds(sync, fns, nrounds, launches):
    per = [[] for _ in fns]
    for r in range(nrounds + 1):
        for k, fn in enumerate(fns):
            sync()
            t0 = time.perf_counter()
            for _ in range(launches):
                fn()
            dt = time.perf_counter() - t0
            if r:
                per[k].append(dt / launches * 1e6)
    return [dict(stat(v), launches_per_round=launches) for v in per]


def make_scene(shift, keep_every=1):
    """(current frame arrays, last-frame arrays, depth of the last frame's keypoints, Tcw, Tcw_last).
    shift: the prediction is turned by that angle about y; keep_every: only every so many-th
    last-frame slot keeps its MapPoint."""
    import oracle as O
    from coeb_front import synth
    ex = O.Extractor()
    fr = synth.make_frames(640, 480, 2, seed=1000)
    r0, r1 = ex.extract(fr[0]), ex.extract(fr[1])
    depth = synth.make_depth(640, 480)
    intr = (synth.TUM_FX, synth.TUM_FY, synth.TUM_CX, synth.TUM_CY, synth.TUM_BF)
    last = O.mapframe_from_extraction(r0["kps"], r0["desc"], depth, *intr)
    _, ldep = O.stereo_from_rgbd(r0["kps"], depth, intr[4])
    last["has_mp"][np.arange(len(last["has_mp"])) % keep_every != 0] = 0
    ur, _ = O.stereo_from_rgbd(r1["kps"], depth, intr[4])
    T = synth.motion_pose().astype(np.float64)
    c, s = np.cos(shift), np.sin(shift)
    Ry = np.array([[c, 0, s, 0], [0, 1, 0, 0], [-s, 0, c, 0], [0, 0, 0, 1]])
    cur = dict(kps=np.ascontiguousarray(r1["kps"]), desc=np.ascontiguousarray(r1["desc"]), ur=np.ascontiguousarray(ur, np.float32))
    return cur, last, np.ascontiguousarray(ldep, np.float32), (Ry @ T).astype(np.float32), np.eye(4, dtype=np.float32)


class Binding:
    """The five entry points the composition needs, bound on any build of the library."""

    def __init__(self, path):
        import coeb_front as cf
        self.cf = cf
        L = self.L = C.CDLL(path)
        L.coeb_create.restype = C.c_void_p
        L.coeb_create.argtypes = [C.POINTER(cf.OrbParams), C.c_int, C.c_int, C.c_int, C.c_int]
        L.coeb_destroy.argtypes = [C.c_void_p]
        L.coeb_synchronize.argtypes = [C.c_void_p]
        L.coeb_match_lastframe.argtypes = [C.c_void_p, C.POINTER(cf.Camera), C.POINTER(cf.CurFrameC), C.POINTER(cf.LastFrameC),
                                           C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
        L.coeb_pose_optimization.argtypes = [C.c_void_p, C.POINTER(cf.Camera), C.POINTER(cf.PoseFrameC), C.c_void_p,
                                             C.c_void_p, C.POINTER(C.c_int)]
        self.h = L.coeb_create(C.byref(cf.OrbParams(1000, 1.2, 8, 20, 7)), 0, 640, 480, 1)
        assert self.h, "coeb_create failed"

    def sync(self):
        assert self.L.coeb_synchronize(self.h) == 0

    def close(self):
        self.L.coeb_destroy(self.h)


def composition(b, cam, cur, last, Tcw, Tcw_last):
    """-> (the function to time, its outputs dict (filled by every call))"""
    cf, L = b.cf, b.L
    n, nl = len(cur["kps"]), len(last["has_mp"])
    cc = cf.CurFrameC(n, vp(cur["kps"]), vp(cur["desc"]), vp(cur["ur"]))
    nobs = np.ascontiguousarray(last["mp_nobs"], np.int32)
    lc = cf.LastFrameC(nl, vp(last["has_mp"]), vp(last["outlier"]), vp(last["xw"]), vp(last["mp_desc"]), vp(nobs),
                       vp(last["keys_un"]))
    match, nm, nin = np.zeros(n, np.int32), C.c_int(), C.c_int()
    has, xw, outl, T = np.zeros(n, np.uint8), np.zeros((n, 3), np.float32), np.zeros(n, np.uint8), Tcw.copy()
    pf = cf.PoseFrameC(n, vp(has), vp(xw), vp(cur["kps"]), vp(cur["ur"]))
    out = {}

    def run():
        T[:] = Tcw
        assert L.coeb_match_lastframe(b.h, C.byref(cam), C.byref(cc), C.byref(lc), vp(T), vp(Tcw_last), TH, 0, 1, vp(match),
                                      C.byref(nm)) == 0
        searches = 1
        if nm.value < MIN_MATCHES:
            assert L.coeb_match_lastframe(b.h, C.byref(cam), C.byref(cc), C.byref(lc), vp(T), vp(Tcw_last), 2 * TH, 0, 1,
                                          vp(match), C.byref(nm)) == 0
            searches = 2
        out.update(nmatches_search=nm.value, searches=searches)
        if nm.value < MIN_MATCHES:
            out.update(match=match.copy(), discarded=np.full(n, -1, np.int32), ninliers_pose=0, nmatches=nm.value,
                       nmatches_map=0, Tcw=T.copy())
            return
        hit = match >= 0
        has[:] = hit                                    # the host gather
        xw[:] = last["xw"][np.maximum(match, 0)]
        outl[:] = 0
        assert L.coeb_pose_optimization(b.h, C.byref(cam), C.byref(pf), vp(T), vp(outl), C.byref(nin)) == 0
        bad = hit & (outl > 0)                          # the discard loop
        disc = np.where(bad, match, -1).astype(np.int32)
        kept = np.where(bad, -1, match).astype(np.int32)
        nmap = int((nobs[np.maximum(kept, 0)][kept >= 0] > 0).sum())
        out.update(match=kept, discarded=disc, ninliers_pose=nin.value, nmatches=nm.value - int(bad.sum()), nmatches_map=nmap,
                   Tcw=T.copy())

    return run, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--composition-lib", default=None)
    a = ap.parse_args()
    import coeb_front as cf
    from coeb_front import synth
    cam = cf.make_camera(synth.TUM_FX, synth.TUM_FY, synth.TUM_CX, synth.TUM_CY, synth.TUM_BF, 640, 480)
    # retry: a prediction 30 px off over a sparse last frame: the first search finds fewer than 20
    scenes = {"tracked": make_scene(0.0), "retry": make_scene(0.06, 20)}
    res = {}
    if a.composition_lib:
        b = Binding(a.composition_lib)
        for name, (cur, last, ldep, Tcw, Tl) in scenes.items():
            run, out = composition(b, cam, cur, last, Tcw, Tl)
            run()
            w = wall_rounds(b.sync, [run], a.rounds, a.launches)
            res[name] = dict(searches=out["searches"], nmatches_search=out["nmatches_search"], nmatches=out["nmatches"],
                             wall_composition_other_build=w[0])
        b.close()
    else:
        b = Binding(cf.LIB_PATH)
        ctx = cf.Context(max_width=640, max_height=480, max_batch=1)
        L = cf.lib()
        for name, (cur, last, ldep, Tcw, Tl) in scenes.items():
            n, nl = len(cur["kps"]), len(last["has_mp"])
            run_c, out_c = composition(b, cam, cur, last, Tcw, Tl)
            cc = cf.CurFrameC(n, vp(cur["kps"]), vp(cur["desc"]), vp(cur["ur"]))
            nobs = np.ascontiguousarray(last["mp_nobs"], np.int32)
            lc = cf.LastFrameC(nl, vp(last["has_mp"]), vp(last["outlier"]), vp(last["xw"]), vp(last["mp_desc"]), vp(nobs),
                               vp(last["keys_un"]))
            # localisation mode: a third of the slots hold no point before UpdateLastFrame
            has_vo = last["has_mp"].copy()
            has_vo[::3] = 0
            lv = cf.LastFrameC(nl, vp(has_vo), vp(last["outlier"]), vp(last["xw"]), vp(last["mp_desc"]), vp(nobs),
                               vp(last["keys_un"]))
            created, cpos = np.zeros(nl, np.uint8), np.zeros((nl, 3), np.float32)
            vo = cf.VoPointsC(vp(ldep), vp(last["mp_desc"]), TH_DEPTH, vp(created), vp(cpos))
            match, disc, outl, T = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8), Tcw.copy()
            cnt = [C.c_int() for _ in range(4)]

            def fused(lastc=lc, vop=None):
                T[:] = Tcw
                ctx.check(L.coeb_track_motion_model(ctx.h, C.byref(cam), C.byref(cc), C.byref(lastc), vop, vp(Tl), vp(T), TH, 0,
                                                    1, MIN_MATCHES, vp(match), vp(disc), vp(outl), *[C.byref(c) for c in cnt]))

            def fused_vo():
                fused(lv, C.byref(vo))

            fused()
            run_c()
            assert out_c["searches"] == (2 if name == "retry" else 1), out_c["searches"]
            assert np.array_equal(match, out_c["match"]) and np.array_equal(disc, out_c["discarded"])
            assert [c.value for c in cnt] == [out_c[k] for k in ("nmatches_search", "ninliers_pose", "nmatches", "nmatches_map")]
            assert np.array_equal(T.view(np.uint32), out_c["Tcw"].view(np.uint32))
            w = wall_rounds(ctx.synchronize, [fused, run_c, fused_vo], a.rounds, a.launches)
            r = dict(keypoints=n, last_keypoints=nl, searches=out_c["searches"], nmatches_search=out_c["nmatches_search"],
                     ninliers_pose=out_c["ninliers_pose"], nmatches=out_c["nmatches"], nmatches_map=out_c["nmatches_map"],
                     wall_track_motion_model=w[0], wall_composition=w[1], wall_track_motion_model_vo=w[2])
            fused_vo()
            r["created_vo"] = int(created.sum())
            r["fused_not_slower"] = bool(w[0]["median_us"] <= w[1]["median_us"])
            from bow_time import rounds
            ctx.profile(True)
            r["kernels_track_motion_model"] = rounds(ctx, KERNELS, fused, a.rounds, a.launches)
            r["kernels_track_motion_model_vo"] = rounds(ctx, ["k_vo_points"] + KERNELS, fused_vo, a.rounds, a.launches)
            ctx.profile(False)
            res[name] = r
        b.close()
        ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
