"""Time of the relocalisation refinement on one MI355X: a current frame of 1000 keypoints and a
KeyFrame of 1000 map points (the scenes of tests/reloc_ref.py), once with thresholds that take the
hypothesis through all three optimisations and both searches (stage 5) and once with the reference's,
which stop it after the first optimisation (stage 1); 1, 4 and 16 hypotheses per round (copies of
the one hypothesis, so every workgroup has the same work).
  * one coeb_reloc_refine call for the round (one upload, one synchronisation)
  * against the composition it replaces, hypothesis after hypothesis: coeb_pose_optimization up to
    three times and coeb_match_keyframe up to twice, with the entry, merge, discard and gate loops on
    the host (numpy, vectorised).
The forms go through ctypes with every argument built beforehand and alternate within every round,
the profiler off; a wall figure is the mean per call of one round, the line gives the median round
and the range, after a warm-up round.  The outputs of the two forms are asserted equal.  The device
times of the kernels come from the library's HIP-event profiler in rounds of their own.

    python tools/reloc_time.py [--rounds 7] [--launches 10] [--out FILE]
    python tools/reloc_time.py --composition-lib OTHER/libcoeb_front.so     (the composition alone, on
        another build of the library, e.g. the parent commit's, through a binding of its own)"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in ("coeb-slam_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(HERE, "..", p))

from twmm_time import stat, vp, wall_rounds     # noqa: E402

KERNELS = ["k_rr_enter", "k_pose", "k_rr_after1", "k_match_kf", "k_rr_merge", "k_rr_after2", "k_rr_tail"]
NHYP = (1, 4, 16)


class Binding:
    """The entry points the composition needs, bound on any build of the library."""

    def __init__(self, path):
        import coeb_front as cf
        self.cf = cf
        L = self.L = C.CDLL(path)
        L.coeb_create.restype = C.c_void_p
        L.coeb_create.argtypes = [C.POINTER(cf.OrbParams), C.c_int, C.c_int, C.c_int, C.c_int]
        L.coeb_destroy.argtypes = [C.c_void_p]
        L.coeb_synchronize.argtypes = [C.c_void_p]
        L.coeb_match_keyframe.argtypes = [C.c_void_p, C.POINTER(cf.Camera), C.POINTER(cf.CurFrameC), C.c_void_p,
                                          C.POINTER(cf.KeyFramePointsC), C.c_void_p, C.c_float, C.c_int, C.c_int, C.c_void_p,
                                          C.POINTER(C.c_int)]
        L.coeb_pose_optimization.argtypes = [C.c_void_p, C.POINTER(cf.Camera), C.POINTER(cf.PoseFrameC), C.c_void_p,
                                             C.c_void_p, C.POINTER(C.c_int)]
        self.h = L.coeb_create(C.byref(cf.OrbParams(1000, 1.2, 8, 20, 7)), 0, 640, 480, 1)
        assert self.h, "coeb_create failed"

    def sync(self):
        assert self.L.coeb_synchronize(self.h) == 0

    def close(self):
        self.L.coeb_destroy(self.h)


def composition(b, cam, fr, hyp, th, nhyp):
    """-> (the function to time: nhyp hypotheses one after the other, the last one's outputs)"""
    import reloc_ref as R
    cf, L = b.cf, b.L
    min_good, low_good, enough_good = th
    k = hyp["kf"]
    n, kn = len(fr["kps"]), len(k["valid"])
    cc = cf.CurFrameC(n, vp(fr["kps"]), vp(fr["desc"]), vp(fr["ur"]))
    valid = k["valid"].copy()
    kc = cf.KeyFramePointsC(kn, vp(valid), vp(k["world_pos"]), vp(k["descriptor"]), vp(k["max_distance"]),
                            vp(k["min_distance"]), vp(k["angle"]))
    mvp, has = np.zeros(n, np.int32), np.zeros(n, np.uint8)
    xw, outl, T = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8), np.zeros((4, 4), np.float32)
    smatch, nm, nin = np.zeros(n, np.int32), C.c_int(), C.c_int()
    pf = cf.PoseFrameC(n, vp(has), vp(xw), vp(fr["kps"]), vp(fr["ur"]))
    entry = np.where(hyp["inlier"] > 0, hyp["match"], -1).astype(np.int32)
    out = {}

    def optimise():
        has[:] = mvp >= 0                               # the host gather
        xw[:] = k["world_pos"][np.maximum(mvp, 0)]
        assert L.coeb_pose_optimization(b.h, C.byref(cam), C.byref(pf), vp(T), vp(outl), C.byref(nin)) == 0
        return nin.value

    def search(found, th_, orb_dist):
        valid[:] = k["valid"]
        valid[found] = 0
        has[:] = mvp >= 0
        assert L.coeb_match_keyframe(b.h, C.byref(cam), C.byref(cc), vp(has), C.byref(kc), vp(T), th_, orb_dist, 1, vp(smatch),
                                     C.byref(nm)) == 0
        hit = smatch >= 0
        mvp[hit] = smatch[hit]
        return nm.value

    def one():
        mvp[:] = entry
        outl[:] = 0
        T[:] = hyp["Tcw"]
        found = entry[entry >= 0]
        g = optimise()
        if g < min_good:
            return 0, g, 0, 0
        mvp[outl > 0] = -1
        if g >= enough_good:
            return 1, g, 0, 0
        a1 = search(found, R.TH1, R.ORB1)
        if a1 + g < enough_good:
            return 2, g, a1, 0
        g = optimise()
        if not (low_good < g < enough_good):
            return 3, g, a1, 0
        a2 = search(mvp[mvp >= 0], R.TH2, R.ORB2)
        if g + a2 < enough_good:
            return 4, g, a1, a2
        g = optimise()
        mvp[(outl > 0) & (mvp >= 0)] = -1
        return 5, g, a1, a2

    def run():
        for _ in range(nhyp):
            stage, g, a1, a2 = one()
        out.update(stage=stage, ngood=g, nadditional1=a1, nadditional2=a2, match=mvp.copy(), Tcw=T.copy())

    return run, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--composition-lib", default=None)
    a = ap.parse_args()
    import coeb_front as cf
    import reloc_ref as R
    cam = R.cameras()[1]
    fr, hyp = R.frame(1000), R.sized(1000, 1000)
    scenes = {"stage5": R.thresholds_for(fr, hyp), "stage1": (R.MIN_GOOD, R.LOW_GOOD, R.ENOUGH_GOOD)}
    res = {}
    b = Binding(a.composition_lib or cf.LIB_PATH)
    ctx = None if a.composition_lib else cf.Context(max_width=640, max_height=480, max_batch=1)
    for name, th in scenes.items():
        want = R.reference(fr, hyp, min_good=th[0], low_good=th[1], enough_good=th[2])
        assert want["stage"] == int(name[-1]), (name, want["stage"])
        for H in NHYP:
            run_c, out_c = composition(b, cam, fr, hyp, th, H)
            run_c()
            assert [out_c[k] for k in R.COUNTS] == [want[k] for k in R.COUNTS], (name, H)
            assert np.array_equal(out_c["match"], want["match"]) and np.array_equal(R.bits(out_c["Tcw"]), R.bits(want["Tcw"]))
            key = "%s_nhyp%d" % (name, H)
            if ctx is None:
                w = wall_rounds(b.sync, [run_c], a.rounds, a.launches)
                res[key] = dict(stage=want["stage"], ngood=want["ngood"], wall_composition_other_build=w[0])
                continue
            L = cf.lib()
            k, n = hyp["kf"], len(fr["kps"])
            cc = cf.CurFrameC(n, vp(fr["kps"]), vp(fr["desc"]), vp(fr["ur"]))
            hy = (cf.RelocHypothesisC * H)()
            T0 = np.ascontiguousarray(hyp["Tcw"], np.float32)
            for h in range(H):
                hy[h].kf = cf.KeyFramePointsC(len(k["valid"]), vp(k["valid"]), vp(k["world_pos"]), vp(k["descriptor"]),
                                              vp(k["max_distance"]), vp(k["min_distance"]), vp(k["angle"]))
                hy[h].match, hy[h].inlier = hyp["match"].ctypes.data, hyp["inlier"].ctypes.data
            match, outl = np.zeros((H, n), np.int32), np.zeros((H, n), np.uint8)
            cnt = {q: np.zeros(H, np.int32) for q in R.COUNTS}
            first = C.c_int()

            def fused():
                for h in range(H):
                    C.memmove(hy[h].Tcw, T0.ctypes.data, 64)
                ctx.check(L.coeb_reloc_refine(ctx.h, C.byref(cam), C.byref(cc), hy, H, R.TH1, R.ORB1, R.TH2, R.ORB2, 1, *th,
                                              vp(match), vp(outl), vp(cnt["ngood"]), vp(cnt["nadditional1"]),
                                              vp(cnt["nadditional2"]), vp(cnt["stage"]), C.byref(first)))

            fused()
            for h in range(H):
                assert [int(cnt[q][h]) for q in R.COUNTS] == [want[q] for q in R.COUNTS], (name, H, h)
                Th = np.ctypeslib.as_array(hy[h].Tcw).reshape(4, 4)
                assert np.array_equal(match[h], want["match"]) and np.array_equal(R.bits(Th.copy()), R.bits(want["Tcw"]))
            w = wall_rounds(ctx.synchronize, [fused, run_c], a.rounds, a.launches)
            r = dict(keypoints=len(fr["kps"]), keyframe_points=len(hyp["kf"]["valid"]), nhyp=H, thresholds=list(th),
                     stage=want["stage"], ngood=want["ngood"], nadditional1=want["nadditional1"],
                     nadditional2=want["nadditional2"], wall_reloc_refine=w[0], wall_composition=w[1],
                     composition_over_fused=w[1]["median_us"] / w[0]["median_us"])
            from bow_time import rounds
            ctx.profile(True)
            r["kernels_reloc_refine"] = rounds(ctx, KERNELS, fused, a.rounds, a.launches)
            ctx.profile(False)
            res[key] = r
    b.close()
    if ctx is not None:
        ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
