"""Time of the single-frame TrackLocalMap on one MI355X: the 640x480 scene of tests/tlm_ref.py
(about 1000 keypoints, about 2000 local-map points, entry MapPoints on half the keypoints).
  * one coeb_track_local_map call (frustum, search, pose, inlier count; one synchronisation)
  * against the two calls it replaces on the same inputs, coeb_match_localmap then
    coeb_pose_optimization, with isInFrustum's fields and the merged mvpMapPoints both computed
    beforehand (the host isInFrustum loop and the host merge between the calls are left out of the
    timed part, which favours the two-call form).
Both forms go through ctypes with every argument built beforehand and alternate within every
round, the profiler off; a wall figure is the mean per call of one round, the line gives the
median round and the range, after a warm-up round.  The outputs of the two forms are asserted
equal.  The device times of the fused call's kernels come from the library's HIP-event profiler
in rounds of their own.

    python tools/tlm_time.py [--rounds 7] [--launches 20] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in ("coeb-slam_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(HERE, "..", p))
import coeb_front as cf  # noqa: E402
import tlm_ref as R  # noqa: E402
from bow_time import rounds  # noqa: E402
from kfdb_time import wall_rounds  # noqa: E402

KERNELS = ["k_frustum", "k_match_local", "k_lm_pose_prep", "k_pose", "k_lm_tail"]


def vp(a):
    return C.c_void_p(a.ctypes.data)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sc = R.scene(640, 480, n_distract=1000)
    want = R.reference(sc)
    n, nq = len(sc["kps"]), len(sc["pts"]["valid"])
    ctx = cf.Context(max_width=640, max_height=480, max_batch=1)
    L = cf.lib()
    cam, T0 = sc["cam"], np.ascontiguousarray(sc["Tcw"], np.float32)
    cur = cf.CurFrameC(n, vp(sc["kps"]), vp(sc["desc"]), vp(sc["ur"]))
    pts = {k: np.ascontiguousarray(sc["pts"][k]) for k in R.POINT_FIELDS}
    lp = cf.LocalPointsC(nq, *[vp(pts[k]) for k in R.POINT_FIELDS])
    # fused outputs
    f_fields = {k: np.zeros(nq, dt) for k, dt in R.FIELDS}
    f_tf = cf.TrackFieldsC(*[vp(f_fields[k]) for k, _ in R.FIELDS])
    f_match, f_outl, f_T = np.zeros(n, np.int32), np.zeros(n, np.uint8), T0.copy()
    f_cnt = [C.c_int() for _ in range(4)]

    def fused():
        f_T[:] = T0
        ctx.check(L.coeb_track_local_map(ctx.h, C.byref(cam), C.byref(cur), vp(sc["cur_obs"]), vp(sc["cur_xw"]), vp(f_T),
                                         C.byref(lp), R.COS_LIMIT, R.TH, R.NNRATIO, 0, C.byref(f_tf), vp(f_match),
                                         vp(f_outl), *[C.byref(c) for c in f_cnt]))

    # the two calls: isInFrustum's fields and the merged mvpMapPoints precomputed
    pre = {k: np.ascontiguousarray(want[k]) for k, _ in R.FIELDS}
    lm = cf.LocalMapC(nq, *[vp(pre[k]) for k, _ in R.FIELDS], vp(pts["descriptor"]), vp(pts["observations"]))
    t_match, t_nm = np.zeros(n, np.int32), C.c_int()
    has2, xw2 = np.ascontiguousarray(want["has2"]), np.ascontiguousarray(want["xw2"])
    pf = cf.PoseFrameC(n, vp(has2), vp(xw2), vp(sc["kps"]), vp(sc["ur"]))
    t_outl, t_T, t_nin = np.zeros(n, np.uint8), T0.copy(), C.c_int()

    def two_calls():
        t_T[:] = T0
        ctx.check(L.coeb_match_localmap(ctx.h, C.byref(cam), C.byref(cur), vp(sc["cur_obs"]), C.byref(lm), R.TH,
                                        R.NNRATIO, vp(t_match), C.byref(t_nm)))
        ctx.check(L.coeb_pose_optimization(ctx.h, C.byref(cam), C.byref(pf), vp(t_T), vp(t_outl), C.byref(t_nin)))

    fused()
    two_calls()
    # both forms give the reference's result, hence each other's
    for k, _ in R.FIELDS:
        assert np.array_equal(R.bits(f_fields[k]), R.bits(pre[k])), k
    assert np.array_equal(f_match, t_match) and np.array_equal(f_match, want["match"])
    assert f_cnt[1].value == t_nm.value == want["nlocal"] and f_cnt[0].value == want["n_to_match"]
    held = has2 > 0
    assert np.array_equal(R.bits(f_T), R.bits(t_T)) and np.array_equal(f_outl[held], t_outl[held])
    assert f_cnt[2].value == t_nin.value == want["ninliers_pose"] and f_cnt[3].value == want["nmatches_inliers"]
    res = dict(keypoints=n, local_points=nq, n_to_match=want["n_to_match"], nlocal=want["nlocal"],
               edges=int(held.sum()), ninliers_pose=want["ninliers_pose"], nmatches_inliers=want["nmatches_inliers"])
    w = wall_rounds(ctx, [fused, two_calls], a.rounds, a.launches)
    res["wall_track_local_map"], res["wall_match_localmap_plus_pose_optimization"] = w
    res["wall_ratio_of_medians"] = w[1]["median_us"] / w[0]["median_us"]
    res["fused_not_slower"] = bool(w[0]["median_us"] <= w[1]["median_us"])
    ctx.profile(True)
    res["kernels_track_local_map"] = rounds(ctx, KERNELS, fused, a.rounds, a.launches)
    res["kernels_two_calls"] = rounds(ctx, ["k_match_local", "k_pose"], two_calls, a.rounds, a.launches)
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
