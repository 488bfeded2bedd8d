"""Time of the RGB-D Frame constructor per frame on one MI355X: a 640x480 stream
(synth.moving_object_sequence, 55 frames, the object's box and a static one), 1000 features,
TUM1 distortion, a 16U depth map.
  * coeb_rgbd_stream_frame with the shadow stream, and with COEB_STREAM_NO_SHADOW
  * the composition it replaces: coeb_moving_object_points -> coeb_blur_flags -> coeb_frame_rgbd
  * coeb_match_lastframe (a 1000 x 1000 keypoint pair, twmm_time.make_scene) issued right after the
    stream call, for both forms: what the shadow kernels cost a following call.
The forms go through ctypes with every argument built beforehand and alternate within every round,
the profiler off.  A round is one pass over the sequence; the first 5 frames warm up, a wall figure
is the mean per call over the other 50; the line gives the median round and the range.  The stream
forms' T_M count and keypoint count are asserted equal to the composition's on every frame.

    python tools/rgbd_stream_time.py [--rounds 7] [--out FILE]
    python tools/rgbd_stream_time.py --composition-lib OTHER/libcoeb_front.so --out FILE   (the composition
        alone on another build of the library, e.g. the parent commit's; merged into FILE when it exists)"""
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

from twmm_time import make_scene, stat, vp     # noqa: E402

W, H, FRAMES, WARM = 640, 480, 55, 5
TUM1 = np.float32([0.262383, -0.953104, -0.005358, 0.002628, 1.163314])


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
        L.coeb_max_keypoints.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.coeb_moving_object_points.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t,
                                                C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p]
        L.coeb_blur_flags.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p]
        L.coeb_frame_rgbd.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t,
                                      C.c_int, C.c_float, C.POINTER(cf.Camera), C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        self.h = L.coeb_create(C.byref(cf.OrbParams(1000, 1.2, 8, 20, 7)), 0, W, H, 1)
        assert self.h, "coeb_create failed"
        self.cap = L.coeb_max_keypoints(self.h, W, H)

    def sync(self):
        assert self.L.coeb_synchronize(self.h) == 0

    def close(self):
        self.L.coeb_destroy(self.h)


def outputs(cap):
    import coeb_front as cf
    return dict(kp=np.empty(cap, cf.KEYPOINT_DTYPE), kun=np.empty(cap, cf.KEYPOINT_DTYPE), desc=np.empty((cap, 32), np.uint8),
                ur=np.empty(cap, np.float32), dep=np.empty(cap, np.float32), tm=np.empty((1024, 2), np.float32),
                blur=np.zeros(2, np.int32))


def composition(b, cam, frames, boxes, depth, scale):
    """-> run(f): the three calls for frame f >= 1 (frame 0: the extraction alone), and its (n_tm, n) log"""
    L, o = b.L, outputs(b.cap)
    nt, n = C.c_int(), C.c_int()
    log = {}

    def run(f):
        ntm = 0
        if f:
            assert L.coeb_moving_object_points(b.h, vp(frames[f - 1]), vp(frames[f]), W, H, W, vp(o["tm"]), 1024,
                                               C.byref(nt), None) == 0
            assert L.coeb_blur_flags(b.h, vp(frames[f]), W, H, W, vp(boxes[f]), 2, vp(o["blur"])) == 0
            ntm = max(nt.value, 0)
        else:
            o["blur"][:] = 0
        assert L.coeb_frame_rgbd(b.h, vp(frames[f]), W, H, W, vp(depth), depth.strides[0], 0, scale, C.byref(cam), vp(TUM1),
                                 vp(boxes[f]), 2, vp(o["tm"]) if ntm else None, ntm, vp(o["blur"]), 2, vp(o["kp"]),
                                 vp(o["kun"]), vp(o["desc"]), vp(o["ur"]), vp(o["dep"]), b.cap, C.byref(n)) == 0
        log[f] = (nt.value if f else 0, n.value)

    return run, log


def stream_form(ctx, st, cam, frames, boxes, depth, scale, after=None):
    import coeb_front as cf
    L, o = cf.lib(), outputs(ctx.max_keypoints(W, H))
    out = cf.RgbdStreamOutC(vp(o["tm"]), 1024, 0, vp(o["blur"]), None, 0, vp(o["kp"]), vp(o["kun"]), vp(o["desc"]),
                            vp(o["ur"]), vp(o["dep"]), ctx.max_keypoints(W, H), 0, 0)
    log = {}

    def run(f):
        if f == 0:
            assert L.coeb_rgbd_stream_reset(st.h) == 0
        assert L.coeb_rgbd_stream_frame(st.h, vp(frames[f]), W, 1, 1, W, H, vp(depth), depth.strides[0], 0, scale,
                                        C.byref(cam), vp(TUM1), vp(boxes[f]), 2, C.byref(out)) == 0
        log[f] = (out.n_tm, out.n)
        if after is not None:
            return after()
        return 0.0

    run.outputs = o         # `out` holds bare addresses: the arrays live as long as the function
    return run, log


def passes(sync, forms, rounds):
    """forms: run(f) functions; -> per form, the mean microseconds per call of frames WARM.. in every
    round but the first, and the same for the time run(f) itself reports (the following call)"""
    per = [[] for _ in forms]
    extra = [[] for _ in forms]
    for r in range(rounds + 1):
        for k, run in enumerate(forms):
            sync()
            tot = ext = 0.0
            for f in range(FRAMES):
                t0 = time.perf_counter()
                e = run(f) or 0.0
                dt = time.perf_counter() - t0 - e
                if f >= WARM:
                    tot += dt
                    ext += e
            if r:
                per[k].append(tot / (FRAMES - WARM) * 1e6)
                extra[k].append(ext / (FRAMES - WARM) * 1e6)
    return per, extra


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--composition-lib", default=None)
    a = ap.parse_args()
    import coeb_front as cf
    from coeb_front import synth
    import stream_ref as R

    frames, obj = synth.moving_object_sequence(W, H, FRAMES, seed=3, obj_shift=(-3, 2))
    boxes = [np.ascontiguousarray(np.stack([obj[f], np.float32([420, 60, 600, 200])])) for f in range(FRAMES)]
    depth = R.depth_map(W, H, "u16")
    scale = C.c_float(R.U16_SCALE)
    fx, fy, cx, cy = R.camera_params(W, H)
    cam = cf.make_camera(fx, fy, cx, cy, R.BF, W, H)
    res = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            res = json.loads(f.read())
    b = Binding(a.composition_lib or cf.LIB_PATH)
    run_c, log_c = composition(b, cam, frames, boxes, depth, scale)
    if a.composition_lib:
        per, _ = passes(b.sync, [run_c], a.rounds)
        res["wall_composition_other_build"] = dict(stat(per[0]), frames_per_round=FRAMES - WARM)
    else:
        ctx = cf.Context(max_width=W, max_height=H, max_batch=1)
        # the call that follows the constructor on a tracked frame
        cur, last, _, Tcw, Tcw_last = make_scene(0.0)
        mcam = cf.make_camera(synth.TUM_FX, synth.TUM_FY, synth.TUM_CX, synth.TUM_CY, synth.TUM_BF, W, H)
        n, nl = len(cur["kps"]), len(last["has_mp"])
        cc = cf.CurFrameC(n, vp(cur["kps"]), vp(cur["desc"]), vp(cur["ur"]))
        nobs = np.ascontiguousarray(last["mp_nobs"], np.int32)
        lc = cf.LastFrameC(nl, vp(last["has_mp"]), vp(last["outlier"]), vp(last["xw"]), vp(last["mp_desc"]), vp(nobs),
                           vp(last["keys_un"]))
        match, nm = np.zeros(n, np.int32), C.c_int()
        L = cf.lib()

        def after():
            t0 = time.perf_counter()
            assert L.coeb_match_lastframe(ctx.h, C.byref(mcam), C.byref(cc), C.byref(lc), vp(Tcw), vp(Tcw_last), 15.0, 0, 1,
                                          vp(match), C.byref(nm)) == 0
            return time.perf_counter() - t0

        st_s, st_n = cf.RGBDStream(ctx, shadow=True), cf.RGBDStream(ctx, shadow=False)
        st_sm, st_nm = cf.RGBDStream(ctx, shadow=True), cf.RGBDStream(ctx, shadow=False)
        forms = [stream_form(ctx, st_s, cam, frames, boxes, depth, scale), stream_form(ctx, st_n, cam, frames, boxes, depth, scale),
                 (run_c, log_c), stream_form(ctx, st_sm, cam, frames, boxes, depth, scale, after),
                 stream_form(ctx, st_nm, cam, frames, boxes, depth, scale, after)]

        def sync():
            ctx.synchronize()
            b.sync()

        per, extra = passes(sync, [f[0] for f in forms], a.rounds)
        for f in range(FRAMES):                     # the three forms computed the same frames
            assert forms[0][1][f] == forms[1][1][f] == log_c[f] == forms[3][1][f] == forms[4][1][f], f
        names = ["wall_stream_shadow", "wall_stream_no_shadow", "wall_composition", "wall_stream_shadow_before_match",
                 "wall_stream_no_shadow_before_match"]
        for k, nmk in enumerate(names):
            res[nmk] = dict(stat(per[k]), frames_per_round=FRAMES - WARM)
        res["wall_match_lastframe_after_shadow"] = stat(extra[3])
        res["wall_match_lastframe_after_no_shadow"] = stat(extra[4])
        res["sequence"] = dict(width=W, height=H, frames=FRAMES, warmup=WARM, boxes=2, nfeatures=1000,
                               mean_tm=float(np.mean([max(v[0], 0) for v in log_c.values()])),
                               mean_keypoints=float(np.mean([v[1] for v in log_c.values()])))
        for s in (st_s, st_n, st_sm, st_nm):
            s.close()
        ctx.close()
    b.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
