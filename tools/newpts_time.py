"""Time of coeb_kfdb_create_new_map_points on one MI355X, on the scene of tools/tri_time.py (10 neighbours of
1000 features, an ORBvoc-shaped random vocabulary, half of the features with MapPoints, half stereo, F12 close
to the line y2 = y1).  The views are the camera fx = fy = 500, cx = 320, cy = 240, mb = 0.08 at the identity and
moved along x by 0.2 (j + 1) for neighbour j, which is what those epipolar lines belong to; the image points of
a pair differ by up to 60 px along x, so the pairs spread over the ways out of the loop body (the status
histogram is part of the result) and most of them run the 4 x 4 Jacobi.
  (a) one coeb_kfdb_create_new_map_points call,
  (b) one coeb_kfdb_search_triangulation call (check_orientation = 0) of the same build on the same inputs,
      the two alternating in every round (wall time, profiler off, both through the Python binding), so the
      added cost of the loop body is one subtraction,
  the device time of k_tri_match and k_tri_points of (a) (the library's HIP-event profiler, rounds of its own).
  (c) (b) plus tools/newpts_host_loop.cpp on its pairs: a plain single-thread C++ loop of the same arithmetic
      without cv::Mat (compiled here with g++ -O2 -ffp-contract=off, loaded through ctypes), in the same
      rounds.  It allocates nothing and builds no cv::Mat temporaries, so it UNDERSTATES the reference's host
      cost; plain -O2 leaves std::fmaf a library call, which overstates the loop's own arithmetic.  Its status bytes, first_ok and x3D bits are compared with the device's (fields host_loop_*).
A wall figure is the mean per call of one round; the line gives the median round and the range over the
rounds, after a warm-up round.

    python tools/newpts_time.py [--rounds 7] [--launches 20] [--out FILE]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "coeb-slam_amd"))
import coeb_front as cf  # noqa: E402
from bow_time import full_tree, rounds  # noqa: E402
from kfdb_time import wall_rounds  # noqa: E402

FX, CX, CY, MB = 500.0, 320.0, 240.0, 0.08
HERE = os.path.dirname(os.path.abspath(__file__))


def host_loop_lib():
    so = os.path.join(tempfile.mkdtemp(prefix="newpts_host_loop_"), "newpts_host_loop.so")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", "-shared", "-fPIC",
                           os.path.join(HERE, "newpts_host_loop.cpp"), "-o", so])
    L = ctypes.CDLL(so)
    L.newpts_host_loop.restype = None
    L.newpts_host_loop.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                   ctypes.POINTER(ctypes.c_void_p)] + [ctypes.c_void_p] * 3 + [ctypes.c_float] + \
        [ctypes.c_void_p] * 3
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.RandomState(2)
    k, L, n, nnb = 10, 6, 1000, 10
    voc = cf.Vocabulary.from_arrays(k, L, *full_tree(k, L, rng))
    ctx = cf.Context(max_width=640, max_height=480, max_batch=1)
    ctx.set_vocabulary(voc)
    res = dict(vocabulary=dict(k=k, L=L, nodes=voc.info()[2], words=voc.info()[3]), features=n, neighbours=nnb)
    voc.close()
    nkf = nnb + 1
    npool = 10 * nkf + n
    pool = rng.randint(0, 256, (npool, 32)).astype(np.uint8)
    pool_xy = np.stack([rng.uniform(20, 620, npool), rng.uniform(20, 460, npool)], 1)
    ang = rng.uniform(0, 359, npool).astype(np.float32)
    db = cf.KeyFrameDatabase(ctx, max_features=n, initial_slots=nkf)
    has_mp, views, feats, octs = [], [], [], []
    for i in range(nkf):
        s = slice(10 * i, 10 * i + n)
        d = pool[s].copy()
        for f in range(n):                                  # <= 12 flipped bits per keyframe
            for b in rng.choice(256, rng.randint(0, 13), replace=False):
                d[f, b >> 3] ^= 1 << (b & 7)
        slot = db.add(d, ctx.bow_transform(d, 4)["node"], ang[s], np.zeros(0, np.int32), np.zeros(0))
        keys = np.zeros(n, cf.KEYPOINT_DTYPE)
        keys["x"] = pool_xy[s, 0] + rng.uniform(-30, 30, n)
        keys["y"] = pool_xy[s, 1] + rng.choice([0.0, 0.5, 1.5, 3.0], n)
        keys["octave"] = rng.randint(0, 8, n)
        keys["angle"] = ang[s]
        stereo = rng.rand(n) < 0.5
        depth = rng.uniform(1.0, 12.0, n)
        ur, dp = np.where(stereo, keys["x"] - FX * MB / depth, -1.0), np.where(stereo, depth, -1.0)
        db.set_geometry(slot, keys, ur)
        db.set_stereo(slot, np.stack([keys["x"], keys["y"]], 1), dp)
        feats.append(np.ascontiguousarray(np.stack([keys["x"], keys["y"], ur, keys["x"], keys["y"], dp], 1), np.float32))
        octs.append(np.ascontiguousarray(keys["octave"], np.int32))
        has_mp.append((rng.rand(n) < 0.5).astype(np.uint8))
        b = 0.2 * i
        views.append(cf.kf_view(np.eye(3), (-b, 0, 0), (b, 0, 0), FX, FX, CX, CY, 1 / FX, 1 / FX, MB, FX * MB))
    line_y = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
    F12 = np.array([line_y + rng.uniform(-1, 1, (3, 3)) * [[1e-5, 1e-5, 1e-3]] * 3 for _ in range(nnb)], np.float32)
    epi = np.stack([rng.uniform(100, 500, nnb), rng.uniform(100, 400, nnb)], 1).astype(np.float32)
    slots2 = list(range(1, nkf))
    v2 = np.array(views[1:])

    def new_points():
        return db.create_new_map_points(0, views[0], has_mp[0], slots2, v2, [has_mp[s] for s in slots2], F12, epi, False)

    def search():
        return db.search_for_triangulation(0, has_mp[0], slots2, [has_mp[s] for s in slots2], F12, epi, False, False)

    L = host_loop_lib()
    t = ctx.tables()
    scale, sigma2 = np.array(t.scale[:8], np.float32), np.array(t.sigma2[:8], np.float32)
    vall = np.ascontiguousarray(np.concatenate([np.array([views[0]]), v2]))
    fp = (ctypes.c_void_p * nkf)(*[f.ctypes.data for f in feats])
    op = (ctypes.c_void_p * nkf)(*[o.ctypes.data for o in octs])
    h_status, h_x3d, h_first = np.zeros((nnb, n), np.int8), np.zeros((nnb, n, 3), np.float32), np.zeros(n, np.int32)
    ratio_factor = float(np.float32(1.5) * np.float32(t.scale_factor))

    def search_and_host_loop():
        mm, _ = search()
        L.newpts_host_loop(vall.ctypes.data, nnb, n, fp, op, mm.ctypes.data, scale.ctypes.data, sigma2.ctypes.data,
                           ratio_factor, h_status.ctypes.data, h_x3d.ctypes.data, h_first.ctypes.data)

    got, (m, nm) = new_points(), search()
    search_and_host_loop()
    acc = got["status"] == 1
    res["host_loop_status_equal"] = bool(np.array_equal(h_status & 15, got["status"]) and
                                         np.array_equal((h_status >> 4) & 3, got["source"]))
    res["host_loop_first_ok_equal"] = bool(np.array_equal(h_first, got["first_ok"]))
    res["host_loop_x3d_bits_equal"] = bool(np.array_equal(h_x3d[acc].view(np.uint32), got["x3d"][acc].view(np.uint32)))
    assert np.array_equal(got["match"], m) and np.array_equal(got["nmatches"], nm)
    res["nmatches"] = [int(x) for x in nm]
    res["status_histogram"] = np.bincount(got["status"].ravel(), minlength=10).tolist()
    res["source_histogram"] = np.bincount(got["source"].ravel(), minlength=4).tolist()
    res["map_points"] = int((got["first_ok"] >= 0).sum())
    w = wall_rounds(ctx, [new_points, search, search_and_host_loop], a.rounds, a.launches)
    res["wall_a_create_new_map_points"], res["wall_b_search_triangulation"], res["wall_c_search_plus_host_loop"] = w
    res["wall_a_minus_b_median_us"] = w[0]["median_us"] - w[1]["median_us"]
    res["wall_c_minus_b_median_us"] = w[2]["median_us"] - w[1]["median_us"]
    res["a_beats_c"] = bool(w[0]["median_us"] < w[2]["median_us"])
    ctx.profile(True)
    res["kernels_a"] = rounds(ctx, ["k_tri_match", "k_tri_points"], new_points, a.rounds, a.launches)
    db.close()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
