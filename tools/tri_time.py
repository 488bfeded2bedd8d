"""Time of SearchForTriangulation over the device keyframe database on one MI355X, on the scene of
tools/kfdb_time.py: an ORBvoc-shaped random vocabulary (k = 10, L = 6, nodes 4 levels up),
keyframes of 1000 features that are windows of one pool of scene descriptors (keyframe i holds
[10 i, 10 i + 1000)), half of the features with MapPoints, half stereo, image points shifted by a
few pixels between keyframes and F12 close to the line y2 = y1.
  * one coeb_kfdb_search_triangulation call for 10 neighbours against the same work as 10
    one-neighbour calls of the same build (wall time, profiler off, the two alternating in every
    round, both through the Python binding),
  * the device time of k_tri_match and k_tri_rot of each (the library's HIP-event profiler, in
    rounds of their own).
A wall figure is the mean per call of one round; the line gives the median round and the range
over the rounds, after a warm-up round.

    python tools/tri_time.py [--rounds 7] [--launches 20] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "coeb-slam_amd"))
import coeb_front as cf  # noqa: E402
from bow_time import full_tree, rounds  # noqa: E402
from kfdb_time import wall_rounds  # noqa: E402


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
    has_mp, nodes = [], []
    for i in range(nkf):
        s = slice(10 * i, 10 * i + n)
        d = pool[s].copy()
        for f in range(n):                                  # <= 12 flipped bits per keyframe
            for b in rng.choice(256, rng.randint(0, 13), replace=False):
                d[f, b >> 3] ^= 1 << (b & 7)
        node = ctx.bow_transform(d, 4)["node"]
        nodes.append(node)
        slot = db.add(d, node, ang[s], np.zeros(0, np.int32), np.zeros(0))
        keys = np.zeros(n, cf.KEYPOINT_DTYPE)
        keys["x"] = pool_xy[s, 0] + rng.uniform(-30, 30, n)
        keys["y"] = pool_xy[s, 1] + rng.choice([0.0, 0.5, 1.5, 3.0], n)
        keys["octave"] = rng.randint(0, 8, n)
        keys["angle"] = ang[s]
        db.set_geometry(slot, keys, np.where(rng.rand(n) < 0.5, keys["x"] - 4.0, -1.0))
        has_mp.append((rng.rand(n) < 0.5).astype(np.uint8))
    line_y = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
    F12 = np.array([line_y + rng.uniform(-1, 1, (3, 3)) * [[1e-5, 1e-5, 1e-3]] * 3 for _ in range(nnb)], np.float32)
    epi = np.stack([rng.uniform(100, 500, nnb), rng.uniform(100, 400, nnb)], 1).astype(np.float32)
    slots2 = list(range(1, nkf))

    def batched():
        return db.search_for_triangulation(0, has_mp[0], slots2, [has_mp[s] for s in slots2], F12, epi, False, False)

    def loop():
        return [db.search_for_triangulation(0, has_mp[0], [s], [has_mp[s]], F12[j:j + 1], epi[j:j + 1], False, False)
                for j, s in enumerate(slots2)]

    (got, nm), one = batched(), loop()
    assert all(np.array_equal(got[j], one[j][0][0]) and nm[j] == one[j][1][0] for j in range(nnb))
    res["nmatches"] = [int(x) for x in nm]
    res["nodes_keyframe1"] = int(len(set(nodes[0][nodes[0] >= 0].tolist())))
    w = wall_rounds(ctx, [batched, loop], a.rounds, a.launches)
    res["wall_one_call_10_neighbours"], res["wall_10_one_neighbour_calls"] = w
    res["wall_ratio_of_medians"] = w[1]["median_us"] / w[0]["median_us"]
    ctx.profile(True)
    res["kernels_one_call_10_neighbours"] = rounds(ctx, ["k_tri_match", "k_tri_rot"], batched, a.rounds, a.launches)
    res["kernels_10_one_neighbour_calls"] = rounds(ctx, ["k_tri_match", "k_tri_rot"], loop, a.rounds,
                                                   max(a.launches // 4, 2))
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
