"""Device time of the bag-of-words kernels on one MI355X, from the library's HIP-event profiler
(coeb_profile_*): an ORBvoc-shaped random vocabulary (k = 10, L = 6, a full tree of 1 111 110 nodes,
35.6 MB of descriptors) and
  * k_bow_transform for 1000 descriptors (coeb_bow_transform, single frame),
  * k_bow_transform over a 1024-frame 640 x 480 batch (coeb_bow_batch_device),
  * coeb_match_bow at 1000 x 1000 (k_bow_csr + k_match_bow + k_bow_rot).
Each figure is the mean per launch of one round of launches; the line gives the median round and
the range over the rounds, after a warm-up round.  Random descriptors walk the tree evenly, so
the single-frame transform is the cold-cache case: 1000 walks touch ~60 k of the 1.1 M nodes.

    python tools/bow_time.py [--rounds 7] [--launches 20] [--frames 1024] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "coeb-slam_amd"))
import coeb_front as cf  # noqa: E402
from coeb_front import synth  # noqa: E402


def full_tree(k, L, rng):
    """Lines of a full k-ary tree in ORBvoc.txt's order: level by level, node ids from 1."""
    starts = np.cumsum([1] + [k ** lvl for lvl in range(1, L)])      # id of the first node of level 1, 2, ..
    parent, leaf = [], []
    for lvl in range(1, L + 1):
        n = k ** lvl
        parent.append(np.zeros(n, np.int64) if lvl == 1 else starts[lvl - 2] + np.arange(n) // k)
        leaf.append(np.full(n, lvl == L, np.uint8))
    parent, leaf = np.concatenate(parent).astype(np.int32), np.concatenate(leaf)
    desc = rng.randint(0, 256, (len(parent), 32)).astype(np.uint8)
    weight = np.where(leaf > 0, rng.uniform(0.1, 5.0, len(parent)), 0.0)
    return parent, leaf, desc, weight


def rounds(ctx, names, fn, nrounds, launches):
    per = {n: [] for n in names}
    for r in range(nrounds + 1):
        ctx.profile_reset()
        for _ in range(launches):
            fn()
        ctx.synchronize()
        got = ctx.profile_read()
        if r == 0:
            continue                          # warm-up round
        for n in names:
            ms, cnt = got[n]
            per[n].append(ms / cnt * 1e3)
    return {n: dict(median_us=float(np.median(v)), min_us=float(min(v)), max_us=float(max(v)), rounds=len(v),
                    launches_per_round=launches) for n, v in per.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.RandomState(1)
    k, L = 10, 6
    voc = cf.Vocabulary.from_arrays(k, L, *full_tree(k, L, rng))
    ctx = cf.Context(max_width=640, max_height=480, max_batch=a.frames)
    ctx.set_vocabulary(voc)
    res = dict(vocabulary=dict(k=k, L=L, nodes=voc.info()[2], words=voc.info()[3]))
    voc.close()
    ctx.profile(True)
    desc = rng.randint(0, 256, (1000, 32)).astype(np.uint8)
    res["single_frame_1000"] = rounds(ctx, ["k_bow_transform", "k_bow_csr"], lambda: ctx.bow_transform(desc, 4),
                                      a.rounds, a.launches)
    # SearchByBoW 1000 x 1000: the frame is the KeyFrame permuted with <= 20 flipped bits
    kf_node = ctx.bow_transform(desc, 4)["node"]
    perm = rng.permutation(1000)
    cur = desc[perm].copy()
    for i in range(1000):
        for b in rng.choice(256, rng.randint(0, 21), replace=False):
            cur[i, b >> 3] ^= 1 << (b & 7)
    keys = np.zeros(1000, cf.KEYPOINT_DTYPE)
    ang = rng.uniform(0, 359, 1000).astype(np.float32)
    keys["angle"] = ang[perm]
    F = cf.Frame(keys, cur)
    F.ComputeBoW(ctx, 4)
    kf = cf.BowKeyFrame(np.ones(1000, np.uint8), desc, kf_node, ang)
    m = cf.ORBmatcher(0.7, True, ctx=ctx)
    nm = m.SearchByBoW(kf, F)
    res["match_bow_1000x1000"] = rounds(ctx, ["k_bow_csr", "k_match_bow", "k_bow_rot"], lambda: m.SearchByBoW(kf, F),
                                        a.rounds, a.launches)
    res["match_bow_1000x1000"]["nmatches"] = nm
    res["match_bow_1000x1000"]["common_nodes"] = int(len(np.intersect1d(kf_node[kf_node >= 0], F.mFeatNode[F.mFeatNode >= 0])))
    # the batch: 8 distinct frames repeated
    base = np.stack(synth.make_frames(640, 480, 8, seed=1000))
    frames = np.tile(base, (a.frames // 8 + 1, 1, 1))[:a.frames]
    dg = ctx.upload(frames)
    ctx.extract_batch_device(dg.ptr, a.frames, 640, 480)
    ctx.synchronize()
    counts = ctx.download(ctx.batch_results()[2], 4 * a.frames, np.int32)
    res["batch"] = rounds(ctx, ["k_bow_transform"], lambda: ctx.bow_batch_device(4), a.rounds, max(a.launches // 4, 2))
    res["batch"]["frames"] = a.frames
    res["batch"]["descriptors"] = int(counts.sum())
    dg.free()
    ctx.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
