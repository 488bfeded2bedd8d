"""Time of the device keyframe database on one MI355X: an ORBvoc-shaped random vocabulary (k = 10,
L = 6), a database of 2000 keyframes of 1000 features and a 1000-feature query frame.  Keyframe i
holds the descriptors [10 i, 10 i + 1000) of a pool of scene descriptors and the frame a window of
the same pool, so that neighbouring keyframes share most words, a couple of hundred keyframes
share some with the frame and the rest none -- the shape of a relocalisation query.
  * coeb_kfdb_query: device time of k_kfdb_common and k_kfdb_score (the library's HIP-event
    profiler, in rounds of their own) and the wall time of the whole call (profiler off),
  * SearchByBoW against 20 candidates of 1000 features: one coeb_match_bow_kfdb call against 20
    consecutive coeb_match_bow calls on the same inputs in the same process (wall time, profiler off,
    the two alternating in every round; both through the Python binding), and the kernels of each.
A wall figure is the mean per call of one round; the line gives the median round and the range
over the rounds, after a warm-up round.

    python tools/kfdb_time.py [--rounds 7] [--launches 20] [--keyframes 2000] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "coeb-slam_amd"))
import coeb_front as cf  # noqa: E402
from bow_time import full_tree, rounds  # noqa: E402


def stat(v):
    return dict(median_us=float(np.median(v)), min_us=float(min(v)), max_us=float(max(v)), rounds=len(v))


def wall_rounds(ctx, fns, nrounds, launches):
    """Mean wall time per call of each fn, the fns alternating within a round; every fn ends in a
    device synchronise of its own."""
    per = [[] for _ in fns]
    for r in range(nrounds + 1):
        for k, fn in enumerate(fns):
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(launches):
                fn()
            dt = time.perf_counter() - t0
            if r:
                per[k].append(dt / launches * 1e6)
    return [dict(stat(v), launches_per_round=launches) for v in per]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.RandomState(2)
    k, L, n, ncand = 10, 6, 1000, 20
    voc = cf.Vocabulary.from_arrays(k, L, *full_tree(k, L, rng))
    ctx = cf.Context(max_width=640, max_height=480, max_batch=1)
    ctx.set_vocabulary(voc)
    res = dict(vocabulary=dict(k=k, L=L, nodes=voc.info()[2], words=voc.info()[3]), keyframes=a.keyframes, features=n)
    voc.close()
    npool = 10 * a.keyframes + n
    pool = rng.randint(0, 256, (npool, 32)).astype(np.uint8)
    ang = rng.uniform(0, 359, npool).astype(np.float32)
    word, weight, node = (np.empty(npool, dt) for dt in (np.int32, np.float64, np.int32))
    for o in range(0, npool, 4000):
        r = ctx.bow_transform(pool[o:o + 4000], 4)
        word[o:o + 4000], weight[o:o + 4000], node[o:o + 4000] = r["word"], r["weight"], r["node"]
    db = cf.KeyFrameDatabase(ctx, max_features=n, initial_slots=a.keyframes)
    for i in range(a.keyframes):
        s = slice(10 * i, 10 * i + n)
        db.add(pool[s], node[s], ang[s], *cf.bow_vector(word[s], weight[s], node[s]))
    # the frame: the window of keyframe `at`, 30 % of it replaced, <= 20 flipped bits, one common rotation
    at = a.keyframes // 2
    s = slice(10 * at, 10 * at + n)
    cur = pool[s].copy()
    for i in range(n):
        for b in rng.choice(256, rng.randint(0, 21), replace=False):
            cur[i, b >> 3] ^= 1 << (b & 7)
    noise = rng.rand(n) < 0.3
    cur[noise] = rng.randint(0, 256, (int(noise.sum()), 32)).astype(np.uint8)
    keys = np.zeros(n, cf.KEYPOINT_DTYPE)
    keys["angle"] = np.mod(ang[s] - np.float32(40.0), 360)
    F = cf.Frame(keys, cur)
    F.ComputeBoW(ctx, 4)
    F.mBowVec = cf.bow_vector(F.mBowWord, F.mBowWeight, F.mFeatNode)
    q = db.query(*F.mBowVec)
    res["query"] = dict(query_words=int(len(F.mBowVec[0])), sharing=int(len(q["order"])), max_common=q["max_common"],
                        min_common=q["min_common"], scored=int((q["common"] > q["min_common"]).sum()))
    res["query"]["wall"] = wall_rounds(ctx, [lambda: db.query(*F.mBowVec)], a.rounds, a.launches)[0]
    # 20 candidates around the frame's window
    slots = [at - 10 + j for j in range(ncand)]
    valids = [(rng.rand(n) >= 0.3).astype(np.uint8) for _ in slots]
    bkf = [cf.BowKeyFrame(v, pool[10 * sl:10 * sl + n], node[10 * sl:10 * sl + n], ang[10 * sl:10 * sl + n])
           for sl, v in zip(slots, valids)]
    m = cf.ORBmatcher(0.75, True, ctx=ctx)

    def loop():
        out = []
        for kf in bkf:
            nm = m.SearchByBoW(kf, F)
            out.append((F.mvpMapPoints, nm))
        return out

    def batched():
        return db.SearchByBoW(slots, valids, F, 0.75, True)

    one, (got, nm) = loop(), batched()
    assert all(np.array_equal(got[j], one[j][0]) and nm[j] == one[j][1] for j in range(ncand))
    res["match_20x1000"] = dict(nmatches=[int(x) for x in nm])
    w = wall_rounds(ctx, [batched, loop], a.rounds, a.launches)
    res["match_20x1000"]["wall_one_kfdb_call"], res["match_20x1000"]["wall_20_match_bow_calls"] = w
    res["match_20x1000"]["wall_ratio_of_medians"] = w[1]["median_us"] / w[0]["median_us"]
    ctx.profile(True)
    res["query"]["kernels"] = rounds(ctx, ["k_kfdb_common", "k_kfdb_score"], lambda: db.query(*F.mBowVec), a.rounds,
                                     a.launches)
    res["match_20x1000"]["kernels_one_kfdb_call"] = rounds(ctx, ["k_bow_csr", "k_match_bow_db", "k_bow_rot_db"], batched,
                                                           a.rounds, a.launches)
    res["match_20x1000"]["kernels_per_match_bow_call"] = rounds(ctx, ["k_bow_csr", "k_match_bow", "k_bow_rot"], loop,
                                                                a.rounds, max(a.launches // 4, 2))
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
