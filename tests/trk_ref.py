"""Tracking::TrackReferenceKeyFrame on one frame as the CPU references compose it (no GPU):
Frame::ComputeBoW (bow_ref.compute_bow), ORBmatcher::SearchByBoW (bow_ref.search_by_bow),
Optimizer::PoseOptimization (oracle.pose_optimization) and the discard loop of
src/Tracking.cc:843-862 written out literally.  Plus the scenes the TrackReferenceKeyFrame tests
share: no images, only points in front of a camera, their projections and their descriptors."""
import functools

import numpy as np

import bow_ref as B
import coeb_front as cf
import oracle as O

NNRATIO, MIN_MATCHES = 0.7, 15                      # ORBmatcher matcher(0.7, true), `if (nmatches < 15)`
W, H = 640, 480
INTR = (517.3, 516.5, 318.6, 255.3, 40.0)           # fx, fy, cx, cy, bf
# frame x KeyFrame sizes of the GPU test; MAIN is the scene the preconditions are asserted on
MAIN = (300, 300)
SIZES = ((0, 0), (0, 5), (5, 0), (1, 1), (63, 65), (64, 64), (65, 63), MAIN, (4095, 4095))


@functools.lru_cache(maxsize=None)
def extractor():
    return O.Extractor()


@functools.lru_cache(maxsize=None)
def voc_case(name):
    """-> (the vocabulary's arrays, bow_ref.Voc, levelsup)"""
    if name == "k3_ragged":                         # ragged, words of weight 0: node id -1 occurs
        args = B.random_voc(3, 6, seed=8, ragged=True, zero_weight=0.1)
        return args, B.Voc(*args), 4
    if name == "k10":
        args = B.random_voc(10, 3, seed=5)
        return args, B.Voc(*args), 2
    if name == "hand":                              # tests/test_trk_ref.py works it through
        d = lambda b: [b] * 32
        args = (2, 2, [0, 0, 1, 1, 2, 2], [0, 0, 1, 1, 1, 1],
                np.array([d(0x00), d(0xFF), d(0x00), d(0x0F), d(0xFF), d(0xF0)], np.uint8), [0.0, 0.0, 1.0, 0.0, 2.0, 3.0])
        return args, B.Voc(*args), 1
    raise KeyError(name)


def pose(rx, ry, rz, t):
    """Tcw (float32 4x4) of a rotation by the three small angles and the translation t."""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T.astype(np.float32)


def project(T, xw):
    """Pixel position and depth of world points under Tcw (float64)."""
    Pc = np.asarray(xw, np.float64) @ T[:3, :3].astype(np.float64).T + T[:3, 3].astype(np.float64)
    fx, fy, cx, cy, _ = INTR
    return fx * Pc[:, 0] / Pc[:, 2] + cx, fy * Pc[:, 1] / Pc[:, 2] + cy, Pc[:, 2]


def assemble(voc_name, kf, kps, desc, ur, Tcw):
    """A scene dict from its arrays; the KeyFrame's node ids are its own ComputeBoW's, and "bow" is
    the frame's (computed once: the references of a scene share it)."""
    args, voc, levelsup = voc_case(voc_name)
    kf = dict(kf)
    kf["desc"] = np.ascontiguousarray(kf["desc"], np.uint8).reshape(-1, 32)
    kf["node"] = B.compute_bow(voc, kf["desc"], levelsup)["node"]
    ex = extractor()
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    return dict(voc_name=voc_name, voc_args=args, voc=voc, levelsup=levelsup, kf=kf, kps=np.ascontiguousarray(kps),
                desc=desc, bow=B.compute_bow(voc, desc, levelsup), ur=np.ascontiguousarray(ur, np.float32),
                Tcw=np.ascontiguousarray(Tcw, np.float32), intr=INTR,
                isg=np.array(list(ex.p.inv_sigma2), np.float32), cam=cf.make_camera(*INTR, W, H))


@functools.lru_cache(maxsize=None)
def scene(n_cur, n_kf, seed=3, voc_name="k3_ragged", shared=0.8, invalid=0.1, displaced=0.1, mono=0.3, odd_angle=0.08):
    """n_kf KeyFrame features with MapPoints in front of the camera; the frame sees `shared` of
    min(n_cur, n_kf) of them (descriptors with 0..6 bits flipped, angles turned by a common 40
    degrees, `odd_angle` of them by something else), the rest of its keypoints are distractors.
    `displaced` of the KeyFrame's positions are off by decimetres: the optimiser flags them."""
    rng = np.random.default_rng(1000 * seed + 7 * n_cur + n_kf)
    fx, fy, cx, cy, bf = INTR
    xw = np.stack([rng.uniform(-1.6, 1.6, n_kf), rng.uniform(-1.2, 1.2, n_kf), rng.uniform(2.0, 6.0, n_kf)], 1)
    xw = xw.astype(np.float32).reshape(n_kf, 3)
    kf_desc = rng.integers(0, 256, (n_kf, 32)).astype(np.uint8)
    kf_angle = rng.uniform(0.0, 360.0, n_kf).astype(np.float32)
    T_true = pose(0.01, -0.015, 0.02, (0.03, -0.02, 0.05))
    m = int(round(shared * min(n_cur, n_kf))) if min(n_cur, n_kf) > 2 else min(n_cur, n_kf)
    src = rng.permutation(n_kf)[:m]                 # the KeyFrame feature each shared keypoint shows
    u, v, z = project(T_true, xw[src])
    u = u + rng.normal(0, 0.4, m)
    v = v + rng.normal(0, 0.4, m)
    nd = n_cur - m
    kps = np.zeros(n_cur, cf.KEYPOINT_DTYPE)
    kps["x"] = np.concatenate([u, rng.uniform(20, W - 20, nd)])
    kps["y"] = np.concatenate([v, rng.uniform(20, H - 20, nd)])
    kps["size"], kps["response"], kps["class_id"] = 31.0, 50.0, -1
    kps["octave"] = rng.integers(0, 8, n_cur)
    turn = np.where(rng.random(m) < odd_angle, rng.uniform(60.0, 330.0, m), 40.0 + rng.normal(0, 2.0, m))
    kps["angle"] = np.concatenate([np.mod(kf_angle[src].astype(np.float64) - turn, 360.0), rng.uniform(0, 360, nd)])
    zz = np.concatenate([z, rng.uniform(2.0, 6.0, nd)])
    ur = (kps["x"].astype(np.float64) - bf / zz).astype(np.float32)
    ur[rng.random(n_cur) < mono] = -1.0
    desc = np.concatenate([kf_desc[src], rng.integers(0, 256, (nd, 32)).astype(np.uint8)])
    for i in range(m):
        for b in rng.integers(0, 256, int(rng.integers(0, 7))):
            desc[i, b >> 3] ^= np.uint8(1 << (b & 7))
    order = rng.permutation(n_cur)
    kps, ur, desc = kps[order], ur[order], desc[order]
    bad = rng.random(n_kf) < displaced
    xw[bad] += rng.normal(0, 0.3, (int(bad.sum()), 3)).astype(np.float32)
    kf = dict(valid=(rng.random(n_kf) >= invalid).astype(np.uint8), desc=kf_desc, angle=kf_angle,
              xw=np.ascontiguousarray(xw), obs=rng.choice(np.array([0, 1, 2, 3], np.int32), n_kf, p=[0.25, 0.25, 0.3, 0.2]))
    Tcw = pose(0.012, -0.013, 0.018, (0.034, -0.024, 0.044))
    return assemble(voc_name, kf, kps, desc, ur, Tcw)


def sized(n_cur, n_kf):
    """The shared scene of one SIZES entry: the vocabularies alternate."""
    return scene(n_cur, n_kf, voc_name="k10" if (n_cur, n_kf) in ((64, 64), (5, 0), (0, 5)) else "k3_ragged")


def two_matches():
    """Two keypoints showing the KeyFrame's two valid features: SearchByBoW finds both."""
    return scene(2, 2, seed=5, voc_name="k10", invalid=0.0, displaced=0.0, odd_angle=0.0)


def hand_scene():
    """Six KeyFrame features and seven keypoints a reader can match by eye (test_trk_ref.py)."""
    def d(fill, **bytes_):
        row = np.full(32, fill, np.uint8)
        for k, v in bytes_.items():
            row[int(k[1:])] = v
        return row
    kf_desc = [d(0x00, b0=0x01), d(0x00, b1=0x03), d(0xFF), d(0xFF, b0=0xFE), d(0xFF, b2=0xFC), d(0xF0)]
    cur_desc = [d(0x00, b0=0x01, b5=0x10), d(0x00, b1=0x03, b7=0x80), d(0xFF, b9=0x7F), d(0xFF, b0=0xFC),
                d(0xF0, b31=0xE0), d(0x0F), d(0xFF, b2=0xFC)]
    xw = np.array([[-1, -0.5, 4], [1, -0.5, 3], [-1, 0.5, 5], [1, 0.5, 4], [0, 0, 4], [0.5, 0.8, 3.5]], np.float32)
    T_true = pose(0, 0, 0, (0.02, -0.01, 0.03))
    shows = [0, 1, 2, 3, 5, 4, 4]                   # the KeyFrame point each keypoint is a projection of
    u, v, z = project(T_true, xw[shows])
    kps = np.zeros(7, cf.KEYPOINT_DTYPE)
    kps["x"], kps["y"], kps["angle"], kps["size"], kps["class_id"] = u, v, 60.0, 31.0, -1
    ur = (kps["x"].astype(np.float64) - INTR[4] / z).astype(np.float32)
    ur[3] = -1.0                                    # one monocular edge
    xw[5, 0] += 0.5                                 # the map has KeyFrame point 5 half a metre off
    kf = dict(valid=np.array([1, 1, 1, 1, 0, 1], np.uint8), desc=np.array(kf_desc), angle=np.full(6, 100.0, np.float32),
              xw=xw, obs=np.array([2, 0, 1, 3, 1, 1], np.int32))
    return assemble("hand", kf, kps, np.array(cur_desc), ur, np.eye(4, dtype=np.float32))


def discard_loop(match, outlier, kf_obs, nmatches):
    """Tracking.cc:843-862, literally.  match: vpMapPointMatches as KeyFrame indices (-1: NULL).
    -> (mvpMapPoints afterwards, discarded KeyFrame index per keypoint, nmatches, nmatchesMap)"""
    mvp = np.array(match, np.int32)
    discarded = np.full(len(mvp), -1, np.int32)
    nmatchesMap = 0
    for i in range(len(mvp)):
        if mvp[i] >= 0:
            if outlier[i]:
                discarded[i] = mvp[i]               # pMP->mbTrackInView = false; pMP->mnLastFrameSeen = mnId
                mvp[i] = -1                         # mvpMapPoints[i] = NULL; mvbOutlier[i] = false
                nmatches -= 1
            elif kf_obs[mvp[i]] > 0:
                nmatchesMap += 1
    return mvp, discarded, nmatches, nmatchesMap


def reference(sc, check_orientation=True, min_matches=MIN_MATCHES, nnratio=NNRATIO):
    """Every output of coeb_track_reference_keyframe on scene sc, plus match_bow (SearchByBoW's
    assignments before the discard), outlier (the optimiser's flags) and SearchByBoW's stats."""
    bow = sc["bow"]
    kf = sc["kf"]
    match, nmb, stats = B.search_by_bow(kf["valid"], kf["desc"], kf["node"], kf["angle"], sc["desc"], bow["node"],
                                        sc["kps"]["angle"], nnratio, check_orientation)
    n = len(sc["kps"])
    res = dict(word=bow["word"], node=bow["node"], weight=bow["weight"], match_bow=match.copy(), nmatches_bow=nmb,
               stats=stats)
    if nmb < min_matches:                           # :835
        res.update(match=match, discarded=np.full(n, -1, np.int32), Tcw=sc["Tcw"].copy(), ninliers_pose=0,
                   nmatches=nmb, nmatches_map=0, outlier=np.zeros(n, np.uint8))
        return res
    has = (match >= 0).astype(np.uint8)
    xw = kf["xw"][np.maximum(match, 0)] if len(kf["xw"]) else np.zeros((n, 3), np.float32)
    nin, T, outl = O.pose_optimization(sc["kps"], has, xw, sc["ur"], sc["isg"], *sc["intr"], sc["Tcw"])
    mvp, disc, nm, nmap = discard_loop(match, outl, kf["obs"], nmb)
    res.update(match=mvp, discarded=disc, Tcw=T, ninliers_pose=nin, nmatches=nm, nmatches_map=nmap,
               outlier=np.where(has > 0, outl, 0).astype(np.uint8))
    return res


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def bow_keyframe(sc):
    kf = sc["kf"]
    return cf.BowKeyFrame(kf["valid"], kf["desc"], kf["node"], kf["angle"])


def frame(sc):
    return cf.Frame(sc["kps"], sc["desc"], sc["ur"], Tcw=sc["Tcw"])
