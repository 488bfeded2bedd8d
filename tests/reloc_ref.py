"""Tracking::Relocalization behind PnPsolver::iterate (src/Tracking.cc:1502-1565) for one hypothesis
as the CPU references compose it (no GPU): Optimizer::PoseOptimization (oracle.pose_optimization)
and ORBmatcher::SearchByProjection(F, pKF, sFound, th, ORBdist) (oracle.search_keyframe), with the
entry, discard, merge and gate loops written out from the reference's text.  Plus the scenes the
relocalisation tests share: one current frame of keypoints that are the images of world points, and
KeyFrames that hold some of those points, seen from a nearby pose."""
import functools

import numpy as np

import coeb_front as cf
import oracle as O
import twmm_ref as TW

TH1, ORB1, TH2, ORB2 = 10.0, 100, 3.0, 64           # :1531, :1545
MIN_GOOD, LOW_GOOD, ENOUGH_GOOD = 10, 30, 50        # :1521, :1539, :1529 / :1533 / :1548 / :1561
W, H, INTR = TW.W, TW.H, TW.INTR
cameras, extractor, bits, pose = TW.cameras, TW.extractor, TW.bits, TW.pose
MAIN = (300, 300)
SIZES = ((0, 0), (0, 5), (5, 0), (1, 1), (63, 65), (64, 64), (65, 63), (255, 257), MAIN, (1000, 1000))
COUNTS = ("ngood", "nadditional1", "nadditional2", "stage")


# ---- the composition ----
def reference(fr, hyp, th1=TH1, orb_dist1=ORB1, th2=TH2, orb_dist2=ORB2, check_orientation=True, min_good=MIN_GOOD,
              low_good=LOW_GOOD, enough_good=ENOUGH_GOOD, bounded=False, gates=True):
    """Every output of coeb_reloc_refine for hypothesis hyp on frame fr: match (mvpMapPoints as
    KeyFrame indices), outlier (mvbOutlier where the keypoint held a point at the last optimisation
    that ran, else 0) with written (that mask), Tcw, ngood, nadditional1/2, stage; plus trace: the
    nGood of every optimisation run, found1 / found2 (sFound of the two searches) and held_at (the
    mvpMapPoints each optimisation saw).  gates=False takes every branch whatever the counts say
    (the counts a scene would give at each step, to choose thresholds from)."""
    cam_o = cameras(bounded)[0]
    kps, desc, ur, isg = fr["kps"], fr["desc"], fr["ur"], fr["isg"]
    kf, N = hyp["kf"], len(fr["kps"])
    kn = len(kf["valid"])
    mvp = np.full(N, -1, np.int32)                  # mCurrentFrame.mvpMapPoints
    outl = np.zeros(N, np.uint8)                    # mCurrentFrame.mvbOutlier
    written = np.zeros(N, bool)
    state = dict(T=np.ascontiguousarray(hyp["Tcw"], np.float32).reshape(4, 4).copy())
    trace = dict(ngood=[], held_at=[], found1=None, found2=None)

    def pose_optimization():
        nonlocal outl, written
        has = (mvp >= 0).astype(np.uint8)
        xw = kf["world_pos"][np.maximum(mvp, 0)] if kn else np.zeros((N, 3), np.float32)
        nin, T, out = O.pose_optimization(kps, has, xw, ur, isg, *INTR, state["T"])
        state["T"] = T
        outl = np.where(has > 0, out, outl).astype(np.uint8)    # the flags of keypoints without a point stay
        written = has > 0
        trace["ngood"].append(nin)
        trace["held_at"].append(mvp.copy())
        return nin

    def search(sFound, th, orb_dist):
        if kn == 0:
            return 0
        kv = dict(kf)
        kv["valid"] = kf["valid"].copy()
        for q in sFound:
            kv["valid"][q] = 0
        nm, m = O.search_keyframe(cam_o, kps, desc, (mvp >= 0).astype(np.uint8), kv, state["T"], th, orb_dist,
                                  check_orientation)
        for j in range(N):                          # CurrentFrame.mvpMapPoints[bestIdx2] = pMP (ORBmatcher.cc:1560)
            if m[j] >= 0:
                mvp[j] = m[j]
        return nm

    def result(stage, nGood, nadd1=0, nadd2=0):
        return dict(match=mvp, outlier=np.where(written, outl, 0).astype(np.uint8), written=written, Tcw=state["T"],
                    ngood=nGood, nadditional1=nadd1, nadditional2=nadd2, stage=stage, trace=trace)

    if N == 0:
        return result(0, 0)
    sFound = set()
    for j in range(N):                              # :1508-1517
        if hyp["inlier"][j]:
            mvp[j] = hyp["match"][j]
            sFound.add(int(hyp["match"][j]))
        else:
            mvp[j] = -1
    nGood = pose_optimization()                     # :1519
    if nGood < min_good and gates:                  # :1521
        return result(0, nGood)
    for io in range(N):                             # :1524-1526
        if outl[io]:
            mvp[io] = -1
    if not (nGood < enough_good) and gates:         # :1529
        return result(1, nGood)
    trace["found1"] = set(sFound)
    nadd1 = search(sFound, th1, orb_dist1)          # :1531
    if not (nadd1 + nGood >= enough_good) and gates:    # :1533
        return result(2, nGood, nadd1)
    nGood = pose_optimization()                     # :1535
    if not (nGood > low_good and nGood < enough_good) and gates:    # :1539
        return result(3, nGood, nadd1)
    sFound = set()                                  # :1541-1544
    for ip in range(N):
        if mvp[ip] >= 0:
            sFound.add(int(mvp[ip]))
    trace["found2"] = set(sFound)
    nadd2 = search(sFound, th2, orb_dist2)          # :1545
    if not (nGood + nadd2 >= enough_good) and gates:    # :1548
        return result(4, nGood, nadd1, nadd2)
    nGood = pose_optimization()                     # :1550
    for io in range(N):                             # :1552-1554
        if outl[io]:
            mvp[io] = -1
    return result(5, nGood, nadd1, nadd2)


def first_good(refs, enough_good=ENOUGH_GOOD):
    """The candidate the loop of :1479-1567 breaks on (:1561): the first hypothesis with nGood >= 50."""
    for h, r in enumerate(refs):
        if r["ngood"] >= enough_good:
            return h
    return -1


# ---- scenes ----
T_TRUE = (pose(0.004, -0.006, 0.003, (0.02, -0.015, 0.03)).astype(np.float64) @ TW.T_LAST.astype(np.float64)).astype(np.float32)
ROLES = ("good", "noisy", "disp", "noninl", "w_good", "w_disp", "w_invalid")
SHARES = dict(good=0.3, noisy=0.05, disp=0.05, noninl=0.1, w_good=0.2, w_disp=0.05, w_invalid=0.05)


def scales():
    return np.array(list(extractor().p.scale)[:8], np.float64)


@functools.lru_cache(maxsize=None)
def frame(n_cur, seed=1, mono=0.3):
    """The current frame: n_cur keypoints, each the image (0.3 px noise per level scale) of a world
    point 0.8 to 8 m in front of the camera at T_TRUE; `mono` of them without a right coordinate."""
    rng = np.random.default_rng(500 * seed + n_cur)
    fx, fy, cx, cy, bf = INTR
    kps = np.zeros(n_cur, cf.KEYPOINT_DTYPE)
    u, v = rng.uniform(40, W - 40, n_cur), rng.uniform(40, H - 40, n_cur)
    z = rng.uniform(0.8, 8.0, n_cur)
    kps["octave"] = rng.integers(0, 8, n_cur)
    kps["angle"] = rng.uniform(0.0, 360.0, n_cur)
    kps["size"], kps["response"], kps["class_id"] = 31.0, 50.0, -1
    T = T_TRUE.astype(np.float64)
    Pc = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], 1)
    xw = ((Pc - T[:3, 3]) @ T[:3, :3]).astype(np.float32)          # R^T (Pc - t)
    noise = 0.3 * scales()[kps["octave"]]
    kps["x"], kps["y"] = u + rng.normal(0, 1, n_cur) * noise, v + rng.normal(0, 1, n_cur) * noise
    ur = (kps["x"].astype(np.float64) - bf / z).astype(np.float32)
    ur[rng.random(n_cur) < mono] = -1.0
    desc = rng.integers(0, 256, (n_cur, 32)).astype(np.uint8)
    isg = np.array(list(extractor().p.inv_sigma2), np.float32)
    return dict(kps=np.ascontiguousarray(kps), desc=desc, ur=np.ascontiguousarray(ur), isg=isg, xw=xw, z=z)


def counts_for(n_cur, n_kf, shares=None):
    m = min(n_cur, n_kf)
    sh = SHARES if shares is None else shares
    return tuple(int(sh[k] * m) for k in ROLES) if m > 2 else (m,) + (0,) * 6


@functools.lru_cache(maxsize=None)
def hypothesis(n_cur, n_kf, seed=1, counts=None, shift=0.004, odd_angle=0.05, frame_seed=1, mono=0.3):
    """A candidate KeyFrame of n_kf map points over frame(n_cur, frame_seed, mono), with what
    SearchByBoW and the PnP solver would hand over.  counts = how many keypoints play each role:
      good       matched, inlier, the KeyFrame's point is where the keypoint sees it
      noisy      matched, inlier, the point 2.85 px (per level scale) off in x: past chi2 (8.1 > 5.991),
                 so the first optimisation discards it and it stays in sFound for the first search,
                 but inside the second search's 3 px window, which finds it again
      disp       matched, inlier, the point 6.5 px off: flagged by every optimisation
      noninl     matched, not an inlier: NULL at entry and not in sFound
      w_good     withheld from `match`: only the searches can find it
      w_disp     withheld and 6.5 px off: the first search's window (10 px) takes it, the optimiser flags it
      w_invalid  withheld, and the KeyFrame's slot is not valid (NULL or isBad())
    The other KeyFrame slots hold points this frame does not see.  The KeyFrame's camera sits a few
    centimetres from the frame's (mfMaxDistance / mfMinDistance as UpdateNormalAndDepth leaves
    them), the PnP pose is T_TRUE turned by `shift` radians about y, and `odd_angle` of the shared
    points have a keypoint angle the rotation histogram rejects."""
    fr = frame(n_cur, frame_seed, mono)
    rng = np.random.default_rng(9000 * seed + 31 * n_cur + n_kf)
    cnt = counts_for(n_cur, n_kf) if counts is None else tuple(counts)
    assert sum(cnt) <= min(n_cur, n_kf), (cnt, n_cur, n_kf)
    fx, fy, cx, cy, bf = INTR
    sc = scales()
    m = sum(cnt)
    src = rng.permutation(n_cur)[:m]                # the shared keypoints
    slot = rng.permutation(n_kf)[:m]                # their KeyFrame indices
    role = np.repeat(np.arange(len(ROLES)), cnt)
    T = T_TRUE.astype(np.float64)
    # KeyFrame slots: first random points nobody sees, then the shared ones
    z = rng.uniform(0.8, 8.0, n_kf)
    Pc = np.stack([(rng.uniform(-100, W + 100, n_kf) - cx) * z / fx, (rng.uniform(-100, H + 100, n_kf) - cy) * z / fy, z], 1)
    octave = rng.integers(0, 8, n_kf)
    angle = rng.uniform(0.0, 360.0, n_kf)
    kdesc = rng.integers(0, 256, (n_kf, 32)).astype(np.uint8)
    valid = (rng.random(n_kf) >= 0.1).astype(np.uint8)
    kx = fr["kps"]["x"][src].astype(np.float64)
    zz = fr["z"][src]
    Ps = (fr["xw"][src].astype(np.float64) @ T[:3, :3].T) + T[:3, 3]          # the shared points in the camera
    off = np.zeros((m, 2))
    sgn = rng.choice([-1.0, 1.0], m)
    lv = sc[fr["kps"]["octave"][src]]
    noisy, far = role == 1, (role == 2) | (role == 5)
    off[noisy, 0] = 2.85 * lv[noisy] * sgn[noisy]
    axis = rng.integers(0, 2, m)
    off[far, 0] = np.where(axis[far] == 0, 6.5 * lv[far] * sgn[far], 0.0)
    off[far, 1] = np.where(axis[far] == 1, 6.5 * lv[far] * sgn[far], 0.0)
    Ps[:, 0] += off[:, 0] * zz / fx
    Ps[:, 1] += off[:, 1] * zz / fy
    Pc[slot] = Ps
    octave[slot] = fr["kps"]["octave"][src]
    turn = np.where(rng.random(m) < odd_angle, rng.uniform(60.0, 330.0, m), rng.normal(0, 2.0, m))
    angle[slot] = np.mod(fr["kps"]["angle"][src].astype(np.float64) + turn, 360.0)
    d = fr["desc"][src].copy()
    for i in range(m):
        for b in rng.integers(0, 256, int(rng.integers(0, 7))):
            d[i, b >> 3] ^= np.uint8(1 << (b & 7))
    kdesc[slot] = d
    valid[slot] = np.where(role == 6, 0, 1)
    valid[slot[(role == 0) & (rng.random(m) < 0.1)]] = 0            # positions are read whether or not valid is set
    xw = ((Pc - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    Okf = -T[:3, :3].T @ T[:3, 3] + np.array([0.05, -0.04, 0.08]) * (1 + seed % 3)
    dist = np.linalg.norm(xw.astype(np.float64) - Okf, axis=1)
    maxd = (dist * sc[octave]).astype(np.float32)
    mind = (maxd / np.float32(sc[7])).astype(np.float32)
    kf = dict(valid=valid, world_pos=np.ascontiguousarray(xw), descriptor=kdesc, max_distance=maxd, min_distance=mind,
              angle=angle.astype(np.float32))
    match = np.full(n_cur, -1, np.int32)
    inlier = np.zeros(n_cur, np.uint8)
    matched = role <= 3
    match[src[matched]] = slot[matched]
    inlier[src[role <= 2]] = 1
    Tcw = (pose(0.0, shift, 0.0, (0.003 * (seed % 5), 0.0, -0.002 * (seed % 3))).astype(np.float64) @ T).astype(np.float32)
    return dict(kf=kf, match=match, inlier=inlier, Tcw=np.ascontiguousarray(Tcw), src=src, slot=slot, role=role)


def sized(n_cur, n_kf, seed=1):
    return hypothesis(n_cur, n_kf, seed)


def thresholds_for(fr, hyp, **kw):
    """(min_good, low_good, enough_good) that take hyp through every step where its counts allow it
    (enough_good just above both nGood, below both sums), else the reference's."""
    t = reference(fr, hyp, gates=False, **kw)
    if len(t["trace"]["ngood"]) < 3:
        return MIN_GOOD, LOW_GOOD, ENOUGH_GOOD
    g1, g2 = t["trace"]["ngood"][:2]
    e = max(g1, g2) + 1
    if e <= min(g1 + t["nadditional1"], g2 + t["nadditional2"]) and g1 >= 1:
        return min(MIN_GOOD, g1), min(LOW_GOOD, g2 - 1), e
    return MIN_GOOD, LOW_GOOD, ENOUGH_GOOD


# ---- directed scenes: (name, n_cur, n_kf, counts) with the thresholds chosen from the scene's own counts ----
# counts: good, noisy, disp, noninl, w_good, w_disp, w_invalid
BASES = dict(
    few=(300, 130, (8, 1, 1, 6, 20, 4, 3)),         # nGood < 10 at the reference's thresholds
    rich=(300, 300, (90, 10, 10, 20, 60, 12, 10)),  # nGood >= 50 at once
    short=(300, 210, (22, 3, 3, 10, 12, 3, 4)),     # the first search cannot reach 50
    wide=(300, 310, (34, 5, 4, 15, 70, 10, 8)),     # the second optimisation reaches 50
    mid=(300, 250, (24, 16, 3, 6, 10, 10, 6)),      # 30 < nGood < 50 twice; the second search rediscovers the noisy
    thin=(300, 250, (30, 0, 3, 6, 8, 10, 6)),      # ... and with no noisy inliers it finds too little
)


@functools.lru_cache(maxsize=None)
def base(name):
    n_cur, n_kf, counts = BASES[name]
    return frame(n_cur), hypothesis(n_cur, n_kf, seed=11 + sorted(BASES).index(name), counts=counts)


@functools.lru_cache(maxsize=None)
def base_trace(name):
    fr, hyp = base(name)
    t = reference(fr, hyp, gates=False)
    g = t["trace"]["ngood"]
    return dict(g1=g[0], g2=g[1], g3=g[2], a1=t["nadditional1"], a2=t["nadditional2"])


def directed():
    """[(tag, base name, (min_good, low_good, enough_good), expected stage)].  The reference's
    10 / 30 / 50 on one scene per stage, then every gate on both sides of its boundary with the
    thresholds set from the scene's own counts (base_trace)."""
    D = (MIN_GOOD, LOW_GOOD, ENOUGH_GOOD)
    out = [("default-0", "few", D, 0), ("default-1", "rich", D, 1), ("default-2", "short", D, 2),
           ("default-3", "wide", D, 3), ("default-4", "thin", D, 4), ("default-5", "mid", D, 5)]
    t = base_trace("mid")
    g1, g2, a1 = t["g1"], t["g2"], t["a1"]
    u = base_trace("thin")
    big = 10 ** 6
    out += [
        ("min_good-1", "mid", (g1 + 1, 0, big), 0),                     # nGood == min_good - 1
        ("min_good", "mid", (g1, big, g1), 1),                          # nGood == min_good (and == enough_good)
        ("enough-1@1", "mid", (0, big, g1 + 1), 3 if a1 >= 1 else 2),   # nGood == enough_good - 1 after the first optimisation
        ("sum1-1", "mid", (0, 0, g1 + a1 + 1), 2),                      # nadditional1 + nGood == enough_good - 1
        ("sum1", "mid", (0, big, g1 + a1), 3),                          # ... == enough_good
        ("low", "mid", (0, g2, g1 + a1), 3),                            # second nGood == low_good
        # the second search needs an outlier at the second optimisation (else nGood == the first sum >= enough_good),
        # and to fall short it must find less than the first sum leaves room for: the scene without noisy inliers
        ("low+1", "thin", (0, u["g2"] - 1, u["g2"] + u["a2"] + 1), 4),  # second nGood == low_good + 1: the search runs, falls one short
        ("low+1,5", "thin", (0, u["g2"] - 1, u["g2"] + u["a2"]), 5),    # ... and just reaches enough_good
        ("enough@2", "mid", (0, 0, g2), 3),                             # second nGood == enough_good
    ]
    return out


def directed_case(tag):
    for t, name, th, stage in directed():
        if t == tag:
            fr, hyp = base(name)
            return fr, hyp, th, stage
    raise KeyError(tag)


@functools.lru_cache(maxsize=None)
def directed_ref(tag, check_orientation=True):
    fr, hyp, (mg, lg, eg), _ = directed_case(tag)
    return reference(fr, hyp, check_orientation=check_orientation, min_good=mg, low_good=lg, enough_good=eg)


# ---- the binding's arguments ----
def cur_frame(fr):
    return cf.Frame(fr["kps"], fr["desc"], fr["ur"])


def hyp_args(hyp):
    k = hyp["kf"]
    return (cf.KeyFramePoints(k["valid"], k["world_pos"], k["descriptor"], k["max_distance"], k["min_distance"], k["angle"]),
            hyp["match"], hyp["inlier"], hyp["Tcw"])
