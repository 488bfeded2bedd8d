"""A plain float64 model of Optimizer::PoseOptimization(Frame*) (Optimizer.cc:239-451), written
from g2o's published definitions, and the directed problems the pose tests share.

The model is independent of oracle/orb_oracle.c and of csrc/coeb_pose.hip: poses are rotation
matrices, the Jacobians are the chain rule d proj / d p * [-[p]x | I] written as matrix products,
sums are np.sum / einsum, the linear system goes through np.linalg.  It makes no attempt at the
oracle's operation or summation order, so it agrees with it to roundoff amplified by the LM
trajectory, not bit for bit; the tests compare results (flags, inlier count, pose), never the
iteration or trial counts.

What it restates:
  * EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose: e = obs - cam_project(T * Xw);
    the stereo cam_project divides by `const float invz = 1.0f / z`.
  * RobustKernelHuber with delta = (float)sqrt(5.991) / (float)sqrt(7.815); the robustified
    information is rho' * Omega (g2o's second-order term is commented out in that release).
  * OptimizationAlgorithmLevenberg::solve: lambda0 = 1e-5 * max |H_jj|; rho = (chi - chi') /
    (x . (lambda x + b) + 1e-3); accepted steps scale lambda by clamp(1 - (2 rho - 1)^3, 1/3, 2/3)
    and reset ni = 2, rejected ones do lambda *= ni, ni *= 2; at most 10 trials per iteration;
    Terminate on qmax == 10 or rho == 0.
  * SE3Quat::exp (small-angle branch below 1e-5: R = I + W + W^2, V = R) applied on the left.
  * Four optimize(10) calls from the entry pose, the robust kernel off in the last; after each,
    `const float chi2 = e->chi2()` against the float threshold, where an edge that was active
    keeps the error of the LAST computeActiveErrors (possibly a rejected trial's estimate) and an
    inactive one is recomputed at the final estimate.
  * nInitialCorrespondences < 3 returns 0 with the pose untouched; fewer than 10 edges stop
    after the first round.
A failed factorisation (H + lambda I not positive definite, or not finite) takes x = 0 and
tempChi = DBL_MAX, as the oracle does; g2o would reuse the solver's previous x there.
"""
import numpy as np

CHI2_TH = (np.float32(5.991), np.float32(7.815))                       # mono, stereo
DELTA = (float(np.float32(np.sqrt(5.991))), float(np.float32(np.sqrt(7.815))))
TUM_CAM = (535.4, 539.2, 320.1, 247.6, 40.0)


def inv_sigma2(nlevels=8, sf=1.2):
    """mvInvLevelSigma2 as ORBextractor.cc:426-438 builds it: float products of the float scale
    factor (the tables the context and the oracle's Extractor hold)."""
    s = [np.float32(1.0)]
    for _ in range(1, nlevels):
        s.append(np.float32(s[-1] * np.float32(sf)))
    return np.array([np.float32(1.0) / np.float32(x * x) for x in s], np.float32)


# ------------------------------------------------------------------------------- SE3
def skew(v):
    z = v.dtype.type(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], v.dtype)


def nearest_rotation(M):
    """The rotation closest to M (Frobenius): what normalising the quaternion of a nearly
    orthogonal matrix amounts to, up to second order in its defect."""
    U, _, Vt = np.linalg.svd(M)
    if np.linalg.det(U @ Vt) < 0:
        U[:, 2] = -U[:, 2]
    return U @ Vt


def se3_exp(u):
    """SE3Quat::exp(update), update = (omega, upsilon) -> (R, t).  Works in u's dtype above the
    small-angle threshold (np.longdouble for the difference quotients)."""
    ft = u.dtype.type
    om, ups = u[:3], u[3:]
    th = np.sqrt(np.sum(om * om))
    W = skew(om)
    W2 = W @ W
    I = np.eye(3, dtype=u.dtype)
    if th < 0.00001:
        R = I + W + W2
        V = R
        R = nearest_rotation(R.astype(np.float64)).astype(u.dtype)
    else:
        s, c = np.sin(th), np.cos(th)
        R = I + (s / th) * W + ((ft(1) - c) / (th * th)) * W2
        V = I + ((ft(1) - c) / (th * th)) * W + ((th - s) / (th * th * th)) * W2
    return R, V @ ups


def oplus(u, R, t):
    """VertexSE3Expmap::oplusImpl: exp(u) * (R, t)."""
    dR, dt = se3_exp(u)
    return dR @ R, dR @ t + dt


# ------------------------------------------------------------------------------- edges
def edge_errors(R, t, X, obs, stereo, cam, float_invz=True):
    """Errors (ne, 3) of all edges at (R, t); a monocular edge's third component is 0.
    float_invz: the stereo cam_project's `const float invz` (off for the difference quotients)."""
    fx, fy, cx, cy, bf = cam
    p = X @ R.T + t
    with np.errstate(all="ignore"):
        invz = 1 / p[:, 2]
        if float_invz:
            invz_s = (np.float32(1.0) / p[:, 2].astype(np.float32)).astype(p.dtype)
            invz = np.where(stereo, invz_s, invz)
        u = p[:, 0] * invz * fx + cx
        v = p[:, 1] * invz * fy + cy
        ur = u - bf * invz
        e = np.stack([obs[:, 0] - u, obs[:, 1] - v, np.where(stereo, obs[:, 2] - ur, 0)], 1)
    return e


def edge_jacobians(R, t, X, stereo, cam):
    """d e / d delta (ne, 3, 6) for T <- exp(delta) * T, delta = (omega, upsilon):
    p' = p + omega x p + upsilon, so dp / d delta = [-[p]x | I], and e = obs - proj(p)."""
    fx, fy, cx, cy, bf = cam
    p = X @ R.T + t
    ne = len(p)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        dproj = np.zeros((ne, 3, 3))
        dproj[:, 0, 0] = fx / z
        dproj[:, 0, 2] = -fx * x / (z * z)
        dproj[:, 1, 1] = fy / z
        dproj[:, 1, 2] = -fy * y / (z * z)
        dproj[:, 2, 0] = fx / z
        dproj[:, 2, 2] = -(fx * x - bf) / (z * z)
        dproj[~stereo, 2, :] = 0.0
        dp = np.zeros((ne, 3, 6))
        dp[:, 0, 1], dp[:, 0, 2] = z, -y                      # -[p]x
        dp[:, 1, 0], dp[:, 1, 2] = -z, x
        dp[:, 2, 0], dp[:, 2, 1] = y, -x
        dp[:, 0, 3] = dp[:, 1, 4] = dp[:, 2, 5] = 1.0
        return -(dproj @ dp)


def huber(e2, delta):
    """RobustKernelHuber::robustify -> (rho, rho')."""
    e2 = np.asarray(e2, np.float64)
    d2 = delta * delta
    with np.errstate(all="ignore"):
        sq = np.sqrt(e2)
        inl = e2 <= d2
        return np.where(inl, e2, 2 * sq * delta - d2), np.where(inl, 1.0, delta / sq)


# ------------------------------------------------------------------------------- the optimiser
class _Problem:
    def __init__(self, kps, has_mp, xw, ur, isg, cam):
        self.idx = np.nonzero(np.asarray(has_mp) > 0)[0]
        k = kps[self.idx]
        self.X = np.asarray(xw, np.float32).reshape(-1, 3)[self.idx].astype(np.float64)
        u = np.asarray(ur, np.float32)[self.idx]
        self.stereo = ~(u < 0)                                            # Optimizer.cc:286
        self.obs = np.stack([k["x"].astype(np.float64), k["y"].astype(np.float64),
                             np.where(self.stereo, u.astype(np.float64), 0.0)], 1)
        self.w = np.asarray(isg, np.float32)[k["octave"]].astype(np.float64)
        self.cam = tuple(float(np.float32(c)) for c in cam)               # Frame's intrinsics are float
        self.delta = np.where(self.stereo, DELTA[1], DELTA[0])
        self.th = np.where(self.stereo, CHI2_TH[1], CHI2_TH[0]).astype(np.float32)

    def chi2(self, R, t, sel):
        e = edge_errors(R, t, self.X[sel], self.obs[sel], self.stereo[sel], self.cam)
        with np.errstate(all="ignore"):
            return self.w[sel] * np.sum(e * e, 1), e


def _active_chi2(P, R, t, act, robust, chi2_last):
    c, e = P.chi2(R, t, act)
    chi2_last[act] = c
    r = huber(c, P.delta[act])[0] if robust else c
    return float(np.sum(r)), c, e


def _optimize(P, R, t, act, robust, chi2_last, trace):
    """One SparseOptimizer::optimize(10)."""
    lam, ni = 0.0, 2.0
    for it in range(10):
        cur, c, e = _active_chi2(P, R, t, act, robust, chi2_last)
        J = edge_jacobians(R, t, P.X[act], P.stereo[act], P.cam)
        wgt = P.w[act] * (huber(c, P.delta[act])[1] if robust else 1.0)
        with np.errstate(all="ignore"):
            H = np.einsum("n,nri,nrj->ij", wgt, J, J)
            b = -np.einsum("n,nri,nr->i", wgt, J, e)
        if it == 0:
            lam, ni = 1e-5 * float(np.max(np.abs(np.diag(H)))), 2.0
        rho, qmax = 0.0, 0
        while True:
            A = H + lam * np.eye(6)
            ok = bool(np.all(np.isfinite(A)) and np.all(np.isfinite(b)))
            if ok:
                try:
                    np.linalg.cholesky(A)
                    x = np.linalg.solve(A, b)
                except np.linalg.LinAlgError:
                    ok = False
            if not ok:
                x = np.zeros(6)
            Rn, tn = oplus(x, R, t)
            tmp = _active_chi2(P, Rn, tn, act, robust, chi2_last)[0]
            if not ok:
                tmp = np.finfo(np.float64).max
            with np.errstate(all="ignore"):
                rho = (cur - tmp) / (float(x @ (lam * x + b)) + 1e-3)
            good = bool(rho > 0 and np.isfinite(tmp))
            if trace is not None:
                trace.append(dict(robust=robust, iteration=it, trial=qmax, lam=lam, H=H, b=b, x=x, rho=rho,
                                  accepted=good, R=Rn, t=tn))
            if good:
                alpha = min(1.0 - (2.0 * rho - 1.0) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                cur = tmp
                R, t = Rn, tn
            else:
                lam *= ni
                ni *= 2.0
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        if qmax == 10 or rho == 0:
            break
    return R, t


def pose_optimization(kps, has_mp, xw, ur, isg, cam, Tcw, trace=None):
    """-> (ninliers, T float64 4x4, outlier flags uint8 (n), chi2 of the final classification
    float64 (n), NaN where no MapPoint).  trace: a list that receives one dict per LM trial."""
    n = len(kps)
    P = _Problem(kps, has_mp, xw, ur, isg, cam)
    ne = len(P.idx)
    outl = np.zeros(n, np.uint8)
    chi2 = np.full(n, np.nan)
    T0 = np.asarray(Tcw, np.float32).astype(np.float64).reshape(4, 4)
    if ne < 3:
        return 0, T0.copy(), outl, chi2
    R0, t0 = nearest_rotation(T0[:3, :3]), T0[:3, 3].copy()              # Converter::toSE3Quat
    act = np.ones(ne, bool)
    chi2_last = np.zeros(ne)
    for rnd in range(4):
        R, t = _optimize(P, R0, t0, act, rnd < 3, chi2_last, trace)
        if (~act).any():
            chi2_last[~act] = P.chi2(R, t, ~act)[0]
        with np.errstate(all="ignore"):
            bad = chi2_last.astype(np.float32) > P.th                     # const float chi2 = e->chi2()
        act = ~bad
        if ne < 10:
            break
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    outl[P.idx] = bad
    chi2[P.idx] = chi2_last
    return int(ne - bad.sum()), T, outl, chi2


def run_model(P, trace=None):
    return pose_optimization(P["kps"], P["has_mp"], P["xw"], P["ur"], inv_sigma2(), P.get("cam", TUM_CAM),
                             P["Tcw_init"], trace)


def run_oracle(O, P):
    return O.pose_optimization(P["kps"], P["has_mp"], P["xw"], P["ur"], inv_sigma2(), *P.get("cam", TUM_CAM),
                               P["Tcw_init"])


# ------------------------------------------------------------------------------- agreement
# max |T_oracle - T_model| over PROBLEMS, measured on the CPU (the table in DESIGN.md s2.1): the
# oracle's pose is rounded to float, so half a float ulp of an entry near 1 (2.98e-8) is the floor.
POSE_MEASURED_MAX = 2.92e-8
POSE_BOUND = 4 * POSE_MEASURED_MAX


def compare_with_model(P, nin, T, outl, model=None):
    """The comparison of an implementation's result (oracle or kernel) with the model's: inlier
    count and flags equal, except that at most one edge whose model chi2 lies within relative
    1e-6 of its threshold may differ; max |T - T_model| <= POSE_BOUND.  Returns that maximum."""
    m_nin, m_T, m_out, m_chi = model if model is not None else run_model(P)
    has = P["has_mp"] > 0
    diff = np.nonzero(has & (np.asarray(outl) != m_out))[0]
    ur = np.asarray(P["ur"])
    for i in diff:
        th = float(CHI2_TH[0] if ur[i] < 0 else CHI2_TH[1])
        assert abs(m_chi[i] - th) <= 1e-6 * th, ("flag differs away from the threshold", int(i), m_chi[i], th)
    assert len(diff) <= 1, ("more than one borderline flag", diff)
    if has.sum() >= 3:
        assert nin == int(has.sum()) - int(np.asarray(outl)[has].sum()), (nin, int(has.sum()))
    assert nin == m_nin + int(m_out[diff].astype(int).sum()) - int(np.asarray(outl)[diff].astype(int).sum()), (nin, m_nin)
    d =float(np.max(np.abs(np.asarray(T, np.float64) - m_T)))
    assert d <= POSE_BOUND, (d, POSE_BOUND)
    return d


# ------------------------------------------------------------------------------- directed problems
def rot180(axis):
    """The half turn about a coordinate axis: an exact sign flip of the other two."""
    d = -np.ones(3)
    d[axis] = 1.0
    return np.diag(d)


def reworld(P, Rw):
    """P in a world frame rotated by Rw: xw <- Rw xw, Tcw <- Tcw Rw^T (camera-frame points, and so
    the whole optimisation, are unchanged up to rounding; the entry rotation is not)."""
    Q = dict(P)
    Q["xw"] = (P["xw"].astype(np.float64) @ Rw.T).astype(np.float32)
    for k in ("Tcw_init", "Tcw_true"):
        T = P[k].astype(np.float64).copy()
        T[:3, :3] = T[:3, :3] @ Rw.T
        Q[k] = T.astype(np.float32)
    return Q


def behind(P, every=7, dz=8.0, zero="inf"):
    """Every `every`-th point pushed dz metres behind along the entry camera's axis, the entry
    rotation made exactly the identity (the world re-expressed in the entry camera's axes), and
    one monocular point appended whose camera-frame z at the entry pose is exactly 0: with
    x, y != 0 its projection is +-inf (zero="inf"), with x = y = 0 it is NaN (zero="nan")."""
    Q = reworld(P, P["Tcw_init"][:3, :3].astype(np.float64))
    for k in ("Tcw_init", "Tcw_true"):
        Q[k] = Q[k].copy()
    Q["Tcw_init"][:3, :3] = np.eye(3, dtype=np.float32)
    xw = Q["xw"].copy()
    xw[::every, 2] -= np.float32(dz)
    tz = Q["Tcw_init"][2, 3]
    extra = np.array([[0.3, -0.2, -tz]] if zero == "inf" else [[-Q["Tcw_init"][0, 3], -Q["Tcw_init"][1, 3], -tz]],
                     np.float32)
    Q["xw"] = np.concatenate([xw, extra])
    kp = P["kps"][:1].copy()
    kp["octave"] = 0
    Q["kps"] = np.concatenate([P["kps"], kp])
    Q["ur"] = np.concatenate([P["ur"], np.float32([-1.0])])
    Q["has_mp"] = np.concatenate([P["has_mp"], np.uint8([1])])
    Q["gross"] = np.concatenate([P["gross"], [True]])
    return Q


def sized(n, has_frac=None, **kw):
    """make_pose_problem(n, seed=n) with every keypoint holding a MapPoint (ne == n), or a
    has_frac share of them."""
    from coeb_front import synth
    P = synth.make_pose_problem(n=n, seed=kw.pop("seed", n), **kw)
    if has_frac is None:
        P["has_mp"] = np.ones(n, np.uint8)
    return P


def ept_of(n):
    """Which k_pose template the single-frame entry runs for n keypoints: launch_pose takes
    stride = max(n, 1) and ceil(stride / 256) edges per thread; <= 5 -> k_pose<5>, <= 9 -> k_pose<9>,
    else k_pose<0> (edges in global scratch)."""
    ept = (max(n, 1) + 255) // 256
    return 5 if ept <= 5 else 9 if ept <= 9 else 0


SIZES = (1, 3, 9, 10, 31, 32, 33, 255, 256, 257, 512, 1280, 1281, 2304, 2305, 2600)


def _problems():
    from coeb_front import synth
    mk = synth.make_pose_problem
    out = {}
    for seed, kw in [(0, {}), (1, {"outlier_frac": 0.4}), (2, {"mono_frac": 1.0}), (3, {"mono_frac": 0.0, "n": 1500}),
                     (4, {"noise": 3.0}), (5, {"init_err": (0.15, 0.3)})]:
        out["base-seed%d%s" % (seed, "-rejectrun7" if seed == 4 else "")] = lambda seed=seed, kw=kw: mk(seed=seed, **kw)
    out["n12-seed6"] = lambda: mk(n=12, seed=6)
    out["init0.5-seed2"] = lambda: mk(seed=2, init_err=(0.5, 0.5))
    out["qmax10-init1.0-seed3"] = lambda: mk(seed=3, init_err=(1.0, 1.0))
    for ax in range(3):
        out["quat%d-turn180%s" % (ax, "xyz"[ax])] = lambda ax=ax: reworld(mk(n=300, seed=11), rot180(ax))
    out["behind-every7-zinf"] = lambda: behind(mk(n=300, seed=7), 7, 8.0, "inf")
    out["behind-every7-znan"] = lambda: behind(mk(n=300, seed=7), 7, 8.0, "nan")
    for n in SIZES:
        out["n%d" % n] = lambda n=n: sized(n)
    out["n2600-has90"] = lambda: sized(2600, has_frac=0.9, seed=1)
    return out


PROBLEMS = _problems()


def problem_id(name):
    """The test id of a problem: its name and the k_pose template its size selects."""
    return "%s-ept%d" % (name, ept_of(len(PROBLEMS[name]()["kps"])))


_cache = {}


def problem(name):
    """(P, model result) of a named problem, built and solved once per process; treat as read-only."""
    if name not in _cache:
        P = PROBLEMS[name]()
        _cache[name] = (P, run_model(P))
    return _cache[name]


# ------------------------------------------------------------------------------- the kernel
def run_kernel(ctx, P, cam=None):
    """coeb_pose_optimization through coeb_front.Optimizer -> (ninliers, Tcw float32, mvbOutlier)."""
    import coeb_front
    intr = P.get("cam", TUM_CAM)
    cam = cam or coeb_front.make_camera(*intr, 640, 480)
    F = coeb_front.Frame(P["kps"], np.zeros((len(P["kps"]), 32), np.uint8), P["ur"], Tcw=P["Tcw_init"])
    F.mvpMapPoints = np.where(P["has_mp"] > 0, 0, -1).astype(np.int32)
    F.mvMapPointPos = P["xw"]
    nin = coeb_front.Optimizer.PoseOptimization(F, cam, ctx)
    return nin, F.mTcw, F.mvbOutlier


def pose_both(ctx, oracle_mod, P, cam=None, result=None):
    """coeb_pose_optimization vs oracle.pose_optimization: pose bits, outlier flags and the
    inlier count identical (same canonical operations and reduction order)."""
    isg = np.array(ctx.tables().inv_sigma2[:8], np.float32)
    intr = P.get("cam", TUM_CAM)
    nin_ref, T_ref, out_ref = oracle_mod.pose_optimization(P["kps"], P["has_mp"], P["xw"], P["ur"], isg, *intr,
                                                           P["Tcw_init"])
    nin, T, outl = result if result is not None else run_kernel(ctx, P, cam)
    assert nin == nin_ref, (nin, nin_ref)
    assert np.array_equal(T.view(np.uint32), T_ref.view(np.uint32)), (T, T_ref)
    has = P["has_mp"] > 0
    assert np.array_equal(outl[has], out_ref[has])
    return nin
