"""Directed point sets for findFundamentalMat's loops (k_fm of csrc/coeb_flow.hip, the oracle's
oc_find_fundamental, the model of tests/flow_ref.py).  Every set is a pair of (n, 2) float32 arrays
whose coordinates stay inside [6, W - 6) x [6, H - 6) of a W x H frame, to run on a flat image
pair (every 3x3 SAD is 0).  What each set reaches is asserted on the model's trace in
tests/test_flow_ref.py; the seeds below were found by search with that trace.

The scenes: 3-D points seen by two cameras a small rotation and a translation apart, `sigma`
pixels of noise, and a share of the pairs displaced by up to 8 px (30%, or 60% in noisy40 and larger)."""
import numpy as np

W, H = 120, 100
MARGIN = 6
FOCAL = 110.0


def flat_pair():
    img = np.full((H, W), 10, np.uint8)
    return img, img.copy()


def inside(m):
    return (m[:, 0] >= MARGIN) & (m[:, 0] < W - MARGIN) & (m[:, 1] >= MARGIN) & (m[:, 1] < H - MARGIN)


def f32(m):
    m = np.ascontiguousarray(m, np.float32)
    assert inside(m).all()
    return m


def scene(n, seed, sigma=0.0, outliers=0.0, shift=None):
    """n pairs of a two-view scene (or of a pure image shift), all inside the margin."""
    rng = np.random.default_rng(seed)
    X = np.concatenate([rng.uniform(-3.5, 3.5, (8 * n + 64, 2)), rng.uniform(4, 12, (8 * n + 64, 1))], 1)
    ang = rng.uniform(-0.03, 0.03, 3)
    (cx, cy, cz), (sx, sy, sz) = np.cos(ang), np.sin(ang)
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
         np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    t = rng.uniform(-0.4, 0.4, 3)
    K = np.array([[FOCAL, 0, W / 2], [0, FOCAL, H / 2], [0, 0, 1]])
    a, b = (K @ X.T).T, (K @ (R @ X.T + t[:, None])).T
    m1, m2 = a[:, :2] / a[:, 2:], b[:, :2] / b[:, 2:]
    if shift is not None:
        m2 = m1 + np.asarray(shift, np.float64)
    m2 = m2 + rng.normal(0, 1, m2.shape) * sigma
    out = rng.uniform(0, 1, len(m2)) < outliers
    m2 = m2 + out[:, None] * rng.uniform(-8, 8, m2.shape)
    m1, m2 = m1.astype(np.float32), m2.astype(np.float32)
    ok = np.nonzero(inside(m1) & inside(m2))[0][:n]
    assert len(ok) == n, (n, seed)
    return f32(m1[ok]), f32(m2[ok])


def on_line(k, seed, x0=10.0, y0=12.0, dx=1.0, dy=0.75):
    """k distinct points of a line whose float32 coordinates are exact (multiples of 1/4)."""
    s = np.random.default_rng(seed).permutation(96)[:k].astype(np.float64)
    return np.stack([x0 + dx * s, y0 + dy * s], 1)


def random_pairs(n, seed):
    rng = np.random.default_rng(seed)
    lo, hi = [MARGIN, MARGIN], [W - MARGIN - 0.01, H - MARGIN - 0.01]
    return f32(rng.uniform(lo, hi, (n, 2))), f32(rng.uniform(lo, hi, (n, 2)))


def line_mix(n, k, seed):
    """n pairs of a noisy scene of which the first k previous points are moved onto one line, then
    shuffled: many redraws between good subsets."""
    m1, m2 = scene(n, seed, sigma=0.3)
    m1 = m1.copy()
    m1[:k] = on_line(k, seed)
    p = np.random.default_rng(seed + 1).permutation(n)
    return f32(m1[p]), f32(m2[p])


def rare_subset(seed):
    """14 pairs with a drawable subset that 1000 attempts do not find.  Previous points 0..12 lie
    on one line, so the seventh point of a subset must be pair 13; the current points 0..12 lie on
    six rays from current point 13 (3, 3, 3, 2, 1, 1 points), so the other six must come from six
    different rays: 54 of the 1716 six-subsets, one subset in 445."""
    m1 = np.concatenate([on_line(13, seed), [[40.0, 70.0]]])
    c = np.array([60.0, 50.0])
    dirs = np.array([[1, 0], [0, 1], [1, 1], [-1, 1], [-1, -0.5], [1, -0.75]], np.float64)
    rays = [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 4, 5]
    steps = [8, 16, 24, 8, 16, 24, 8, 16, 24, 8, 16, 8, 8]
    m2 = np.concatenate([np.array([c + dirs[r] * s for r, s in zip(rays, steps)]), [c]])
    p = np.random.default_rng(seed).permutation(14)
    return f32(m1[p]), f32(m2[p])


def seven_repeated():
    """Seven pairs of which only five are distinct: the 7x9 system loses rank and the solver
    returns no model."""
    m1, m2 = scene(5, 3)
    i = [0, 1, 2, 3, 4, 0, 1]
    return f32(m1[i]), f32(m2[i])


# name -> builder.  Seeds: see the module docstring.
SETS = {
    "none": lambda: (np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32)),
    "six": lambda: scene(6, 1),
    "seven_one_root": lambda: scene(7, SEEDS["seven_one_root"], sigma=0.5),
    "seven_three_roots": lambda: scene(7, SEEDS["seven_three_roots"], sigma=0.5),
    "seven_repeated": seven_repeated,
    "clean8": lambda: scene(8, 8), "clean9": lambda: scene(9, 9), "clean14": lambda: scene(14, 14),
    "noisy8": lambda: scene(8, SEEDS["noisy8"], sigma=0.3, outliers=0.15),
    "noisy9": lambda: scene(9, SEEDS["noisy9"], sigma=0.3, outliers=0.2),
    "noisy12": lambda: scene(12, 12, sigma=0.3, outliers=0.2),
    "noisy14": lambda: scene(14, 14, sigma=0.3, outliers=0.2),
    "clean15": lambda: scene(15, 15), "clean16": lambda: scene(16, 16), "clean40": lambda: scene(40, 40),
    "clean129": lambda: scene(129, 129), "clean300": lambda: scene(300, 300), "clean1024": lambda: scene(1024, 1024),
    "noisy15": lambda: scene(15, SEEDS["noisy15"], sigma=0.05, outliers=0.3),
    "noisy16": lambda: scene(16, SEEDS["noisy16"], sigma=0.05, outliers=0.3),
    "noisy40": lambda: scene(40, 40, sigma=0.05, outliers=0.6),
    "noisy129": lambda: scene(129, 129, sigma=0.05, outliers=0.6),
    "noisy300": lambda: scene(300, 300, sigma=0.05, outliers=0.6),
    "noisy1024": lambda: scene(1024, 1024, sigma=0.05, outliers=0.6),
    "chunk_boundary": lambda: scene(SEEDS["chunk_boundary"][0], SEEDS["chunk_boundary"][1], sigma=0.05, outliers=0.3),
    "chunk_plus_one": lambda: scene(SEEDS["chunk_plus_one"][0], SEEDS["chunk_plus_one"][1], sigma=0.05, outliers=0.3),
    "shift45": lambda: (lambda g: (f32(g), f32(g + [2.5, 1.25])))(
        np.stack(np.meshgrid(10.0 + 11 * np.arange(9), 12.0 + 17 * np.arange(5)), -1).reshape(-1, 2)),
    "collinear20": lambda: (f32(on_line(20, 20)), scene(20, 20)[1]),
    "collinear12": lambda: (scene(12, 12)[0], f32(on_line(12, 12, 100.0, 10.0, -0.75, 0.5))),
    "five_points20": lambda: (lambda m: (f32(np.tile(m[0], (4, 1))), f32(np.tile(m[1], (4, 1)))))(scene(5, 5)),
    "line14_of_24": lambda: line_mix(24, 14, 24),
    "line7_of_12": lambda: line_mix(12, 7, 12),
    "identity20": lambda: (lambda m: (m, m.copy()))(scene(20, 0)[0]),
    "random30": lambda: random_pairs(30, 30),
    "random12": lambda: random_pairs(12, 12),
    "rare_subset14": lambda: rare_subset(SEEDS["rare_subset14"]),
    "rare_subset14_late": lambda: rare_subset(SEEDS["rare_subset14_late"]),
    "near_line16": lambda: near_line(16, SEEDS["near_line16"]),
}
SEEDS = {"seven_one_root": 0, "seven_three_roots": 2, "noisy8": 8, "noisy9": 9, "noisy15": 15, "noisy16": 16,
         "chunk_boundary": (20, 39), "chunk_plus_one": (20, 88), "rare_subset14": 4, "rare_subset14_late": 9,
         "near_line16": 0}


def near_line(n, seed):
    """Unrelated pairs whose previous points lie within 1e-4 px of one line without passing the
    collinearity test: the 7-point systems are close to rank-deficient."""
    rng = np.random.default_rng(seed)
    m1 = on_line(n, seed) + rng.uniform(-1e-4, 1e-4, (n, 2))
    return f32(m1), random_pairs(n, seed + 100)[1]


_cache = {}


def get(name):
    if name not in _cache:
        m1, m2 = SETS[name]()
        m1.setflags(write=False)
        m2.setflags(write=False)
        _cache[name] = (m1, m2)
    return _cache[name]


# ---- thinning: noisy1024 with all but a few pairs removed before findFundamentalMat
def spread(k, n=1024):
    """k kept indices spread over 0..n - 1, the last one n - 1."""
    return np.unique(np.round(np.linspace(5, n - 1, k)).astype(int))


def thin_states():
    """name -> state (1024,) u8 for noisy1024.  k_fm's 128-thread form gives a thread 8 consecutive
    indices: `runs` keeps a whole run of 8, clears the next and keeps index 1023."""
    out = {}
    for k in (7, 8, 14, 15, 129):
        s = np.zeros(1024, np.uint8)
        s[spread(k)] = 1
        assert s.sum() == k and s[1023] == 1
        out["keep%d" % k] = s
    s = np.zeros(1024, np.uint8)
    s[512:520] = 1
    s[[3, 100, 333, 777, 900, 1016, 1023]] = 1
    assert s[520:528].sum() == 0
    out["runs15"] = s
    return out


def sad_thinned():
    """(prev, cur, state): a bright block in `cur` fails the SAD check of every pair of noisy1024
    whose current point lies in or next to it; all states are set."""
    prev, cur = flat_pair()
    cur[30:70, 20:100] = 255
    return prev, cur, np.ones(1024, np.uint8)


def thin_cases():
    """name -> (prev, cur, previous points, current points, state): noisy1024 thinned by state and
    by SAD, and noisy40 followed by the edge-rule points of flow_shapes.tail_edge_points."""
    import flow_shapes as fs
    m1, m2 = get("noisy1024")
    prev, cur = flat_pair()
    out = {k: (prev, cur, m1, m2, s) for k, s in thin_states().items()}
    out["sad_block"] = sad_thinned()[:2] + (m1, m2, sad_thinned()[2])
    a1, a2 = get("noisy40")
    ep, en, _ = fs.tail_edge_points(W, H)
    out["edges"] = (prev, cur, np.concatenate([a1, ep]), np.concatenate([a2, en]), np.ones(len(a1) + len(ep), np.uint8))
    return out


def oracle_solver(O):
    """The oracle's run7Point in flow_ref's solver interface."""
    lib = O.lib()

    def solve(s1, s2):
        s1, s2 = np.ascontiguousarray(s1, np.float32), np.ascontiguousarray(s2, np.float32)
        F = np.zeros(27, np.float64)
        n = lib.oc_run7point(O.ptr(s1), O.ptr(s2), O.ptr(F))
        return n, [F[9 * k:9 * k + 9].copy() for k in range(max(n, 0))]
    return solve


def oracle_tail_capped(O, prev, cur, pxy, nxy, state, cap, sentinel=-7.0):
    """oc_moving_tail with a T_M capacity: (|T_M|, the (len, 2) buffer filled with the sentinel first)."""
    import ctypes as C
    h, w = prev.shape
    pxy, nxy = np.ascontiguousarray(pxy, np.float32), np.ascontiguousarray(nxy, np.float32)
    st = np.ascontiguousarray(state, np.uint8).copy()
    tm = np.full((len(pxy), 2), sentinel, np.float32)
    nt = O.lib().oc_moving_tail(O.ptr(prev), O.ptr(cur), w, h, w, O.ptr(pxy), O.ptr(nxy), O.ptr(st), len(pxy), 5,
                                C.c_double(2120.0), O.ptr(tm), cap, None, None)
    return nt, tm
