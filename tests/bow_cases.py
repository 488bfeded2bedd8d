"""Directed inputs for the bag-of-words front end and the device keyframe database: vocabularies,
node arrays, SearchByBoW scenes and database queries built by construction -- every descriptor is
a chosen set of bits, so every distance is the builder's choice -- each sitting on a boundary of
k_bow_transform, k_bow_csr, bow_match_node, k_kfdb_common / k_kfdb_score or k_match_bow_db.
No GPU here.  Each builder returns the call's inputs; the *_facts functions derive from the
reference's own result (tests/bow_ref.py, tests/kfdb_ref.py) what the case is for, and
tests/test_bow_cases.py asserts those facts, so a case that stops reaching its path fails there.
The GPU files (tests/test_gpu_bow_directed.py, tests/test_gpu_kfdb_directed.py) compare the
device's results with the same references bit for bit."""
import functools

import numpy as np

import bow_ref as R
import kfdb_ref as K

BLK = 12                                    # bits per block: 20 blocks in 256 bits
COUNTS = (1, 7, 8, 9, 15, 16, 17, 31, 32, 33)
WIDE_K = (2, 15, 16, 17, 20)
LIST_LENGTHS = (1, 63, 64, 65, 127, 128, 129, 192, 193)
EDGE_PAIRS = ((50, 256), (51, 256), (15, 25), (27, 45), (30, 50), (7, 10), (35, 50), (34, 50), (14, 25), (15, 26),
              (3, 5), (6, 10))              # the last two: 0.6f * b2 is a float32 tie that rounds down to d1
MAX_COMMON = (1, 4, 5, 6, 9, 10, 11)


def depths(ref):
    """node -> depth of a bow_ref.Voc"""
    depth = {0: 0}
    for nd in range(ref.nnodes):
        for ch in ref.children[nd]:
            depth[ch] = depth[nd] + 1
    return depth


def D(*bit_sets):
    """The descriptor with exactly the given bits set: hamming(D(a), D(b)) = |a ^ b|."""
    d = np.zeros(32, np.uint8)
    for s in bit_sets:
        for b in s:
            d[b >> 3] |= 1 << (b & 7)
    return d


def blk(j, n=BLK):
    return range(BLK * j, BLK * j + n)


# ================================================================ vocabularies
class Tree:
    """A vocabulary under construction; arrays() numbers it breadth first, children consecutive."""

    def __init__(self, k, L):
        self.k, self.L = k, L
        self.parent, self.desc, self.weight, self.children = [None], [None], [None], [[]]

    def add(self, parent, desc, weight=None):
        self.parent.append(parent); self.desc.append(desc); self.weight.append(weight); self.children.append([])
        self.children[parent].append(len(self.parent) - 1)
        return len(self.parent) - 1

    def arrays(self):
        order = [0]
        for nd in order:
            order.extend(self.children[nd])
        new = {old: i for i, old in enumerate(order)}
        parent = [new[self.parent[o]] for o in order[1:]]
        leaf = [0 if self.children[o] else 1 for o in order[1:]]
        desc = np.array([self.desc[o] for o in order[1:]], np.uint8)
        weight = [0.0 if self.children[o] else (1.0 + 0.125 * (new[o] % 9) if self.weight[o] is None else self.weight[o])
                  for o in order[1:]]
        return self.k, self.L, parent, leaf, desc, np.array(weight)


def _wide(k):
    """Root with k children; below, child i of a node has (i % k) + 1 children, so most nodes leave
    lanes without a child.  Child i at level l carries block (i + l - 1) % 20."""
    L = 3 if k == 2 else 2
    t = Tree(k, L)

    def grow(nd, level, cnt):
        for i in range(cnt):
            c = t.add(nd, D(blk((i + level - 1) % 20)), 0.0 if level == L and (i + nd) % 7 == 3 else None)
            if level < L:
                grow(c, level + 1, (i % k) + 1)
    grow(0, 1, k)
    return t.arrays()


def wide_queries(k):
    """One strict winner per root child, then for every pair j < j' a query as far from both and
    farther from the rest: half of each block."""
    q = [D(blk(j)) for j in range(k)]
    q += [D(blk(j, BLK // 2), blk(jj, BLK // 2)) for j in range(k) for jj in range(j + 1, k)]
    return np.array(q)


def _complement(k):
    """L = 3.  Root: A, B, C.  A has the single child X = ~qA (an inner node: the walk has to
    descend into it); B has three leaves, all ~qB; C has k leaves, all ~qC."""
    t = Tree(k, 3)
    qa, qb, qc = complement_queries()
    a, b, c = t.add(0, D()), t.add(0, D(blk(0))), t.add(0, D(blk(1)))
    x = t.add(a, ~qa)
    t.add(x, D()); t.add(x, D(blk(3)))
    for _ in range(3):
        t.add(b, ~qb)
    for _ in range(k):
        t.add(c, ~qc)
    return t.arrays()


def complement_queries():
    return np.array([D([250]), D(blk(0), [251]), D(blk(1), [252])])


def _level1(k):
    t = Tree(k, 1)
    for j in range(k):
        t.add(0, D(blk(j)), 0.0 if j == 1 else None)
    return t.arrays()


def _chain():
    """k = 2, L = 10: one chain, the other child a leaf at each level (the chain child is child 0
    at odd levels, child 1 at even ones).  The chain children are all zero, the leaf of level l
    carries block l - 1."""
    t = Tree(2, 10)
    nd = 0
    for level in range(1, 11):
        pair = [(D(), True), (D(blk(level - 1)), False)]
        if level % 2 == 0:
            pair.reverse()
        ids = [t.add(nd, d) for d, _ in pair]
        nd = ids[0] if pair[0][1] else ids[1]
    return t.arrays()


def chain_queries():
    """All zero (10 levels deep); block e - 1 (leaves the chain at level e); half of block e - 1
    (a tie at level e: the first child wins, the chain at odd e, the leaf at even e)."""
    q = [D()] + [D(blk(e - 1)) for e in range(1, 11)] + [D(blk(e - 1, BLK // 2)) for e in range(1, 11)]
    return np.array(q)


DEPTH_PATHS = ((0,), (1, 3), (1, 4, 6), (1, 4, 5, 7), (1, 4, 5, 8), (1, 4, 5, 9), (2, 10), (2, 11))


def _depth():
    """k = 3, L = 4, leaves at depths 1, 2, 3 and 4; node names are block numbers (DEPTH_PATHS)."""
    t = Tree(3, 4)
    n = {}
    for path in DEPTH_PATHS:
        for i, b in enumerate(path):
            if b not in n:
                n[b] = t.add(n[path[i - 1]] if i else 0, D(blk(b)), 0.0 if b == 11 else None)
    return t.arrays()


def depth_queries():
    return np.array([D(*[blk(b) for b in path]) for path in DEPTH_PATHS])


GRID_BITS = 5


def _grid():
    """k = 16, L = 3, 4096 leaves; child i at level l carries 5 bits at 80 (l - 1) + 5 i, so a
    descriptor chooses its leaf level by level.  Leaf 4095 has weight 0."""
    t = Tree(16, 3)
    level = [0]
    for lv in range(3):
        nxt = []
        for nd in level:
            for i in range(16):
                nxt.append(t.add(nd, D(range(80 * lv + GRID_BITS * i, 80 * lv + GRID_BITS * i + GRID_BITS)),
                                 0.0 if lv == 2 and len(nxt) == 4095 else None))
        level = nxt
    return t.arrays()


def grid_desc(labels):
    """The descriptor that walks to leaf t of the grid (t = -1: leaf 4095, whose weight is 0)."""
    out = np.zeros((len(labels), 32), np.uint8)
    for n, t in enumerate(labels):
        t = 4095 if t < 0 else int(t)
        out[n] = D(*[range(80 * lv + GRID_BITS * i, 80 * lv + GRID_BITS * i + GRID_BITS)
                     for lv, i in enumerate((t >> 8, (t >> 4) & 15, t & 15))])
    return out


@functools.lru_cache(maxsize=None)
def voc_args(name):
    kind, _, k = name.partition("_k")
    make = dict(wide=_wide, complement=_complement, level1=_level1)
    if kind in make:
        return make[kind](int(k))
    return dict(chain=_chain, depth=_depth, grid=_grid)[name]()


@functools.lru_cache(maxsize=None)
def voc_ref(name):
    return R.Voc(*voc_args(name))


@functools.lru_cache(maxsize=None)
def _walk(voc, desc_bytes, levelsup, mut):
    """The reference's walk of one descriptor, once per distinct descriptor (the CSR cases repeat them)."""
    return voc_ref(voc).transform(np.frombuffer(desc_bytes, np.uint8), levelsup, mut)


# ---------------------------------------------------------------- node arrays for the CSR
def _scatter(sorted_labels, step=7):
    """The labels at indices i * step % n: a node's features are spread over the whole array."""
    n = len(sorted_labels)
    assert np.gcd(step, n) == 1
    out = np.empty(n, np.int64)
    out[(np.arange(n) * step) % n] = sorted_labels
    return out


@functools.lru_cache(maxsize=None)
def csr_labels(name):
    """-> (labels: node per feature or -1, valid mask or None)"""
    if name == "n1":
        return np.array([7]), None
    if name == "all_minus":
        return np.full(70, -1), None
    if name.startswith("one_node_"):
        return np.full(int(name[9:]), 5), None
    if name.startswith("distinct_"):
        _, n, way = name.split("_")
        lab = np.arange(int(n))
        return (lab if way == "asc" else lab[::-1].copy()), None
    if name == "runs":              # run lengths 1 .. 9 cycling: heads on every residue mod 4
        lab = np.concatenate([np.full(r % 9 + 1, 3 * r + 2) for r in range(400)])[:1100]
        return _scatter(lab), None
    if name == "valid_mask":        # a whole node, and the first and the last feature of a node, masked out
        lab = np.concatenate([np.full(r % 9 + 1, 3 * r + 2) for r in range(30)])
        lab = _scatter(lab[:149])
        valid = np.ones(len(lab), np.uint8)
        valid[lab == 3 * 4 + 2] = 0
        for nd in (3 * 7 + 2, 3 * 8 + 2):
            idx = np.flatnonzero(lab == nd)
            valid[idx[0 if nd == 23 else -1]] = 0
        return lab, valid
    if name == "sparse_4095":       # 40 listed features among 4095
        lab = np.full(4095, -1)
        at = [0, 4094] + [97 * i + 13 for i in range(1, 39)]
        lab[at] = [3 + (i % 6) for i in range(40)]
        return lab, None
    raise KeyError(name)


CSR_TRANSFORM = ("n1", "all_minus", "one_node_4095", "distinct_1025_asc", "distinct_1025_desc", "distinct_4095_asc",
                 "distinct_4095_desc", "runs", "sparse_4095")
CSR_MATCH = ("n1", "all_minus", "one_node_300", "distinct_1025_asc", "distinct_1025_desc", "distinct_4095_asc",
             "distinct_4095_desc", "runs", "valid_mask", "sparse_4095")


def csr_facts(name):
    lab, valid = csr_labels(name)
    node, off, idx = R.csr(lab, valid)
    heads = off[:-1]
    return dict(n=len(lab), m=len(idx), nd=len(node), head_residues=sorted(set(int(h) % 4 for h in heads)),
                run_over_1024=any(a < 1024 <= b - 1 for a, b in zip(off[:-1], off[1:])),
                node_over_index_1024=any(idx[a] < 1024 <= idx[b - 1] for a, b in zip(off[:-1], off[1:])),
                second_trip=len(lab) > 1024)


# ---------------------------------------------------------------- transform cases
def transform_names():
    names = ["wide_k%d" % k for k in WIDE_K] + ["complement_k3", "complement_k17", "level1_k16", "level1_k20", "chain"]
    names += ["depth_ls%d" % ls for ls in (0, 1, 3, 4, 7)]
    names += ["count_k%d_n%d" % (k, n) for k in (17, 16) for n in COUNTS]
    return names + ["csr_" + nm for nm in CSR_TRANSFORM]


@functools.lru_cache(maxsize=None)
def transform_case(name):
    """-> (vocabulary name, descriptors, levelsup)"""
    if name.startswith("wide_k"):
        return name, wide_queries(int(name[6:])), 1
    if name.startswith("complement_k"):
        return name, complement_queries(), 1
    if name.startswith("level1_k"):
        return name, wide_queries(int(name[8:])), 0
    if name == "chain":
        return "chain", chain_queries(), 4
    if name.startswith("depth_ls"):
        return "depth", depth_queries(), int(name[8:])
    if name.startswith("count_k"):
        k, n = (int(x) for x in name[7:].split("_n"))
        return "wide_k%d" % k, wide_queries(k)[::3][:n], 1
    if name.startswith("csr_"):
        return "grid", grid_desc(csr_labels(name[4:])[0]), 0
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def transform_ref(name, mut=frozenset()):
    """bow_ref.compute_bow's result (tests/test_bow_cases.py compares the two), put together from
    one reference walk per distinct descriptor and the reference's CSR of the node array."""
    voc, desc, levelsup = transform_case(name)
    walks = [_walk(voc, d.tobytes(), levelsup, mut) for d in desc]
    word = np.array([w for w, _, _ in walks], np.int32).reshape(-1)
    weight = np.array([wt for _, wt, _ in walks], np.float64).reshape(-1)
    node = np.array([nid if wt > 0 else -1 for _, wt, nid in walks], np.int32).reshape(-1)
    fv_node, fv_off, fv_idx = R.csr(node, None, mut)
    return dict(word=word, node=node, weight=weight, fv_node=fv_node, fv_off=fv_off, fv_idx=fv_idx)


def transform_traces(name):
    voc, desc, levelsup = transform_case(name)
    out = []
    for d in desc:
        tr = []
        voc_ref(voc).transform(d, levelsup, trace=tr)
        out.append(tr)
    return out


def transform_facts(name):
    """What the reference's walks over the case's descriptors met."""
    voc, desc, levelsup = transform_case(name)
    ref, traces = voc_ref(voc), transform_traces(name)
    want = transform_ref(name)
    root = [tr[0] for tr in traces]
    strict, pairs = set(), set()
    for _, dist, win in root:
        low = [j for j, x in enumerate(dist) if x == min(dist)]
        if len(low) == 1:
            strict.add(win)
        elif len(low) == 2 and win == low[0]:
            pairs.add(tuple(low))
    dp = depths(ref)
    leaves = [ref.word_node[w] for w in want["word"]]
    # lanes, workgroups: launch_transform's choice (coeb_bow.hip): G = 16 lanes per descriptor up to
    # k = 16, else 32, and kBowThreads = 256 threads, so 256 / G descriptors per workgroup
    return dict(k=ref.k, L=ref.L, lanes=16 if ref.k <= 16 else 32, n=len(desc), strict=strict, pairs=pairs,
                min_children=min(len(ch) for ch in ref.children if ch),
                all_256=sorted(len(d) for tr in traces for _, d, _ in tr if set(d) == {256}),
                descended_256=any(set(d) == {256} and i + 1 < len(tr) for tr in traces for i, (_, d, _) in enumerate(tr)),
                walk_depths=sorted(set(len(tr) for tr in traces)), leaf_depths=sorted(set(dp[nd] for nd in leaves)),
                minus_one=int((want["node"] < 0).sum()), nodes=sorted(set(int(x) for x in want["node"])),
                leaf_is_nid=sum(1 for i, nd in enumerate(leaves) if want["node"][i] == nd and dp[nd] < ref.L - levelsup),
                workgroups=-(-len(desc) // (256 // (16 if ref.k <= 16 else 32))))


# ================================================================ SearchByBoW scenes
class Scene:
    """KeyFrame side and frame side; one node per sub-case, a node's features consecutive on both
    sides, so a frame feature's list position is its rank among the sub-case's frame features."""

    def __init__(self):
        self.kf, self.cur, self.sub = [], [], {}

    def node(self, name, kf, cur):
        """kf: [(descriptor, valid, angle)], cur: [(descriptor, angle)]; both may give the descriptor only."""
        nd = 10 + 7 * len(self.sub)
        k0, c0 = len(self.kf), len(self.cur)
        for e in kf:
            e = e if isinstance(e, tuple) else (e, 1, 0.0)
            self.kf.append((nd,) + tuple(e))
        for e in cur:
            e = e if isinstance(e, tuple) else (e, 0.0)
            self.cur.append((nd,) + tuple(e))
        self.sub[name] = dict(node=nd, kf=list(range(k0, len(self.kf))), cur=list(range(c0, len(self.cur))))

    def arrays(self):
        return dict(valid=np.array([e[2] for e in self.kf], np.uint8),
                    kf_desc=np.array([e[1] for e in self.kf], np.uint8).reshape(-1, 32),
                    kf_node=np.array([e[0] for e in self.kf], np.int32),
                    kf_angle=np.array([e[3] for e in self.kf], np.float32),
                    cur_desc=np.array([e[1] for e in self.cur], np.uint8).reshape(-1, 32),
                    cur_node=np.array([e[0] for e in self.cur], np.int32),
                    cur_angle=np.array([e[2] for e in self.cur], np.float32), sub=self.sub)


FILL = D(range(100, 160))                   # 60 bits from the zero descriptor: never within TH_LOW
CHAIN = (0, 1, 3, 7, 15, 31)                # d[i] < 0.6 d[i + 1] and d <= 50


def far(d, at=0):
    return D(range(at, at + d))


def _list_with(length, at):
    """A frame list of FILL with the given {position: descriptor}."""
    return [at.get(p, FILL) for p in range(length)]


def _scene_lists():
    """Per length: KeyFrame feature A (zero) has its unique best (3 bits) in the last position,
    B its best (1 bit off) in position 0.  Lengths up to 128 sit in LDS, longer ones are read
    from global memory; 64 / 65 and 128 / 129 and 192 / 193 are the trip edges of a lane."""
    s = Scene()
    first = D(range(200, 210))
    for n in LIST_LENGTHS:
        s.node("len%d" % n, [D(), D(range(200, 210), [250])], _list_with(n, {0: first, n - 1: far(3)}))
    return s


def _scene_lanes():
    """Lists of 130.  best / second-best in one lane (p, p + 64) and in two, in both orders, accepted
    (2 against 10) and rejected (8 against 10); equal bests in one lane and in two."""
    s = Scene()
    for tag, p1, p2 in (("same_lane", 5, 69), ("diff_lane", 5, 70), ("same_lane_rev", 69, 5), ("diff_lane_rev", 70, 3)):
        s.node(tag + "_acc", [D()], _list_with(130, {p1: far(2), p2: far(10, 50)}))
        s.node(tag + "_rej", [D()], _list_with(130, {p1: far(8), p2: far(10, 50)}))
    s.node("tie_one_lane", [D()], _list_with(130, {5: far(4), 69: far(4, 50)}))
    s.node("tie_two_lanes", [D()], _list_with(130, {5: far(4), 70: far(4, 50)}))
    return s


def _scene_edges():
    """(d1, b2) per node, in both list orders; b2 = 256: a list of one."""
    s = Scene()
    for d1, b2 in EDGE_PAIRS:
        cur = [far(d1)] + ([far(b2, 128)] if b2 < 256 else [])
        s.node("e%d_%d" % (d1, b2), [D()], cur)
        s.node("e%d_%d_rev" % (d1, b2), [D()], cur[::-1])
    for m in range(1, 6):                     # 0.7 b2 = d1 in the rationals
        s.node("seven_tenths_%d" % m, [D()], [far(7 * m), far(10 * m, 128)])
    return s


def _scene_chains():
    """c + 1 equal KeyFrame features against a list of c at CHAIN's distances: each takes the
    best that is left, the last finds everything taken (b1 stays 256).  chain130: the accepted
    positions 129, 65, 1 set the bits of trips 2, 1, 0 of lane 1."""
    s = Scene()
    for c in (1, 2, 3, 6):
        s.node("full%d" % c, [D()] * (c + 1), [far(d) for d in CHAIN[:c]][::-1])
    s.node("chain130", [D()] * 5, _list_with(130, {129: far(0), 65: far(1), 1: far(3)}))
    return s


def _scene_big_list():
    """One list of 4095 against 40 equal KeyFrame features: position 4094 (bit 63 of lane 62) goes
    first and is every later feature's best over the whole list."""
    s = Scene()
    at = dict(zip((4094, 2047, 64, 0, 4032, 63), (far(d) for d in CHAIN)))
    s.node("big", [D()] * 40, _list_with(4095, at))
    return s


def _scene_big_kf():
    s = Scene()
    s.node("big", [D()] * 4095, [far(3), far(0), far(1)])
    return s


def _pairs(s, pairs):
    """One accepted pair (equal descriptors) per node: (name, KeyFrame angle, frame angle)."""
    for name, ka, ca in pairs:
        s.node(name, [(D(), 1, ka)], [(D(), ca)])
    return s


def _scene_rot(max1):
    """Bins: round(100 / 30) = 3 holds max1 pairs, 7 holds 5, 10 holds 3 -- on the 0.1 max1 edge
    at max1 = 30 (3 < 0.1f * 30 is false: kept), below it at 31 -- and bin 5 holds one, which goes."""
    return _pairs(Scene(), [("a%d" % i, 100.0 + i, float(i)) for i in range(max1)] +
                  [("b%d" % i, 200.0, 0.0) for i in range(5)] + [("c%d" % i, 300.0, 0.0) for i in range(3)] +
                  [("lone", 150.0, 0.0)])


# The rotation bin decides who survives: in each scene the bin a special angle belongs to is one of
# the three kept maxima (four ordinary pairs hold it) and the bin a wrong reading gives is not.
ROT_SCENES = dict(
    # 15 / 30 and 135 / 30 are exactly .5 and 4.5 in float32: round() gives 1 and 5, rint() or a
    # cast 0 and 4.  10 - 350 and 100 - 190 are negative: + 360 gives bins 1 and 9, without it no bin.
    rot_half=dict(kept=(1, 5, 9), special=dict(half15=(15.0, 0.0), half135=(135.0, 0.0), negative20=(10.0, 350.0),
                                               negative270=(100.0, 190.0)), gone=()),
    # 45 / 30 is 1.5000001 and 44.999996 / 30 exactly 1.5: bin 2 (a cast gives 1); 358 .. 359.99 stay
    # in bin 12, which HISTO_LENGTH = 30 never wraps: bin 0's three pairs stay a fourth maximum
    rot_wrap=dict(kept=(2, 7, 12), special=dict(half45=(45.0, 0.0), half45_below=(44.999996, 0.0),
                                                below360=(359.99, 0.0), below360_b=(359.9, 0.0), below360_c=(359.5, 0.0),
                                                below360_d=(358.0, 0.0)),
                  gone=dict(zero_a=(50.0, 50.0), zero_b=(53.0, 50.0), zero_c=(58.0, 50.0))),
    # equal angles: rot = 0 is not negative and stays in bin 0 (with + 360 it would be alone in bin 12)
    rot_zero=dict(kept=(0, 4, 8), special=dict(zero=(77.0, 77.0), zero360=(0.0, 0.0)), gone=()))


def _scene_rot_bins(name):
    sc = ROT_SCENES[name]
    pairs = [(tag, ka, ca) for tag, (ka, ca) in sc["special"].items()]
    pairs += [(tag, ka, ca) for tag, (ka, ca) in dict(sc["gone"]).items()]
    for b in sc["kept"]:
        if not (name == "rot_wrap" and b == 12):           # the four below360 pairs hold bin 12 themselves
            pairs += [("bin%d_%d" % (b, i), 30.0 * b + 3.0 * i + 1.0 + 20.0, 20.0) for i in range(4)]
    return _pairs(Scene(), pairs)


@functools.lru_cache(maxsize=None)
def _csr_scene(name):
    """The node array on the KeyFrame side (with its valid mask) and reversed on the frame side;
    every KeyFrame descriptor zero, every frame descriptor one bit off.  Run at nnratio 1.5, each
    KeyFrame feature takes the first frame feature of its node that is left, so the matches spell
    out both CSR orders."""
    lab, valid = csr_labels(name)
    n = len(lab)
    kf_node = np.where(lab >= 0, 3 * lab + 1, -1).astype(np.int32)
    z = np.zeros(n, np.float32)
    return dict(valid=np.ones(n, np.uint8) if valid is None else valid, kf_desc=np.zeros((n, 32), np.uint8),
                kf_node=kf_node, kf_angle=z, cur_desc=np.tile(D([0]), (n, 1)), cur_node=kf_node[::-1].copy(),
                cur_angle=z, sub={})


SCENES = dict(lists=_scene_lists, lanes=_scene_lanes, edges=_scene_edges, chains=_scene_chains, big_list=_scene_big_list,
              big_kf=_scene_big_kf, rot30=lambda: _scene_rot(30), rot31=lambda: _scene_rot(31),
              **{nm: functools.partial(_scene_rot_bins, nm) for nm in ROT_SCENES})
# (scene, nnratio, check_ori) of every directed matcher run
MATCH_RUNS = ([(s, r, False) for s in ("lists", "lanes", "edges", "chains") for r in (0.6, 0.7)] +
              [("lanes", 1.5, False), ("big_list", 0.7, False), ("big_kf", 0.7, False), ("rot30", 0.7, True),
               ("rot31", 0.7, True), ("rot30", 0.7, False)] + [(nm, 0.7, True) for nm in ROT_SCENES] + [("csr_" + nm, 1.5, False) for nm in CSR_MATCH])
FUSED_RUNS = (("lanes", 0.7, False), ("chains", 0.6, False), ("rot_half", 0.7, True))      # also through the fused call


@functools.lru_cache(maxsize=None)
def scene(name):
    return _csr_scene(name[4:]) if name.startswith("csr_") else SCENES[name]().arrays()


def scene_args(m):
    return m["valid"], m["kf_desc"], m["kf_node"], m["kf_angle"], m["cur_desc"], m["cur_node"], m["cur_angle"]


@functools.lru_cache(maxsize=None)
def match_ref(name, nnratio, check_ori, mut=frozenset()):
    """-> (match, nmatches, stats, trace by KeyFrame feature)"""
    trace = []
    m, nm, st = R.search_by_bow(*scene_args(scene(name)), nnratio, check_ori, mut, trace)
    return m, nm, st, {t["ikf"]: t for t in trace}


def sub_trace(name, nnratio, check_ori, sub):
    """The trace records of one sub-case's KeyFrame features, in order."""
    tr = match_ref(name, nnratio, check_ori)[3]
    return [tr[i] for i in scene(name)["sub"][sub]["kf"] if i in tr]


# ---------------------------------------------------------------- the database form (kValid)
@functools.lru_cache(maxsize=None)
def db_scene():
    """Keyframes by slot, the frame and candidate lists.  Slot 0, node `skip`: KeyFrame features
    a (valid), b (invalid under the first mask; it equals frame feature f1), c (valid, one bit off
    f1): with b skipped c takes f1; were b to claim first, c would find nothing.  Slot 1: two
    features.  Slot 2: none."""
    s = Scene()
    f1 = D(range(50, 60))
    s.node("skip", [D(), (f1, 0, 0.0), D(range(50, 60), [70])], [D([0]), f1])
    s.node("chain", [D()] * 4, [far(d) for d in CHAIN[:3]])
    s.node("edge", [D()], [far(15), far(25, 128)])
    s.node("list65", [D(), (D(range(200, 210), [250]), 0, 0.0)], _list_with(65, {0: D(range(200, 210)), 64: far(3)}))
    m = s.arrays()
    sub = m["sub"]
    tiny = [sub["chain"]["kf"][0], sub["edge"]["kf"][0]]
    kfs = [dict(desc=m["kf_desc"], node=m["kf_node"], angle=m["kf_angle"]),
           dict(desc=m["kf_desc"][tiny], node=m["kf_node"][tiny], angle=m["kf_angle"][tiny]),
           dict(desc=np.zeros((0, 32), np.uint8), node=np.zeros(0, np.int32), angle=np.zeros(0, np.float32))]
    n0 = len(m["valid"])
    ones, zeros, e = np.ones(n0, np.uint8), np.zeros(n0, np.uint8), np.zeros(0, np.uint8)
    t = [np.array(v, np.uint8) for v in ((1, 1), (1, 0), (0, 1), (0, 0))]
    cands = dict(main=[(0, m["valid"]), (0, ones), (0, zeros), (2, e), (1, t[0]), (0, m["valid"])],
                 one=[(0, m["valid"])],
                 most=[((0, m["valid"]), (1, t[0]), (1, t[1]), (2, e), (1, t[2]), (0, ones), (1, t[3]))[j % 7] for j in range(256)])
    cur = dict(desc=m["cur_desc"], node=m["cur_node"], angle=m["cur_angle"])
    return kfs, cur, cands, sub


@functools.lru_cache(maxsize=None)
def db_match_ref(which, nnratio, check_ori, mut=frozenset()):
    kfs, cur, cands, _ = db_scene()
    memo, out = {}, []
    for slot, valid in cands[which]:
        key = (slot, valid.tobytes())
        if key not in memo:
            kf = kfs[slot]
            memo[key] = R.search_by_bow(valid, kf["desc"], kf["node"], kf["angle"], cur["desc"], cur["node"], cur["angle"],
                                        nnratio, check_ori, mut)
        out.append(memo[key])
    return out


# ================================================================ database queries
MAXF = 200


def query_words(nq):
    return [10 * (i + 1) for i in range(nq)]


def kf_words(nw, hits, nq):
    """nw ascending words, those at the positions `hits` among the query's (multiples of 10 up to
    10 nq), the others not."""
    words, cur = [], 0
    for p in range(nw):
        cur += 1
        if p in hits:
            cur = -(-cur // 10) * 10
            assert cur <= 10 * nq, "the query has no word left for position %d" % p
        elif cur % 10 == 0:
            cur += 1
        words.append(cur)
    return words


def bow_of(words, salt):
    return {w: (1 + (w * 7 + salt) % 13) / 63.0 for w in words}


def keyframe(nw, hits, nq, salt):
    return bow_of(kf_words(nw, set(hits), nq), salt)


def _q(bow):
    return ("query", bow)


def _adds(bows):
    return [("add", b) for b in bows]


BLOCK_KFS = ((63, (0, 1, 61, 62)), (64, (0, 1, 62, 63)), (65, (0, 1, 63, 64)), (128, (0, 63, 64, 127)),
             (129, (0, 1, 2, 128)), (200, (5, 70, 135, 199)), (200, (0, 1, 2, 3)), (200, (128, 129, 130, 131)),
             (200, (1, 2, 140, 141)), (200, (199,)), (1, (0,)), (0, ()))


@functools.lru_cache(maxsize=None)
def query_case(name):
    """-> (initial_slots, operations): ("add", bow) | ("erase", slot) | ("clear",) | ("query", bow)"""
    if name.startswith("blocks_q"):
        nq = int(name[8:])
        if nq == 1:                         # the query's one word at keyframe positions 0, 9, 0; absent; no words
            kfs = [keyframe(1, (0,), 1, 1), keyframe(63, (9,), 1, 2), keyframe(200, (0,), 1, 3), keyframe(65, (), 1, 4), {}]
        else:
            kfs = [keyframe(nw, hits, nq, i) for i, (nw, hits) in enumerate(BLOCK_KFS)]
        return 4, _adds(kfs) + [_q(bow_of(query_words(nq), 5))]
    if name.startswith("min_common_"):
        mx = int(name[11:])
        mn = K.min_common_words(mx)
        counts = [mn, mx, mn + 1, 0, mn]
        return 2, _adds([keyframe(20, range(c), 12, i) for i, c in enumerate(counts)]) + [_q(bow_of(query_words(12), 9))]
    lo, hi = keyframe(20, range(2), 12, 1), keyframe(20, range(10), 12, 2)
    F = _q(bow_of(query_words(12), 9))
    if name.startswith("wave_"):            # exactly one wave of the workgroup scores
        return 4, _adds([hi if s == int(name[5:]) else lo for s in range(4)]) + [F]
    if name == "wg1_only":                  # no wave of workgroup 0 scores, one of workgroup 1 does
        return 8, _adds([lo, {}, lo, lo, lo, lo, hi, lo]) + [F]
    if name.startswith("nslots_"):          # the last slot scored, alone in its workgroup
        ns = int(name[7:])
        return 1, _adds([lo] * (ns - 1) + [hi]) + [F]
    if name == "erased_between":
        return 4, _adds([hi, keyframe(20, range(10), 12, 3), keyframe(20, range(10), 12, 4), lo]) + [F, ("erase", 1), F]
    if name == "order_sensitive":
        F_bow, kf_bow = order_sensitive()
        return 2, _adds([kf_bow, dict(kf_bow)]) + [_q(F_bow)]
    if name == "lifecycle":
        kfs = [keyframe(20, range(3 + i % 3), 12, i) for i in range(12)]
        ops = []
        for b in kfs[:9]:                   # initial_slots = 1: the storage grows at the 2nd, 3rd, 5th and 9th add
            ops += [("add", b), F]
        ops += [("erase", 0), ("erase", 8), F, ("add", kfs[9]), ("add", kfs[10]), F, ("clear",), ("add", kfs[11]), F]
        return 1, ops
    raise KeyError(name)


def query_names():
    return (["blocks_q%d" % n for n in (1, 64, MAXF)] + ["min_common_%d" % m for m in MAX_COMMON] +
            ["wave_%d" % w for w in range(4)] + ["wg1_only"] + ["nslots_%d" % n for n in (1, 5, 9)] +
            ["erased_between", "order_sensitive", "lifecycle"])


def order_sensitive():
    """A query and a keyframe of 140 words whose common words' terms are -2 (1 + 2^-24) at the
    first word and -2^-53 at sixteen later ones (3 in the first block of 64, 8 in the second, 5
    in the third).  Added one after the other every small term is lost below half an ulp of the
    sum, which stays -2 (1 + 2^-24): the score is the midpoint of two float32 and rounds to even,
    1.0.  Any order that first gathers small terms ends above the midpoint."""
    big, small = 1.0 + 2.0 ** -24, 2.0 ** -54
    hits = [0, 10, 20, 30] + list(range(64, 72)) + list(range(128, 133))
    words = kf_words(140, set(hits), 64)
    kf = {w: 0.25 for w in words}
    F = {w: 0.125 for w in query_words(64)}
    for j, p in enumerate(hits):
        kf[words[p]] = F[words[p]] = big if j == 0 else small
    return F, kf


def order_sensitive_bits():
    """-> the float32 bits of the score under the reference's order and the three others"""
    F, kf = order_sensitive()
    return {m: int(np.float32(K.l1_score(F, kf, frozenset([m]) if m else frozenset())).view(np.uint32))
            for m in ("", "sum_reversed", "sum_pairwise", "sum_blocks64")}


def expect_query(r, slot_of, nslots):
    """coeb_kfdb_query's outputs from detect_reloc's result; slot_of: KeyFrame id -> slot."""
    common, score = np.zeros(nslots, np.int32), np.full(nslots, -1, np.float32)
    for kf in r["sharing"]:
        common[slot_of[kf.id]] = kf.reloc_words
    for s, kf in r["scored"]:
        score[slot_of[kf.id]] = s
    return dict(common=common, score=score, order=np.array([slot_of[kf.id] for kf in r["sharing"]], np.int32),
                max_common=r["max_common"], min_common=r["min_common"])


@functools.lru_cache(maxsize=None)
def query_ref(name, mut=frozenset()):
    """The operations replayed on the reference with the database's slot rule (the lowest free slot
    first; the slot count is one past the highest slot handed out since the last clear).
    -> per operation: the slot of an add, the expected outputs of a query, else None."""
    _, ops = query_case(name)
    db, at, out = K.Database(), [], []      # at[slot]: the reference KeyFrame or None
    made = 0
    for qid, op in enumerate(ops):
        if op[0] == "add":
            slot = at.index(None) if None in at else len(at)
            kf = K.KeyFrame(made, op[1])
            made += 1
            if slot == len(at):
                at.append(kf)
            else:
                at[slot] = kf
            db.add(kf)
            out.append(slot)
        elif op[0] == "erase":
            db.erase(at[op[1]])
            at[op[1]] = None
            out.append(None)
        elif op[0] == "clear":
            db.clear()
            at = []
            out.append(None)
        else:
            r = K.detect_reloc(op[1], db, qid, lambda kf: [], mut)
            out.append(expect_query(r, {kf.id: s for s, kf in enumerate(at) if kf is not None}, len(at)))
    return out


def query_facts(name):
    """Per keyframe alive at the last query: words, common words per block of 64, whether scored."""
    _, ops = query_case(name)
    ref = query_ref(name)
    last = max(i for i, op in enumerate(ops) if op[0] == "query")
    F = ops[last][1]
    at = {}
    for op, r in zip(ops[:last], ref):
        if op[0] == "add":
            at[r] = op[1]
        elif op[0] == "erase":
            del at[op[1]]
        elif op[0] == "clear":
            at = {}
    want = ref[last]
    kfs = {}
    for slot, bow in at.items():
        keys = sorted(bow)
        kfs[slot] = dict(nw=len(keys), hits=[sum(1 for w in keys[b:b + 64] if w in F) for b in range(0, len(keys), 64)],
                         scored=bool(want["score"][slot] != -1), common=int(want["common"][slot]),
                         first_is_last=bool(keys) and min(set(keys) & set(F), default=None) == keys[-1])
    return dict(nslots=len(want["common"]), nq=len(F), kfs=kfs, max_common=want["max_common"],
                min_common=want["min_common"], order=list(want["order"]),
                scored_slots=[s for s in range(len(want["common"])) if want["score"][s] != -1])
