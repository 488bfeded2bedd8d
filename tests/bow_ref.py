"""CPU reference of the bag-of-words front end, as literal Python / numpy loops:
the ORBvoc.txt parser, TemplatedVocabulary::transform, Frame::ComputeBoW's feature vector and
ORBmatcher::SearchByBoW (src/ORBmatcher.cc:159-288).  DBoW2 itself is not available: this file
restates the specification and tests/test_bow_ref.py pins it on a hand-worked vocabulary."""
import numpy as np

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
TH_LOW = 50
HISTO_LENGTH = 30


def hamming(a, b):
    """DescriptorDistance of one 32-byte descriptor against one or many (== oracle.descriptor_distance)."""
    return _POP[np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))].sum(axis=-1)


# ---------------------------------------------------------------- vocabulary
def voc_text(k, L, parent, is_leaf, desc, weight, scoring=0, weighting=0):
    lines = ["%d %d %d %d" % (k, L, scoring, weighting)]
    for p, lf, d, w in zip(parent, is_leaf, desc, weight):
        lines.append("%d %d %s %r" % (p, lf, " ".join(str(int(b)) for b in d), float(w)))
    return "\n".join(lines) + "\n"


def parse_text(text):
    """-> (k, L, parent, is_leaf, desc, weight); ValueError where coeb_voc_from_text gives COEB_EINVAL."""
    lines = [ln.split() for ln in text.split("\n")]
    lines = [f for f in lines if f]
    if not lines or len(lines[0]) != 4:
        raise ValueError("header")
    k, L, scoring, weighting = (int(x) for x in lines[0])
    if not (2 <= k <= 20 and 1 <= L <= 10 and 0 <= scoring <= 5 and 0 <= weighting <= 3):
        raise ValueError("header range")
    parent, is_leaf, desc, weight = [], [], [], []
    for f in lines[1:]:
        if len(f) != 35:
            raise ValueError("line length")
        p, lf = int(f[0]), int(f[1])
        if not 0 <= p <= len(parent):
            raise ValueError("parent not defined")
        d = [int(x) for x in f[2:34]]
        if min(d) < 0 or max(d) > 255:
            raise ValueError("byte")
        parent.append(p); is_leaf.append(1 if lf > 0 else 0); desc.append(d); weight.append(float(f[34]))
    if not parent:
        raise ValueError("no nodes")
    return k, L, parent, is_leaf, np.array(desc, np.uint8), weight


class Voc:
    """Node ids as in the file: 0 the root, line i defines node i; children in line order."""

    def __init__(self, k, L, parent, is_leaf, desc, weight):
        n = len(parent)
        self.k, self.L = k, L
        self.children = [[] for _ in range(n + 1)]
        self.desc = np.zeros((n + 1, 32), np.uint8)
        self.desc[1:] = np.asarray(desc, np.uint8).reshape(n, 32)
        self.weight = [0.0] + [float(w) for w in weight]
        self.word_of = [-1] * (n + 1)
        self.word_node = []
        depth = [0] * (n + 1)
        for i in range(1, n + 1):
            p = parent[i - 1]
            if not 0 <= p < i or (p > 0 and is_leaf[p - 1]):
                raise ValueError("parent")
            self.children[p].append(i)
            depth[i] = depth[p] + 1
            if len(self.children[p]) > k or depth[i] > L:
                raise ValueError("shape")
            if is_leaf[i - 1]:
                self.word_of[i] = len(self.word_node)
                self.word_node.append(i)
        for i in range(1, n + 1):
            if bool(is_leaf[i - 1]) != (not self.children[i]):
                raise ValueError("leaf flag")
        self.nnodes, self.nwords = n + 1, len(self.word_node)

    def slots(self):
        """The device order: breadth first, a node's children contiguous in their original order."""
        order = [0]
        first = {}
        for s in range(self.nnodes):
            nd = order[s]
            first[nd] = len(order)
            order.extend(self.children[nd])
        return order, first

    def transform(self, d, levelsup):
        """-> (word id, weight, nid) of one descriptor."""
        nid_level = self.L - levelsup
        node, level, nid = 0, 0, 0
        while True:
            level += 1
            ch = self.children[node]
            best, best_d = ch[0], int(hamming(d, self.desc[ch[0]]))
            for c in ch[1:]:
                dd = int(hamming(d, self.desc[c]))
                if dd < best_d:
                    best, best_d = c, dd
            node = best
            if level == nid_level:
                nid = node
            if not self.children[node]:
                break
        if level < nid_level:
            nid = node          # defined here; the reference leaves nid uninitialised
        return self.word_of[node], self.weight[node], nid


def compute_bow(voc, desc, levelsup):
    """Frame::ComputeBoW: word / weight / node per feature (node -1 when the weight is not > 0) and
    the feature vector as a CSR (node ids ascending, feature indices ascending)."""
    n = len(desc)
    word, node, weight = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.float64)
    fv = {}
    for i in range(n):
        w, wt, nid = voc.transform(desc[i], levelsup)
        word[i], weight[i] = w, wt
        if wt > 0:
            node[i] = nid
            fv.setdefault(nid, []).append(i)
    keys = sorted(fv)
    off = np.zeros(len(keys) + 1, np.int32)
    for j, kk in enumerate(keys):
        off[j + 1] = off[j] + len(fv[kk])
    idx = np.array([i for kk in keys for i in fv[kk]], np.int32)
    return dict(word=word, node=node, weight=weight, fv_node=np.array(keys, np.int32), fv_off=off, fv_idx=idx)


def random_voc(k, L, seed, ragged=False, zero_weight=0.0):
    """A random vocabulary in ORBvoc.txt's line order (every parent's children consecutive).
    ragged: four nodes in ten get 1..k-1 children and some nodes at depth >= 2 stay leaves above level L."""
    rng = np.random.RandomState(seed)
    parent, is_leaf, depth = [], [], []
    frontier = [(0, 0)]
    while frontier:
        nxt = []
        for p, dp in frontier:
            nc = int(rng.randint(1, k)) if ragged and rng.rand() < 0.4 else k
            for _ in range(nc):
                parent.append(p); depth.append(dp + 1)
                leaf = dp + 1 == L or (ragged and dp + 1 >= 2 and rng.rand() < 0.15)
                is_leaf.append(1 if leaf else 0)
                if not leaf:
                    nxt.append((len(parent), dp + 1))
        frontier = nxt
    n = len(parent)
    desc = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    weight = rng.uniform(0.1, 5.0, n)
    weight[rng.rand(n) < zero_weight] = 0.0
    weight[np.array(is_leaf) == 0] = 0.0
    return k, L, parent, is_leaf, desc, weight


# ---------------------------------------------------------------- SearchByBoW
def three_maxima(hist):
    """ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:1602-1638)."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(hist):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if max2 < np.float32(0.1) * np.float32(max1):
        ind2 = ind3 = -1
    elif max3 < np.float32(0.1) * np.float32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def feature_vector(node, valid=None):
    fv = {}
    for i, nd in enumerate(node):
        if nd >= 0 and (valid is None or valid[i]):
            fv.setdefault(int(nd), []).append(i)
    return fv


def search_by_bow(kf_valid, kf_desc, kf_node, kf_angle, cur_desc, cur_node, cur_angle, nnratio, check_ori):
    """-> (match [n_cur] KeyFrame index or -1, nmatches, stats).  stats counts what the GPU tests
    require their inputs to exercise: matches the rotation filter removed, accepted KeyFrame
    features whose best frame feature over the whole node had been taken before, and rejections
    with bestDist1 == bestDist2."""
    n = len(cur_desc)
    match = np.full(n, -1, np.int32)
    kf_fv = feature_vector(kf_node)        # mFeatVec lists every feature; validity is checked in the loop
    cur_fv = feature_vector(cur_node)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    nnratio = np.float32(nnratio)
    factor = np.float32(1.0) / np.float32(HISTO_LENGTH)
    nmatches = 0
    stats = dict(rot_removed=0, claim_dependency=0, tie_rejected=0)
    for nd in sorted(kf_fv):
        if nd not in cur_fv:
            continue
        idx_f = cur_fv[nd]
        sub = np.asarray(cur_desc, np.uint8)[idx_f]
        for ikf in kf_fv[nd]:
            if not kf_valid[ikf]:
                continue
            dist = hamming(kf_desc[ikf], sub)
            best1, best_f, best2 = 256, -1, 256
            for j, real in enumerate(idx_f):
                if match[real] >= 0:
                    continue
                d = int(dist[j])
                if d < best1:
                    best2, best1, best_f = best1, d, real
                elif d < best2:
                    best2 = d
            if best1 <= TH_LOW:
                if np.float32(best1) < nnratio * np.float32(best2):
                    first_choice = idx_f[int(np.argmin(dist))]
                    if match[first_choice] >= 0:
                        stats["claim_dependency"] += 1
                    match[best_f] = ikf
                    if check_ori:
                        rot = np.float32(kf_angle[ikf]) - np.float32(cur_angle[best_f])
                        if rot < 0.0:
                            rot = np.float32(rot + np.float32(360.0))
                        fb = float(np.float32(rot * factor))          # C round(): halves away from zero
                        b = int(np.floor(fb + 0.5)) if fb >= 0 else -int(np.floor(-fb + 0.5))
                        if b == HISTO_LENGTH:
                            b = 0
                        assert 0 <= b < HISTO_LENGTH
                        rot_hist[b].append(best_f)
                    nmatches += 1
                elif best1 == best2:
                    stats["tie_rejected"] += 1
    if check_ori:
        keep = three_maxima([len(h) for h in rot_hist])
        for b in range(HISTO_LENGTH):
            if b in keep:
                continue
            for f in rot_hist[b]:
                match[f] = -1
                nmatches -= 1
                stats["rot_removed"] += 1
    return match, nmatches, stats
