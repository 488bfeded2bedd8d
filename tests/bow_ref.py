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

    def transform(self, d, levelsup, mut=frozenset(), trace=None):
        """-> (word id, weight, nid) of one descriptor.  trace: a list that receives, per level,
        (node, the distances to its children, the index of the child taken).  mut: MUTATIONS."""
        nid_level = self.L - levelsup - ("nid_level_off" in mut)
        node, level, nid = 0, 0, 0
        while True:
            level += 1
            ch = self.children[node]
            if mut & {"tie_last", "tie_15_16_lost", "sentinel_256"}:
                best = _mutated_child(ch, [int(hamming(d, self.desc[c])) for c in ch], mut)
                if best is None:                # no child beat the sentinel: the walk ends without a word
                    return -1, 0.0, -1
            else:
                best, best_d = ch[0], int(hamming(d, self.desc[ch[0]]))
                for c in ch[1:]:
                    dd = int(hamming(d, self.desc[c]))
                    if dd < best_d:
                        best, best_d = c, dd
            if trace is not None:
                trace.append((node, [int(hamming(d, self.desc[c])) for c in ch], ch.index(best)))
            node = best
            if level == nid_level:
                nid = node
            if not self.children[node]:
                break
        if level < nid_level:
            nid = node          # defined here; the reference leaves nid uninitialised
        return self.word_of[node], self.weight[node], nid


def _mutated_child(ch, dist, mut):
    """The child a wrong reading of the walk takes (tests/test_bow_cases.py shows that the directed
    vocabularies notice each): tie_last -- the last of equal children wins; tie_15_16_lost -- each
    row of 16 children keeps its first minimum, but the second row wins an equal first row;
    sentinel_256 -- a child has to be closer than 256 to be taken at all."""
    def first_min(idx):
        b = idx[0]
        for j in idx[1:]:
            if dist[j] < dist[b] or ("tie_last" in mut and dist[j] == dist[b]):
                b = j
        return b
    idx = list(range(len(ch)))
    if "tie_15_16_lost" in mut and len(ch) > 16:
        a, b = first_min(idx[:16]), first_min(idx[16:])
        j = b if dist[b] <= dist[a] else a
    else:
        j = first_min(idx)
    if "sentinel_256" in mut and dist[j] >= 256:
        return None
    return ch[j]


MUTATIONS = ("tie_last", "tie_15_16_lost", "sentinel_256", "nid_level_off", "ratio_le", "ratio_f64", "ratio_f64_of_f32",
             "d1_lt_50", "taken_ignored", "taken_trip0_only", "b2_min_only", "invalid_claims", "csr_first_1024",
             "rot_half_even", "rot_truncated", "rot_no_360", "rot_wrap_12", "rot_le_zero")


def _fv_order(idx, mut):
    """A node's features in list order; csr_first_1024: ascending only among the first 1024."""
    if "csr_first_1024" in mut:
        return [i for i in idx if i >= 1024] + [i for i in idx if i < 1024]
    return idx


def compute_bow(voc, desc, levelsup, mut=frozenset()):
    """Frame::ComputeBoW: word / weight / node per feature (node -1 when the weight is not > 0) and
    the feature vector as a CSR (node ids ascending, feature indices ascending)."""
    n = len(desc)
    word, node, weight = np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.float64)
    fv = {}
    for i in range(n):
        w, wt, nid = voc.transform(desc[i], levelsup, mut)
        word[i], weight[i] = w, wt
        if wt > 0:
            node[i] = nid
            fv.setdefault(nid, []).append(i)
    for kk in fv:
        fv[kk] = _fv_order(fv[kk], mut)
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


def feature_vector(node, valid=None, mut=frozenset()):
    fv = {}
    for i, nd in enumerate(node):
        if nd >= 0 and (valid is None or valid[i]):
            fv.setdefault(int(nd), []).append(i)
    for nd in fv:
        fv[nd] = _fv_order(fv[nd], mut)
    return fv


def csr(node, valid=None, mut=frozenset()):
    """The feature vector of a plain node array as coeb_bow_transform returns it."""
    fv = feature_vector(node, valid, mut)
    keys = sorted(fv)
    off = np.cumsum([0] + [len(fv[kk]) for kk in keys]).astype(np.int32)
    return np.array(keys, np.int32), off, np.array([i for kk in keys for i in fv[kk]], np.int32)


def _accepts(best1, best2, nnratio, mut):
    """bestDist1 <= TH_LOW and float(bestDist1) < mfNNratio * bestDist2, the product in float32."""
    if not (best1 < TH_LOW if "d1_lt_50" in mut else best1 <= TH_LOW):
        return False
    if "ratio_f64" in mut:                 # the caller's ratio as a double, the product in double
        return float(best1) < float(nnratio) * float(best2)
    if "ratio_f64_of_f32" in mut:          # the float32 ratio the matcher holds, the product in double
        return float(best1) < float(np.float32(nnratio)) * float(best2)
    r = np.float32(nnratio) * np.float32(best2)
    return np.float32(best1) <= r if "ratio_le" in mut else np.float32(best1) < r


def _rot_bin(a_kf, a_cur, factor, mut):
    """rot = angle difference, + 360 when negative; bin = round(rot * factor), HISTO_LENGTH -> 0
    (:237-244).  The wrong readings: rot_half_even (rint), rot_truncated ((int)), rot_no_360,
    rot_wrap_12 (the bin of 360 degrees, 12, wraps instead of HISTO_LENGTH), rot_le_zero (<= 0)."""
    rot = np.float32(a_kf) - np.float32(a_cur)
    if (rot <= 0.0 if "rot_le_zero" in mut else rot < 0.0) and "rot_no_360" not in mut:
        rot = np.float32(rot + np.float32(360.0))
    fb = float(np.float32(rot * factor))
    if "rot_half_even" in mut:
        b = int(np.rint(fb))
    elif "rot_truncated" in mut:
        b = int(fb)
    else:                                  # C round(): halves away from zero
        b = int(np.floor(fb + 0.5)) if fb >= 0 else -int(np.floor(-fb + 0.5))
    if b == (12 if "rot_wrap_12" in mut else HISTO_LENGTH):
        b = 0
    if "rot_no_360" in mut and not 0 <= b < HISTO_LENGTH:
        return HISTO_LENGTH
    assert 0 <= b < HISTO_LENGTH
    return b


def search_by_bow(kf_valid, kf_desc, kf_node, kf_angle, cur_desc, cur_node, cur_angle, nnratio, check_ori,
                  mut=frozenset(), trace=None):
    """-> (match [n_cur] KeyFrame index or -1, nmatches, stats).  stats counts what the GPU tests
    require their inputs to exercise: matches the rotation filter removed, accepted KeyFrame
    features whose best frame feature over the whole node had been taken before, and rejections
    with bestDist1 == bestDist2.
    trace: a list that receives one dict per valid KeyFrame feature that meets a frame list -- ikf,
    node, len (of the list), d1, b2, p1 / p2 (list positions of the best and of the first
    second-best, -1: none), accepted, first_taken (the best over the whole list had been given
    away), bin (the rotation bin of an accepted match, else -1).
    mut: MUTATIONS, the wrong readings tests/test_bow_cases.py shows the directed scenes notice."""
    n = len(cur_desc)
    match = np.full(n, -1, np.int32)
    kf_fv = feature_vector(kf_node, None, mut)   # mFeatVec lists every feature; validity is checked in the loop
    cur_fv = feature_vector(cur_node, None, mut)
    rot_hist = [[] for _ in range(HISTO_LENGTH + 1)]     # [HISTO_LENGTH]: no bin (rot_no_360 only), never kept
    ratio_arg, nnratio = nnratio, np.float32(nnratio)
    factor = np.float32(1.0) / np.float32(HISTO_LENGTH)
    nmatches = 0
    stats = dict(rot_removed=0, claim_dependency=0, tie_rejected=0)
    ghost = set()                          # invalid_claims: frame features an invalid KeyFrame feature took
    for nd in sorted(kf_fv):
        if nd not in cur_fv:
            continue
        idx_f = cur_fv[nd]
        sub = np.asarray(cur_desc, np.uint8)[idx_f]
        for ikf in kf_fv[nd]:
            if not kf_valid[ikf] and "invalid_claims" not in mut:
                continue
            dist = hamming(kf_desc[ikf], sub)
            best1, best_f, best2 = 256, -1, 256
            p1 = p2 = -1
            lane_b2 = {}                   # b2_min_only: the second-best of the positions p, p + 64, ..
            for j, real in enumerate(idx_f):
                taken = match[real] >= 0 or real in ghost
                if "taken_ignored" in mut or ("taken_trip0_only" in mut and j >= 64):
                    taken = False
                if taken:
                    continue
                d = int(dist[j])
                if "b2_min_only" in mut:
                    lb1, lb2 = lane_b2.get(j % 64, (256, 256))
                    lane_b2[j % 64] = (d, lb1) if d < lb1 else (lb1, min(lb2, d))
                if d < best1:
                    best2, best1, best_f = best1, d, real
                    p2, p1 = p1, j
                elif d < best2:
                    best2, p2 = d, j
            if "b2_min_only" in mut:
                best2 = min([b for _, b in lane_b2.values()] + [256])
            rec = dict(ikf=ikf, node=nd, len=len(idx_f), d1=best1, b2=best2, p1=p1, p2=p2, accepted=False,
                       first_taken=bool(match[idx_f[int(np.argmin(dist))]] >= 0), bin=-1)
            if trace is not None and kf_valid[ikf]:
                trace.append(rec)
            if not kf_valid[ikf]:          # invalid_claims only: it takes the frame feature and is skipped then
                if _accepts(best1, best2, ratio_arg, mut):
                    ghost.add(best_f)
                continue
            if _accepts(best1, best2, ratio_arg, mut):
                rec["accepted"] = True
                first_choice = idx_f[int(np.argmin(dist))]
                if match[first_choice] >= 0:
                    stats["claim_dependency"] += 1
                match[best_f] = ikf
                if check_ori:
                    b = _rot_bin(kf_angle[ikf], cur_angle[best_f], factor, mut)
                    rot_hist[b].append(best_f)
                    rec["bin"] = b
                nmatches += 1
            elif best1 <= TH_LOW and best1 == best2:
                stats["tie_rejected"] += 1
    if check_ori:
        keep = three_maxima([len(h) for h in rot_hist[:HISTO_LENGTH]])
        for b in range(HISTO_LENGTH + 1):
            if b in keep:
                continue
            for f in rot_hist[b]:
                match[f] = -1
                nmatches -= 1
                stats["rot_removed"] += 1
    return match, nmatches, stats
