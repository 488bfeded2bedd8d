"""CPU reference of the keyframe database, as literal Python: DBoW2's
BowVector::addWeight / normalize(L1), L1Scoring::score, KeyFrameDatabase's inverted file with add and
erase (src/KeyFrameDatabase.cc:40-73) and DetectRelocalizationCandidates (:199-309).  DBoW2 itself
is not available: this file restates the definitions and tests/test_kfdb_ref.py pins it on a
hand-worked case.  Python floats are IEEE doubles and `+=` on them is the sequential double add the
definitions ask for."""
import numpy as np


def bow_vector(word, weight, node, normalize_l1=True):
    """-> dict word -> value.  addWeight over the features with node >= 0 in feature order
    (present: value += v, else insert v), then normalize(L1): norm = sum of fabs(value) in
    ascending word order; if norm > 0.0 every value /= norm."""
    bv = {}
    for w, v, nd in zip(word, weight, node):
        if nd < 0:
            continue
        w, v = int(w), float(v)
        if w in bv:
            bv[w] += v
        else:
            bv[w] = v
    if normalize_l1:
        norm = 0.0
        for w in sorted(bv):
            norm += abs(bv[w])
        if norm > 0.0:
            for w in bv:
                bv[w] /= norm
    return bv


MUTATIONS = ("min_common_f64", "common_ge", "sum_reversed", "sum_pairwise", "sum_blocks64", "carry_zero_block")


def pairwise(t):
    """A balanced tree over the terms: the halves summed first, then added."""
    if len(t) <= 1:
        return t[0] if t else 0.0
    return pairwise(t[:len(t) // 2]) + pairwise(t[len(t) // 2:])


def score_terms(v, w):
    """-> per 64 words of w in ascending order (the device's unit of work) the list of the
    common words' terms fabs(vi - wi) - fabs(vi) - fabs(wi)."""
    keys = sorted(w)
    return [[abs(v[k] - w[k]) - abs(v[k]) - abs(w[k]) for k in keys[b:b + 64] if k in v] for b in range(0, len(keys), 64)]


def l1_score(v, w, mut=frozenset()):
    """L1Scoring::score(v, w): both maps in ascending word order; per common word
    s += fabs(vi - wi) - fabs(vi) - fabs(wi), left to right; -s / 2.0.
    mut: other orders of the same double sum (sum_reversed, sum_pairwise, sum_blocks64: per 64 of
    w's words a partial sum, the partial sums added in order) and carry_zero_block (a block of 64
    words without a common word adds the previous block's terms once more)."""
    if mut & set(MUTATIONS[2:]):
        blocks = score_terms(v, w)
        flat = [t for b in blocks for t in b]
        if "sum_reversed" in mut:
            s = 0.0
            for t in reversed(flat):
                s += t
        elif "sum_pairwise" in mut:
            s = pairwise(flat)
        elif "sum_blocks64" in mut:
            s = 0.0
            for b in blocks:
                part = 0.0
                for t in b:
                    part += t
                s += part
        else:
            s, last = 0.0, []
            for b in blocks:
                last = b or last
                for t in last:
                    s += t
        return -s / 2.0
    s = 0.0
    for word in sorted(v):
        if word in w:
            vi, wi = v[word], w[word]
            s += abs(vi - wi) - abs(vi) - abs(wi)
    return -s / 2.0


class KeyFrame:
    """What the database reads and writes of a KeyFrame: mBowVec and the three mnReloc* fields."""

    def __init__(self, kf_id, bow):
        self.id = kf_id
        self.bow = bow
        self.reloc_query = -1           # mnRelocQuery (no frame has this id)
        self.reloc_words = 0            # mnRelocWords
        self.reloc_score = 0.0          # mRelocScore (a float)


class Database:
    """mvInvertedFile: word -> the keyframes that hold it, in insertion order."""

    def __init__(self):
        self.inverted = {}

    def add(self, kf):
        for word in sorted(kf.bow):
            self.inverted.setdefault(word, []).append(kf)

    def erase(self, kf):
        for word in sorted(kf.bow):
            lst = self.inverted.get(word, [])
            for i, other in enumerate(lst):
                if other is kf:
                    del lst[i]
                    break

    def clear(self):
        self.inverted = {}


def min_common_words(max_common, mut=frozenset()):
    """int minCommonWords = maxCommonWords*0.8f: a float32 product, truncated."""
    if "min_common_f64" in mut:
        return int(float(max_common) * 0.8)
    return int(np.float32(max_common) * np.float32(0.8))


def detect_reloc(F_bow, db, frame_id, neighbours, mut=frozenset()):
    """DetectRelocalizationCandidates(F).  neighbours(kf) -> GetBestCovisibilityKeyFrames(10).
    -> dict(sharing: lKFsSharingWords, max_common, min_common, scored: [(float32 score, kf)] =
    lScoreAndMatch, candidates: vpRelocCandidates).  mut: MUTATIONS."""
    sharing = []
    for word in sorted(F_bow):
        for kf in db.inverted.get(word, []):
            if kf.reloc_query != frame_id:
                kf.reloc_words = 0
                kf.reloc_query = frame_id
                sharing.append(kf)
            kf.reloc_words += 1
    out = dict(sharing=sharing, max_common=0, min_common=0, scored=[], candidates=[])
    if not sharing:
        return out
    max_common = 0
    for kf in sharing:
        if kf.reloc_words > max_common:
            max_common = kf.reloc_words
    min_common = min_common_words(max_common, mut)
    out["max_common"], out["min_common"] = max_common, min_common
    scored = []
    for kf in sharing:
        if kf.reloc_words > min_common or ("common_ge" in mut and kf.reloc_words == min_common):
            si = np.float32(l1_score(F_bow, kf.bow, mut))
            kf.reloc_score = si
            scored.append((si, kf))
    out["scored"] = scored
    if not scored:
        return out
    acc = []
    best_acc = np.float32(0)
    for si, kf in scored:
        best_score, acc_score, best_kf = si, si, kf
        for kf2 in neighbours(kf):
            if kf2.reloc_query != frame_id:
                continue
            acc_score = np.float32(acc_score + np.float32(kf2.reloc_score))
            if kf2.reloc_score > best_score:
                best_kf, best_score = kf2, np.float32(kf2.reloc_score)
        acc.append((acc_score, best_kf))
        if acc_score > best_acc:
            best_acc = acc_score
    min_retain = np.float32(0.75) * best_acc
    added = set()
    for si, kf in acc:
        if si > min_retain and id(kf) not in added:
            out["candidates"].append(kf)
            added.add(id(kf))
    return out
