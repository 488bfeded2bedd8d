"""Directed frame lists for the batched moving-object chain (coeb_frame_batch_device -> pmo_batch).

Pair z of a case is frames z and z + 1.  The textured sequences the other batch tests feed give
every pair 400-600 corners; these lists mix pairs with 0 corners, a handful, the 1000-corner cap,
runs of empty pairs, and neighbours that look nothing alike, so that the code that exists only
for more than one pair (k_flow_index, flow_item, flow_code, the chained pyramids, the per-pair
strides and T_M slots) is visible: tests/test_flow_batch_cases.py asserts the conditions on the
oracle alone, tests/test_gpu_flow_batch.py runs the lists on the device.

Frame kinds, all at one size per case: textured (synth.moving_object_sequence with a scaled
object), flat, noise and its shifted copy, a few blobs and their shifted copy, a single blob.

Also here: a numpy model of the flattened work list (index_offsets, item_map) with the wrong
readings tests/test_flow_batch_cases.py separates.
"""
import hashlib

import numpy as np

from coeb_front import synth

MAX_PTS = 1024          # kMaxPts: the clamp of a pair's count, and the slots of a pair
IDX_BITS = 10           # kFlowIdxBits
ROUND = 1024            # pairs per k_flow_index round

# 8 levels at 1.2: level 7 is round(size / 1.2^7) and must hold one 30-px FAST cell between the
# 16-px borders, i.e. >= 62 px, so 221 is the smallest width and the smallest height a default
# context plans (224x208 has a 58-px level 7 and is refused)
MIXED_SIZE = (221, 221)
# 5 levels: level 4 is round(size / 1.2^4) >= 62 from 128 on; an odd pitch and an odd frame stride
SMALL_SIZE = (163, 131)
SMALL_LEVELS = 5
# the smallest w x (3 w / 4) noise frame whose pairs both reach maxCorners = 1000 (384x288: 998, 994)
CAP_SIZE = (385, 288)
# two levels at 1.2 are all that 96x80 allows (level 1 is 80x67, level 2 would be 67x56)
ROUND_SIZE = (96, 80)
ROUND_LEVELS = 2
ROUND_F = 1030


# ---- frame kinds ----
def textured(w, h, n, seed=3):
    """n frames of synth.moving_object_sequence with the object scaled into a w x h frame;
    (frames, object box per frame)."""
    ow, oh = max(24, w // 4), max(24, (h * 3) // 10)
    ox, oy = (w * 2) // 5, h // 4
    return synth.moving_object_sequence(w, h, n, seed=seed, n_small=max(20, w * h // 500), obj=(ox, oy, ow, oh),
                                        obj_shift=(-3, 2))


def flat(w, h, v=118):
    return np.full((h, w), v, np.uint8)


def noise(w, h, seed=11):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def shifted(img, k=1):
    return np.roll(img, (k * 1, k * 2), axis=(0, 1))


def blobs(w, h, n=3, seed=5, size=9):
    """n bright squares of `size` px on a flat ground, well apart and away from the border."""
    img = flat(w, h, 60).astype(np.int16)
    rng = np.random.default_rng(seed)
    placed = []
    while len(placed) < n:
        x, y = int(rng.integers(30, w - 30 - size)), int(rng.integers(30, h - 30 - size))
        if all(abs(x - px) > 3 * size or abs(y - py) > 3 * size for px, py in placed):
            placed.append((x, y))
            img[y:y + size, x:x + size] = 150 + 20 * len(placed)
    return img.astype(np.uint8)


def single_blob(w, h):
    img = flat(w, h, 60)
    img[h // 2:h // 2 + 9, w // 3:w // 3 + 9] = 230
    return img


def _box(w, h, x0, y0, x1, y1):
    return np.float32([x0 * w, y0 * h, x1 * w, y1 * h])


# ---- cases ----
def _case(name, w, h, frames, boxes, **kw):
    frames = np.ascontiguousarray(np.stack(frames), np.uint8)
    assert frames.shape[1:] == (h, w)
    boxes = [np.zeros((0, 4), np.float32) if b is None else np.asarray(b, np.float32).reshape(-1, 4) for b in boxes]
    assert len(boxes) == len(frames)
    return dict(name=name, w=w, h=h, frames=frames, boxes=boxes, **kw)


def mixed(w=MIXED_SIZE[0], h=MIXED_SIZE[1]):
    """F = 10.  Pairs: 0, 1 ordinary; 2 textured -> flat; 3 flat -> textured (0 corners); 4
    textured -> noise; 5 noise -> shifted noise (>= 400 corners, all on the epipolar lines); 6
    shifted noise -> blobs; 7 blobs -> one blob (8..15 corners); 8 one blob twice (1..7 corners,
    identical frames)."""
    tex, obj = textured(w, h, 5, seed=7)
    nz = noise(w, h)
    one = single_blob(w, h)
    # textured frames 0, 1, 3: the second ordinary pair spans two steps of the motion, so its T_M
    # is not the size of the first one's
    frames = [tex[0], tex[1], tex[3], flat(w, h), tex[4], nz, shifted(nz), blobs(w, h), one, one]
    mid = _box(w, h, 0.25, 0.25, 0.75, 0.75)
    # frame 2's two small boxes lie on T_M points of pair 1 that neither pair 0 nor pair 2 has
    # (found with the oracle at 221x221; test_flow_batch_cases.py asserts what they are for)
    wide = _box(w, h, 0.05, 0.05, 0.95, 0.95)
    boxes = [np.stack([obj[0]]), np.stack([obj[1], _box(w, h, 0.6, 0.1, 0.95, 0.5)]),
             np.stack([obj[3], _box(w, h, 100 / 221, 175 / 221, 125 / 221, 200 / 221),
                       _box(w, h, 183 / 221, 63 / 221, 208 / 221, 96 / 221)]),
             np.stack([mid]), np.stack([obj[4]]), np.stack([mid, obj[4]]), np.stack([mid]), np.stack([wide]),
             np.stack([mid]), None]
    return _case("mixed", w, h, frames, boxes,
                 roles=dict(ordinary=(0, 1), to_flat=2, from_flat=3, many=5, few=7, fewer=8, identical=8))


def _empties(name, kinds, w, h):
    tex, obj = textured(w, h, 5, seed=4)
    bl = blobs(w, h)
    src = dict(f=flat(w, h), b=bl, B=shifted(bl, 2), t0=tex[0], t1=tex[1], t2=tex[2])
    frames = [src[k] for k in kinds]
    wide = _box(w, h, 0.1, 0.1, 0.9, 0.9)
    boxes = [np.stack([wide]) if k[0] == "t" else None for k in kinds]
    return _case(name, w, h, frames, boxes)


def empty_first(w=MIXED_SIZE[0], h=MIXED_SIZE[1]):
    """F = 5: pair 0 has no corners (flat -> blobs), then blobs -> shifted blobs and textured pairs."""
    return _empties("empty_first", ["f", "b", "B", "t0", "t1"], w, h)


def empty_last(w=MIXED_SIZE[0], h=MIXED_SIZE[1]):
    """F = 5: the last pair has no corners (flat -> textured)."""
    return _empties("empty_last", ["t0", "t1", "b", "f", "t2"], w, h)


def empty_run(w=MIXED_SIZE[0], h=MIXED_SIZE[1]):
    """F = 6: three consecutive pairs without corners (flat -> flat, flat -> flat, flat -> blobs)
    between two non-empty ones (textured -> flat, blobs -> shifted blobs).  Three empty pairs
    between two others are five pairs, hence six frames, not the five of the other two."""
    return _empties("empty_run", ["t0", "f", "f", "f", "b", "B"], w, h)


def cap(w=CAP_SIZE[0], h=CAP_SIZE[1]):
    """F = 3 noise frames (one frame and two shifts): both pairs reach the 1000-corner cap."""
    nz = noise(w, h, seed=12)
    return _case("cap", w, h, [nz, shifted(nz), shifted(nz, 2)], [None, np.stack([_box(w, h, 0.2, 0.2, 0.8, 0.8)]), None])


def two_frames(w=MIXED_SIZE[0], h=MIXED_SIZE[1]):
    """F = 2: one pair, the unchained two-pyramid path."""
    tex, obj = textured(w, h, 2, seed=6)
    return _case("two_frames", w, h, [tex[0], tex[1]], [obj[0:1], obj[1:2]])


def one_frame(w=MIXED_SIZE[0], h=MIXED_SIZE[1]):
    """F = 1: no pair, no flow."""
    tex, obj = textured(w, h, 1, seed=6)
    return _case("one_frame", w, h, [tex[0]], [obj[0:1]])


ROUND_BUSY = (0, 1, 1022, 1023, 1024, 1025, 1026, 1028)     # the pairs with corners (F = 1030)


def round_case(w=ROUND_SIZE[0], h=ROUND_SIZE[1], F=ROUND_F):
    """F = 1030 at 96x80, 1029 pairs (0 .. 1028): flat everywhere but frames 0, 1 (textured),
    1022 .. 1026 (noise, its shift, textured, noise, its shift) and 1028, 1029 (noise, its shift).
    Pairs 0, 1, 1022 .. 1026 and 1028 have corners, so k_flow_index's second round of 1024 pairs
    starts inside a run of non-empty pairs and must carry their base; pair 1027 (flat -> noise)
    is an empty pair of the second round."""
    fl = flat(w, h)
    frames = [fl] * F
    tex, _ = synth.moving_object_sequence(w, h, 3, seed=8, n_small=30, obj=(40, 24, 28, 30), obj_shift=(-2, 1))
    na, nb, nc = noise(w, h, 21), noise(w, h, 22), noise(w, h, 23)
    put = {0: tex[0], 1: tex[1], 1022: na, 1023: shifted(na), 1024: tex[2], 1025: nb, 1026: shifted(nb),
           F - 2: nc, F - 1: shifted(nc)}
    for f, img in put.items():
        frames[f] = img
    wide = _box(w, h, 0.1, 0.1, 0.9, 0.9)
    boxes = [np.stack([wide]) if f in (1, 2, 1023, 1024, 1025, 1027, F - 1) else None for f in range(F)]
    return _case("round", w, h, frames, boxes)


CASES = dict(mixed=mixed, empty_first=empty_first, empty_last=empty_last, empty_run=empty_run, cap=cap,
             two_frames=two_frames, one_frame=one_frame, round=round_case)
_built = {}


def build(name, *size):
    key = (name,) + tuple(size)
    if key not in _built:
        _built[key] = CASES[name](*size)
    return _built[key]


def box_arrays(case):
    """(boxes (n, 4), box_off (F + 1,)) as coeb_frame_batch_device takes them."""
    off = np.zeros(len(case["boxes"]) + 1, np.int32)
    off[1:] = np.cumsum([len(b) for b in case["boxes"]])
    allb = np.concatenate(case["boxes"]) if off[-1] else np.zeros((0, 4), np.float32)
    return allb, off


# ---- the oracle, pair by pair and frame by frame ----
_pair_cache = {}


def _digest(img):
    return hashlib.sha1(img.tobytes()).digest() + bytes(str(img.shape), "ascii")


def oracle_pair(O, prev, cur):
    """Frame::ProcessMovingObject(prev -> cur) stage by stage: dict(npts, corners, next_pts,
    status, state, F (None: findFundamentalMat returned no matrix), nf, tm (None with F))."""
    key = (_digest(prev), _digest(cur))
    if key not in _pair_cache:
        pts = O.corner_subpix(prev, O.good_features(prev))
        if len(pts):
            nxt, st = O.lk_pyr(prev, cur, pts)
        else:
            nxt, st = np.zeros((0, 2), np.float32), np.zeros(0, np.uint8)
        tm, state, F, nf = O.moving_tail(prev, cur, pts, nxt, st)
        whole = O.process_moving_object(prev, cur)
        assert (whole is None) == (tm is None) and (tm is None or np.array_equal(whole, tm))
        _pair_cache[key] = dict(npts=len(pts), corners=pts, next_pts=nxt, status=st, state=state, F=F, nf=nf, tm=tm)
    return _pair_cache[key]


_oracle_cache = {}


def oracle_case(O, case, nlevels=8):
    """dict(pairs: oracle_pair per pair; tm: T_M per frame (frame 0: empty; None as the oracle
    gives it); blur: flags per frame; ext: the masked extraction per frame)."""
    key = (case["name"], case["w"], case["h"], nlevels)
    if key in _oracle_cache:
        return _oracle_cache[key]
    fr, boxes = case["frames"], case["boxes"]
    pairs = [oracle_pair(O, fr[z], fr[z + 1]) for z in range(len(fr) - 1)]
    tms = [np.zeros((0, 2), np.float32)] + [p["tm"] for p in pairs]
    ex = O.Extractor(nlevels=nlevels)
    blur, ext, memo = [], [], {}
    for f in range(len(fr)):
        b = boxes[f]
        bl = O.blur_flags(fr[f], b)[0] if f and len(b) else np.zeros(len(b), np.int32)
        blur.append(bl)
        ext.append(masked_extract(ex, fr[f], b, tms[f], bl, memo))
    res = dict(pairs=pairs, tm=tms, blur=blur, ext=ext, ex=ex)
    _oracle_cache[key] = res
    return res


def masked_extract(ex, frame, boxes, tm, blur, memo=None):
    tm = np.zeros((0, 2), np.float32) if tm is None else tm
    key = (_digest(frame), boxes.tobytes(), tm.tobytes(), blur.tobytes())
    if memo is not None and key in memo:
        return memo[key]
    r = ex.extract(frame, boxes, tm, blur)
    if memo is not None:
        memo[key] = r
    return r


def counts(res):
    return np.array([p["npts"] for p in res["pairs"]], np.int64)


def tm_counts(res):
    """|T_M| per frame, -1 where the oracle returns None."""
    return [-1 if t is None else len(t) for t in res["tm"]]


def same_extraction(a, b):
    return all(np.array_equal(a["kps"][n], b["kps"][n]) for n in a["kps"].dtype.names) and np.array_equal(a["desc"], b["desc"])


# ---- numpy model of the flattened work list (k_flow_index, flow_item, flow_code) ----
def index_offsets(n, clamp=True, carry=True):
    """offs[z] = points before pair z, offs[P] = all: the counts clamped to 0..MAX_PTS, summed in
    rounds of ROUND pairs whose base carries on.  clamp=False / carry=False: the wrong readings."""
    n = np.asarray(n, np.int64)
    v = np.clip(n, 0, MAX_PTS) if clamp else np.minimum(n, MAX_PTS)
    offs = np.zeros(len(n) + 1, np.int64)
    base = 0
    for c0 in range(0, len(n), ROUND):
        part = v[c0:c0 + ROUND]
        incl = np.cumsum(part)
        offs[c0:c0 + len(part)] = base + incl - part
        total = base + (int(incl[-1]) if len(part) else 0)
        base = total if carry else 0
        last = total
    offs[len(n)] = last if len(n) else 0
    return offs


def item_map(offs, strict=False, idx_bits=IDX_BITS):
    """(pair, point) of every flattened item 0 .. offs[P] - 1 as flow_item's binary search finds
    them and flow_code / flow_decode carry them.  strict=True compares with < for <=, idx_bits=9
    narrows the index field: the wrong readings."""
    P = len(offs) - 1
    out = np.zeros((max(int(offs[P]), 0), 2), np.int64)
    for item in range(len(out)):
        lo, hi = 0, P
        while hi - lo > 1:
            mid = (lo + hi) >> 1
            if (offs[mid] < item) if strict else (offs[mid] <= item):
                lo = mid
            else:
                hi = mid
        code = (lo << idx_bits) | int(item - offs[lo])
        out[item] = (code >> idx_bits, code & ((1 << idx_bits) - 1))
    return out


def expected_map(n):
    """The list the kernels must walk: every point of every pair once, pairs in order."""
    n = np.clip(np.asarray(n, np.int64), 0, MAX_PTS)
    pair = np.repeat(np.arange(len(n)), n)
    start = np.repeat(np.cumsum(n) - n, n)
    return np.stack([pair, np.arange(len(pair)) - start], axis=1) if len(pair) else np.zeros((0, 2), np.int64)


WRONG_READINGS = dict(
    strict_compare=lambda n: item_map(index_offsets(n), strict=True),
    no_negative_clamp=lambda n: item_map(index_offsets(n, clamp=False)),
    round_base_dropped=lambda n: item_map(index_offsets(n, carry=False)),
    nine_bit_index=lambda n: item_map(index_offsets(n), idx_bits=9),
)
