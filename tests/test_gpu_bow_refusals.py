"""The refusals of the bag-of-words and keyframe-database calls that take host arrays (MI355X only, as
every call takes a context): coeb_bow_transform, coeb_match_bow, coeb_kfdb_query, coeb_match_bow_kfdb,
coeb_kfdb_add and coeb_kfdb_set_geometry through the raw C entry points -- code, message and precedence.
The expected strings are the ones the library carried while these calls still staged their arrays by
hand.  All but one case return from a host-side check before anything is launched, with the caller's
arrays as they were; coeb_bow_transform's fv_cap refusal comes after the transform and leaves the
feature-vector arrays alone.  The double faults at the end of each group pin the order of the checks.
coeb_match_localmap / coeb_match_keyframe: tests/test_gpu_track_refusals.py."""
import ctypes as C

import numpy as np
import pytest

import coeb_front as cf
import test_gpu_bow as GB

pytestmark = pytest.mark.gpu

OK, EINVAL, ERANGE = 0, -22, -34                    # include/coeb_front.h
SENT = 0x5A
CAP = 4200          # every array holds at least this many elements: a size that slipped past its check reads inside them
MAXF = 32           # the database's max_features
NLEVELS = 8         # the context's pyramid
VOC = "k10"


def vp(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def sent(n, dt=np.int32):
    return np.full(n, SENT, dt)


def counts(k):
    return [C.c_int(SENT) for _ in range(k)]


def ref(c, m, name):
    return None if m.get("null") == name else C.byref(c)


class Env:
    """A context with a vocabulary, one without, and a database of MAXF features on the first: slot 0 a
    keyframe of 4 features, slot 1 erased, slot 2 a keyframe without features."""

    def __init__(self):
        self.ctx = cf.Context(max_width=640, max_height=480, max_batch=1)
        self.bare = cf.Context(max_width=640, max_height=480, max_batch=1)
        v = cf.Vocabulary.from_arrays(*GB.voc_case(VOC)[0])
        self.ctx.set_vocabulary(v)
        v.close()
        self.db = cf.KeyFrameDatabase(self.ctx, max_features=MAXF, initial_slots=1)
        w, val = np.array([1, 7], np.int32), np.array([0.25, 0.75])
        for n in (4, 4, 0):
            self.db.add(np.zeros((n, 32), np.uint8), np.zeros(n, np.int32), np.zeros(n, np.float32), w, val)
        self.db.erase(1)

    def close(self):
        self.db.close()
        self.ctx.close()
        self.bare.close()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


def drop(arrays, prefix, m):
    return [None if prefix + "." + k == m.get("drop") or prefix + "." + k == m.get("drop2") else vp(a) for k, a in arrays.items()]


# ---- the calls: m -> (rc, the handle whose last error is read, arrays that must stay SENT, counts, their expected value)
def coeb_bow_transform(env, m):
    c = env.bare if m.get("bare") else env.ctx
    n = m.get("n", 3)
    desc = np.zeros((CAP, 32), np.uint8)
    outs = dict(word=sent(CAP), node=sent(CAP), weight=np.full(CAP, float(SENT)))
    fv = dict(fv_node=sent(CAP), fv_off=sent(CAP + 1), fv_idx=sent(CAP))
    nfv = counts(1)
    want_fv = m.get("fv", True)
    h = None if m.get("null") == "ctx" else c.h
    rc = cf.lib().coeb_bow_transform(h, None if m.get("drop") == "desc" else vp(desc), n, m.get("levelsup", 1),
                                     *drop(outs, "out", m), *(drop(fv, "fv", m) if want_fv else [None] * 3),
                                     m.get("fv_cap", CAP), None if m.get("null") == "nfv" else C.byref(nfv[0]))
    written = m.get("ran")              # the fv_cap refusal: the transform ran, its ids are delivered
    return rc, h, list(fv.values()) + ([] if written else list(outs.values())), nfv, m.get("nfv", SENT)


def bow_frame(m, cap):
    """-> (the arrays, the struct that points into them): the caller keeps the arrays alive over its call"""
    a = dict(descriptor=np.zeros((cap, 32), np.uint8), node_id=np.zeros(cap, np.int32), angle=np.zeros(cap, np.float32))
    return a, cf.BowFrameC(m.get("n", 1), *drop(a, "cur", m))


def coeb_match_bow(env, m):
    ka = dict(valid=np.ones(CAP, np.uint8), descriptor=np.zeros((CAP, 32), np.uint8), node_id=np.zeros(CAP, np.int32),
              angle=np.zeros(CAP, np.float32))
    kf = cf.BowKeyFrameC(m.get("nq", 1), *drop(ka, "kf", m))
    _keep, cur = bow_frame(m, CAP)
    match, cnt = sent(CAP), counts(1)
    h = None if m.get("null") == "ctx" else env.ctx.h
    rc = cf.lib().coeb_match_bow(h, ref(kf, m, "kf"), ref(cur, m, "cur"), 0.75, 1,
                                 None if m.get("drop") == "match" else vp(match), ref(cnt[0], m, "nm"))
    # the count is zeroed once the pointers are there
    return rc, h, [match], cnt, SENT if m.get("null") else 0


def coeb_kfdb_query(env, m):
    nw = m.get("nw", 2)
    word = np.arange(CAP, dtype=np.int32)
    if m.get("flat"):
        word[1] = word[0]
    value = np.ones(CAP)
    outs = dict(common=sent(CAP), score=sent(CAP, np.float32), order=sent(CAP))
    cnt = counts(3)
    h = None if m.get("null") == "db" else env.db.h
    rc = cf.lib().coeb_kfdb_query(h, None if m.get("drop") == "word" else vp(word), None if m.get("drop") == "value" else vp(value),
                                  nw, *drop(outs, "out", m), *[None if m.get("null") == "cnt%d" % i else C.byref(c)
                                                                for i, c in enumerate(cnt)])
    return rc, None if h is None else env.ctx.h, list(outs.values()), cnt, SENT


def coeb_match_bow_kfdb(env, m):
    slots = np.array(m.get("slots", [0, 2]), np.int32)
    ncand = m.get("ncand", len(slots))
    valid = np.ones(CAP, np.uint8)
    masks = (C.c_void_p * max(len(slots), 1))(*[None if j in m.get("nomask", ()) else valid.ctypes.data for j in range(len(slots))])
    _keep, cur = bow_frame(m, CAP)
    out, nm = sent(300 * 8), sent(300)
    h = None if m.get("null") == "db" else env.db.h
    rc = cf.lib().coeb_match_bow_kfdb(h, None if m.get("drop") == "slots" else vp(slots), ncand,
                                      None if m.get("drop") == "valid" else masks, ref(cur, m, "cur"), 0.75, 1,
                                      None if m.get("drop") == "match" else vp(out), None if m.get("drop") == "nm" else vp(nm))
    return rc, None if h is None else env.ctx.h, [out, nm], [], SENT


def coeb_kfdb_add(env, m):
    a = dict(descriptor=np.zeros((CAP, 32), np.uint8), node_id=np.zeros(CAP, np.int32), angle=np.zeros(CAP, np.float32),
             bow_word=np.arange(CAP, dtype=np.int32), bow_value=np.ones(CAP))
    if m.get("flat"):
        a["bow_word"][1] = a["bow_word"][0]
    p = drop(a, "kf", m)
    kf = cf.KfdbKeyFrameC(m.get("n", 2), *p, m.get("nw", 2))
    slot = counts(1)
    h = None if m.get("null") == "db" else env.db.h
    before = env.db.size()
    rc = cf.lib().coeb_kfdb_add(h, ref(kf, m, "kf"), ref(slot[0], m, "slot"))
    assert env.db.size() == before
    return rc, None if h is None else env.ctx.h, [], slot, SENT


def coeb_kfdb_set_geometry(env, m):
    keys = np.zeros(CAP, cf.KEYPOINT_DTYPE)
    keys["octave"] = m.get("octave", 0)
    ur = np.full(CAP, -1, np.float32)
    h = None if m.get("null") == "db" else env.db.h
    rc = cf.lib().coeb_kfdb_set_geometry(h, m.get("slot", 0), None if m.get("drop") == "keys" else vp(keys),
                                         None if m.get("drop") == "ur" else vp(ur))
    return rc, None if h is None else env.ctx.h, [], [], SENT


def group(entry, rows):
    who = entry.__name__
    return [pytest.param(entry, m, code, msg.replace("@", who), id="%s-%s" % (who, tag)) for tag, m, code, msg in rows]


CASES = (
    group(coeb_bow_transform, [
        ("null", dict(null="ctx"), EINVAL, "@: invalid arguments"),
        ("negative", dict(n=-1), EINVAL, "@: invalid arguments"),
        ("levelsup", dict(levelsup=-1), EINVAL, "@: invalid arguments"),
        ("no-desc", dict(drop="desc"), EINVAL, "@: invalid arguments"),
        ("no-vocabulary", dict(bare=1, nfv=0), EINVAL, "@: no vocabulary (coeb_bow_set_vocabulary)"),
        ("4096", dict(n=4096, nfv=0), EINVAL, "@: more than 4095 descriptors"),
        ("fv-partial", dict(drop="fv.fv_off", nfv=0), EINVAL, "@: incomplete feature-vector outputs"),
        ("fv-no-count", dict(null="nfv"), EINVAL, "@: incomplete feature-vector outputs"),
        ("fv-negative-cap", dict(fv_cap=-1, nfv=0), EINVAL, "@: incomplete feature-vector outputs"),
        ("fv-cap", dict(fv_cap=0, nfv=1, ran=1), ERANGE, "@: feature vector exceeds fv_cap nodes"),
        ("negative+no-vocabulary", dict(bare=1, n=-1), EINVAL, "@: invalid arguments"),
        ("4096+no-vocabulary", dict(bare=1, n=4096, nfv=0), EINVAL, "@: no vocabulary (coeb_bow_set_vocabulary)"),
        ("4096+fv-partial", dict(n=4096, drop="fv.fv_idx", nfv=0), EINVAL, "@: more than 4095 descriptors")])
    + group(coeb_match_bow, [
        ("null", dict(null="ctx"), EINVAL, "@: invalid arguments"),
        ("null-kf", dict(null="kf"), EINVAL, "@: invalid arguments"),
        ("null-count", dict(null="nm"), EINVAL, "@: invalid arguments"),
        ("negative", dict(n=-1), EINVAL, "negative frame / keyframe size"),
        ("negative-kf", dict(nq=-1), EINVAL, "negative frame / keyframe size"),
        ("4096", dict(n=4096), EINVAL, "@: more than 4095 features"),
        ("4096-kf", dict(nq=4096), EINVAL, "@: more than 4095 features"),
        ("missing-kf", dict(drop="kf.valid"), EINVAL, "@: missing keyframe arrays"),
        ("missing-cur", dict(drop="cur.angle"), EINVAL, "@: missing current-frame arrays"),
        ("missing-match", dict(drop="match"), EINVAL, "@: missing current-frame arrays"),
        ("negative+4096", dict(n=-1, nq=4096), EINVAL, "negative frame / keyframe size"),
        ("4096+missing", dict(n=4096, drop="kf.angle"), EINVAL, "@: more than 4095 features"),
        ("missing-both", dict(drop="kf.node_id", drop2="cur.node_id"), EINVAL, "@: missing keyframe arrays")])
    + group(coeb_kfdb_query, [
        ("null", dict(null="db"), EINVAL, "@: invalid arguments"),
        ("null-count", dict(null="cnt1"), EINVAL, "@: invalid arguments"),
        ("negative", dict(nw=-1), EINVAL, "@: invalid arguments"),
        ("no-words", dict(drop="value"), EINVAL, "@: invalid arguments"),
        ("missing-out", dict(drop="out.score"), EINVAL, "@: missing output arrays"),
        ("too-many", dict(nw=MAXF + 1), EINVAL, "@: more query words than max_features"),
        ("ascending", dict(flat=1), EINVAL, "@: word is not strictly ascending"),
        ("negative+missing-out", dict(nw=-1, drop="out.order"), EINVAL, "@: invalid arguments"),
        ("missing-out+too-many", dict(nw=MAXF + 1, drop="out.common"), EINVAL, "@: missing output arrays"),
        ("too-many+ascending", dict(nw=MAXF + 1, flat=1), EINVAL, "@: more query words than max_features")])
    + group(coeb_match_bow_kfdb, [
        ("null", dict(null="db"), EINVAL, "@: invalid arguments"),
        ("null-frame", dict(null="cur"), EINVAL, "@: invalid arguments"),
        ("negative", dict(ncand=-1), EINVAL, "@: invalid arguments"),
        ("257", dict(slots=[0] * 257), EINVAL, "@: more than 256 candidates"),
        ("negative-frame", dict(n=-1), EINVAL, "@: frame size outside 0..4095"),
        ("4096", dict(n=4096), EINVAL, "@: frame size outside 0..4095"),
        ("missing-slots", dict(drop="slots"), EINVAL, "@: missing arrays"),
        ("missing-cur", dict(drop="cur.descriptor"), EINVAL, "@: missing arrays"),
        ("missing-counts", dict(drop="nm"), EINVAL, "@: missing arrays"),
        ("erased-slot", dict(slots=[0, 1]), EINVAL, "@: no keyframe in a candidate's slot"),
        ("unused-slot", dict(slots=[3]), EINVAL, "@: no keyframe in a candidate's slot"),
        ("negative-slot", dict(slots=[-1]), EINVAL, "@: no keyframe in a candidate's slot"),
        ("missing-mask", dict(nomask=(0,)), EINVAL, "@: missing valid mask"),
        ("257+4096", dict(slots=[0] * 257, n=4096), EINVAL, "@: more than 256 candidates"),
        ("4096+missing", dict(n=4096, drop="valid"), EINVAL, "@: frame size outside 0..4095"),
        ("missing+erased", dict(slots=[1], drop="match"), EINVAL, "@: missing arrays"),
        ("erased+missing-mask", dict(slots=[1, 0], nomask=(1,)), EINVAL, "@: no keyframe in a candidate's slot"),
        ("missing-mask+erased", dict(slots=[0, 1], nomask=(0,)), EINVAL, "@: missing valid mask")])
    + group(coeb_kfdb_add, [
        ("null", dict(null="db"), EINVAL, "@: invalid arguments"),
        ("null-kf", dict(null="kf"), EINVAL, "@: invalid arguments"),
        ("null-slot", dict(null="slot"), EINVAL, "@: invalid arguments"),
        ("negative", dict(n=-1), EINVAL, "@: n or nw outside 0..max_features"),
        ("too-many", dict(n=MAXF + 1), EINVAL, "@: n or nw outside 0..max_features"),
        ("too-many-words", dict(nw=MAXF + 1), EINVAL, "@: n or nw outside 0..max_features"),
        ("missing", dict(drop="kf.angle"), EINVAL, "@: missing keyframe arrays"),
        ("missing-words", dict(drop="kf.bow_value"), EINVAL, "@: missing keyframe arrays"),
        ("ascending", dict(flat=1), EINVAL, "@: bow_word is not strictly ascending"),
        ("too-many+missing", dict(nw=MAXF + 1, drop="kf.descriptor"), EINVAL, "@: n or nw outside 0..max_features"),
        ("missing+ascending", dict(flat=1, drop="kf.node_id"), EINVAL, "@: missing keyframe arrays")])
    + group(coeb_kfdb_set_geometry, [
        ("null", dict(null="db"), EINVAL, "@: invalid arguments"),
        ("erased-slot", dict(slot=1), EINVAL, "@: no keyframe in that slot"),
        ("unused-slot", dict(slot=3), EINVAL, "@: no keyframe in that slot"),
        ("negative-slot", dict(slot=-1), EINVAL, "@: no keyframe in that slot"),
        ("missing", dict(drop="ur"), EINVAL, "@: missing keyframe arrays"),
        ("octave", dict(octave=NLEVELS), EINVAL, "@: keypoint octave outside the pyramid"),
        ("erased+missing", dict(slot=1, drop="keys"), EINVAL, "@: no keyframe in that slot"),
        ("missing+octave", dict(octave=NLEVELS, drop="ur"), EINVAL, "@: missing keyframe arrays")]))


@pytest.mark.parametrize("entry,m,code,msg", CASES)
def test_refusal(env, entry, m, code, msg):
    rc, h, outs, cnt, cnt_want = entry(env, m)
    got = cf.lib().coeb_last_error(h).decode()
    assert rc == code and got == msg, (rc, got)
    for o in outs:
        assert (o == o.dtype.type(SENT)).all()
    assert [c.value for c in cnt] == [cnt_want] * len(cnt)


def test_what_is_not_refused(env):
    """The neighbours of the refusals: no candidates, a keyframe without features (no mask, no geometry
    arrays needed), an empty query; and the database still answers after all of the above."""
    L = cf.lib()
    _keep, cur = bow_frame(dict(n=1), CAP)
    assert L.coeb_match_bow_kfdb(env.db.h, None, 0, None, C.byref(cur), 0.75, 1, None, None) == OK
    out, nm = sent(8), sent(2)
    slots, masks = np.array([2], np.int32), (C.c_void_p * 1)(None)
    assert L.coeb_match_bow_kfdb(env.db.h, vp(slots), 1, masks, C.byref(cur), 0.75, 1, vp(out), vp(nm)) == OK
    assert out[0] == -1 and nm[0] == 0 and (out[1:] == SENT).all() and nm[1] == SENT
    assert L.coeb_kfdb_set_geometry(env.db.h, 2, None, None) == OK
    q = env.db.query(np.zeros(0, np.int32), np.zeros(0))
    assert len(q["order"]) == 0 and not q["common"].any()
    assert env.db.size() == (2, 3)
    q = env.db.query(np.array([7], np.int32), np.array([1.0]))
    assert list(q["order"]) == [0, 2] and list(q["common"]) == [1, 0, 1]
