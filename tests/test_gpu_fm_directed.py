"""k_fm (csrc/coeb_flow.hip) on the directed point sets of tests/fm_sets.py (MI355X only): the
7-point case, LMedS and RANSAC with stops inside, at the end of and one iteration past a chunk of
32 hypotheses, subsets that cannot be drawn, hypotheses without a model, and the thinning of 1024
pairs by state, SAD and the edge rule.  Every comparison is bit for bit against the CPU oracle,
which tests/test_flow_ref.py holds against the independent model of tests/flow_ref.py and whose
trace shows what each set reaches.  120x100 frames; a call takes milliseconds."""
import ctypes as C
import time

import numpy as np
import pytest

import coeb_front as cf
import fm_sets as S

pytestmark = pytest.mark.gpu

COEB_OK, COEB_EINVAL = 0, -22                          # include/coeb_front.h
THREADS = (None, 1024)                                 # COEB_FM_THREADS: the default (128) and the widest form
# The whole module took 3.1 s on an MI355X when it was written (an all-collinear set, 32 x 10000
# redraws on one lane, takes 0.2 s a call at 128 threads and 0.8 s at 1024); the limit leaves a
# factor of ten for a loaded machine.
MODULE_LIMIT_S = 30.0
EMPTY = ("none", "six", "seven_repeated", "collinear20", "collinear12", "five_points20", "rare_subset14")


@pytest.fixture(scope="module", autouse=True)
def module_time():
    t0 = time.perf_counter()
    yield
    dt = time.perf_counter() - t0
    print("test_gpu_fm_directed: %.2f s" % dt)
    assert dt <= MODULE_LIMIT_S, dt


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_tail(got, ref, tag):
    (tm, st, F, nf), (rtm, rst, rF, rnf) = got, ref
    assert np.array_equal(st, rst), (tag, np.nonzero(st != rst)[0][:8])
    assert nf == rnf, (tag, nf, rnf)
    assert (F is None) == (rF is None) and (tm is None) == (rtm is None), (tag, F, rF)
    if rF is not None:
        assert np.array_equal(bits(F), bits(rF)), (tag, F, rF)
        assert tm.shape == rtm.shape and np.array_equal(bits(tm), bits(rtm)), (tag, len(tm), len(rtm))


def set_threads(monkeypatch, threads):
    if threads is not None:
        monkeypatch.setenv("COEB_FM_THREADS", str(threads))


_ref = {}


def reference(oracle_mod, key, args):
    if key not in _ref:
        _ref[key] = oracle_mod.moving_tail(*args)
    return _ref[key]


def set_args(name):
    m1, m2 = S.get(name)
    return S.flat_pair() + (m1, m2, np.ones(len(m1), np.uint8))


@pytest.mark.parametrize("threads", THREADS, ids=["default", "1024"])
@pytest.mark.parametrize("name", list(S.SETS))
def test_directed_set(ctx, oracle_mod, monkeypatch, name, threads):
    set_threads(monkeypatch, threads)
    args = set_args(name)
    ref = reference(oracle_mod, name, args)
    assert (ref[2] is None) == (name in EMPTY), name
    same_tail(cf.MovingTail(ctx, *args), ref, name)


@pytest.mark.parametrize("threads", THREADS, ids=["default", "1024"])
@pytest.mark.parametrize("name", list(S.thin_cases()))
def test_thinned(ctx, oracle_mod, monkeypatch, name, threads):
    """noisy1024 thinned by state to 7, 8, 14, 15 and 129 survivors (a run of 8 kept, a run of 8
    cleared, index 1023 kept), by a bright block through the SAD check, and noisy40 with the edge
    rule's points: the oracle's result, which is also the result on the survivors alone."""
    set_threads(monkeypatch, threads)
    args = S.thin_cases()[name]
    ref = reference(oracle_mod, "thin " + name, args)
    got = cf.MovingTail(ctx, *args)
    same_tail(got, ref, name)
    k = ref[1] != 0
    alone = cf.MovingTail(ctx, args[0], args[1], args[2][k], args[3][k], np.ones(k.sum(), np.uint8))
    assert alone[3] == k.sum() and (alone[2] is None) == (got[2] is None)
    if got[2] is not None:
        assert np.array_equal(bits(alone[2]), bits(got[2])) and np.array_equal(bits(alone[0]), bits(got[0]))


def raw_tail(ctx, prev, cur, pxy, nxy, state, cap, n=None, sentinel=-7.0):
    h, w = prev.shape
    pxy, nxy = np.ascontiguousarray(pxy, np.float32), np.ascontiguousarray(nxy, np.float32)
    st = np.ascontiguousarray(state, np.uint8).copy()
    tm = np.full((len(pxy), 2), sentinel, np.float32)
    F = np.zeros(9, np.float64)
    nt, nf = C.c_int(-99), C.c_int(-99)
    rc = cf.lib().coeb_moving_tail(ctx.h, prev.ctypes.data, cur.ctypes.data, w, h, w, pxy.ctypes.data, nxy.ctypes.data,
                                   st.ctypes.data, len(pxy) if n is None else n, tm.ctypes.data, cap, C.byref(nt),
                                   F.ctypes.data, C.byref(nf))
    return rc, nt.value, tm, st, F, nf.value


@pytest.mark.parametrize("name", ["noisy40", "noisy1024"])
def test_tm_capacity(ctx, oracle_mod, name):
    """tm_cap 0 and |T_M| - 1 through the C ABI: the full count, the oracle's prefix, and nothing
    written past the capacity."""
    args = set_args(name)
    full = reference(oracle_mod, name, args)
    nt = len(full[0])
    assert nt >= 2
    for cap in (0, nt - 1):
        rc, got_nt, tm, st, F, nf = raw_tail(ctx, *args, cap)
        ont, otm = S.oracle_tail_capped(oracle_mod, *args, cap)
        assert rc == COEB_OK and got_nt == ont == nt and nf == full[3]
        assert np.array_equal(bits(tm[:cap]), bits(otm[:cap])) and np.array_equal(bits(tm[:cap]), bits(full[0][:cap]))
        assert (tm[cap:] == -7.0).all()
        assert np.array_equal(bits(F.reshape(3, 3)), bits(full[2]))


def test_too_many_points_is_rejected(ctx, oracle_mod):
    """n = 1025 is COEB_EINVAL and writes nothing; the call that follows is right."""
    args = set_args("noisy1024")
    p = np.concatenate([args[2], args[2][:1]])
    q = np.concatenate([args[3], args[3][:1]])
    rc, nt, tm, st, F, nf = raw_tail(ctx, args[0], args[1], p, q, np.ones(1025, np.uint8), 1025)
    assert rc == COEB_EINVAL and nt == -99 and nf == -99 and (tm == -7.0).all() and st.all() and not F.any()
    same_tail(cf.MovingTail(ctx, *args), reference(oracle_mod, "noisy1024", args), "after the rejection")


def test_empty_results_leave_nothing_behind(ctx, oracle_mod):
    """Every set that ends without an F, each followed on the same context by a set that has one
    (and the other way round): no F or T_M of the call before shows through."""
    for a, b in zip(EMPTY, ("noisy40", "clean15", "noisy9", "seven_one_root", "identity20", "noisy14", "shift45")):
        for name in (b, a, b):
            args = set_args(name)
            got = cf.MovingTail(ctx, *args)
            same_tail(got, reference(oracle_mod, name, args), "%s around %s" % (b, a))
            assert (got[2] is None) == (name == a)
