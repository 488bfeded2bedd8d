"""The keyframe database without a GPU: the CPU restatement (tests/kfdb_ref.py) pinned on a
hand-worked case, coeb_bow_vector (csrc/coeb_kfdb_host.cpp) against it, and the host code as a
stand-alone program under ASan + UBSan (tests/host/kfdb_host_main.cpp)."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import kfdb_ref as K
from conftest import ROOT

ERANGE = -34
SAN = ["-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

# ---- the hand-worked case: 5 words (0..4), 3 keyframes, every value a binary fraction ----
#   F   = {0: 1/2, 1: 1/4, 3: 1/4}
#   KF0 = {0: 1/2, 2: 1/2}                   common {0}:       |0| - 1/2 - 1/2 = -1              score 1/2
#   KF1 = {1: 1/2, 3: 1/4, 4: 1/4}           common {1, 3}:    (1/4 - 1/4 - 1/2) + (0 - 1/4 - 1/4) = -1   score 1/2
#   KF2 = {0: 1/4, 1: 1/4, 3: 1/4, 4: 1/4}   common {0, 1, 3}: 3 x -1/2                          score 3/4
# inverted file: word 0 -> KF0, KF2; word 1 -> KF1, KF2: lKFsSharingWords = KF0, KF2, KF1
# maxCommonWords 3, minCommonWords = int(3 * 0.8f) = 2: only KF2 (3 > 2) is scored, KF1 (2 > 2) is not
F_BOW = {0: 0.5, 1: 0.25, 3: 0.25}
KF_BOW = [{0: 0.5, 2: 0.5}, {1: 0.5, 3: 0.25, 4: 0.25}, {0: 0.25, 1: 0.25, 3: 0.25, 4: 0.25}]
# ---- addWeight: word 2 three times and word 1 six times with weight 0.1, word 4 without a node ----
AW_WORD = [2, 0, 2, 2, 4, 1, 1, 1, 1, 1, 1]
AW_WEIGHT = [0.1, 0.5, 0.1, 0.1, 0.25, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1]
AW_NODE = [1, 1, 1, 1, -1, 1, 1, 1, 1, 1, 1]


def _map():
    kfs = [K.KeyFrame(i, dict(b)) for i, b in enumerate(KF_BOW)]
    db = K.Database()
    for kf in kfs:
        db.add(kf)
    return kfs, db


def test_add_weight_is_sequential():
    bv = K.bow_vector(AW_WORD, AW_WEIGHT, AW_NODE, normalize_l1=False)
    # 0.1 + 0.1 + 0.1 (which is not 0.3); six sequential adds give 0.6 where 6 * 0.1 is 0.6000000000000001
    assert bv == {0: 0.5, 1: 0.6, 2: 0.30000000000000004}
    assert bv[2] != 0.3 and bv[1] != 6 * 0.1
    bv = K.bow_vector(AW_WORD, AW_WEIGHT, AW_NODE)
    assert bv == {0: 0.3571428571428571, 1: 0.4285714285714285, 2: 0.2142857142857143}
    assert K.bow_vector([], [], []) == {} and K.bow_vector([3], [0.0], [1]) == {3: 0.0}     # norm 0: left alone


def test_l1_score_hand_worked():
    assert [K.l1_score(F_BOW, b) for b in KF_BOW] == [0.5, 0.5, 0.75]
    assert K.l1_score(F_BOW, F_BOW) == 1.0 and K.l1_score(F_BOW, {2: 1.0}) == 0.0


def test_detect_reloc_hand_worked():
    kfs, db = _map()
    r = K.detect_reloc(F_BOW, db, 7, lambda kf: [])
    assert [kf.id for kf in r["sharing"]] == [0, 2, 1]
    assert [kf.reloc_words for kf in kfs] == [1, 2, 3] and (r["max_common"], r["min_common"]) == (3, 2)
    assert [(float(s), kf.id) for s, kf in r["scored"]] == [(0.75, 2)]
    assert [kf.id for kf in r["candidates"]] == [2]
    # a second frame {0: 1}: KF0 (score 1/2) and KF2 (1/4) share one word, minCommonWords = int(0.8f) = 0.
    # KF0's neighbours: KF2 (this query, + 1/4) and KF1 (last query's: skipped) -> 3/4, best KF0;
    # KF2's neighbour KF0 scores higher: 3/4, best KF0 again -- the duplicate is dropped
    nb = {0: [kfs[2], kfs[1]], 2: [kfs[0]]}
    r = K.detect_reloc({0: 1.0}, db, 8, lambda kf: nb[kf.id])
    assert [kf.id for kf in r["sharing"]] == [0, 2] and (r["max_common"], r["min_common"]) == (1, 0)
    assert [(float(s), kf.id) for s, kf in r["scored"]] == [(0.5, 0), (0.25, 2)]
    assert kfs[1].reloc_query == 7 and [kf.id for kf in r["candidates"]] == [0]
    # erase: KF0 leaves both of its lists; a keyframe added afterwards comes last under word 0
    db.erase(kfs[0])
    again = K.KeyFrame(3, dict(KF_BOW[0]))
    db.add(again)
    r = K.detect_reloc(F_BOW, db, 9, lambda kf: [])
    assert [kf.id for kf in r["sharing"]] == [2, 3, 1]
    db.clear()
    assert K.detect_reloc(F_BOW, db, 10, lambda kf: [])["sharing"] == []


# ---- coeb_bow_vector against the restatement ----
@functools.lru_cache(maxsize=None)
def k10_features():
    """word / weight / node of the 1000 features tests/test_gpu_bow.py transforms over its k10 vocabulary."""
    import test_gpu_bow as G
    r = G.bow_ref_case("k10", 1, 1000)
    return r["word"], r["weight"], r["node"]


def bow_cases():
    word, weight, node = k10_features()
    fold = (word % 40).astype(np.int32)                    # 40 words, ~25 adds each
    some = node.copy()
    some[::3] = -1
    none = np.full(len(node), -1, np.int32)
    e_i, e_f = np.zeros(0, np.int32), np.zeros(0, np.float64)
    return [("k10", word, weight, node, 1, 1000), ("k10_raw", word, weight, node, 0, 1000),
            ("fold", fold, weight, some, 1, 40), ("fold_raw", fold, weight, node, 0, 1000),
            ("hand", np.array(AW_WORD, np.int32), np.array(AW_WEIGHT), np.array(AW_NODE, np.int32), 1, 3),
            ("empty", e_i, e_f, e_i, 1, 0), ("all_minus_one", word, weight, none, 1, 8),
            ("cap_overflow", fold, weight, node, 1, 39)]


def _want(word, weight, node, norm, cap):
    bv = K.bow_vector(word, weight, node, bool(norm))
    keys = sorted(bv)
    if len(keys) > cap:
        return ERANGE, len(keys), None, None
    return 0, len(keys), np.array(keys, np.int32), np.array([bv[k] for k in keys], np.float64)


@pytest.mark.parametrize("case", bow_cases(), ids=lambda c: c[0])
def test_bow_vector_matches_restatement(case):
    import ctypes as C
    from coeb_front import _p, bow_vector, lib
    _, word, weight, node, norm, cap = case
    rc, nw, want_w, want_v = _want(word, weight, node, norm, cap)
    w_out, v_out = np.full(cap + 1, -7, np.int32), np.full(cap + 1, -7.0)
    got_nw = C.c_int(-1)
    got = lib().coeb_bow_vector(_p(word), _p(weight), _p(node), len(word), norm, _p(w_out), _p(v_out), cap,
                                C.byref(got_nw))
    assert (got, got_nw.value) == (rc, nw)
    assert w_out[cap] == -7 and v_out[cap] == -7.0
    if rc:
        assert (w_out == -7).all()                          # COEB_ERANGE: nothing written
        return
    assert np.array_equal(w_out[:nw], want_w) and np.array_equal(v_out[:nw], want_v)      # doubles bit for bit
    if cap >= len(word):                                    # the Python mirror sizes cap = n
        w, v = bow_vector(word, weight, node, bool(norm))
        assert np.array_equal(w, want_w) and np.array_equal(v, want_v)


def test_bow_vector_cases_reach_their_branches():
    word, weight, node = k10_features()
    assert len(word) == 1000 and (node >= 0).all()
    assert _want(*bow_cases()[2][1:])[1] == 40 and _want(*bow_cases()[7][1:])[0] == ERANGE
    assert _want(*bow_cases()[6][1:])[1] == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_host_code_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "kfdb_host")
    csrc = os.path.join(ROOT, "coeb-slam_amd", "csrc")
    cmd = ["g++", "-std=c++17"] + SAN + ["-I", os.path.join(ROOT, "include"), "-I", csrc,
                                         os.path.join(ROOT, "tests", "host", "kfdb_host_main.cpp"),
                                         os.path.join(csrc, "coeb_kfdb_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    argv = [exe]
    for name, word, weight, node, norm, cap in bow_cases():
        rc, nw, want_w, want_v = _want(word, weight, node, norm, cap)
        path = str(tmp_path / (name + ".bin"))
        with open(path, "wb") as f:
            f.write(np.array([len(word), norm, cap, rc, nw], np.int32).tobytes())
            for a, dt in ((word, np.int32), (node, np.int32), (weight, np.float64)):
                f.write(np.ascontiguousarray(a, dt).tobytes())
            if rc == 0:
                f.write(want_w.tobytes())
                f.write(want_v.tobytes())
        argv.append(path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run(argv, capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
