"""The bag-of-words drop-in adapters (adapter/BoW_coeb.h, ORBmatcher_coeb.h SearchByBoW): the
translation unit compiles against reference-shaped types without a GPU, and on the GPU the shim
program (tests/adapter_shim/bow_exec.cpp) fills DBoW2-shaped containers and vpMapPointMatches
exactly as the CPU reference (tests/bow_ref.py) says."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bow_ref as R
from conftest import ROOT

SHIM = os.path.join(ROOT, "tests", "adapter_shim")
INCLUDES = ["-I", SHIM, "-I", os.path.join(ROOT, "coeb-slam_amd", "adapter"), "-I", os.path.join(ROOT, "include")]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_bow_adapters_compile():
    cmd = ["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Werror"] + INCLUDES + [os.path.join(SHIM, "bow_tu.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.gpu
def test_bow_adapters_run_against_library(tmp_path):
    lib_dir = os.path.join(ROOT, "coeb-slam_amd", "lib")
    exe = str(tmp_path / "bow_exec")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Werror"] + INCLUDES + [
        os.path.join(SHIM, "bow_exec.cpp"), "-o", exe, "-L", lib_dir, "-lcoeb_front", "-Wl,-rpath," + lib_dir,
        "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # k = 4, L = 5, levelsup 4: the feature-vector nodes are the 4 children of the root
    args = R.random_voc(4, 5, seed=31, zero_weight=0.1)
    ref = R.Voc(*args)
    rng = np.random.RandomState(32)
    n = 300
    kf = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    kf[150:] = kf[:150]
    for i in range(150, n):                                  # near copies: features compete
        for b in rng.choice(256, 3, replace=False):
            kf[i, b >> 3] ^= 1 << (b & 7)
    perm = rng.permutation(n)
    cur = kf[perm].copy()
    for i in range(n):
        for b in rng.choice(256, rng.randint(0, 15), replace=False):
            cur[i, b >> 3] ^= 1 << (b & 7)
    kang = rng.uniform(0, 359, n).astype(np.float32)
    fang = np.mod(kang[perm] - np.float32(30.0), 360).astype(np.float32)
    fang[fang >= 360] = 0
    fang[::9] = rng.uniform(0, 359, len(fang[::9])).astype(np.float32)
    valid = (rng.rand(n) >= 0.3).astype(np.uint8)
    with open(str(tmp_path / "voc.txt"), "w") as f:
        f.write(R.voc_text(*args))
    for name, a in (("kf_desc.u8", kf), ("cur_desc.u8", cur), ("kf_valid.u8", valid), ("kf_angle.f32", kang),
                    ("cur_angle.f32", fang)):
        a.tofile(str(tmp_path / name))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr

    def containers(path):
        bv, fv = [], []
        for ln in open(path):
            f = ln.split()
            if f[0] == "w":
                bv.append((int(f[1]), float(f[2])))
            else:
                fv.append((int(f[1]), [int(x) for x in f[2:]]))
        return bv, fv

    nodes = {}
    for side, desc in (("kf", kf), ("cur", cur)):
        want = R.compute_bow(ref, desc, 4)
        nodes[side] = want["node"]
        bv, fv = containers(str(tmp_path / (side + "_bow.txt")))
        acc = {}
        for w, wt, nd in zip(want["word"], want["weight"], want["node"]):   # addWeight in feature order
            if nd >= 0:
                acc[int(w)] = acc.get(int(w), 0.0) + wt
        assert bv == sorted(acc.items())
        assert fv == [(int(nd), list(want["fv_idx"][want["fv_off"][j]:want["fv_off"][j + 1]]))
                      for j, nd in enumerate(want["fv_node"])]
        assert (want["node"] < 0).any()                       # a word of weight 0 went to neither container
    want, want_nm, st = R.search_by_bow(valid, kf, nodes["kf"], kang, cur, nodes["cur"], fang, 0.7, True)
    assert want_nm >= 30 and st["rot_removed"] >= 1
    assert np.array_equal(np.fromfile(str(tmp_path / "match.i32"), np.int32), want)
    assert int(np.fromfile(str(tmp_path / "nmatch.i32"), np.int32)[0]) == want_nm
