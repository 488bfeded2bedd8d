"""The LocalMapping drop-in adapter (adapter/LocalMapping_coeb.h): the translation unit compiles
against reference-shaped types without a GPU; the host half of the two entry points runs as a
stand-alone program under ASan + UBSan (tests/host/tri_host_main.cpp); and on the GPU the shim
program (tests/adapter_shim/local_mapping_exec.cpp) runs KeyFrameStore and
SearchForTriangulationNeighbors over a 5-keyframe map, whose pairs must be what tests/tri_ref.py says."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import tri_cases as C
import tri_ref as T
from conftest import ROOT

SHIM = os.path.join(ROOT, "tests", "adapter_shim")
CSRC = os.path.join(ROOT, "coeb-slam_amd", "csrc")
INCLUDES = ["-I", SHIM, "-I", os.path.join(ROOT, "coeb-slam_amd", "adapter"), "-I", os.path.join(ROOT, "include")]
SAN = ["-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
NKF, N = 5, 120
CAM = np.array([517.3, 516.5, 318.6, 255.3], np.float32)
f32 = np.float32


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_local_mapping_adapter_compiles():
    cmd = ["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Werror"] + INCLUDES + [os.path.join(SHIM, "local_mapping_tu.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_host_code_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "tri_host")
    cmd = ["g++", "-std=c++17"] + SAN + ["-I", os.path.join(ROOT, "include"), "-I", CSRC,
                                         os.path.join(ROOT, "tests", "host", "tri_host_main.cpp"),
                                         os.path.join(CSRC, "coeb_kfdb_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def _rot(ax, deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    m = {0: [[1, 0, 0], [0, c, -s], [0, s, c]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]], 2: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}
    return np.array(m[ax], np.float64)


@functools.lru_cache(maxsize=None)
def scene():
    """Five keyframes of 120 features over 12 nodes: copies of 100 scene descriptors with a few
    flipped bits, points a few pixels off the line y2 = y1, a third of the features with MapPoints,
    half stereo.  Poses: small rotations and a sideways baseline; F12 is close to LINE_Y."""
    rng = np.random.RandomState(41)
    base = rng.randint(0, 256, (100, 32)).astype(np.uint8)
    base_xy = np.stack([rng.uniform(30, 600, 100), rng.uniform(30, 450, 100)], 1)
    kfs, pose = [], []
    for k in range(NKF):
        src = rng.randint(0, 100, N)
        d = np.unpackbits(base[src], axis=1)
        for i in range(N):
            d[i, rng.choice(256, rng.randint(0, 12), replace=False)] ^= 1
        xy = base_xy[src] + np.stack([rng.uniform(-40, 40, N), rng.choice([0.0, 1.0, 2.5, 5.0], N)], 1)
        node = (src % 12).astype(np.int32)
        node[rng.rand(N) < 0.05] = -1
        stereo = rng.rand(N) < 0.5
        kfs.append(dict(desc=np.packbits(d, axis=1), node=node, x=xy[:, 0].astype(f32), y=xy[:, 1].astype(f32),
                        octave=rng.randint(0, 8, N).astype(np.int32), angle=rng.uniform(0, 360, N).astype(f32),
                        u_right=np.where(stereo, xy[:, 0] - 3.0, -1.0).astype(f32),
                        has_mp=(rng.rand(N) < 0.33).astype(np.uint8)))
        R = (_rot(1, 2.0 * k) @ _rot(0, -1.5 * k)).astype(f32)
        t = np.array([-0.3 * k, 0.02 * k, 0.05 * k + 0.01], f32)
        Ow = (-(R.astype(np.float64).T @ t.astype(np.float64))).astype(f32)
        pose.append(np.concatenate([R.ravel(), t, Ow]).astype(f32))
    F12 = np.array([C.LINE_Y + rng.uniform(-1, 1, (3, 3)) * [[1e-5, 1e-5, 1e-3]] * 3 for _ in range(NKF - 1)], f32)
    return kfs, np.array(pose, f32), F12


def epipole(pose1, pose2):
    """ORBmatcher.cc:664-670 in float32, the matrix product in element order as the shim's operator*."""
    Cw, R, t = pose1[12:15], pose2[:9].reshape(3, 3), pose2[9:12]
    C2 = []
    for r in range(3):
        s = f32(0.0)
        for k in range(3):
            s = f32(s + f32(R[r, k] * Cw[k]))
        C2.append(f32(s + t[r]))
    invz = f32(f32(1.0) / C2[2])
    return f32(f32(f32(CAM[0] * C2[0]) * invz) + CAM[2]), f32(f32(f32(CAM[1] * C2[1]) * invz) + CAM[3])


@functools.lru_cache(maxsize=None)
def expected(only_stereo, check_ori):
    kfs, pose, F12 = scene()
    out = []
    for k in range(1, NKF):
        out.append(T.search_for_triangulation(kfs[0], kfs[k], kfs[0]["has_mp"], kfs[k]["has_mp"], F12[k - 1],
                                              epipole(pose[0], pose[k]), C.SCALE, C.SIGMA2, only_stereo, check_ori))
    return out


def test_scene_has_what_it_is_for():
    kfs, pose, _ = scene()
    plain = [nm for _, nm in expected(False, False)]
    assert min(plain) >= 8 and sum(nm for _, nm in expected(True, False)) < sum(plain)
    assert sum(nm for _, nm in expected(False, True)) < sum(plain)
    # the epipoles lie in the image plane's neighbourhood and differ per neighbour
    e = np.array([epipole(pose[0], pose[k]) for k in range(1, NKF)])
    assert np.isfinite(e).all() and len({tuple(v) for v in e.tolist()}) == NKF - 1


@pytest.mark.gpu
@pytest.mark.parametrize("only_stereo,check_ori", [(False, False), (True, True)])
def test_local_mapping_adapter_runs_against_library(tmp_path, only_stereo, check_ori):
    lib_dir = os.path.join(ROOT, "coeb-slam_amd", "lib")
    exe = str(tmp_path / "local_mapping_exec")
    cmd = ["g++", "-std=c++14", "-O2", "-Wall", "-Werror"] + INCLUDES + [
        os.path.join(SHIM, "local_mapping_exec.cpp"), "-o", exe, "-L", lib_dir, "-lcoeb_front", "-Wl,-rpath," + lib_dir,
        "-Wl,-rpath-link,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    kfs, pose, F12 = scene()
    cat = lambda key: np.concatenate([kf[key] for kf in kfs])          # noqa: E731
    keys = np.stack([cat("x"), cat("y"), cat("angle"), cat("u_right")], 1).astype(f32)
    for name, a in (("counts.i32", np.array([N] * NKF, np.int32)), ("desc.u8", cat("desc")), ("node.i32", cat("node")),
                    ("keys.f32", keys), ("octave.i32", cat("octave")), ("has_mp.u8", cat("has_mp")), ("pose.f32", pose),
                    ("cam.f32", CAM), ("F12.f32", F12), ("flags.i32", np.array([only_stereo, check_ori], np.int32))):
        np.ascontiguousarray(a).tofile(str(tmp_path / name))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
    match = np.fromfile(str(tmp_path / "match.i32"), np.int32).reshape(NKF - 1, N)
    nm = np.fromfile(str(tmp_path / "nmatch.i32"), np.int32)
    want = expected(only_stereo, check_ori)
    for j, (w, w_nm) in enumerate(want):
        assert nm[j] == w_nm and np.array_equal(match[j], w), j
    assert nm[-1] == sum(w_nm for _, w_nm in want)
