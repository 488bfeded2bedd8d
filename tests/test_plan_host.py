"""The extraction's plan builder without a GPU: csrc/coeb_plan.cpp (make_tables, make_plan, the
resize tables and row descriptors, the FAST cells, every buffer offset and the octree's LDS size)
as a stand-alone program under ASan + UBSan, checked against the oracle's tables and the layout
invariants the kernels rely on (tests/host/plan_host_main.cpp)."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SAN = ["-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(shutil.which("g++") is None or shutil.which("gcc") is None, reason="g++ / gcc not available")
def test_plan_builder_clean_under_asan_ubsan(tmp_path):
    oracle_o, exe = str(tmp_path / "orb_oracle.o"), str(tmp_path / "plan_host")
    r = subprocess.run(["gcc", "-std=c11"] + SAN + ["-c", os.path.join(ROOT, "oracle", "orb_oracle.c"), "-o", oracle_o],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cmd = ["g++", "-std=c++17"] + SAN + ["-I", os.path.join(ROOT, "coeb-slam_amd", "csrc"), "-I", os.path.join(ROOT, "oracle"),
                                         os.path.join(ROOT, "tests", "host", "plan_host_main.cpp"),
                                         os.path.join(ROOT, "coeb-slam_amd", "csrc", "coeb_plan.cpp"), oracle_o, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
