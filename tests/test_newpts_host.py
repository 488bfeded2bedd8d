"""The host half of coeb_kfdb_set_stereo / coeb_kfdb_create_new_map_points (stereo records, argument rules, the
unpacking of the downloaded rows) as a stand-alone program under ASan + UBSan (tests/host/newpts_host_main.cpp):
no Python process, no GPU."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "coeb-slam_amd", "csrc")
SAN = ["-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_host_code_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "newpts_host")
    cmd = ["g++", "-std=c++17"] + SAN + ["-I", os.path.join(ROOT, "include"), "-I", CSRC,
                                         os.path.join(ROOT, "tests", "host", "newpts_host_main.cpp"),
                                         os.path.join(CSRC, "coeb_kfdb_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
