#!/usr/bin/env python3
"""Wall time of the Fuse search of LocalMapping::SearchInNeighbors on one MI355X, measured by
tests/adapter_shim/fuse_exec.cpp (`fuse_exec time T`) for 10 and 30 targets:
  * one coeb_kfdb_fuse_search for all targets, the snapshot of the point list included, against the work it
    replaces in the reference's thread: the search part of ORBmatcher::Fuse as a host loop on one thread over
    the same scene (keyframes of about 1000 features, half of them with MapPoints, true poses; the
    keyframes' grids prebuilt, as KeyFrame::mGrid is), and against T one-job calls of the same build (launch
    and copy floor only); the three alternate within every round;
  * direction 2: the targets' deduplicated points against the current keyframe, one call against the loop;
  * the device time of k_fuse per launch (the library's HIP-event profiler, in rounds of their own).
Median of 7 rounds of 20 calls with the range; profiler off for the wall times.

  python tools/fuse_time.py [out.json]
"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "adapter_shim")


def main():
    lib_dir = os.path.join(ROOT, "coeb-slam_amd", "lib")
    exe = os.path.join(tempfile.mkdtemp(), "fuse_exec")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-I", SHIM, "-I", os.path.join(ROOT, "coeb-slam_amd", "adapter"),
                           "-I", os.path.join(ROOT, "include"), os.path.join(SHIM, "fuse_exec.cpp"), "-o", exe, "-L", lib_dir,
                           "-lcoeb_front", "-Wl,-rpath," + lib_dir, "-Wl,-rpath-link,/opt/rocm/lib"])
    out = {}
    for T in (10, 30):
        r = json.loads(subprocess.run([exe, "time", str(T)], check=True, capture_output=True, text=True, timeout=600).stdout)
        r["host_over_call"] = round(r["host_loop_search"]["median_us"] / r["one_call_with_snapshot"]["median_us"], 2)
        r["direction2_host_over_call"] = round(r["direction2_host_loop"]["median_us"] / r["direction2_one_call"]["median_us"], 2)
        out["targets_%d" % T] = r
    text = json.dumps(out, indent=1)
    print(text)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        open(sys.argv[1], "w").write(text + "\n")


if __name__ == "__main__":
    main()
