"""TrackReferenceKeyFrame on one host frame, timed from C++ (tools/track_ref_kf_c.cpp): the fused
coeb_track_reference_keyframe against coeb_bow_transform + coeb_match_bow + coeb_pose_optimization
with the host steps between, on the 1000 x 1000 scene of tests/trk_ref.py (the workload's own
size).  Writes the scene to a directory, runs the program and prints its JSON line.

usage: trk_time.py [--exe PATH] [--calls N] [--warm N] [--out FILE]"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("coeb-slam_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))


def write_scene(d, n_cur=1000, n_kf=1000):
    import bow_ref as B
    import trk_ref as R
    sc = R.scene(n_cur, n_kf)
    kf = sc["kf"]
    with open(os.path.join(d, "voc.txt"), "w") as f:
        f.write(B.voc_text(*sc["voc_args"]))
    for name, a in (("meta.i32", np.array([sc["levelsup"]], np.int32)),
                    ("cam.f32", np.array(list(sc["intr"]) + [R.W, R.H], np.float32)), ("T.f32", sc["Tcw"]),
                    ("kps.bin", sc["kps"]), ("desc.u8", sc["desc"]), ("ur.f32", sc["ur"]), ("k_valid.u8", kf["valid"]),
                    ("k_desc.u8", kf["desc"]), ("k_node.i32", np.asarray(kf["node"], np.int32)),
                    ("k_angle.f32", kf["angle"]), ("k_xw.f32", kf["xw"]), ("k_obs.i32", np.asarray(kf["obs"], np.int32))):
        np.ascontiguousarray(a).tofile(os.path.join(d, name))
    return R.reference(sc, True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exe", default=os.path.join(ROOT, "tools", "track_ref_kf_c"))
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warm", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        want = write_scene(d)
        r = subprocess.run([a.exe, d, str(a.calls), str(a.warm)], capture_output=True, text=True)
    sys.stderr.write(r.stderr)
    line = r.stdout.strip()
    print(line)
    print("reference: nmatches_bow %d ninliers_pose %d nmatches %d nmatches_map %d" % (
        want["nmatches_bow"], want["ninliers_pose"], want["nmatches"], want["nmatches_map"]), file=sys.stderr)
    if a.out and r.returncode == 0:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
