#!/usr/bin/env python3
"""Survivors of k_fast's pixel pre-test per FAST cell, for pre-tests of 2, 4, 6 and 8 opposite
ring pairs, on the bench frames (numpy only, no GPU).

    tools/fast_filter_counts.py [--frames 8] [--pass-cost 2:..,4:..,6:..,8:..]

A pre-test of depth n keeps a pixel iff, for the dark or for the bright sign, each of its first n
opposite ring pairs (order 0/8, 4/12, 2/10, 6/14, 1/9, 5/13, 3/11, 7/15) has a pixel beyond v -/+ t.
Every nine-pixel arc holds one pixel of each opposite pair, so each depth is a necessary condition
of a corner and the kernel's output does not depend on it; only the survivor count does.  Counted
over the kernel's own cell windows (ROI minus its 3-px inset) on every pyramid level, at the two
minTh values (7, and 10 for dynamic-area frames).  Prints the table of
profiles/r10/fast_filter_counts.md and, with the static cost of one pre-test pass per depth, the
cost model  passes x pass cost + 62 x ceil(survivors / 64)  averaged over cells.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "coeb-slam_amd"))

import orb_ref as R  # noqa: E402
from coeb_front import synth  # noqa: E402

PAIR_ORDER = (0, 4, 2, 6, 1, 5, 3, 7)


def survivors(lvl, t, depth):
    """bool (h, w): pixels passing the depth-pair pre-test at t (False on the 3-px border)"""
    a = lvl.astype(np.int32)
    h, w = a.shape
    v = a[3:h - 3, 3:w - 3]
    ring = [a[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in R.RING]
    dark = np.ones_like(v, bool)
    bright = np.ones_like(v, bool)
    for k in PAIR_ORDER[:depth]:
        dark &= np.minimum(ring[k], ring[k + 8]) < v - t
        bright &= np.maximum(ring[k], ring[k + 8]) > v + t
    out = np.zeros((h, w), bool)
    out[3:h - 3, 3:w - 3] = dark | bright
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--pass-cost", default="", help="static instructions of one pre-test pass, e.g. 2:70,4:94")
    a = ap.parse_args()
    cost = {int(k): float(v) for k, v in (p.split(":") for p in a.pass_cost.split(",") if p)}
    tab = R.Tables(1000, 1.2, 8)
    frames = synth.make_frames(640, 480, a.frames, seed=1000)
    depths = (8, 6, 4, 2)
    counts = {(t, d): [] for t in (7, 10) for d in depths}
    passes, corners = [], {7: [], 10: []}
    for f in frames:
        for lvl in R.pyramid(f, tab):
            h, w = lvl.shape
            cells = R.level_cells(w, h)
            M = R.fast_strength(lvl)
            for t in (7, 10):
                S = {d: survivors(lvl, t, d) for d in depths}
                for _, _, x0, y0, x1, y1 in cells:
                    for d in depths:
                        counts[(t, d)].append(int(S[d][y0 + 3:y1 - 3, x0 + 3:x1 - 3].sum()))
                    corners[t].append(int((M[y0 + 3:y1 - 3, x0 + 3:x1 - 3] > t).sum()))
            for _, _, x0, y0, x1, y1 in cells:
                ww, wh = x1 - x0 - 6, y1 - y0 - 6
                rpi = 4 if (ww + 3) // 4 > 8 else 8            # window rows per pre-test pass
                passes.append(-(-wh // rpi))
    passes = np.array(passes)
    print("%d frames, %d cells; pre-test passes per cell: mean %.2f" % (len(frames), len(passes), passes.mean()))
    print("| minTh | pairs | mean | p95 | max | > 64 | > 128 | > 192 | strength blocks | model cost |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for t in (7, 10):
        for d in depths:
            c = np.array(counts[(t, d)])
            blocks = np.ceil(c / 64.0)
            model = "%.0f" % (passes * cost[d] + 62 * blocks).mean() if d in cost else "-"
            print("| %d | %d | %.1f | %d | %d | %.1f %% | %.1f %% | %.1f %% | %.2f | %s |" % (
                t, d, c.mean(), np.percentile(c, 95), c.max(), 100 * (c > 64).mean(), 100 * (c > 128).mean(),
                100 * (c > 192).mean(), blocks.mean(), model))
        print("| %d | corners | %.1f | %d | %d | | | | | |" % (
            t, np.mean(corners[t]), np.percentile(corners[t], 95), np.max(corners[t])))


if __name__ == "__main__":
    main()
