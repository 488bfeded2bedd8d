"""k_octree (and k_fast in front of it) on directed candidate layouts, against the oracle, bit for
bit (MI355X only).

Natural images almost never give two keys of one node the same response, so a scatter that
permutes keys inside a node, or a sort that breaks size ties differently, is invisible on them.
The frames here are isolated dots on a flat background (tests/octree_ref.py): level 0's candidates
are exactly the dots, all of one or two responses, placed to reach one path of the kernel each.
tests/test_octree_ref.py (no GPU) asserts that every layout reaches the regime it is named after,
from a Python model of DistributeOctTree; here each frame's keypoints and descriptors must equal
the oracle's in order, and per level the FAST candidate count (cand_n summed over the level's
cells) and the kept count (lvl_n) must equal the oracle's ncand / nkept, so that a failure names
the stage.  Levels >= 1 see the resized dots: not controlled, still compared."""
import numpy as np
import pytest

import octree_ref as R
from test_gpu_parity import assert_same

pytestmark = pytest.mark.gpu

LAYOUTS = R.layouts()


@pytest.fixture(scope="module")
def ex(oracle_mod):
    return oracle_mod.Extractor()


def check_counts(ex, read, w, h, ref, tag):
    """per-level cand_n / lvl_n of the frame `read` reads, against the oracle's debug counts"""
    cells = R.cells_per_level(ex.level_sizes(w, h))
    cn = read("cand_n").view(np.int32)
    assert len(cn) == sum(cells), (tag, len(cn), cells)
    edges = np.concatenate([[0], np.cumsum(cells)])
    ncand = [int(cn[edges[l]:edges[l + 1]].sum()) for l in range(len(cells))]
    assert ncand == ref["ncand"], (tag, "FAST candidates per level", ncand, ref["ncand"])
    nkept = read("lvl_n").view(np.int32).tolist()
    assert nkept == ref["nkept"], (tag, "keypoints per level", nkept, ref["nkept"])


@pytest.fixture(scope="module")
def wide7(oracle_mod):
    """context and oracle extractor of the 7-level pyramid the 1280x360 layouts run with"""
    from coeb_front import Context
    c = Context(1000, 1.2, 7, 20, 7, max_width=1280, max_height=360)
    yield c, oracle_mod.Extractor(1000, 1.2, 7, 20, 7)
    c.close()


def run_layout(ctx, ex, name):
    lay = LAYOUTS[name]
    assert ex.nlevels == lay.nlevels
    img = lay.image()
    ref = ex.extract(img, lay.boxes, lay.tm, lay.blur, debug=True)
    assert ref["ncand"][0] == len(lay.candidates(bool(ref["area_flag"]))[0]), name
    k, d = ctx.extract(img, lay.boxes, lay.tm, lay.blur)
    check_counts(ex, ctx.debug_read, lay.w, lay.h, ref, name)
    assert_same(k, d, ref["kps"], ref["desc"], name)
    return ref


@pytest.mark.parametrize("spacing", [12, 6])
def test_equal_scores_lattice(ctx, ex, spacing):
    """Every node's maximum is tied: the first key of the node in the reference's key order must
    win.  Spacing 6 has more than 4096 candidates on levels 0..2: keys in the global buffers."""
    run_layout(ctx, ex, "equal_scores_lattice_%d" % spacing)


@pytest.mark.parametrize("spacing", [12, 6])
def test_two_valued_scores(ctx, ex, spacing):
    run_layout(ctx, ex, "two_valued_scores_%d" % spacing)


@pytest.mark.parametrize("name,kept", [("cluster_straddling", 2), ("cluster_in_quadrant", 1)])
def test_cluster_one_child_chains(ctx, ex, name, kept):
    """100 candidates in 40 x 40 px: once every node has a single non-empty child the list stops
    growing and `lNodes.size() == prevSize` (ORBextractor.cc:676) ends the loop with multi-key
    nodes: 2 keypoints where the cluster straddles the first split, 1 inside a quadrant."""
    ref = run_layout(ctx, ex, name)
    assert ref["nkept"][0] == kept


@pytest.mark.parametrize("name", ["final_phase_ties", "n_not_reached"])
def test_final_phase_ties(ctx, ex, name):
    run_layout(ctx, ex, name)


@pytest.mark.parametrize("n", [R.OCT_KEYS_SMALL_BATCH - 1, R.OCT_KEYS_SMALL_BATCH, R.OCT_KEYS_SMALL_BATCH + 1])
def test_key_capacity_single(ctx, ex, n):
    """One frame: level 0 one key below, at and one above the LDS key capacity of a small batch."""
    ref = run_layout(ctx, ex, "keys_%d" % n)
    assert ref["ncand"][0] == n


def test_key_capacity_batch(ex):
    """65 frames (F * L = 520 > 512: the plan's own key capacity) cycling through level-0 counts
    around that capacity and the smallest ones; every frame against its layout's oracle result.
    The same frames as a 64-frame batch (the doubled capacity) must give identical results."""
    from coeb_front.pipeline import BatchPipeline
    K = R.OCT_KEYS_LARGE_BATCH
    names = ["keys_%d" % n for n in (K - 1, K, K + 1, 0, 1, 2)]
    refs, imgs = {}, {}
    for n in names:
        imgs[n] = LAYOUTS[n].image()
        refs[n] = ex.extract(imgs[n], debug=True)
        assert refs[n]["ncand"][0] == int(n.split("_")[1])
    F = 65
    order = [names[f % len(names)] for f in range(F)]
    frames = np.stack([imgs[n] for n in order])
    got = {}
    for nf in (F, F - 1):
        bp = BatchPipeline(640, 480, nf)
        try:
            bp.ctx.set_batch_streams(1)          # one launch over all nf frames
            bp.load(frames[:nf])
            bp.run(match=False)
            bp.synchronize()
            out, _, _ = bp.results()
            if nf == F:
                for f in range(F):
                    tag = "batch f%d %s" % (f, order[f])
                    check_counts(ex, lambda what: bp.ctx.debug_read(what, f), 640, 480, refs[order[f]], tag)
                    assert_same(out[f][0], out[f][1], refs[order[f]]["kps"], refs[order[f]]["desc"], tag)
            got[nf] = out
        finally:
            bp.close()
    for f in range(F - 1):
        assert np.array_equal(got[F][f][0], got[F - 1][f][0]) and np.array_equal(got[F][f][1], got[F - 1][f][1]), f


@pytest.mark.parametrize("name", ["wide_1280", "wide_960", "wide_sparse_nodes"])
def test_wide(ctx, ex, wide7, name):
    """Four and three initial nodes; wide_sparse_nodes leaves one initial node empty (erased,
    :588-589) and one with a single dot (bNoMore, :583-587).  1280x360 with 7 levels: the plan
    supports up to 4 initial nodes, and an eighth level would have 5."""
    if LAYOUTS[name].nlevels == 7:
        ctx, ex = wide7
    run_layout(ctx, ex, name)


@pytest.mark.parametrize("name", ["min_threshold_only", "strong_dot_in_weak_cell"])
def test_min_threshold_only(ctx, ex, name):
    """Dots 12 above the background: candidates through the minThFAST retry alone (:834-838); a
    cell that also holds one strong dot reports only that one."""
    ref = run_layout(ctx, ex, name)
    assert ref["ncand"][0] == (1850 if name == "min_threshold_only" else 1847)


def test_detection_tile_edges(ctx, ex):
    """Dots on the first and last detected column and row of several cells and of the image; the
    four dots one pixel outside the detected area must not appear."""
    ref = run_layout(ctx, ex, "detection_tile_edges")
    lay = LAYOUTS["detection_tile_edges"]
    k0 = ref["kps"][ref["kps"]["octave"] == 0]
    seen = set(zip(k0["x"].astype(int).tolist(), k0["y"].astype(int).tolist()))
    inside = {(p[0], p[1]) for p in lay.points if 19 <= p[0] < lay.w - 19 and 19 <= p[1] < lay.h - 19}
    assert seen == inside and len(inside) == len(lay.points) - 4


def test_area_flag(ctx, ex):
    """One box over 200 000 px marked by its T_M points: thresholds 30 / 10, N = 0.7 N, and the
    cull before the octree (:854-858), which looks the mask up at the keys' relative coordinates."""
    ref = run_layout(ctx, ex, "area_flag")
    assert ref["area_flag"] == 1 and ref["ncand"][0] == 7400 and ref["nkept"][0] >= 151
