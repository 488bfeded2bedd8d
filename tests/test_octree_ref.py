"""DistributeOctTree twice: the oracle's C restatement (oc_distribute_octree) against the literal
Python model of tests/octree_ref.py, index list against index list in order, and the directed
layouts of tests/test_gpu_octree_layouts.py against the regimes they are named after (no GPU)."""
import numpy as np
import pytest

import octree_ref as R

# boxes (minX, maxX, minY, maxY) of 640x480, 1280x360, 960x360 and 716x360 levels: nIni 1, 4, 3, 2
BOXES = {1: (16, 624, 16, 464), 4: (16, 1264, 16, 344), 3: (16, 944, 16, 344), 2: (16, 700, 16, 344)}


@pytest.fixture(scope="module")
def extractors(oracle_mod):
    return {n: oracle_mod.Extractor(1000, 1.2, n, 20, 7) for n in (7, 8)}


def both(oracle_mod, xs, ys, score, box, N):
    kept, trace = R.distribute(list(map(int, xs)), list(map(int, ys)), list(map(int, score)), *box, N)
    got = oracle_mod.distribute_octree(xs, ys, score, *box, N)
    assert got.tolist() == kept, (len(xs), N, box, len(got), len(kept))
    return kept, trace


@pytest.mark.parametrize("scores", ["equal", "two_valued", "distinct"])
@pytest.mark.parametrize("nini", [1, 2, 3, 4])
def test_model_equals_oracle_on_random_points(oracle_mod, nini, scores):
    box = BOXES[nini]
    rng = np.random.default_rng(100 * nini + len(scores))
    seen = set()
    for n in (0, 1, 2, 3, 50, 1000, 5000):
        for N in (1, 2, 61, 217, 434, n + 10):
            xs = rng.integers(0, box[1] - box[0], n)
            ys = rng.integers(0, box[3] - box[2], n)
            if scores == "equal":
                s = np.full(n, 254)
            elif scores == "two_valued":
                s = rng.choice(np.array([199, 254]), n)
            else:
                s = rng.permutation(n) + 10
            kept, trace = both(oracle_mod, xs, ys, s, box, N)
            assert trace["nini"] == nini and len(set(kept)) == len(kept)
            if n == 0:
                assert kept == []
            seen.add(trace["exit"])
    assert seen == {"size>=N", "size==prevSize", "break"}


def test_hand_worked_case(oracle_mod):
    """Eight keys in the box [0, 8) x [0, 8), N = 6, worked through ORBextractor.cc:546-769 by hand.

    nIni = round(8 / 8) = 1, hX = 8: one node R = [0, 8] x [0, 8] with all keys (allocation 0).
    Main loop, pass 1: prevSize = 1.  DivideNode(R): halfX = halfY = 4.  n1 (x < 4, y < 4) =
    {0, 1, 7}, n2 (x >= 4, y < 4) = {2}, n3 (x < 4, y >= 4) = {3}, n4 = {4, 5, 6}.  push_front in
    that order (allocations 1..4): list n4, n3, n2, n1; nToExpand = 2,
    vSizeAndPointerToNode = [(3, n1), (3, n4)].  R erased; the children lie before the iterator,
    so the pass ends.  size 4 < 6 and != 1; 4 + 2 * 3 = 10 > 6: final phase.
    Round 1: prevSize = 4.  The sort leaves (3, n1), (3, n4): equal sizes, n1 allocated first.
    j = 1, n4 = [4, 8] x [4, 8], halves 2: key 6 (5, 5) -> child 1 = {6}; keys 4 (6, 6) and 5
    (7, 7) -> child 4 = {4, 5}.  push_front {6} (allocation 5) then {4, 5} (6); n4 erased: size 5.
    j = 0, n1 = [0, 4] x [0, 4], halves 2: key 0 (1, 1) -> child 1, key 1 (2, 1) -> child 2, key 7
    (3, 3) -> child 4.  push_front {0}, {1}, {7}; n1 erased: size 7 >= 6: break at j = 0.
    (Had the tie been ordered the other way, n1 would go first, size 6 would break the sweep and
    n4 would stay whole: 6 results, not 7.)
    List: {7}, {1}, {0}, {4, 5}, {6}, {3}, {2}.  Best of {4, 5}: both 7, strict > keeps key 4."""
    xs = [1, 2, 6, 1, 6, 7, 5, 3]
    ys = [1, 1, 1, 6, 6, 7, 5, 3]
    score = [5, 5, 9, 3, 7, 7, 2, 6]
    kept, trace = both(oracle_mod, np.array(xs), np.array(ys), np.array(score), (0, 8, 0, 8), 6)
    assert kept == [7, 1, 0, 4, 6, 3, 2]
    assert trace == dict(nini=1, ini_sizes=[8], iterations=1, final_phase=True, final_rounds=1, exit="break",
                         sweep_left=0, max_equal_sizes=2, one_child_divisions=0, tied_max_nodes=1, mixed_nodes=0,
                         multi_key_nodes=1)
    # a strictly larger later response wins its node
    score[5] = 8
    kept, trace = both(oracle_mod, np.array(xs), np.array(ys), np.array(score), (0, 8, 0, 8), 6)
    assert kept == [7, 1, 0, 5, 6, 3, 2] and trace["tied_max_nodes"] == 0 and trace["mixed_nodes"] == 1
    # N = 5: the sweep stops after n4 (size 5), one sorted entry left, n1 whole with keys 0, 1 tied at 5
    score[5] = 7
    kept, trace = both(oracle_mod, np.array(xs), np.array(ys), np.array(score), (0, 8, 0, 8), 5)
    assert kept == [4, 6, 3, 2, 7] and trace["exit"] == "break" and trace["sweep_left"] == 1
    # N = 4: the main loop's own exit
    kept, trace = both(oracle_mod, np.array(xs), np.array(ys), np.array(score), (0, 8, 0, 8), 4)
    assert kept == [4, 3, 2, 7] and trace["exit"] == "size>=N" and not trace["final_phase"]


def check_regime(lay, r, ncand, n_in, kept, tr):
    """what each layout is there to reach, from the model's trace and the oracle's counts"""
    g = lay.regime
    if g == "equal_scores":
        assert tr["multi_key_nodes"] == len(kept) == tr["tied_max_nodes"] and tr["mixed_nodes"] == 0
        if lay.name.endswith("_6"):        # the global-key path of a single-frame call, three levels
            assert all(c > R.OCT_KEYS_SMALL_BATCH for c in r["ncand"][:3]), r["ncand"]
    elif g == "two_valued":
        assert tr["tied_max_nodes"] == len(kept) == tr["mixed_nodes"]
    elif g == "one_child_chain":
        assert tr["exit"] == "size==prevSize" and not tr["final_phase"]
        assert tr["one_child_divisions"] == len(kept) == tr["multi_key_nodes"] and ncand == 100
        assert len(kept) == (2 if lay.name == "cluster_straddling" else 1)
    elif g == "final_phase_break":
        assert tr["final_phase"] and tr["final_rounds"] >= 2 and tr["max_equal_sizes"] >= 8
        assert tr["exit"] == "break" and tr["sweep_left"] > 0
    elif g == "all_singletons":
        assert 100 < ncand == len(kept) < 217 and tr["multi_key_nodes"] == 0 and tr["exit"] == "size==prevSize"
    elif g == "count":
        assert ncand == int(lay.name.split("_")[1]) == len(lay.points)
    elif g in ("nini4", "nini3"):
        assert tr["nini"] == int(g[-1]) and min(tr["ini_sizes"]) > 1000
    elif g == "ini_empty_and_single":
        assert tr["nini"] == 4 and tr["ini_sizes"][1:3] == [1, 0] and min(tr["ini_sizes"][0], tr["ini_sizes"][3]) > 1000
    elif g == "min_th":
        assert ncand == len(lay.points) == 1850 and r["ncand"][1:] == [0] * (lay.nlevels - 1)
        assert lay.value - lay.background <= 20
    elif g == "min_th_shared_cell":
        assert ncand == len(lay.points) - 4      # the cell's four weak dots give way to the strong one
        assert tr["mixed_nodes"] == 1
    elif g == "tile_edges":
        assert ncand == len(lay.points) - 4 == len(kept)      # all but the four dots one px outside
    elif g == "area_cull":
        assert r["area_flag"] == 1 and ncand == len(lay.points) == 7400
        # relative coordinates 4 + 6 a, 4 + 6 b: 86 columns below 520 and 66 rows below 400 are culled
        assert n_in == 100 * 74 - 86 * 66 == 1724
        assert tr["final_phase"] and len(kept) >= 151
    else:
        raise AssertionError("unknown regime " + g)


@pytest.mark.parametrize("name", sorted(R.layouts()))
def test_layouts_reach_their_regimes(extractors, name):
    """Level 0 of every directed layout: the oracle finds exactly the dots as candidates, the
    model run on the candidate list rebuilt from the dots keeps what the oracle keeps, in order,
    and the model's trace shows the regime the layout exists for."""
    lay = R.layouts()[name]
    ex = extractors[lay.nlevels]
    r = ex.extract(lay.image(), lay.boxes, lay.tm, lay.blur, debug=True)
    area = bool(r["area_flag"])
    xs, ys, score, pts = lay.candidates(area)
    ncand = len(xs)
    assert r["ncand"][0] == ncand, (r["ncand"], ncand)
    if area:
        xs, ys, score, pts = R.area_cull(lay, xs, ys, score, pts)
    nfeat = ex.p.nfeat[0]
    N = int(nfeat * 0.7) if area else nfeat
    kept, tr = R.distribute(xs, ys, score, 16, lay.w - 16, 16, lay.h - 16, N)
    k0 = r["kps"][r["kps"]["octave"] == 0]
    assert r["nkept"][0] == len(k0) == len(kept), (r["nkept"], len(kept))
    assert k0["x"].tolist() == [float(pts[k][0]) for k in kept]
    assert k0["y"].tolist() == [float(pts[k][1]) for k in kept]
    assert k0["response"].tolist() == [float(score[k]) for k in kept]
    check_regime(lay, r, ncand, len(xs), kept, tr)
