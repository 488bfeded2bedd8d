"""A literal Python model of ORBextractor::DistributeOctTree, and directed candidate layouts.

Written from the reference's text (ExtractorNode::DivideNode, src/ORBextractor.cc:489-544, and
ORBextractor::DistributeOctTree, :546-769), statement by statement, not from the oracle's C
restatement (oracle/orb_oracle.c, oc_distribute_octree): tests/test_octree_ref.py compares the
two, so that each pins the other.

One thing the reference leaves open: `sort(vPrevSizeAndPointerToNode)` (:691) orders pairs of
equal size by the node's address.  As DESIGN.md s4.3 and the oracle's `seq` do, the model takes
the pointer order to be the allocation order: a node allocated later compares greater.

Float arithmetic: `static_cast<float>` expressions are evaluated here in double and rounded to
float32 (f32), which for one +, -, * or / of float32 operands gives the float32 result exactly.

The second half builds the test frames: isolated dots whose level-0 FAST candidates are known
in advance (dot_image, level0_candidates) and the layouts shared by tests/test_octree_ref.py
(CPU: each layout reaches the regime it is named after) and tests/test_gpu_octree_layouts.py.
"""
import math
import struct

import numpy as np

EDGE_THRESHOLD = 19


def f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def c_round(v):
    """round(float), half away from zero"""
    return int(math.floor(v + 0.5)) if v >= 0 else -int(math.floor(-v + 0.5))


class Node:
    """ExtractorNode (include/ORBextractor.h): corners as (x, y) ints, vKeys as indices into the
    input list, bNoMore; seq is the allocation order standing in for the node's address; prev /
    next are the std::list links (the node's `lit`)."""

    def __init__(self):
        self.UL = self.UR = self.BL = self.BR = (0, 0)
        self.keys = []
        self.no_more = False
        self.seq = -1
        self.prev = self.next = None


class NodeList:
    """std::list<ExtractorNode>: push_front, push_back, erase, size, iteration from begin()."""

    def __init__(self):
        self.head = self.tail = None
        self.size = 0
        self.nalloc = 0

    def _alloc(self, n):
        n.seq = self.nalloc
        self.nalloc += 1
        self.size += 1

    def push_back(self, n):
        self._alloc(n)
        n.prev, n.next = self.tail, None
        if self.tail is None:
            self.head = n
        else:
            self.tail.next = n
        self.tail = n

    def push_front(self, n):
        self._alloc(n)
        n.prev, n.next = None, self.head
        if self.head is None:
            self.tail = n
        else:
            self.head.prev = n
        self.head = n

    def erase(self, n):
        """returns the element after n, as list::erase does"""
        if n.prev is None:
            self.head = n.next
        else:
            n.prev.next = n.next
        if n.next is None:
            self.tail = n.prev
        else:
            n.next.prev = n.prev
        self.size -= 1
        return n.next


def divide_node(p, xs, ys):
    """ExtractorNode::DivideNode (:489-544): the four children n1..n4"""
    halfX = int(math.ceil(f32(f32(p.UR[0] - p.UL[0]) / 2)))
    halfY = int(math.ceil(f32(f32(p.BR[1] - p.UL[1]) / 2)))
    n1, n2, n3, n4 = Node(), Node(), Node(), Node()
    n1.UL = p.UL
    n1.UR = (p.UL[0] + halfX, p.UL[1])
    n1.BL = (p.UL[0], p.UL[1] + halfY)
    n1.BR = (p.UL[0] + halfX, p.UL[1] + halfY)
    n2.UL = n1.UR
    n2.UR = p.UR
    n2.BL = n1.BR
    n2.BR = (p.UR[0], p.UL[1] + halfY)
    n3.UL = n1.BL
    n3.UR = n1.BR
    n3.BL = p.BL
    n3.BR = (n1.BR[0], p.BL[1])
    n4.UL = n3.UR
    n4.UR = n2.BR
    n4.BL = n3.BR
    n4.BR = p.BR
    for k in p.keys:
        if xs[k] < n1.UR[0]:
            if ys[k] < n1.BR[1]:
                n1.keys.append(k)
            else:
                n3.keys.append(k)
        elif ys[k] < n1.BR[1]:
            n2.keys.append(k)
        else:
            n4.keys.append(k)
    for n in (n1, n2, n3, n4):
        if len(n.keys) == 1:
            n.no_more = True
    return n1, n2, n3, n4


def distribute(xs, ys, score, minX, maxX, minY, maxY, N):
    """DistributeOctTree(vToDistributeKeys, minX, maxX, minY, maxY, N) (:546-769) over the keys
    (xs[i], ys[i], response score[i]), coordinates relative to (minX, minY) as the caller passes
    them (:844-845).  Returns (kept, trace): kept is the list of input indices of vResultKeys,
    in its order; trace is a dict:
      nini            initial nodes (:550)
      ini_sizes       keys in each initial node before the empty ones are erased (:573-592)
      iterations      passes of the main loop (:601, the reference's `iteration`)
      final_phase     the sorted phase (:683-743) was entered
      final_rounds    passes of its loop
      exit            what set bFinish: "size>=N" or "size==prevSize" (:676 in the main loop,
                      :741 in the final phase), or "break" when the sweep left at :737-738
      sweep_left      with exit "break": entries of the sorted vector not yet divided
      max_equal_sizes largest number of entries of equal size in any sorted vector (:691)
      one_child_divisions  DivideNode calls that left exactly one non-empty child
      tied_max_nodes  result nodes whose largest response is held by more than one key
      mixed_nodes     result nodes that hold keys of more than one response
      multi_key_nodes result nodes with more than one key
    Sort ties (:691) are broken by allocation order, see the module docstring."""
    nIni = c_round(f32(f32(maxX - minX) / (maxY - minY)))
    assert nIni >= 1, "the reference divides by zero here"
    hX = f32(f32(maxX - minX) / nIni)
    trace = dict(nini=nIni, ini_sizes=[], iterations=0, final_phase=False, final_rounds=0, exit=None, sweep_left=0,
                 max_equal_sizes=0, one_child_divisions=0, tied_max_nodes=0, mixed_nodes=0, multi_key_nodes=0)
    lNodes = NodeList()
    vpIniNodes = []
    for i in range(nIni):
        ni = Node()
        ni.UL = (int(f32(hX * f32(i))), 0)
        ni.UR = (int(f32(hX * f32(i + 1))), 0)
        ni.BL = (ni.UL[0], maxY - minY)
        ni.BR = (ni.UR[0], maxY - minY)
        lNodes.push_back(ni)
        vpIniNodes.append(ni)
    for i in range(len(xs)):
        vpIniNodes[int(f32(f32(xs[i]) / hX))].keys.append(i)
    trace["ini_sizes"] = [len(n.keys) for n in vpIniNodes]

    lit = lNodes.head
    while lit is not None:
        if len(lit.keys) == 1:
            lit.no_more = True
            lit = lit.next
        elif len(lit.keys) == 0:
            lit = lNodes.erase(lit)
        else:
            lit = lit.next

    def add_children(children, vSize):
        """:628-667 / :698-733; returns how many children had more than one key"""
        nexp = 0
        nonempty = 0
        for c in children:
            if len(c.keys) > 0:
                nonempty += 1
                lNodes.push_front(c)
                if len(c.keys) > 1:
                    nexp += 1
                    vSize.append((len(c.keys), c))
        if nonempty == 1:
            trace["one_child_divisions"] += 1
        return nexp

    bFinish = False
    vSizeAndPointerToNode = []
    while not bFinish:
        trace["iterations"] += 1
        prevSize = lNodes.size
        lit = lNodes.head
        nToExpand = 0
        vSizeAndPointerToNode = []
        while lit is not None:
            if lit.no_more:
                lit = lit.next
                continue
            nToExpand += add_children(divide_node(lit, xs, ys), vSizeAndPointerToNode)
            lit = lNodes.erase(lit)
        if lNodes.size >= N or lNodes.size == prevSize:
            bFinish = True
            trace["exit"] = "size>=N" if lNodes.size >= N else "size==prevSize"
        elif lNodes.size + nToExpand * 3 > N:
            trace["final_phase"] = True
            while not bFinish:
                trace["final_rounds"] += 1
                prevSize = lNodes.size
                vPrev = vSizeAndPointerToNode
                vSizeAndPointerToNode = []
                vPrev.sort(key=lambda e: (e[0], e[1].seq))
                run = 0
                for j in range(len(vPrev)):
                    run = run + 1 if j and vPrev[j][0] == vPrev[j - 1][0] else 1
                    trace["max_equal_sizes"] = max(trace["max_equal_sizes"], run)
                broke = False
                for j in range(len(vPrev) - 1, -1, -1):
                    node = vPrev[j][1]
                    add_children(divide_node(node, xs, ys), vSizeAndPointerToNode)
                    lNodes.erase(node)
                    if lNodes.size >= N:
                        broke = True
                        trace["sweep_left"] = j
                        break
                if lNodes.size >= N or lNodes.size == prevSize:
                    bFinish = True
                    trace["exit"] = "break" if broke else ("size>=N" if lNodes.size >= N else "size==prevSize")

    kept = []
    lit = lNodes.head
    while lit is not None:
        best = lit.keys[0]
        maxResponse = score[best]
        for k in lit.keys[1:]:
            if score[k] > maxResponse:
                best = k
                maxResponse = score[k]
        kept.append(best)
        if len(lit.keys) > 1:
            trace["multi_key_nodes"] += 1
            if sum(1 for k in lit.keys if score[k] == maxResponse) > 1:
                trace["tied_max_nodes"] += 1
            if any(score[k] != maxResponse for k in lit.keys):
                trace["mixed_nodes"] += 1
        lit = lit.next
    return kept, trace


# ------------------------------------------------------------------ frames with known candidates
def dot_image(w, h, points, value=255, background=0):
    """(h, w) uint8 image of `background` with one pixel per point: points are (x, y) or
    (x, y, v) tuples, v defaulting to `value`."""
    img = np.full((h, w), background, np.uint8)
    for p in points:
        img[p[1], p[0]] = p[2] if len(p) > 2 else value
    return img


def fast_grid(w, h):
    """ComputeKeyPointsOctTree's cell grid of a w x h level (:795-809):
    (nCols, nRows, wCell, hCell, maxBorderX, maxBorderY)"""
    minB = EDGE_THRESHOLD - 3
    maxBX, maxBY = w - EDGE_THRESHOLD + 3, h - EDGE_THRESHOLD + 3
    width, height = f32(maxBX - minB), f32(maxBY - minB)
    nCols, nRows = int(f32(width / 30)), int(f32(height / 30))
    return nCols, nRows, int(math.ceil(f32(width / nCols))), int(math.ceil(f32(height / nRows))), maxBX, maxBY


def cells_per_level(level_sizes):
    """FAST cells the reference visits on each level (:811-829: rows with iniY >= maxBorderY - 3 and
    columns with iniX >= maxBorderX - 6 are skipped)"""
    out = []
    for w, h in level_sizes:
        nCols, nRows, wCell, hCell, maxBX, maxBY = fast_grid(w, h)
        rows = sum(1 for i in range(nRows) if 16 + i * hCell < maxBY - 3)
        cols = sum(1 for j in range(nCols) if 16 + j * wCell < maxBX - 6)
        out.append(rows * cols)
    return out


def level0_candidates(w, h, points, value=255, background=0, ini_th=20, min_th=7):
    """Level 0's vToDistributeKeys of dot_image(w, h, points, value, background), for isolated
    dots (at least 4 px from each other): (xs, ys, score, pts) in the reference's order.

    An isolated pixel brighter than a flat background by d is a FAST-9 corner for every
    threshold below d, of score d - 1, and nothing around it is one.  Cell (i, j) detects the
    pixels x in [19 + j wCell, 19 + (j + 1) wCell), y likewise, below w - 19 / h - 19 (the ROI
    of :831 inset by FAST's 3-px border); its keys come in raster order, those of iniThFAST, or
    when it has none those of minThFAST (:834-838), and cells are visited row-major (:811-850).
    The key of a dot at (x, y) is (x - 16, y - 16) (:844-845 add the cell offset to ROI
    coordinates).  pts are the dots behind the keys."""
    _, _, wCell, hCell, _, _ = fast_grid(w, h)
    cells = {}
    for p in points:
        x, y = p[0], p[1]
        d = (p[2] if len(p) > 2 else value) - background
        if not (19 <= x < w - 19 and 19 <= y < h - 19) or d <= min_th:
            continue
        cells.setdefault(((y - 19) // hCell, (x - 19) // wCell), []).append((y, x, d))
    xs, ys, score, pts = [], [], [], []
    for key in sorted(cells):
        dots = sorted(cells[key])
        strong = [q for q in dots if q[2] > ini_th]
        for y, x, d in strong or dots:
            xs.append(x - 16)
            ys.append(y - 16)
            score.append(d - 1)
            pts.append((x, y))
    return xs, ys, score, pts


def lattice(w, h, spacing, x0=20, y0=20, x1=None, y1=None):
    """dots at (x0 + a spacing, y0 + b spacing) below (w - 20, h - 20) or (x1, y1), row by row"""
    x1 = w - 20 if x1 is None else x1
    y1 = h - 20 if y1 is None else y1
    return [(x, y) for y in range(y0, y1, spacing) for x in range(x0, x1, spacing)]


def two_valued(points, low=200):
    """every third dot at `low`"""
    return [(p[0], p[1], low) if i % 3 == 2 else p for i, p in enumerate(points)]


# the key capacities of k_octree at launch (oct_launch_keys; pinned for 640x480 and the default
# parameters by tests/host/plan_host_main.cpp, check_oct_launch_keys): up to 64 frames, from 65
OCT_KEYS_SMALL_BATCH = 4096
OCT_KEYS_LARGE_BATCH = 1024
# the final phase's layout: the first FINAL_PHASE_DOTS dots of the spacing-12 lattice (found with
# the model; test_layouts_reach_their_regimes asserts what it reaches)
FINAL_PHASE_DOTS = 1500
AREA_BOX = (0.0, 0.0, 520.0, 400.0)          # 208 000 px > 200 000: area_flag


class Layout:
    """One test frame: w, h, points (see dot_image), value / background, the extractor inputs
    boxes / tm / blur, the pyramid's nlevels (1000 features and scale 1.2 throughout), and
    `regime`, the name test_layouts_reach_their_regimes checks."""

    def __init__(self, name, regime, w, h, points, value=255, background=0, boxes=None, tm=None, blur=None,
                 nlevels=8):
        self.name, self.regime, self.w, self.h, self.points = name, regime, w, h, points
        self.nlevels = nlevels
        self.value, self.background = value, background
        self.boxes, self.tm, self.blur = boxes, tm, blur

    def image(self):
        return dot_image(self.w, self.h, self.points, self.value, self.background)

    def candidates(self, area_flag=False):
        return level0_candidates(self.w, self.h, self.points, self.value, self.background,
                                 30 if area_flag else 20, 10 if area_flag else 7)


def tile_edge_points(w=640, h=480):
    """Dots on the first and last detected column / row of several cells, on the image-side
    limits 19 and w - 20 / h - 20, and one pixel outside them (which must not be detected).
    Dots that are neighbours across a cell border sit on different rows (columns), 8 px apart."""
    _, _, wCell, hCell, _, _ = fast_grid(w, h)
    pts = []
    for n, j in enumerate((0, 1, 7, 18)):                  # columns: last of cell j, first of cell j + 1
        pts.append((19 + j * wCell + wCell - 1, 100 + 16 * n))
        pts.append((19 + (j + 1) * wCell, 108 + 16 * n))
    for n, i in enumerate((0, 1, 6, 12)):                  # rows: last of cell i, first of cell i + 1
        pts.append((200 + 16 * n, 19 + i * hCell + hCell - 1))
        pts.append((208 + 16 * n, 19 + (i + 1) * hCell))
    pts += [(19, 40), (w - 20, 48), (18, 56), (w - 19, 64)]
    pts += [(300, 19), (308, h - 20), (316, 18), (324, h - 19)]
    pts += [(19, 19), (w - 20, h - 20), (19, h - 20), (w - 20, 19)]       # the four corners of the detected area
    return pts


def layouts():
    """Every directed layout, by name."""
    W, H = 640, 480
    out = []

    def add(*a, **k):
        out.append(Layout(*a, **k))

    for s in (12, 6):
        add("equal_scores_lattice_%d" % s, "equal_scores", W, H, lattice(W, H, s))
        add("two_valued_scores_%d" % s, "two_valued", W, H, two_valued(lattice(W, H, s)))
    add("cluster_straddling", "one_child_chain", W, H, lattice(W, H, 4, 300, 200, 340, 240))
    add("cluster_in_quadrant", "one_child_chain", W, H, lattice(W, H, 4, 100, 60, 140, 100))
    add("final_phase_ties", "final_phase_break", W, H, lattice(W, H, 12)[:FINAL_PHASE_DOTS])
    add("n_not_reached", "all_singletons", W, H, lattice(W, H, 40))
    raster = lattice(W, H, 4)
    for n in (OCT_KEYS_SMALL_BATCH - 1, OCT_KEYS_SMALL_BATCH, OCT_KEYS_SMALL_BATCH + 1):
        add("keys_%d" % n, "count", W, H, raster[:n])
    for n in (OCT_KEYS_LARGE_BATCH - 1, OCT_KEYS_LARGE_BATCH, OCT_KEYS_LARGE_BATCH + 1, 0, 1, 2):
        add("keys_%d" % n, "count", W, H, raster[:n])
    # 1280x360 runs with 7 levels: an eighth (357x100) would have nIni = round(325 / 68) = 5, and the
    # HIP plan supports at most 4 initial nodes (make_plan rejects the size, tests/host/plan_host_main.cpp)
    add("wide_1280", "nini4", 1280, 360, lattice(1280, 360, 8), nlevels=7)
    add("wide_960", "nini3", 960, 360, lattice(960, 360, 8))
    # 1280x360: the four initial nodes span 312 relative px each: a lattice, one dot, nothing, a lattice
    add("wide_sparse_nodes", "ini_empty_and_single", 1280, 360,
        lattice(1280, 360, 8, x1=320) + [(500, 180)] + lattice(1280, 360, 8, x0=960), nlevels=7)
    weak = lattice(W, H, 12)
    add("min_threshold_only", "min_th", W, H, weak, value=30, background=18)
    # (206, 110) lies in the cell of columns 205..235, rows 83..114, as the weak dots (212 / 224, 92 / 104) do
    add("strong_dot_in_weak_cell", "min_th_shared_cell", W, H, weak + [(206, 110, 255)], value=30, background=18)
    add("detection_tile_edges", "tile_edges", W, H, tile_edge_points(W, H))
    # 24 T_M points in the box: 24 * 10000 > 208 000 marks it (layer 1, :1145)
    tm = [(30.0 + 20 * i, 50.0 + 10 * i) for i in range(24)]
    add("area_flag", "area_cull", W, H, lattice(W, H, 6), boxes=np.array([AREA_BOX], np.float32),
        tm=np.array(tm, np.float32), blur=np.zeros(1, np.int32))
    return {l.name: l for l in out}


def area_cull(layout, xs, ys, score, pts):
    """CheckMovingKeyPoints before the octree (:854-858) for the area_flag layout at level 0:
    the mask is 0 on [int(xmin), int(xmax)) x [int(ymin), int(ymax)) and is looked up at the
    key's relative coordinates, i.e. 16 px up and left of the dot."""
    x0, y0, x1, y1 = (int(v) for v in layout.boxes[0])
    keep = [i for i in range(len(xs)) if not (x0 <= xs[i] < x1 and y0 <= ys[i] < y1)]
    return [xs[i] for i in keep], [ys[i] for i in keep], [score[i] for i in keep], [pts[i] for i in keep]
