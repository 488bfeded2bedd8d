"""The directed bag-of-words and keyframe-database inputs (tests/bow_cases.py) without a GPU:
every case reaches the path it is built for (facts of the reference's own result), every wrong
reading the references can be switched to (their `mut` argument) changes the expected output of
a named case, and the order-sensitive score separates four orders of one double sum."""
import numpy as np
import pytest

import bow_cases as B
import bow_ref as R
import kfdb_ref as K


# ------------------------------------------------------------------ the transform
@pytest.mark.parametrize("k", B.WIDE_K)
def test_wide_vocabulary_has_every_winner_and_every_tie(k):
    f = B.transform_facts("wide_k%d" % k)
    assert (f["k"], f["lanes"]) == (k, 32 if k > 16 else 16) and f["L"] >= 2 and f["min_children"] == 1
    assert f["strict"] == set(range(k))
    assert f["pairs"] == {(j, jj) for j in range(k) for jj in range(j + 1, k)}
    assert f["minus_one"] >= 1 or k == 2


@pytest.mark.parametrize("k", [3, 17])
def test_complement_vocabulary(k):
    f = B.transform_facts("complement_k%d" % k)
    assert f["all_256"] == [1, 3, k] and f["descended_256"] and f["lanes"] == (32 if k > 16 else 16)


def test_level_counts_and_depths():
    for k in (16, 20):
        f = B.transform_facts("level1_k%d" % k)
        assert f["L"] == 1 and f["walk_depths"] == [1] and f["strict"] == set(range(k)) and f["minus_one"] >= 1
        assert (0, k - 1) in f["pairs"] and ((15, 16) in f["pairs"]) == (k > 16)
    f = B.transform_facts("chain")
    assert (f["k"], f["L"]) == (2, 10) and f["walk_depths"] == list(range(1, 11)) and f["leaf_is_nid"] >= 5
    assert len(B.voc_args("chain")[2]) == 20
    # the ties at even levels leave the chain, those at odd levels stay on it
    walks = [len(tr) for tr in B.transform_traces("chain")][11:]
    assert walks == [10, 2, 10, 4, 10, 6, 10, 8, 10, 10]
    ref = B.voc_ref("depth")
    assert sorted(set(B.depths(ref)[nd] for nd in ref.word_node)) == [1, 2, 3, 4]
    for ls in (0, 1, 3, 4, 7):
        f = B.transform_facts("depth_ls%d" % ls)
        assert f["leaf_depths"] == [1, 2, 3, 4] and f["minus_one"] == 1
        assert (f["nodes"] == [-1, 0]) == (ls >= 4)                 # levelsup >= L: the root
        assert (f["leaf_is_nid"] > 0) == (ls < 3)


@pytest.mark.parametrize("k", [17, 16])
def test_counts_sit_on_the_groups_per_workgroup(k):
    per = 256 // (32 if k > 16 else 16)
    got = {n: B.transform_facts("count_k%d_n%d" % (k, n)) for n in B.COUNTS}
    assert all(f["n"] == n for n, f in got.items())
    for edge in (per, 2 * per):
        assert [got[n]["workgroups"] for n in (edge - 1, edge, edge + 1)] == [edge // per] * 2 + [edge // per + 1]


# ------------------------------------------------------------------ the CSR
def test_csr_cases():
    f = {nm: B.csr_facts(nm) for nm in set(B.CSR_TRANSFORM + B.CSR_MATCH)}
    assert (f["n1"]["n"], f["n1"]["nd"]) == (1, 1) and (f["all_minus"]["m"], f["all_minus"]["nd"]) == (0, 0)
    assert (f["one_node_4095"]["m"], f["one_node_4095"]["nd"]) == (4095, 1)
    for n in (1025, 4095):
        for way in ("asc", "desc"):
            assert f["distinct_%d_%s" % (n, way)]["nd"] == n and f["distinct_%d_%s" % (n, way)]["second_trip"]
    r = f["runs"]
    assert r["head_residues"] == [0, 1, 2, 3] and r["run_over_1024"] and r["node_over_index_1024"] and r["second_trip"]
    assert (f["sparse_4095"]["n"], f["sparse_4095"]["m"]) == (4095, 40)
    lab, valid = B.csr_labels("valid_mask")
    node = R.csr(lab, valid)[0]
    assert 14 in lab and 14 not in node and f["valid_mask"]["m"] == valid.sum() == len(lab) - 7
    for nd, which in ((23, 0), (26, -1)):
        assert not valid[np.flatnonzero(lab == nd)[which]] and valid[lab == nd].sum() == (lab == nd).sum() - 1
    # through the grid vocabulary the transform returns the labels' own CSR
    for nm in ("runs", "sparse_4095"):
        want = B.transform_ref("csr_" + nm)
        node, off, idx = R.csr(B.csr_labels(nm)[0])
        assert np.array_equal(want["fv_off"], off) and np.array_equal(want["fv_idx"], idx) and len(want["fv_node"]) == len(node)


def test_transform_ref_is_compute_bow():
    """bow_cases.transform_ref walks each distinct descriptor once; the result is compute_bow's."""
    for name in ("wide_k17", "complement_k3", "chain", "depth_ls1", "csr_runs", "csr_sparse_4095"):
        voc, desc, levelsup = B.transform_case(name)
        want, got = R.compute_bow(B.voc_ref(voc), desc, levelsup), B.transform_ref(name)
        assert set(want) == set(got) and all(np.array_equal(want[k], got[k]) and want[k].dtype == got[k].dtype for k in want), name


# ------------------------------------------------------------------ SearchByBoW scenes
@pytest.mark.parametrize("nnratio", [0.6, 0.7])
def test_list_lengths(nnratio):
    for n in B.LIST_LENGTHS:
        a, b = B.sub_trace("lists", nnratio, False, "len%d" % n)
        assert (a["len"], a["p1"], a["d1"], a["accepted"]) == (n, n - 1, 3, True)
        if n > 1:
            assert (b["p1"], b["d1"], b["accepted"], b["first_taken"]) == (0, 1, True, False)
        else:
            assert b["d1"] == 256 and not b["accepted"]


@pytest.mark.parametrize("nnratio", [0.6, 0.7, 1.5])
def test_lanes(nnratio):
    t = lambda sub: B.sub_trace("lanes", nnratio, False, sub)[0]       # noqa: E731
    for tag, p1, p2 in (("same_lane", 5, 69), ("diff_lane", 5, 70), ("same_lane_rev", 69, 5), ("diff_lane_rev", 70, 3)):
        acc, rej = t(tag + "_acc"), t(tag + "_rej")
        assert (acc["p1"], acc["p2"], acc["d1"], acc["b2"], acc["accepted"]) == (p1, p2, 2, 10, True)
        assert (rej["p1"], rej["p2"], rej["d1"], rej["b2"], rej["accepted"]) == (p1, p2, 8, 10, nnratio > 1)
        assert ((p1 - p2) % 64 == 0) == tag.startswith("same")
    for tag, p2 in (("tie_one_lane", 69), ("tie_two_lanes", 70)):
        r = t(tag)
        assert (r["p1"], r["p2"], r["d1"], r["b2"], r["accepted"]) == (5, p2, 4, 4, nnratio > 1)


def test_acceptance_edges():
    def accepted(nnratio):
        return {sub: B.sub_trace("edges", nnratio, False, sub)[0]["accepted"] for sub in B.scene("edges")["sub"]}
    a6, a7 = accepted(0.6), accepted(0.7)
    for sub, t in ((s, B.sub_trace("edges", 0.6, False, s)[0]) for s in B.scene("edges")["sub"]):
        if sub.startswith("e"):
            d1, b2 = (int(x) for x in sub[1:].replace("_rev", "").split("_"))
            assert (t["d1"], t["b2"]) == (d1, b2) and t["p1"] == (1 if sub.endswith("_rev") and b2 < 256 else 0)
    # float32: 0.6f * b2 rounds above d1 for these three, although 0.6 b2 = d1 in the rationals
    for d1, b2 in ((15, 25), (27, 45), (30, 50)):
        assert a6["e%d_%d" % (d1, b2)] and a6["e%d_%d_rev" % (d1, b2)] and not 10 * d1 < 6 * b2
        assert not float(d1) < 0.6 * b2
    assert not any(a7["seven_tenths_%d" % m] for m in range(1, 6)) and not a7["e7_10"] and not a7["e35_50"]
    for r in (a6, a7):
        assert r["e50_256"] and not r["e51_256"]
    assert a7["e34_50"] and not a6["e34_50"] and a6["e14_25"] and a6["e15_26"]
    # 0.6f * 5 and 0.6f * 10 are float32 ties that round to even, 3 and 6: rejected, although 0.6f > 0.6
    for d1, b2 in ((3, 5), (6, 10)):
        assert not a6["e%d_%d" % (d1, b2)] and float(d1) < float(np.float32(0.6)) * b2
        assert np.float32(0.6) * np.float32(b2) == np.float32(d1)


@pytest.mark.parametrize("nnratio", [0.6, 0.7])
def test_claim_chains(nnratio):
    for c in (1, 2, 3, 6):
        tr = B.sub_trace("chains", nnratio, False, "full%d" % c)
        assert [t["accepted"] for t in tr] == [True] * c + [False] and tr[-1]["d1"] == 256
        assert [t["p1"] for t in tr[:-1]] == list(range(c - 1, -1, -1)) and all(t["first_taken"] for t in tr[1:])
    tr = B.sub_trace("chains", nnratio, False, "chain130")
    assert [(t["p1"], t["accepted"]) for t in tr] == [(129, True), (65, True), (1, True), (0, False), (0, False)]
    assert tr[3]["d1"] == tr[3]["b2"] == 60


def test_longest_lists():
    m, nm, st, tr = B.match_ref("big_list", 0.7, False)
    t = [tr[i] for i in range(40)]
    assert t[0]["len"] == 4095 and [x["p1"] for x in t[:6]] == [4094, 2047, 64, 0, 4032, 63] and nm == 6
    assert 4094 == 63 * 64 + 62 and all(x["first_taken"] for x in t[1:]) and not any(x["accepted"] for x in t[6:])
    m, nm, st, tr = B.match_ref("big_kf", 0.7, False)
    assert nm == 3 and list(m) == [2, 0, 1] and len(tr) == 4095 and all(tr[i]["d1"] == 256 for i in range(3, 4095))


def _rot_outcome(name):
    m, nm, st, tr = B.match_ref(name, 0.7, True)
    sub = B.scene(name)["sub"]
    bins = {tag: tr[s["kf"][0]]["bin"] for tag, s in sub.items()}
    gone = {tag for tag, s in sub.items() if m[s["cur"][0]] < 0}
    assert st["rot_removed"] == len(gone) and nm == len(sub) - len(gone)
    return bins, gone


def test_third_maximum_on_the_edge():
    for max1 in (30, 31):
        bins, gone = _rot_outcome("rot%d" % max1)
        assert sorted(set(bins[x] for x in bins if x[0] == "a")) == [3] and bins["b0"] == 7 and bins["c0"] == 10
        assert gone == {"lone"} | ({"c0", "c1", "c2"} if max1 == 31 else set())
    assert B.match_ref("rot30", 0.7, False)[1] == len(B.scene("rot30")["sub"])


def test_rotation_bins_decide_who_survives():
    """Every special angle sits in a kept bin and survives; the bin a wrong reading would give it
    (rint: 0 and 4; a cast: 0, 1, 4, 11; no + 360: none; + 360 at rot = 0: 12) holds no kept maximum."""
    want = dict(rot_half=dict(half15=1, half135=5, negative20=1, negative270=9),
                rot_wrap=dict(half45=2, half45_below=2, below360=12, below360_b=12, below360_c=12, below360_d=12),
                rot_zero=dict(zero=0, zero360=0))
    f = np.float32(1.0) / np.float32(30.0)
    assert float(np.float32(15.0) * f) == 0.5 and float(np.float32(135.0) * f) == 4.5
    assert float(np.float32(44.999996) * f) == 1.5 < float(np.float32(45.0) * f)
    for name, sc in B.ROT_SCENES.items():
        bins, gone = _rot_outcome(name)
        assert {t: bins[t] for t in sc["special"]} == want[name]
        assert gone == set(sc["gone"]) and set(want[name].values()) <= set(sc["kept"])
        assert sorted(set(bins[t] for t in bins if t not in gone)) == sorted(sc["kept"])
    assert set(_rot_outcome("rot_wrap")[0][t] for t in B.ROT_SCENES["rot_wrap"]["gone"]) == {0}


def test_csr_scenes_spell_out_both_orders():
    for nm in B.CSR_MATCH:
        m = B.scene("csr_" + nm)
        match, nmatches, _, _ = B.match_ref("csr_" + nm, 1.5, False)
        kf = R.feature_vector(m["kf_node"], m["valid"])
        cur = R.feature_vector(m["cur_node"])
        want = np.full(len(match), -1, np.int32)
        for nd in kf:                                   # the r-th KeyFrame feature takes the r-th frame feature
            for a, b in zip(kf[nd], cur.get(nd, [])):
                want[b] = a
        assert np.array_equal(match, want) and nmatches == (want >= 0).sum(), nm


def test_database_scene():
    kfs, cur, cands, sub = B.db_scene()
    main = B.db_match_ref("main", 0.75, True)
    a, b, c = sub["skip"]["kf"]
    f0, f1 = sub["skip"]["cur"]
    assert (main[0][0][f0], main[0][0][f1]) == (a, c)                 # b skipped: c takes f1
    assert (main[1][0][f0], main[1][0][f1]) == (a, b) and c not in main[1][0]      # every feature valid: b takes it
    assert main[2][1] == 0 and main[3][1] == 0 and len(kfs[2]["node"]) == 0
    assert np.array_equal(main[0][0], main[5][0]) and not np.array_equal(main[0][0], main[1][0])
    assert len(cands["one"]) == 1 and len(cands["most"]) == 256
    assert len({(r[0].tobytes(), r[1]) for r in B.db_match_ref("most", 0.75, True)}) >= 5


# ------------------------------------------------------------------ database queries
def test_block_cases():
    for nq in (64, B.MAXF):
        f = B.query_facts("blocks_q%d" % nq)
        hits = [f["kfs"][s]["hits"] for s in range(12)]
        assert [f["kfs"][s]["nw"] for s in range(12)] == [63, 64, 65, 128, 129, 200, 200, 200, 200, 200, 1, 0]
        assert hits[:5] == [[4], [4], [3, 1], [2, 2], [3, 0, 1]]
        assert hits[5:10] == [[1, 1, 1, 1], [4, 0, 0, 0], [0, 0, 4, 0], [2, 0, 2, 0], [0, 0, 0, 1]]
        assert f["kfs"][9]["first_is_last"] and f["scored_slots"] == list(range(9)) and (f["max_common"], f["nq"]) == (4, nq)
        assert sorted(f["order"]) == list(range(11))
    f = B.query_facts("blocks_q1")
    assert f["nq"] == 1 and [f["kfs"][s]["common"] for s in range(5)] == [1, 1, 1, 0, 0] and f["order"] == [0, 1, 2]
    assert f["scored_slots"] == [0, 1, 2] and f["kfs"][1]["hits"] == [1]


@pytest.mark.parametrize("mx", B.MAX_COMMON)
def test_min_common_cases(mx):
    f = B.query_facts("min_common_%d" % mx)
    mn = {1: 0, 4: 3, 5: 4, 6: 4, 9: 7, 10: 8, 11: 8}[mx]
    assert (f["max_common"], f["min_common"]) == (mx, mn)
    assert [f["kfs"][s]["common"] for s in range(5)] == [mn, mx, mn + 1, 0, mn]
    assert f["scored_slots"] == [1, 2]                            # min_common words are not enough, one more is
    assert not f["kfs"][0]["scored"] and not f["kfs"][4]["scored"]


def test_slot_arrangements():
    for w in range(4):
        f = B.query_facts("wave_%d" % w)
        assert f["scored_slots"] == [w] and f["nslots"] == 4 and sorted(f["order"]) == [0, 1, 2, 3]
    f = B.query_facts("wg1_only")
    assert f["scored_slots"] == [6] and f["nslots"] == 8 and 1 not in f["order"]
    for ns in (1, 5, 9):
        f = B.query_facts("nslots_%d" % ns)
        assert f["nslots"] == ns and f["scored_slots"] == [ns - 1]
    ref = B.query_ref("erased_between")
    before, after = ref[4], ref[6]
    assert [s for s in range(4) if before["score"][s] != -1] == [0, 1, 2]
    assert [s for s in range(4) if after["score"][s] != -1] == [0, 2] and after["common"][1] == 0 and list(after["order"]) == [0, 2, 3]


def test_lifecycle_case():
    slots, ops = B.query_case("lifecycle")
    ref = B.query_ref("lifecycle")
    assert slots == 1 and [r for op, r in zip(ops, ref) if op[0] == "add"] == list(range(9)) + [0, 8, 0]
    queries = [r for op, r in zip(ops, ref) if op[0] == "query"]
    assert [len(q["common"]) for q in queries] == list(range(1, 10)) + [9, 9, 1]
    assert [list(q["order"]) for q in queries[:9]] == [list(range(n)) for n in range(1, 10)]      # one first word: insertion order
    assert list(queries[9]["order"]) == list(range(1, 8)) and list(queries[10]["order"]) == list(range(1, 8)) + [0, 8]


def test_order_sensitive_score_separates_the_sum_orders():
    bits = B.order_sensitive_bits()
    print({k or "sequential": hex(v) for k, v in bits.items()})
    assert bits[""] == 0x3F800000                                   # the midpoint, rounded to even
    assert bits["sum_reversed"] == bits["sum_pairwise"] == bits["sum_blocks64"] == 0x3F800001
    F, kf = B.order_sensitive()
    blocks = K.score_terms(F, kf)
    assert [len(b) for b in blocks] == [4, 8, 5] and K.l1_score(F, kf) == 1.0 + 2.0 ** -24
    f = B.query_facts("order_sensitive")
    assert f["scored_slots"] == [0, 1] and f["max_common"] == 17


# ------------------------------------------------------------------ every wrong reading is noticed
def _transform_out(name, mut):
    r = B.transform_ref(name, mut)
    return [r[k] for k in ("word", "node", "fv_node", "fv_off", "fv_idx")]


def _match_out(run, mut):
    m, nm, _, _ = B.match_ref(*run, mut)
    return [m, np.array(nm)]


def _db_out(which, mut):
    return [x for r in B.db_match_ref(which, 0.75, True, mut) for x in (r[0], np.array(r[1]))]


def _query_out(name, mut):
    out = []
    for r in B.query_ref(name, mut):
        if isinstance(r, dict):
            out += [r["common"], r["score"].view(np.uint32), r["order"], np.array([r["max_common"], r["min_common"]])]
    return out


# wrong reading -> the directed cases looked at (the first has to notice it)
NOTICED_BY = {
    "tie_last": [(_transform_out, "wide_k16"), (_transform_out, "wide_k2"), (_transform_out, "level1_k20")],
    "tie_15_16_lost": [(_transform_out, "wide_k17"), (_transform_out, "wide_k20"), (_transform_out, "complement_k17")],
    "sentinel_256": [(_transform_out, "complement_k3"), (_transform_out, "complement_k17")],
    "nid_level_off": [(_transform_out, "depth_ls1"), (_transform_out, "chain")],
    "ratio_le": [(_match_out, ("edges", 0.7, False))],
    "ratio_f64": [(_match_out, ("edges", 0.6, False))],
    "ratio_f64_of_f32": [(_match_out, ("edges", 0.6, False))],
    "rot_half_even": [(_match_out, ("rot_half", 0.7, True))],
    "rot_truncated": [(_match_out, ("rot_half", 0.7, True)), (_match_out, ("rot_wrap", 0.7, True))],
    "rot_no_360": [(_match_out, ("rot_half", 0.7, True))],
    "rot_wrap_12": [(_match_out, ("rot_wrap", 0.7, True))],
    "rot_le_zero": [(_match_out, ("rot_zero", 0.7, True))],
    "d1_lt_50": [(_match_out, ("edges", 0.7, False))],
    "taken_ignored": [(_match_out, ("chains", 0.7, False)), (_match_out, ("big_list", 0.7, False))],
    "taken_trip0_only": [(_match_out, ("chains", 0.7, False)), (_match_out, ("big_list", 0.7, False))],
    "b2_min_only": [(_match_out, ("lanes", 0.7, False))],
    "invalid_claims": [(_db_out, "main"), (_db_out, "one")],
    "csr_first_1024": [(_match_out, ("csr_runs", 1.5, False)), (_transform_out, "csr_runs")],
    "common_ge": [(_query_out, "min_common_5"), (_query_out, "min_common_11")],
    "sum_reversed": [(_query_out, "order_sensitive")],
    "sum_pairwise": [(_query_out, "order_sensitive")],
    "sum_blocks64": [(_query_out, "order_sensitive")],
    "carry_zero_block": [(_query_out, "blocks_q64"), (_query_out, "blocks_q200")],
}


@pytest.mark.parametrize("mut", [m for m in R.MUTATIONS + K.MUTATIONS if m != "min_common_f64"])
def test_every_wrong_reading_is_noticed(mut):
    noticed = []
    for out, case in NOTICED_BY[mut]:
        ref, bad = out(case, frozenset()), out(case, frozenset([mut]))
        if not all(np.array_equal(a, b) for a, b in zip(ref, bad)):
            noticed.append(case)
    print(mut, "is noticed by", noticed)
    assert NOTICED_BY[mut][0][1] in noticed


def test_min_common_in_double_cannot_differ():
    """max_common * 0.8 truncates alike in float32 and in double for every count a database can
    hold: 0.8f lies 1.5e-8 above 0.8 relatively, a quarter of a float32 ulp, so the product of a
    multiple of 5 rounds back to the integer and every other product is at least 0.2 from one.
    No input separates the two, so no directed case is asked to.  The bound is the API's:
    coeb_kfdb_create (csrc/coeb_kfdb.hip) rejects max_features > kBowMax = 4095, coeb_kfdb_add and
    coeb_kfdb_query reject nw > max_features, and max_common <= nw.  Should that limit be raised,
    widen this range: the two forms first differ far above it, and a case belongs there then."""
    for mx in range(0, 4096):
        assert K.min_common_words(mx) == K.min_common_words(mx, frozenset(["min_common_f64"])) == (4 * mx) // 5
