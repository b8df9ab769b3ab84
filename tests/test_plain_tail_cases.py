"""tests/plain_tail_cases.py on the CPU: every case is what its name says before a GPU sees it.

Placement: jp_tiles restates k_join_par's greedy packing, layout() puts every candidate of the merged list on its tile and slot,
and each case names the tiles, slots and chains it is about.  Exactness: sets B-D are dyadic (multiples of 2^-13, sums far below
2^53 quanta), set A passes anneal_checker.check_precondition and is join-free.  Case C: the model, with the oracle generator's
COUNTER stream for the cases' seed, meets the 5-sigma condition -- so the GPU assertion is about the kernel, not the seed.
Case D: the float path of the model is the Fraction path on a thinned copy, and the full list has its open chain on the window
boundary.

Which deliberate mistake of the model (anneal_checker.join_walker2) is caught by which case:
  close_at_ge            sum_equal_min_wt_inside_a_tile, sum_equal_min_wt_on_a_tiles_last_candidate
  carrier_inverted       every case with a join in its bits; by its statistics: carrier_of_4096_chains_per_sign (C)
  perm_initiator_joins   untouched_walkers_between_the_members_of_a_chain
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import anneal_checker as AC
import plain_tail_cases as PT
import test_gpu_anneal_edges as GE

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_BUILT = {}


def counter_draw(oracle):
    """the join draw of the oracle generator's COUNTER stream (stage 2, keyed by the later walker's index among the merged
    heads) for the seed of the cases, step 0.  The generator alone: the oracle's join is not asked."""
    L = oracle.lib()
    L.orc_rng_seek.argtypes = [C.c_void_p, C.c_int, C.c_uint64]
    L.orc_rannyu.restype = C.c_double
    L.orc_rannyu.argtypes = [C.c_void_p]
    L.orc_rng_set_mode.argtypes = [C.c_void_p, C.c_int]
    rng = oracle.Rng()
    L.orc_setrn(C.byref(rng), (C.c_int * 4)(*PT.SEED))
    L.orc_rng_set_mode(C.byref(rng), 1)

    def draw(i):
        L.orc_rng_seek(C.byref(rng), 2, int(i))
        return L.orc_rannyu(C.byref(rng))
    return draw


def built(oracle, c2_walk, c2_setup, which):
    """the cases of one set with the model's answers, built once per session: 'A', 'B', 'C', 'D' or 'D_thin'"""
    if "base" not in _BUILT:
        uu, ud, in_table = GE.universe(c2_setup)
        ct = {(int(c2_setup.ct_up[i]), int(c2_setup.ct_dn[i])): (float(c2_setup.ct_num[i]), float(c2_setup.ct_den[i])) for i in in_table}
        gu, gd = PT.generated_universe(int(c2_walk.norb), int(c2_walk.nup), int(c2_walk.ndn))
        _BUILT["base"] = dict(uu=uu, ud=ud, ct=ct, gu=gu, gd=gd, consts=PT.kernel_constants(), tables=GE.tables_of(c2_walk))
    base = _BUILT["base"]
    if which == "base":
        return base
    if which not in _BUILT:
        if which == "A":
            cases = PT.set_a(base["uu"], base["ud"])
        elif which == "B":
            cases = PT.build_join_cases(base["gu"], base["gd"], base["consts"])
        elif which == "C":
            cases = [PT.carrier_case(base["gu"], base["gd"])]
        else:
            cases = [PT.window_case(base["gu"], base["gd"], base["consts"], run_len=525 if which == "D" else 5)]
        _BUILT[which] = PT.solve(cases, base["ct"], counter_draw(oracle))
    return _BUILT[which]


def test_rannyu48_is_the_references_generator():
    gold = json.load(open(os.path.join(GOLD, "rannyu.json")))
    assert len(gold) == 2
    for rec in gold:
        x = PT.rannyu_seed(rec["seed"])
        mine = []
        for _ in range(len(rec["hex"])):
            x, r = PT.rannyu48(x)
            mine.append(r.hex())
        assert len(mine) == 1000 and mine == rec["hex"]
    assert PT.rannyu_limbs(PT.rannyu_seed((1, 2, 3, 4))) == [1, 2, 3, 5]


def test_jp_tiles_is_the_greedy_packing():
    k = dict(JP_TILE=2048, JP_CW=1024)
    assert PT.jp_tiles([1500, 600], k) == [(0, 1, 1500), (1, 2, 600)]
    assert PT.jp_tiles([1024, 1024, 0], k) == [(0, 3, 2048)]
    assert PT.jp_tiles([1025, 1024], k) == [(0, 1, 1025), (1, 2, 1024)]
    assert PT.jp_tiles([0] * 5, k) == [(0, 5, 0)]
    assert PT.jp_tiles([3] + [0] * 1023 + [0, 0], k) == [(0, 1024, 3), (1024, 1026, 0)]          # never across a window of JP_CW chunks
    assert PT.jp_tiles([2048, 2048], k) == [(0, 1, 2048), (1, 2, 2048)]


def test_set_a_is_exact_and_join_free(oracle, c2_walk, c2_setup):
    cases = built(oracle, c2_walk, c2_setup, "A")
    T = built(oracle, c2_walk, c2_setup, "base")["consts"]["TPB"]
    assert T == 256 and len(cases) >= 35
    names = {c["name"] for c in cases}
    assert {"nall_%d" % n for n in (T - 1, T, T + 1, 2 * T, 3 * T + 1)} <= names and "run_ends_on_slot_T-1" in names and "every_run_64_or_65" in names
    for c in cases:
        assert c["prm"]["semistochastic"] == 0 and c["prm"]["min_wt"] == 0.25
        AC.check_precondition(c["res"], c["sp"], c["prm"])
        assert c["want"][1]["joins"] == 0 and not any(len(m) > 1 for s in (1, -1) for m, _, _ in c["chains"][s])
        assert not any(0 < abs(w) < 0.25 for w in c["heads"]["wt"])
        for k in ("up", "wt", "initiator"):
            assert np.array_equal(c["want"][0][k], c["want"][1][k])


def test_join_cases_sit_where_they_say(oracle, c2_walk, c2_setup):
    base = built(oracle, c2_walk, c2_setup, "base")
    consts = base["consts"]
    Ct = consts["JP_TILE"]
    cases = built(oracle, c2_walk, c2_setup, "B")
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names) >= 25
    for c in cases:
        assert PT.is_exact(c) and c["prm"]["min_wt"] == PT.MIN_WT and c["prm"]["r_initiator"] == -1.0, c["name"]
        assert int((c["res"]["imp_distance"] == 0).sum()) >= 1, c["name"]
        lay = PT.layout(c, c["heads"], consts)
        ch = PT.chains_by_ordinal(lay, c["chains"])
        meta = c["meta"]
        for sign, k, tile, slot in meta.get("pos", ()):
            assert lay["at"][sign][k] == (tile, slot), (c["name"], sign, k, lay["at"][sign][k], (tile, slot))
        for sign, first, last, closed in meta.get("chain", ()):
            hit = [x for x in ch[sign] if (first is None or x[0] == first) and (last is None or x[1] == last) and x[2] == closed]
            assert len(hit) == 1, (c["name"], sign, first, last, closed, ch[sign][:5])
        if "tiles" in meta:
            for sign, n in meta["tiles"].items():
                assert len(lay["tiles"][sign]) == n, (c["name"], lay["tiles"][sign])
        if "nall" in meta:
            assert lay["nall"] == meta["nall"], c["name"]
        if "joins" in meta:
            assert c["want"][1]["joins"] == meta["joins"], c["name"]
        for mode in (0, 1):          # what comes out is below min_wt only where a chain stayed open
            w = c["want"][mode]
            small = (np.abs(w["wt"]) < PT.MIN_WT * c["prm"]["reweight_factor_inv"]) & (w["initiator"] < 3)
            assert small.sum() <= 2, c["name"]
    by = {c["name"]: (c, PT.layout(c, c["heads"], consts)) for c in cases}
    for tag, sign in (("pos", 1), ("neg", -1)):
        c, lay = by["full_tile_of_single_quanta_" + tag]
        assert lay["tiles"][sign][0][2] == Ct and all(s < Ct for s in lay["slot"][lay["cand"][sign][:Ct]])          # nc == JP_TILE, the whole chunk candidates
        c, lay = by["chain_open_across_three_tiles_" + tag]
        assert [t[2] for t in lay["tiles"][sign][:3]][1] == Ct and len(lay["tiles"][sign]) == 3
    c, lay = by["signs_alternate_over_two_chunks"]
    order = sorted([(int(lay["slot"][h]), s) for s in (1, -1) for h in lay["cand"][s]])
    assert all(a[1] != b[1] and b[0] == a[0] + 1 for a, b in zip(order, order[1:])) and order[-1][0] > Ct
    for nall in (Ct - 1, Ct, Ct + 1, 2 * Ct, 2 * Ct + 1):
        c, lay = by["nall_%d" % nall]
        last = ((nall - 1) // Ct) * Ct
        slots = sorted(int(lay["slot"][h]) for s in (1, -1) for h in lay["cand"][s])
        assert slots[-1] == nall - 1 and (nall - last < 8 or (last in slots and last + 1 in slots and nall - 2 in slots))
    c, lay = by["every_slot_of_the_partial_last_chunk_a_candidate"]
    slots = sorted(int(lay["slot"][h]) for s in (1, -1) for h in lay["cand"][s])
    assert [x for x in slots if x >= Ct] == list(range(Ct, lay["nall"])) and lay["nall"] - Ct == 699
    c, lay = by["candidates_that_come_out_of_the_fold"]
    seam = c["meta"]["fold_seam"]
    assert seam in lay["slot"][lay["cand"][1]].tolist() and len(c["heads"]["up"]) < lay["nall"] - 12 and c["n_discarded"] >= 1
    c, lay = by["chains_across_the_staging_tiles_of_the_serial_join"]
    JT = c["meta"]["join_seam"]
    pos = lay["slot"][lay["cand"][1]].tolist()
    assert JT - 1 in pos and JT in pos
    neg = lay["slot"][lay["cand"][-1]].tolist()
    assert [x // JT for x in neg[:3]] == [0, 1, 2]


def test_each_deliberate_mistake_changes_a_named_case(oracle, c2_walk, c2_setup):
    by = {c["name"]: c for c in built(oracle, c2_walk, c2_setup, "B")}
    draw = counter_draw(oracle)

    def differs(name, **mistake):
        c = by[name]
        m = AC.plain_step(c["res"], c["sp"], c["prm"], draw, **mistake)
        w = c["want"][1]
        same = len(m["up"]) == len(w["up"]) and np.array_equal(m["up"], w["up"]) and np.array_equal(m["dn"], w["dn"]) and np.array_equal(m["wt"], w["wt"])
        return not same, AC.chain_layer(c["heads"], c["chains"], c["prm"], m)
    for name in ("sum_equal_min_wt_inside_a_tile", "sum_equal_min_wt_on_a_tiles_last_candidate"):
        d, layer = differs(name, close_at_ge=True)
        assert d and layer, name          # the draw-free layer sees it too: chains end elsewhere
    d, layer = differs("untouched_walkers_between_the_members_of_a_chain", perm_initiator_joins=True)
    assert d and layer
    d, layer = differs("chain_closes_on_a_tiles_last_candidate_pos", carrier_inverted=True)
    assert d and not layer                # another carrier, the same chains: only the bits (and case C's statistics) see it


def test_carrier_case_meets_its_bounds_with_the_counter_stream(oracle, c2_walk, c2_setup):
    (c,) = built(oracle, c2_walk, c2_setup, "C")
    assert PT.is_exact(c) and c["want"][1]["joins"] == 2 * 4096 * 3
    for sign in (1, -1):
        assert len(c["chains"][sign]) == 4096 and all(len(m) == 4 and closed and total == 9.0 / 16.0 for m, total, closed in c["chains"][sign])
    w = c["want"][1]
    why, counts = PT.carrier_verdict(c, w["up"], w["dn"], w["wt"])
    print("carriers per class (1, 2, 3, 3)/9 of 4096, model with the COUNTER stream:", counts, "bounds", [(round(a, 1), round(b, 1)) for a, b in PT.carrier_bounds()])
    assert why is None, why
    bad = AC.plain_step(c["res"], c["sp"], c["prm"], counter_draw(oracle), carrier_inverted=True)
    why, counts = PT.carrier_verdict(c, bad["up"], bad["dn"], bad["wt"])
    assert why is not None and counts is not None, "the inverted comparison of the draw falls outside the bounds"


def test_window_case(oracle, c2_walk, c2_setup):
    base = built(oracle, c2_walk, c2_setup, "base")
    consts = base["consts"]
    (thin,) = built(oracle, c2_walk, c2_setup, "D_thin")
    assert PT.is_exact(thin)
    ex = AC.plain_step(thin["res"], thin["sp"], thin["prm"], counter_draw(oracle), exact=True)
    for k in ("up", "dn", "wt", "imp_distance", "initiator"):
        assert np.array_equal(ex[k], thin["want"][1][k]), k          # the float path is the Fraction path
    assert ex["joins"] == thin["want"][1]["joins"] > 300
    (c,) = built(oracle, c2_walk, c2_setup, "D")
    assert PT.is_exact(c)
    lay = PT.layout(c, c["heads"], consts)
    Bd, Ct, W = c["meta"]["boundary"], consts["JP_TILE"], consts["JP_CW"]
    assert Bd == Ct * W < lay["nall"] == c["meta"]["nall"] and c["meta"]["mwalk"] > 2200000
    assert len(lay["tiles"][1]) == 2 and lay["tiles"][1][0][:2] == (0, W) and lay["tiles"][1][1][0] == W and lay["tiles"][1][1][2] > 100
    assert len(lay["tiles"][-1]) == 2 and lay["tiles"][-1][1] == (W, (lay["nall"] + Ct - 1) // Ct, 0)          # no candidate, and the chain in front is open:
    ch = PT.chains_by_ordinal(lay, c["chains"])
    assert ch[-1][-1][2] is False
    pos_slots = lay["slot"][lay["cand"][1]]
    across = [x for x in ch[1] if pos_slots[x[0]] < Bd <= pos_slots[x[1]]]
    assert len(across) == 1 and across[0][2] and Bd - 1 in pos_slots.tolist() and Bd in pos_slots.tolist()
    assert sum(1 for x in ch[1] if pos_slots[x[0]] > Bd and x[2]) >= 10          # further chains begin and close behind the boundary
    assert max(int(lay["slot"][h]) for s in (1, -1) for h in lay["cand"][s]) < (lay["nall"] // Ct) * Ct          # none in the partial last chunk
    assert 300 < c["want"][1]["joins"] < 1000
