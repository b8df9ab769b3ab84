"""tests/psit_cases.py on the CPU: every case is what its name says before a GPU sees it.

Set H: the named sizes are there, every C(T) slot carries weight, the gate and the rounding are draw-free; a quantised case has all
three forms of its head sums equal (any difference on the device is an indexing error), a full-mantissa case has tree and
left-to-right sums that DIFFER in bits (a case that could not tell the orders apart is not pinned), and every form lies within its
bound of the exact value.  Set T: each case sits on the tile and slot it names, by a restatement of the sorted order
(psit_cases.sorted_slots); it is exact, needs no draw, gives the same bits in both sum orders, and its named determinants end as the
reference's text says.  Nothing is skipped or compared loosely: asserted by count."""
import time

import numpy as np
import pytest

import anneal_checker as AC
import psit_cases as PC
import psit_checker as PS
import test_gpu_anneal_edges as GE

_BUILT = {}


def built(c2_walk):
    """the cases of both sets with the model's answers, built once per session"""
    if not _BUILT:
        t0 = time.time()
        uu, ud = PC.universe(int(c2_walk.norb), int(c2_walk.nup), int(c2_walk.ndn))
        assert len(uu) > PC.MAXTERMS + 1 and np.all((uu[1:] > uu[:-1]) | ((uu[1:] == uu[:-1]) & (ud[1:] > ud[:-1])))
        consts = PC.kernel_constants()
        H = PC.build_h_cases(uu, ud)
        sums = {c["name"]: PC.solve_h(c) for c in H}
        T, draws = {}, 0
        for items in (2, 3):
            T[items] = PC.build_t_cases(uu, ud, consts["TPB"] * items, consts)
            for c in T[items]:
                try:
                    PC.solve_t(c)
                except AC.NeedsDraw:
                    draws += 1
        _BUILT.update(uu=uu, ud=ud, consts=consts, H=H, sums=sums, T=T, draws=draws, tables=GE.tables_of(c2_walk), seconds=time.time() - t0)
        print("psit cases and the model's answers: %.1f s on the CPU" % _BUILT["seconds"])
    return _BUILT


def test_set_h_has_the_named_shapes(c2_walk):
    b = built(c2_walk)
    H = b["H"]
    n_ct = {c["meta"]["n_ct"] for c in H}
    npm1 = {c["meta"]["n_psit"] - 1 for c in H}
    assert {1, 63, 64, 65, 4095, 4096, 4097, 8192, 8193, 3 * 4096 + 37, 64 ** 3} <= n_ct
    assert {0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 2 * 4096 + 29} <= npm1
    assert len({(c["meta"]["n_ct"], c["meta"]["n_psit"]) for c in H}) == len(PC.H_PAIRS) == 14
    assert {c["meta"]["n_imp"] for c in H} == {1, 4, 5}
    assert {(c["meta"]["cti"], c["meta"]["perm"]) for c in H} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert {c["meta"]["spread"] for c in H} == {True, False}
    both = neither = last = s4095 = 0
    for c in H:
        tb, wk, m = c["tables"], c["walkers"], c["meta"]
        assert m["n_psit"] <= m["n_ct"] and np.all(wk["wt"] != 0.0), "every C(T) slot carries weight"
        assert c["prm"]["always_spawn_cutoff_wt"] == 0.0 and c["prm"]["min_wt"] == 0.0 and c["prm"]["semistochastic"] == 1
        assert tb["loc_psit"][0] == 0 and tb["loc_imp"][0] == 0 and np.all(np.diff(tb["loc_psit"]) > 0) and tb["ct_den"][0] != 1.0
        assert (wk["initiator"][0] == 3) == bool(m["perm"]) and np.array_equal(np.nonzero(wk["imp_distance"] == 0)[0], tb["loc_imp"])
        assert c["n_children"] >= m["n_ct"] - 1 and m["mwalk"] < (1 << 20), "below the switch to three slots per thread"
        inter = set(tb["loc_psit"].tolist()) & set(tb["loc_imp"].tolist())
        both += len(inter) > 1
        neither += m["n_ct"] > len(set(tb["loc_psit"].tolist()) | set(tb["loc_imp"].tolist()))
        last += m["spread"] and tb["loc_psit"][-1] == m["n_ct"] - 1
        s4095 += {4095, 4096} <= set(tb["loc_psit"].tolist()) and m["spread"]
        if m["n_ct"] >= 63:
            assert {1, 2} <= set(wk["initiator"][1:].tolist()), "c_t_initiator needs slots a check would change"
    assert both >= 8 and neither >= 8 and last >= 6 and s4095 >= 4


def test_set_h_quantised_sums_are_exact_and_full_mantissa_orders_differ(c2_walk):
    b = built(c2_walk)
    worst = {"ct_row": 0.0, "psit_row": 0.0}
    n_f = 0
    for c in b["H"]:
        s, m = b["sums"][c["name"]], c["meta"]
        for name in ("ct_row", "psit_row"):
            r = PS.within_bound(s[name])
            worst[name] = max(worst[name], max(r.values()))
            if m["kind"] == "q":
                assert s[name]["lr"] == s[name]["tree"] and PS.Fraction(s[name]["lr"]) == s[name]["exact"], (c["name"], name)
        if m["kind"] == "q":
            assert np.array_equal(c["head"][0], c["head"][1])
        else:
            n_f += 1
            assert m["n_ct"] > 65 and s["ct_row"]["lr"] != s["ct_row"]["tree"], c["name"]
            assert c["head"][0][0] != c["head"][1][0], c["name"]
            if m["n_psit"] - 1 > 65:
                assert s["psit_row"]["lr"] != s["psit_row"]["tree"], c["name"]
            assert abs(float(s["ct_row"]["exact"])) < 1e-3 * float(s["ct_row"]["mass"]), "the row cancels"
    assert n_f == sum(1 for p in PC.H_PAIRS if 65 < p[0] < PC.MAXTERMS) == 8
    print("largest |form - exact| / (2^-53 sum|term|) of the head sums:", worst)


@pytest.mark.parametrize("items", [2, 3])
def test_set_t_sits_where_it_says(c2_walk, items):
    b = built(c2_walk)
    T = b["consts"]["TPB"] * items
    MS = b["consts"]["MERGE_SELF"]
    assert T == 256 * items and MS == 8
    cases = {c["name"]: c for c in b["T"][items]}
    assert b["draws"] == 0, "cases that would need a rounding draw"
    for c in cases.values():
        m = c["meta"]
        slot, n_live = PC.sorted_slots(c)
        assert n_live == m["slots"]
        for label, u, o, at in m["marks"]:
            assert slot[(u, o)] == at, (c["name"], label)
        for label, at in m.get("want_slots", {}).items():
            got = [s for (l, u, o, s) in m["marks"] if l == label]
            assert got == [at], (c["name"], label, got, at)
        w = np.concatenate([c["res"]["wt"], c["sp"]["wt"]]) * 4.0
        assert np.all(w == np.floor(w)) and np.abs(w).max() <= 16 and c["tables"]["cdet"][0] == 0.5 and np.all(c["tables"]["cdet"] * 4 == np.floor(c["tables"]["cdet"] * 4))
        assert set(np.unique(c["sp"]["imp_distance"]).tolist()) <= {-1, 1, 2, 3}
        for k in ("up", "dn", "wt", "imp_distance", "initiator"):
            assert np.array_equal(c["want"][0][k], c["want"][1][k]), (c["name"], k)
        n_ct = m["n_ct"]
        assert np.array_equal(c["want"][1]["up"][:n_ct], c["tables"]["ct_up"]), "all of C(T) stays"
        u, d = c["want"][1]["up"][n_ct:], c["want"][1]["dn"][n_ct:]
        assert np.all((u[1:] > u[:-1]) | ((u[1:] == u[:-1]) & (d[1:] > d[:-1])))
    for d in (-1, 0, 1):
        assert cases["nct_is_tile%+d" % d]["meta"]["n_ct"] == T + d
        c = cases["ct_boundary_on_slot_T%+d" % d]
        assert c["meta"]["n_ct"] + 5 == T + d and c["n_discarded"] >= 1
    for tag in ("one_sign", "mixed_signs"):
        c = cases["run_leaves_the_tile_into_hbm_" + tag]
        head = [s for (l, u, o, s) in c["meta"]["marks"] if l == "head_of_the_long_run"][0]
        assert head < T and head + 309 - T > 256
    c = cases["runs_of_%d_%d_64_65_followers_on_ct_residents" % (MS, MS + 1)]
    runs = sorted(np.unique(c["meta"]["sp_univ"], return_counts=True)[1].tolist())
    assert {MS, MS + 1, 64, 65} <= set(runs)
    # what the named determinants come to (reweight_factor_inv of the case applied)
    c = cases["ct_residents_cancelled_to_zero"]
    rfi = c["prm"]["reweight_factor_inv"]
    at = {l: (u, s) for (l, u, o, s) in c["meta"]["marks"]}
    have = {(int(a), int(bb)): (float(w), int(i)) for a, bb, w, i in zip(c["want"][1]["up"], c["want"][1]["dn"], c["want"][1]["wt"], c["want"][1]["imp_distance"])}
    det = lambda u: (int(b["uu"][u]), int(b["ud"][u]))
    w1 = c["want"][1]["wt"][0] / rfi
    assert have[det(at["cancelled_outside_det_space"][0])] == (0.0, -2) and have[det(at["cancelled_in_det_space"][0])] == (0.0, 0)
    assert have[det(at["cancelled_psit"][0])] == ((0.0 - 0.25 * w1) * rfi, -2), "a cancelled Psi_T determinant takes T^-1's share"
    assert have[det(at["minus_one_onto_distance_0"][0])] == (1.0 * rfi, 0) and have[det(at["minus_one_onto_distance_-2"][0])] == (1.5 * rfi, -2)
    c = cases["outside_ct_discards_new_determinants_q1_q2"]
    at = {l: u for (l, u, o, s) in c["meta"]["marks"]}
    have = {(int(a), int(bb)): (float(w), int(i)) for a, bb, w, i in zip(c["want"][1]["up"], c["want"][1]["dn"], c["want"][1]["wt"], c["want"][1]["imp_distance"])}
    rfi = c["prm"]["reweight_factor_inv"]
    for gone in ("survivor_discarded", "new_fails_the_initiator_test", "q1_first_survivor_discarded"):
        assert det(at[gone]) not in have, gone
    assert have[det(at["new_passes"])] == (0.5 * rfi, 2) and have[det(at["minus_one_becomes_one"])] == (0.75 * rfi, 1)
    assert have[det(at["q1_new_between_two_survivors"])] == (1.5 * rfi, 1) and have[det(at["q1_second_survivor"])] == (2.0 * rfi, 1)
    assert at["q1_first_survivor_discarded"] < at["q1_new_between_two_survivors"] < at["q1_second_survivor"]
    c = cases["outside_determinant_with_key_koff"]
    assert int(c["tables"]["ct_up"][0]) == int(b["uu"][2]) and (int(b["uu"][0]), int(b["ud"][0])) == ((1 << int(c2_walk.nup)) - 1, (1 << int(c2_walk.ndn)) - 1)
    assert det(0) not in {(int(a), int(bb)) for a, bb in zip(c["want"][1]["up"], c["want"][1]["dn"])} and c["prm"]["reweight_factor_inv"] == 0.5
    for n_all in ((1 << 20) - 1, 1 << 20):
        c = cases["sorted_slots_%d" % n_all]
        assert len(c["res"]["up"]) + len(c["sp"]["up"]) == n_all and c["meta"]["items"] == (2 if n_all < (1 << 20) else 3) and c["meta"]["only"] == PC.NO_SWITCH
        assert np.count_nonzero(c["sp"]["wt"]) < 200


def test_nothing_is_skipped_or_compared_loosely(c2_walk):
    b = built(c2_walk)
    every = b["H"] + b["T"][2] + b["T"][3]
    loose = [c["name"] for c in every if c["meta"].get("loose") or c["meta"].get("skip")]
    assert len(loose) == 0 and b["draws"] == 0
    # every case of every variant's file is run by psit_cases.main in both sum orders; its only filter is psit_cases.runs_in
    big = {"sorted_slots_%d" % n for n in ((1 << 20) - 1, 1 << 20)}
    limit = "H_nct%d_np%d_q" % (64 ** 3, 2 * 4096 + 30)
    ran_anywhere = set()
    for v in PC.VARIANTS:
        cases = b["H"] + b["T"][PC.VARIANTS[v][1]]
        ran = {(c["name"], o) for c in cases for o in (0, 1) if PC.runs_in(c, v, o)}
        ran_anywhere |= ran
        left_out = {(c["name"], o) for c in cases for o in (0, 1)} - ran
        assert {n for n, o in left_out} <= {limit} | (big if v not in PC.NO_SWITCH else set()), (v, left_out)
    assert ran_anywhere == {(c["name"], o) for c in b["H"] + b["T"][2] for o in (0, 1)}, "every case in both sum orders in some child"
    assert all("want" in c for c in b["T"][2] + b["T"][3]) and all("head" in c for c in b["H"])
