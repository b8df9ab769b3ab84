"""tests/psit_checker.py on the CPU: the independent model of the hf_to_psit step against the oracle's restatement
(oracle/sqmc_oracle_psit.c) on the C2 walk, bit for bit in both sum orders; its three forms of every long sum against their bound;
and its deliberate mistakes, each noticed by named cases of tests/psit_cases.py.

The two were written from the same Fortran lines by different routes: the oracle keeps the reference's three segments and its
running scans, the model folds per determinant (a dict for C(T), anneal_checker.fold for the rest) and shares no code with it.

Which deliberate mistake is caught by which case (test_every_mistake_is_caught_by_its_named_cases):
  chunk_off_by_one      H: every case with a sum that ends in a partial chunk, e.g. H_nct65_np65_q, H_nct4097_np1025_{q,f}
  drop_last_block       H: H_nct4097_np1025_q (C(T) row), H_nct8193_np4096_f, H_nct16421_np4098_q (also T^-1's sum: 4097 terms)
  tinv_from_premerge    T: psit_on_a_tiles_last_and_first_slot, ct_residents_cancelled_to_zero
  discard_ct_zero       T: ct_residents_cancelled_to_zero
  cti_checks_all        H: the c_t_initiator = 1 cases: H_nct64_np64_q, H_nct4095_np66_q, H_nct4097_np1025_q, H_nct8193_np4096_f
  first_row_enum_raw    H: every case (e_den(1) /= 1 in all of them)
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import anneal_checker as AC
import psit_checker as PS

SEED = [1346, 5634, 6635, 4361]


def tables_of(s, q, prj_values=None):
    return dict(ct_up=s.ct_up, ct_dn=s.ct_dn, ct_num=s.ct_num, ct_den=s.ct_den, loc_psit=q.loc_psit, cdet=q.cdet, diag_elems=q.diag_elems, loc_imp=q.loc_imp,
                prj_counts=q.prj_counts, prj_indices=q.prj_indices, prj_values=q.prj_values if prj_values is None else prj_values)


def lockstep(oracle, sysm, s, q, nsteps, sum_order, w_begin=50.0, target=2000.0, draws=False, seed=SEED):
    """the oracle's walk step by step; the model is given the list the oracle stood on and the spawn records of its premerge(), and
    must give the oracle's premerge weights, its new list and its sums.  Returns what the steps went through."""
    wk = oracle.initial_walkers_psit(s, q, w_begin)
    ow = oracle.OracleWalk(sysm, s, wk, 400000, list(seed), rng_mode=1, psit=q, sum_order=sum_order)
    ow.debug_premerge()
    pc = oracle.PopControl(s.tau, s.e_trial0, target)
    w_abs = float(np.abs(wk["wt"]).sum())
    n_ct = len(s.ct_up)
    prj = q.prj_values.copy()
    sign0 = int(wk["perm_sign"][0])
    seen = dict(outside_spawns=0, outside_residents=0, discarded=0, on_ct=0, ratios=[], outs=[])
    L = oracle.lib()
    L.orc_det_rank.restype = C.c_uint64
    L.orc_det_rank.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64]
    L.orc_rng_seek.argtypes = [C.c_void_p, C.c_int, C.c_uint64]
    L.orc_rannyu.restype = C.c_double
    L.orc_rannyu.argtypes = [C.c_void_p]
    for it in range(nsteps):
        r = pc.pre_step(w_abs)
        if r != 1.0:
            ow.scale_projector(r); prj *= r
        prm = pc.params() if draws else pc.params(min_wt=0.0, cutoff=0.0)
        rng = oracle.Rng.from_buffer_copy(ow.w.rng)          # the generator alone, at this step: the COUNTER stream keyed by the determinant's rank

        def draw(up, dn):
            L.orc_rng_seek(C.byref(rng), 2, L.orc_det_rank(int(sysm.norb), int(sysm.ndn), up, dn))
            return L.orc_rannyu(C.byref(rng))
        before = ow.walkers()
        hii = before["matrix_elements"].copy()
        for i in range(n_ct, len(hii)):
            if hii[i] > 1e50:
                hii[i] = sysm.ham(int(before["up"][i]), int(before["dn"][i]), int(before["up"][i]), int(before["dn"][i]))
        tb = tables_of(s, q, prj)
        st, oc = ow.step(prm)
        assert st == 0
        po, n0 = ow.premerge()
        assert n0 == len(before["wt"])
        h = PS.head(dict(before, matrix_elements=hii), tb, prm)
        assert np.array_equal(h["wt"][sum_order], po["wt"][:n0]), (it, "head", np.nonzero(h["wt"][sum_order] != po["wt"][:n0])[0][:5])
        if not draws:
            assert int(oc[15]) == int(PS.children(before, prm).sum())
        flags = dict(before, perm_sign=np.where(np.arange(n0) == 0, sign0, 0))
        sp = {k: po[k][n0:] for k in ("up", "dn", "wt", "imp_distance", "initiator")}
        assert not np.any((sp["up"] == s.ct_up[0]) & (sp["dn"] == s.ct_dn[0])), "3676: nothing is spawned onto the first state"
        t = PS.tail(po["wt"][:n0], flags, sp, tb, prm, draw=draw if draws else None)
        seen["outs"].append(t[sum_order]["stats_seq"])
        after = ow.walkers()
        for k in ("up", "dn", "wt", "imp_distance", "initiator"):
            assert np.array_equal(t[sum_order][k], after[k]), (it, k)
        for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13):
            assert t[sum_order]["stats_seq"][k] == oc[k], (it, k, t[sum_order]["stats_seq"][k], oc[k])
        assert abs(t[sum_order]["stats"][14] - oc[14]) <= len(po["wt"]) * PS.U * oc[14]
        for sm in (h["sums"]["ct_row"], h["sums"]["psit_row"], t["sums"]["tinv"]):
            seen["ratios"].append(PS.within_bound(sm))
        ct = set(zip(s.ct_up.tolist(), s.ct_dn.tolist()))
        on_ct = sum((int(a), int(b)) in ct for a, b in zip(sp["up"], sp["dn"]))
        seen["on_ct"] += on_ct; seen["outside_spawns"] += len(sp["up"]) - on_ct
        seen["outside_residents"] += n0 - n_ct; seen["discarded"] += len(t["discarded"])
        r = pc.post_step(oc)
        if r != 1.0:
            ow.scale_projector(r); prj *= r
        w_abs = oc[1]
    seen["walkers"], seen["n_out"] = t[sum_order], len(t[sum_order]["up"]) - n_ct
    ow.close()
    return seen


@pytest.fixture(scope="module")
def small(oracle, c2_walk):
    s = oracle.setup_walk(c2_walk, 20, 100, 0.1, rediagonalize=True)
    return s, oracle.psit_setup(c2_walk, s)


@pytest.mark.parametrize("sum_order", [1, 0])
def test_head_and_tail_equal_the_oracle_bit_for_bit(oracle, c2_walk, small, sum_order):
    """from the first state alone through the first steps that spawn onto C(T), outside it, onto survivors outside it, and discard"""
    s, q = small
    seen = lockstep(oracle, c2_walk, s, q, 7, sum_order)
    assert seen["on_ct"] > 0 and seen["outside_spawns"] > 100 and seen["outside_residents"] > 100 and seen["discarded"] > 0, seen


def test_frozen_trajectory_is_reproduced_where_the_model_computes_it(oracle, c2_walk):
    """tests/golden/psit_c2_8steps.json, COUNTER discipline: the model -- given each step's spawn records and the generator's rounding
    draws -- reproduces the stored sums 0-13 of all eight steps in bits, the number of determinants outside C(T) and both checksums
    of the final list.  (Sum 14 is added in sorted order there and correctly rounded here; 15 counts the gate's draws.)"""
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "psit_c2_8steps.json")))
    s = oracle.setup_walk(c2_walk, 100, 1000, 0.1, coeffs="pt1")
    q = oracle.psit_setup(c2_walk, s)
    seen = lockstep(oracle, c2_walk, s, q, 8, 1, w_begin=gold["w_abs_gen_begin"], target=gold["w_target"], draws=True, seed=gold["seed"])
    gm = gold["modes"]["1"]
    for k in range(8):
        assert [float(x).hex() for x in seen["outs"][k][:14]] == gm["steps"][k][:14], k
    w = seen["walkers"]
    assert seen["n_out"] == gm["n_outside_ct"]
    assert int(np.bitwise_xor.reduce(w["up"] * np.uint64(0x9E3779B97F4A7C15) + w["dn"])) == gm["det_checksum"]
    assert float(np.sum(w["wt"] * np.arange(1, len(w["wt"]) + 1) % 7.0)).hex() == gm["wt_checksum"]


def test_three_forms_of_a_sum_and_their_bound():
    rng = np.random.default_rng(11)
    for n in (1, 2, 63, 64, 65, 4095, 4096, 4097, 8193, 12400, 64 ** 3):
        x = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)
        s = PS.ordered_sums(x.tolist())
        assert s["exact"] == sum(AC.Fraction(float(v)) for v in x.tolist()[:5000]) + (PS.exact_sum(x.tolist()[5000:]) if n > 5000 else 0)
        r = PS.within_bound(s)
        assert s["chain"][0] == n - 1 and s["chain"][1] <= 63 + 63 + 63 and s["chain"][1] <= s["chain"][0] and (n <= 128 or s["chain"][1] < s["chain"][0])
        assert max(r.values()) <= max(s["chain"].values())
    # the tree is the documented one: by hand at 130 terms (three chunks of 64, 64, 2)
    x = [float(v) for v in rng.standard_normal(130)]
    by_hand = (PS.left_to_right(x[:64]) + PS.left_to_right(x[64:128])) + (x[128] + x[129])
    assert PS.ordered_sums(x)["tree"] == by_hand
    assert PS.ordered_sums(x, chunk_off_by_one=True)["tree"] == (PS.left_to_right(x[:64]) + PS.left_to_right(x[64:128])) + x[128]
    y = [float(v) for v in rng.standard_normal(4097)]
    assert PS.ordered_sums(y, drop_last_block=True)["tree"] == PS.ordered_sums(y[:4096])["tree"]
    assert PS.ordered_sums([])["tree"] == 0.0 and PS.ordered_sums([])["lr"] == 0.0


def test_every_mistake_is_caught_by_its_named_cases(c2_walk):
    """each deliberate mistake of the model changes the bits the GPU test compares, on the cases named in this file's docstring"""
    import psit_cases as PC
    import test_psit_cases as TC
    b = TC.built(c2_walk)
    H = {c["name"]: c for c in b["H"]}
    T = {c["name"]: c for c in b["T"][2]}
    none = dict(up=np.zeros(0, np.uint64), dn=np.zeros(0, np.uint64), wt=np.zeros(0), imp_distance=np.zeros(0, np.int8), initiator=np.zeros(0, np.int8))

    def head_changes(name, order, **mistake):
        c = H[name]
        return not np.array_equal(PS.head(c["walkers"], c["tables"], c["prm"], **mistake)["wt"][order], c["head"][order])

    def tail_changes(case, res_wt, flags, sp, order, **mistake):
        a = PS.tail(res_wt, flags, sp, case["tables"], case["prm"])[order]
        m = PS.tail(res_wt, flags, sp, case["tables"], case["prm"], **mistake)[order]
        return len(a["wt"]) != len(m["wt"]) or any(not np.array_equal(a[k], m[k]) for k in ("up", "wt", "initiator"))
    for name in ("H_nct65_np65_q", "H_nct4097_np1025_q", "H_nct4097_np1025_f"):
        assert head_changes(name, 1, chunk_off_by_one=True) and not head_changes(name, 0, chunk_off_by_one=True), name
    x = [1.0 + 2.0 ** -k for k in range(1, 41)] * 205
    assert PS.ordered_sums(x[:4096], chunk_off_by_one=True)["tree"] == PS.ordered_sums(x[:4096])["tree"], "no partial chunk there"
    for name in ("H_nct4097_np1025_q", "H_nct8193_np4096_f", "H_nct16421_np4098_q"):
        assert head_changes(name, 1, drop_last_block=True), name
    assert not head_changes("H_nct4096_np1024_q", 1, drop_last_block=True)
    c = H["H_nct16421_np4098_q"]          # ... and in T^-1's sum, which has 4097 terms there
    assert tail_changes(c, c["head"][1], c["walkers"], none, 1, drop_last_block=True)
    for name in H:
        assert head_changes(name, 1, first_row_enum_raw=True) and head_changes(name, 0, first_row_enum_raw=True), name
    for name in ("H_nct4095_np66_q", "H_nct4097_np1025_q", "H_nct8193_np4096_f", "H_nct64_np64_q"):
        c = H[name]
        assert c["prm"]["c_t_initiator"] == 1 and tail_changes(c, c["head"][1], c["walkers"], none, 1, cti_checks_all=True), name
    for name, mistake in (("psit_on_a_tiles_last_and_first_slot", "tinv_from_premerge"), ("ct_residents_cancelled_to_zero", "discard_ct_zero"),
                          ("ct_residents_cancelled_to_zero", "tinv_from_premerge")):
        c = T[name]
        assert tail_changes(c, c["res"]["wt"], c["res"], c["sp"], 1, **{mistake: True}), (name, mistake)


def test_children_is_the_draw_free_gate():
    w = dict(wt=np.array([7.0, 0.2, -0.5, 1.5, -2.5, 2.49, 1e-9, -300.4]))
    assert PS.children(w, dict(always_spawn_cutoff_wt=0.0)).tolist() == [0, 1, 1, 2, 3, 2, 1, 300]
    with pytest.raises(AssertionError):
        PS.children(w, dict(always_spawn_cutoff_wt=0.5))
