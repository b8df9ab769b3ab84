"""tests/head_checker.py and tests/head_cases.py on the CPU: the independent model of a step's head against the oracle's own step
(orc_walk_step, _heatbath, _heg) in both disciplines, every case on the seam it is named for, and the model's deliberate mistakes,
each noticed by a named case.

The model and the oracle were written from the same Fortran lines by different routes: the oracle appends children walker by
walker inside move_uniform2's loop (or, threaded, from a prefix sum of its own); the model gates the whole list, takes np.repeat
for the parents and builds all records at once.  They share the generator and the moves, which are not under test here.

Which deliberate mistake is caught by which case (test_every_mistake_is_noticed_by_its_named_case):
  nint_half_to_even              G_cutoff_0.5 (|w| = 2.5 and 4.5)
  wchild_divides_below_cutoff    G_weights_on_both_sides_of_their_draw_counter
  parent_last_of_ties_wrong      W_run1023_mid_block, W_run1024_before_block_start
  window_edge_off_by_one         W_next_parent_on_window_entry_1022, _1023 and _1024
  hint_block_start_exclusive     W_heavy_parents_at_offset_0_mod_256 (searched from parent_hint)
  flags_of_previous_parent       W_heavy_on_first_and_last_slot
  heatbath_slots_swapped         H_heatbath_two_slots_per_child
"""
import types

import numpy as np
import pytest

import anneal_checker as AC
import head_cases as HS
import head_checker as HC

_BUILT = {}


def built(oracle):
    """the first-step cases with the model's answers, built once per session (the GPU driver uses the same)"""
    if "first" not in _BUILT:
        _BUILT["consts"] = HC.kernel_constants()
        _BUILT["first"] = HS.build_first_step(oracle, _BUILT["consts"])
        _BUILT["systems"] = HS.Systems(oracle)
    return _BUILT["first"], _BUILT["systems"], _BUILT["consts"]


def by_name(cases, name):
    return [c for c in cases if c["name"] == name][0]


def test_nint_rounds_halves_away_from_zero():
    for a, n in ((0.0, 0), (0.5, 1), (0.5 - 2.0 ** -54, 0), (1.5, 2), (1.5 - 2.0 ** -52, 1), (2.5, 3), (3.5, 4), (2.0 ** 20 + 0.5, 2 ** 20 + 1), (0.49999999999999994, 0)):
        assert HC.nint(a) == n, a
    assert HC.nint(2.5, half_to_even=True) == 2 and HC.nint(3.5, half_to_even=True) == 4 and HC.nint(0.5, half_to_even=True) == 0


def test_gate_on_the_named_weights(oracle):
    """do_walk.f90:3577-3593 on set G's weights: the counts and child weights, stated here once more by hand"""
    never = lambda i: 1.0          # a draw that never spawns;  always: 0.0 < |w / cutoff| for every non-zero w
    always = lambda i: 0.0
    w = np.array([0.5, 1.5, -2.5, 1.5 - 2.0 ** -52, 0.5 - 2.0 ** -54, -0.25, 0.0, 2.0 ** -31, 2.0 ** 20 + 0.5, -4.5])
    n, wc = HC.gate(dict(wt=w), dict(always_spawn_cutoff_wt=0.5), never)
    assert n.tolist() == [1, 2, 3, 1, 0, 0, 0, 0, 2 ** 20 + 1, 5]
    assert wc.tolist() == [0.5, 0.75, -2.5 / 3, 1.5 - 2.0 ** -52, 0.0, 0.0, 0.0, 0.0, (2.0 ** 20 + 0.5) / (2 ** 20 + 1), -0.9]
    n, wc = HC.gate(dict(wt=w), dict(always_spawn_cutoff_wt=0.5), always)
    assert n.tolist() == [1, 2, 3, 1, 1, 1, 0, 1, 2 ** 20 + 1, 5] and wc[4] == 0.5 and wc[5] == -0.5 and wc[7] == 0.5          # |w| = 0: 0 < 0 fails
    n, wc = HC.gate(dict(wt=np.array([0.25, 0.3, -0.4, 0.5 - 2.0 ** -54, 0.2])), dict(always_spawn_cutoff_wt=0.25), never)
    assert n.tolist() == [1, 1, 1, 1, 0] and wc.tolist()[:4] == [0.25, 0.3, -0.4, 0.5 - 2.0 ** -54]          # nint = 0 -> one child of w
    n, wc = HC.gate(dict(wt=np.array([0.0, -0.0, 2.0 ** -1000, -0.3])), dict(always_spawn_cutoff_wt=0.0), never)
    assert n.tolist() == [1, 1, 1, 1] and wc.tolist() == [0.0, -0.0, 2.0 ** -1000, -0.3]          # a cutoff of 0: nobody is below it


def test_records_carry_what_move_uniform2_sets():
    """3703-3726 flag by flag, saturation at 127 included"""
    wk = dict(imp_distance=np.array([0, -2, 1, 5, 126, 127], np.int8), initiator=np.array([1, 0, 2, 3, 1, 2], np.int8))
    par = np.arange(6)
    mv = (np.arange(6, dtype=np.uint64), np.arange(6, dtype=np.uint64), np.full(6, 0.125))
    wch = np.array([1.0, -2.0, 0.5, 3.0, 0.0, 0.3])
    r = HC.records(wk, dict(c_t_initiator=0, semistochastic=1), par, wch, mv)
    assert r["imp_distance"].tolist() == [-1, 2, 2, 6, 127, 127] and r["initiator"].tolist() == [1, 0, 1, 1, 0, 1]
    assert r["wt"].tolist() == [0.125, -0.25, 0.0625, 0.375, 0.0, 0.3 * 0.125]
    r = HC.records(wk, dict(c_t_initiator=1, semistochastic=0), par, wch, mv)
    assert r["imp_distance"].tolist() == [1, 1, 2, 6, 127, 127] and r["initiator"].tolist() == [0, 1, 1, 1, 0, 1]


def _oracle_step(oracle, systems, case, mode):
    sysm, _, hb = systems.get(case["system"])
    wk, prm = case["walkers"], case["prm"]
    n0 = len(wk["wt"])
    n_imp = int((wk["imp_distance"] == 0).sum())
    k = min(8, n0)
    setup = types.SimpleNamespace(ct_up=wk["up"][:k].copy(), ct_dn=wk["dn"][:k].copy(), ct_num=np.full(k, -0.5), ct_den=np.where(np.arange(k) == 0, 1.0, 0.0),
                                  prj_counts=np.ones(n_imp, np.int64), prj_indices=np.arange(1, n_imp + 1, dtype=np.int64), prj_values=np.zeros(n_imp))
    big = np.full(n0, 1e51)
    ow = oracle.OracleWalk(sysm, setup, dict(wk, matrix_elements=big, e_num=big, e_den=big), case["meta"]["mwalk"] + 16, list(HS.SEED), rng_mode=mode, heatbath=hb)
    st, out = ow.step(prm)
    after, rng = ow.walkers(), ow.rng_state()
    ow.close()
    return st, out, after, rng


@pytest.mark.parametrize("mode", [1, 0])
def test_model_equals_the_oracles_step(oracle, mode):
    """sets G, W, S and H at modest sizes: out[15] is the model's child count, and anneal_checker.fold of the model's records over the
    residents' weights in front of the merge gives the oracle's new list bit for bit; REPLAY's generator ends where the model's ends"""
    cases, systems, _ = built(oracle)
    n_run = 0
    for c in cases:
        if mode not in c["want"] or c["want"][mode]["n_children"] > 8000 or len(c["walkers"]["wt"]) > 5000 or c["meta"].get("status"):
            continue
        sysm = systems.get(c["system"])[0]
        wk, prm, want = c["walkers"], c["prm"], c["want"][mode]
        st, out, after, rng = _oracle_step(oracle, systems, c, mode)
        assert st == 0 and int(out[15]) == want["n_children"], (c["name"], st, out[15], want["n_children"])
        hii = np.array([sysm.ham(int(u), int(d), int(u), int(d)) for u, d in zip(wk["up"], wk["dn"])])
        res = dict(wk, wt=HC.residents_after(wk, prm, hii))
        m = AC.fold(res, want["rec"], prm, exact=False)
        for k in ("up", "dn", "wt", "imp_distance", "initiator"):
            assert np.array_equal(m[k], after[k]), (c["name"], k)
        if mode == 0:
            assert rng == want["rng"], c["name"]
        n_run += 1
    assert n_run >= (24 if mode else 20), n_run


def _counts(systems, c):
    """the model's child counts of a case in the COUNTER discipline, step 0"""
    st, up, dn = systems.streams(c["system"], 1), c["walkers"]["up"].tolist(), c["walkers"]["dn"].tolist()
    return HC.gate(c["walkers"], c["prm"], lambda i: st.gate_draw(up[i], dn[i]))[0]


def test_every_case_sits_on_the_seam_it_is_named_for(oracle):
    """layout() with the constants as compiled: the claims of every case hold (build_first_step asserts them; here once more, with the
    restated search finding np.repeat's parents from the narrowing and from parent_hint alike), and the counts stay within their caps"""
    cases, systems, consts = built(oracle)
    T, W, ST = consts["TPB"], consts["SPAWN_WIN"], consts["SCAN_TILE"]
    names = {c["name"] for c in cases}
    for c in cases:
        lay = c["layout"]
        assert HS.check_claims(lay, c["claims"]) is None, c["name"]
    # the searches, from both starting points, on the model's own counts
    for c in cases:
        if 1 not in c["want"] or c["layout"]["n_children"] > 20000:
            continue
        nchild = _counts(systems, c)
        assert int(nchild.sum()) == c["layout"]["n_children"]
        for hint in (False, True):
            assert np.array_equal(HC.search(nchild, consts, hint=hint)["parent"], HC.parents(nchild)), (c["name"], hint)
    for R in (W - 2, W - 1, W, W + 1):
        assert {"W_run%d_mid_block" % R, "W_run%d_before_block_start" % R} <= names
    for n0 in (W, W + 1, T * W, T * W + 1, ST - 1, ST, ST + 1, 2 * ST + 1):
        assert any(c["layout"]["n0"] == n0 for c in cases), n0
    big = [c for c in cases if c["layout"]["n0"] >= T * W]
    assert [c["layout"]["narrowing_rounds"] for c in big] == [1, 2] and all(c["layout"]["n_children"] <= 6000 for c in big)
    assert all(c["want"][0]["n_children"] <= HS.REPLAY_MAX_CHILDREN for c in cases if 0 in c["want"])
    assert sum(1 for c in cases if 0 in c["want"]) >= 20
    assert by_name(cases, "W_next_parent_on_window_entry_%d" % (W - 1))["layout"]["children_beyond_window"] == by_name(cases, "W_next_parent_on_window_entry_%d" % (W - 2))["layout"]["children_beyond_window"] + 1


def test_every_mistake_is_noticed_by_its_named_case(oracle):
    cases, systems, consts = built(oracle)
    W = consts["SPAWN_WIN"]

    def differs(name, hint=False, **mistake):
        c = by_name(cases, name)
        good = c["want"][1]
        mover = systems.get(c["system"])[1]
        bad = HC.head(c["walkers"], c["prm"], systems.streams(c["system"], 1), mover, consts, hint=hint, **mistake)
        return HS.compare(bad["rec"], good["rec"], good["n_children"], bad["n_children"], mover.slots) is not None

    assert not differs("G_cutoff_0.5") and not differs("W_heavy_parents_at_offset_0_mod_256", hint=True)          # no mistake: no difference
    assert differs("G_cutoff_0.5", nint_half_to_even=True)
    assert differs("G_weights_on_both_sides_of_their_draw_counter", wchild_divides_below_cutoff=True)
    for name in ("W_run%d_mid_block" % (W - 1), "W_run%d_before_block_start" % W):
        assert differs(name, parent_last_of_ties_wrong=True), name
    for k in (W - 2, W - 1, W):
        assert differs("W_next_parent_on_window_entry_%d" % k, window_edge_off_by_one=True), k
    assert not differs("W_children_0_mod_256", window_edge_off_by_one=True) and not differs("W_children_0_mod_256", parent_last_of_ties_wrong=True)
    assert differs("W_heavy_parents_at_offset_0_mod_256", hint=True, hint_block_start_exclusive=True)
    assert differs("W_heavy_on_first_and_last_slot", flags_of_previous_parent=True)
    assert differs("H_heatbath_two_slots_per_child", heatbath_slots_swapped=True)


def test_p_lists_are_built_for_their_seams(oracle):
    """set P's L0 (the three systems): its own head reaches the seams the second step is meant to meet -- the child repeats this on the
    list step 1 really leaves -- searched from parent_hint and from the narrowing"""
    _, systems, consts = built(oracle)
    for c in HS.build_p():
        nchild = _counts(systems, c)
        for hint in (False, True):
            assert HS.check_claims(HC.layout(nchild, consts, hint=hint), c["claims"]) is None, (c["name"], hint)
        assert (c["walkers"]["initiator"] == 1).all() and (c["walkers"]["wt"] != 0).all() and np.abs(c["walkers"]["wt"]).min() > c["prm"]["min_wt"]
