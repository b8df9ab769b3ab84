"""The HIP proposal kernels and hamiltonian_batch against tests/proposal_checker.py, which shares nothing with them or with the
oracle: matrix elements against second quantisation within the derived rounding bound, 2^22 proposals per fixed parent through
the test doors against the exact row (closure, sign and size, G-test, reach, first moment), and one real RNG_COUNTER step from
a single heavy determinant against the projector row.  tests/test_proposal_unbiased.py runs the same on the CPU oracle."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from conftest import gpu_ctx_from_oracle, gpu_ctx_heg, gpu_ctx_hub          # noqa: E402
from tests import proposal_checker as PC                                    # noqa: E402
from tests import test_proposal_unbiased as TU                              # noqa: E402

pytestmark = pytest.mark.gpu
FCIDUMP = TU.FCIDUMP
N_GPU = 1 << 22
TAU = TU.TAU
SYSTEMS = ["c2_walk", "c2_hci", "heg14", "heg57", "hub44"]


@pytest.fixture(scope="module")
def c2_10e(oracle):
    return oracle.ChemSystem(FCIDUMP, 10, 5, "d2h", time_sym=False, hf_mode=0)


@pytest.fixture(scope="module")
def c2_10e_ts(oracle):
    return oracle.ChemSystem(FCIDUMP, 10, 5, "d2h", time_sym=True, z=1, hf_mode=0)


def _ctx(sysm, which, **kw):
    import sqmc_amd
    sqmc_amd.set_device(0)
    if which.startswith("heg"):
        return gpu_ctx_heg(sysm, **kw)
    if which.startswith("hub"):
        return gpu_ctx_hub(sysm, **kw)
    return gpu_ctx_from_oracle(sysm, **kw)


def _u64(v, n):
    return np.full(n, v, np.uint64)


@pytest.mark.parametrize("which", SYSTEMS)
def test_hamiltonian_batch_matches_second_quantisation(request, which):
    """hamiltonian_batch on the pair classes of test_hamiltonian_batch_bit_exact and on the ones it leaves out (the diagonal, three
    or more excitations apart, orbital 0 and orbital norb - 1 -- bit 56 for the 57 plane waves --, closed shells), then on
    TU.span_pairs: singles and doubles that empty orbital 0 and fill orbital norb - 1 of one string with that string's other
    electrons in between, so that the parity string spans the word (on the periodic 4 x 4 Hubbard lattice the widest hops,
    0 <-> 12 and 3 <-> 15): |H_gpu - H_ref| <= 4 n_terms 2^-53 sum|terms|, exact zeros exact, signs equal"""
    sysm = request.getfixturevalue(which)
    ts = which == "c2_hci"
    H = TU.chem_checker(sysm) if which.startswith("c2") else TU.heg_checker(sysm) if which.startswith("heg") else TU.hub_checker(sysm)
    pairs = TU.matrix_element_pairs(H.norb, sysm.nup, sysm.ndn, ts, seed=5, n_random=600 if which == "heg57" else 1200)
    if not which.startswith("c2"):
        par = (sysm.hf_up, sysm.hf_dn)
        ex = PC.excitations_heg(H, *par) if which.startswith("heg") else PC.excitations_hubbard(H, *par)
        pairs += [par + c for c in ex[:400]]
    span = TU.span_pairs(TU.children_of(H, which), sysm.nup, sysm.ndn, TU.span_ends(which, H.norb), ts)
    g = _ctx(sysm, which)
    try:
        a = np.array(pairs, dtype=np.uint64)
        got = g.hamiltonian_batch(a[:, 0], a[:, 1], a[:, 2], a[:, 3])
        a = np.array(span, dtype=np.uint64)
        got_span = g.hamiltonian_batch(a[:, 0], a[:, 1], a[:, 2], a[:, 3])
    finally:
        g.close()
    n_first = len(pairs)
    worst, nonzero, _ = TU.compare_elements(H, pairs[:n_first], got[:n_first].tolist(), ts)
    print("%s: %d pairs, %d with terms, worst |dH| / bound = %.3g" % (which, n_first, nonzero, worst))
    assert nonzero > n_first // 6
    worst, nonzero, live = TU.compare_elements(H, span, got_span.tolist(), ts)
    print("%s: %d pairs whose parity string spans the word, %d above their bound, worst |dH| / bound = %.3g" % (which, len(span), live, worst))
    assert live >= TU.MIN_SPANNING[which]


@pytest.mark.parametrize("which", SYSTEMS)
def test_uniform_door_is_unbiased(request, which):
    """propose_batch: 2^22 proposals per parent, one hashed rannyu state each, all five checks against the exact row"""
    sysm = request.getfixturevalue(which)
    kind = TU.UNIFORM[which][0]
    H, parents, children, ts = TU.uniform_case(sysm, which)
    if which == "c2_walk":
        parents = parents + [("second_double", (0x1e, 0x10e))]
    seeds = PC.state_limbs(PC.splitmix_states(N_GPU))
    g = _ctx(sysm, which)
    try:
        for name, par in parents:
            rowd = PC.row(H, par, children(par), ts)
            ju, jd, w, _ = g.propose_batch(TAU[kind], _u64(par[0], N_GPU), _u64(par[1], N_GPU), seeds)
            fails, rep = PC.analyse(rowd, par, ju, jd, w, TAU[kind], (sysm.nup, sysm.ndn), True, ts)
            TU._assert_clean("gpu %s/%s" % (which, name), fails, rep)
    finally:
        g.close()


@pytest.mark.parametrize("time_sym", [False, True])
def test_heatbath_door_is_unbiased(request, oracle, time_sym):
    """propose_heatbath_batch on the 10-electron system: closure, reach (an unvisited connected determinant must be one the move's
    own tables cannot or hardly ever reach) and the first moment of every child, both slots of every proposal"""
    sysm = request.getfixturevalue("c2_10e_ts" if time_sym else "c2_10e")
    hb = oracle.HeatBath(sysm)
    H = TU.chem_checker(sysm)
    seeds = PC.state_limbs(PC.splitmix_states(N_GPU))
    g = _ctx(sysm, "c2")
    try:
        g.set_heatbath_tables(hb.fortran_arrays())
        for name, par in PC.parents_chem(H, (sysm.hf_up, sysm.hf_dn), H.norb, time_sym):
            rowd = PC.row(H, par, PC.excitations_chem(par[0], par[1], H.norb), time_sym)
            ju, jd, w, _ = g.propose_heatbath_batch(TAU["hb"], _u64(par[0], N_GPU), _u64(par[1], N_GPU), seeds)
            fails, rep = PC.analyse(rowd, par, ju, jd, w, TAU["hb"], (sysm.nup, sysm.ndn), False, time_sym,
                                    table_prob=TU.heatbath_table_prob(H, hb, par, time_sym))
            TU._assert_clean("gpu heatbath%s/%s" % ("_ts" if time_sym else "", name), fails, rep)
            if name == "hf":
                assert int(np.count_nonzero((w[:, 0] != 0) & (w[:, 1] != 0))) > 1000
    finally:
        g.close(); hb.close()


STEP_CASES = {"c2_walk": ("c2_setup", "open_double"), "c2_hci": ("c2_setup_ts", "open_single"), "heg14": ("heg_setup", "off_fermi_sphere"),
              "heg57": ("heg57_setup", "off_fermi_sphere"), "hub44": ("hub_setup", "three_hops"), "heatbath": (None, "open_double"),
              "heatbath_ts": (None, "open_single")}
STEP_W = 262144.25          # lround gives 2^18 children of weight W / 2^18 each
STEP_R = 64


@pytest.mark.parametrize("case", sorted(STEP_CASES))
def test_one_counter_step_applies_the_projector_row(request, oracle, case):
    """One sqmc_gpu_step in RNG_COUNTER mode (the benchmark's mode: the spawn kernel's own stream and child count) from one
    determinant of weight W, semistochastic off, every child an initiator's child (the parent is an initiator, r_initiator = 0,
    initiator_power = 0: nothing is discarded), E_T two hartree above H_ii so that the diagonal factor is not 1 and cannot go
    negative (the clamp of a negative factor, do_walk.f90's f < 0 branch, is the one rule of the step that is not mean-preserving
    and stays out of reach), reweight_factor_inv = 0.93, min_wt = always_spawn_cutoff_wt = 0.5 (join_walker2 runs).  Over 64 seeds
    the mean weight on every determinant over W is the projector row within 5 standard errors of the spread over the repeats,
    and out[15] is lround(|W|): one proposal per unit weight."""
    import sqmc_amd
    setup_name, parent_name = STEP_CASES[case]
    hb = None
    if case.startswith("heatbath"):
        ts = case.endswith("_ts")
        sysm = request.getfixturevalue("c2_10e_ts" if ts else "c2_10e")
        setup = oracle.setup_walk(sysm, 100, 1000, 0.1)
        hb = oracle.HeatBath(sysm)
        H = TU.chem_checker(sysm)
        parents, children, which, kind = PC.parents_chem(H, (sysm.hf_up, sysm.hf_dn), H.norb, ts), (lambda p: PC.excitations_chem(p[0], p[1], H.norb)), "c2", "hb"
    else:
        which = case
        sysm, setup = request.getfixturevalue(which), request.getfixturevalue(setup_name)
        H, parents, children, ts = TU.uniform_case(sysm, which)
        kind = TU.UNIFORM[which][0]
    par = dict(parents)[parent_name]
    rowd = PC.row(H, par, children(par), ts)
    h_ii = (H.element_ts(*par, *par) if ts else H.element(*par, *par))[0]
    tau, rfi = TAU[kind], 0.93
    e_trial = h_ii + 2.0
    expected = PC.projector_row(rowd, h_ii, tau, e_trial, rfi)
    prm = dict(tau=tau, e_trial=e_trial, reweight_factor_inv=rfi, r_initiator=0.0, min_wt=0.5, always_spawn_cutoff_wt=0.5,
               initiator_power=0, initiator_min_distance=0, c_t_initiator=0, semistochastic=0, reached_w_abs_gen=0)
    wk = dict(up=np.array([par[0]], np.uint64), dn=np.array([par[1]], np.uint64), wt=np.array([STEP_W]), imp_distance=np.ones(1, np.int8),
              initiator=np.full(1, 2, np.int8), perm_sign=np.zeros(1, np.int8), matrix_elements=np.full(1, 1e51), e_num=np.full(1, 1e51),
              e_den=np.full(1, 1e51))
    g = _ctx(sysm, which, rng_mode=sqmc_amd.RNG_COUNTER, mwalk=1 << 20)
    repeats = []
    try:
        if hb is not None:
            g.set_heatbath_tables(hb.fortran_arrays())
        g.set_ct_table(setup.ct_up, setup.ct_dn, setup.ct_num, setup.ct_den)
        seeds = PC.state_limbs(PC.splitmix_states(STEP_R))
        for r in range(STEP_R):
            g.set_rng([int(x) for x in seeds[r]])
            g.upload_walkers(wk)
            out = g.step(prm)
            assert out[15] == round(abs(STEP_W)), (r, out[15])
            got = g.download_walkers()
            repeats.append({(int(a), int(b)): float(x) / STEP_W for a, b, x in zip(got["up"], got["dn"], got["wt"]) if x != 0.0})
    finally:
        g.close()
        if hb is not None:
            hb.close()
    assert len({tuple(sorted(r.items())) for r in repeats}) == STEP_R          # the seeds gave different steps
    fails, rep = PC.analyse_step_repeats(expected, par, repeats, quantum=0.5 * rfi / STEP_W)
    print(PC.step_summary("gpu step %-12s" % case, par, rep))
    assert not fails, fails[:10]
    assert rep["tested"] > 20
