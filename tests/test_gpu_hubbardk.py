"""The plane-wave Hubbard operator (sys_type 3, 'hubbardk') on the GPU against tests/hubbardk_checker.py: matrix elements, the
proposal door, one RNG_COUNTER step, the connection generator, the sparse matrix, PT2, a walk with nothing stochastic in it
against exact diagonalisation, a stochastic walk's invariants, two ranks over gloo and the deck runner.  Tolerances and statistics
are those of tests/proposal_checker.py.  Every context comes from HubbardKHost.gpu()."""
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import proposal_checker as PC          # noqa: E402
from tests import hubbardk_checker as HK          # noqa: E402

pytestmark = pytest.mark.gpu
T_HOP, U = 1.0, 4.0
TAU = 0.01
N_GPU = 1 << 22
SEED = (1346, 5634, 6635, 4361)
DECK = os.path.join(ROOT, "tests", "golden", "hubbardk4x3_i_walk")


def _host(l_x, l_y, nup, ndn):
    import sqmc_amd
    from sqmc_amd.host import HubbardKHost
    sqmc_amd.set_device(0)
    return HubbardKHost(l_x, l_y, nup, ndn, T_HOP, U)


def _checker(l_x, l_y):
    return HK.HubbardKH(l_x, l_y, T_HOP, U)


def _compare(H, pairs, got):
    """|H_gpu - H_ref| <= 4 n_terms 2^-53 sum|terms| on every pair, exact zeros exact; returns (worst ratio, pairs with terms)"""
    worst, nonzero = 0.0, 0
    for (iu, id_, ju, jd), g in zip(pairs, got):
        ref, n, sa = H.element(iu, id_, ju, jd)
        if n == 0:
            assert g == 0.0, ((iu, id_, ju, jd), g)
            continue
        nonzero += 1
        b = PC.rounding_bound(n, sa)
        assert abs(g - ref) <= b, ((iu, id_, ju, jd), g, ref, b)
        if ref != 0.0:
            assert math.copysign(1.0, g) == math.copysign(1.0, ref)
        worst = max(worst, abs(g - ref) / b)
    return worst, nonzero


def _batch(g, pairs):
    a = np.array(pairs, dtype=np.uint64)
    return g.hamiltonian_batch(a[:, 0], a[:, 1], a[:, 2], a[:, 3]).tolist()


# ------------------------------------------------------------------------------------------------ 1. elements
def test_elements_4x3_all_pairs_of_a_sample():
    H, hst = _checker(4, 3), _host(4, 3, 2, 2)
    dets = random.Random(3).sample(HK.all_determinants(12, 2, 2), 300)
    pairs = [a + b for a in dets for b in dets]
    g = hst.gpu()
    try:
        got = _batch(g, pairs)
    finally:
        g.close()
    worst, nonzero = _compare(H, pairs, got)
    print("4x3 (2,2): %d pairs, %d with terms, worst |dH| / bound = %.3g" % (len(pairs), nonzero, worst))
    assert nonzero > 300 and sum(1 for x in got if x == 0.0) > len(pairs) // 2


def test_elements_4x4_row_of_the_start_determinant_and_random_pairs():
    H, hst = _checker(4, 4), _host(4, 4, 5, 5)
    par = (hst.hf_up, hst.hf_dn)
    kids = HK.excitations_hubbardk(H, *par)
    rng = random.Random(5)
    strings = lambda n: sum(1 << o for o in rng.sample(range(16), n))
    pairs = [par + par] + [par + c for c in kids] + [c + par for c in kids[:50]]
    for _ in range(1200):
        a = (strings(5), strings(5))
        kind = rng.randrange(3)
        b = a if kind == 0 else rng.choice(HK.excitations_hubbardk(H, *a)) if kind == 1 else (strings(5), strings(5))
        pairs.append(a + b)
    g = hst.gpu()
    try:
        got = _batch(g, pairs)
    finally:
        g.close()
    worst, nonzero = _compare(H, pairs, got)
    print("4x4 (5,5): %d pairs (%d children of the start determinant), %d with terms, worst |dH| / bound = %.3g" % (len(pairs), len(kids), nonzero, worst))
    assert len(kids) > 100 and nonzero > len(kids) + 400


def test_elements_8x8_moves_that_span_the_word():
    """an electron between orbital 1 and orbital 64 (bits 0 and 63) with the string's other electrons in between, in either
    string and in either direction: bit 63 and a parity string that spans the word"""
    H, hst = _checker(8, 8), _host(8, 8, 3, 3)
    pairs = []
    for lo_side in (True, False):
        a, b = (0, 63) if lo_side else (63, 0)
        for mid_u, mid_d in (((20, 41), (30, 50)), ((1, 62), (2, 61)), ((31, 32), (5, 58))):
            up = (1 << a) | (1 << mid_u[0]) | (1 << mid_u[1])
            dn = (1 << a) | (1 << mid_d[0]) | (1 << mid_d[1])
            for c in HK.excitations_hubbardk(H, up, dn):
                moved_up = (c[0] >> b & 1) and not (c[0] >> a & 1)
                moved_dn = (c[1] >> b & 1) and not (c[1] >> a & 1)
                if moved_up or moved_dn:
                    pairs += [(up, dn) + c, c + (up, dn)]
    g = hst.gpu()
    try:
        got = _batch(g, pairs)
    finally:
        g.close()
    worst, nonzero = _compare(H, pairs, got)
    signs = {math.copysign(1.0, x) for x in got}
    print("8x8 (3,3): %d pairs across bits 0 and 63, worst |dH| / bound = %.3g, signs %s" % (len(pairs), worst, sorted(signs)))
    assert nonzero == len(pairs) >= 40 and signs == {1.0, -1.0}


# ------------------------------------------------------------------------------------------------ 2. the proposal door
DOOR_PARENTS = [("4x4_start", (4, 4, 5, 5), None), ("4x4_moving", (4, 4, 5, 5), (0b1000001111, 0b10011011)), ("4x3", (4, 3, 2, 2), (0b100100, 0b1000010)),
                ("8x8_ends", (8, 8, 3, 3), ((1 << 63) | (1 << 20) | 1, (1 << 63) | (1 << 33) | 1))]
LCG_M3 = pow(11 ** 13, 3, 1 << 48)


@pytest.mark.parametrize("name,shape,par", DOOR_PARENTS, ids=[p[0] for p in DOOR_PARENTS])
def test_proposal_door_is_unbiased(name, shape, par):
    """2^22 proposals, one hashed rannyu state each: the five checks of proposal_checker.analyse against the exact row, the share of
    blocked (zero-weight) proposals against the blocked triples, and three draws consumed by accepted and blocked proposals alike"""
    l_x, l_y, nup, ndn = shape
    H, hst = _checker(l_x, l_y), _host(*shape)
    par = par or (hst.hf_up, hst.hf_dn)
    assert (PC._pop(par[0]), PC._pop(par[1])) == (nup, ndn)
    if name == "4x4_moving":
        assert H.momentum(*par) != (0, 0)
    tr = HK.triples_hubbardk(H, *par)
    blocked = sum(1 for x in tr if x[4] is None) / len(tr)
    rowd = PC.row(H, par, HK.excitations_hubbardk(H, *par))
    st = PC.splitmix_states(N_GPU)
    g = hst.gpu()
    try:
        ju, jd, w, after = g.propose_batch(TAU, np.full(N_GPU, par[0], np.uint64), np.full(N_GPU, par[1], np.uint64), PC.state_limbs(st))
    finally:
        g.close()
    fails, rep = PC.analyse(rowd, par, ju, jd, w, TAU, (nup, ndn), weight_by_child=True)
    print(PC.summary("gpu hubbardk/%s" % name, rep))
    assert not fails, fails
    seen = float(np.count_nonzero(w == 0.0)) / N_GPU
    sd = math.sqrt(blocked * (1.0 - blocked) / N_GPU)
    print("    blocked: %.6f seen, %.6f of the %d triples, %.2f sd" % (seen, blocked, len(tr), (seen - blocked) / sd if sd else 0.0))
    assert abs(seen - blocked) <= 5.0 * sd
    exp = (st.astype(np.uint64) * np.uint64(LCG_M3)) & np.uint64((1 << 48) - 1)      # uint64 products wrap modulo 2^64: exact modulo 2^48
    assert int(exp[0]) == (int(st[0]) * LCG_M3) % (1 << 48)
    assert np.array_equal(after.astype(np.int64), PC.state_limbs(exp).astype(np.int64))


# ------------------------------------------------------------------------------------------------ 3. one real step
STEP_W, STEP_R = 262144.25, 64


def test_one_counter_step_applies_the_projector_row():
    """the parameters of test_gpu_proposal_unbiased.test_one_counter_step_applies_the_projector_row on the 4x4 (5,5) start determinant"""
    import sqmc_amd
    H, hst = _checker(4, 4), _host(4, 4, 5, 5)
    par = (hst.hf_up, hst.hf_dn)
    rowd = PC.row(H, par, HK.excitations_hubbardk(H, *par))
    h_ii = H.element(*par, *par)[0]
    rfi, e_trial = 0.93, h_ii + 2.0
    expected = PC.projector_row(rowd, h_ii, TAU, e_trial, rfi)
    prm = dict(tau=TAU, e_trial=e_trial, reweight_factor_inv=rfi, r_initiator=0.0, min_wt=0.5, always_spawn_cutoff_wt=0.5,
               initiator_power=0, initiator_min_distance=0, c_t_initiator=0, semistochastic=0, reached_w_abs_gen=0)
    wk = dict(up=np.array([par[0]], np.uint64), dn=np.array([par[1]], np.uint64), wt=np.array([STEP_W]), imp_distance=np.ones(1, np.int8),
              initiator=np.full(1, 2, np.int8), perm_sign=np.zeros(1, np.int8), matrix_elements=np.full(1, 1e51), e_num=np.full(1, 1e51),
              e_den=np.full(1, 1e51))
    g = hst.gpu(rng_mode=sqmc_amd.RNG_COUNTER, mwalk=1 << 20)
    repeats = []
    try:
        setup = hst.setup_walk(g, 20, 30, 0.5)
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
    assert len({tuple(sorted(r.items())) for r in repeats}) == STEP_R
    fails, rep = PC.analyse_step_repeats(expected, par, repeats, quantum=0.5 * rfi / STEP_W)
    print(PC.step_summary("gpu step hubbardk", par, rep))
    assert not fails, fails[:10]
    assert rep["tested"] > 20


# ------------------------------------------------------------------------------------------------ 4. connections
@pytest.fixture(scope="module")
def conn_case():
    """40 reference determinants of 4x3 (2,2); |H| = U / 12 throughout, so |H c| > eps cuts on |c|: coefficients on both sides of
    the cut, one zero (emits nothing, its own slot included) and one exact tie (|H c| == eps: dropped)"""
    H = _checker(4, 3)
    rng = random.Random(17)
    refs = rng.sample(HK.all_determinants(12, 2, 2), 40)
    c_tie = 0.03
    eps = abs(H.ubyn * c_tie)
    coeffs = [rng.choice((-1, 1)) * 10.0 ** rng.uniform(-2.5, -0.5) for _ in refs]
    coeffs[7], coeffs[19] = 0.0, -c_tie
    assert sum(1 for c in coeffs if abs(H.ubyn * c) > eps) > 8 and sum(1 for c in coeffs if c != 0.0 and not abs(H.ubyn * c) > eps) > 8
    return H, refs, coeffs, eps


@pytest.mark.parametrize("diag_mode", [0, 1, 2])
def test_connections_against_brute_force(conn_case, diag_mode):
    H, refs, coeffs, eps = conn_case
    hst = _host(4, 3, 2, 2)
    ru, rd = np.array([r[0] for r in refs], np.uint64), np.array([r[1] for r in refs], np.uint64)
    g = hst.gpu()
    try:
        cu, cd, num, den = g.hci_connections(ru, rd, coeffs, eps, diag_mode=diag_mode)
        slices = [g.hci_connections(ru, rd, coeffs, eps, diag_mode=diag_mode, slice=s, n_slices=3) for s in range(3)] if diag_mode != 2 else []
    finally:
        g.close()
    want = HK.connections(H, refs, coeffs, eps, diag_mode)
    got_keys = list(zip(cu.tolist(), cd.tolist()))
    if diag_mode == 2:                            # the unmerged list in generation order, e_mix_den = the source's index
        assert got_keys == [w[0] for w in want]
        for (k, wn, wi), gn, gi in zip(want, num.tolist(), den.tolist()):
            assert abs(gn - wn) <= PC.rounding_bound(1, abs(wn)) and gi == wi, (k, gn, wn, gi, wi)
        assert refs[7] not in [w[0] for w in want if w[2] == 7.0] and not any(w[2] == 7.0 for w in want)
        assert sum(1 for w in want if w[2] == 19.0) == 1          # the tie keeps its own slot and nothing else
        return
    assert got_keys == sorted(want)
    worst = 0.0
    for k, gn, gd in zip(got_keys, num.tolist(), den.tolist()):
        wn, wd, n, sa = want[k]
        b = PC.rounding_bound(n, sa)
        assert abs(gn - wn) <= b and gd == wd, (k, gn, wn, gd, wd)
        worst = max(worst, abs(gn - wn) / b if b else 0.0)
    print("diag_mode %d: %d connections of %d reference determinants, worst |d num| / bound = %.3g" % (diag_mode, len(got_keys), len(refs), worst))
    union = {}
    for su, sd, sn, se in slices:
        for k, a, b in zip(zip(su.tolist(), sd.tolist()), sn.tolist(), se.tolist()):
            assert k not in union
            union[k] = (a, b)
    assert union == {k: (a, b) for k, a, b in zip(got_keys, num.tolist(), den.tolist())}
    assert sum(1 for s in slices if len(s[0])) >= 2


def test_unsupported_doors_are_refused():
    import sqmc_amd
    from sqmc_amd._lib import GpuChem, Pt2StochasticPlan
    UNSUPPORTED, BAD_ARG = -3, -1                 # SQMC_ERR_UNSUPPORTED, SQMC_ERR_BAD_ARG of include/sqmc_gpu.h
    hst = _host(4, 3, 2, 2)
    one, two = np.ones(1, np.int64), np.ones(1)
    g = hst.gpu()
    try:
        doors = {"diag-update mode": lambda: g.hci_set_diag_update(1),
                 "active-space masks": lambda: g.hci_set_active_space(1, 1, 0, 0, 1),
                 "diag-update record": lambda: g.hci_connections_record([hst.hf_up], [hst.hf_dn], [1.0], 1e-9),
                 "diag-update batch": lambda: g.diag_update_batch([0.0], [[1, 13, 2, 14]], [hst.hf_up], [hst.hf_dn]),
                 "stochastic-PT plan": lambda: Pt2StochasticPlan(g, [hst.hf_up], [hst.hf_dn], [1.0], -1.0, 1e-9, 1e-3, 10),
                 "hf_to_psit": lambda: g.set_hf_to_psit(one, two, two),
                 "hf_to_psit, sharded": lambda: g.set_hf_to_psit_shard(one, two, one, one, two)}
        for name, call in doors.items():
            with pytest.raises(sqmc_amd.SqmcGpuError) as ei:
                call()
            assert ei.value.code == UNSUPPORTED, (name, str(ei.value))
    finally:
        g.close()
    kv, ke = hst.k_vectors, hst.k_energies
    for bad, code in ((dict(l_x=2, l_y=3), UNSUPPORTED), (dict(l_x=4, l_y=2), UNSUPPORTED), (dict(l_x=13, l_y=5), UNSUPPORTED), (dict(l_x=1, l_y=1), BAD_ARG),
                      (dict(nup=0), BAD_ARG), (dict(nup=12), BAD_ARG), (dict(ndn=0), BAD_ARG), (dict(ndn=12), BAD_ARG)):
        a = dict(l_x=4, l_y=3, nup=2, ndn=2); a.update(bad)
        n = a["l_x"] * a["l_y"]
        with pytest.raises(sqmc_amd.SqmcGpuError) as ei:
            GpuChem.hubbardk(a["l_x"], a["l_y"], a["nup"], a["ndn"], T_HOP, U, np.resize(kv, (n, 2)), np.resize(ke, n))
        assert ei.value.code == code, (bad, str(ei.value))
    twice = kv.copy(); twice[5] = twice[4]        # a momentum twice, another one missing
    odd = kv.copy(); odd[3, 0] += 1               # not a momentum of the periodic lattice
    for table in (twice, odd):
        with pytest.raises(sqmc_amd.SqmcGpuError) as ei:
            GpuChem.hubbardk(4, 3, 2, 2, T_HOP, U, table, ke)
        assert ei.value.code == BAD_ARG, str(ei.value)
    from sqmc_amd.host import HubbardKHost
    with pytest.raises(ValueError):
        HubbardKHost(4, 3, 2, 2, 1.0, 0.0)        # no element to screen on: refused, not an empty set-up
    g = _host(6, 1, 2, 2).gpu()                   # a chain is supported
    g.close()


# ------------------------------------------------------------------------------------------------ 5. the sparse matrix
@pytest.fixture(scope="module")
def sector33():
    H = _checker(3, 3)
    dets = HK.sector(H, 2, 2, H.momentum(3, 3))
    A = HK.dense(H, dets, lambda u, d: HK.excitations_hubbardk(H, u, d))
    return H, dets, A


def test_build_sparse_ham_is_the_dense_matrix(sector33):
    H, dets, A = sector33
    assert len(dets) == 144
    hst = _host(3, 3, 2, 2)
    g = hst.gpu()
    try:
        cnt, idx, val = g.build_sparse_ham([d[0] for d in dets], [d[1] for d in dets])
    finally:
        g.close()
    n = len(dets)
    rows = np.repeat(np.arange(n), cnt)
    seen = {}
    for r, c, v in zip(rows.tolist(), (idx - 1).tolist(), val.tolist()):
        k = (min(r, c), max(r, c))
        assert k not in seen, k
        seen[k] = v
        if r != c:
            assert v != 0.0                        # zero elements are absent
    want = {(i, j) for i in range(n) for j in range(i, n) if i == j or A[i, j] != 0.0}
    assert set(seen) == want
    for (i, j), v in seen.items():
        ref, nt, sa = H.element(dets[j][0], dets[j][1], dets[i][0], dets[i][1])
        assert abs(v - ref) <= PC.rounding_bound(nt, sa), ((i, j), v, ref)
    print("3x3 (2,2) sector: %d determinants, %d stored elements" % (n, len(seen)))


# ------------------------------------------------------------------------------------------------ 6. PT2
def test_hci_pt2_against_the_explicit_sum():
    """variational space: the start determinant and its first-order space, its lowest eigenvector from the checker's dense matrix;
    delta_E = sum over outside determinants a of (sum_i H_ai c_i)^2 / (E_var - H_aa).  Relative tolerance 4 n_terms 2^-53 sum|terms| / |sum|,
    terms: the outside determinants' contributions, n_terms: the products H_ai c_i that enter them."""
    H, hst = _checker(3, 3), _host(3, 3, 2, 2)
    eps_pt = 1e-12
    g = hst.gpu()
    try:
        vu, vd = hst.first_order_space(1, g)
        var = list(zip(vu.tolist(), vd.tolist()))
        A = HK.dense(H, var, lambda u, d: HK.excitations_hubbardk(H, u, d))
        w, X = np.linalg.eigh(A)
        e_var, c = float(w[0]), X[:, 0]
        got, n_conn = g.hci_pt2(vu, vd, c, e_var, eps_pt)
    finally:
        g.close()
    inside, sums = set(var), {}
    for (u, d), ci in zip(var, c.tolist()):
        for a in HK.excitations_hubbardk(H, u, d):
            if a in inside:
                continue
            x = H.element(u, d, a[0], a[1])[0] * ci
            assert abs(x) > 10 * eps_pt or x == 0.0
            if abs(x) > eps_pt:
                sums.setdefault(a, []).append(x)
    terms = [math.fsum(xs) ** 2 / (e_var - H.element(a[0], a[1], a[0], a[1])[0]) for a, xs in sums.items()]
    want = math.fsum(terms)
    n_terms = sum(len(xs) for xs in sums.values())
    tol = 4.0 * n_terms * 2.0 ** -53 * math.fsum(abs(x) for x in terms) / abs(want)
    print("3x3 (2,2): %d variational, %d outside determinants, delta_E = %.15g (device %.15g), relative difference %.3g, tolerance %.3g"
          % (len(var), len(sums), want, got, abs(got - want) / abs(want), tol))
    assert 1 < len(var) < 144 and len(sums) > 10 and want < 0
    assert abs(got - want) <= tol * abs(want)


# ------------------------------------------------------------------------------------------------ 7. a deterministic walk
class _Levels:
    """the host with setup_walk's n_levels fixed (GpuWalk calls setup_walk with its own four arguments)"""

    def __init__(self, hst, n_levels):
        self._h, self._n = hst, n_levels

    def __getattr__(self, name):
        return getattr(self._h, name)

    def setup_walk(self, g, n_truncate_trial_wf, size_deterministic, tau_multiplier):
        return self._h.setup_walk(g, n_truncate_trial_wf, size_deterministic, tau_multiplier, n_levels=self._n)


@pytest.mark.parametrize("l_x,l_y,dim", [(3, 3, 144), (4, 3, 366)])
def test_walk_with_nothing_stochastic_finds_the_sector_ground_state(l_x, l_y, dim):
    """the whole momentum sector as the deterministic space: the walk is power iteration, and its projected energy converges to
    the sector's ground state.  |E - E0| <= 1e-10: rounding of dim 2^-53 range / overlap is about 1e-12, times 100."""
    from sqmc_amd import host as Hh
    H, hst = _checker(l_x, l_y), _host(l_x, l_y, 2, 2)
    dets = HK.sector(H, 2, 2, H.momentum(hst.hf_up, hst.hf_dn))
    assert len(dets) == dim
    e0 = float(np.linalg.eigvalsh(HK.dense(H, dets, lambda u, d: HK.excitations_hubbardk(H, u, d)))[0])
    w = Hh.GpuWalk(_Levels(hst, 8), 1.0e4, w_begin=1.0e4, n_truncate_trial_wf=20, size_deterministic=10 * dim, tau_multiplier=0.5, seed=SEED)
    try:
        assert len(w.setup.imp_up) == dim and sorted(zip(w.setup.imp_up.tolist(), w.setup.imp_dn.tolist())) == dets
        prev, steps, e = None, 0, 0.0
        while steps < 8000:
            out = w.step(); steps += 1
            e = out[3] / out[2]
            if prev is not None and abs(e - prev) < 1e-13:
                break
            prev = e
    finally:
        w.close()
    print("%dx%d (2,2): sector of %d, E0 = %.15f, walk %.15f after %d steps, error %.3g" % (l_x, l_y, dim, e0, e, steps, abs(e - e0)))
    assert steps < 8000
    assert abs(e - e0) <= 1e-10


# ------------------------------------------------------------------------------------------------ 8. a stochastic walk
def test_stochastic_walk_invariants_and_energy_bracket():
    from sqmc_amd import host as Hh
    H, hst = _checker(4, 3), _host(4, 3, 2, 2)
    dets = HK.sector(H, 2, 2, H.momentum(hst.hf_up, hst.hf_dn))
    e0 = float(np.linalg.eigvalsh(HK.dense(H, dets, lambda u, d: HK.excitations_hubbardk(H, u, d)))[0])
    h_start = H.element(hst.hf_up, hst.hf_dn, hst.hf_up, hst.hf_dn)[0]
    w = Hh.GpuWalk(hst, 2.0e4, w_begin=2000.0, n_truncate_trial_wf=20, size_deterministic=30, tau_multiplier=0.5, seed=SEED)
    try:
        for _ in range(200):
            w.step()
        outs = np.array([w.step().copy() for _ in range(400)])
        wk = w.g.download_walkers()
    finally:
        w.close()
    keys = list(zip(wk["up"].tolist(), wk["dn"].tolist()))
    assert keys == sorted(set(keys))
    assert int(outs[-1][5]) == len(keys)
    assert np.isclose(float(np.abs(wk["wt"]).sum()), outs[-1][1], rtol=1e-12)
    assert set(keys) <= set(dets)
    e = outs[:, 3].sum() / outs[:, 2].sum()
    blocks = [outs[k:k + 40, 3].sum() / outs[k:k + 40, 2].sum() for k in range(0, 400, 40)]
    se = float(np.std(blocks, ddof=1) / math.sqrt(len(blocks)))
    print("4x3 (2,2) stochastic walk: E = %.6f, E0 = %.6f, deviation %.3g, blocked standard error %.3g, %d walkers" % (e, e0, e - e0, se, len(keys)))
    assert e0 - 0.5 < e < h_start


# ------------------------------------------------------------------------------------------------ 9. two ranks
def _shard_worker(rank, world, port, outdir):
    import torch                                   # noqa: F401  before the HIP library (one libamdhip64 per process)
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    hst = H.HubbardKHost(4, 4, 5, 5, T_HOP, U)
    w = H.ShardedWalk(hst, 20000, rank, world, w_begin=2000, seed=SEED, mwalk=400000, n_truncate_trial_wf=20, size_deterministic=100, tau_multiplier=0.5)
    outs = [w.step().copy() for _ in range(40)]
    wk = w.g.download_walkers()
    owner = w.g.det_owner(wk["up"], wk["dn"], world)
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), outs=np.array(outs), owner=owner, n_imp_global=w.n_imp_global, **wk)
    w.close()
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_walk_invariants(tmp_path):
    """the invariants of test_gpu_sharded.test_sharded_hubbard_walk_invariants for the plane-wave operator"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    import socket
    with socket.socket() as sk:                   # a port that is free now, not a fixed one another run may hold
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ps = [ctx.Process(target=_shard_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in ps: p.start()
    for p in ps: p.join(600)
    assert all(p.exitcode == 0 for p in ps), [p.exitcode for p in ps]
    res = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(2)]
    assert np.array_equal(res[1]["outs"][:, :7], res[0]["outs"][:, :7])
    keys, n_imp = [], 0
    for rank, r in enumerate(res):
        assert np.all(r["owner"] == rank)
        k = [(int(a), int(b)) for a, b in zip(r["up"], r["dn"])]
        assert k == sorted(set(k))
        keys += k
        n_imp += int((r["imp_distance"] == 0).sum())
    assert len(keys) == len(set(keys)) and n_imp == int(res[0]["n_imp_global"])
    out = res[0]["outs"][-1]
    assert int(out[5]) == len(keys)
    assert np.isclose(sum(float(np.abs(r["wt"]).sum()) for r in res), out[1], rtol=1e-12)
    assert all(len(r["up"]) > 0 for r in res) and out[1] > 1.5 * 2000


# ------------------------------------------------------------------------------------------------ 10. the deck
def test_deck_runs_end_to_end():
    r = subprocess.run([sys.executable, "-m", "sqmc_amd.run", "-i", DECK], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "iblk, w_perm_initiator, nwalk, w_abs, w_abs_imp=" in r.stdout and "Energy=" in r.stdout and "uniform2" in r.stdout
