"""The real-space Hubbard connection generator (the sys_type 2 branch of k_hci_gen, find_connected_dets_hubbard) on the GPU against
tests/hubbard_gen_checker.py: connections in all three modes with slices, hops at the ends of the 64-bit word, a chain and half
filling, the first-order space and its lowest state, PT2, the walk set-up against the kept host construction bit for bit, the
variational stage, and the doors that stay refused.  Every context comes from HubbardHost.gpu()."""
import itertools
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import proposal_checker as PC          # noqa: E402
from tests import hubbard_gen_checker as HG       # noqa: E402

pytestmark = pytest.mark.gpu
T_HOP, U = 0.75, 3.0


def _host(l_x, l_y, pbc, nup, ndn, t=T_HOP, u=U):
    import sqmc_amd
    from sqmc_amd.host import HubbardHost
    sqmc_amd.set_device(0)
    return HubbardHost(l_x, l_y, pbc, nup, ndn, t, u)


def _arrays(dets):
    return np.array([d[0] for d in dets], np.uint64), np.array([d[1] for d in dets], np.uint64)


def _check_modes(H, g, refs, coeffs, eps, slices=False):
    """the generator's three modes on (refs, coeffs, eps) against HG.connections; returns the raw model list"""
    ru, rd = _arrays(refs)
    raw = None
    for diag_mode in (2, 0, 1):
        cu, cd, num, den = g.hci_connections(ru, rd, coeffs, eps, diag_mode=diag_mode)
        want = HG.connections(H, refs, coeffs, eps, diag_mode)
        got_keys = list(zip(cu.tolist(), cd.tolist()))
        if diag_mode == 2:                        # the unmerged list in generation order, e_mix_den = the source's index
            raw = want
            assert got_keys == [w[0] for w in want]
            for (k, wn, wi), gn, gi in zip(want, num.tolist(), den.tolist()):
                assert abs(gn - wn) <= PC.rounding_bound(1, abs(wn)) and gi == wi, (k, gn, wn, gi, wi)
            continue
        assert got_keys == sorted(want)
        worst = 0.0
        for k, gn, gd in zip(got_keys, num.tolist(), den.tolist()):
            wn, wd, n, sa = want[k]
            b = PC.rounding_bound(n, sa)
            assert abs(gn - wn) <= b and gd == wd, (diag_mode, k, gn, wn, gd, wd)
            worst = max(worst, abs(gn - wn) / b if b else 0.0)
        print("diag_mode %d: %d connections of %d reference determinants, worst |d num| / bound = %.3g" % (diag_mode, len(got_keys), len(refs), worst))
        if slices:
            parts = [g.hci_connections(ru, rd, coeffs, eps, diag_mode=diag_mode, slice=s, n_slices=3) for s in range(3)]
            union = {}
            for su, sd, sn, se in parts:
                for k, a, b in zip(zip(su.tolist(), sd.tolist()), sn.tolist(), se.tolist()):
                    assert k not in union
                    union[k] = (a, b)
            assert union == {k: (a, b) for k, a, b in zip(got_keys, num.tolist(), den.tolist())}
            assert sum(1 for s in parts if len(s[0])) >= 2
    return raw


# ------------------------------------------------------------------------------------------------ 1. connections
@pytest.mark.parametrize("l_x,l_y,pbc,seed", [(4, 3, False, 17), (3, 3, True, 18)], ids=["4x3_open", "3x3_periodic"])
def test_connections_against_brute_force(l_x, l_y, pbc, seed):
    H, refs, coeffs, eps = HG.conn_case(l_x, l_y, pbc, T_HOP, U, seed)
    g = _host(l_x, l_y, pbc, 2, 2).gpu()
    try:
        raw = _check_modes(H, g, refs, coeffs, eps, slices=True)
        raw_sl = [g.hci_connections(*_arrays(refs), coeffs, eps, diag_mode=2, slice=s, n_slices=3) for s in range(3)]
    finally:
        g.close()
    assert not any(w[2] == 7.0 for w in raw)                                  # c = 0 emits nothing, its own slot included
    assert [w[0] for w in raw if w[2] == 19.0] == [refs[19]]                  # the tie keeps its own slot and nothing else
    # raw slices: every entry of the unsliced raw list in exactly one slice, each slice in generation order
    got = [sorted(zip(zip(s[0].tolist(), s[1].tolist()), s[2].tolist(), s[3].tolist())) for s in raw_sl]
    assert sorted(itertools.chain(*got)) == sorted(raw) and sum(1 for s in got if s) >= 2
    for s in raw_sl:
        order = [(k, i) for k, i in zip(zip(s[0].tolist(), s[1].tolist()), s[3].tolist())]
        assert order == [(w[0], w[2]) for w in raw if (w[0], w[2]) in set(order)]
    if not pbc:
        assert any(len(HG.hops(H, u, d)) < 16 for u, d in refs)               # edges: disallowed neighbours


def test_t_zero_emits_only_the_own_slot():
    H = HG.Lattice(3, 3, True, 0.0, U)
    refs = [(0b11, 0b101), (0b110, 0b11)]
    g = _host(3, 3, True, 2, 2, 0.0, U).gpu()
    try:
        raw = _check_modes(H, g, refs, [0.5, -0.25], 1e-300)
    finally:
        g.close()
    assert [w[0] for w in raw] == refs


# ------------------------------------------------------------------------------------------------ 2. the ends of the word
def test_hops_at_the_ends_of_the_word_8x8():
    """8x8 periodic (2,2), electrons on sites 1, 8, 57 and 64 (bits 0, 7, 56, 63): LEFT of site 1 is site 8, DOWN of it site 57, RIGHT of
    site 64 is site 57, UP of it site 8 -- hops wrap in both directions, set and clear bit 63, and their parity strings span the word"""
    H, hst = HG.Lattice(8, 8, True, T_HOP, U), _host(8, 8, True, 2, 2)
    corner = [0, 7, 56, 63]
    pairs = [(1 << a) | (1 << b) for a, b in itertools.combinations(corner, 2)]
    refs = [(u, d) for u in pairs for d in pairs]
    g = hst.gpu()
    try:
        raw = _check_modes(H, g, refs, [1.0] * len(refs), 1e-300)
        cu, cd, num, src = g.hci_connections(*_arrays(refs), np.ones(len(refs)), 1e-300, diag_mode=2)
        su, sd = _arrays([refs[int(i)] for i in src])
        hb = g.hamiltonian_batch(cu, cd, su, sd)
        hb_t = g.hamiltonian_batch(su, sd, cu, cd)
    finally:
        g.close()
    own = (cu == su) & (cd == sd)
    assert np.array_equal(num[~own], hb[~own]) and np.array_equal(num[~own], hb_t[~own])        # bit for bit
    assert np.all(num[own] == 0.0) and int(own.sum()) == len(refs)
    model = np.array([H.element(int(a), int(b), int(c), int(d))[0] for a, b, c, d in zip(su[~own], sd[~own], cu[~own], cd[~own])])
    assert np.array_equal(num[~own], model) and set(np.abs(model).tolist()) == {T_HOP}
    top = np.uint64(1 << 63)
    sets63 = ((cu & ~su) | (cd & ~sd)) & top != 0
    clears63 = ((su & ~cu) | (sd & ~cd)) & top != 0
    print("8x8: %d sources, %d hops, %d set bit 63, %d clear it, signs %s" % (len(refs), int((~own).sum()), int(sets63.sum()), int(clears63.sum()), sorted(set(np.sign(model).tolist()))))
    assert sets63.sum() > 4 and clears63.sum() > 4 and set(np.sign(model).tolist()) == {1.0, -1.0}
    # wraps in both directions: bit 0 -> bit 7 (LEFT) and bit 0 -> bit 56 (DOWN); bit 63 -> bit 56 (RIGHT) and bit 63 -> bit 7 (UP)
    moves = {(int(a ^ b) if a != b else int(c ^ d)) for a, b, c, d in zip(su[~own], cu[~own], sd[~own], cd[~own])}
    assert {(1 << 0) | (1 << 7), (1 << 0) | (1 << 56), (1 << 63) | (1 << 56), (1 << 63) | (1 << 7)} <= moves
    assert len(raw) == len(cu)


# ------------------------------------------------------------------------------------------------ 3. other lattices
def test_chain_6x1_has_no_up_or_down():
    H = HG.Lattice(6, 1, True, T_HOP, U)
    dets = HG.all_determinants(6, 2, 2)
    rng = random.Random(5)
    refs = rng.sample(dets, 30)
    coeffs = [rng.choice((-1, 1)) * rng.uniform(0.1, 1.0) for _ in refs]
    g = _host(6, 1, True, 2, 2).gpu()
    try:
        raw = _check_modes(H, g, refs, coeffs, 1e-300, slices=True)
    finally:
        g.close()
    assert all(k in (0, 1) for u, d in refs for _, _, k, _ in HG.hops(H, u, d))
    assert max(sum(1 for w in raw if w[2] == float(i)) for i in range(len(refs))) <= 1 + 2 * 4


def test_half_filling_4x4():
    """(8,8) on 4x4 periodic: from the Neel state every hop is open (64 of them); from two overlapping blocks of rows most are
    blocked and H_ii = U n_double"""
    H, hst = HG.Lattice(4, 4, True, T_HOP, U), _host(4, 4, True, 8, 8)
    rows = (0x00FF, 0x0FF0)
    refs = [(hst.hf_up, hst.hf_dn), rows, (0x0F0F, 0x0FF0)]
    assert (hst.hf_up, hst.hf_dn) == HG.neel(4, 4, 8, 8)
    nh = [len(HG.hops(H, u, d)) for u, d in refs]
    assert nh[0] == 64 and 0 < nh[1] < 32 and PC._pop(rows[0] & rows[1]) == 4
    g = hst.gpu()
    try:
        raw = _check_modes(H, g, refs, [0.6, -0.3, 0.2], 1e-300, slices=True)
        cu, cd, num, den = g.hci_connections(*_arrays(refs[1:2]), [-0.3], 1e-300, diag_mode=1)
    finally:
        g.close()
    assert [sum(1 for w in raw if w[2] == float(i)) - 1 for i in range(3)] == nh
    k = list(zip(cu.tolist(), cd.tolist())).index(rows)
    assert num[k] == (U * 4) * -0.3 and den[k] == -0.3


# ------------------------------------------------------------------------------------------------ 4. first-order space, lowest state
@pytest.fixture(scope="module")
def model33():
    H = HG.Lattice(3, 3, True, T_HOP, U)
    dets = HG.all_determinants(9, 2, 2)
    return H, dets, np.linalg.eigvalsh(HG.dense(H, dets))


def _unit(up, dn, det):
    """the unit vector on det in the list (up, dn), as a Davidson start vector"""
    v0 = np.zeros((len(up), 1))
    v0[list(zip(up.tolist(), dn.tolist())).index(det), 0] = 1.0
    return v0


def test_first_order_space_and_lowest_state(model33):
    """The ground level of 3x3 periodic (2,2) is fourfold, and the first determinant of the sorted list (both spins on sites 1 and 2,
    unchanged when up and dn are exchanged) has no component in it: the Davidson iteration never leaves the symmetry sector of its
    start vector, so from its default start (the unit vector on the first row) it ends on the lowest level of that sector, the fifth
    eigenvalue.  The ground energy is asked from the unit vector on the walk's start determinant, which overlaps the ground level."""
    from sqmc_amd.host import lowest_state
    H, dets, spectrum = model33
    e0 = float(spectrum[0])
    hst = _host(3, 3, True, 2, 2)
    start = (hst.hf_up, hst.hf_dn)
    assert start == HG.neel(3, 3, 2, 2)
    g = hst.gpu()
    try:
        for n_levels in (1, 2, 3):
            up, dn = hst.first_order_space(n_levels, g)
            assert list(zip(up.tolist(), dn.tolist())) == HG.breadth_first(H, start, n_levels), n_levels
        up, dn = hst.first_order_space(12, g)
        assert list(zip(up.tolist(), dn.tolist())) == dets and len(dets) == 1296
        w, X, _ = lowest_state(g, up, dn, v0=_unit(up, dn, start))
        w_first, _, _ = lowest_state(g, up, dn)
    finally:
        g.close()
    print("3x3 (2,2): E0 = %.12f (device Davidson from the start determinant), %.12f (dense), difference %.3g; from the first row %.12f, dense levels %s"
          % (w[0], e0, abs(w[0] - e0), w_first[0], np.round(spectrum[:6], 9).tolist()))
    assert abs(float(w[0]) - e0) <= 1e-9
    assert float(np.min(np.abs(spectrum - float(w_first[0])))) <= 1e-9 and float(w_first[0]) >= e0 - 1e-9        # an exact level of its own sector
    # without a context: one is opened for the call; the lists of the host loops
    for a, b in ((hst.first_order_space(2), hst._first_order_space_host(2)), (hst.connected(*start), hst._connected_host(*start)),
                 (hst.connected(0b11, 0b11), hst._connected_host(0b11, 0b11))):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].dtype == b[0].dtype == np.uint64


# ------------------------------------------------------------------------------------------------ 5. PT2
def test_hci_pt2_against_the_explicit_sum():
    """variational space: the start determinant and its hops, with its lowest_state vector; the device's delta_E against the
    checker's explicit sum within the checker's propagated rounding bound, with 1 and with 3 slices, and the same number of
    connections (the merged list, the variational determinants' own slots included)"""
    from sqmc_amd.host import lowest_state
    H, hst = HG.Lattice(3, 3, True, T_HOP, U), _host(3, 3, True, 2, 2)
    eps_pt = 1e-12
    g = hst.gpu()
    try:
        vu, vd = hst.first_order_space(1, g)
        w, X, _ = lowest_state(g, vu, vd)
        e_var, c = float(w[0]), X[:, 0].copy()
        got1, n1 = g.hci_pt2(vu, vd, c, e_var, eps_pt)
        got3, n3 = g.hci_pt2(vu, vd, c, e_var, eps_pt, n_slices=3)
    finally:
        g.close()
    var = list(zip(vu.tolist(), vd.tolist()))
    for (u, d), ci in zip(var, c.tolist()):                # nothing near the screen: the two sides cannot decide differently
        assert not 0.1 * eps_pt < abs(T_HOP * ci) < 10 * eps_pt
    want, n_out, n_vis, bound = HG.pt2(H, var, c.tolist(), e_var, eps_pt)
    print("3x3 (2,2): %d variational, %d outside, %d visited; delta_E = %.15g, device %.15g (1 slice) %.15g (3 slices), |difference| %.3g / %.3g, bound %.3g"
          % (len(var), n_out, n_vis, want, got1, got3, abs(got1 - want), abs(got3 - want), bound))
    assert 1 < len(var) < 1296 and n_out > 10 and want < 0
    assert n1 == n_vis and n3 == n_vis
    assert abs(got1 - want) <= bound and abs(got3 - want) <= bound


# ------------------------------------------------------------------------------------------------ 6. the walk set-up
SETUP_ARRAYS = ("psi_up", "psi_dn", "psi_c", "imp_up", "imp_dn", "prj_counts", "prj_indices", "prj_values", "ct_up", "ct_dn", "ct_num", "ct_den")


@pytest.mark.parametrize("shape,kw", [((4, 4, True, 8, 8), {}), ((4, 3, False, 3, 3), {}), ((4, 4, True, 8, 8), dict(n_levels=3, size_deterministic=2000, n_truncate_trial_wf=60))],
                         ids=["4x4_half_filling", "4x3_open_33", "4x4_three_levels"])
def test_setup_walk_equals_the_host_construction_bit_for_bit(shape, kw):
    hst = _host(*shape, 1.0, 4.0)
    g = hst.gpu()
    try:
        dev = hst.setup_walk(g, **kw)
        ref = hst._setup_walk_host(g, **kw)
    finally:
        g.close()
    for name in SETUP_ARRAYS:
        a, b = getattr(dev, name), getattr(ref, name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
    assert dev.tau == ref.tau and dev.e_var == ref.e_var and dev.e_trial0 == ref.e_trial0
    print("%s %s: Psi_T %d, deterministic %d, C(T) %d, e_var %.12f, e_trial0 %.12f" % (shape, kw, len(dev.psi_up), len(dev.imp_up), len(dev.ct_up), dev.e_var, dev.e_trial0))
    assert len(dev.psi_up) > 1 and len(dev.ct_up) > len(dev.psi_up)


# ------------------------------------------------------------------------------------------------ 7. the variational stage
def test_hci_variational_energies(model33):
    """Two eps_var values that leave the list well inside the space of 1296.  The screen is on |t c|, and determinants that the lattice
    symmetries map onto each other carry equal |c|, so such a list is closed under the symmetries and its levels keep their exact
    degeneracies.  (A list that is the whole space but for a determinant or two is not: at eps_var = 5e-3 the stage ends with 1295
    determinants, the fourfold ground level is split by about 1e-5, and the Davidson iteration, which stops when the eigenvalue moves by
    less than 1e-10 in a sweep, stalls inside the cluster: -6.824299230 from hci_variational, -6.824284671 from lowest_state started on
    the start determinant, both above the exact -6.824300765.  That is the iteration's stopping rule, not the generator.)
    lowest_state starts on the start determinant, the symmetry sector hci_variational itself starts in."""
    from sqmc_amd.host import hci_variational, lowest_state
    H, dets, spectrum = model33
    e0 = float(spectrum[0])
    hst = _host(3, 3, True, 2, 2)
    g = hst.gpu()
    res = []
    try:
        for eps_var in (1e-1, 5e-2):
            up, dn, wts, energy, hist = hci_variational(hst, g, eps_var)
            o = np.lexsort((dn, up))
            w, _, _ = lowest_state(g, up[o], dn[o], v0=_unit(up[o], dn[o], (hst.hf_up, hst.hf_dn)))      # the sector hci_variational itself starts in
            res.append((eps_var, len(up), float(energy[0]), float(w[0])))
    finally:
        g.close()
    for eps_var, n, e, e_own in res:
        print("eps_var %.0e: %d determinants, E = %.12f (lowest_state on the list %.12f), exact %.12f" % (eps_var, n, e, e_own, e0))
        assert e >= e0 - 1e-9 and abs(e - e_own) <= 1e-9 and 1 < n <= 1296
    assert res[1][2] <= res[0][2] + 1e-9 and res[1][1] > res[0][1] and res[1][1] < 1296 // 2
    assert res[0][2] < H.element(hst.hf_up, hst.hf_dn, hst.hf_up, hst.hf_dn)[0] - 0.1      # it did lower the energy


# ------------------------------------------------------------------------------------------------ 8. what stays refused
def test_doors_that_stay_refused():
    import sqmc_amd
    from sqmc_amd._lib import Pt2StochasticPlan
    UNSUPPORTED = -3                              # SQMC_ERR_UNSUPPORTED of include/sqmc_gpu.h
    hst = _host(4, 3, False, 2, 2)
    g = hst.gpu()
    try:
        doors = {"stochastic-PT plan": lambda: Pt2StochasticPlan(g, [hst.hf_up], [hst.hf_dn], [1.0], -1.0, 1e-9, 1e-3, 10),
                 "diag-update record": lambda: g.hci_connections_record([hst.hf_up], [hst.hf_dn], [1.0], 1e-9),
                 "diag-update mode": lambda: g.hci_set_diag_update(1),
                 "diag-update batch": lambda: g.diag_update_batch([0.0], [[1, 13, 2, 14]], [hst.hf_up], [hst.hf_dn]),
                 "active-space masks": lambda: g.hci_set_active_space(1, 1, 0, 0, 1)}
        for name, call in doors.items():
            with pytest.raises(sqmc_amd.SqmcGpuError) as ei:
                call()
            assert ei.value.code == UNSUPPORTED, (name, str(ei.value))
            if name == "stochastic-PT plan":
                assert "hubbard2" in str(ei.value)
        cu, cd, _, _ = g.hci_connections([hst.hf_up], [hst.hf_dn], [1.0], 1e-9)      # the context is still good
        assert len(cu) == 1 + len(HG.hops(HG.Lattice(4, 3, False, T_HOP, U), hst.hf_up, hst.hf_dn))
    finally:
        g.close()
