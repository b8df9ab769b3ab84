"""The orbital-gradient checker held against itself and against the other checkers, and the host-side pieces of the orbital step.
No GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import orbopt_checker as OC       # noqa: E402
from tests import rdm2_checker as R2         # noqa: E402

LD = OC.LD


def _pairs(n):
    return [(p, q) for p in range(n) for q in range(n) if p != q]


def test_fourier_derivatives_agree_with_central_differences():
    """every pair of a 4-orbital system: the gap to a central difference shrinks by 4 when the step is halved (its error is
    E''' step^2 / 6 and E'''' step^2 / 12; the next order changes the ratio by step^2 ~ 1e-4)"""
    n = 4
    h, e, D, G = OC.random_system(n, 11)
    E0 = OC.energy(h, e, D, G)
    for p, q in _pairs(n):
        d1, d2 = OC.fourier_derivatives(OC.full_samples(h, e, D, G, p, q))
        gaps = []
        for step in (LD(1) / 64, LD(1) / 128):
            ep, em = (OC.energy(h, e, D, G, OC.plane_rotation(n, p, q, s)) for s in (step, -step))
            gaps.append((abs((ep - em) / (2 * step) - d1), abs((ep - 2 * E0 + em) / (step * step) - d2)))
        for k in (0, 1):
            assert gaps[0][k] > 1e-9 and 3.9 < float(gaps[0][k] / gaps[1][k]) < 4.1, (p, q, k, gaps)


@pytest.mark.parametrize("n", [2, 3, 5])
def test_plane_expansion_equals_the_transformed_integrals(n):
    """plane_samples + E(0) against full_samples, and their derivatives: longdouble roundings of sums of about n^4 terms apart"""
    for sym in (True, False):
        h, e, D, G = OC.random_system(n, 20 + n, symmetric_g=sym)
        scale = float(np.sum(np.abs(h) * np.abs(D)) + 0.5 * np.sum(np.abs(e) * np.abs(G).transpose(0, 2, 1, 3)))
        E0 = OC.energy(h, e, D, G)
        for p, q in _pairs(n):
            a, b = OC.plane_samples(h, e, D, G, p, q), OC.full_samples(h, e, D, G, p, q)
            assert max(abs(float(x + E0 - y)) for x, y in zip(a, b)) <= 64 * n ** 4 * 2.0 ** -63 * scale
            da, db = OC.fourier_derivatives(a), OC.fourier_derivatives(b)
            assert abs(float(da[0] - db[0])) <= 1e3 * n ** 4 * 2.0 ** -63 * scale and abs(float(da[1] - db[1])) <= 1e4 * n ** 4 * 2.0 ** -63 * scale


def test_energy_of_rotated_integrals_is_the_expectation_value():
    """E(U) from the density matrices of rdm_checker / rdm2_checker equals <Psi|H'|Psi> with proposal_checker's second-quantised
    Hamiltonian on the rotated integrals"""
    n, core = 4, -1.25
    h, e, _, _ = OC.random_system(n, 31)
    dets = OC.complete_space(n, 2, 1)
    rng = np.random.default_rng(32)
    keep = sorted(rng.choice(len(dets), 13, replace=False).tolist())
    dets = [dets[k] for k in keep]
    c = rng.standard_normal(len(dets)); c /= np.linalg.norm(c)
    D, G = OC.density_matrices(dets, c, n)
    n2 = R2.norm2(c)
    U = np.linalg.qr(rng.standard_normal((n, n)))[0]
    for rot in (None, U, OC.plane_rotation(n, 1, 3, 0.7)):
        h2, e2 = (h, e) if rot is None else OC.rotate_integrals(h, e, rot)
        want, bound, sa = R2.expectation(OC.dense_hamiltonian(np.asarray(h2, float), np.asarray(e2, float), core), dets, c)
        got = float(OC.energy(h, e, D, G, rot)) + core * n2
        # the rotated integrals are rounded to double for the Hamiltonian: 2^-53 of every term; the matrices' own roundings ride on sa
        assert abs(got - want) <= bound + 64 * 2.0 ** -53 * (sa + abs(core))


@pytest.mark.parametrize("nup,ndn", [(1, 1), (2, 1), (2, 2)])
def test_gradient_vanishes_for_the_exact_ground_state(nup, ndn):
    """complete space of 2, 3 and 4 electrons in 4 orbitals, dense eigh: every gradient entry below 1e-9 max|F| (a generous margin
    over eigh's n 2^-53 ||H||, not a measurement); truncated to half its determinants the gradient is far above it"""
    n = 4
    h, e, _, _ = OC.random_system(n, 40 + nup + ndn)
    dets = OC.complete_space(n, nup, ndn)
    Hm = OC.hamiltonian_matrix(OC.dense_hamiltonian(h, e), dets)
    assert np.allclose(Hm, Hm.T, atol=1e-12)
    c = np.linalg.eigh(Hm)[1][:, 0]
    D, G = OC.density_matrices(dets, c, n)
    fmax = float(np.max(np.abs(OC.fock_literal(h, e, D, G))))
    g = max(abs(float(v[0])) for v in OC.derivatives(h, e, D, G).values())
    assert g < 1e-9 * fmax, (g, fmax)
    big = np.argsort(-np.abs(c), kind="stable")[:len(dets) // 2]
    D, G = OC.density_matrices([dets[k] for k in big], c[big], n)
    g = max(abs(float(v[0])) for v in OC.derivatives(h, e, D, G).values())
    assert g > 1e-3 * fmax, (g, fmax)


@pytest.mark.parametrize("n", [2, 5, 26, 64])
def test_rotation_from_kappa(n):
    from sqmc_amd import host as H
    rng = np.random.default_rng(50 + n)
    k = rng.uniform(-0.3, 0.3, (n, n)); k = np.triu(k, 1); k = k - k.T
    U = H.rotation_from_kappa(k)
    assert U.dtype == np.float64 and U.shape == (n, n)
    assert np.max(np.abs(U.T @ U - np.eye(n))) <= n * 2.0 ** -50
    p, q, th = 0, n - 1, 0.37
    k = np.zeros((n, n)); k[p, q], k[q, p] = th, -th
    assert np.max(np.abs(H.rotation_from_kappa(k) - np.asarray(OC.plane_rotation(n, p, q, th), float))) <= n * 2.0 ** -50
    assert np.array_equal(H.rotation_from_kappa(np.zeros((n, n))), np.eye(n))
    with pytest.raises(ValueError):
        H.rotation_from_kappa(np.ones((n, n)))


def test_orbital_step_is_zero_between_irreps_and_respects_max_step():
    from sqmc_amd import host as H
    n = 7
    rng = np.random.default_rng(60)
    g = rng.standard_normal((n, n)); g = g - g.T
    hd = rng.standard_normal((n, n)) * 3.0; hd = hd + hd.T; np.fill_diagonal(hd, 0.0)
    hd[0, 1] = hd[1, 0] = 1e-9                     # below min_hess
    sym = np.array([1, 1, 2, 1, 3, 2, 1])
    for max_step in (0.05, 1e9):
        k = H.orbital_step(g, hd, sym, min_hess=0.1, max_step=max_step)
        assert np.array_equal(k, -k.T) and not np.signbit(k[k == 0.0]).any()
        assert np.max(np.abs(k)) <= max_step
        for p in range(n):
            for q in range(n):
                if sym[p] != sym[q] or p == q:
                    assert k[p, q] == 0.0
        raw = np.array([[-g[p, q] / max(abs(hd[p, q]), 0.1) if sym[p] == sym[q] and p != q else 0.0 for q in range(n)] for p in range(n)])
        if max_step > 1e8:
            assert np.allclose(k, raw, rtol=1e-15, atol=0.0)
            assert k[0, 1] == -g[0, 1] / 0.1
        else:
            assert np.max(np.abs(k)) > 0.05 * (1 - 1e-12)
            assert np.allclose(k / np.max(np.abs(k)), raw / np.max(np.abs(raw)), rtol=1e-12, atol=1e-15)


def test_host_formulas_are_the_derivatives():
    """host.orbital_gradient_host (the door's formulas in numpy) against the Fourier derivatives, within the door's bounds"""
    from sqmc_amd import host as H
    n = 5
    h, e, D, G = OC.random_system(n, 70)

    class _Dense(H.ChemHost):
        def __init__(self):
            pass
    keep = H.dense_integrals
    H.dense_integrals = lambda host: (h, e, 0.0)
    try:
        got = H.orbital_gradient_host(_Dense(), D, G)
    finally:
        H.dense_integrals = keep
    fabs = OC.fock_abs(h, e, D, G)
    assert np.all(np.abs(got["fock"] - np.asarray(OC.fock_literal(h, e, D, G), float)) <= OC.fock_bound(n, fabs))
    habs = OC.hdiag_abs(h, e, D, G, _pairs(n), fabs)
    for (p, q), (d1, d2) in OC.derivatives(h, e, D, G).items():
        assert abs(got["gradient"][p, q] - float(d1)) <= OC.gradient_bound(n, fabs, p, q)
        assert abs(got["hdiag"][p, q] - float(d2)) <= OC.hdiag_bound(n, habs[(p, q)])
