"""tests/orbhess_checker.py against itself and against orbopt_checker, and host.orbital_newton_step against dense Hessians built from
the checker.  No GPU.

The tolerances: the checker works in longdouble (64-bit mantissa here, 2^-64 ~ 5e-20); its energy route takes differences of nine
energies weighted by at most 16 x 205/72, so 1e-15 relative to the scale of the energy's terms is a margin of four orders over its
rounding and still ten orders below any error of sign, factor or index."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import orbopt_checker as OC       # noqa: E402
from tests import orbhess_checker as HC      # noqa: E402

LD = np.longdouble
SIZES = [3, 4, 5, 6]


def _sys(n):
    return OC.random_system(n, 9100 + n)


def _scale(h, e, D, G):
    return float(np.sum(np.abs(h)) * np.max(np.abs(D)) + np.sum(np.abs(e)) * np.max(np.abs(G)))


@pytest.mark.parametrize("n", SIZES)
def test_energy_route_agrees_with_the_literal_statement(n):
    h, e, D, G = _sys(n)
    k = HC.random_kappa(n, 10 + n)
    a, b = HC.sigma_from_energy(h, e, D, G, k), HC.sigma_literal(h, e, D, G, k)
    assert np.array_equal(a, -a.T)
    assert float(np.max(np.abs(a - b))) <= 1e-15 * _scale(h, e, D, G)
    assert float(np.max(np.abs(a))) > 1e-2 * float(np.max(np.abs(D)))          # and it is not zero


@pytest.mark.parametrize("n", [3, 5])
def test_energy_route_agrees_with_central_differences_of_the_energy(n):
    """d2/ds dt E(exp(s kappa + t K_pq)) by the four-point cross difference at step 1e-4 in longdouble: truncation ~ step^2"""
    h, e, D, G = _sys(n)
    k = HC.random_kappa(n, 20 + n)
    sig = HC.sigma_from_energy(h, e, D, G, k)

    def expm(X):
        out, term = np.eye(n, dtype=LD), np.eye(n, dtype=LD)
        for j in range(1, 30):
            term = term @ X / LD(j)
            out = out + term
        return out
    st = LD(1) / LD(10000)
    kl = np.asarray(k, LD)
    for p, q in [(0, 1), (0, n - 1), (n - 2, n - 1)]:
        Y = HC.K(n, p, q)
        E = lambda s, t: OC.energy(h, e, D, G, expm(s * kl + t * Y))
        fd = (E(st, st) - E(st, -st) - E(-st, st) + E(-st, -st)) / (4 * st * st)
        assert abs(float(fd - sig[p, q])) <= 1e-6 * _scale(h, e, D, G), (p, q)


@pytest.mark.parametrize("n", SIZES)
def test_sigma_of_a_pair_generator_is_the_second_derivative_along_it(n):
    h, e, D, G = _sys(n)
    pairs = [(0, 1), (1, n - 1), (0, n - 1)]
    want = OC.derivatives(h, e, D, G, pairs)
    for p, q in pairs:
        got = HC.sigma_dot(h, e, D, G, HC.K(n, p, q), HC.K(n, p, q))
        assert abs(float(got - want[(p, q)][1])) <= 1e-15 * _scale(h, e, D, G), (p, q)


@pytest.mark.parametrize("n", SIZES)
def test_the_hessian_is_symmetric(n):
    h, e, D, G = _sys(n)
    k, lam = HC.random_kappa(n, 30 + n), HC.random_kappa(n, 40 + n)
    s_k, s_l = HC.sigma_literal(h, e, D, G, k), HC.sigma_literal(h, e, D, G, lam)
    dot = lambda a, b: np.sum(np.triu(np.asarray(a, LD), 1) * np.triu(np.asarray(b, LD), 1))
    assert abs(float(dot(k, s_l) - dot(lam, s_k))) <= 1e-15 * n * n * _scale(h, e, D, G)
    assert abs(float(dot(lam, s_k) - HC.sigma_dot(h, e, D, G, k, lam))) <= 1e-15 * n * n * _scale(h, e, D, G)


@pytest.mark.parametrize("n", SIZES)
def test_one_index_transform_is_the_first_order_coefficient_of_the_rotation(n):
    """rotate_integrals(I + t kappa) is a polynomial of degree 4 in t: its t^1 coefficient from five samples at t = -2 .. 2 by the
    five-point first-derivative formula, exact up to degree 4.  A general (not antisymmetric) kappa."""
    h, e, _, _ = _sys(n)
    k = HC.random_kappa(n, 50 + n, antisymmetric=False)
    ht, et = HC.one_index_literal(h, e, k)
    w = {-2: LD(1) / LD(12), -1: LD(-2) / LD(3), 1: LD(2) / LD(3), 2: LD(-1) / LD(12)}
    d1, d2 = np.zeros((n, n), LD), np.zeros((n,) * 4, LD)
    for t, wt in w.items():
        a, b = OC.rotate_integrals(h, e, np.eye(n, dtype=LD) + LD(t) * np.asarray(k, LD))
        d1, d2 = d1 + wt * a, d2 + wt * b
    assert float(np.max(np.abs(d1 - ht))) <= 1e-15 * float(np.max(np.abs(h))) * n * n
    assert float(np.max(np.abs(d2 - et))) <= 1e-15 * float(np.max(np.abs(e))) * n ** 4
    # the 8-fold symmetry survives any kappa
    et = np.asarray(et, float)
    assert np.allclose(et, et.transpose(1, 0, 2, 3), atol=1e-13) and np.allclose(et, et.transpose(2, 3, 0, 1), atol=1e-13)
    a1, a2 = HC.one_index_abs(h, e, k)
    assert np.all(np.abs(np.asarray(ht, float)) <= a1 * (1 + 1e-12)) and np.all(np.abs(et) <= a2 * (1 + 1e-12))


def test_entries_agree_with_the_dense_literal_statement():
    n = 5
    h, e, D, G = _sys(n)
    k = HC.random_kappa(n, 60)
    F = OC.fock_literal(h, e, D, G)
    g = 2 * (F - F.T)
    full = HC.sigma_literal(h, e, D, G, k)
    pairs = [(0, 1), (3, 1), (2, 4)]
    for (p, q), v in HC.sigma_literal_entries(h, e, D, G, k, pairs, g).items():
        assert abs(float(v - full[p, q])) <= 1e-15 * _scale(h, e, D, G)


# ------------------------------------------------------------------------------------------------------------------ the Newton-CG step
# The cases were chosen by running the checker.  Random D and G are no state's matrices and none of 200 seeds gave a positive
# definite Hessian, so the positive case takes the integrals of seed 9204 at 4 orbitals and the matrices of a wavefunction: the
# exact ground state of the complete space of 3 electrons (a minimum of the fixed-coefficient energy: eigenvalues 12 .. 155) with
# seeded noise of 0.1 on its coefficients, which leaves the Hessian positive definite (8.3 .. 129) and makes max|g| 6.4.
# Seed 9205 at 5 orbitals with random matrices is indefinite (-430 .. 387).
def _system(n, seed, state):
    h, e, D, G = OC.random_system(n, seed)
    if state:
        dets = OC.complete_space(n, 2, 1)
        Hm = OC.hamiltonian_matrix(OC.dense_hamiltonian(h, e, 0.0), dets)
        c = np.linalg.eigh((Hm + Hm.T) / 2)[1][:, 0]
        c = c + 0.1 * np.random.default_rng(seed).standard_normal(len(c))
        D, G = OC.density_matrices(dets, c / np.linalg.norm(c), n)
    return h, e, D, G


def _dense(n, seed, sym, state=False):
    h, e, D, G = _system(n, seed, state)
    pairs = [(p, q) for p in range(n) for q in range(p + 1, n) if sym[p] == sym[q]]
    Hm = HC.hessian_matrix(h, e, D, G, pairs)
    d1, d2 = OC.all_pair_derivatives(h, e, D, G)
    g, hd = np.asarray(d1, float), np.asarray(d2, float)
    P, Q = np.array([p for p, _ in pairs]), np.array([q for _, q in pairs])

    def hv(kappa):
        assert np.array_equal(kappa, -kappa.T)
        out = np.full((n, n), 123.0)                 # entries outside the pairs must not be read
        out[P, Q] = Hm @ kappa[P, Q]
        out[Q, P] = -out[P, Q]
        return out
    return g, hd, pairs, P, Q, Hm, hv


POSITIVE = (4, 9204)
INDEFINITE = (5, 9205)


def test_newton_step_solves_a_positive_definite_system():
    from sqmc_amd import host as H
    n, seed = POSITIVE
    g, hd, pairs, P, Q, Hm, hv = _dense(n, seed, [1] * n, state=True)
    assert np.linalg.eigvalsh(Hm)[0] > 1.0 and np.max(np.abs(g)) > 1.0
    assert np.allclose(np.diag(Hm), hd[P, Q], rtol=1e-12)          # the checker's diagonal is orbopt_checker's second derivative
    kappa, rec = H.orbital_newton_step(hv, g, hd, [1] * n, max_step=1e9, cg_tol=1e-12, max_cg=4 * len(P))
    want = -np.linalg.solve(Hm, g[P, Q])
    assert rec["cg_stop"] == "converged" and 1 <= rec["cg_iterations"] <= 4 * len(P)
    assert np.max(np.abs(kappa[P, Q] - want)) <= 1e-9 * np.max(np.abs(want))
    assert np.array_equal(kappa, -kappa.T) and not np.signbit(kappa[kappa == 0.0]).any()
    x = kappa[P, Q]
    assert abs(rec["predicted_change"] - (g[P, Q] @ x + 0.5 * x @ Hm @ x)) <= 1e-12 * abs(rec["predicted_change"])
    assert rec["predicted_change"] < 0


def test_newton_step_stops_on_negative_curvature():
    from sqmc_amd import host as H
    n, seed = INDEFINITE
    g, hd, pairs, P, Q, Hm, hv = _dense(n, seed, [1] * n)
    assert np.linalg.eigvalsh(Hm)[0] < 0 < np.linalg.eigvalsh(Hm)[-1]
    kappa, rec = H.orbital_newton_step(hv, g, hd, [1] * n, cg_tol=1e-12, max_cg=10 * len(P))
    assert rec["cg_stop"] == "negative_curvature"
    x = kappa[P, Q]
    assert g[P, Q] @ x < 0 and np.max(np.abs(kappa)) <= H.ORBOPT_MAX_STEP
    assert abs(rec["predicted_change"] - (g[P, Q] @ x + 0.5 * x @ Hm @ x)) <= 1e-12 * max(abs(rec["predicted_change"]), abs(g[P, Q] @ x))
    # negative curvature at the very first direction: the preconditioned steepest-descent direction itself
    Hneg = -np.eye(len(P))

    def hv2(k):
        out = np.zeros((n, n)); out[P, Q] = Hneg @ k[P, Q]; out[Q, P] = -out[P, Q]
        return out
    k2, rec2 = H.orbital_newton_step(hv2, g, hd, [1] * n, min_hess=0.1, max_step=1e9)
    assert rec2["cg_stop"] == "negative_curvature" and rec2["cg_iterations"] == 1
    assert np.array_equal(k2[P, Q], -g[P, Q] / np.maximum(np.abs(hd[P, Q]), 0.1))


def test_newton_step_caps_counts_and_respects_irreps():
    from sqmc_amd import host as H
    n, seed = 5, 9205
    sym = [1, 2, 1, 2, 1]
    g, hd, pairs, P, Q, Hm, hv = _dense(n, seed, sym)
    shift = max(0.0, -float(np.linalg.eigvalsh(Hm)[0])) + 1.0
    Hp = Hm + shift * np.eye(len(P))
    calls = []

    def hvp(k):
        calls.append(1)
        between = np.not_equal.outer(np.array(sym), np.array(sym))
        assert np.all(k[between] == 0.0)
        out = np.full((n, n), 7.0); out[P, Q] = Hp @ k[P, Q]; out[Q, P] = -out[P, Q]
        return out
    kappa, rec = H.orbital_newton_step(hvp, g, hd, sym, max_step=0.01, cg_tol=1e-12, max_cg=2)
    assert rec["cg_stop"] == "max_iterations" and rec["cg_iterations"] == 2 == len(calls)
    between = np.not_equal.outer(np.array(sym), np.array(sym))
    assert np.all(kappa[between] == 0.0) and np.all(np.diag(kappa) == 0.0) and not np.signbit(kappa[kappa == 0.0]).any()
    assert 0.0 < np.max(np.abs(kappa)) <= 0.01 and np.max(np.abs(kappa)) > 0.01 * (1 - 1e-12)
    x = kappa[P, Q]
    assert abs(rec["predicted_change"] - (g[P, Q] @ x + 0.5 * x @ Hp @ x)) <= 1e-12 * abs(g[P, Q] @ x)
    # a zero gradient: no product, a zero step
    k0, rec0 = H.orbital_newton_step(hvp, np.zeros((n, n)), hd, sym)
    assert not k0.any() and rec0 == {"cg_iterations": 0, "cg_stop": "converged", "predicted_change": 0.0} and len(calls) == 2
    with pytest.raises(ValueError):
        H.orbital_newton_step(hvp, g, hd, sym, max_cg=0)
    with pytest.raises(ValueError):
        H.orbital_newton_step(hvp, g[:3, :3], hd, sym)


def test_host_yardstick_is_the_literal_formula():
    """host.orbital_hessian_vector_host on a ChemHost-free stand-in: the function only needs dense_integrals, so it is given one"""
    from sqmc_amd import host as H
    n = 4
    h, e, D, G = _sys(n)
    k = HC.random_kappa(n, 70)
    saved = H.dense_integrals
    H.dense_integrals = lambda host: (h, e, 0.0)
    try:
        got = H.orbital_hessian_vector_host(None, D, G, k)
        ht, et = H.one_index_transform_host(None, k)
    finally:
        H.dense_integrals = saved
    want = np.asarray(HC.sigma_from_energy(h, e, D, G, k), float)
    assert np.max(np.abs(got - want)) <= 1e-12 * _scale(h, e, D, G)
    lt, le = HC.one_index_literal(h, e, k)
    assert np.max(np.abs(ht - np.asarray(lt, float))) <= 1e-13 * n and np.max(np.abs(et - np.asarray(le, float))) <= 1e-13 * n
