"""tests/hubbardk_sym_checker.py against the facts the symmetry-adapted hubbardk path rests on (4x4, t = 1, U = 4; no GPU):
the sizes of the sectors, their lowest eigenvalues, that the orbit basis is an invariant subspace of the plain Hamiltonian, and that
the modelled move is unbiased by exact enumeration of its triples."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import hubbardk_checker as HK          # noqa: E402
from tests import hubbardk_sym_checker as HS      # noqa: E402

T_HOP, U, TAU = 1.0, 4.0, 0.01
SECTORS = [(1, 1), (1, -1), (-1, 1), (-1, -1)]
LIVE_22 = {(1, 1): 91, (1, -1): 46, (-1, 1): 53, (-1, -1): 50}
E0_22 = {(1, 1): -10.910328101765, (1, -1): -8.0, (-1, 1): -7.561297824015, (-1, -1): -8.0}
PLAIN_E0_22 = -11.530292402630


@pytest.fixture(scope="module")
def plain22():
    H = HK.HubbardKH(4, 4, T_HOP, U)
    dets = HK.sector(H, 2, 2, (0, 0))
    A = HK.dense(H, dets, lambda u, d: HK.excitations_hubbardk(H, u, d))
    return H, dets, A


@pytest.fixture(scope="module")
def sectors22(plain22):
    H, dets, A = plain22
    return {zp: HS.Sector(H, 2, 2, zp[0], zp[1], dets, A) for zp in SECTORS}


def test_orbital_order_and_start_determinants():
    H = HK.HubbardKH(4, 4, T_HOP, U)
    assert H.k[:5] == [(0, 0), (-2, 0), (0, -2), (0, 2), (2, 0)]
    assert H.momentum(3, 3) == H.fold((-4, 0)) != (0, 0)
    assert H.momentum(17, 3) == (0, 0)


def test_group_is_c4_times_reflection_times_spin_inversion():
    H = HK.HubbardKH(4, 4, T_HOP, U)
    G = HS.Group(H, 2, 2, 1, 1)
    c4, rf = G.maps_one_based()
    n = H.norb
    m = [[c4[i][q] - 1 for i in range(n)] for q in range(3)] + [[x - 1 for x in rf]]
    for q in range(4):
        assert sorted(m[q]) == list(range(n))
        assert all(H.eps[m[q][i]] == H.eps[i] for i in range(n))
    assert all(m[0][m[0][i]] == m[1][i] and m[0][m[1][i]] == m[2][i] and m[0][m[2][i]] == i and m[3][m[3][i]] == i for i in range(n))
    assert len({tuple(e[0]) for e in G.elements}) == 16


def test_sector_sizes_2up_2dn(plain22, sectors22):
    H, dets, A = plain22
    assert len(dets) == 912
    for zp, S in sectors22.items():
        assert len(S.reps) == 102
        assert len(S.live) == LIVE_22[zp], (zp, len(S.live))


def test_sector_sizes_1up_1dn():
    H = HK.HubbardKH(4, 4, T_HOP, U)
    dets = HK.sector(H, 1, 1, (0, 0))
    assert len(dets) == 16
    A = HK.dense(H, dets, lambda u, d: HK.excitations_hubbardk(H, u, d))
    for zp in SECTORS:
        S = HS.Sector(H, 1, 1, zp[0], zp[1], dets, A)
        assert len(S.reps) == 6 and len(S.live) == (6 if zp == (1, 1) else 0)
        if zp == (1, 1):
            e = np.linalg.eigvalsh(S.M)[0]
            assert abs(e - (-7.838927194942)) < 1e-11 and abs(e - np.linalg.eigvalsh(A)[0]) < 1e-12


def test_lowest_eigenvalues_and_invariance(plain22, sectors22):
    H, dets, A = plain22
    wa = np.linalg.eigvalsh(A)
    assert abs(wa[0] - PLAIN_E0_22) < 1e-11
    for zp, S in sectors22.items():
        V, M = S.V, S.M
        assert np.max(np.abs(V.T @ V - np.eye(V.shape[1]))) < 1e-14
        assert np.max(np.abs(A @ V - V @ M)) < 1e-13
        assert np.max(np.abs(M - M.T)) < 1e-14
        wm = np.linalg.eigvalsh(M)
        assert abs(wm[0] - E0_22[zp]) < 1e-11, (zp, wm[0])
        assert max(np.min(np.abs(wa - x)) for x in wm) < 1e-12
        assert abs(wm[0] - PLAIN_E0_22) > 0.5          # the plain ground state is in none of the four sectors


def test_reduce_is_consistent_with_the_orbit_vectors(plain22, sectors22):
    H, dets, A = plain22
    for zp, S in sectors22.items():
        for d in dets[::7]:
            imgs, phases, rep, pw, norm, nd = S.G.reduce(d)
            assert rep == S.rep_of[d] and imgs[0] == d and phases[0] == 1
            assert (nd > 0) == S.is_live(d)
            if nd:
                assert nd == len(set(imgs)) and abs(norm * norm * nd - 16.0) < 1e-12
                seen = {}
                for x, ph in zip(imgs, phases):
                    assert seen.setdefault(x, ph) == ph          # equal images carry equal phases


def test_move_is_unbiased_by_exact_enumeration(plain22, sectors22):
    """for every live representative i of every sector: sum over all nup ndn (nsites - nup) triples, each with probability 1 / N, of the
    modelled move's weight per returned determinant = -tau M[:, i] off the diagonal, to 1e-13"""
    H, dets, A = plain22
    for zp, S in sectors22.items():
        for i in S.live:
            tr = HK.triples_hubbardk(H, *i)
            assert len(tr) == 2 * 2 * 14
            acc = {}
            for t in tr:
                j, w = S.move(i, t[4], TAU)
                if w != 0.0:
                    assert j != i and j in S.pos
                    acc[j] = acc.get(j, 0.0) + w / len(tr)
            want = -TAU * S.M[:, S.pos[i]]
            for j in S.live:
                if j != i:
                    assert abs(acc.get(j, 0.0) - want[S.pos[j]]) <= 1e-13, (zp, i, j)
