"""tests/rdm_checker.py against what a 1-RDM is known to satisfy, and the host-side pieces of the natural-orbital stage
(host.natural_orbitals, the printed forms) against direct computation.  No GPU."""
import math
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import rdm_checker as RC          # noqa: E402


def _string(rng, norb, n):
    return sum(1 << k for k in rng.sample(range(norb), n))


def _random_list(rng, norb, nup, ndn, n):
    dets = set()
    while len(dets) < n:
        dets.add((_string(rng, norb, nup), _string(rng, norb, ndn)))
    dets = sorted(dets)
    rng.shuffle(dets)
    return dets, [rng.uniform(-1.0, 1.0) for _ in dets]


def test_operators_on_tuples():
    assert RC.occupation(0b101001) == (0, 3, 5)
    assert RC.annihilate((0, 3, 5), 3) == ((0, 5), -1) and RC.annihilate((0, 3, 5), 1) is None
    assert RC.create((0, 5), 3) == ((0, 3, 5), -1) and RC.create((0, 5), 5) is None
    # 0 -> 7 across 0, 1, 2 and 3 other electrons: the sign alternates
    for between in range(4):
        occ = (0,) + tuple(range(1, between + 1))
        assert RC.move(occ, 0, 7) == (tuple(range(1, between + 1)) + (7,), (-1) ** between)


def test_hf_determinant_gives_the_occupation_matrix():
    norb = 6
    m = RC.one_rdm([(0b000111, 0b000011)], [1.0], norb).matrix()
    want = [[0.0] * norb for _ in range(norb)]
    want[0][0] = want[1][1] = 2.0
    want[2][2] = 1.0
    assert m == want


def test_trace_and_symmetry_of_random_lists():
    rng = random.Random(20161)
    for norb, nup, ndn, n in ((5, 2, 2, 30), (6, 3, 1, 40), (7, 1, 3, 25), (4, 2, 2, 36)):
        dets, c = _random_list(rng, norb, nup, ndn, n)
        r = RC.one_rdm(dets, c, norb)
        norm = math.fsum(x * x for x in c)
        assert abs(r.trace() - (nup + ndn) * norm) <= r.trace_bound() + 4 * RC.U * (nup + ndn) * norm
        off = 0
        for p in range(norb):
            for q in range(norb):
                assert r.count(p, q) == r.count(q, p)
                assert abs(r.value(p, q) - r.value(q, p)) <= r.bound(p, q) + r.bound(q, p)
                off += (p != q) and r.count(p, q) > 0
        assert off > 0
        # the filter drops whole entries and leaves the others' terms alone
        sym = [1 + (k % 2) for k in range(norb)]
        f = RC.one_rdm(dets, c, norb, sym)
        for p in range(norb):
            for q in range(norb):
                if sym[p] != sym[q]:
                    assert f.count(p, q) == 0 and f.value(p, q) == 0.0
                else:
                    assert f.terms[p][q] == r.terms[p][q]


def test_two_electron_natural_occupations():
    """one up and one dn electron, psi = sum C[a][b] |a up, b dn>: the spin-traced 1-RDM is C C^T + C^T C"""
    from sqmc_amd import host as H
    rng = random.Random(4)
    for norb in (4, 5, 6):
        C = np.array([[rng.uniform(-1, 1) for _ in range(norb)] for _ in range(norb)])
        dets = [(1 << a, 1 << b) for a in range(norb) for b in range(norb)]
        c = [C[a][b] for a in range(norb) for b in range(norb)]
        order = list(range(len(dets)))
        rng.shuffle(order)
        r = RC.one_rdm([dets[k] for k in order], [c[k] for k in order], norb)
        direct = C @ C.T + C.T @ C
        m = np.array(r.matrix())
        assert np.max(np.abs(m - direct)) <= 4 * norb * RC.U * np.max(np.abs(C)) ** 2 * norb
        occ, _ = H.natural_orbitals(m, [1] * norb)
        want = np.sort(np.linalg.eigvalsh(direct))[::-1]
        assert np.max(np.abs(occ - want)) <= 64 * norb * 2.0 ** -52 * np.max(np.abs(want))       # eigh of two matrices 1e-16 apart: backward stable, Weyl


def test_natural_orbitals_by_block():
    from sqmc_amd import host as H
    rng = np.random.RandomState(7)
    sym = np.array([1, 2, 1, 3, 2, 1, 2])
    n = len(sym)
    m = np.zeros((n, n))
    blocks = {}
    for irrep in (1, 2, 3):
        ix = np.nonzero(sym == irrep)[0]
        a = rng.uniform(-1, 1, (len(ix), len(ix)))
        blocks[irrep] = a + a.T
        m[np.ix_(ix, ix)] = blocks[irrep]
    occ, vec = H.natural_orbitals(m, sym)
    for irrep in (1, 2, 3):
        ix = np.nonzero(sym == irrep)[0]
        want = np.linalg.eigh(blocks[irrep])[0][::-1]
        assert np.array_equal(occ[ix], want)
        assert np.all(np.diff(occ[ix]) <= 0)
        other = np.nonzero(sym != irrep)[0]
        assert np.all(vec[np.ix_(other, ix)] == 0.0)
    assert np.max(np.abs(vec @ np.diag(occ) @ vec.T - m)) <= 64 * n * 2.0 ** -52 * np.max(np.abs(occ))
    assert np.max(np.abs(vec.T @ vec - np.eye(n))) <= 64 * n * 2.0 ** -52


def test_printed_forms():
    from sqmc_amd import host as H
    m = [[1.98767, -0.0004, 0.0], [-0.0004, 0.5, -12.3456], [0.0, -12.3456, 123456.7891]]
    assert H.format_real_matrix(m) == ("     1.988    -0.000     0.000\n"
                                       "    -0.000     0.500   -12.346\n"
                                       "     0.000   -12.346123456.789")
    assert H.format_eigenvalues([1.98767, 0.0125, -3.2e-7]) == " 1.9877E+00 1.2500E-02-3.2000E-07"
    v = [2.0] * 10 + [1.0e-3]
    assert H.format_eigenvalues(v) == " 2.0000E+00" * 10 + "\n 1.0000E-03"
