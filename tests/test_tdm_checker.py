"""tests/tdm_checker.py against itself, against tests/rdm2_checker.py / tests/rdm_checker.py and against tests/proposal_checker.py on
systems small enough to hold every determinant: all determinants of 2, 3 and 4 electrons in 4 orbitals.  No GPU, nothing from sqmc_amd."""
import math
import os
import random
import sys
from fractions import Fraction
from itertools import combinations

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import proposal_checker as PC     # noqa: E402
from tests import rdm_checker as RC          # noqa: E402
from tests import rdm2_checker as R2         # noqa: E402
from tests import tdm_checker as TC          # noqa: E402
from tests.test_rdm2_checker import RandomH  # noqa: E402

NORB = 4
SECTORS = [(1, 1), (2, 1), (2, 2), (2, 0), (3, 1)]


def _all_dets(nup, ndn):
    strings = lambda k: [sum(1 << o for o in c) for c in combinations(range(NORB), k)]
    return [(a, b) for a in strings(nup) for b in strings(ndn)]


def _coeffs(rng, n):
    c = [rng.uniform(-1.0, 1.0) for _ in range(n)]
    c[rng.randrange(n)] = 0.0
    return c


def _dyadic(rng, n):
    return [rng.randrange(-1024, 1025) / 1024.0 for _ in range(n)]


@pytest.mark.parametrize("nup,ndn", SECTORS)
def test_equal_vectors_reproduce_the_density_matrices_term_for_term(nup, ndn):
    rng = random.Random(13 * nup + ndn)
    dets = _all_dets(nup, ndn)
    c = _coeffs(rng, len(dets))
    two, ref2 = TC.two_tdm(dets, c, c, NORB), R2.two_rdm(dets, c, NORB)
    assert two.reached == ref2.reached
    for b in R2.BLOCKS:
        assert two.terms[b] == ref2.terms[b], b                      # the same loop: the same terms in the same order
    one, ref1 = TC.one_tdm(dets, c, c, NORB), RC.one_rdm(dets, c, NORB)
    for p in range(NORB):
        for r in range(NORB):
            assert sorted(one.terms[p][r]) == sorted(ref1.terms[p][r]), (p, r)
    sym = [0, 1, 0, 1]
    fil, ref = TC.one_tdm(dets, c, c, NORB, sym), RC.one_rdm(dets, c, NORB, sym)
    for p in range(NORB):
        for r in range(NORB):
            assert sorted(fil.terms[p][r]) == sorted(ref.terms[p][r]) and (sym[p] == sym[r] or not fil.terms[p][r])


@pytest.mark.parametrize("nup,ndn", SECTORS)
def test_polarisation_identity_is_exact_in_fractions(nup, ndn):
    """T(u,v) + T(v,u) = [Gamma(u+v) - Gamma(u-v)] / 2 and T(v,u)[p,q,r,s] = T(u,v)[r,s,p,q], one[v,u] = one[u,v]^t: on dyadic
    coefficients (integers / 1024) the sums and differences, every product and every sum of products are exact in Fractions, and
    rdm2_checker's doubles hold them exactly as well (products are multiples of 2^-20 below 2^2, a few hundred terms)"""
    rng = random.Random(17 * nup + ndn)
    dets = _all_dets(nup, ndn)
    u, v = _dyadic(rng, len(dets)), _dyadic(rng, len(dets))
    plus, minus = [a + b for a, b in zip(u, v)], [a - b for a, b in zip(u, v)]
    uv, vu = TC.two_tdm(dets, u, v, NORB, number=Fraction), TC.two_tdm(dets, v, u, NORB, number=Fraction)
    gp, gm = R2.two_rdm(dets, plus, NORB), R2.two_rdm(dets, minus, NORB)
    seen = 0
    for b in R2.BLOCKS:
        keys = set(uv.terms[b]) | set(vu.terms[b]) | set(gp.terms[b]) | set(gm.terms[b])
        for idx in keys:
            p, q, r, s = idx
            t_uv, t_vu = sum(uv.terms[b].get(idx, ()), Fraction(0)), sum(vu.terms[b].get(idx, ()), Fraction(0))
            assert t_vu == sum(uv.terms[b].get((r, s, p, q), ()), Fraction(0)), (b, idx)
            pol = (sum(map(Fraction, gp.terms[b].get(idx, ())), Fraction(0)) - sum(map(Fraction, gm.terms[b].get(idx, ())), Fraction(0))) / 2
            assert t_uv + t_vu == pol, (b, idx)
            assert Fraction(gp.value(b, idx)) - Fraction(gm.value(b, idx)) == 2 * pol
            seen += t_uv != t_vu
    assert seen > 0                                                  # the transition matrix is not symmetric
    o_uv, o_vu = TC.one_tdm(dets, u, v, NORB, number=Fraction), TC.one_tdm(dets, v, u, NORB, number=Fraction)
    dp, dm = RC.one_rdm(dets, plus, NORB), RC.one_rdm(dets, minus, NORB)
    for p in range(NORB):
        for r in range(NORB):
            a, bt = sum(o_uv.terms[p][r], Fraction(0)), sum(o_vu.terms[p][r], Fraction(0))
            assert bt == sum(o_uv.terms[r][p], Fraction(0))
            assert a + bt == (sum(map(Fraction, dp.terms[p][r]), Fraction(0)) - sum(map(Fraction, dm.terms[p][r]), Fraction(0))) / 2


@pytest.mark.parametrize("nup,ndn", SECTORS)
@pytest.mark.parametrize("kind", ["random", "hubbard"])
def test_transition_energy_from_the_matrices_is_the_matrix_element(nup, ndn, kind):
    H = RandomH(10 * nup + ndn) if kind == "random" else PC.HubbardH(2, 2, False, 1.0, 4.0)
    rng = random.Random(200 * nup + ndn)
    dets = _all_dets(nup, ndn)
    u, v = _coeffs(rng, len(dets)), _coeffs(rng, len(dets))
    one, two = TC.one_tdm(dets, u, v, NORB), TC.two_tdm(dets, u, v, NORB)
    e, be = TC.energy(H, one, two, TC.overlap(u, v))
    want, bw, _ = TC.expectation(H, dets, u, v)
    ovl_bound = abs(H.const) * len(dets) * RC.U * math.fsum(abs(a * b) for a, b in zip(u, v))
    print("%s (%d, %d): <u|H|v> = %.15g from the matrices, %.15g from the elements, bound = %.3g" % (kind, nup, ndn, e, want, be + bw + ovl_bound))
    assert abs(e - want) <= be + bw + ovl_bound
    assert abs(want) > 1e-3
    # the partial trace: sum_q sf[p,q,r,q] = (N - 1) one[r][p]
    n = nup + ndn
    for p in range(NORB):
        for r in range(NORB):
            got, bg = R2.partial_trace(two, p, r, n)
            w1 = (n - 1) * one.value(r, p)
            assert abs(got - w1) <= bg + (n - 1) * one.bound(r, p) + 2 * RC.U * abs(w1), (p, r, got, w1)
    tr = math.fsum(one.value(p, p) for p in range(NORB))
    assert abs(tr - n * TC.overlap(u, v)) <= math.fsum(one.bound(p, p) for p in range(NORB)) + (NORB + 2 * len(dets)) * RC.U * n * math.fsum(abs(a * b) for a, b in zip(u, v))


def test_two_eigenvectors_of_the_2x2_lattice():
    """two exact eigenvectors of different energy: <1|H|2> and the overlap vanish, <1|S^2|2> is the polarised rdm2_checker.s_squared"""
    H = PC.HubbardH(2, 2, False, 1.0, 4.0)
    dets = _all_dets(2, 2)
    n = len(dets)
    M = np.array([[H.element(ju, jd, iu, id_)[0] for (ju, jd) in dets] for (iu, id_) in dets])
    assert np.array_equal(M, M.T)
    e, vec = np.linalg.eigh(M)
    k = next(k for k in range(1, n) if e[k] - e[0] > 0.1)
    v1, v2 = vec[:, 0].tolist(), vec[:, k].tolist()
    one, two = TC.one_tdm(dets, v1, v2, NORB), TC.two_tdm(dets, v1, v2, NORB)
    ovl = TC.overlap(v1, v2)
    # LAPACK's eigenvectors are orthogonal and satisfy M v = e v to a modest multiple of n eps |M|
    slack = 64 * n * RC.U * max(1.0, float(np.abs(M).sum(axis=1).max()))
    assert abs(ovl) <= slack
    res = float(np.linalg.norm(M @ vec[:, k] - e[k] * vec[:, k]))
    h12, be = TC.energy(H, one, two, ovl)
    want, bw, _ = TC.expectation(H, dets, v1, v2)
    print("2x2: overlap %.3g, <1|H|2> = %.3g (elements: %.3g), bounds %.3g + %.3g, residual %.3g" % (ovl, h12, want, be, bw, res))
    assert abs(h12 - want) <= be + bw
    assert abs(h12) <= be + bw + abs(e[k]) * slack + res + slack
    s12, bs = TC.s_squared(two, dets, ovl)
    pol = TC.s_squared_polarised(dets, v1, v2, NORB)
    bp = TC.s_squared_polarised_bound(dets, v1, v2, NORB)
    assert abs(s12 - pol) <= bs + bp, (s12, pol, bs + bp)
    # and a transition matrix element of S^2 that does not vanish: random vectors
    rng = random.Random(9)
    a, b = _coeffs(rng, n), _coeffs(rng, n)
    t2 = TC.two_tdm(dets, a, b, NORB)
    sab, bs = TC.s_squared(t2, dets, TC.overlap(a, b))
    pol = TC.s_squared_polarised(dets, a, b, NORB)
    bp = TC.s_squared_polarised_bound(dets, a, b, NORB)
    assert abs(sab - pol) <= bs + bp and abs(pol) > 1e-3, (sab, pol)


def test_a_sample_gives_the_same_entries():
    rng = random.Random(5)
    dets = _all_dets(2, 2)
    u, v = _coeffs(rng, len(dets)), _coeffs(rng, len(dets))
    full = TC.two_tdm(dets, u, v, NORB)
    sample = {b: set(rng.sample(sorted(full.terms[b]), 10)) | {(0, 0, 0, 0)} for b in R2.BLOCKS}
    part = TC.two_tdm(dets, u, v, NORB, sample)
    assert part.reached == full.reached == R2.pattern(dets, NORB)
    for b in R2.BLOCKS:
        assert set(part.terms[b]) == sample[b] & set(full.terms[b])
        for idx in part.terms[b]:
            assert part.terms[b][idx] == full.terms[b][idx]
