"""tests/rdm2_checker.py against itself and against tests/proposal_checker.py / tests/rdm_checker.py on systems small enough to hold
every determinant: all determinants of 2, 3 and 4 electrons in 4 orbitals.  No GPU, nothing from sqmc_amd."""
import math
import os
import random
import sys
from itertools import combinations

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import proposal_checker as PC     # noqa: E402
from tests import rdm_checker as RC          # noqa: E402
from tests import rdm2_checker as R2         # noqa: E402

NORB = 4


class RandomH(PC.Hamiltonian):
    """a symmetric t and an 8-fold symmetric (pq|rs) on 4 orbitals, diagonal in spin"""

    def __init__(self, seed):
        rng = random.Random(seed)
        self.norb, self.const = NORB, rng.uniform(-1.0, 1.0)
        self.h1 = {(p, q): rng.uniform(-1.0, 1.0) for p in range(NORB) for q in range(p + 1)}
        self.h2 = {}
        for p in range(NORB):
            for q in range(NORB):
                for r in range(NORB):
                    for s in range(NORB):
                        self.h2.setdefault(PC._eri_key(p, q, r, s), rng.uniform(-1.0, 1.0))

    def t(self, P, Q):
        n = self.norb
        return self.h1[(max(P % n, Q % n), min(P % n, Q % n))] if P // n == Q // n else 0.0

    def v(self, P, Q, R, S):
        n = self.norb
        if P // n != Q // n or R // n != S // n:
            return 0.0
        return self.h2[PC._eri_key(P % n, Q % n, R % n, S % n)]


def _all_dets(nup, ndn):
    strings = lambda k: [sum(1 << o for o in c) for c in combinations(range(NORB), k)]
    return [(a, b) for a in strings(nup) for b in strings(ndn)]


def _coeffs(rng, n):
    c = [rng.uniform(-1.0, 1.0) for _ in range(n)]
    c[rng.randrange(n)] = 0.0
    return c


SECTORS = [(1, 1), (2, 1), (2, 2), (2, 0), (3, 1)]


@pytest.mark.parametrize("nup,ndn", SECTORS)
@pytest.mark.parametrize("kind", ["random", "hubbard"])
def test_energy_from_the_matrices_is_the_expectation_value(nup, ndn, kind):
    H = RandomH(10 * nup + ndn) if kind == "random" else PC.HubbardH(2, 2, False, 1.0, 4.0)
    rng = random.Random(100 * nup + ndn)
    dets = _all_dets(nup, ndn)
    c = _coeffs(rng, len(dets))
    one, two = RC.one_rdm(dets, c, NORB), R2.two_rdm(dets, c, NORB)
    e, be = R2.energy(H, one, two, R2.norm2(c))
    want, bw, _ = R2.expectation(H, dets, c)
    print("%s (%d, %d): E = %.15g, <H> = %.15g, |delta| = %.3g, bound = %.3g" % (kind, nup, ndn, e, want, abs(e - want), be + bw))
    assert abs(e - want) <= be + bw
    assert abs(want) > 1e-3


@pytest.mark.parametrize("nup,ndn", SECTORS)
def test_partial_trace_is_the_one_body_matrix(nup, ndn):
    rng = random.Random(7 * nup + ndn)
    dets = _all_dets(nup, ndn)
    c = _coeffs(rng, len(dets))
    one, two = RC.one_rdm(dets, c, NORB), R2.two_rdm(dets, c, NORB)
    n = nup + ndn
    for p in range(NORB):
        for r in range(NORB):
            got, bg = R2.partial_trace(two, p, r, n)
            want = (n - 1) * one.value(r, p)           # rdm_checker: M[p][r] = <a+_r a_p>
            assert abs(got - want) <= bg + (n - 1) * one.bound(r, p) + 2 * RC.U * abs(want), (p, r, got, want)


@pytest.mark.parametrize("nup,ndn", SECTORS)
def test_traces_and_symmetries(nup, ndn):
    rng = random.Random(3 * nup + ndn)
    dets = _all_dets(nup, ndn)
    c = _coeffs(rng, len(dets))
    two, n2 = R2.two_rdm(dets, c, NORB), R2.norm2(c)
    for b, want in (("aa", nup * (nup - 1)), ("bb", ndn * (ndn - 1)), ("ab", nup * ndn)):
        tr = math.fsum(two.value(b, (p, q, p, q)) for p in range(NORB) for q in range(NORB))
        # every determinant puts the double c_i c_i into `want` diagonal entries, so the exact sums agree; what differs is one rounding per
        # fsum (each entry's, the trace's, norm2's) and the product want * n2
        mass = math.fsum(abs(two.value(b, (p, q, p, q))) for p in range(NORB) for q in range(NORB))
        assert abs(tr - want * n2) <= RC.U * (mass + abs(tr) + 2 * want * n2), (b, tr, want * n2)
        for (p, q, r, s) in two.terms[b]:
            assert abs(two.value(b, (p, q, r, s)) - two.value(b, (r, s, p, q))) <= 2 * two.bound(b, (p, q, r, s))
            if b != "ab":
                assert p != q and r != s
                assert abs(two.value(b, (p, q, r, s)) + two.value(b, (q, p, r, s))) <= 2 * two.bound(b, (p, q, r, s))
    assert two.terms["aa"] or nup < 2
    assert not two.terms["bb"] or ndn >= 2
    assert R2.pattern(dets, NORB) == {b: set(two.terms[b]) for b in R2.BLOCKS}


def test_a_sample_gives_the_same_entries():
    rng = random.Random(5)
    dets = _all_dets(2, 2)
    c = _coeffs(rng, len(dets))
    full = R2.two_rdm(dets, c, NORB)
    sample = {b: set(rng.sample(sorted(full.terms[b]), 10)) | {(0, 0, 0, 0)} for b in R2.BLOCKS}
    part = R2.two_rdm(dets, c, NORB, sample)
    assert part.reached == full.reached == R2.pattern(dets, NORB)
    for b in R2.BLOCKS:
        assert set(part.terms[b]) == sample[b] & set(full.terms[b])
        for idx in part.terms[b]:
            assert part.terms[b][idx] == full.terms[b][idx]


def test_s_squared_of_hand_built_spin_states():
    p, q = 1 << 0, 1 << 2
    open_shell = [(p, q), (q, p)]                       # |p up, q dn>, |q up, p dn>
    assert R2.s_squared(open_shell, [1.0, 1.0], NORB) == 0.0           # the singlet, norm 2
    assert R2.s_squared(open_shell, [1.0, -1.0], NORB) == 4.0          # the Sz = 0 triplet, norm 2: 2 * 2
    assert R2.s_squared([(p | q, 0)], [1.0], NORB) == 2.0              # the Sz = 1 triplet
    assert R2.s_squared([(p, p)], [1.0], NORB) == 0.0                  # a closed shell
    assert R2.s_squared([(p, q)], [1.0], NORB) == 1.0                  # half singlet, half triplet


@pytest.mark.parametrize("nup,ndn", SECTORS)
def test_s_squared_from_the_ab_block(nup, ndn):
    """<S^2> = (Sz^2 + Sz + ndn) sum c^2 - sum_pq ab[q,p,p,q], against the direct evaluation"""
    rng = random.Random(11 * nup + ndn)
    dets = _all_dets(nup, ndn)
    c = _coeffs(rng, len(dets))
    two, n2 = R2.two_rdm(dets, c, NORB), R2.norm2(c)
    sz = 0.5 * (nup - ndn)
    ex = math.fsum(two.value("ab", (q, p, p, q)) for p in range(NORB) for q in range(NORB))
    got, want = (sz * sz + sz + ndn) * n2 - ex, R2.s_squared(dets, c, NORB)
    assert abs(got - want) <= R2.s_squared_bound(dets, c, NORB) + 2 * RC.U * abs(ex), (got, want)
