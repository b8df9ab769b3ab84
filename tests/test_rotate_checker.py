"""The independent model of the integral rotation (tests/rotate_checker.py) against properties that hold exactly."""
from fractions import Fraction

import numpy as np

import rotate_checker as RC


def _random_integrals(norb, seed, density=1.0):
    rng = np.random.default_rng(seed)
    P, Q, R, S = RC.canonical_keys(norb)
    vals = rng.uniform(-1.0, 1.0, len(P))
    vals[rng.uniform(size=len(P)) > density] = 0.0
    h = rng.uniform(-1.0, 1.0, (norb, norb))
    ints = RC.Integrals.from_arrays(norb, vals, h, -3.25)
    ints.two = {k: v for k, v in ints.two.items() if v != 0.0}
    return ints


def _signed_permutation(norb, seed):
    rng = np.random.default_rng(seed)
    perm, sign = rng.permutation(norb), rng.choice([-1.0, 1.0], norb)
    U = np.zeros((norb, norb))
    U[perm, np.arange(norb)] = sign                 # new orbital p = sign[p] * old orbital perm[p]
    return U, perm, sign


def test_canonical_keys_enumerate_every_class_once():
    for n in (1, 2, 3, 6):
        P, Q, R, S = RC.canonical_keys(n)
        keys = list(zip(P.tolist(), Q.tolist(), R.tolist(), S.tolist()))
        assert len(set(keys)) == len(keys) == (n * (n + 1) // 2) * (n * (n + 1) // 2 + 1) // 2
        assert all(k == RC.canon(*k) for k in keys) and [RC.key_position(k) for k in keys] == list(range(len(keys)))
        assert {RC.canon(p, q, r, s) for p in range(n) for q in range(n) for r in range(n) for s in range(n)} == set(keys)


def test_identity_returns_the_input():
    ints = _random_integrals(4, 1)
    for out in (RC.transform_exact(ints, np.eye(4)), RC.transform_sparse(ints, np.eye(4))):
        for k, v in ints.two.items():
            assert out.value(*k) == Fraction(v)
        for k, v in ints.one.items():
            assert out.one_value(*k) == Fraction(v)
        assert out.core == ints.core
    fast = RC.transform_fast(ints, np.eye(4))
    assert all(float(fast.value(*k)) == v for k, v in ints.two.items()) and all(float(fast.one_value(*k)) == v for k, v in ints.one.items())


def test_signed_permutation_relabels_with_the_sign_product():
    n = 5
    ints = _random_integrals(n, 2)
    U, perm, sign = _signed_permutation(n, 3)
    for out in (RC.transform_exact(ints, U), RC.transform_sparse(ints, U)):
        for p in range(n):
            for q in range(n):
                assert out.one_value(p, q) == Fraction(sign[p] * sign[q]) * Fraction(ints.h(perm[p], perm[q]))
                for r in range(n):
                    for s in range(n):
                        want = Fraction(sign[p] * sign[q] * sign[r] * sign[s]) * Fraction(ints.v(perm[p], perm[q], perm[r], perm[s]))
                        assert out.value(p, q, r, s) == want
    assert any(s < 0 for s in sign) and list(perm) != list(range(n))


def test_two_rotations_compose_exactly():
    n = 3
    rng = np.random.default_rng(4)
    ints = _random_integrals(n, 5)
    U1 = np.round(rng.uniform(-1, 1, (n, n)) * 64) / 64          # dyadic entries: the float product U1 U2 is exact
    U2 = np.round(rng.uniform(-1, 1, (n, n)) * 64) / 64
    step = RC.transform_exact(RC.transform_exact(ints, U1).integrals(), U2)
    once = RC.transform_exact(ints, U1 @ U2)
    P, Q, R, S = RC.canonical_keys(n)
    for k in zip(P.tolist(), Q.tolist(), R.tolist(), S.tolist()):
        assert step.value(*k) == once.value(*k)
    for p in range(n):
        for q in range(p + 1):
            assert step.one_value(p, q) == once.one_value(p, q)


def test_exact_and_fast_paths_agree_within_the_bound():
    n = 5
    rng = np.random.default_rng(6)
    ints = _random_integrals(n, 7)
    U = np.linalg.qr(rng.standard_normal((n, n)))[0]
    ex, fa = RC.transform_exact(ints, U), RC.transform_fast(ints, U)
    P, Q, R, S = RC.canonical_keys(n)
    worst = 0.0
    for k in zip(P.tolist(), Q.tolist(), R.tolist(), S.tolist()):
        b = ex.bound(*k)
        assert b > 0 and abs(fa.bound(*k) / fa.factor - b) <= 1e-12 * b          # S by Fractions' floats and by tensordot
        d = abs(Fraction(float(fa.value(*k))) - ex.value(*k))
        assert d <= b
        worst = max(worst, float(d) / b)
    for p in range(n):
        for q in range(p + 1):
            assert abs(Fraction(float(fa.one_value(p, q))) - ex.one_value(p, q)) <= ex.one_bound(p, q)
    print("exact vs fast, norb 5: worst |delta| / bound = %.3g" % worst)
    # the sparse path on the same dense problem is the same exact numbers
    sp = RC.transform_sparse(ints, U)
    assert all(sp.value(*k) == ex.value(*k) for k in zip(P.tolist(), Q.tolist(), R.tolist(), S.tolist()))


def test_output_keeps_the_eightfold_symmetry_exactly():
    """the full tensor sum_abcd U_aP U_bQ U_cR U_dS (ab|cd), formed here term by term for every index order, equals the canonical entry"""
    n = 3
    rng = np.random.default_rng(8)
    ints = _random_integrals(n, 9)
    U = rng.uniform(-1, 1, (n, n))
    ex = RC.transform_exact(ints, U)
    Uf = [[Fraction(x) for x in row] for row in U.tolist()]
    rg = range(n)
    for P in rg:
        for Q in rg:
            for R in rg:
                for S in rg:
                    full = sum((Uf[a][P] * Uf[b][Q] * Uf[c][R] * Uf[d][S] * Fraction(ints.v(a, b, c, d)) for a in rg for b in rg for c in rg for d in rg), Fraction(0))
                    for m in RC.class_members(P, Q, R, S):
                        assert ex.value(*m) == full


def test_compare_addresses_through_combine_2_and_flags_a_wrong_entry():
    n = 4
    ints = _random_integrals(n, 10, density=0.5)
    U, _, _ = _signed_permutation(n, 11)
    ex = RC.transform_sparse(ints, U)
    order = np.array([0, 3, 1, 4, 2])                                     # a scrambled pair numbering, as an energy-sorted orbital order gives
    c2 = np.zeros((n + 2, n + 2), np.int64)
    for i in range(1, n + 1):
        for j in range(1, n + 1):
            a, b = max(order[i], order[j]), min(order[i], order[j])
            c2[i, j] = a * (a - 1) // 2 + b
    c2[n + 1, n + 1] = (n + 1) * n // 2 + n + 1
    a2, a1, ac = RC.addresses(n, c2)
    size = ac + 1
    assert len(set(a2.tolist())) == len(a2) and RC.unaddressed(n, c2, size).sum() == size - len(a2) - n * (n + 1) // 2 - 1
    got = np.zeros(size)
    P, Q, R, S = RC.canonical_keys(n)
    for i, k in enumerate(zip(P.tolist(), Q.tolist(), R.tolist(), S.tolist())):
        got[a2[i]] = float(ex.value(*k))
    for p in range(n):
        for q in range(p + 1):
            got[a1[p, q]] = float(ex.one_value(p, q))
    got[ac] = ex.core
    assert RC.compare(ex, got, c2) == ([], 0.0)
    k = next(iter(ex.two))
    got[a2[RC.key_position(k)]] += 1e-9
    fails, _ = RC.compare(ex, got, c2)
    assert [f[0] for f in fails] == [k]
