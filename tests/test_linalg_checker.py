"""The linear-algebra checker (tests/linalg_checker.py) against dense numpy and LAPACK on small cases, and the oracle's serial
matvec inside the checker's derived bound on every generator.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import linalg_checker as LC


def test_storage_is_the_projects_format():
    c, i, v = LC.storage(4, {(0, 0): 1.0, (2, 0): 2.0, (1, 3): 3.0, (3, 3): 4.0, (3, 2): 5.0})
    assert c.tolist() == [1, 1, 2, 3]
    assert i.tolist() == [1, 2, 3, 1, 4, 2, 3]                     # diagonal first, then j < i ascending, 1-based
    assert v.tolist() == [1.0, 0.0, 0.0, 2.0, 4.0, 3.0, 5.0]
    A = LC.dense(c, i, v)
    assert np.array_equal(A, A.T) and A[0, 2] == 2.0 and A[1, 3] == 3.0 and A[2, 3] == 5.0
    assert np.array_equal(LC.diagonal_of(c, v), [1.0, 0.0, 0.0, 4.0])
    assert LC.norm1(c, i, v) == 12.0


@pytest.mark.parametrize("name", sorted(LC.generators()))
def test_exact_matvec_against_fractions(name):
    """the fsum-of-two-products matvec is the rational one rounded once; sum|a x| and the row lengths likewise"""
    c, i, v, x = LC.generators()[name]
    exact, sabs, length = LC.exact_matvec(c, i, v, x)
    r, cc, vv = LC.triplets(c, i, v)
    rng = np.random.default_rng(1)
    rows = sorted(set(rng.integers(0, len(c), 12).tolist()) | {0, len(c) - 1, int(np.argmax(length))})
    for row in rows:
        m = r == row
        terms = [Fraction(float(a)) * Fraction(float(x[j])) for a, j in zip(vv[m], cc[m])]
        assert length[row] == len(terms)
        assert exact[row] == float(sum(terms)), (name, row)
        assert sabs[row] == float(sum(abs(t) for t in terms)), (name, row)


def test_generators_have_the_shapes_they_promise():
    g = LC.generators()
    _, _, length = LC.exact_matvec(*g["row_length_ladder"])
    assert set(LC.LADDER) == set(length.tolist())
    c, i, v, x = g["cancellation_130"]
    exact, sabs, length = LC.exact_matvec(c, i, v, x)
    assert length[0] == 130 and exact[0] == 1.0 + 43.0 and sabs[0] > 8e17
    c, i, v, x = g["stored_zeros"]
    assert np.count_nonzero(v == 0.0) > 50 and np.any(np.signbit(v) & (v == 0.0)) and np.any(~np.signbit(v) & (v == 0.0))
    c, i, v, x = g["diagonal"]
    assert np.all(c == 1)
    A = LC.dense(*g["block_diagonal"][:3])
    assert np.all(A[:4, 4:] == 0.0) and np.all(A[:1, 1:] == 0.0)
    A = LC.dense(*g["banded"][:3])
    assert A[0, 70] != 0.0 and np.all(np.triu(A, 71) == 0.0)
    for n in LC.SIZES:
        assert len(LC.sized(n)[0]) == n


@pytest.mark.parametrize("name", sorted(LC.generators()))
def test_numpy_matvec_is_inside_the_bound_and_a_wrong_one_is_not(name):
    c, i, v, x = LC.generators()[name]
    exact, sabs, length = LC.exact_matvec(c, i, v, x)
    A = LC.dense(c, i, v)
    assert len(LC.matvec_violations(A @ x, exact, sabs, length)) == 0
    # one entry dropped from the longest row, where dropping it changes the sum at all: caught
    r, cc, vv = LC.triplets(c, i, v)
    row = int(np.argmax(length))
    cand = np.flatnonzero((r == row) & (vv * x[cc] != 0.0))
    k = cand[np.argmax(np.abs(vv[cand] * x[cc[cand]]))]
    y = exact.copy(); y[row] = exact[row] - vv[k] * x[cc[k]]
    assert LC.matvec_violations(y, exact, sabs, length).tolist() == [row]
    y = exact.copy(); y[-1] = np.nan
    assert LC.matvec_violations(y, exact, sabs, length).tolist() == [len(c) - 1]


def test_oracle_matvec_is_inside_the_bound_on_every_generator(oracle):
    cases = dict(LC.generators())
    for n in LC.SIZES:
        cases["sized_%d" % n] = LC.sized(n)
    for name, (c, i, v, x) in cases.items():
        exact, sabs, length = LC.exact_matvec(c, i, v, x)
        y = oracle.spmv_sym_upper(c, i, v, x)
        bad = LC.matvec_violations(y, exact, sabs, length)
        assert len(bad) == 0, (name, bad[:5], y[bad[:5]], exact[bad[:5]])


def test_bisections_against_lapack_at_200():
    n = 200
    d, b = LC.arrow_random(n, 5, coupling=1.5)
    c, i, v = LC.arrow(d, b)
    w, X = LC.eigh_dense(c, i, v)
    slack = LC.eigenvalue_slack(n, LC.norm1(c, i, v))
    lam = LC.arrow_lowest(d, b)
    assert abs(lam - w[0]) <= slack
    xv = LC.arrow_vector(d, b, lam)
    assert min(np.abs(xv - X[:, 0]).max(), np.abs(xv + X[:, 0]).max()) < 1e-12
    assert LC.residual(c, i, v, lam, xv) <= slack
    # a decoupled row below everything is not in row 0's sector: the secular root ignores it, LAPACK's lowest is that row
    d2, b2 = d.copy(), b.copy(); d2[7] = -50.0; b2[7] = 0.0
    w2 = np.linalg.eigvalsh(LC.dense(*LC.arrow(d2, b2)))
    slack2 = LC.eigenvalue_slack(n, LC.norm1(*LC.arrow(d2, b2)))
    assert abs(w2[0] + 50.0) <= slack2 and abs(LC.arrow_lowest(d2, b2) - w2[1]) <= slack2
    rng = np.random.default_rng(6)
    a, e = rng.standard_normal(n), rng.standard_normal(n - 1)
    c, i, v = LC.tridiagonal(a, e)
    A = LC.dense(c, i, v)
    assert np.array_equal(np.diag(A), a) and np.array_equal(np.diag(A, 1), e) and np.array_equal(A, A.T)
    w = np.linalg.eigvalsh(A)
    slack = LC.eigenvalue_slack(n, LC.norm1(c, i, v))
    for k in (0, 1, 57, n - 1):
        assert abs(LC.tridiagonal_eigenvalue(a, e, k) - w[k]) <= slack
    assert LC.sturm_count(a, e, w[10] + 1e-9) == 11
