"""Self-test of tests/extrap_checker.py, the independent model of the energies for extrapolation.  No GPU, no library."""
import numpy as np
import pytest

import extrap_checker as EC
import linalg_checker as LC


@pytest.mark.parametrize("n", [0, 1, 2, 3, 10, 11, 23, 500])
def test_sort_is_a_permutation_with_non_increasing_magnitudes(n):
    rng = np.random.default_rng(n)
    for a in (rng.standard_normal(n), rng.choice([-1.0, 0.5, 1.0], n), np.full(n, -2.0)):
        s, o = EC.shell_sort_magnitude(a)
        assert sorted(o) == list(range(n))
        flip = -1.0 if n and s[0] != a[o[0]] else 1.0
        assert [flip * a[k] for k in o] == s
        assert all(abs(s[k]) >= abs(s[k + 1]) for k in range(n - 1))
        assert n == 0 or s[0] >= 0


def test_hand_worked_orders_with_ties():
    # n = 2: one gap of 1; equal magnitudes do not move, a negative leader flips the signs of all
    assert EC.shell_sort_magnitude([1.0, -1.0]) == ([1.0, -1.0], [0, 1])
    assert EC.shell_sort_magnitude([-1.0, 1.0]) == ([1.0, -1.0], [0, 1])
    assert EC.shell_sort_magnitude([0.5, -2.0]) == ([2.0, -0.5], [1, 0])
    # n = 3: gap 1 only, an insertion sort that stops at an equal magnitude
    assert EC.shell_sort_magnitude([1.0, 2.0, -2.0]) == ([2.0, -2.0, 1.0], [1, 2, 0])
    # n = 11: gaps 5, 2, 1.  All equal: nothing moves
    assert EC.shell_sort_magnitude([1.0] * 11)[1] == list(range(11))
    # the 2 at place 5 trades places with place 0 in the gap-5 pass, and place 0's 1 stays behind places 1..4: a stable sort
    # would give 5, 0, 1, 2, ...
    a = [1.0] * 11; a[5] = 2.0
    assert EC.shell_sort_magnitude(a)[1] == [5, 1, 2, 3, 4, 0, 6, 7, 8, 9, 10]
    # the 2 at the end walks down its gap-5 chain 10 -> 5 -> 0, pushing the 1s of places 5 and 0 up it
    a = [1.0] * 11; a[10] = -2.0
    s, o = EC.shell_sort_magnitude(a)
    assert o == [10, 1, 2, 3, 4, 0, 6, 7, 8, 9, 5] and s == [2.0] + [-1.0] * 10


def test_truncation_sizes():
    assert EC.truncations(10, 3) == [(3, 3), (6, 6), (9, 9), (10, 12)]
    assert EC.truncations(10, 5) == [(2, 2), (4, 4), (6, 6), (8, 8), (10, 10), (10, 12)]
    assert EC.truncations(10, 10) == [(k, k) for k in range(1, 11)] + [(10, 11)]
    assert EC.truncations(7, 1) == [(7, 7), (7, 14)]


def test_submatrix_is_the_dense_principal_block():
    for name, (c, i, v, _) in LC.generators().items():
        n = len(c)
        if n > 600:
            continue
        rng = np.random.default_rng(n)
        for sel in (np.arange(n), np.arange(0, n, 2), np.array([n - 1]), np.sort(rng.choice(n, max(1, n // 3), replace=False))):
            sc, si, sv = EC.submatrix(c, i, v, sel)
            assert np.array_equal(LC.dense(sc, si, sv), LC.dense(c, i, v)[np.ix_(sel, sel)]), name
            starts = np.concatenate(([0], np.cumsum(sc)))[:-1]
            assert np.array_equal(si[starts], np.arange(1, len(sel) + 1))              # diagonal first
            for r in range(len(sel)):
                cols = si[starts[r] + 1:starts[r] + sc[r]]
                assert np.all(np.diff(cols) > 0) and np.all(cols < r + 1)            # then j < i ascending


def test_edit_descriptors():
    assert EC._e(1e-4, 9, 2) == " 0.10E-03" and EC._e(2e-5, 9, 2) == " 0.20E-04" and EC._e(0.0, 9, 2) == " 0.00E+00"
    assert EC._e(9.96e-7, 9, 2) == " 0.10E-05" and EC._e(5e-7, 9, 2) == " 0.50E-06" and EC._e(1.0, 9, 2) == " 0.10E+01"
    assert EC._f(-75.5, 15, 9) == "  -75.500000000"
    r = dict(truncation=1, state=1, ndets_printed=12, ndets_pt=10, e_var=-75.5, pt_big=-0.25, pt_diff=0.0, pt_diff_std_dev=0.0, n_connected=345)
    lines = EC.format_records([r], 1e-4, 1e-6, True)
    assert lines[:6] == ["", EC.SORTING, "", EC.TO_DETS, EC.NO_MORE, ""]
    assert lines[6:9] == ["", "State   1:", "Variational energy(1)=" + " " * 13 + "  -75.500000000"]
    assert lines[9].index("-0.25") == 35 + 15 - len("-0.250000000") and lines[10].startswith("Total energy( 1)=")
    assert lines[11].endswith("(1)= 0.10E-03 0.10E-05       12        345   -75.500000000   -0.250000000   -0.250000000   -75.750000000")
    assert lines[12] == " ndets:           10 energy: -7.5500000000000000E+001" and len(lines) == 13
