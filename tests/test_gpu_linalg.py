"""The linear-algebra side every HCI run goes through -- sqmc_gpu_spmv_prepare / _apply / _sym_upper, sqmc_gpu_build_spmv_plan and
sqmc_gpu_davidson -- at the shapes where its kernels can go wrong, against tests/linalg_checker.py (an exact matvec and eigenvalue
references that share no code with the library or the oracle).

Matvec: every row of every case must lie within gamma_{L+1} sum|a x| of the exact sum (derived in linalg_checker; no row is left
out).  Davidson: orthonormality to (k+2) n 2^-52, the residual theorem against the independent eigenvalues, the state expected from
the start's sector, and a residual no larger than the oracle's on the same instance times one sweep's convergence factor, plus
the error with which doubles evaluate that residual at all (linalg_checker.residual_parts derives it; it is what lets a device whose
sums round differently from the oracle's pass where both stand at rounding level, and it is far under every unconverged residual).

DAVIDSON_TABLE, per well-posed case: the oracle's residual ||A x - e x|| of its worst state and the factor by which its last sweep
shrank the residual (the square root of the ratio of its last two eigenvalue moves: the eigenvalue error goes like the residual
squared), both measured with oracle.davidson_sparse on the CPU; and the device's residual from the MI355X run of this module."""
import ctypes as C
import math

import numpy as np
import pytest

import linalg_checker as LC

pytestmark = pytest.mark.gpu

# case: (oracle residual, oracle sweep factor, device residual on the MI355X)
DAVIDSON_TABLE = {
    "dense_n2_k1": (4.309e-16, 1, 1.570e-16),
    "dense_n2_k2": (8.882e-16, 1, 1.256e-15),
    "dense_n3_k1": (4.003e-16, 2.84, 4.578e-16),
    "dense_n5_k5": (8.130e-15, 1, 5.401e-15),
    "dense_n49_k1": (2.038e-06, 6.62, 2.038e-06),
    "dense_n50_k1": (4.135e-06, 4.74, 4.135e-06),
    "dense_n51_k1": (3.723e-06, 4.71, 3.723e-06),
    "dense_n70_k2": (1.108e-05, 6.41, 1.108e-05),
    "dense_n255_k1": (1.462e-05, 3.28, 1.462e-05),
    "dense_n257_k2": (1.785e-05, 4.71, 1.785e-05),
    "dense_n300_k3": (1.103e-05, 5.28, 1.103e-05),
    "dense_n1025_k2": (1.710e-05, 4.59, 1.710e-05),
    "arrow_n2000": (7.748e-16, 125, 2.379e-16),
    "arrow_n262145": (4.532e-15, 129, 8.200e-16),
    "arrow_n300001": (2.593e-15, 128, 7.048e-16),
    "start_near_eigenvector_k2_nearly_parallel": (7.917e-06, 6.34, 7.917e-06),
}


# ------------------------------------------------------------------------------------------------------------ Davidson cases
class Case:
    """one Davidson input.  ref(): the independent eigenvalues (ascending) the returned ones are matched against;
    expect: the index in ref() that state q must land on (the start's sector), or None where only membership is asked"""

    def __init__(self, name, sto, k, v0=None, ref=None, expect=None, reach=None):
        self.name, self.sto, self.k, self.v0, self._ref, self.expect, self.reach = name, sto, k, v0, ref, expect, reach
        self.n = len(sto[0])

    def ref(self):
        if self._ref is not None:
            return np.atleast_1d(self._ref())
        return LC.eigh_dense(*self.sto)[0]

    def diag(self):
        return LC.diagonal_of(self.sto[0], self.sto[2])


def _dense_case(n, k, seed=None):
    A = LC.random_symmetric(n, 100 * n + k if seed is None else seed)
    return Case("dense_n%d_k%d" % (n, k), LC.storage_from_dense(A), k, expect=list(range(k)))


def _arrow_case(n, seed):
    d, b = LC.arrow_random(n, seed)
    return Case("arrow_n%d" % n, LC.arrow(d, b), 1, ref=lambda: LC.arrow_lowest(d, b), expect=[0])


WELL_POSED_NK = ((2, 1), (2, 2), (3, 1), (5, 5), (49, 1), (50, 1), (51, 1), (70, 2), (255, 1), (257, 2), (300, 3), (1025, 2))


def well_posed_cases():
    out = [_dense_case(n, k) for n, k in WELL_POSED_NK]
    out.append(_arrow_case(2000, 11))
    out.append(_arrow_case(262145, 12))
    out.append(_arrow_case(300001, 13))
    A = LC.random_symmetric(60, 61)
    w, X = np.linalg.eigh(A)
    rng = np.random.default_rng(62)
    a = X[:, 0] + 1e-3 * rng.standard_normal(60)
    b = a + 1e-3 * rng.standard_normal(60)
    out.append(Case("start_near_eigenvector_k2_nearly_parallel", LC.storage_from_dense(A), 2, v0=np.stack([a, b], axis=1), expect=[0, 1]))
    return out


SMALL_A = LC.random_symmetric(12, 1212, dominance=0.0)        # every (n, k), n <= 12, on the leading blocks of one seeded matrix


def _small_case(n, k):
    return Case("small_n%d_k%d" % (n, k), LC.storage_from_dense(SMALL_A[:n, :n]), k, expect=list(range(k)))


def ill_posed_cases():
    """inputs on which the reference's iteration is undefined (a correction vector that is zero or rounding noise gets normalised,
    or the last basis vectors are never diagonalised).  reach: the rows of the invariant subspace the start vectors can reach."""
    out = []
    out.append(Case("diagonal_n5", LC.diagonal([1.0, 2.0, 3.0, 4.0, 5.0]), 1, expect=[0], reach=[0]))
    out.append(Case("diagonal_n300", LC.diagonal(1.0 + np.arange(300) * 0.25), 1, expect=[0], reach=[0]))
    # a 3x3 block decoupled from the other 97 rows; the start is its middle row
    rng = np.random.default_rng(3100)
    B = rng.standard_normal((3, 3)); B = B + B.T
    R = LC.random_symmetric(97, 3197, dominance=0.0) - 8.0 * np.eye(97)         # the rest lies lower: the global minimum is elsewhere
    A = np.zeros((100, 100)); A[40:43, 40:43] = B
    rest = [i for i in range(100) if not 40 <= i < 43]
    A[np.ix_(rest, rest)] = R
    v0 = np.zeros((100, 1)); v0[41, 0] = 1.0
    out.append(Case("start_inside_3x3_block_of_100", LC.storage_from_dense(A), 1, v0=v0, expect=None, reach=[40, 41, 42]))
    A = LC.random_symmetric(5, 54, dominance=0.0)
    out.append(Case("n5_k4_niter_not_a_multiple", LC.storage_from_dense(A), 4, expect=[0, 1, 2, 3]))
    # rows 0 and 1 degenerate, each weakly coupled to one other row
    ent = {(i, i): 1.0 + 0.5 * i for i in range(8)}
    ent[(1, 1)] = 1.0; ent[(0, 5)] = 0.04; ent[(1, 6)] = 0.05
    out.append(Case("two_degenerate_starts_weakly_coupled", LC.storage(8, ent), 2, expect=None, reach=[0, 5, 1, 6]))
    # an exact LAPACK eigenvector as the start: the correction is rounding noise at once (the oracle returns 4.20 for 5.96, the
    # lower Ritz value of the start and a unit vector of noise), so the case stands here and not among the well-posed ones
    A = LC.random_symmetric(60, 61)
    out.append(Case("start_is_eigenvector_3_of_60", LC.storage_from_dense(A), 1, v0=np.linalg.eigh(A)[1][:, 3:4].copy(), expect=[3]))
    for n in range(1, 13):
        for k in range(1, n + 1):
            out.append(_small_case(n, k))
    return out


def reachable_eigenvalues(case):
    """eigenvalues of the matrix restricted to the invariant subspace the start vectors reach"""
    if case.reach is None:
        return case.ref()
    A = LC.dense(*case.sto)
    rows = np.array(case.reach)
    rest = np.setdiff1d(np.arange(case.n), rows)
    assert np.all(A[np.ix_(rows, rest)] == 0.0)
    return np.linalg.eigvalsh(A[np.ix_(rows, rows)])


def oracle_measure(oracle, case):
    """(eigenvalues, vectors, residual of the worst state, sweep factor) of oracle.davidson_sparse on this instance"""
    tr = []
    w, X = oracle.davidson_sparse(*case.sto, case.k, initial_vectors=case.v0, trace=tr)
    r = max(LC.residual(*case.sto, w[q], X[:, q]) for q in range(case.k))
    mv = [float(np.max(np.abs(tr[j] - tr[j - 1]))) for j in range(1, len(tr))]
    f = math.sqrt(mv[-2] / mv[-1]) if len(mv) >= 2 and mv[-1] > 0 and mv[-2] > mv[-1] else 1.0
    return w, X, r, f


def check_eigenpairs(case, ev, X, ref, expect):
    """the assertions of a solved case, each against the independent reference; returns over the states the worst residual, the
    largest evaluation floor of a residual, and the largest residual the library's documented test lets through,
    sqrt(2e-12 (|A x|^2 + max diag^2)) (include/sqmc_gpu.h)"""
    n, k = case.n, case.k
    a1 = LC.norm1(*case.sto)
    assert np.all(np.isfinite(ev)) and np.all(np.isfinite(X))
    G = X.T @ X
    assert np.abs(G - np.eye(k)).max() <= (k + 2) * n * 2.0 ** -52, np.abs(G - np.eye(k)).max()
    worst = floor = documented = 0.0
    dmax = float(np.abs(case.diag()).max())
    for q in range(k):
        r, fl, h = LC.residual_parts(*case.sto, ev[q], X[:, q])
        worst, floor, documented = max(worst, r), max(floor, fl), max(documented, math.sqrt(2e-12 * (h * h + dmax * dmax)))
        j = int(np.argmin(np.abs(ref - ev[q])))
        assert abs(ref[j] - ev[q]) <= r + LC.eigenvalue_slack(n, a1), (case.name, q, ev[q], ref[j], r)
        if expect is not None:
            assert j == expect[q], (case.name, q, j, expect[q], ev[q], ref[:k + 2])
    return worst, floor, documented


# ---------------------------------------------------------------------------------------------------------------- matvec
def _matvec_cases():
    out = dict(LC.generators())
    for n in LC.SIZES:
        out["sized_%d" % n] = LC.sized(n)
    return out


MATVEC_NAMES = sorted(LC.generators()) + ["sized_%d" % n for n in LC.SIZES]


def _assert_inside_bound(tag, y, sto, x):
    exact, sabs, length = LC.exact_matvec(*sto, x)
    bad = LC.matvec_violations(y, exact, sabs, length)           # every row
    worst = float(np.max(np.abs(y - exact) / np.maximum(LC.matvec_bound(sabs, length), 1e-300)))
    print("%s: n=%d longest row %d, worst |y - exact| / bound = %.3g" % (tag, len(sto[0]), length.max(), worst))
    assert len(bad) == 0, (tag, bad[:5], y[bad[:5]], exact[bad[:5]])


def _sym_upper(sto, x):
    import sqmc_amd
    L = sqmc_amd.load_library()
    c, i, v = np.ascontiguousarray(sto[0], np.int64), np.ascontiguousarray(sto[1], np.int64), np.ascontiguousarray(sto[2], np.float64)
    x = np.ascontiguousarray(x, np.float64); y = np.zeros(len(c))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    st = L.sqmc_gpu_spmv_sym_upper(len(c), p(c), p(i), p(v), p(x), p(y))
    return st, y


@pytest.mark.parametrize("name", MATVEC_NAMES)
def test_matvec_inside_the_derived_bound(name):
    import sqmc_amd
    c, i, v, x = _matvec_cases()[name]
    plan = sqmc_amd.SpmvPlan(c, i, v)
    try:
        y = plan.apply(x)
        _assert_inside_bound(name, y, (c, i, v), x)
        assert np.array_equal(y, plan.apply(x), equal_nan=True)              # a repeated apply: identical bits
        st, y2 = _sym_upper((c, i, v), x)
        assert st == 0 and y2.tobytes() == y.tobytes()                       # the one-call door: the same bits
        # a non-finite x_j reaches exactly the rows that hold column j
        r, cc, _ = LC.triplets(c, i, v)
        for j, bad in ((0, np.nan), (len(c) // 2, np.inf), (len(c) - 1, -np.inf)):
            xb = x.copy(); xb[j] = bad
            yb = plan.apply(xb)
            hit = np.zeros(len(c), bool); hit[r[cc == j]] = True
            assert not np.any(np.isfinite(yb[hit])), (name, j)
            assert yb[~hit].tobytes() == y[~hit].tobytes(), (name, j)
    finally:
        plan.close()


def test_matvec_one_wave_walks_a_300001_entry_row():
    import sqmc_amd
    n = 300001
    d, b = LC.arrow_random(n, 31, coupling=40.0)
    sto = LC.arrow(d, b)
    x = np.random.default_rng(32).standard_normal(n)
    plan = sqmc_amd.SpmvPlan(*sto)
    try:
        y = plan.apply(x)
        _assert_inside_bound("arrow_300001", y, sto, x)
        assert np.array_equal(y, plan.apply(x))
    finally:
        plan.close()


def test_matvec_refusals_leave_the_next_call_working():
    import sqmc_amd
    good = LC.sized(5)
    def works():
        plan = sqmc_amd.SpmvPlan(*good[:3])
        y = plan.apply(good[3]); plan.close()
        _assert_inside_bound("after a refusal", y, good[:3], good[3])
    c, i, v, x = good
    for tag, sto in (("n = 0", (c[:0], i[:0], v[:0])),):
        with pytest.raises(sqmc_amd.SqmcGpuError) as e:
            sqmc_amd.SpmvPlan(*sto)
        assert e.value.code == -1, tag
        works()
    L = sqmc_amd.load_library()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    h = C.c_void_p()
    assert L.sqmc_gpu_spmv_prepare(-3, p(c), p(i), p(v), C.byref(h)) == -1 and not h.value
    works()
    for tag, col in (("a column 0", 0), ("a column n + 1", 6)):
        ib = i.copy(); ib[len(ib) - 1] = col
        with pytest.raises(sqmc_amd.SqmcGpuError) as e:
            sqmc_amd.SpmvPlan(c, ib, v)
        assert e.value.code == -1 and "column" in str(e.value), tag
        st, _ = _sym_upper((c, ib, v), x)
        assert st == -1, tag
        works()


# ------------------------------------------------------------------------------------------------------- device-built plan
SCAN_TILE, RS_TILE = 2048, 1024          # csrc/scan_sort.h
PLAN_SIZES = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, SCAN_TILE + 1, 4095, 4096, 4097)


def _chem(time_sym):
    from conftest import FCIDUMP
    from sqmc_amd import host as H
    h = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=bool(time_sym), z=1, hf_symmetry=1)
    g = h.gpu()
    g.set_hb_tables(*h.hb_tables(g))
    return h, g


def _sorted(up, dn):
    up, dn = np.asarray(up, np.uint64), np.asarray(dn, np.uint64)
    o = np.lexsort((dn, up))
    return up[o], dn[o]


def _check_plan(tag, h, g, up, dn, checker, time_sym, rng):
    """the device-built plan of one determinant list: the same bits as the host-expanded plan of build_sparse_ham's triplets, both
    inside the derived bound of the exact matvec of those triplets, and 200 stored elements against the independent Hamiltonian"""
    import sqmc_amd
    import proposal_checker as PC
    n = len(up)
    counts, idx, val = g.build_sparse_ham(up, dn)
    assert len(counts) == n and np.all(counts >= 1)
    starts = np.concatenate(([0], np.cumsum(counts)))[:-1]
    assert np.array_equal(idx[starts], np.arange(1, n + 1))                       # diagonal first
    plan_a = sqmc_amd.SpmvPlan(counts, idx, val)
    plan_b, diag, nnz = sqmc_amd.SpmvPlan.from_dets(g, up, dn)
    try:
        assert nnz == len(val) and np.array_equal(diag, val[starts])
        for _ in range(2):
            x = rng.standard_normal(n)
            ya, yb = plan_a.apply(x), plan_b.apply(x)
            _assert_inside_bound(tag, yb, (counts, idx, val), x)
            assert np.array_equal(ya, yb), (tag, np.abs(ya - yb).max())      # the same entries in the same order in every row
            assert np.array_equal(yb, plan_b.apply(x))
    finally:
        plan_a.close(); plan_b.close()
    rows = np.repeat(np.arange(n), counts)
    for q in rng.choice(len(val), min(200, len(val)), replace=False):
        i, j = int(rows[q]), int(idx[q]) - 1
        a = (int(up[i]), int(dn[i]), int(up[j]), int(dn[j]))
        ref, nt, sa = checker.element_ts(*a, z=1) if time_sym else checker.element(*a)
        assert abs(val[q] - ref) <= PC.rounding_bound(nt, sa), (tag, i, j, val[q], ref)
    return len(val) - n


@pytest.mark.parametrize("time_sym", [0, 1])
def test_device_built_plan_at_edge_sizes(time_sym):
    import proposal_checker as PC
    from conftest import FCIDUMP
    h, g = _chem(time_sym)
    try:
        checker = PC.ChemH(FCIDUMP, [h.orb_order[i] for i in range(1, h.norb + 1)])
        rng = np.random.default_rng(40 + time_sym)
        # no connected pair: closed-shell determinants on disjoint orbital quadruples are mutual quadruple (or higher) excitations
        quad = [sum(1 << o for o in range(4 * q, 4 * q + 4)) for q in range(3)]
        for n in (1, 2, 3):
            up, dn = _sorted(quad[:n], quad[:n])
            assert _check_plan("disconnected_%d" % n, h, g, up, dn, checker, time_sym, rng) == 0          # n_strict = 0
        # the star: HF and its connections; HF's transposed row holds about n entries
        su, sd, _, _ = g.hci_connections([h.hf_up], [h.hf_dn], [1.0], 1e-6)
        su, sd = np.asarray(su, np.uint64), np.asarray(sd, np.uint64)
        is_hf = (su == np.uint64(h.hf_up)) & (sd == np.uint64(h.hf_dn))
        assert is_hf.sum() == 1 and len(su) > 513                # 696 with time_sym, more without
        others = np.flatnonzero(~is_hf)
        # sizes beyond the star drop out: with time_sym it has 696 determinants, so 1023 and 1025 are run without time_sym only, and
        # there 513 and the whole star are the two that cross the sort tile
        sizes = [m for m in (2, 3, 64, 513, 1023, 1025) if m < len(su)] + [len(su)]
        assert sum(m >= 513 for m in sizes) >= 2 and (time_sym or len(su) > 1025)
        for n in sizes:
            pick = np.concatenate((np.flatnonzero(is_hf), rng.choice(others, n - 1, replace=False)))
            up, dn = _sorted(su[pick], sd[pick])
            strict = _check_plan("star_%d" % n, h, g, up, dn, checker, time_sym, rng)
            assert strict >= (n - 1) // 2
            if n >= 513:
                assert n + strict > RS_TILE                      # n diagonals + at least n - 1 couplings to HF: the sort crosses its tile
        # random subsets of an HCI space
        for eps in (5e-3, 1e-3, 2e-4, 1e-5):                     # the first screening threshold that gives enough determinants
            cu, cd, _, _ = g.hci_connections(su, sd, np.full(len(su), 0.05), eps)
            if len(cu) > max(PLAN_SIZES):
                break
        cu, cd = np.asarray(cu, np.uint64), np.asarray(cd, np.uint64)
        assert len(cu) > max(PLAN_SIZES)
        for n in PLAN_SIZES:
            pick = rng.choice(len(cu), n, replace=False)
            up, dn = _sorted(cu[pick], cd[pick])
            _check_plan("subset_%d" % n, h, g, up, dn, checker, time_sym, rng)
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------------------------- Davidson
def _device(case):
    """(status, eigenvalues, vectors, matvecs, message)"""
    import sqmc_amd
    plan = sqmc_amd.SpmvPlan(*case.sto)
    try:
        try:
            ev, X, nmv = plan.davidson(case.diag(), k=case.k, v0=case.v0)
        except sqmc_amd.SqmcGpuError as e:
            return e.code, None, None, None, str(e)
        return 0, ev, X, nmv, ""
    finally:
        plan.close()


def _niter(case):
    return min(case.n, case.k * min(case.n, 50))


@pytest.mark.parametrize("case", well_posed_cases(), ids=lambda c: c.name)
def test_davidson_well_posed(case):
    r_oracle, factor, _ = DAVIDSON_TABLE[case.name]
    st, ev, X, nmv, msg = _device(case)
    assert st == 0, msg
    worst, floor, _ = check_eigenpairs(case, ev, X, case.ref(), case.expect)
    print("%s: device residual %.3e (oracle %.3e, sweep factor %.3g, evaluation floor %.3e), %d products" % (case.name, worst, r_oracle, factor, floor, nmv))
    assert worst <= factor * r_oracle + floor
    assert 0 < nmv <= 10 * _niter(case)
    st2, ev2, X2, nmv2, _ = _device(case)
    assert st2 == 0 and ev2.tobytes() == ev.tobytes() and X2.tobytes() == X.tobytes() and nmv2 == nmv


@pytest.mark.parametrize("case", ill_posed_cases(), ids=lambda c: c.name)
def test_davidson_where_the_reference_iteration_is_undefined(oracle, case):
    """Never SQMC_OK with a non-finite number or with an eigenvalue the start vectors cannot reach.  Where the oracle itself
    solves the instance the well-posed assertions apply with its residual measured here.  Where it does not there is no residual
    to measure against, and the residual theorem alone would let any vector with a large residual through: the residual must then
    be inside what the library documents for a result it returns from such an input, |A x - e x|^2 <= 2e-12 (|A x|^2 + max diag^2),
    evaluated here with the exact matvec (plus the floor of that evaluation)."""
    import warnings
    ref = reachable_eigenvalues(case)
    solved = None
    if case.n > 1:
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                w, Xo, r_oracle, factor = oracle_measure(oracle, case)
                check_eigenpairs(case, w, Xo, ref, case.expect)
            solved = (r_oracle, factor)
        except (AssertionError, np.linalg.LinAlgError):
            solved = None
    st, ev, X, nmv, msg = _device(case)
    print("%s: status %d %s %s, the oracle %s" % (case.name, st, "" if ev is None else np.array2string(ev, precision=12), msg,
                                                   "solves it (r = %.3e)" % solved[0] if solved else "does not solve it"))
    if st != 0:
        assert st == -4 and len(msg) > 20 and solved is None          # a refusal with a message, and only where the reference fails too
        return
    worst, floor, documented = check_eigenpairs(case, ev, X, ref, case.expect)
    print("%s: device residual %.3e, evaluation floor %.3e, documented %.3e" % (case.name, worst, floor, documented))
    if solved:
        assert worst <= solved[1] * solved[0] + floor
    else:
        assert worst <= documented + floor
    if case.reach is not None:
        out = np.setdiff1d(np.arange(case.n), case.reach)
        assert np.all(X[out, :] == 0.0)                               # no weight outside what the start can reach
    if case.n > 1:
        assert 0 < nmv <= 10 * _niter(case)
    st2, ev2, X2, _, _ = _device(case)
    assert st2 == 0 and ev2.tobytes() == ev.tobytes() and X2.tobytes() == X.tobytes()


# evals (float.hex) and products of sqmc_gpu_davidson on the C2 1000-row matrix for k = 1 and k = 2, recorded from the library as it
# was before the breakdown guard, on the MI355X: the guard must not move an iterate of a well-defined run
C2_PINNED = {1: (("-0x1.2ea6ca7954eebp+6",), 13), 2: (("-0x1.2ea6ca7954f55p+6", "-0x1.2dc6c10d64e18p+6"), 28)}


def test_davidson_c2_1000_rows_is_bit_for_bit_what_it_was(c2_setup):
    import sqmc_amd
    s = c2_setup
    counts, idx = s.prj_counts, s.prj_indices
    val = s.prj_values / (-s.tau)
    diag = LC.diagonal_of(counts, val)
    plan = sqmc_amd.SpmvPlan(counts, idx, val)
    try:
        for k, (hexes, products) in C2_PINNED.items():
            ev, X, nmv = plan.davidson(diag, k=k)
            print("k = %d: %s, %d products" % (k, [float(e).hex() for e in ev], nmv))
            assert tuple(float(e).hex() for e in ev) == hexes and nmv == products
    finally:
        plan.close()
