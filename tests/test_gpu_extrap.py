"""Energies for extrapolation from truncated wavefunctions (energies_for_extrapolation, hci.f90:1824-2017) on the device:
sqmc_gpu_spmv_plan_submatrix at the seams of its 64-entry round and of its four-row block, its refusals and its scratch, device-built
plans against the plan of the subset itself, host.hci_extrapolation_energies and the deck, against tests/extrap_checker.py,
tests/linalg_checker.py and tests/hci_checker.py, none of which shares code with the library.  The reference runs this routine only
in an MPI build, so no reference output stands behind these tests (tests/golden/README_extrapolation.md)."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from conftest import FCIDUMP                                    # noqa: E402
import extrap_checker as EC                                     # noqa: E402
import linalg_checker as LC                                     # noqa: E402
from tests import hci_checker as HC                             # noqa: E402
from tests import proposal_checker as PC                        # noqa: E402

pytestmark = pytest.mark.gpu
ROWS_PER_BLOCK = 4                       # SPMV_ROWS_PER_BLOCK, csrc/spmv_kernels.h
OK, BAD_ARG, HIP, UNSUPPORTED = 0, -1, -2, -3
DECK = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_i_extrap")
SHIPPED = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_i_1sigma_g")
DAVIDSON_TOL = 1e-10                     # the eigenvalue criterion of hci_variational and of hci_extrapolation_energies


@pytest.fixture(scope="module", autouse=True)
def dev():
    import sqmc_amd
    sqmc_amd.set_device(0)


# ---------------------------------------------------------------------------------------------------- the door at its seams
_GEN = {}


def _matrix(name):
    if not _GEN:
        g = LC.generators()
        for k in ("random_sparse", "banded", "diagonal", "row_length_ladder"):
            _GEN[k] = g[k][:3]
    return _GEN[name]


def _full_lengths(sto):
    r, _, _ = LC.triplets(*sto)
    return np.bincount(r, minlength=len(sto[0]))


def _hub(sto, length):
    """(row, its neighbours) of the ladder's hub whose full row has `length` entries"""
    r, c, _ = LC.triplets(*sto)
    rows = np.flatnonzero(_full_lengths(sto) == length)
    assert len(rows) == 1
    h = int(rows[0])
    return h, np.sort(c[(r == h) & (c != h)])


def _selections():
    out = []
    rng = np.random.default_rng(7)
    for name in ("random_sparse", "banded", "diagonal", "row_length_ladder"):
        n = len(_matrix(name)[0])
        out += [(name, "first row", [0]), (name, "last row", [n - 1]), (name, "all rows", np.arange(n)), (name, "every other row", np.arange(0, n, 2))]
    n = len(_matrix("random_sparse")[0])
    for k in (1, 16):
        for m in (ROWS_PER_BLOCK * k - 1, ROWS_PER_BLOCK * k, ROWS_PER_BLOCK * k + 1):          # a partly filled last block
            out.append(("random_sparse", "m = %d" % m, np.sort(rng.choice(n, m, replace=False))))
    # banded, bandwidth 70: row 100 keeps its diagonal and entries of its transposed part only (no row of 30 .. 99 is selected)
    out.append(("banded", "transposed part only", np.concatenate(([3, 17], np.arange(100, 171), [250, 299]))))
    # ... and row 200 only entries of its stored part; row 5 and row 290 only their diagonals
    out.append(("banded", "stored part only, diagonals only", np.concatenate(([5], np.arange(130, 201), [290]))))
    lad = _matrix("row_length_ladder")
    hubs = {L: _hub(lad, L) for L in LC.LADDER if L > 2}
    # every hub but the longest with all its leaves: rows that keep exactly 63, 64, 65, 127, 128, 129 entries, all of them; the
    # 4097-entry row keeps its diagonal alone
    whole = np.concatenate([np.concatenate(([h], lv)) for L, (h, lv) in hubs.items() if L != 4097] + [[hubs[4097][0]]])
    out.append(("row_length_ladder", "whole hubs, 4097 -> 1", np.sort(whole)))
    h, leaves = hubs[4097]
    for keep in (2, 63, 64, 65, 127, 128, 129, 4096):          # the 4097-entry row keeps exactly `keep` entries scattered over its rounds
        lv = rng.choice(leaves, keep - 1, replace=False)
        out.append(("row_length_ladder", "4097 -> %d" % keep, np.sort(np.concatenate(([h], lv)))))
    return out


SELECTIONS = _selections()


@pytest.mark.parametrize("case", SELECTIONS, ids=lambda c: "%s: %s" % (c[0], c[1]))
def test_submatrix_is_the_plan_of_the_subset(case):
    import sqmc_amd
    name, tag, sel = case
    sel = np.asarray(sel, np.int64)
    c, i, v = _matrix(name)
    m = len(sel)
    sc, si, sv = EC.submatrix(c, i, v, sel)
    kept = _full_lengths((sc, si, sv))
    if "->" in tag:                                               # the seam this selection is there for is really in it
        want = int(tag.split("->")[1])
        assert want in kept.tolist(), (tag, sorted(set(kept.tolist()))[-5:])
    if "diagonals only" in tag or tag.endswith("4097 -> 1"):
        assert 1 in kept.tolist()
    if tag == "transposed part only":
        k = int(np.flatnonzero(sel == 100)[0])
        assert sc[k] == 1 and kept[k] == 71                       # nothing of its stored part but the diagonal, 70 transposed entries
    src = sqmc_amd.SpmvPlan(c, i, v)
    ref = sqmc_amd.SpmvPlan(sc, si, sv)
    sub = None
    try:
        x_src = np.random.default_rng(1).standard_normal(len(c))
        before = src.apply(x_src)
        sub = src.submatrix(sel)
        assert sub.n == m and sub.nnz_full == 2 * len(sv) - m
        for seed in (11, 12, 13):
            x = np.random.default_rng(seed).standard_normal(m)
            y = sub.apply(x)
            assert y.tobytes() == ref.apply(x).tobytes(), (name, tag, seed)
            exact, sabs, length = LC.exact_matvec(sc, si, sv, x)
            bad = LC.matvec_violations(y, exact, sabs, length)
            assert len(bad) == 0, (name, tag, bad[:5])
        assert src.apply(x_src).tobytes() == before.tobytes()     # the source is as it was
        if m == len(c):
            assert sub.apply(x_src).tobytes() == before.tobytes()
        again = src.submatrix(sel)                                # run after run the same plan
        try:
            assert again.nnz_full == sub.nnz_full and again.apply(x).tobytes() == y.tobytes()
        finally:
            again.close()
    finally:
        for p in (src, ref, sub):
            if p is not None:
                p.close()


# -------------------------------------------------------------------------------------------------------------- refusals
def _lib():
    import sqmc_amd
    L = sqmc_amd.load_library()
    V, i64 = C.c_void_p, C.c_int64
    L.sqmc_gpu_spmv_plan_submatrix.argtypes = [V, i64, V, V, V]
    L.sqmc_gpu_debug_scratch.argtypes = [V, V, V, V, C.c_int]
    L.sqmc_gpu_debug_scratch_fail_at.argtypes = [i64]
    return L


def _scratch(L):
    a = [C.c_int64() for _ in range(4)]
    assert L.sqmc_gpu_debug_scratch(*[C.byref(x) for x in a], 0) == OK
    return dict(zip(("live_allocs", "live_bytes", "peak_bytes", "n_takes"), (x.value for x in a)))


SENTINEL_H, SENTINEL_NNZ = 0x5A5A5A5A, -777


def _raw_call(L, src, m, sel, null=None):
    """the door through ctypes with recognisable words in both outputs; sel 1-based.  Returns (status, dst word, nnz word)"""
    s = np.ascontiguousarray(sel, np.int64)
    h, nnz = C.c_void_p(SENTINEL_H), C.c_int64(SENTINEL_NNZ)
    args = [src.h, m, s.ctypes.data_as(C.c_void_p), C.byref(h), C.byref(nnz)]
    if null is not None:
        args[null] = None
    st = L.sqmc_gpu_spmv_plan_submatrix(*args)
    return st, h.value, nnz.value


def test_refusals_leave_the_source_and_the_outputs_alone():
    import sqmc_amd
    L = _lib()
    c, i, v = _matrix("random_sparse")
    n = len(c)
    x = np.random.default_rng(5).standard_normal(n)
    src = sqmc_amd.SpmvPlan(c, i, v)
    try:
        before = src.apply(x)
        base = _scratch(L)
        good = np.arange(1, n + 1, 3, dtype=np.int64)
        m = len(good)
        swap_mid = good.copy(); swap_mid[[m // 2, m // 2 + 1]] = swap_mid[[m // 2 + 1, m // 2]]
        swap_end = good.copy(); swap_end[[m - 2, m - 1]] = swap_end[[m - 1, m - 2]]
        repeat = good.copy(); repeat[m // 3] = repeat[m // 3 - 1]
        low = good.copy(); low[0] = 0
        high = good.copy(); high[-1] = n + 1
        far = good.copy(); far[m // 2] = 2 ** 40
        neg = good.copy(); neg[0] = -5
        cases = [("null src", m, good, 0), ("null sel", m, good, 2), ("null dst", m, good, 3), ("null count", m, good, 4),
                 ("m = 0", 0, good, None), ("m = -1", -1, good, None), ("m = n + 1", n + 1, np.arange(1, n + 2), None),
                 ("row 0", m, low, None), ("row n + 1", m, high, None), ("row 2^40", m, far, None), ("row -5", m, neg, None),
                 ("a repeat", m, repeat, None), ("one swap in the middle", m, swap_mid, None), ("one swap at the end", m, swap_end, None)]
        for tag, mm, sel, null in cases:
            st, h, nnz = _raw_call(L, src, mm, sel, null)
            assert st == BAD_ARG, (tag, st)
            assert h == SENTINEL_H and nnz == SENTINEL_NNZ, tag
            now = _scratch(L)
            assert now["live_allocs"] == base["live_allocs"] and now["live_bytes"] == base["live_bytes"], tag
            assert src.apply(x).tobytes() == before.tobytes(), tag
        with pytest.raises(sqmc_amd.SqmcGpuError) as e:            # the wrapper: numpy's 0-based rows
            src.submatrix([0, 2, 2, 5])
        assert e.value.code == BAD_ARG and "ascending" in str(e.value)
        with pytest.raises(sqmc_amd.SqmcGpuError):
            src.submatrix([0, n])
        with pytest.raises(sqmc_amd.SqmcGpuError):
            src.submatrix([])
        # the measurement-only layout: switched on for the call, and a source plan that carries the stored triangle
        os.environ["SQMC_SPMV_UPPER_ATOMIC"] = "1"
        try:
            st, h, nnz = _raw_call(L, src, m, good)
            assert st == UNSUPPORTED and h == SENTINEL_H and nnz == SENTINEL_NNZ
            tri = sqmc_amd.SpmvPlan(c, i, v)
        finally:
            del os.environ["SQMC_SPMV_UPPER_ATOMIC"]
        try:
            st, h, nnz = _raw_call(L, tri, m, good)
            assert st == UNSUPPORTED and h == SENTINEL_H and nnz == SENTINEL_NNZ
        finally:
            tri.close()
        now = _scratch(L)
        assert now["live_allocs"] == base["live_allocs"] and now["live_bytes"] == base["live_bytes"]
        assert src.apply(x).tobytes() == before.tobytes()
        sub = src.submatrix(good - 1)                             # and an ordinary call afterwards
        try:
            ref = sqmc_amd.SpmvPlan(*EC.submatrix(c, i, v, good - 1))
            xs = x[:m]
            assert sub.apply(xs).tobytes() == ref.apply(xs).tobytes()
            ref.close()
        finally:
            sub.close()
        now = _scratch(L)
        assert now["live_allocs"] == base["live_allocs"] and now["live_bytes"] == base["live_bytes"]
    finally:
        src.close()


def test_every_failing_allocation_leaks_nothing():
    import sqmc_amd
    L = _lib()
    c, i, v = _matrix("banded")
    n = len(c)
    x = np.random.default_rng(6).standard_normal(n)
    src = sqmc_amd.SpmvPlan(c, i, v)
    try:
        before = src.apply(x)
        base = _scratch(L)
        sel = np.arange(1, n + 1, 2, dtype=np.int64)
        st, h, nnz = _raw_call(L, src, len(sel), sel)
        assert st == OK and h not in (None, SENTINEL_H) and nnz > 0
        takes = _scratch(L)["n_takes"] - base["n_takes"]
        held = _scratch(L)["live_allocs"] - base["live_allocs"]
        assert takes >= 8 and held == 5                           # per-call scratch and the five arrays the new plan keeps
        L.sqmc_gpu_spmv_free.argtypes = [C.c_void_p]
        assert L.sqmc_gpu_spmv_free(C.c_void_p(h)) == OK
        assert _scratch(L)["live_allocs"] == base["live_allocs"]
        try:
            for k in range(1, takes + 1):
                assert L.sqmc_gpu_debug_scratch_fail_at(k) == OK
                st, h2, nnz2 = _raw_call(L, src, len(sel), sel)
                assert st == HIP, (k, st)
                assert h2 == SENTINEL_H and nnz2 == SENTINEL_NNZ, k
                now = _scratch(L)
                assert now["live_allocs"] == base["live_allocs"] and now["live_bytes"] == base["live_bytes"], k
        finally:
            L.sqmc_gpu_debug_scratch_fail_at(0)
        assert src.apply(x).tobytes() == before.tobytes()
        sub = src.submatrix(sel - 1)
        try:
            assert sub.nnz_full == nnz
        finally:
            sub.close()
    finally:
        src.close()


# ------------------------------------------------------------------------------------------------------ device-built plans
class Wf:
    pass


def _wavefunction(time_sym, want, cap):
    """C2, i_1sigma_g conventions with time_sym on or off: two states on the first variational space of at least `want`
    determinants, cut to its `cap` leading ones (by state 1) and re-diagonalised there, in (up, dn) order"""
    from sqmc_amd import host as H
    import sqmc_amd
    w = Wf()
    w.h = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=bool(time_sym), z=1, hf_symmetry=1)
    w.g = w.h.gpu()
    w.g.set_hb_tables(*w.h.hb_tables(w.g))
    for eps in (2e-2, 1e-2, 5e-3, 3e-3, 2e-3, 1e-3):
        up, dn, wts, e, hist = H.hci_variational(w.h, w.g, eps, n_states=2, max_iters=2)
        if len(up) >= want:
            break
    assert len(up) >= want, hist
    lead = np.argsort(-np.abs(wts[:, 0]), kind="stable")[:cap]
    up, dn, wts = up[lead], dn[lead], wts[lead]
    o = H.sort_dets(up, dn)
    w.up, w.dn = np.ascontiguousarray(up[o]), np.ascontiguousarray(dn[o])
    plan, diag, _ = sqmc_amd.SpmvPlan.from_dets(w.g, w.up, w.dn)
    try:
        w.e, w.wts, _ = plan.davidson(diag, k=2, v0=wts[o], tol=DAVIDSON_TOL)
    finally:
        plan.close()
    w.eps, w.n = eps, len(w.up)
    w.checker = PC.ChemH(FCIDUMP, [w.h.orb_order[i] for i in range(1, w.h.norb + 1)])
    return w


@pytest.fixture(scope="module")
def wf_ts():
    w = _wavefunction(1, 600, 1500)
    yield w
    w.g.close()


@pytest.fixture(scope="module")
def wf_plain():
    w = _wavefunction(0, 600, 1500)
    yield w
    w.g.close()


@pytest.mark.parametrize("which", ["wf_ts", "wf_plain"])
def test_device_built_plans(request, which):
    import sqmc_amd
    w = request.getfixturevalue(which)
    n = w.n
    assert 600 <= n <= 1500
    rng = np.random.default_rng(21)
    full, diag, nnz = sqmc_amd.SpmvPlan.from_dets(w.g, w.up, w.dn)
    try:
        picks = [np.arange(0, n, 2), np.sort(rng.choice(n, n // 3, replace=False)), np.sort(rng.choice(n, 257, replace=False)), np.arange(n), np.array([n // 2])]
        for sel in picks:
            m = len(sel)
            sub = full.submatrix(sel)
            ref, dref, nref = sqmc_amd.SpmvPlan.from_dets(w.g, w.up[sel], w.dn[sel])
            try:
                assert np.array_equal(diag[sel], dref)
                assert (sub.nnz_full + m) % 2 == 0 and (sub.nnz_full + m) // 2 == nref
                for _ in range(3):
                    x = rng.standard_normal(m)
                    assert sub.apply(x).tobytes() == ref.apply(x).tobytes(), (which, m)
                if m >= 100:
                    v0 = 0.01 * rng.standard_normal((m, 2)); v0[0, 0] += 1.0; v0[1, 1] += 1.0
                    ea, xa, na = sub.davidson(diag[sel], k=2, v0=v0, tol=DAVIDSON_TOL)
                    eb, xb, nb = ref.davidson(dref, k=2, v0=v0, tol=DAVIDSON_TOL)
                    assert ea.tobytes() == eb.tobytes() and xa.tobytes() == xb.tobytes() and na == nb, (which, m)
            finally:
                sub.close(); ref.close()
    finally:
        full.close()


# ------------------------------------------------------------------------------------------- hci_extrapolation_energies
PHYSICS = ("truncation", "state", "ndets", "ndets_printed", "ndets_pt", "e_var", "pt_big", "pt_diff", "pt_diff_std_dev", "n_connected", "n_matvec")


def _same_records(a, b):
    assert len(a) == len(b)
    for ra, rb in zip(a, b):
        for k in PHYSICS:
            assert np.float64(ra[k]).tobytes() == np.float64(rb[k]).tobytes(), (ra["truncation"], ra["state"], k, ra[k], rb[k])
        if "coeffs" in ra:
            assert ra["coeffs"].tobytes() == rb["coeffs"].tobytes() and np.array_equal(ra["up"], rb["up"]) and np.array_equal(ra["dn"], rb["dn"])


def _check_order_and_sizes(w, wts, k, records, n_states):
    """the truncations are the checker's: sizes, printed counts, and the determinants of every one"""
    from sqmc_amd import host as H
    want_sorted, want_order = EC.shell_sort_magnitude(wts[:, 0])
    iorder, ws = H.extrapolation_order(wts)
    assert iorder.tolist() == want_order
    assert ws[:, 0].tobytes() == np.array(want_sorted).tobytes()
    for q in range(1, n_states):
        assert ws[:, q].tobytes() == np.ascontiguousarray(wts[want_order, q]).tobytes()      # the other states: permuted, nothing else
    sizes = EC.truncations(len(wts), k)
    assert [(r["ndets"], r["ndets_printed"]) for r in records if r["state"] == 1] == sizes
    assert [(r["truncation"], r["state"]) for r in records] == [(t, s) for t in range(1, k + 2) for s in range(1, n_states + 1)]
    for r in records:
        nt = r["ndets"]
        want = sorted(zip(w.up[want_order[:nt]].tolist(), w.dn[want_order[:nt]].tolist()))
        assert list(zip(r["up"].tolist(), r["dn"].tolist())) == want, (r["truncation"], r["state"])


def _reference_eigenvalue(eigs, q, e):
    """state 1 is the lowest eigenvalue.  A higher state is held against the eigenvalue nearest to it, which is what the residual
    theorem speaks of: the space may hold states of a symmetry the point group does not resolve (a Delta_g state of a linear molecule
    in D2h), which the start vectors do not contain and the iteration therefore never finds"""
    return eigs[0] if q == 0 else eigs[int(np.argmin(np.abs(eigs - e)))]


def _residual_bound_check(tag, sto, a1, ref_eigs, q, e, x):
    r = LC.residual(*sto, e, x)
    ref = _reference_eigenvalue(ref_eigs, q, e)
    assert abs(ref - e) <= r + LC.eigenvalue_slack(len(sto[0]), a1), (tag, q, e, ref, r)
    return r


@pytest.mark.parametrize("which", ["wf_ts", "wf_plain"])
def test_extrapolation_energies_reuse_against_rebuild(request, which):
    from sqmc_amd import host as H
    w = request.getfixturevalue(which)
    n = w.n
    k_uneven = next(k for k in (7, 9, 11, 13) if n % k)            # batch_size K /= ndets: the extra truncation is the only full one
    eps_pt = 1e-5
    for k in (4, k_uneven):
        a = H.hci_extrapolation_energies(w.h, w.g, w.up, w.dn, w.wts, k, w.eps, eps_pt, reuse_matrix=True, keep_vectors=True)
        b = H.hci_extrapolation_energies(w.h, w.g, w.up, w.dn, w.wts, k, w.eps, eps_pt, reuse_matrix=False, keep_vectors=True)
        _same_records(a, b)
        _check_order_and_sizes(w, w.wts, k, a, 2)
        for q in (1, 2):
            # interlacing.  The spaces are nested, so the exact eigenvalues do not rise; a Ritz value lies above the exact eigenvalue
            # it approximates and, by the residual theorem, within its residual of it: E(t + 1) <= E(t) + residual(t + 1)
            rs = [r for r in a if r["state"] == q]
            ev = [r["e_var"] for r in rs]
            if k == 4:
                for t in range(len(rs) - 1):
                    sto_t = w.g.build_sparse_ham(rs[t + 1]["up"], rs[t + 1]["dn"])
                    res = LC.residual(*sto_t, ev[t + 1], rs[t + 1]["coeffs"])
                    print("%s K=4 state %d truncation %d: E_var %.12f (before %.12f), residual %.3e" % (which, q, t + 2, ev[t + 1], ev[t], res))
                    assert ev[t + 1] <= ev[t] + res, (q, t, ev[t], ev[t + 1], res)
            assert all(r["pt_big"] < 0 and r["pt_diff_std_dev"] == 0.0 and r["n_connected"] > r["ndets_pt"] for r in a if r["state"] == q)
        if w.h.time_sym:
            assert all(r["ndets_pt"] >= r["ndets"] for r in a)
        else:
            assert all(r["ndets_pt"] == r["ndets"] for r in a)
    # the last truncation is the full space: LAPACK on the stored matrix, the residual theorem and LAPACK's own error
    sto = w.g.build_sparse_ham(w.up, w.dn)
    eigs = np.linalg.eigvalsh(LC.dense(*sto))
    a1 = LC.norm1(*sto)
    for q in (0, 1):
        last = [r for r in a if r["state"] == q + 1][-1]
        assert last["ndets"] == n
        r_last = _residual_bound_check(which + " last truncation", sto, a1, eigs, q, last["e_var"], last["coeffs"])
        r_full = _residual_bound_check(which + " full space", sto, a1, eigs, q, w.e[q], w.wts[:, q])
        print("%s state %d: E_var %.12f (full space %.12f), residuals %.2e / %.2e" % (which, q + 1, last["e_var"], w.e[q], r_last, r_full))


def test_extrapolation_order_with_ties_added_by_hand(wf_ts):
    from sqmc_amd import host as H
    w = wf_ts
    wts = w.wts.copy()
    by_mag = np.argsort(-np.abs(wts[:, 0]), kind="stable")
    # twelve determinants in the middle of the first truncation, around its end and at the tail get one magnitude each, signs mixed
    for lo, val in ((20, 0.03), (w.n // 5 - 6, 0.004), (w.n - 12, 1e-5)):
        grp = by_mag[lo:lo + 12]
        wts[grp, 0] = val * np.where(np.arange(12) % 3 == 1, -1.0, 1.0)
    k = 5
    stable = np.argsort(-np.abs(wts[:, 0]), kind="stable").tolist()
    order = EC.shell_sort_magnitude(wts[:, 0])[1]
    assert sorted(order) == sorted(stable) and order != stable                   # the ties fall differently than a stable sort leaves them
    a = H.hci_extrapolation_energies(w.h, w.g, w.up, w.dn, wts, k, w.eps, 1e-4, reuse_matrix=True, keep_vectors=True)
    _check_order_and_sizes(w, wts, k, a, 2)
    b = H.hci_extrapolation_energies(w.h, w.g, w.up, w.dn, wts, k, w.eps, 1e-4, reuse_matrix=False, keep_vectors=True)
    _same_records(a, b)
    for bad in (0, -1, w.n + 1):
        with pytest.raises(ValueError) as e:
            H.hci_extrapolation_energies(w.h, w.g, w.up, w.dn, wts, bad, w.eps, 1e-4)
        assert "n_energy_batch" in str(e.value)


def test_extrapolation_against_a_dense_solve_and_brute_force_pt(wf_ts):
    """the 150 leading combinations of the time-symmetric wavefunction: every truncation's E_var against LAPACK on the block of the
    independent checker's elements; and its 6 leading ones in batches of two: the first truncation's PT correction against the
    brute-force Epstein-Nesbet sum of hci_checker"""
    from sqmc_amd import host as H
    w = wf_ts
    ck, z = w.checker, w.h.z
    lead = np.sort(np.argsort(-np.abs(w.wts[:, 0]), kind="stable")[:150])
    up, dn, wts = w.up[lead], w.dn[lead], w.wts[lead]
    n = len(up)
    A = np.zeros((n, n))
    for i in range(n):
        for j in range(i + 1):
            A[i, j] = A[j, i] = ck.element_ts(int(up[i]), int(dn[i]), int(up[j]), int(dn[j]), z)[0]
    k = 4
    rec = H.hci_extrapolation_energies(w.h, w.g, up, dn, wts, k, w.eps, 1e-4, keep_vectors=True)
    order = EC.shell_sort_magnitude(wts[:, 0])[1]
    worst = 0.0
    for r in rec:
        members = np.sort(np.asarray(order[:r["ndets"]]))
        assert np.array_equal(up[members], r["up"]) and np.array_equal(dn[members], r["dn"])
        B = A[np.ix_(members, members)]
        sto = LC.storage_from_dense(B)
        eigs = np.linalg.eigvalsh(B)
        q = r["state"] - 1
        res = LC.residual(*sto, r["e_var"], r["coeffs"])
        bound = res + LC.eigenvalue_slack(len(members), LC.norm1(*sto))
        ref = _reference_eigenvalue(eigs, q, r["e_var"])
        assert abs(ref - r["e_var"]) <= bound, (r["truncation"], r["state"], r["e_var"], ref, res)
        worst = max(worst, abs(ref - r["e_var"]) / bound)
    print("dense: %d truncations x 2 states, worst |E_var - LAPACK| / bound = %.3g" % (k + 1, worst))
    # PT: one state, six combinations, batches of two
    lead = np.sort(np.argsort(-np.abs(w.wts[:, 0]), kind="stable")[:6])
    eps_pt = 2e-4
    rec = H.hci_extrapolation_energies(w.h, w.g, w.up[lead], w.dn[lead], w.wts[lead, :1], 3, w.eps, eps_pt, keep_vectors=True)
    first = rec[0]
    assert first["ndets"] == 2 and first["ndets_printed"] == 2 and rec[-1]["ndets_printed"] == 8 and rec[-1]["ndets"] == 6
    dets, co = [], []
    s = 1.0 / np.sqrt(2.0)
    for u, d, c in zip(first["up"].tolist(), first["dn"].tolist(), first["coeffs"].tolist()):      # back to determinants, by hand
        if u == d:
            dets.append((u, d)); co.append(c)
        else:
            dets += [(u, d), (d, u)]; co += [s * c, z * s * c]
    assert len(dets) == first["ndets_pt"] <= 64
    o = sorted(range(len(dets)), key=lambda t: dets[t])
    dets, co = [dets[t] for t in o], [co[t] for t in o]
    want, n_out, n_visited, bound, borderline = HC.pt2(ck, dets, co, first["e_var"], eps_pt, False, 1)
    assert not borderline
    print("PT of %d determinants: %.12f, checker %.12f, |delta| / bound = %.3g" % (len(dets), first["pt_big"], want, abs(first["pt_big"] - want) / bound))
    assert first["n_connected"] == n_visited
    assert abs(first["pt_big"] - want) <= bound, (first["pt_big"], want, bound)


# -------------------------------------------------------------------------------------------------------------- the deck
def _from_sorting(lines):
    at = lines.index(EC.SORTING)
    assert lines[at - 1] == ""
    return lines[at - 1:]


def test_deck_prints_the_reference_lines(monkeypatch):
    from sqmc_amd import run as R
    text = open(DECK).read()
    deck = R.parse_hci_deck(text)
    assert deck["n_energy_batch"] == 3 and deck["n_states"] == 2 and deck["time_sym"]
    buf = io.StringIO()
    res = R.run_hci(deck, FCIDUMP, out=buf)
    lines = buf.getvalue().split("\n")
    assert lines[-1] == ""
    lines = lines[:-1]
    rec = res["extrapolation"]
    n = res["ndets"]
    assert [(r["ndets"], r["ndets_printed"]) for r in rec if r["state"] == 1] == EC.truncations(n, 3)
    if n % 3:
        assert rec[-1]["ndets_printed"] > n                      # unclamped
    want = EC.format_records(rec, deck["eps_var"], deck["eps_pt"], True)
    got = _from_sorting(lines)
    assert got == want, [(a, b) for a, b in zip(got, want) if a != b][:3]
    assert got.count(EC.TO_DETS) == 4 and got.count(EC.NO_MORE) == 4 and got.count("State   1:") == 4 and got.count("State   2:") == 4
    txt = "\n".join(lines)
    assert "sqmc_amd: variational stage" not in txt and "Getting natural orbitals" not in txt and "states" not in res      # it stops there
    assert sum(l.startswith("eps_var, eps_pt, ndets,") for l in lines) == 8
    # --extrap-rebuild: the same text, and the command line hands the switch on
    buf = io.StringIO()
    res2 = R.run_hci(R.parse_hci_deck(text), FCIDUMP, out=buf, extrap_rebuild=True)
    assert buf.getvalue().split("\n")[:-1] == lines
    assert [tuple(r[k] for k in PHYSICS) for r in res2["extrapolation"]] == [tuple(r[k] for k in PHYSICS) for r in rec]
    # more batches than determinants: refused with the message, before any truncation
    buf = io.StringIO()
    with pytest.raises(SystemExit) as e:
        R.run_hci(R.parse_hci_deck(text.replace("n_energy_batch=3", "n_energy_batch=%d" % (n + 1))), FCIDUMP, out=buf)
    assert "n_energy_batch" in str(e.value) and "empty spaces" in str(e.value) and EC.SORTING not in buf.getvalue()
    monkeypatch.setattr(R, "run_hci", lambda deck, fcidump, **kw: kw)
    assert R.main(["-i", DECK, "--extrap-rebuild"])["extrap_rebuild"] is True and R.main(["-i", DECK])["extrap_rebuild"] is False


def test_deck_without_n_energy_batch_runs_as_before():
    """the shipped deck: no n_energy_batch, the ordinary PT block with the numbers of the reference's run"""
    from sqmc_amd import run as R
    deck = R.parse_hci_deck(open(SHIPPED).read())
    assert deck["n_energy_batch"] == 0
    buf = io.StringIO()
    res = R.run_hci(deck, FCIDUMP, out=buf, extrap_rebuild=True)           # the switch alone changes nothing
    txt = buf.getvalue()
    assert "extrapolation" not in res and EC.SORTING not in txt and res["ndets"] == 12776
    (e1, d1, n1), (e2, d2, n2) = res["states"]
    assert abs(e1 - (-75.719473642)) < 2e-9 and abs(d1 - (-0.008762133)) < 2e-8 and abs(e2 - (-75.631097209)) < 2e-9 and abs(e2 + d2 - (-75.638806440)) < 2e-8
    assert "Variational energy(1)=" in txt and "Variational energy(2)=" in txt
    assert "Total energy(1)=" in txt and "Total energy(2)=" in txt and "sqmc_amd: variational stage" in txt
    assert "Iteration   5 eps1=1.0E-3 ndets=    12776" in txt
    assert sum(l.startswith("eps_var, eps_pt, ndets,") for l in txt.split("\n")) == 2
