"""The doors' per-call device scratch through its owner (sqmc_amd/csrc/dev_scratch.h), seen from outside by the two debug doors
sqmc_gpu_debug_scratch (live allocations / bytes, peak bytes, takes so far) and sqmc_gpu_debug_scratch_fail_at (the nth take from
now fails on the host, without a hipMalloc call).  For every door: the live counters come back to where they were, after success,
after every refusal, and after a failure injected at each of its takes in turn; a failed call writes no output; a clean call after
all that returns the bytes of the first.  Nothing here runs the device out of memory: the injected failure is the only one."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V = C.c_void_p
OK, BAD_ARG, ERR_HIP = 0, -1, -2
TPB = 256                                   # threads of a door kernel's block (sqmc_gpu.hip)
SCAN_TILE, RS_TILE, RS_MAX_RADIX, RDM_CHUNK = 2048, 1024, 1024, 1024      # scan_sort.h, rdm_kernels.h
FILL = 0xA5


def _p(a):
    return a.ctypes.data_as(V)


def _bind(L):
    i64, i32, f64 = C.c_int64, C.c_int32, C.c_double
    L.sqmc_gpu_debug_scratch.argtypes = [V, V, V, V, C.c_int]
    L.sqmc_gpu_debug_scratch_fail_at.argtypes = [i64]
    L.sqmc_gpu_propose_heatbath_batch.argtypes = [V, i64, f64] + [V] * 7
    L.sqmc_gpu_propose_cauchy_schwarz_batch.argtypes = [V, i64, f64] + [V] * 7
    L.sqmc_gpu_build_spmv_plan.argtypes = [V, i64] + [V] * 5
    L.sqmc_gpu_davidson.argtypes = [V, V, i32, V, f64, V, V, V]
    L.sqmc_gpu_hci_connections_slice.argtypes = [V, i64, V, V, V, f64, C.c_int, i32, i32] + [V] * 5
    L.sqmc_gpu_hci_connections_record.argtypes = [V, i64, V, V, V, f64, C.c_int, i32, i32] + [V] * 7
    L.sqmc_gpu_diag_update_batch.argtypes = [V, i64, V, V, V, V, i32, V]
    L.sqmc_gpu_debug_bucket_boundaries.argtypes = [V, i64, V, i32] + [V] * 8
    L.sqmc_gpu_hci_pt2.argtypes = [V, i64, V, V, V, f64, f64, i32, V, V]
    L.sqmc_gpu_hci_set_diag_update.argtypes = [V, i32]
    L.sqmc_gpu_hci_1rdm.argtypes = [V, i64] + [V] * 5
    L.sqmc_gpu_hci_1rdm_pt.argtypes = [V, i64, V, V, V, f64, f64, i32, V, V]
    L.sqmc_gpu_hci_greens_function.argtypes = [V, i64, V, V, V, f64, i32, V, i32, V, V]
    L.sqmc_gpu_rotate_integrals.argtypes = [V, V, V]
    L.sqmc_gpu_hci_pt2_stochastic_prepare.argtypes = [V, i64, V, V, V, f64, f64, f64, i32, V]
    L.sqmc_gpu_hci_pt2_stochastic_sample.argtypes = [V, i64] + [V] * 4
    L.sqmc_gpu_hci_pt2_stochastic_stats.argtypes = [V] * 5
    L.sqmc_gpu_hci_pt2_stochastic_free.argtypes = [V]


def counters(L, reset_peak=False):
    """(live allocations, live bytes, peak bytes, takes so far)"""
    a = [C.c_int64() for _ in range(4)]
    assert L.sqmc_gpu_debug_scratch(*[C.byref(x) for x in a], 1 if reset_peak else 0) == OK
    return tuple(x.value for x in a)


class Outs:
    """the outputs of one raw call: arrays filled with a byte pattern, null pointers, scalars holding a sentinel"""

    def __init__(self, L):
        self.L, self.arrays, self.ptrs, self.scalars = L, [], [], []

    def arr(self, n, dtype):
        a = np.full(max(int(n), 1) * np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype)
        self.arrays.append(a)
        return a

    def ptr(self):
        q = V()
        self.ptrs.append(q)
        return q

    def scalar(self, ctype, also_zero=False):
        x = ctype(-7777)
        self.scalars.append((x, also_zero))
        return x

    def untouched(self):
        return (all(bool(np.all(a.view(np.uint8) == FILL)) for a in self.arrays) and all(q.value is None for q in self.ptrs)
                and all(x.value == -7777 or (z and x.value == 0) for x, z in self.scalars))

    def blob(self, lengths=()):
        """bytes of every array and scalar, then of what the pointers hold (lengths: (ctype, count) per pointer); frees the pointers"""
        parts = [a.tobytes() for a in self.arrays] + [bytes(x) for x, _ in self.scalars]
        for q, (ct, n) in zip(self.ptrs, lengths):
            assert q.value is not None
            parts.append(bytes(np.ctypeslib.as_array(C.cast(q, C.POINTER(ct)), shape=(max(n, 1),))[:n].tobytes()))
        for q in self.ptrs:
            if q.value is not None:
                self.L.sqmc_gpu_free(q)
        return b"".join(parts)


def finish(rc, o, lengths=()):
    """what a case returns: (status, bytes of the outputs) of a call that succeeded, (status, None) of one that wrote nothing"""
    if rc != OK:
        assert o.untouched(), "a failed call wrote an output"
        return rc, None
    return rc, o.blob(lengths)


def exercise(L, call, label):
    """balance of a clean call, then a failure at every one of its takes, then the first call's bytes again.  Returns its takes."""
    base = counters(L)
    rc, first = call()
    assert rc == OK and first is not None, (label, rc, L.sqmc_gpu_last_error())
    after = counters(L)
    assert after[:2] == base[:2], (label, "live after a clean call", base, after)
    n = after[3] - base[3]
    assert 1 <= n <= 200, (label, n)
    for k in range(1, n + 1):
        assert L.sqmc_gpu_debug_scratch_fail_at(k) == OK
        rc, res = call()
        L.sqmc_gpu_debug_scratch_fail_at(0)
        assert rc == ERR_HIP and res is None, (label, "take", k, "of", n, rc, L.sqmc_gpu_last_error())
        assert counters(L)[:2] == base[:2], (label, "live after a failure at take", k, base, counters(L))
    rc, again = call()
    assert rc == OK and again == first, (label, "the clean call after the failures differs")
    assert counters(L)[:2] == base[:2]
    print("%s: %d takes, every early return balanced" % (label, n))
    return n


class Sys:
    """one context with its determinant lists: lists[n] = (up, dn, coeffs) sorted by (up, dn), n = 1, 3, TPB + 1"""

    def __init__(self, name, host, g, chem):
        from sqmc_amd import host as H
        self.name, self.host, self.g, self.L, self.h, self.chem = name, host, g, g.L, g.h, chem
        seen = {(int(host.hf_up), int(host.hf_dn))}
        frontier = [(int(host.hf_up), int(host.hf_dn))]
        while len(seen) < TPB + 1:
            fu, fd = np.array([a for a, _ in frontier], np.uint64), np.array([b for _, b in frontier], np.uint64)
            cu, cd, _, _ = g.hci_connections(fu, fd, np.ones(len(fu)), 1e-9, diag_mode=0)
            new = sorted({(int(a), int(b)) for a, b in zip(cu, cd)} - seen)
            assert new, "the connected space ran out"
            seen.update(new); frontier = new
        dets = sorted(seen)
        hf = dets.index((int(host.hf_up), int(host.hf_dn)))
        lo = min(max(hf - 1, 0), len(dets) - (TPB + 1))
        dets = dets[lo:lo + TPB + 1]                 # a window of the sorted space that holds the HF determinant
        up, dn = np.array([a for a, _ in dets], np.uint64), np.array([b for _, b in dets], np.uint64)
        o = H.sort_dets(up, dn)
        up, dn = np.ascontiguousarray(up[o]), np.ascontiguousarray(dn[o])
        self.lists = {}
        for n in (1, 3, TPB + 1):
            c = np.array([(-1.0) ** i / (1.0 + i) for i in range(n)])
            self.lists[n] = (up[:n].copy(), dn[:n].copy(), np.ascontiguousarray(c / np.sqrt((c * c).sum())))
        hfu, hfd = np.array([host.hf_up], np.uint64), np.array([host.hf_dn], np.uint64)
        self.e_var = float(g.hamiltonian_batch(hfu, hfd, hfu, hfd)[0]) - 0.3      # below every diagonal element: no denominator near zero


@pytest.fixture(scope="module")
def chem():
    import sqmc_amd
    from conftest import FCIDUMP
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    h = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=False)
    g = h.gpu()
    _bind(g.L)
    g.set_hb_tables(*h.hb_tables(g))
    yield Sys("chem", h, g, True)
    g.close()


@pytest.fixture(scope="module")
def heg():
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    h = H.HegHost(3, 0.5, 14, 7, 1.49)      # 19 plane waves, indices within +-1
    g = h.gpu()
    _bind(g.L)
    yield Sys("heg", h, g, False)
    g.close()


@pytest.fixture(params=["chem", "heg"])
def sysm(request):
    return request.getfixturevalue(request.param)


# ------------------------------------------------------------------------------------------------ the raw calls
def connections(s, n, eps, mode, rec, slice=0, n_slices=1, coeffs=None):
    """one sqmc_gpu_hci_connections_slice / _record call; also returns the count through box[0]"""
    up, dn, co = s.lists[n]
    co = co if coeffs is None else coeffs
    box = [0]

    def call():
        o = Outs(s.L)
        cnt = o.scalar(C.c_int64, also_zero=True)
        ptrs = [o.ptr() for _ in range(6 if rec else 4)]
        fn = s.L.sqmc_gpu_hci_connections_record if rec else s.L.sqmc_gpu_hci_connections_slice
        rc = fn(s.h, n, _p(up), _p(dn), _p(co), eps, mode, slice, n_slices, C.byref(cnt), *[C.byref(q) for q in ptrs])
        k = cnt.value if rc == OK else 0
        box[0] = k
        if rc == OK and k == 0:
            assert all(q.value is None for q in ptrs), "zero connections came with an array"
            return rc, b"none"
        lens = [(C.c_uint64, k), (C.c_uint64, k), (C.c_double, k), (C.c_double, k)] + ([(C.c_double, k), (C.c_int32, 4 * k)] if rec else [])
        return finish(rc, o, lens)
    return call, box


def eps_for(s, n):
    return 1e-4 if n > 3 else 1e-6


@pytest.mark.parametrize("n", [1, 3, TPB + 1])
@pytest.mark.parametrize("rec", [False, True])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_hci_connections(sysm, n, rec, mode):
    call, box = connections(sysm, n, eps_for(sysm, n), mode, rec)
    takes = exercise(sysm.L, call, "%s hci_connections n=%d mode=%d rec=%d" % (sysm.name, n, mode, rec))
    assert box[0] > 0 and takes <= 40


def test_hci_connections_refusals_balance(sysm):
    L = sysm.L
    base = counters(L)[:2]
    for rec in (False, True):
        # no eps yields zero connections (a reference's own slot is always generated): an eps nothing else passes leaves those slots,
        # and the zero-connection return is reached by coefficients that are all zero
        call, box = connections(sysm, 3, 1e9, 0, rec)
        assert call()[0] == OK and box[0] == 3 and counters(L)[:2] == base
        for mode in (0, 1, 2):
            call, box = connections(sysm, 3, 1e-6, mode, rec, coeffs=np.zeros(3))
            assert call() == (OK, b"none") and box[0] == 0 and counters(L)[:2] == base
            assert exercise(L, call, "%s hci_connections, zero connections, mode %d rec %d" % (sysm.name, mode, rec)) == 7
    empty = None
    for sl in range(64):                                                # a slice of the rank range that comes out empty
        call, box = connections(sysm, 1, 1e-6, 0, False, slice=sl, n_slices=64)
        rc, res = call()
        assert rc == OK and counters(L)[:2] == base
        if box[0] == 0:
            empty = sl
    assert empty is not None
    call, _ = connections(sysm, 1, 1e-6, 0, False, slice=empty, n_slices=64)
    exercise(L, call, "%s hci_connections, empty slice %d of 64" % (sysm.name, empty))


def test_hamiltonian_and_proposal_batches(sysm):
    s, L = sysm, sysm.L
    up, dn, _ = s.lists[TPB + 1]
    n = len(up)
    ju, jd = np.ascontiguousarray(up[::-1]), np.ascontiguousarray(dn[::-1])

    def ham(fn):
        def call():
            o = Outs(L)
            h = o.arr(n, np.float64)
            return finish(fn(s.h, n, _p(up), _p(dn), _p(ju), _p(jd), _p(h)), o)
        return call
    assert exercise(L, ham(L.sqmc_gpu_hamiltonian_batch), s.name + " hamiltonian_batch") == 5
    if s.chem:
        assert exercise(L, ham(L.sqmc_gpu_hamiltonian_chem_batch), s.name + " hamiltonian_chem_batch") == 5
    seeds = np.ascontiguousarray((np.arange(4 * n, dtype=np.int64) * 2654435761 % 4096).astype(np.int32))

    def propose():
        o = Outs(L)
        a, b, w, sa = o.arr(n, np.uint64), o.arr(n, np.uint64), o.arr(n, np.float64), o.arr(4 * n, np.int32)
        return finish(L.sqmc_gpu_propose_batch(s.h, n, 0.01, _p(up), _p(dn), _p(seeds), _p(a), _p(b), _p(w), _p(sa)), o)
    assert exercise(L, propose, s.name + " propose_batch") == 7


def test_heatbath_and_cauchy_schwarz_proposal_batches(chem):
    from conftest import FCIDUMP
    from sqmc_amd import host as H
    n = TPB + 1
    seeds = np.ascontiguousarray((np.arange(4 * n, dtype=np.int64) * 2654435761 % 4096).astype(np.int32))
    for kind in ("heatbath", "cauchy"):
        # the efficient heat-bath tables are refused for the 8-electron system (as in the reference): 10 electrons there, walkers on its HF determinant
        h = H.ChemHost(FCIDUMP, 10, 5, "d2h") if kind == "heatbath" else H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=False)
        g = h.gpu(proposal="cauchyschwarz" if kind == "cauchy" else "uniform")
        up, dn = (np.full(n, h.hf_up, np.uint64), np.full(n, h.hf_dn, np.uint64)) if kind == "heatbath" else chem.lists[n][:2]
        try:
            if kind == "heatbath":
                assert g.setup_efficient_heatbath()
            width = 2 if kind == "heatbath" else 1
            fn = g.L.sqmc_gpu_propose_heatbath_batch if kind == "heatbath" else g.L.sqmc_gpu_propose_cauchy_schwarz_batch

            def call():
                o = Outs(g.L)
                a, b, w, sa = o.arr(width * n, np.uint64), o.arr(width * n, np.uint64), o.arr(width * n, np.float64), o.arr(4 * n, np.int32)
                return finish(fn(g.h, n, 0.01, _p(up), _p(dn), _p(seeds), _p(a), _p(b), _p(w), _p(sa)), o)
            assert exercise(g.L, call, "chem propose_%s_batch" % kind) == 7
        finally:
            g.close()


@pytest.mark.parametrize("n", [3, 63, 64, TPB + 1])
def test_build_sparse_ham_both_branches(chem, n):
    """n below 64: every pair tested; from 64 on: candidates from string groups (ham_rows_dev)"""
    s, L = chem, chem.L
    up, dn = s.lists[TPB + 1][0][:n].copy(), s.lists[TPB + 1][1][:n].copy()
    nnz_box = [0]

    def call():
        o = Outs(L)
        nnz = o.scalar(C.c_int64)
        prc, pix, pvl = o.ptr(), o.ptr(), o.ptr()
        rc = L.sqmc_gpu_build_sparse_ham(s.h, n, _p(up), _p(dn), C.byref(nnz), C.byref(prc), C.byref(pix), C.byref(pvl))
        k = nnz.value if rc == OK else 0
        nnz_box[0] = k
        return finish(rc, o, [(C.c_int64, n), (C.c_int64, k), (C.c_double, k)])
    exercise(L, call, "chem build_sparse_ham n=%d" % n)
    assert nnz_box[0] >= n


def test_build_sparse_ham_heg(heg):
    s, L = heg, heg.L
    up, dn, _ = s.lists[TPB + 1]
    n = len(up)

    def call():
        o = Outs(L)
        nnz = o.scalar(C.c_int64)
        prc, pix, pvl = o.ptr(), o.ptr(), o.ptr()
        rc = L.sqmc_gpu_build_sparse_ham(s.h, n, _p(up), _p(dn), C.byref(nnz), C.byref(prc), C.byref(pix), C.byref(pvl))
        k = nnz.value if rc == OK else 0
        return finish(rc, o, [(C.c_int64, n), (C.c_int64, k), (C.c_double, k)])
    exercise(L, call, "heg build_sparse_ham")


@pytest.mark.parametrize("n", [3, TPB + 1])
def test_spmv_plan_and_davidson(sysm, n):
    s, L = sysm, sysm.L
    up, dn = s.lists[TPB + 1][0][:n].copy(), s.lists[TPB + 1][1][:n].copy()
    k = 2 if n == 3 else 1                          # two states of the 3 x 3 matrix, the lowest of the larger one

    def call():
        o = Outs(L)
        plan, diag, nnz = o.ptr(), o.arr(n, np.float64), o.scalar(C.c_int64)
        rc = L.sqmc_gpu_build_spmv_plan(s.h, n, _p(up), _p(dn), C.byref(plan), _p(diag), C.byref(nnz))
        if rc != OK:
            return finish(rc, o)
        o.ptrs.remove(plan)                       # a plan, not an array: freed by its own door
        try:
            o2 = Outs(L)
            ev, vec, nmv = o2.arr(k, np.float64), o2.arr(k * n, np.float64), C.c_int32(-7777)
            rc = L.sqmc_gpu_davidson(plan, _p(diag), k, None, 1e-10, _p(ev), _p(vec), C.byref(nmv))
            if rc != OK:
                return finish(rc, o2)
            return rc, o.blob() + o2.blob() + bytes(nmv)
        finally:
            assert L.sqmc_gpu_spmv_free(plan) == OK
    takes = exercise(L, call, "%s build_spmv_plan + davidson n=%d" % (s.name, n))
    assert takes <= 60


def test_spmv_sym_upper(chem):
    s, L = chem, chem.L
    up, dn, _ = s.lists[TPB + 1]
    rc_, ix, vl = s.g.build_sparse_ham(up, dn)
    n = len(up)
    x = np.ascontiguousarray(np.cos(np.arange(n)))

    def call():
        o = Outs(L)
        y = o.arr(n, np.float64)
        return finish(L.sqmc_gpu_spmv_sym_upper(n, _p(rc_), _p(ix), _p(vl), _p(x), _p(y)), o)
    assert exercise(L, call, "spmv_sym_upper") == 5


def test_diag_update_batch(sysm):
    s, L = sysm, sysm.L
    up, dn, co = s.lists[3]
    cu, cd, _, _, old, pqrs = s.g.hci_connections_record(up, dn, co, 1e-6, diag_mode=2)
    dbl = np.flatnonzero(np.all(np.asarray(pqrs) > 0, axis=1))      # the double excitations: a reference's own slot and the singles carry no record
    cu, cd, old = np.ascontiguousarray(cu[dbl]), np.ascontiguousarray(cd[dbl]), np.ascontiguousarray(old[dbl])
    n = len(cu)
    assert n > TPB
    pq = np.ascontiguousarray(np.asarray(pqrs)[dbl], np.int32).reshape(-1)
    for form in (0, 1):
        def call():
            o = Outs(L)
            out = o.arr(n, np.float64)
            return finish(L.sqmc_gpu_diag_update_batch(s.h, n, _p(old), _p(pq), _p(cu), _p(cd), form, _p(out)), o)
        assert exercise(L, call, "%s diag_update_batch form %d" % (s.name, form)) == 6
    base = counters(L)[:2]
    bad = pq.copy(); bad[4 * (n // 2):4 * (n // 2) + 4] = 0                # a record that names no orbitals
    o = Outs(L)
    out = o.arr(n, np.float64)
    assert L.sqmc_gpu_diag_update_batch(s.h, n, _p(old), _p(bad), _p(cu), _p(cd), 0, _p(out)) == BAD_ARG
    assert o.untouched() and counters(L)[:2] == base


def test_debug_bucket_boundaries(chem):
    s, L = chem, chem.L
    B = 4
    keys = np.ascontiguousarray(np.sort((np.arange(1000, dtype=np.uint64) * 2654435761 % 100000).astype(np.uint32)))
    kb = np.array([0, 25000, 50000, 75000, 0xFFFFFFFF], np.uint32)
    sc = np.array([250, 250, 250, 250, 0], np.uint32)

    def call():
        o = Outs(L)
        pos, kbo, ho = o.arr(B + 1, np.uint32), o.arr(B, np.uint32), o.arr(B, np.uint32)
        return finish(L.sqmc_gpu_debug_bucket_boundaries(s.h, len(keys), _p(keys), B, _p(kb), None, None, None, _p(sc), _p(pos), _p(kbo), _p(ho)), o)
    assert exercise(L, call, "debug_bucket_boundaries") == 2


@pytest.mark.parametrize("du_mode", [0, 1])
@pytest.mark.parametrize("n,n_slices", [(1, 1), (3, 2), (TPB + 1, 2)])
def test_hci_pt2(sysm, n, n_slices, du_mode):
    s, L = sysm, sysm.L
    up, dn, co = s.lists[n]
    assert L.sqmc_gpu_hci_set_diag_update(s.h, du_mode) == OK
    try:
        def call():
            o = Outs(L)
            de, nc = o.scalar(C.c_double), o.scalar(C.c_int64)
            return finish(L.sqmc_gpu_hci_pt2(s.h, n, _p(up), _p(dn), _p(co), s.e_var, eps_for(s, n), n_slices, C.byref(de), C.byref(nc)), o)
        exercise(L, call, "%s hci_pt2 n=%d slices=%d du_mode=%d" % (s.name, n, n_slices, du_mode))
    finally:
        assert L.sqmc_gpu_hci_set_diag_update(s.h, 0) == OK


@pytest.mark.parametrize("n", [1, 3, TPB + 1])
def test_one_rdm_doors(sysm, n):
    s, L = sysm, sysm.L
    up, dn, co = s.lists[n]
    nn = s.g.norb * s.g.norb
    sym = np.ascontiguousarray(np.arange(s.g.norb) % 3, np.int32)
    for labels in (None, sym):
        def call():
            o = Outs(L)
            rdm = o.arr(nn, np.float64)
            return finish(L.sqmc_gpu_hci_1rdm(s.h, n, _p(up), _p(dn), _p(co), None if labels is None else _p(labels), _p(rdm)), o)
        exercise(L, call, "%s hci_1rdm n=%d labels=%s" % (s.name, n, labels is not None))

    def call_pt():
        o = Outs(L)
        rdm, nc = o.arr(nn, np.float64), o.scalar(C.c_int64)
        return finish(L.sqmc_gpu_hci_1rdm_pt(s.h, n, _p(up), _p(dn), _p(co), s.e_var, eps_for(s, n), 2, _p(rdm), C.byref(nc)), o)
    exercise(L, call_pt, "%s hci_1rdm_pt n=%d, 2 slices" % (s.name, n))


def test_one_rdm_repeated_determinant_balances(sysm):
    s, L = sysm, sysm.L
    up, dn, co = s.lists[3]
    up2, dn2 = up.copy(), dn.copy()
    up2[2], dn2[2] = up2[0], dn2[0]
    nn = s.g.norb * s.g.norb
    base = counters(L)[:2]
    o = Outs(L)
    rdm, nc = o.arr(nn, np.float64), o.scalar(C.c_int64)
    assert L.sqmc_gpu_hci_1rdm(s.h, 3, _p(up2), _p(dn2), _p(co), None, _p(rdm)) == BAD_ARG
    assert b"appears twice" in L.sqmc_gpu_last_error() and o.untouched() and counters(L)[:2] == base
    assert L.sqmc_gpu_hci_1rdm_pt(s.h, 3, _p(up2), _p(dn2), _p(co), s.e_var, 1e-6, 2, _p(rdm), C.byref(nc)) == BAD_ARG
    assert o.untouched() and counters(L)[:2] == base


@pytest.mark.parametrize("n", [1, 3, TPB + 1])
def test_greens_function_both_halves(chem, n):
    s, L = chem, chem.L
    up, dn, co = s.lists[n]
    w = np.array([-1.0, 0.25, 2.0])
    ng = len(w) * s.g.norb * s.g.norb
    for halves in ("both", "np1", "nm1"):
        def call():
            o = Outs(L)
            gp = o.arr(ng, np.float64) if halves != "nm1" else None
            gm = o.arr(ng, np.float64) if halves != "np1" else None
            return finish(L.sqmc_gpu_hci_greens_function(s.h, n, _p(up), _p(dn), _p(co), s.e_var, len(w), _p(w), 0, None if gp is None else _p(gp),
                                                         None if gm is None else _p(gm)), o)
        exercise(L, call, "greens_function n=%d %s" % (n, halves))


def test_hubbardk_sym_images():
    """the images door of a hubbardk context with space_sym works in one device buffer: one take"""
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    hst = H.HubbardKHost(4, 4, 2, 2, 1.0, 4.0, space_sym=True, z=1, p=1, start=(17, 3))      # 2 up 2 dn at total momentum 0
    g = hst.gpu()
    try:
        L = g.L
        _bind(L)
        L.sqmc_gpu_hubbardk_sym_images.argtypes = [V, C.c_int64] + [V] * 10
        n = TPB + 1
        up = np.ascontiguousarray(np.full(n, 17, np.uint64) << (np.arange(n, dtype=np.uint64) % np.uint64(11)))
        dn = np.full(n, 3, np.uint64)

        def call():
            o = Outs(L)
            outs = [o.arr(16 * n, np.uint64), o.arr(16 * n, np.uint64), o.arr(16 * n, np.int32), o.arr(n, np.uint64), o.arr(n, np.uint64),
                    o.arr(n, np.int32), o.arr(n, np.float64), o.arr(n, np.int32)]
            return finish(L.sqmc_gpu_hubbardk_sym_images(g.h, n, _p(up), _p(dn), *[_p(a) for a in outs]), o)
        assert exercise(L, call, "hubbardk_sym_images") == 1
    finally:
        g.close()


def test_rotate_integrals(chem):
    s, L = chem, chem.L
    norb = s.g.norb
    k = np.arange(norb)
    rot = np.ascontiguousarray(np.eye(norb) + 0.01 * np.sin(np.add.outer(k, 2.0 * k)))
    n_out = len(s.g._tabs[3])

    def call():
        o = Outs(L)
        out = o.arr(n_out, np.float64)
        return finish(L.sqmc_gpu_rotate_integrals(s.h, _p(rot), _p(out)), o)
    assert exercise(L, call, "rotate_integrals") == 3


@pytest.mark.parametrize("du_mode", [0, 1])
def test_stochastic_pt2_plan(sysm, du_mode):
    """prepare, a first sample from the smallest coefficient, a second from the eight largest that has to grow the connection buffers"""
    s, L = sysm, sysm.L
    up, dn, co = s.lists[TPB + 1]
    n, n_mc = len(up), 8
    small_ids, small_cnt = np.array([n - 1], np.int64), np.array([n_mc], np.int64)
    big_ids, big_cnt = np.arange(n_mc, dtype=np.int64), np.ones(n_mc, np.int64)
    grown = [0]
    assert L.sqmc_gpu_hci_set_diag_update(s.h, du_mode) == OK
    try:
        def call():
            o = Outs(L)
            plan = o.ptr()
            rc = L.sqmc_gpu_hci_pt2_stochastic_prepare(s.h, n, _p(up), _p(dn), _p(co), s.e_var, 1e-7, 1e-3, n_mc, C.byref(plan))
            if rc != OK:
                return finish(rc, o)
            o.ptrs.remove(plan)
            blob = b""
            try:
                for ids, cnt in ((small_ids, small_cnt), (big_ids, big_cnt)):
                    o2 = Outs(L)
                    val, ncon = o2.scalar(C.c_double), o2.scalar(C.c_int64)
                    rc = L.sqmc_gpu_hci_pt2_stochastic_sample(plan, len(ids), _p(ids), _p(cnt), C.byref(val), C.byref(ncon))
                    if rc != OK:
                        return finish(rc, o2)
                    blob += o2.blob()
                st = [C.c_int64() for _ in range(4)]
                assert L.sqmc_gpu_hci_pt2_stochastic_stats(plan, *[C.byref(x) for x in st]) == OK
                grown[0] = st[0].value
                return OK, blob + b"".join(bytes(x) for x in st)
            finally:
                assert L.sqmc_gpu_hci_pt2_stochastic_free(plan) == OK      # the plan remains freeable whatever failed
        exercise(L, call, "%s stochastic PT2 plan, du_mode %d" % (s.name, du_mode))
        assert grown[0] == 2, "the second sample did not have to grow: n_alloc = %d" % grown[0]
        base = counters(L)[:2]
        o = Outs(L)
        plan = o.ptr()
        assert L.sqmc_gpu_hci_pt2_stochastic_prepare(s.h, n, _p(up), _p(dn), _p(np.zeros(n)), s.e_var, 1e-7, 1e-3, n_mc, C.byref(plan)) == BAD_ARG
        assert o.untouched() and counters(L)[:2] == base
    finally:
        assert L.sqmc_gpu_hci_set_diag_update(s.h, 0) == OK


# ------------------------------------------------------------------------------------------------ peak bytes
def _at_least_8(b):
    return b if b else 8


def _conn_bytes(n_ref, T, U, rec):
    """Live bytes at the peak of one dedup-mode call of the connection generator before the owner, from its allocation sequence
    (nothing was freed before the dedup kernel had run, so the peak is the sum):
      count pass  ref_up, ref_dn, coeffs, counts, offsets: 5 * 8 n_ref; total: 8; scan state: 8 (tiles + 1), tiles = ceil(n_ref / SCAN_TILE) + 1
      fill        up, dn, num, den: 4 * 8 T; with records old_diag 8 T and packed pqrs 4 T
      sort        keys, keys_alt: 2 * 8 T; vals, vals_alt: 2 * 4 T; hist: 4 RS_MAX_RADIX ceil(T / RS_TILE); rowtot: 4 RS_MAX_RADIX
      heads       flags, pos: 2 * 8 T; scan state: 8 (tiles2 + 1), tiles2 = ceil(T / SCAN_TILE) + 1; total: 8
      unique      up, dn, num, den: 4 * 8 U; with records 8 U + 4 U"""
    tiles, tiles2 = -(-n_ref // SCAN_TILE) + 1, -(-T // SCAN_TILE) + 1
    return (5 * 8 * n_ref + 8 + 8 * (tiles + 1) + 32 * T + (12 * T if rec else 0) + 16 * T + 8 * T + 4 * RS_MAX_RADIX * -(-T // RS_TILE) + 4 * RS_MAX_RADIX
            + 16 * T + 8 * (tiles2 + 1) + 8 + 32 * U + (12 * U if rec else 0))


def _counts(s, n, eps, slice=0, n_slices=1):
    """(T, U): raw and unique connections of a slice, from raw mode and dedup mode"""
    out = []
    for mode in (2, 0):
        call, box = connections(s, n, eps, mode, False, slice, n_slices)
        assert call()[0] == OK
        out.append(box[0])
    return tuple(out)


def test_peak_bytes_of_hci_connections_do_not_rise(sysm):
    """One sqmc_gpu_hci_connections_record call in dedup mode (diag_mode 0) over TPB + 1 references.  The parent's peak is the sum that
    _conn_bytes writes out, an exact function of n_ref, the raw count T (what raw mode returns) and the unique count U: it freed its
    first buffer (the raw records) only after the dedup kernel, with every buffer of the call alive.  peak_bytes of the tree, reset just
    before the call and taken relative to what was live then, must not exceed it."""
    s, L = sysm, sysm.L
    n = TPB + 1
    T, U = _counts(s, n, 1e-4)
    assert U > 0 and T >= U
    call, box = connections(s, n, 1e-4, 0, True)
    live0 = counters(L, reset_peak=True)[1]
    assert call()[0] == OK and box[0] == U
    peak = counters(L)[2] - live0
    parent = _conn_bytes(n, T, U, True)
    print("%s hci_connections_record: n_ref %d T %d U %d: peak %d bytes, parent's %d" % (s.name, n, T, U, peak, parent))
    assert 0 < peak <= parent


def test_peak_bytes_of_hci_1rdm_pt_do_not_rise(sysm):
    """One sqmc_gpu_hci_1rdm_pt call with 2 slices over n = TPB + 1 determinants, nn = norb^2, nchunks = ceil(n / RDM_CHUNK).  The parent:
      list build   ranks, ranks_alt, up, dn, coeffs in rank order: 5 * 8 n; perm, perm_alt: 2 * 4 n; hist: 4 RS_MAX_RADIX (ceil(n / RS_TILE) + 1);
                   rowtot: 4 RS_MAX_RADIX; repeat flag: 4 -- these (L) lived to the end of the call; caller-order up, dn, coeffs: 3 * 8 n, freed
                   at the end of the build.  Build peak: L + 24 n.
      call         d_var, d_T, d_out: 3 * 8 nn; part: 16 nchunks nn.  A = L + 24 nn + 16 nchunks nn lived through the rest.
      var pass     its own part, 16 nchunks nn, on top of A.
      slice        the connection generator without records (its peak: _conn_bytes) on top of A; what it leaves behind, 32 U + 16 n, with
                   ckey and psi1 (16 U) on top, is less than that peak, which counts the same 32 U + 16 n among more.
    The parent's peak is the largest of the three; the tree's peak_bytes for the call must not exceed it."""
    s, L = sysm, sysm.L
    n, eps = TPB + 1, 1e-4
    up, dn, co = s.lists[n]
    nn = s.g.norb * s.g.norb
    nchunks = -(-n // RDM_CHUNK)
    Lb = 40 * n + 8 * n + 4 * RS_MAX_RADIX * (-(-n // RS_TILE) + 1) + 4 * RS_MAX_RADIX + 4
    A = Lb + 24 * nn + 16 * nchunks * nn
    slices = [_counts(s, n, eps, sl, 2) for sl in range(2)]
    parent = max([Lb + 24 * n, A + 16 * nchunks * nn] + [A + _conn_bytes(n, T, U, False) for T, U in slices if T > 0])
    o = Outs(L)
    rdm, nc = o.arr(nn, np.float64), o.scalar(C.c_int64)
    live0 = counters(L, reset_peak=True)[1]
    assert L.sqmc_gpu_hci_1rdm_pt(s.h, n, _p(up), _p(dn), _p(co), s.e_var, eps, 2, _p(rdm), C.byref(nc)) == OK
    peak = counters(L)[2] - live0
    print("%s hci_1rdm_pt: n %d slices (T, U) %r: peak %d bytes, parent's %d" % (s.name, n, slices, peak, parent))
    assert nc.value == sum(U for _, U in slices)
    assert 0 < peak <= parent
