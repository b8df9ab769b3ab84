"""The O(N) diagonal update of the HIP library (sqmc_gpu_diag_update_batch, the generator's record, sqmc_gpu_hci_set_diag_update in
sqmc_gpu_hci_pt2 and in the stochastic-PT plan) against tests/diag_update_checker.py, which shares nothing with the library or
the oracle.  Systems: the 8-electron C2 in d2h, the electron gas with 14 electrons in 19 and in 57 plane waves -- the systems of
tests/test_gpu_hci_edges.py.  Every tolerance is a derived bound (diag_update_checker.bound and its propagation through the
Epstein-Nesbet sum); every test prints its worst |delta| / bound.  On a library without the two new entry points every test here
fails (no skip): the methods they call do not exist."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from conftest import gpu_ctx_from_oracle, gpu_ctx_heg, gpu_ctx_hub          # noqa: E402
from tests import diag_update_checker as DU                                  # noqa: E402
from tests import hci_checker as HC                                          # noqa: E402
from tests import test_hci_checker as TH                                     # noqa: E402
from tests import test_proposal_unbiased as TU                               # noqa: E402

pytestmark = pytest.mark.gpu
BAD_ARG, UNSUPPORTED = -1, -3


def _ctx(sysm, which):
    import sqmc_amd
    sqmc_amd.set_device(0)
    if which.startswith("heg"):
        return gpu_ctx_heg(sysm)
    g = gpu_ctx_from_oracle(sysm)
    r, s_, a, pi, pc = sysm.hb_tables()
    g.set_hb_tables(r, s_, a, pi, pc, sysm.s.max_double)
    return g


@pytest.fixture
def ctx(request):
    made = []

    def make(which, sysm=None):
        sysm = sysm or request.getfixturevalue(which)
        g = _ctx(sysm, which)
        made.append(g)
        return g
    yield make
    for g in made:
        g.close()


def _model(request, which):
    sysm = request.getfixturevalue(which)
    chem = which.startswith("c2")
    H = TU.chem_checker(sysm) if chem else TU.heg_checker(sysm)
    return sysm, H, DU.ints_of(H, None if chem else sysm)


_REF = {}


def _reference(key, H, ints, sources):
    """every double excitation of the sources, once per session: records, the brute-force old_diag and H_aa, the plain-Python
    left-to-right value of the reference's statements and the sum of |integrals| each record uses"""
    if key not in _REF:
        rec = [(s, pqrs, new) for s in sources for pqrs, new in DU.double_records(H, s)]
        old = np.array([DU.brute(H, s)[0] for s, _, _ in rec])
        ref, sab = np.empty(len(rec)), np.empty(len(rec))
        for k, (s, pqrs, new) in enumerate(rec):
            ref[k], sab[k], _ = DU.update(ints, H.norb, old[k], pqrs, new[0], new[1])
        want = DU.brute_many(H, [r[2] for r in rec])
        _REF[key] = dict(rec=rec, old=old, ref=ref, sab=sab, want=want, pqrs=np.array([r[1] for r in rec], np.int32),
                         nu=np.array([r[2][0] for r in rec], np.uint64), nd=np.array([r[2][1] for r in rec], np.uint64))
    return _REF[key]


def _judge(tag, got, R, nelec):
    b = DU.gamma(DU.n_additions(nelec)) * (np.abs(R["old"]) + R["sab"])
    d = np.abs(got - R["want"])
    worst = float((d / b).max())
    bad = np.nonzero(~(d <= b))[0]
    print("%-34s %6d records, worst |delta| / bound = %.3g" % (tag, len(got), worst))
    assert len(bad) == 0, "%s: %d records outside the bound, worst |delta| / bound = %.3g, first %s" % (
        tag, len(bad), worst, [(R["rec"][k], float(got[k]), float(R["want"][k]), float(b[k])) for k in bad[:3]])
    return worst


def _door_case(tag, g, H, ints, sources, nelec):
    R = _reference(tag, H, ints, sources)
    kinds = {(int(p) <= H.norb, int(q) <= H.norb) for p, q in R["pqrs"][:, :2]}
    for form in (0, 1):
        got = g.diag_update_batch(R["old"], R["pqrs"], R["nu"], R["nd"], form)
        _judge("%s form %d" % (tag, form), got, R, nelec)
        if form == 0:
            differ = np.nonzero(got.view(np.uint64) != R["ref"].view(np.uint64))[0]
            assert len(differ) == 0, "%s: form 0 differs from the reference's statement order in %d of %d records, first %s" % (
                tag, len(differ), len(got), [(R["rec"][k], float(got[k]), float(R["ref"][k])) for k in differ[:3]])
    return kinds


# ---------------------------------------------------------------------------------------------- 1. the door against the brute force
@pytest.mark.parametrize("which", ["c2_walk", "heg14", "heg57"])
def test_door_against_brute_force(request, ctx, which):
    """every double excitation of HF and 7 seeded determinants, both forms within the bound, form 0 bit for bit the plain-Python
    left-to-right evaluation of chemistry.f90:9696-9737"""
    sysm, H, ints = _model(request, which)
    src = DU.seeded_sources((sysm.hf_up, sysm.hf_dn), H.norb, sysm.nup, sysm.ndn, 8)
    kinds = _door_case(which, ctx(which), H, ints, src, sysm.nup + sysm.ndn)
    assert kinds == {(True, True), (False, False), (True, False)}                      # up-up, dn-dn, up-dn
    R = _REF[which]
    near = sum(1 for s, (p, q, r, s_), n in R["rec"] if min(abs(r - p), abs(r - q), abs(s_ - p), abs(s_ - q)) == 1)
    assert near > 0                                                                     # r or s next to p or q


# ---------------------------------------------------------------------------------------------- 2. degenerate spin sectors
@pytest.mark.parametrize("nup,ndn", [(1, 1), (4, 0)])
def test_degenerate_spins(request, nup, ndn):
    """the same FCIDUMP with one electron per spin (both loops skip everything) and with no dn electron at all"""
    import sqmc_amd
    sysm, H, ints = _model(request, "c2_walk")
    sqmc_amd.set_device(0)
    g = sqmc_amd.GpuChem(sysm.norb, nup, ndn, sysm.orbsym(), sysm.prod().reshape(-1), sysm.combine_2().reshape(-1), sysm.integrals(),
                         n_group=sysm.s.n_group, time_sym=False, z=1)
    try:
        hf = ((1 << nup) - 1, (1 << ndn) - 1)
        src = DU.seeded_sources(hf, H.norb, nup, ndn, 8)
        kinds = _door_case("c2 nup %d ndn %d" % (nup, ndn), g, H, ints, src, nup + ndn)
        assert kinds == ({(True, False)} if ndn == 1 else {(True, True)})
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------- 3. bad records
def test_bad_records_are_refused(request, ctx):
    """each bad record returns SQMC_ERR_BAD_ARG -- alone and hidden among 600 good ones -- and the next valid call succeeds.
    The door sees a record and the determinant it leads to, not the source; "p not occupied in the source" shows there as p still
    occupied in the new determinant (an orbital the excitation did not empty), which is what the case feeds."""
    import sqmc_amd
    sysm, H, ints = _model(request, "c2_walk")
    g = ctx("c2_walk")
    n = H.norb
    src = (sysm.hf_up, sysm.hf_dn)
    rec = [(pqrs, new) for pqrs, new in DU.double_records(H, src)]
    old = DU.brute(H, src)[0]
    good_pq = np.array([r[0] for r in rec[:600]], np.int32)
    good_u, good_d = np.array([r[1][0] for r in rec[:600]], np.uint64), np.array([r[1][1] for r in rec[:600]], np.uint64)
    good = g.diag_update_batch(np.full(600, old), good_pq, good_u, good_d, 0)
    (p, q, r, s), (nu, nd) = next(x for x in rec if x[0][0] <= n < x[0][1])           # an up-dn record
    (p2, q2, r2, s2), (nu2, nd2) = next(x for x in rec if x[0][1] <= n)                # an up-up record
    stay = next(o + 1 for o in range(n) if (nu >> o) & 1 and o + 1 != r)              # an up orbital occupied before and after
    empty = next(o + 1 for o in range(n) if not (nu >> o) & 1 and o + 1 != p)          # an up orbital empty before and after
    empty_dn = next(o + 1 for o in range(n) if not (nd >> o) & 1 and o + 1 != q - n)   # a dn orbital empty before and after
    bad = {
        "p not emptied: still occupied in the new determinant": ((stay, q, r, s), nu, nd),
        "r not occupied in the target": ((p, q, empty, s), nu, nd),
        "s not occupied in the target": ((p, q, r, empty_dn + n), nu, nd),
        "spins: r of the other spin than p": ((p, q, s, r), nu, nd),
        "spins: up-up record with a dn target orbital": ((p2, q2, r2, s2 + n), nu2, nd2),
        "orbital number 0": ((0, q, r, s), nu, nd),
        "orbital number 2 norb + 1": ((p, q, r, 2 * n + 1), nu, nd),
        "orbital number far out of range": ((p, q, 1 << 20, s), nu, nd),
        "negative orbital number": ((p, -3, r, s), nu, nd),
        "p equal to q": ((p2, p2, r2, s2), nu2, nd2),
        "wrong electron number in the new determinant": ((p, q, r, s), nu | (1 << (empty - 1)), nd),
    }
    for name, (pq, u, d) in bad.items():
        for hide in (False, True):
            pqa = np.array([pq], np.int32); ua = np.array([u], np.uint64); da = np.array([d], np.uint64)
            if hide:
                pqa, ua, da = np.concatenate((good_pq[:300], pqa, good_pq[300:])), np.concatenate((good_u[:300], ua, good_u[300:])), np.concatenate((good_d[:300], da, good_d[300:]))
            with pytest.raises(sqmc_amd.SqmcGpuError) as e:
                g.diag_update_batch(np.full(len(ua), old), pqa, ua, da, int(hide))
            assert e.value.code == BAD_ARG, (name, hide, e.value)
        again = g.diag_update_batch(np.full(600, old), good_pq, good_u, good_d, 0)
        assert np.array_equal(again, good), name
    with pytest.raises(sqmc_amd.SqmcGpuError) as e:
        g.diag_update_batch(np.full(600, old), good_pq, good_u, good_d, 2)
    assert e.value.code == BAD_ARG
    with pytest.raises(sqmc_amd.SqmcGpuError) as e:
        g.hci_set_diag_update(3)
    assert e.value.code == BAD_ARG
    assert np.array_equal(g.diag_update_batch(np.full(600, old), good_pq, good_u, good_d, 0), good)


def test_time_sym_and_hubbard_are_unsupported(request):
    import sqmc_amd
    sqmc_amd.set_device(0)
    one = (np.array([-75.0]), np.array([[1, 2, 5, 6]], np.int32), np.array([0b111100], np.uint64), np.array([0b1111], np.uint64))
    for g in (gpu_ctx_from_oracle(request.getfixturevalue("c2_hci")), gpu_ctx_hub(request.getfixturevalue("hub44"))):
        try:
            for call in (lambda: g.diag_update_batch(*one, 0), lambda: g.diag_update_batch(*one, 1), lambda: g.hci_set_diag_update(1),
                         lambda: g.hci_set_diag_update(2)):
                with pytest.raises(sqmc_amd.SqmcGpuError) as e:
                    call()
                assert e.value.code == UNSUPPORTED, e.value
            g.hci_set_diag_update(0)                      # the default is always accepted
        finally:
            g.close()


# ---------------------------------------------------------------------------------------------- 4. the generator's record
@pytest.mark.parametrize("which", ["c2_walk", "heg14"])
def test_generator_record(request, ctx, which):
    """lists of 8 (C2) and 16 (HEG14) sources at the middle threshold: in raw mode every record reproduces its connection from its
    source and carries the source's H_ii bit for bit; merged, every determinant keeps the record of the first entry of its run;
    without the option the outputs are those of a second, untouched context bit for bit"""
    sysm = request.getfixturevalue(which)
    c = TH.build_case(sysm, which)
    g, g2 = ctx(which), ctx(which)
    u, d = TH.arrays(c.sources)
    eps, n = c.eps[1], c.norb
    hii = g.hamiltonian_batch(u, d, u, d)
    cu, cd, x, src, old, pq = g.hci_connections_record(u, d, c.coeffs, eps, 2)
    src = src.astype(np.int64)
    assert len(cu) > 100
    assert np.array_equal(old.view(np.uint64), hii[src].view(np.uint64))
    n_double = 0
    for k in range(len(cu)):
        s, new = c.sources[src[k]], (int(cu[k]), int(cd[k]))
        moved = bin(s[0] & ~new[0]).count("1") + bin(s[1] & ~new[1]).count("1")
        if moved < 2:
            assert not pq[k].any(), (k, s, new, pq[k])               # self slot or single excitation: no record, from scratch
            continue
        n_double += 1
        p, q, r, s_ = (int(v) for v in pq[k])
        assert DU.apply(s, (p, q, r, s_), n) == new, (k, s, new, pq[k])
        assert (p <= n) == (r <= n) and (q <= n) == (s_ <= n), pq[k]
    assert n_double > 50
    first = {}
    for k in range(len(cu)):
        first.setdefault((int(cu[k]), int(cd[k])), k)
    mu, md, mnum, mden, mold, mpq = g.hci_connections_record(u, d, c.coeffs, eps, 0)
    assert len(mu) == len(first) and len(mu) < len(cu)                 # some determinant is reached more than once
    for k in range(len(mu)):
        j = first[(int(mu[k]), int(md[k]))]
        assert mold[k] == old[j] and np.array_equal(mpq[k], pq[j]), (k, j, mpq[k], pq[j])
    for ns, sl in ((1, 0), (3, 1)):
        plain = g.hci_connections(u, d, c.coeffs, eps, 0, sl, ns)
        other = g2.hci_connections(u, d, c.coeffs, eps, 0, sl, ns)
        withrec = g.hci_connections_record(u, d, c.coeffs, eps, 0, sl, ns)
        for col in range(4):
            assert np.array_equal(plain[col], other[col]) and np.array_equal(plain[col], withrec[col]), (ns, col)
    raw_plain, raw_other = g.hci_connections(u, d, c.coeffs, eps, 2), g2.hci_connections(u, d, c.coeffs, eps, 2)
    for col, a in enumerate((cu, cd, x, src.astype(float))):
        assert np.array_equal(raw_plain[col], raw_other[col]) and np.array_equal(raw_plain[col], a), col
    print("%s: %d raw connections (%d doubles with a record), %d determinants" % (which, len(cu), n_double, len(mu)))


# ---------------------------------------------------------------------------------------------- 5. PT2
class _Pt2Door:
    def __init__(self, g):
        self.g = g

    def pt2(self, up, dn, coeffs, e_var, eps, n_slices=1):
        return self.g.hci_pt2(up, dn, coeffs, e_var, eps, n_slices)


def _record_bound(H, ints, source, new, nelec, cache):
    """the update's bound for the connection source -> new; 0 for a single excitation (recomputed from scratch in every mode)"""
    key = (source, new)
    if key not in cache:
        moved = bin(source[0] & ~new[0]).count("1") + bin(source[1] & ~new[1]).count("1")
        if moved != 2:
            cache[key] = 0.0
        else:
            old = DU.brute(H, source)[0]
            _, sab, _ = DU.update(ints, H.norb, old, DU.record_of(source, new, H.norb), new[0], new[1])
            cache[key] = DU.bound(old, sab, nelec)
    return cache[key]


SLICES = (1, 2, 5, 64)


@pytest.mark.parametrize("which", ["c2_walk", "heg14"])
def test_pt2_modes(request, ctx, which):
    """variational spaces of 8 (C2) and 16 (HEG14) determinants, not closed under H.  Mode 0 in 1, 2, 5 and 64 slices: the
    checker's value within its bound and n_connections as tests/test_gpu_hci_edges.py checks it, and the bits of a second
    context on which the mode was never set.  Modes 1 and 2: n_connections identical and delta_e within
        sum_a (sum_i H_ai c_i)^2 bound_a / (E - H_aa)^2
    of mode 0, bound_a the largest update bound among the sources that generate a.  No connected determinant of these inputs has
    |E - H_aa| < 1e-6 (asserted from the brute force), so a wrong H_aa cannot hide behind a small denominator."""
    sysm, H, ints = _model(request, which)
    c = TH.build_case(sysm, which)
    nelec = c.nup + c.ndn
    order = sorted(range(len(c.sources)), key=lambda k: c.sources[k])
    var, co = [c.sources[k] for k in order], [c.coeffs[k] for k in order]
    assert len(var) == TH.N_SOURCES[which]
    eps, e_var = c.eps[1], TH.e_var_of(c, var, co)
    g, g2 = ctx(which), ctx(which)
    TH.check_pt2(_Pt2Door(g), c, var, co, e_var, eps, slices=SLICES)
    con = HC.connections(H, var, co, eps, 0)
    assert not con.borderline
    inside = set(var)
    outside = [a for a in con.merged if a not in inside]
    assert outside
    haa = DU.brute_many(H, outside)
    gap = float(np.abs(e_var - haa).min())
    assert gap >= 1e-6, gap
    gen, cache = {}, {}
    for det, i, num, b in con.raw:
        if det not in inside:
            gen[det] = max(gen.get(det, 0.0), _record_bound(H, ints, var[i], det, nelec, cache))
    prop = math.fsum(con.merged[a][0] ** 2 * gen[a] / (e_var - h) ** 2 for a, h in zip(outside, haa.tolist()))
    assert prop > 0.0
    u, d = TH.arrays(var)
    base = {ns: g.hci_pt2(u, d, co, e_var, eps, ns) for ns in SLICES}
    for ns in SLICES:
        assert g2.hci_pt2(u, d, co, e_var, eps, ns) == base[ns], ns
    worst = 0.0
    for mode in (1, 2):
        g.hci_set_diag_update(mode)
        try:
            for ns in SLICES:
                de, nconn = g.hci_pt2(u, d, co, e_var, eps, ns)
                assert nconn == base[ns][1], (mode, ns, nconn, base[ns][1])
                ratio = abs(de - base[ns][0]) / prop
                worst = max(worst, ratio)
                assert abs(de - base[ns][0]) <= prop, "mode %d, %d slices: %r against %r, |delta| / bound = %.3g" % (mode, ns, de, base[ns][0], ratio)
        finally:
            g.hci_set_diag_update(0)
    for ns in SLICES:                                     # back in mode 0: the same bits as before
        assert g.hci_pt2(u, d, co, e_var, eps, ns) == base[ns], ns
    print("%s PT2 modes 1, 2 against mode 0: %d outside determinants, min |E - H_aa| %.3g, propagated bound %.3g, worst |delta| / bound = %.3g" % (
        which, len(outside), gap, prop, worst))


# ---------------------------------------------------------------------------------------------- 6. the stochastic plan
def test_stochastic_plan_modes(request, ctx):
    """HEG14, the 16-determinant space: one plan per mode, three samples with the same draws.  n_connected identical, values of
    modes 1 and 2 within sum_k |T_k| bound_k / (E - H_kk)^2 / (n_mc (n_mc - 1)) of mode 0, T_k = term1^2 + term2 - term1_big^2 -
    term2_big from the brute force; mode 0 has the bits of a context on which the mode was never set."""
    from sqmc_amd._lib import Pt2StochasticPlan
    which = "heg14"
    sysm, H, ints = _model(request, which)
    c = TH.build_case(sysm, which)
    nelec = c.nup + c.ndn
    order = sorted(range(len(c.sources)), key=lambda k: c.sources[k])
    var, co = [c.sources[k] for k in order], np.array([c.coeffs[k] for k in order])
    eps_pt, eps_big, n_mc = c.eps[0], c.eps[2], 6
    e_var = TH.e_var_of(c, var, co)
    u, d = TH.arrays(var)
    prob = np.abs(co) / np.abs(co).sum()
    draws = [([0, 3, 5, 9], [2, 1, 2, 1]), ([1, 2, 3, 4, 14, 15], [1, 1, 1, 1, 1, 1]), ([7], [6])]
    g, g2 = ctx(which), ctx(which)
    plans = {}
    try:
        for mode in (0, 1, 2):
            g.hci_set_diag_update(mode)
            plans[mode] = Pt2StochasticPlan(g, u, d, co, e_var, eps_pt, eps_big, n_mc)
        g.hci_set_diag_update(0)
        plans["fresh"] = Pt2StochasticPlan(g2, u, d, co, e_var, eps_pt, eps_big, n_mc)
        inside, cache, worst = set(var), {}, 0.0
        for ids, counts in draws:
            got = {m: p.sample(np.array(ids), np.array(counts)) for m, p in plans.items()}
            assert got[0] == got["fresh"], (ids, got)
            srcs = [var[i] for i in ids]
            con = HC.connections(H, srcs, [float(co[i]) for i in ids], eps_pt, 2)
            assert not con.borderline
            w = {k: counts[k] / prob[i] for k, i in enumerate(ids)}
            T, bnd = {}, {}
            for det, k, xv, _ in con.raw:
                if det in inside:
                    continue
                t = T.setdefault(det, [0.0, 0.0, 0.0, 0.0])
                a1, a2 = xv * w[k], xv * xv * ((n_mc - 1) * w[k] - w[k] * w[k])
                t[0] += a1; t[1] += a2
                if abs(xv) > eps_big:
                    t[2] += a1; t[3] += a2
                bnd[det] = max(bnd.get(det, 0.0), _record_bound(H, ints, srcs[k], det, nelec, cache))
            dets = sorted(T)
            hkk = DU.brute_many(H, dets)
            assert float(np.abs(e_var - hkk).min()) >= 1e-6
            prop = math.fsum(abs(T[a][0] ** 2 + T[a][1] - T[a][2] ** 2 - T[a][3]) * bnd[a] / (e_var - h) ** 2 for a, h in zip(dets, hkk.tolist())) / (n_mc * (n_mc - 1.0))
            assert prop > 0.0
            for mode in (1, 2):
                assert got[mode][1] == got[0][1] == len(dets), (mode, ids, got[mode][1], got[0][1], len(dets))
                ratio = abs(got[mode][0] - got[0][0]) / prop
                worst = max(worst, ratio)
                assert abs(got[mode][0] - got[0][0]) <= prop, "mode %d, ids %s: %r against %r, |delta| / bound = %.3g" % (mode, ids, got[mode][0], got[0][0], ratio)
        print("stochastic plan, modes 1, 2 against mode 0 over %d samples: worst |delta| / bound = %.3g" % (len(draws), worst))
    finally:
        for p in plans.values():
            p.close()
