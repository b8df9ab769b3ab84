"""The samples of the semistochastic PT2 on the device (sqmc_gpu_hci_pt2_stochastic_prepare / _sample) against tests/pt2s_checker.py,
which shares nothing with the library, the oracle or the numpy host path, at the shapes no deck reaches.

Against the brute force (sample(): derived bound, n_connected equal): every multiset of draws of a 5-determinant list with
n_mc = 4 and of 1, 2 and 3 determinants with n_mc = 2, each sample singly and their probability-weighted sum against
hci_checker.pt2(eps_pt) - hci_checker.pt2(eps_pt_big) and against the device's own deterministic PT2; n_var = 1; one determinant
carrying every draw; n_distinct = n_mc and = n_var; an eps_pt nothing passes and a closed space (exactly 0.0 and 0); eps_pt_big =
eps_pt and eps_pt_big above everything; connected determinants below and above every variational key; one run as long as the
sample; the active-space modes; the O(N) diagonal update; zero coefficients; the refusal of a time_sym context.

Anchored to the raw generator (from_raw(): the list sqmc_gpu_hci_connections returns in raw mode, which
tests/test_gpu_hci_edges.py holds to the brute force): samples whose raw connection count T puts nb = min(ceil(T / 256), 1024), the
grid of k_pt2s_terms, at 1, 40, 64, 65 and 1024, the last one with T below and above the 262144 connections one sweep of the grid
covers, each on a fresh plan and on one whose buffers a larger sample has already sized.

Conventions pinned here: the eps_pt_big test is strict (|H c| > eps_pt_big) for every excitation class; a sampled determinant with
coefficient 0 contributes nothing and changes no bit; a time_sym context is refused (the estimator is biased there:
tests/test_pt2s_checker.py::test_time_symmetry_biases_the_estimator).  Every tolerance is a derived bound; every test prints its
worst |delta| / bound.  The printed table of the large cases is kept in tests/golden/README_pt2_stochastic_edges.md."""
import math
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from conftest import gpu_ctx_from_oracle, gpu_ctx_heg          # noqa: E402
from tests import diag_update_checker as DU                     # noqa: E402
from tests import hci_checker as HC                             # noqa: E402
from tests import pt2s_checker as PS                            # noqa: E402
from tests import test_hci_checker as TH                        # noqa: E402
from tests import test_pt2s_checker as TP                       # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
UNSUPPORTED = -3


def _ctx(sysm, which):
    import sqmc_amd
    sqmc_amd.set_device(0)
    if which.startswith("heg"):
        return gpu_ctx_heg(sysm)
    g = gpu_ctx_from_oracle(sysm)
    r, s_, a, pi, pc = sysm.hb_tables()
    g.set_hb_tables(r, s_, a, pi, pc, sysm.s.max_double)
    return g


@pytest.fixture(scope="module")
def door(request):
    """which -> (context, case, system): one context per system for the module"""
    made = {}

    def make(which):
        if which not in made:
            sysm = request.getfixturevalue(which)
            made[which] = (_ctx(sysm, which), TH.build_case(sysm, which), sysm)
        return made[which]
    yield make
    for g, _, _ in made.values():
        g.close()


def _plan(g, var, co, e_var, eps_pt, eps_big, n_mc):
    from sqmc_amd import Pt2StochasticPlan
    u, d = TH.arrays(var)
    return Pt2StochasticPlan(g, u, d, np.array(co, float), e_var, eps_pt, eps_big, n_mc)


def _bits(x):
    return np.float64(x).tobytes()


def _against_model(tag, c, plan, var, co, e_var, eps, n_mc, draws, active_space=None):
    """the given (ids, counts) through the plan and through sample(): [(model Result, value, n_connected)], worst ratio printed"""
    out, worst = [], 0.0
    for ids, counts in draws:
        res = PS.sample(c.H, var, co, ids, counts, e_var, eps[0], eps[1], n_mc, active_space=active_space)
        v, n = plan.sample(ids, counts)
        fails, ratio = PS.compare(res, v, n)
        assert not fails, (tag, ids, counts, fails)
        worst = max(worst, ratio)
        out.append((res, v, n))
    print("%s: %d samples, worst |delta| / bound = %.3g" % (tag, len(out), worst))
    return out


# ---------------------------------------------------------------------------------------------- against the brute force
@pytest.mark.parametrize("which,n_var,n_mc", [(w, a, b) for w in ("c2_walk", "heg14") for a, b in TP.SHAPES])
def test_exhaustive_expectation(door, which, n_var, n_mc):
    """every multiset of draws: each sample within the model's bound with the model's n_connected; sum P value within the summed
    bounds of the brute-force PT2(eps_pt) - PT2(eps_pt_big), and of the same difference from sqmc_gpu_hci_pt2"""
    g, c, _ = door(which)
    var, co, e_var = TP.space(c, n_var)
    eps = TP.thresholds(c, n_var)
    t0 = time.time()
    with _plan(g, var, co, e_var, eps[0], eps[1], n_mc) as plan:
        run, _ = TP.check_unbiased(c, n_var, n_mc, lambda ids, counts: plan.sample(ids, counts), "device")
    want, wb = TP.reference_difference(c, var, co, e_var, *eps)
    u, d = TH.arrays(var)
    dev = g.hci_pt2(u, d, co, e_var, eps[0], 1)[0] - g.hci_pt2(u, d, co, e_var, eps[1], 1)[0]
    ratio = abs(run["mean"] - dev) / (run["bound"] + 2 * wb)
    print("%s (%d, %d): against the device's deterministic difference %.15g: |delta| / bound = %.3g; %.1f s" % (which, n_var, n_mc, dev, ratio, time.time() - t0))
    assert abs(run["mean"] - dev) <= run["bound"] + 2 * wb
    if which == "c2_walk" or n_var == 5:
        assert want != 0.0 and any(r[5] > 0 for r in run["rows"])


@pytest.mark.parametrize("which", ["c2_walk", "heg14"])
def test_one_determinant_space(door, which):
    """n_var = 1, counts = [n_mc]: p = 1, every sample is itself the deterministic difference"""
    g, c, _ = door(which)
    var, co, e_var = TP.space(c, 1)
    eps = TP.thresholds(c, 1)
    want, wb = TP.reference_difference(c, var, co, e_var, *eps)
    for n_mc in (2, 3, 200):
        with _plan(g, var, co, e_var, eps[0], eps[1], n_mc) as plan:
            (res, v, n), = _against_model("%s n_var 1 n_mc %d" % (which, n_mc), c, plan, var, co, e_var, eps, n_mc, [([0], [n_mc])])
        print("    value %.15g, deterministic difference %.15g, |delta| / bound = %.3g" % (v, want, abs(v - want) / (res.bound + wb)))
        assert abs(v - want) <= res.bound + wb and n > 0


@pytest.mark.parametrize("which", ["c2_walk", "heg14"])
def test_draw_shapes(door, which):
    """one determinant of the 5 carries every draw (first, middle, last); n_distinct = n_mc with every count 1; n_distinct = n_var"""
    g, c, _ = door(which)
    var, co, e_var = TP.space(c, 5)
    eps = TP.thresholds(c, 5)
    with _plan(g, var, co, e_var, eps[0], eps[1], 4) as plan:
        _against_model("%s one determinant carries all 4 draws" % which, c, plan, var, co, e_var, eps, 4, [([k], [4]) for k in (0, 2, 4)])
        _against_model("%s n_distinct = n_mc = 4" % which, c, plan, var, co, e_var, eps, 4, [([0, 1, 3, 4], [1] * 4), ([1, 2, 3, 4], [1] * 4)])
    with _plan(g, var, co, e_var, eps[0], eps[1], 5) as plan:
        _against_model("%s n_distinct = n_var = n_mc = 5" % which, c, plan, var, co, e_var, eps, 5, [(list(range(5)), [1] * 5)])
    with _plan(g, var, co, e_var, eps[0], eps[1], 9) as plan:
        _against_model("%s n_distinct = n_var = 5, n_mc 9" % which, c, plan, var, co, e_var, eps, 9, [(list(range(5)), [3, 1, 2, 1, 2])])


@pytest.mark.parametrize("which", ["c2_walk", "heg14"])
def test_nothing_connected(door, which):
    """eps_pt above every |H c|: only self slots are generated, value exactly 0.0 and n_connected 0; on HEG14 also the space closed
    under the screened generator.  An ordinary sample before and after has the same bits."""
    g, c, _ = door(which)
    var, co, e_var = TP.space(c, 5)
    eps = TP.thresholds(c, 5)
    draw = ([0, 2, 3], [2, 1, 1])
    with _plan(g, var, co, e_var, eps[0], eps[1], 4) as plan:
        (_, good, n_good), = _against_model("%s ordinary sample" % which, c, plan, var, co, e_var, eps, 4, [draw])
        assert n_good > 0
        high = TP.above_everything(c, 5)
        with _plan(g, var, co, e_var, high, 2 * high, 4) as empty:
            for ids, counts, _ in PS.expectation(co, 4):
                v, n = empty.sample(ids, counts)
                assert _bits(v) == _bits(0.0) and n == 0, (ids, counts, v, n)
                assert empty.stats()["last_raw"] == len(ids)
            res = PS.sample(c.H, var, co, draw[0], draw[1], e_var, high, 2 * high, 4)
            assert res.value == 0.0 and res.n_connected == 0 and res.n_raw == 3
        again = plan.sample(*draw)
        assert _bits(again[0]) == _bits(good) and again[1] == n_good
        if which == "heg14":
            name, cv, cc, ceps, zero = next(s for s in TH.pt2_spaces(c) if s[0] == "closed space")
            order = sorted(range(len(cv)), key=lambda k: cv[k])
            cv, cc = [cv[k] for k in order], [cc[k] for k in order]
            live = [k for k, x in enumerate(cc) if abs(x) > 0.5]
            assert zero and len(live) == 3
            e_closed = TH.e_var_of(c, cv, cc)
            with _plan(g, cv, cc, e_closed, ceps, 4 * ceps, 6) as closed:
                for ids, counts in ((live, [2, 2, 2]), (live[:1], [6]), (sorted(set(live + [0, len(cv) - 1])), None)):
                    counts = counts or [1] * len(ids)
                    v, n = closed.sample(ids, counts)
                    res = PS.sample(c.H, cv, cc, ids, counts, e_closed, ceps, 4 * ceps, 6)
                    assert not res.borderline and res.n_connected == 0 and res.n_raw > len(ids)
                    assert _bits(v) == _bits(0.0) and n == 0, (ids, v, n)
                print("heg14 closed space of %d determinants: 0.0 and 0 (raw connections of the last sample %d)" % (len(cv), closed.stats()["last_raw"]))
            again = plan.sample(*draw)
            assert _bits(again[0]) == _bits(good) and again[1] == n_good


@pytest.mark.parametrize("which", ["c2_walk", "heg14"])
def test_eps_pt_big_at_its_ends(door, which):
    """eps_pt_big = eps_pt: every kept path is big, the value stays within the bound of 0 (not exactly 0: ((a + b) - a) - b rounds).
    eps_pt_big above everything: the full estimator, whose expectation is hci_checker.pt2(eps_pt)."""
    g, c, _ = door(which)
    var, co, e_var = TP.space(c, 5)
    eps_pt = TP.thresholds(c, 5)[0]
    with _plan(g, var, co, e_var, eps_pt, eps_pt, 4) as plan:
        draws = [(i, w) for i, w, _ in PS.expectation(co, 4)]
        out = _against_model("%s eps_pt_big = eps_pt" % which, c, plan, var, co, e_var, (eps_pt, eps_pt), 4, draws)
        worst = 0.0
        for res, v, n in out:
            assert res.value == 0.0 or abs(res.value) <= res.bound
            assert abs(v) <= res.bound
            worst = max(worst, abs(v) / res.bound if res.bound else 0.0)
        print("    largest |value| / bound = %.3g" % worst)
    n_var, n_mc = (5, 4) if which == "heg14" else (3, 2)
    var, co, e_var = TP.space(c, n_var)
    eps = (TP.thresholds(c, n_var)[0], TP.above_everything(c, n_var))
    with _plan(g, var, co, e_var, eps[0], eps[1], n_mc) as plan:
        run, _ = TP.check_unbiased(c, n_var, n_mc, lambda ids, counts: plan.sample(ids, counts), "device, eps_pt_big above everything", eps=eps)
    full = HC.pt2(c.H, var, co, e_var, eps[0])
    assert abs(run["mean"] - full[0]) <= run["bound"] + full[3] and full[0] < 0.0


@pytest.mark.parametrize("which", ["c2_walk", "heg14"])
def test_extreme_keys(door, which):
    """TH.extreme_key_space: connected determinants below the smallest and above the largest variational key, both ends of the
    membership search; every multiset of 3 draws"""
    g, c, _ = door(which)
    var, co = TH.extreme_key_space(c)
    e_var = min(TH.e_var_of(c, var, co), HC.diagonal(c.H, c.sources[0])[0] - 0.1)             # HF is outside this space: below its diagonal too
    vals = HC.screen_values(c.H, var, co)
    eps = (HC.pick_eps(vals, TH._k_for(vals, len(vals) // 2)), HC.pick_eps(vals, TH._k_for(vals, len(vals) // 8)))
    keys = [HC.det_key(v, c.norb, c.ndn) for v in var]
    tb = PS.table(c.H, var, co, eps[0])
    outside = [HC.det_key(k, c.norb, c.ndn) for k, inside in zip(tb.keys, tb.key_inside) if not inside]
    assert min(outside) < min(keys) and max(outside) > max(keys)
    with _plan(g, var, co, e_var, eps[0], eps[1], 3) as plan:
        TP.check_unbiased(c, 2, 3, lambda ids, counts: plan.sample(ids, counts), "device, extreme keys", eps=eps, given=(var, co, e_var))


def test_one_long_run(door):
    """HEG14: the list is made of determinants that HF reaches (38 of them), HF left out, all of them sampled once: HF is a
    connected determinant outside the list that every source reaches, so one thread walks a run of n_distinct connections"""
    g, c, _ = door("heg14")
    src, co, _ = TH.long_list(c, 40)
    hf = c.sources[0]
    pairs = sorted((s, x) for s, x in zip(src, co) if s != hf and any(p.det == hf and not p.noise for p in HC.raw_paths(c.H, s)))
    var, co = [p[0] for p in pairs], [p[1] for p in pairs]
    n = len(var)
    assert n >= 32
    e_var = HC.diagonal(c.H, hf)[0] - 0.1
    vals = HC.screen_values(c.H, var, co)
    to_hf = [abs(p.raw * x) for s, x in zip(var, co) for p in HC.raw_paths(c.H, s) if p.det == hf]
    assert len(to_hf) == n
    distinct = sorted({abs(v) for v in vals}, reverse=True)
    k = sum(1 for v in distinct if v >= min(to_hf))                  # a threshold between two values, below every path to HF
    eps = (HC.pick_eps(vals, k) if k < len(distinct) else 0.7 * distinct[-1], HC.pick_eps(vals, TH._k_for(vals, len(vals) // 2)))
    assert eps[0] < min(to_hf)
    assert eps[0] < eps[1]
    ids, counts = list(range(n)), [1] * n
    res = PS.sample(c.H, var, co, ids, counts, e_var, eps[0], eps[1], n)
    assert res.longest_run == n and hf in res.terms, res.longest_run
    with _plan(g, var, co, e_var, eps[0], eps[1], n) as plan:
        _against_model("heg14 a run of %d" % n, c, plan, var, co, e_var, eps, n, [(ids, counts), (ids[::2], [2] * (len(ids[::2]) - 1) + [2 - n % 2])])


def test_active_space_modes(door):
    """C2, the (5, 4) case with the lowest orbital frozen and the last 8 virtual: modes 1 and 2 against the model, and since they
    partition the connected determinants a sample's two values add up to the unmasked one: each of the three sums is within
    K 2^-53 of its share of A, the shares of modes 1 and 2 add up to A, and three divisions and one addition round once more each"""
    g, c, _ = door("c2_walk")
    var, co, e_var = TP.space(c, 5)
    eps = TP.thresholds(c, 5)
    mask = TH.active_space_of(c)
    draws = [(i, w) for i, w, _ in PS.expectation(co, 4)]
    out = {}
    try:
        with _plan(g, var, co, e_var, eps[0], eps[1], 4) as plan:
            for mode in (0, 1, 2):
                g.hci_set_active_space(*mask, mode)
                out[mode] = _against_model("c2_walk active-space mode %d" % mode, c, plan, var, co, e_var, eps, 4, draws, active_space=mask + (mode,) if mode else None)
    finally:
        g.hci_set_active_space(0, 0, 0, 0, 0)
    worst = 0.0
    for (r0, v0, n0), (r1, v1, n1), (r2, v2, n2) in zip(out[0], out[1], out[2]):
        assert n1 + n2 == n0 and r1.n_connected + r2.n_connected == r0.n_connected
        b = (r0.K + 2) * 2 * U * r0.A
        worst = max(worst, abs(v1 + v2 - v0) / b)
        assert abs(v1 + v2 - v0) <= b, (v0, v1, v2, b)
    assert any(n1 > 0 and n2 > 0 for (_, _, n1), (_, _, n2) in zip(out[1], out[2]))
    print("c2_walk: largest |mode1 + mode2 - mode0| / ((K + 2) 2^-52 A) = %.3g" % worst)


def _update_bounds(c, sysm, var, tb):
    """per connected determinant: the largest bound of the O(N) update (tests/diag_update_checker.py) among the double excitations
    that reach it from the list; 0 where only single excitations do (those are recomputed from scratch)"""
    ints = DU.ints_of(c.H, None if c.chem else sysm)
    nelec = c.nup + c.ndn
    out = {}
    for k, s in zip(tb.kid.tolist(), tb.src.tolist()):
        det, source = tb.keys[k], var[s]
        moved = bin(source[0] & ~det[0]).count("1") + bin(source[1] & ~det[1]).count("1")
        b = 0.0
        if moved == 2:
            old = DU.brute(c.H, source)[0]
            _, sab, _ = DU.update(ints, c.H.norb, old, DU.record_of(source, det, c.H.norb), det[0], det[1])
            b = DU.bound(old, sab, nelec)
        out[det] = max(out.get(det, 0.0), b)
    return out


@pytest.mark.parametrize("which", ["c2_walk", "heg14"])
def test_diag_update_modes(door, which):
    """sqmc_gpu_hci_set_diag_update 1 and 2 (k_pt2s_terms_upd) on the (5, 4) case: the model's bound plus the update's own,
    sum_k A_k b_k / (E_var - H_kk)^2 / (n_mc (n_mc - 1)), b_k from tests/diag_update_checker.py; mode 0 afterwards has its bits"""
    g, c, sysm = door(which)
    var, co, e_var = TP.space(c, 5)
    eps = TP.thresholds(c, 5)
    tb = PS.table(c.H, var, co, eps[0])
    t0 = time.time()
    upd = _update_bounds(c, sysm, var, tb)
    draws = [(i, w) for i, w, _ in PS.expectation(co, 4)]
    with _plan(g, var, co, e_var, eps[0], eps[1], 4) as plan:
        base = [plan.sample(i, w) for i, w in draws]
    worst = {}
    try:
        for mode in (1, 2):
            g.hci_set_diag_update(mode)
            with _plan(g, var, co, e_var, eps[0], eps[1], 4) as plan:
                g.hci_set_diag_update(0)                      # the plan keeps the mode it was prepared with
                for (ids, counts), (v0, n0) in zip(draws, base):
                    res = PS.sample(c.H, var, co, ids, counts, e_var, eps[0], eps[1], 4)
                    extra = math.fsum((t[0] ** 2 + abs(t[1]) + t[2] ** 2 + abs(t[3])) * upd[d] / (e_var - t[4]) ** 2 for d, t in res.terms.items()) / 12.0
                    v, n = plan.sample(ids, counts)
                    assert n == n0 and res.n_connected <= n <= res.n_connected + res.n_optional
                    assert not res.borderline
                    ratio = abs(v - res.value) / (res.bound + extra) if res.bound + extra > 0 else 0.0
                    worst[mode] = max(worst.get(mode, 0.0), ratio)
                    assert abs(v - res.value) <= res.bound + extra, (mode, ids, counts, v, res.value, res.bound, extra)
    finally:
        g.hci_set_diag_update(0)
    with _plan(g, var, co, e_var, eps[0], eps[1], 4) as plan:
        again = [plan.sample(i, w) for i, w in draws]
    assert [(_bits(v), n) for v, n in again] == [(_bits(v), n) for v, n in base]
    print("%s diag-update modes: worst |delta| / bound = %s over %d samples; %.1f s" % (which, {m: "%.3g" % w for m, w in worst.items()}, len(draws), time.time() - t0))


@pytest.mark.parametrize("which", ["c2_walk", "heg14"])
def test_zero_coefficients(door, which):
    """a sampled determinant with coefficient 0 (p = 0, w/p = inf) next to live ones: the bits and the count of the sample without
    it, a finite value, the model's value; a sample of such determinants only: 0.0 and 0"""
    g, c, _ = door(which)
    var, co, e_var = TP.space(c, 5)
    eps = TP.thresholds(c, 5)
    co = [0.0 if k in (1, 4) else x for k, x in enumerate(co)]
    with _plan(g, var, co, e_var, eps[0], eps[1], 4) as plan:
        for with_zero, without in ((([0, 1, 2], [2, 1, 1]), ([0, 2], [2, 1])), (([0, 3, 4], [1, 1, 2]), ([0, 3], [1, 1])), (([1, 2, 4], [1, 2, 1]), ([2], [2]))):
            a, b = plan.sample(*with_zero), plan.sample(*without)
            assert math.isfinite(a[0]) and a[1] > 0
            assert _bits(a[0]) == _bits(b[0]) and a[1] == b[1], (with_zero, a, b)
        _against_model("%s zero coefficients among the sampled" % which, c, plan, var, co, e_var, eps, 4, [([0, 1, 2], [2, 1, 1]), ([1, 2, 4], [1, 2, 1])])
        for ids, counts in (([1], [4]), ([4], [4]), ([1, 4], [3, 1])):
            v, n = plan.sample(ids, counts)
            assert _bits(v) == _bits(0.0) and n == 0 and plan.stats()["last_raw"] == 0


def test_time_sym_context_is_refused(door):
    """the estimator is biased on time-reversal representatives (tests/test_pt2s_checker.py): prepare says so and points to the
    determinant-basis expansion; an ordinary plan on a context without time_sym works afterwards"""
    from sqmc_amd import SqmcGpuError
    g, c, _ = door("c2_hci")
    var, co, e_var = TP.space(c, 5)
    with pytest.raises(SqmcGpuError) as ei:
        _plan(g, var, co, e_var, c.eps[0], c.eps[1], 4)
    assert ei.value.code == UNSUPPORTED and "determinant-basis" in str(ei.value) and "time_sym = 0" in str(ei.value), str(ei.value)
    u, d = TH.arrays(var)
    assert g.hci_pt2(u, d, co, e_var, c.eps[1], 1)[1] > 0           # the context itself is alive
    g, c, _ = door("c2_walk")
    var, co, e_var = TP.space(c, 3)
    eps = TP.thresholds(c, 3)
    with _plan(g, var, co, e_var, eps[0], eps[1], 2) as plan:
        _against_model("c2_walk after the refusal", c, plan, var, co, e_var, eps, 2, [([0, 2], [1, 1])])


# ---------------------------------------------------------------------------------------------- anchored to the raw generator
N_POOL, LARGE_EPS = 2200, 1e-5
TARGETS = [("nb 1", 200), ("nb 40", 39 * 256 + 100), ("nb 64", 63 * 256 + 37), ("nb 65", 64 * 256 + 37), ("nb 1024, one sweep", 1023 * 256 + 101),
           ("nb 1024, grid-stride", 262144 + 4321)]
_POOL = {}


def large_pool(connections, hf):
    """2200 HEG14 determinants found by breadth-first connection from HF through the generator itself (HF's own connections are
    277, too few for 262144 raw connections, so theirs are added), sorted.  Three in eleven get a coefficient of 1e-30, with which
    a determinant generates its own slot and nothing else: they tune a sample's raw connection count one by one.  The others get
    mixed signs and magnitudes from 0.5 down to 1e-4 by geomspace, in list order.  cnt = raw connections of each at LARGE_EPS."""
    if "pool" not in _POOL:
        have, eps = [hf], 1e-3
        while len(have) < N_POOL:
            u, dn = TH.arrays(have[:64])
            cu, cd, _, _ = connections(u, dn, np.ones(len(u)), eps, 0)
            have = sorted(set(have) | set(zip(cu.tolist(), cd.tolist())))
            eps *= 0.5
            assert eps > 1e-9
        var = have[:N_POOL]
        k = np.arange(N_POOL)
        tiny = np.isin(k % 11, (2, 5, 8))
        live = np.nonzero(~tiny)[0]
        co = np.where(k % 3 == 1, -1.0, 1.0) * 1e-30
        co[live] *= 1e30 * np.geomspace(0.5, 1e-4, len(live))
        u, dn = TH.arrays(var)
        src = connections(u, dn, co, LARGE_EPS, 2)[3].astype(np.int64)
        cnt = np.bincount(src, minlength=N_POOL)
        assert (cnt[tiny] == 1).all() and cnt[live].max() > 256
        _POOL["pool"] = dict(var=var, u=u, d=dn, co=co, cnt=cnt, tiny=np.nonzero(tiny)[0], live=live)
    return _POOL["pool"]


def choose(pool, target):
    """(ids of a sample with exactly `target` raw connections, ids of as many determinants with more): live determinants in list
    order as long as they fit, then one-connection determinants for the rest; the larger sample takes live ones only"""
    ids, total = [], 0
    for i in pool["live"]:
        if total + pool["cnt"][i] <= target - 1:
            ids.append(int(i)); total += int(pool["cnt"][i])
    rest = target - total
    assert 1 <= rest <= len(pool["tiny"]) and ids, (target, total)
    ids = sorted(ids + pool["tiny"][:rest].tolist())
    assert 2 <= len(ids) <= len(pool["live"])
    larger = sorted(pool["live"][:len(ids)].tolist())
    assert int(pool["cnt"][larger].sum()) > target
    return ids, larger


def large_reference(pool, ids, connections, h_kk_of, e_var):
    """from_raw() on the raw list of the sampled determinants, counts all 1, n_mc = their number; eps_pt_big is chosen from that
    list, between two of its |H c| (pick_eps) with about half of the connections above it.  Returns (Result, eps_pt_big)."""
    ids = np.array(ids)
    prob = np.abs(pool["co"]) / np.abs(pool["co"]).sum()
    cu, cd, x, src = connections(pool["u"][ids], pool["d"][ids], pool["co"][ids], LARGE_EPS, 2)
    vals = np.abs(x[x != 0.0]).tolist()
    eps_big = HC.pick_eps(vals, TH._k_for(vals, len(vals) // 2))
    return PS.from_raw(cu, cd, x, src, pool["var"], 1.0 / prob[ids], e_var, h_kk_of, eps_big, len(ids), n_var=N_POOL), eps_big


@pytest.mark.parametrize("name,target", TARGETS)
def test_block_and_stride_seams(door, name, target):
    from sqmc_amd import Pt2StochasticPlan
    g, c, _ = door("heg14")
    t0 = time.time()
    pool = large_pool(lambda u, d, co, eps, mode: g.hci_connections(u, d, co, eps, mode), c.sources[0])
    e_var = float(g.hamiltonian_batch(pool["u"], pool["d"], pool["u"], pool["d"]).min()) - 0.1
    ids, larger = choose(pool, target)
    n_mc = len(ids)
    res, eps_big = large_reference(pool, ids, lambda u, d, co, eps, mode: g.hci_connections(u, d, co, eps, mode), lambda u, d: g.hamiltonian_batch(u, d, u, d), e_var)
    assert res.n_raw == target and target % 256 != 0
    assert 0 < res.n_big < res.n_paths
    nb = PS.blocks(target)
    assert nb == {"nb 1": 1, "nb 40": 40, "nb 64": 64, "nb 65": 65}.get(name, 1024)
    if target > 256:
        assert len(res.crosses_256) > 0
    if target > 262144:
        assert len(res.crosses_stride) + len(res.starts_on_stride) > 0
    ones = np.ones(n_mc, np.int64)
    with Pt2StochasticPlan(g, pool["u"], pool["d"], pool["co"], e_var, LARGE_EPS, eps_big, n_mc) as fresh, \
            Pt2StochasticPlan(g, pool["u"], pool["d"], pool["co"], e_var, LARGE_EPS, eps_big, n_mc) as used:
        v, n = fresh.sample(ids, ones)
        assert fresh.stats()["last_raw"] == target
        used.sample(larger, ones)
        st = used.stats()
        assert st["last_raw"] > target and st["n_alloc"] == 1
        v2, n2 = used.sample(ids, ones)
        assert used.stats()["n_alloc"] == 1 and used.stats()["last_raw"] == target
    fails, ratio = PS.compare(res, v, n)
    print("| %s | %d | %d | %d | %d | %d | %d | %d | %.3g | %.1f s" % (name, target, nb, n_mc, res.n_connected, res.longest_run, len(res.crosses_256),
                                                                    len(res.crosses_stride) + len(res.starts_on_stride), ratio, time.time() - t0))
    assert not fails, fails
    assert res.n_connected > 0 and v != 0.0
    assert _bits(v2) == _bits(v) and n2 == n
