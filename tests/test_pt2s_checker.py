"""tests/pt2s_checker.py on its own terms, on the CPU: the model of a semistochastic PT2 sample is exactly unbiased (its expectation
over every multiset of draws is hci_checker.pt2(eps_pt) - hci_checker.pt2(eps_pt_big) within the summed bounds), the numpy host path
(host.pt2_stochastic_sample_host) fed by the CPU oracle agrees with it sample by sample, every doctored model is rejected at more
than 100 times the bound, and under time-reversal symmetry the estimator on unmerged raw paths is biased (the number is printed and
pinned).  The helpers here (space, exhaustive, reference_difference) are the ones tests/test_gpu_pt2s_edges.py runs with the
library behind them.

Checker wall time: the rows are those tests/test_hci_checker.py caches; what is added is H_kk of every connected determinant by
second quantisation (C2: about 40 000 of them for the 5-determinant list).  Each test prints its own seconds."""
import math
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import hci_checker as HC               # noqa: E402
from tests import pt2s_checker as PS              # noqa: E402
from tests import test_hci_checker as TH          # noqa: E402

U = 2.0 ** -53
SHAPES = [(5, 4), (1, 2), (2, 2), (3, 2)]         # (n_var, n_mc): 70, 1, 3 and 6 multisets
POWER = 100.0
_REF = {}


def space(c, n_var):
    """the first n_var sources of the case in (up, dn) order, their coefficients, a variational energy below every diagonal"""
    order = sorted(range(n_var), key=lambda k: c.sources[k])
    var, co = [c.sources[k] for k in order], [c.coeffs[k] for k in order]
    return var, co, TH.e_var_of(c, var, co)


def thresholds(c, n_var):
    """(eps_pt, eps_pt_big): for the 5-determinant list the case's own first two (nearly every path kept; half of them); a shorter
    list gets the same two choices from its own paths, so that some path lies between them"""
    if n_var == 5:
        return c.eps[0], c.eps[1]
    var, co, _ = space(c, n_var)
    vals = HC.screen_values(c.H, var, co, c.ts, c.z)
    nv = len({abs(v) for v in vals})
    return HC.pick_eps(vals, min(TH._k_for(vals, len(vals) - 3), nv - 1)), HC.pick_eps(vals, TH._k_for(vals, len(vals) // 2))


def above_everything(c, n_var):
    """an eps_pt_big no path reaches: the sample is the full estimator"""
    var, co, _ = space(c, n_var)
    return 2.0 * max(HC.screen_values(c.H, var, co, c.ts, c.z))


def reference_difference(c, var, co, e_var, eps_pt, eps_big):
    """(hci_checker.pt2(eps_pt) - hci_checker.pt2(eps_pt_big), bound); eps_big None: pt2(eps_pt) alone"""
    key = (c.which, tuple(var), tuple(co), e_var, eps_pt, eps_big)
    if key not in _REF:
        a = HC.pt2(c.H, var, co, e_var, eps_pt, c.ts, c.z)
        assert not a[4], a[4][:3]
        if eps_big is None:
            _REF[key] = (a[0], a[3])
        else:
            b = HC.pt2(c.H, var, co, e_var, eps_big, c.ts, c.z)
            assert not b[4], b[4][:3]
            _REF[key] = (a[0] - b[0], a[3] + b[3] + U * (abs(a[0]) + abs(b[0])))
    return _REF[key]


def exhaustive(c, n_var, n_mc, value_of=None, doctor=None, eps=None, active_space=None, time_sym=None, given=None):
    """every multiset of n_mc draws over the first n_var sources.  value_of(ids, counts) -> (value, n_connected) is a door (each of
    its samples is compared with the model's); without one the model itself (doctored or not) gives the values.
    Returns dict(mean, bound, rows=[(ids, counts, P, model Result, value, n_connected)], worst = largest |delta| / bound of a sample)"""
    var, co, e_var = given or space(c, n_var)           # given = (var, co, e_var): a list that is no prefix of the case's (eps with it)
    n_var = len(var)
    eps_pt, eps_big = eps or thresholds(c, n_var)
    ts = c.ts if time_sym is None else time_sym
    rows, worst = [], 0.0
    for ids, counts, P in PS.expectation(co, n_mc):
        res = PS.sample(c.H, var, co, ids, counts, e_var, eps_pt, eps_big, n_mc, active_space=active_space, time_sym=ts, z=c.z)
        if value_of is not None:
            v, n = value_of(ids, counts)
            fails, ratio = PS.compare(res, v, n)
            assert not fails, (c.which, n_var, n_mc, ids, counts, fails)
            worst = max(worst, ratio)
        elif doctor is not None:
            d = PS.sample(c.H, var, co, ids, counts, e_var, eps_pt, eps_big, n_mc, active_space=active_space, time_sym=ts, z=c.z, doctor=doctor)
            v, n = d.value, d.n_connected
        else:
            assert not res.borderline, res.borderline[:3]
            v, n = res.value, res.n_connected
        rows.append((ids, counts, P, res, v, n))
    assert abs(math.fsum(r[2] for r in rows) - 1.0) <= (n_mc * (n_var + 2) + 2) * U
    mean, bound = PS.fold([r[2] for r in rows], [r[4] for r in rows], [r[3].bound for r in rows], [r[3].A for r in rows], n_var, n_mc)
    return dict(mean=mean, bound=bound, rows=rows, worst=worst, var=var, co=co, e_var=e_var, eps=(eps_pt, eps_big))


def check_unbiased(c, n_var, n_mc, value_of=None, label="model", **kw):
    """sum P value against the brute-force difference, within the summed bounds; returns (the run, |delta| / bound)"""
    run = exhaustive(c, n_var, n_mc, value_of, **kw)
    want, wb = reference_difference(c, run["var"], run["co"], run["e_var"], *run["eps"])
    ratio = abs(run["mean"] - want) / (run["bound"] + wb)
    print("%s %s (n_var %d, n_mc %d): %d samples, sum P value %.15g, PT2(eps_pt) - PT2(eps_pt_big) %.15g, |delta| / bound = %.3g, worst sample %.3g" % (
        c.which, label, n_var, n_mc, len(run["rows"]), run["mean"], want, ratio, run["worst"]))
    assert abs(run["mean"] - want) <= run["bound"] + wb, (c.which, n_var, n_mc, run["mean"], want, run["bound"], wb)
    return run, ratio


def preconditions(c):
    """what the (5, 4) case must hold so that the comparisons have something to see; on the model alone"""
    var, co, _ = space(c, 5)
    tb = PS.table(c.H, var, co, c.eps[0], None, c.ts, c.z)
    out = ~tb.row_inside
    reach = {}
    for k, s in zip(tb.kid[out].tolist(), tb.src[out].tolist()):
        reach.setdefault(k, set()).add(s)
    assert any(len(s) >= 2 for s in reach.values()), "no outside determinant is reached from two sources"
    ax = np.abs(tb.x[out])
    assert (ax < c.eps[1]).any() and (ax > c.eps[1]).any(), "no path between the thresholds, or none above both"
    assert tb.row_inside.any(), "no path lands inside the variational list"
    assert not tb.borderline


@pytest.mark.parametrize("which", ["c2_walk", "heg14"])
def test_model_is_unbiased(request, which):
    sysm = request.getfixturevalue(which)
    c = TH.build_case(sysm, which)
    t0 = time.time()
    preconditions(c)
    for n_var, n_mc in SHAPES:
        check_unbiased(c, n_var, n_mc)
    print("%s: checker %.1f s" % (which, time.time() - t0))


class HostAdapter:
    """what host.pt2_stochastic_sample_host asks of a context, answered by the oracle's door"""

    def __init__(self, door):
        self.d = door

    def hci_connections(self, up, dn, c, eps, diag_mode=0):
        return self.d.connections(up, dn, c, eps, diag_mode)

    def hamiltonian_batch(self, au, ad, bu, bd):
        return np.array([self.d.element((int(a), int(b)), (int(p), int(q))) for a, b, p, q in zip(au, ad, bu, bd)], float)


@pytest.mark.parametrize("which", ["c2_walk", "heg14"])
def test_host_path_agrees_with_the_model(request, oracle, which):
    """the numpy evaluation the GPU tests of the plan lean on, with the CPU oracle's generator and elements under it"""
    from sqmc_amd import host
    sysm = request.getfixturevalue(which)
    c = TH.build_case(sysm, which)
    g = HostAdapter(TH.OracleDoor(oracle, sysm))
    t0 = time.time()
    for n_var, n_mc in SHAPES:
        var, co, e_var = space(c, n_var)
        u, d = TH.arrays(var)
        coa = np.array(co)
        prob = np.abs(coa) / np.abs(coa).sum()
        eps_pt, eps_big = thresholds(c, n_var)

        def host_sample(ids, counts):
            return host.pt2_stochastic_sample_host(g, u, d, coa, prob, np.array(ids) + 1, np.array(counts), e_var, eps_pt, eps_big, n_mc)
        check_unbiased(c, n_var, n_mc, host_sample, "host path")
    print("%s: %.1f s" % (which, time.time() - t0))


MUST_CHANGE_COUNT = ("keep_var", "split_run")
# On HEG14 every path between two members of the list, and every path of the longest run, lies above both thresholds, so in the
# difference the terms they touch cancel exactly; those two mistakes are judged on the full estimator (eps_pt_big above everything,
# expectation hci_checker.pt2(eps_pt)) instead.
FULL_CASE = {"keep_var": "full", "split_run": "full"}


def test_doctored_models_are_rejected(request):
    """every mistake moves the expectation, and at least one single sample, by more than 100 times the bound of the comparison
    it would have to pass; those that add or lose a determinant change n_connected too"""
    sysm = request.getfixturevalue("heg14")
    c = TH.build_case(sysm, "heg14")
    t0 = time.time()
    cases = {}
    for name, eps in (("difference", thresholds(c, 5)), ("full", (c.eps[0], above_everything(c, 5)))):
        good = exhaustive(c, 5, 4, eps=eps)
        want, wb = reference_difference(c, good["var"], good["co"], good["e_var"], *good["eps"])
        assert abs(good["mean"] - want) <= good["bound"] + wb
        cases[name] = (eps, good, want, good["bound"] + wb)
    for doctor in PS.DOCTORS:
        eps, good, want, allowed = cases[FULL_CASE.get(doctor, "difference")]
        bad = exhaustive(c, 5, 4, doctor=doctor, eps=eps)
        moved = abs(bad["mean"] - want) / allowed
        single = max(abs(b[4] - g[3].value) / g[3].bound for b, g in zip(bad["rows"], good["rows"]) if g[3].bound > 0)
        counts = sum(b[5] != g[3].n_connected for b, g in zip(bad["rows"], good["rows"]))
        print("%-12s expectation moved by %.3g bounds, the most affected sample by %.3g bounds, n_connected differs in %d of %d samples" % (
            doctor, moved, single, counts, len(bad["rows"])))
        assert moved > POWER and single > POWER, doctor
        if doctor in MUST_CHANGE_COUNT:
            assert counts > 0, doctor
    print("doctored models: %.1f s" % (time.time() - t0))


def time_sym_bias(c, n_var=5, n_mc=4):
    """the expectation of the model on unmerged time-symmetric raw paths against hci_checker.pt2(time_sym=True) differences:
    (bias, bound)"""
    run = exhaustive(c, n_var, n_mc)
    want, wb = reference_difference(c, run["var"], run["co"], run["e_var"], *run["eps"])
    return run["mean"] - want, run["bound"] + wb, run


def test_time_symmetry_biases_the_estimator(request):
    """c2_hci: sources that are time-reversal representatives, raw paths unmerged as the generator's raw mode returns them.  The
    expectation misses the deterministic difference by -1.205e-05 against a bound of 2.9e-13 (4.15e+07 bounds): a plan on a time_sym context would be biased, so prepare
    refuses one (tests/test_gpu_pt2s_edges.py pins the refusal)."""
    sysm = request.getfixturevalue("c2_hci")
    c = TH.build_case(sysm, "c2_hci")
    assert c.ts
    t0 = time.time()
    bias, bound, run = time_sym_bias(c)
    var, co, _ = space(c, 5)
    tb = PS.table(c.H, var, co, c.eps[0], None, True, c.z)
    pairs = {}
    for k, s in zip(tb.kid[~tb.row_inside].tolist(), tb.src[~tb.row_inside].tolist()):
        pairs[(k, s)] = pairs.get((k, s), 0) + 1
    twice = sum(1 for v in pairs.values() if v > 1)
    print("c2_hci time_sym: sum P value %.15g, bias %.6g, bound %.3g, bias / bound = %.3g; %d (source, determinant) pairs joined by two raw paths; %.1f s" % (
        run["mean"], bias, bound, abs(bias) / bound, twice, time.time() - t0))
    assert twice > 0
    assert abs(bias) > POWER * bound
