"""The samples of the semistochastic PT2 (second_order_pt_alias, hci.f90:1314-1660) evaluated by the library
(sqmc_gpu_hci_pt2_stochastic_prepare / _sample / _free, host.hci_pt2_stochastic(on_device=True), run_hci(pt_on_device=True))
against the reference's printed samples, against the numpy evaluation of the same samples, and on their own terms
(same bits run to run, buffers reused, refusals)."""
import copy
import io
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = (2726, 5165, 6543, 6524)
U52 = 2.0 ** -52


def _draws(H, c, n_mc, seed=SEED):
    """the merged draws of successive samples, as hci_pt2_stochastic makes them: yields (ids 1-based ascending, counts)"""
    prob = np.abs(c) / np.abs(c).sum()
    J, q = H.setup_alias(prob)
    rng = H.Rannyu(seed)
    n = len(c)
    while True:
        d = np.empty(n_mc, np.int64)
        for k in range(n_mc):
            i = rng.random_int(n)
            d[k] = i if rng.rannyu() < q[i - 1] else J[i - 1]
        yield np.unique(d, return_counts=True)


def _chain(n_raw, n_terms):
    """K of the bound |device - host| <= K 2^-52 A: the longest chain of additions either side puts between a term and the sum.

    Both sides form every term (term1^2 + term2 - term1_big^2 - term2_big) / (E_var - H_kk) by the same operations in the same
    order from the same inputs (the library is built without floating-point contraction; w/p is computed by the same IEEE
    division from the same p; within a connected determinant both add left to right in generation order), so only the sum over
    the terms differs.  A sum whose longest chain has L additions is within L 2^-53 sum|term| of the exact one to first order,
    so two such sums differ by at most (L_dev + L_host) 2^-53 sum|term| <= max(L_dev, L_host) 2^-52 A.

    Device (k_pt2s_terms + k_pt2s_final over n_raw sorted raw connections, nb = min(ceil(n_raw / 256), 1024) blocks):
      ceil(n_raw / (256 nb)) grid-stride additions per thread (the first onto 0), 6 shuffle levels per wavefront, 4 wavefront
      partials per block, ceil(nb / 64) block partials per lane of the finishing wavefront, 6 shuffle levels.
    Host (numpy's sum over n_terms terms): pieces of 8192 added left to right (ceil(n_terms / 8192) - 1 additions), each piece
      halved down to leaves of at most 128 (ceil(log2(8192 / 128)) = 6 levels at most), a leaf in 8 accumulators of at most
      15 additions each, 3 levels to combine them and at most 7 trailing additions."""
    nb = min(-(-n_raw // 256), 1024)
    dev = -(-n_raw // (256 * nb)) + 6 + 4 + -(-nb // 64) + 6
    piece = min(max(n_terms, 1), 8192)
    host = (-(-n_terms // 8192) - 1) + max(0, math.ceil(math.log2(piece / 128.0))) + 15 + 3 + 7
    return max(dev, host)


def _abs_sum(parts, e_var, n_mc):
    """A = sum_k (term1^2 + |term2| + term1_big^2 + |term2_big|) / |E_var - H_kk| / (n_mc (n_mc - 1)) from the host path's arrays"""
    t1, t2, t1b, t2b, h = (parts[k] for k in ("t1", "t2", "t1b", "t2b", "h_kk"))
    return float(np.sum((t1 * t1 + np.abs(t2) + t1b * t1b + np.abs(t2b)) / np.abs(e_var - h))) / (n_mc * float(n_mc - 1))


def _compare_samples(H, g, plan, up, dn, c, e_var, eps_pt, eps_pt_big, n_mc, n_samples, label):
    """n_samples samples of one stream through the plan and through numpy: equal counts, values within K 2^-52 A.
    Returns (device values, host values, per-sample dicts with A, K, raw count)."""
    prob = np.abs(c) / np.abs(c).sum()
    dev, host, info = [], [], []
    worst, longest = 0.0, 0
    for s, (ids, counts) in zip(range(n_samples), _draws(H, c, n_mc)):
        parts = {}
        vh, nh = H.pt2_stochastic_sample_host(g, up, dn, c, prob, ids, counts, e_var, eps_pt, eps_pt_big, n_mc, parts=parts)
        vd, nd = plan.sample(ids - 1, counts)
        raw = plan.stats()["last_raw"]
        A, K = _abs_sum(parts, e_var, n_mc), _chain(raw, nh)
        run = int(np.diff(np.append(parts["starts"], parts["n_kept"])).max()) if nh else 0
        longest = max(longest, run)
        ratio = abs(vd - vh) / (U52 * A) if A > 0 else 0.0
        worst = max(worst, ratio)
        print("%s sample %3d: raw %8d connected %8d longest run %3d device %.17g host %.17g |d-h|/(2^-52 A) %.3f K %d"
              % (label, s + 1, raw, nh, run, vd, vh, ratio, K))
        dev.append(vd); host.append(vh); info.append(dict(A=A, K=K, raw=raw, nd=nd, nh=nh, ratio=ratio))
    print("%s: largest |device - host| / (2^-52 A) = %.3f over %d samples, longest run %d" % (label, worst, n_samples, longest))
    for s, i in enumerate(info):
        assert i["nd"] == i["nh"], (label, s, i)
        assert abs(dev[s] - host[s]) <= i["K"] * U52 * i["A"], (label, s, dev[s], host[s], i)
    return dev, host, info


@pytest.fixture(scope="module")
def heg():
    """the reference's e2e electron gas: 14 electrons, r_s 0.5, cutoff 1.49, eps_var 1e-3 (9475 determinants), sorted"""
    from sqmc_amd import host as H
    hst = H.HegHost(3, 0.5, 14, 7, 1.49)
    g = hst.gpu()
    up, dn, w, e, hist = H.hci_variational(hst, g, 1e-3, n_states=1)
    assert hist == [1, 277, 9475]
    o = H.sort_dets(up, dn)
    yield dict(H=H, host=hst, g=g, up=np.ascontiguousarray(up[o]), dn=np.ascontiguousarray(dn[o]), c=np.ascontiguousarray(w[o, 0]), e=float(e[0]))
    g.close()


@pytest.fixture(scope="module")
def heg_device_run(heg):
    H = heg["H"]
    return H.hci_pt2_stochastic(heg["host"], heg["g"], heg["up"], heg["dn"], heg["c"], heg["e"], 2e-7, 8.1920e-4, 200, 1e-5, seed=SEED, max_samples=400,
                                on_device=True)


@pytest.fixture(scope="module")
def c2():
    """C2, eps_var 2e-3, expanded to the determinant basis on a context without time-reversal symmetry, sorted"""
    from conftest import FCIDUMP
    from sqmc_amd import host as H
    h = H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=1, hf_symmetry=1)
    g = h.gpu()
    g.set_hb_tables(*h.hb_tables(g))
    up, dn, w, e, hist = H.hci_variational(h, g, 2e-3, n_states=1)
    g.close()
    plain = copy.copy(h); plain.time_sym = False
    du, dd, dc = H.time_symmetrized_to_dets(up, dn, w[:, 0], h.z)
    o = H.sort_dets(du, dd)
    gp = plain.gpu()
    gp.set_hb_tables(*plain.hb_tables(gp))
    yield dict(H=H, host=plain, g=gp, up=np.ascontiguousarray(np.asarray(du, np.uint64)[o]), dn=np.ascontiguousarray(np.asarray(dd, np.uint64)[o]),
               c=np.ascontiguousarray(np.asarray(dc, float)[o]), e=float(e[0]))
    gp.close()


def test_heg_reference_samples_on_the_device_path(heg, heg_device_run):
    """o_st_ref of the reference's e2e directory, as test_heg_semistochastic_pt_reproduces_reference_samples holds the host path
    to it: first five samples and the last, 143 samples, pt_diff and its error bar, the total."""
    res, e = heg_device_run, heg["e"]
    ref5 = [-0.000628947, -0.000488905, -0.000786277, -0.000940695, -0.000707866]
    print("samples %d first5 %r last %.12f pt_big %.12f pt_diff %.12f +- %.12f total %.12f"
          % (len(res["samples"]), res["samples"][:5], res["samples"][-1], res["pt_big"], res["pt_diff"], res["pt_diff_std_dev"], e + res["pt_big"] + res["pt_diff"]))
    assert all(abs(a - b) < 1.5e-9 for a, b in zip(res["samples"][:5], ref5))
    assert len(res["samples"]) == 143 and abs(res["samples"][-1] - (-0.000829319)) < 1.5e-9
    assert abs(res["pt_big"] - (-0.000199339)) < 2e-9
    assert abs(res["pt_diff"] - (-0.000729402)) < 2e-9 and abs(res["pt_diff_std_dev"] - 0.000009966) < 2e-9
    assert abs(e + res["pt_big"] + res["pt_diff"] - 58.275977344) < 3e-9


def test_heg_device_against_host_sample_by_sample(heg, heg_device_run):
    """every one of the 143 samples: the same number of connected determinants, values within K 2^-52 A (_chain); the host
    function as a whole (on_device=False) gives the values of the per-sample host evaluation, the device one those of the plan"""
    from sqmc_amd import Pt2StochasticPlan
    H, g = heg["H"], heg["g"]
    res_host = H.hci_pt2_stochastic(heg["host"], g, heg["up"], heg["dn"], heg["c"], heg["e"], 2e-7, 8.1920e-4, 200, 1e-5, seed=SEED, max_samples=400)
    assert len(res_host["samples"]) == 143
    with Pt2StochasticPlan(g, heg["up"], heg["dn"], heg["c"], heg["e"], 2e-7, 8.1920e-4, 200) as plan:
        dev, host, info = _compare_samples(H, g, plan, heg["up"], heg["dn"], heg["c"], heg["e"], 2e-7, 8.1920e-4, 200, 143, "heg")
    assert host == res_host["samples"] and [i["nh"] for i in info] == res_host["samples_connected"]
    assert dev == heg_device_run["samples"] and [i["nd"] for i in info] == heg_device_run["samples_connected"]


def test_c2_device_against_host_sample_by_sample(c2):
    """the chemistry run of test_semistochastic_pt_chem_agrees_with_deterministic (eps_pt 1e-6, eps_pt_big 2e-4, n_mc 300): 60 samples"""
    from sqmc_amd import Pt2StochasticPlan
    with Pt2StochasticPlan(c2["g"], c2["up"], c2["dn"], c2["c"], c2["e"], 1e-6, 2e-4, 300) as plan:
        _compare_samples(c2["H"], c2["g"], plan, c2["up"], c2["dn"], c2["c"], c2["e"], 1e-6, 2e-4, 300, 60, "c2")


def test_c2_statistics_on_the_device_path(c2):
    """as the chemistry test of the host path: pt_big is hci_pt2 at eps_pt_big, and pt_big + pt_diff agrees with the deterministic
    PT at eps_pt within 4 of its own error bars"""
    H, g = c2["H"], c2["g"]
    det, _ = H.hci_pt2(c2["host"], g, c2["up"], c2["dn"], c2["c"], c2["e"], 1e-6)
    big, _ = H.hci_pt2(c2["host"], g, c2["up"], c2["dn"], c2["c"], c2["e"], 2e-4)
    r = H.hci_pt2_stochastic(c2["host"], g, c2["up"], c2["dn"], c2["c"], c2["e"], 1e-6, 2e-4, 300, 1e-4, max_samples=2000, on_device=True)
    print("c2: %d samples, pt_big %.12f (hci_pt2 %.12f), pt_big + pt_diff %.9f +- %.9f, deterministic %.9f"
          % (len(r["samples"]), r["pt_big"], big, r["pt_big"] + r["pt_diff"], r["pt_diff_std_dev"], det))
    assert abs(r["pt_big"] - big) < 1e-14
    assert r["pt_diff_std_dev"] <= 1e-4 * 1.0001 and len(r["samples"]) >= 10
    assert abs(r["pt_big"] + r["pt_diff"] - det) < 4 * r["pt_diff_std_dev"]


def test_c2_active_space_modes(c2):
    """generator masks (lowest orbital core, last 8 virtual) in modes 1 and 2, twenty samples each: device = host within the bound,
    and since the two modes partition the connected determinants, a sample's mode-1 and mode-2 values add up to the unmasked one
    (one more addition in the chain)"""
    from sqmc_amd import Pt2StochasticPlan
    H, g = c2["H"], c2["g"]
    norb = c2["host"].norb
    core, virt = 1, ((1 << norb) - 1) ^ ((1 << (norb - 8)) - 1)
    out = {}
    try:
        with Pt2StochasticPlan(g, c2["up"], c2["dn"], c2["c"], c2["e"], 1e-6, 2e-4, 300) as plan:
            for mode in (0, 1, 2):
                g.hci_set_active_space(core, core, virt, virt, mode)
                out[mode] = _compare_samples(H, g, plan, c2["up"], c2["dn"], c2["c"], c2["e"], 1e-6, 2e-4, 300, 20, "c2 mode %d" % mode)
    finally:
        g.hci_set_active_space(0, 0, 0, 0, 0)
    worst = 0.0
    for s in range(20):
        i0, i1, i2 = out[0][2][s], out[1][2][s], out[2][2][s]
        assert i1["nd"] > 0 and i2["nd"] > 0 and i1["nd"] + i2["nd"] == i0["nd"]
        diff = abs(out[1][0][s] + out[2][0][s] - out[0][0][s])
        worst = max(worst, diff / (U52 * i0["A"]))
        assert diff <= (i0["K"] + 1) * U52 * i0["A"], (s, diff, i0)
    print("c2 active space: largest |mode1 + mode2 - mode0| / (2^-52 A) = %.3f" % worst)


def test_same_bits_run_to_run(heg):
    """a sample evaluated twice on one plan (with another in between) and on a second plan from the same inputs"""
    from sqmc_amd import Pt2StochasticPlan
    H, g = heg["H"], heg["g"]
    gen = _draws(H, heg["c"], 200)
    (ids_a, cnt_a), (ids_b, cnt_b) = next(gen), next(gen)
    with Pt2StochasticPlan(g, heg["up"], heg["dn"], heg["c"], heg["e"], 2e-7, 8.1920e-4, 200) as p1, \
            Pt2StochasticPlan(g, heg["up"], heg["dn"], heg["c"], heg["e"], 2e-7, 8.1920e-4, 200) as p2:
        a1 = p1.sample(ids_a - 1, cnt_a); b1 = p1.sample(ids_b - 1, cnt_b); a1_again = p1.sample(ids_a - 1, cnt_a)
        b2 = p2.sample(ids_b - 1, cnt_b); a2 = p2.sample(ids_a - 1, cnt_a)
    assert a1[0] != b1[0]
    assert np.float64(a1[0]).tobytes() == np.float64(a1_again[0]).tobytes() == np.float64(a2[0]).tobytes() and a1[1] == a1_again[1] == a2[1]
    assert np.float64(b1[0]).tobytes() == np.float64(b2[0]).tobytes() and b1[1] == b2[1]


def test_buffers_are_reused(heg):
    """the plan's allocation counter (sqmc_gpu_hci_pt2_stochastic_stats): after the first ten samples of the HEG run the connection
    buffers are reallocated only by a sample with more raw connections than every earlier one"""
    from sqmc_amd import Pt2StochasticPlan
    H, g = heg["H"], heg["g"]
    with Pt2StochasticPlan(g, heg["up"], heg["dn"], heg["c"], heg["e"], 2e-7, 8.1920e-4, 200) as plan:
        assert plan.stats()["n_alloc"] == 0
        seen, allocs, grown_late = 0, 0, 0
        for s, (ids, counts) in zip(range(60), _draws(H, heg["c"], 200)):
            plan.sample(ids - 1, counts)
            st = plan.stats()
            assert st["n_samples"] == s + 1 and st["capacity"] >= st["last_raw"] > 0
            if st["n_alloc"] != allocs:
                assert st["n_alloc"] == allocs + 1 and st["last_raw"] > seen, (s, st, seen)
                grown_late += s >= 10
            allocs, seen = st["n_alloc"], max(seen, st["last_raw"])
        print("buffers: %d allocations over 60 samples (%d after the tenth), capacity %d, largest sample %d" % (allocs, grown_late, st["capacity"], seen))
        assert 1 <= allocs <= 10


def test_refusals_leave_the_plan_usable(heg):
    from sqmc_amd import Pt2StochasticPlan, SqmcGpuError
    H, g = heg["H"], heg["g"]
    up, dn, c, e = heg["up"], heg["dn"], heg["c"], heg["e"]
    ids, counts = next(_draws(H, c, 200))
    with Pt2StochasticPlan(g, up, dn, c, e, 2e-7, 8.1920e-4, 200) as plan:
        good = plan.sample(ids - 1, counts)

        def refused(fn, word):
            with pytest.raises(SqmcGpuError) as ei:
                fn()
            assert ei.value.code != 0 and word in str(ei.value), str(ei.value)
            again = plan.sample(ids - 1, counts)
            assert np.float64(again[0]).tobytes() == np.float64(good[0]).tobytes() and again[1] == good[1]

        swapped = np.arange(len(up)); swapped[[3, 4]] = [4, 3]
        refused(lambda: Pt2StochasticPlan(g, up[swapped], dn[swapped], c[swapped], e, 2e-7, 8.1920e-4, 200), "sorted")
        refused(lambda: Pt2StochasticPlan(g, up, dn, c, e, 2e-7, 8.1920e-4, 1), "n_mc")
        bad = (ids - 1).copy(); bad[-1] = len(up)
        refused(lambda: plan.sample(bad, counts), "out of range")
        bad = (ids - 1).copy(); bad[0] = -1
        refused(lambda: plan.sample(bad, counts), "out of range")
        bad = (ids - 1).copy(); bad[[0, 1]] = bad[[1, 0]]
        refused(lambda: plan.sample(bad, counts), "ascending")
        bad = counts.copy(); bad[2] = 0
        refused(lambda: plan.sample(ids - 1, bad), "count")
        hub = H.HubbardHost(4, 4, True, 8, 8).gpu()
        try:
            refused(lambda: Pt2StochasticPlan(hub, [0x00FF], [0xFF00], [1.0], -1.0, 1e-6, 1e-4, 10), "hubbard2")
        finally:
            hub.close()


def test_deck_runner_switch():
    """tests/golden/heg_e2e_i_st through run_hci: with the switch the totals of test_reference_e2e_heg_decks_run_unchanged; without
    it the printed text is that of a call that does not mention it"""
    from sqmc_amd import run as R
    deck = R.parse_hci_deck(open(os.path.join(os.path.dirname(__file__), "golden", "heg_e2e_i_st")).read())
    texts = []
    for kw in ({}, {"pt_on_device": False}, {"pt_on_device": True}):
        buf = io.StringIO()
        res = R.run_hci(copy.deepcopy(deck), out=buf, **kw)
        texts.append(buf.getvalue())
    assert texts[0] == texts[1] and "Sample, E_2pt_now" in texts[0]
    assert res["hist"] == [1, 277, 9475] and abs(res["e_var"] - 58.276906085) < 2e-9
    assert res["n_samples"] == 143
    assert abs(res["pt"] - (-0.000928741)) < 2e-9 and abs(res["pt_err"] - 0.000009966) < 2e-9
    assert abs(res["e_total"] - 58.275977344) < 3e-9 and abs(res["e_total"] + res["madelung"] - 48.051823875) < 3e-9
    lines_host, lines_dev = texts[0].splitlines(), texts[2].splitlines()
    assert len(lines_host) == len(lines_dev)
