"""The walk's spawn-weight histograms and max / min weight ratios (sqmc_gpu_set_spawn_diagnostics; do_walk.f90:3295-3320, 3619-3661,
7603-7636) on the GPU: walks are untouched by them, one REPLAY step against the serial stream replayed through the proposal entries
that are not the code under test, exact integer bin edges on the Hubbard lattice, the first moment against an independent H,
once-per-step counting (chained runs, a tail that gives up, two ranks), and the deck runner's tables.  The bin model and the
formatter's twin are tests/spawn_hist_checker.py; departures from the reference are listed in tests/golden/README_spawn_hist.md."""
import ctypes as C
import functools
import io
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from conftest import gpu_ctx_from_oracle, gpu_ctx_heg, gpu_ctx_hub          # noqa: E402
from tests import proposal_checker as PC                                    # noqa: E402
from tests import hubbardk_checker as HK                                    # noqa: E402
from tests import cauchy_checker as CC                                      # noqa: E402
from tests import spawn_hist_checker as SH                                  # noqa: E402
from tests import test_proposal_unbiased as TU                              # noqa: E402

pytestmark = pytest.mark.gpu
FCIDUMP = TU.FCIDUMP
SEED = (1346, 5634, 6635, 4361)
TAU = TU.TAU
HISTS = ("bins", "bins_hf", "bins_single", "bins_double")
WALKER_KEYS = ("up", "dn", "wt", "imp_distance", "initiator", "matrix_elements", "e_num", "e_den")


def _walkers(up, dn, wt):
    n = len(up)
    return dict(up=np.asarray(up, np.uint64), dn=np.asarray(dn, np.uint64), wt=np.asarray(wt, np.float64), imp_distance=np.ones(n, np.int8),
                initiator=np.full(n, 2, np.int8), perm_sign=np.zeros(n, np.int8), matrix_elements=np.full(n, 1e51), e_num=np.full(n, 1e51),
                e_den=np.full(n, 1e51))


def _plain_params(tau, e_trial, min_wt=0.5, cutoff=0.5):
    return dict(tau=tau, e_trial=e_trial, reweight_factor_inv=1.0, r_initiator=0.0, min_wt=min_wt, always_spawn_cutoff_wt=cutoff, initiator_power=0,
                initiator_min_distance=0, c_t_initiator=0, semistochastic=0, reached_w_abs_gen=0)


def _nint(a):
    return int(math.floor(abs(a) + 0.5))


def _n_proposals(wt):
    """children of a list without gated walkers (always_spawn_cutoff_wt = 0: no |w| lies below it): max(nint|w|, 1) each (do_walk.f90:3588)"""
    return int(sum(max(_nint(w), 1) for w in np.asarray(wt, np.float64).tolist()))


def _same_diag(a, b):
    for k in HISTS:
        assert np.array_equal(a[k], b[k]), (k, np.nonzero(a[k] != b[k])[0][:10])
    assert np.array_equal(a["max_ratio_by_level"], b["max_ratio_by_level"]), (a["max_ratio_by_level"], b["max_ratio_by_level"])
    for k in ("max_ratio", "max_ratio_level", "min_ratio", "n_nan"):
        assert a[k] == b[k], (k, a[k], b[k])


# ------------------------------------------------------------------------------------------------ 1. on equals off
@functools.lru_cache(maxsize=None)
def _host(name):
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    if name == "c2":
        return H.ChemHost(FCIDUMP, 8, 4, "d2h")
    if name == "c2_ts":
        return H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=1, hf_symmetry=1)
    if name == "c2_10e":
        return H.ChemHost(FCIDUMP, 10, 5, "d2h")
    if name == "heg14":
        return H.HegHost(3, 0.5, 14, 7, 1.49)
    if name == "hub44":
        return H.HubbardHost(4, 4, True, 8, 8, 1.0, 4.0)
    return H.HubbardKHost(4, 3, 2, 2, 1.0, 4.0)


WALKS = {
    "c2_uniform": ("c2", dict()),
    "c2_cauchy": ("c2", dict(proposal="cauchyschwarz")),
    "c2_cauchy_ts": ("c2_ts", dict(proposal="cauchyschwarz")),
    "c2_10e_heatbath": ("c2_10e", dict(proposal="heatbath")),
    "heg14": ("heg14", dict(size_deterministic=250, n_truncate_trial_wf=1)),
    "hub44": ("hub44", dict(size_deterministic=500, n_truncate_trial_wf=20, tau_multiplier=0.5)),
    "hubbardk43": ("hubbardk43", dict(size_deterministic=30, n_truncate_trial_wf=20, tau_multiplier=0.5)),
    "c2_replay": ("c2", dict(rng_mode=0)),
    "c2_psit": ("c2", dict(hf_to_psit=True)),
}


def _walk(case, diag, w_target=4000.0, w_begin=2000.0):
    from sqmc_amd import host as H
    hname, kw = WALKS[case]
    return H.GpuWalk(_host(hname), w_target, w_begin=w_begin, seed=SEED, mwalk=400000, spawn_diagnostics=diag, **kw)


def _trajectory(case, diag, nsteps=30):
    w = _walk(case, diag)
    try:
        outs, lists = [], []
        for _ in range(nsteps):
            outs.append(w.step().copy())
            lists.append(w.g.download_walkers())
        return np.array(outs), lists, (w.spawn_diagnostics() if diag else None), w.g.tail_stats()
    finally:
        w.close()


@pytest.mark.parametrize("case", sorted(WALKS))
def test_on_equals_off(case):
    """30 steps with the diagnostics on and off: the walker list after every step and the 16 sums of every step are bit-identical,
    and the histogram holds one entry per child (per slot that holds a move with fast_heatbath: between one and two per child)"""
    o_on, l_on, diag, tail = _trajectory(case, True)
    o_off, l_off, _, tail_off = _trajectory(case, False)
    assert np.array_equal(o_on, o_off)
    for k, (a, b) in enumerate(zip(l_on, l_off)):
        for key in WALKER_KEYS:
            assert np.array_equal(a[key], b[key]), (k, key)
    assert tail == tail_off
    nch = int(o_on[:, 15].sum())
    tot = int(diag["bins"].sum())
    print("%s: %d children, %d histogram entries, max ratio %.6g at level %d, min %.6g, bucket steps %d" %
          (case, nch, tot, diag["max_ratio"], diag["max_ratio_level"], diag["min_ratio"], tail[0]))
    if WALKS[case][1].get("proposal") == "heatbath":
        assert nch <= tot <= 2 * nch
    else:
        assert tot == nch
    assert diag["n_nan"] == 0 and diag["max_ratio"] > diag["min_ratio"] > 1e-9
    if case == "c2_psit":
        assert diag["bins_hf"].sum() == 0          # hf_to_psit: slot 0 proposes nothing (do_walk.f90:3574)
    if case == "c2_uniform" and os.environ.get("SQMC_BUCKET") != "0":
        assert tail[0] > 0           # the short-list form of k_spawn (fused partition) ran


def test_on_equals_off_inside_run_and_chained():
    """The same through sqmc_gpu_run with chained runs past the target population, where the walk without diagnostics enqueues every
    step's head ahead of it and the walk with them runs un-pipelined: sums of every step and the final list bit for bit."""
    res = []
    for diag in (True, False):
        w = _walk("c2_uniform", diag, w_target=2500.0, w_begin=3000.0)
        try:
            w.g.set_chained_runs(True)
            st = np.concatenate([w.run(n)[0] for n in (20, 1, 9)])
            assert w.pc.reached == 2
            w.g.set_chained_runs(False)
            res.append((st, w.g.download_walkers(), w.spawn_diagnostics() if diag else None))
        finally:
            w.close()
    assert np.array_equal(res[0][0], res[1][0])
    for key in WALKER_KEYS:          # the cached H_ii and local-energy terms included: the same entries are filled, with the same bits
        assert np.array_equal(res[0][1][key], res[1][1][key]), key
    assert int((res[0][1]["matrix_elements"] < 1e50).sum()) > len(res[0][1]["up"]) // 2
    assert int(res[0][2]["bins"].sum()) == int(res[0][0][:, 15].sum())


def _pytest_self(keyword, env):
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider", "-k", keyword],
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ, **env))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    return r.stdout


def test_plain_spawn_form_on_equals_off():
    """SQMC_BUCKET=0 (read once per process): every step launches the plain form of k_spawn, k_spawn<., 0, .>"""
    out = _pytest_self("test_on_equals_off and (c2_uniform or heg14 or hub44)", dict(SQMC_BUCKET="0"))
    assert "3 passed" in out, out[-2000:]


# ------------------------------------------------------------------------------------------------ 2. exact replay
def _pool(connected, start, n):
    """n distinct determinants around `start`, in (up, dn) order"""
    seen = {start}
    frontier = [start]
    while len(seen) < n + 50 and frontier:
        nxt = []
        for u, d in frontier[:40]:
            for c in connected(u, d):
                if c not in seen:
                    seen.add(c); nxt.append(c)
        frontier = nxt
    dets = sorted(seen)
    step = max(len(dets) // n, 1)
    return dets[::step][:n]


def _replay_weights(n):
    """0.5 .. 7.3, both signs; none below always_spawn_cutoff_wt = 0.5, so the gate draws nothing"""
    w = np.linspace(0.5, 7.3, n)
    w[1::3] *= -1.0
    return w


def _oracle_connected(sysm):
    def f(u, d):
        cu, cd, _ = sysm.connected(int(u), int(d), with_elems=False)
        return list(zip([int(x) for x in cu], [int(x) for x in cd]))
    return f


@pytest.fixture(scope="module")
def c2_10e(oracle):
    return oracle.ChemSystem(FCIDUMP, 10, 5, "d2h", time_sym=False, hf_mode=0)


@pytest.mark.parametrize("case", ["chem", "heg", "hubbard", "heatbath"])
def test_replay_step_matches_the_serial_stream(request, oracle, case):
    """One RNG_REPLAY step from 200 uploaded walkers, |w| from 0.5 to 7.3: the test walks the single rannyu stream itself -- walker by
    walker, child by child, through the oracle's proposal entry -- and bins the returned weights with the checker's model.  All four
    histograms, the max ratio per level, the overall max with its level and the min ratio equal the device's bit for bit."""
    import sqmc_amd
    sqmc_amd.set_device(0)
    L = oracle.lib()
    hb = None
    if case == "chem":
        sysm, setup, tau = request.getfixturevalue("c2_walk"), request.getfixturevalue("c2_setup"), TAU["chem"]
        g = gpu_ctx_from_oracle(sysm, rng_mode=0, seed=SEED, mwalk=200000); fn = L.orc_off_diagonal_move_chem
    elif case == "heg":
        sysm, setup, tau = request.getfixturevalue("heg14"), request.getfixturevalue("heg_setup"), TAU["heg"]
        g = gpu_ctx_heg(sysm, rng_mode=0, seed=SEED, mwalk=200000); fn = L.orc_off_diagonal_move_heg
    elif case == "hubbard":
        sysm, setup, tau = request.getfixturevalue("hub44"), request.getfixturevalue("hub_setup"), TAU["hub"]
        g = gpu_ctx_hub(sysm, rng_mode=0, seed=SEED, mwalk=200000); fn = L.orc_off_diagonal_move_hubbard
    else:
        sysm, tau = request.getfixturevalue("c2_10e"), TAU["hb"]
        setup = oracle.setup_walk(sysm, 100, 1000, 0.1)
        hb = oracle.HeatBath(sysm)
        g = gpu_ctx_from_oracle(sysm, rng_mode=0, seed=SEED, mwalk=200000)
    try:
        if hb is not None:
            g.set_heatbath_tables(hb.fortran_arrays())
        g.set_ct_table(setup.ct_up, setup.ct_dn, setup.ct_num, setup.ct_den)
        dets = _pool(_oracle_connected(sysm), (int(sysm.hf_up), int(sysm.hf_dn)), 200)
        wt = _replay_weights(len(dets))
        assert len(dets) >= 150
        g.upload_walkers(_walkers([d[0] for d in dets], [d[1] for d in dets], wt))
        g.set_spawn_diagnostics(True)
        r = oracle.Rng()
        L.orc_setrn(C.byref(r), (C.c_int * 4)(*g.rng_state()))
        model = SH.Model(chem=case in ("chem", "heatbath"))
        nch = 0
        a, b, w, nd = C.c_uint64(), C.c_uint64(), C.c_double(), C.c_int()
        for slot, ((u, d), wi) in enumerate(zip(dets, wt.tolist())):
            for _ in range(max(_nint(wi), 1)):
                nch += 1
                if hb is None:
                    fn(sysm.h, C.byref(r), tau, u, d, C.byref(a), C.byref(b), C.byref(w), C.byref(nd))
                    model.add(slot, u, d, a.value, b.value, w.value, tau)
                else:
                    ju, jd, w2, lev = (C.c_uint64 * 2)(), (C.c_uint64 * 2)(), (C.c_double * 2)(), (C.c_int * 2)()
                    nn = L.orc_off_diagonal_move_chem_heatbath(sysm.h, hb.h, C.byref(r), tau, u, d, ju, jd, w2, lev, C.byref(nd))
                    model.add(slot, u, d, ju[0], jd[0], w2[0] if nn >= 1 else 0.0, tau)          # no move: one entry of 0
                    if nn == 2:
                        model.add(slot, u, d, ju[1], jd[1], w2[1], tau)
        out = g.step(_plain_params(tau, setup.e_trial0, min_wt=0.0))          # min_wt = 0: no rounding draws behind the proposals
        assert int(out[15]) == nch
        assert g.rng_state() == [r.l[k] for k in range(4)]
        got = g.spawn_diagnostics()
    finally:
        g.close()
        if hb is not None:
            hb.close()
    want = model.result()
    print("%s: %d proposals, %d bins occupied, max %.6g (level %d), min %.6g" % (case, nch, int((want["bins"] > 0).sum()), want["max_ratio"],
                                                                            want["max_ratio_level"], want["min_ratio"]))
    assert want["bins"].sum() >= nch and want["bins_hf"].sum() >= 1 and (want["bins"] > 0).sum() >= 2
    _same_diag(got, want)


def test_replay_step_matches_the_serial_stream_cauchy_schwarz():
    """the same with proposal_method CauchySchwarz: the moves from cauchy_checker.CSTables.move, weight_j = -tau H_ij / p"""
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    h = H.ChemHost(FCIDUMP, 8, 4, "d2h")
    cs = CC.from_host(h)
    tau = TAU["chem"]
    g = h.gpu(proposal="cauchyschwarz", rng_mode=sqmc_amd.RNG_REPLAY, seed=SEED, mwalk=200000)
    try:
        s = h.setup_walk(g, 100, 1000, 0.1)
        g.set_ct_table(s.ct_up, s.ct_dn, s.ct_num, s.ct_den)
        cu, cd = h.connected_all(h.hf_up, h.hf_dn)
        allc = sorted(set(zip(cu.tolist(), cd.tolist())) | {(int(h.hf_up), int(h.hf_dn))})
        dets = allc[::max(len(allc) // 200, 1)][:200]
        wt = _replay_weights(len(dets))
        g.upload_walkers(_walkers([d[0] for d in dets], [d[1] for d in dets], wt))
        g.set_spawn_diagnostics(True)
        r = CC.Rannyu(CC.limbs_state(g.rng_state()))
        recs = []
        for slot, ((u, d), wi) in enumerate(zip(dets, wt.tolist())):
            for _ in range(max(_nint(wi), 1)):
                lev, ju, jd, p = cs.move(u, d, r)
                recs.append((slot, u, d, ju, jd, lev, p))
        mv = [k for k, rec in enumerate(recs) if rec[5] > 0]
        hij = g.hamiltonian_chem_batch(*[np.array([recs[k][c] for k in mv], np.uint64) for c in (1, 2, 3, 4)])
        wj = np.zeros(len(recs))
        wj[mv] = [-tau * float(hv) / recs[k][6] for hv, k in zip(hij, mv)]
        model = SH.Model(chem=True)
        for (slot, u, d, ju, jd, lev, p), w in zip(recs, wj.tolist()):
            model.add(slot, u, d, ju, jd, w, tau)
        out = g.step(_plain_params(tau, s.e_trial0, min_wt=0.0))
        assert int(out[15]) == len(recs) and CC.limbs_state(g.rng_state()) == r.x
        got = g.spawn_diagnostics()
    finally:
        g.close()
    want = model.result()
    assert want["bins_single"].sum() > 0 and want["bins_double"].sum() > len(recs) // 2
    _same_diag(got, want)


# ------------------------------------------------------------------------------------------------ 3. bin edges with exact integers
@pytest.mark.parametrize("parent", ["neel", "three_hops"])
def test_hubbard_bins_are_exact_integers(request, parent):
    """Hubbard 4x4, t = 1, tau = 2^-6, one step from one determinant of weight 4096: every live ratio is nelec * ctr exactly (ctr = empty
    neighbours of the chosen electron), so the occupied bins are exactly {1 + nelec c}, plus bin 1 for electrons with no empty
    neighbour; the frequencies follow the electrons (each chosen with probability 1 / nelec).  From the Neel state every electron has
    four empty neighbours and all 4096 entries lie in one bin (no G-test with one cell: the count itself is asserted); a second parent
    with unequal ctr gives the G-test its cells."""
    import sqmc_amd
    sqmc_amd.set_device(0)
    hub, setup = request.getfixturevalue("hub44"), request.getfixturevalue("hub_setup")
    H = TU.hub_checker(hub)
    nelec = hub.nup + hub.ndn
    if parent == "neel":
        par = (sum(1 << (4 * y + x) for y in range(4) for x in range(4) if (x + y) % 2 == 0), sum(1 << (4 * y + x) for y in range(4) for x in range(4) if (x + y) % 2 == 1))
    else:
        par = dict(PC.parents_hubbard(H, (hub.hf_up, hub.hf_dn)))["three_hops"]
    kids = PC.excitations_hubbard(H, *par)
    ctr = []                                   # empty neighbours per electron, from the checker's own children
    for spin in (0, 1):
        for s in range(H.norb):
            if par[spin] >> s & 1:
                ctr.append(sum(1 for c in kids if c[1 - spin] == par[1 - spin] and c[spin] != par[spin] and not c[spin] >> s & 1))
    assert len(ctr) == nelec and sum(ctr) == len(kids)
    expv = np.zeros(SH.NBINS)
    for c in ctr:
        expv[nelec * c] += 4096.0 / nelec          # bin 1 + nelec c at index nelec c; c = 0: bin 1
    tau = 2.0 ** -6
    g = gpu_ctx_hub(hub, rng_mode=sqmc_amd.RNG_COUNTER, seed=SEED, mwalk=200000)
    try:
        g.set_ct_table(setup.ct_up, setup.ct_dn, setup.ct_num, setup.ct_den)
        g.upload_walkers(_walkers([par[0]], [par[1]], [4096.0]))
        g.set_spawn_diagnostics(True)
        out = g.step(_plain_params(tau, 0.0))
        d = g.spawn_diagnostics()
    finally:
        g.close()
    assert int(out[15]) == 4096 and int(d["bins"].sum()) == 4096
    assert np.array_equal(d["bins"], d["bins_hf"]) and d["bins_single"].sum() == 0 and d["bins_double"].sum() == 0
    occupied = set(np.nonzero(d["bins"])[0].tolist())
    print("%s: ctr per electron %s, occupied bins %s" % (parent, ctr, sorted(b + 1 for b in occupied)))
    assert occupied == set(np.nonzero(expv)[0].tolist())
    assert d["max_ratio"] == float(nelec * max(ctr)) and d["min_ratio"] == float(nelec * min(c for c in ctr if c > 0))
    if len(occupied) == 1:
        assert parent == "neel" and occupied == {nelec * 4}
    else:
        G, dof, pval, pooled = PC.g_test(d["bins"], expv)
        print("G = %.3f, dof = %d, p = %.3g" % (G, dof, pval))
        assert dof >= 1 and pval > PC.P_MIN


# ------------------------------------------------------------------------------------------------ 4. first moment
STEP_W = 262144.25          # 2^18 proposals
MOMENT_CASES = {"c2_walk": "open_double", "c2_hci": "open_single", "heg14": "off_fermi_sphere", "hub44": "three_hops", "hubbardk": None}


@pytest.mark.parametrize("case", sorted(MOMENT_CASES))
def test_first_moment_is_the_row_sum_of_abs_h(request, case):
    """One RNG_COUNTER step from one determinant of weight 262144.25 (2^18 proposals).  E[x] = sum_j p_j |H_ij| / p_j = sum_j |H_ij| over
    the live elements of the checker's row.  A unit-wide bin b holds lower bound b - 1, so with m_lo = sum n_b (b-1) / N,
    m_hi = sum n_b b / N and se = sqrt((sum n_b b^2 / N - m_lo^2) / N): m_lo - 5 se <= sum_j |H_ij| <= m_hi + 5 se.  The last (open) bin
    must be empty -- the parents are ones whose ratios stay far below 10000 --, sum bins = 2^18, and the highest occupied bin is the
    bin of the reported max ratio."""
    import sqmc_amd
    sqmc_amd.set_device(0)
    if case == "hubbardk":
        from sqmc_amd.host import HubbardKHost
        hst = HubbardKHost(4, 4, 5, 5, 1.0, 4.0)
        H = HK.HubbardKH(4, 4, 1.0, 4.0)
        par, ts, tau = (hst.hf_up, hst.hf_dn), False, 0.01
        rowd = PC.row(H, par, HK.excitations_hubbardk(H, *par))
        g = hst.gpu(rng_mode=sqmc_amd.RNG_COUNTER, mwalk=1 << 20)
        setup = hst.setup_walk(g, 20, 30, 0.5)
    else:
        setup_name = {"c2_walk": "c2_setup", "c2_hci": "c2_setup_ts", "heg14": "heg_setup", "hub44": "hub_setup"}[case]
        sysm, setup = request.getfixturevalue(case), request.getfixturevalue(setup_name)
        H, parents, children, ts = TU.uniform_case(sysm, case)
        par = dict(parents)[MOMENT_CASES[case]]
        tau = TAU[TU.UNIFORM[case][0]]
        rowd = PC.row(H, par, children(par), ts)
        mk = gpu_ctx_heg if case.startswith("heg") else gpu_ctx_hub if case.startswith("hub") else gpu_ctx_from_oracle
        g = mk(sysm, rng_mode=sqmc_amd.RNG_COUNTER, mwalk=1 << 20)
    try:
        g.set_ct_table(setup.ct_up, setup.ct_dn, setup.ct_num, setup.ct_den)
        g.upload_walkers(_walkers([par[0]], [par[1]], [STEP_W]))
        g.set_spawn_diagnostics(True)
        h_ii = (H.element_ts(*par, *par) if ts else H.element(*par, *par))[0]
        out = g.step(_plain_params(tau, h_ii + 2.0))
        d = g.spawn_diagnostics()
    finally:
        g.close()
    N = 1 << 18
    n = d["bins"].astype(np.float64)
    b = np.arange(1, SH.NBINS + 1, dtype=np.float64)
    want = float(sum(abs(v[0]) for v in rowd.values() if PC.is_live(v)))
    m_lo, m_hi = float((n * (b - 1)).sum() / N), float((n * b).sum() / N)
    se = math.sqrt((float((n * b * b).sum()) / N - m_lo * m_lo) / N)
    top = int(np.nonzero(d["bins"])[0].max()) + 1
    print("%s: sum|H_ij| = %.6f, m_lo = %.6f, m_hi = %.6f, se = %.6f, top bin %d, max ratio %.6f (level %d), min ratio %.6g, share in bin 1 %.4f"
          % (case, want, m_lo, m_hi, se, top, d["max_ratio"], d["max_ratio_level"], d["min_ratio"], n[0] / N))
    assert int(out[15]) == N and int(d["bins"].sum()) == N and np.array_equal(d["bins"], d["bins_hf"])
    assert d["bins"][SH.NBINS - 1] == 0
    assert top == int(SH.bin_index(d["max_ratio"])[0][0])
    assert m_lo - 5 * se <= want <= m_hi + 5 * se
    if case == "c2_walk":          # every weighted move is a single or a double; the weightless ones sit in bin 1, unclassified
        assert int((d["bins_single"] + d["bins_double"]).sum()) == int(N - d["bins"][0] + (d["bins_single"][0] + d["bins_double"][0]))
    elif not case.startswith("c2"):
        assert d["bins_single"].sum() == 0 and d["bins_double"].sum() == 0


# ------------------------------------------------------------------------------------------------ 5. counting
def _plain_c2_ctx():
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    h = _host("c2")
    g = h.gpu(rng_mode=sqmc_amd.RNG_COUNTER, seed=SEED, mwalk=200000)
    s = h.setup_walk(g, 100, 1000, 0.1)
    g.set_ct_table(s.ct_up, s.ct_dn, s.ct_num, s.ct_den)
    wk = H.initial_walkers(s, 300)
    keep = np.abs(wk["wt"]) >= 0.5
    return g, s, _walkers(wk["up"][keep], wk["dn"][keep], wk["wt"][keep])


def test_counts_are_the_proposals_of_the_returned_steps():
    """A plain walk with always_spawn_cutoff_wt = 0 has no gated walker (no draw decides whether a walker spawns): after k steps
    sum(bins) is the number of children of the lists downloaded before each step.  reset zeroes everything; off then on keeps the
    counts."""
    g, s, wk = _plain_c2_ctx()
    try:
        g.upload_walkers(wk)
        g.set_spawn_diagnostics(True)
        prm = _plain_params(s.tau, s.e_trial0, cutoff=0.0)
        want = 0
        for k in range(8):
            here = _n_proposals(g.download_walkers()["wt"])
            want += here
            out = g.step(prm)
            d = g.spawn_diagnostics()
            assert int(out[15]) == here and int(d["bins"].sum()) == want, (k, int(d["bins"].sum()), want, out[15], here)
        assert int((d["bins_single"] + d["bins_double"]).sum()) <= want and d["max_ratio"] > d["min_ratio"] > 1e-9
        g.set_spawn_diagnostics(False)
        g.step(prm)                                   # not counted
        held = g.spawn_diagnostics()
        _same_diag(held, d)
        g.set_spawn_diagnostics(True)
        _same_diag(g.spawn_diagnostics(), d)          # off then on keeps the counts
        more = _n_proposals(g.download_walkers()["wt"])
        g.step(prm)
        assert int(g.spawn_diagnostics()["bins"].sum()) == want + more
        g.reset_spawn_diagnostics()
        z = g.spawn_diagnostics()
        assert all(int(z[k].sum()) == 0 for k in HISTS) and z["n_nan"] == 0
        assert z["max_ratio"] == -1e99 and z["max_ratio_level"] == -1 and z["min_ratio"] == 1e99 and np.all(z["max_ratio_by_level"] == -1e99)
    finally:
        g.close()


def test_counts_under_chained_runs_and_a_pending_head():
    """sqmc_gpu_run with chained runs: one entry per child of every returned step (out[15]), also when the diagnostics are switched
    on while the head of the next step is already enqueued in the other form"""
    w = _walk("c2_uniform", False, w_target=2500.0, w_begin=3000.0)
    try:
        w.g.set_chained_runs(True)
        w.run(25)
        assert w.pc.reached == 2                      # the last step enqueued a head
        w.g.set_spawn_diagnostics(True)
        st = np.concatenate([w.run(n)[0] for n in (7, 1, 12)])
        d = w.spawn_diagnostics()
        assert int(d["bins"].sum()) == int(st[:, 15].sum())
        w.g.set_spawn_diagnostics(False)
        w.run(5)
        assert int(w.spawn_diagnostics()["bins"].sum()) == int(st[:, 15].sum())
    finally:
        w.close()


def _retry_job():
    """every third bucket step redoes its tail (SQMC_BUCKET_FORCE_RETRY, read once per process): no proposal is counted twice"""
    w = _walk("c2_uniform", True, w_target=2500.0, w_begin=3000.0)
    try:
        w.g.set_chained_runs(True)
        st = np.concatenate([w.run(n)[0] for n in (30, 10)])
        d = w.spawn_diagnostics()
        retries = w.g.tail_stats()[1]
        print("retries %d, entries %d, children %d" % (retries, int(d["bins"].sum()), int(st[:, 15].sum())))
        assert retries >= 3               # the rollback really ran
        assert int(d["bins"].sum()) == int(st[:, 15].sum())
    finally:
        w.close()


def test_counts_when_a_bucket_tail_gives_up():
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "retry-job"], capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env=dict(os.environ, SQMC_BUCKET_FORCE_RETRY="3", SQMC_BUCKET_HOLDOFF="0"))
    assert r.returncode == 0 and "retries" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ------------------------------------------------------------------------------------------------ 6. sharded
def _shard_worker(rank, world, port, outdir, semi, nsteps):
    import torch                                   # noqa: F401  before the HIP library
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    hst = H.ChemHost(FCIDUMP, 8, 4, "d2h")
    w = H.ShardedWalk(hst, 4000, rank, world, w_begin=2000, seed=SEED, mwalk=400000, semistochastic=semi, spawn_diagnostics=True)
    if not semi:                                   # always_spawn_cutoff_wt = 0: no gated walker, the children follow from the list
        params = w.pc.params
        w.pc.params = lambda **kw: params(cutoff=0.0, **kw)
    counted = 0
    for _ in range(nsteps):
        if not semi:
            counted += _n_proposals(w.g.download_walkers()["wt"])
        w.step()
    local, glob = w.g.spawn_diagnostics(), w.spawn_diagnostics()
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), counted=counted, **{"local_" + k: local[k] for k in HISTS},
             **{k: np.asarray(v) for k, v in glob.items()})
    w.close()
    dist.barrier()
    dist.destroy_process_group()


def _single_worker(outdir, nsteps):
    os.environ["SQMC_BUCKET"] = "0"                # the radix tail, the one the sharded step runs
    sys.path.insert(0, ROOT)
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    w = H.GpuWalk(H.ChemHost(FCIDUMP, 8, 4, "d2h"), 4000, w_begin=2000, seed=SEED, mwalk=400000, spawn_diagnostics=True)
    for _ in range(nsteps):
        w.step()
    d = w.spawn_diagnostics()
    np.savez(os.path.join(outdir, "single.npz"), **{k: np.asarray(v) for k, v in d.items()})
    w.close()


def _spawn_all(targets):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    ps = [ctx.Process(target=t, args=a) for t, a in targets]
    for p in ps: p.start()
    for p in ps: p.join(600)
    assert all(p.exitcode == 0 for p in ps), [p.exitcode for p in ps]


def test_sharded_two_ranks_sum_their_histograms(tmp_path):
    """Two ranks of a plain walk (always_spawn_cutoff_wt = 0: no gated walker) over gloo: every rank's local sum(bins) is the children of the lists it held, the
    all-reduced histogram is the sum of both, the ratios are the max / min over the ranks, and both ranks hold the same result"""
    _spawn_all([(_shard_worker, (r, 2, 29631, str(tmp_path), False, 12)) for r in range(2)])
    res = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(2)]
    for r in res:
        assert int(r["local_bins"].sum()) == int(r["counted"]) > 0
    for k in HISTS:
        assert np.array_equal(res[0][k], res[0]["local_" + k] + res[1]["local_" + k]), k
        assert np.array_equal(res[0][k], res[1][k])
    assert int(res[0]["bins"].sum()) == int(res[0]["counted"]) + int(res[1]["counted"])
    for k in ("max_ratio", "min_ratio", "max_ratio_level", "max_ratio_by_level"):
        assert np.array_equal(res[0][k], res[1][k])
    assert float(res[0]["max_ratio"]) == float(res[0]["max_ratio_by_level"].max()) > float(res[0]["min_ratio"]) > 0


def test_one_rank_sharded_histograms_equal_single_gpu(tmp_path, monkeypatch):
    """one rank: the sharded step walks the single-GPU trajectory (radix tail on both sides), so the histograms agree bit for bit"""
    monkeypatch.setenv("SQMC_SHARD_BUCKET", "0")
    _spawn_all([(_shard_worker, (0, 1, 29633, str(tmp_path), True, 25))])
    _spawn_all([(_single_worker, (str(tmp_path), 25))])
    a, b = np.load(os.path.join(str(tmp_path), "rank0.npz")), np.load(os.path.join(str(tmp_path), "single.npz"))
    for k in HISTS + ("max_ratio_by_level", "max_ratio", "max_ratio_level", "min_ratio", "n_nan"):
        assert np.array_equal(a[k], b[k]), k
    assert int(a["bins"].sum()) > 25 * 1000


def _inlib_diag_worker(rank, world, port, outdir, fake, diag, semi, nsteps, env):
    """one rank of a walk whose exchanges the library issues itself (attach_rccl: sqmc_gpu_shard_step, then chained sqmc_gpu_shard_run
    calls past the target population, where the walk without diagnostics pipelines its steps)"""
    os.environ.update(env or {})
    import torch                                   # noqa: F401  before the HIP library
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    if fake:
        os.environ["SQMC_RCCL_LIB"] = fake         # before the library binds its communication entry points
    dist.init_process_group("gloo", rank=rank, world_size=world)     # carries the unique id and the diagnostics' all-reduce
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    hst = H.ChemHost(FCIDUMP, 8, 4, "d2h")
    w = H.ShardedWalk(hst, 2500, rank, world, w_begin=3000, seed=SEED, mwalk=400000, semistochastic=semi, spawn_diagnostics=diag)
    w.attach_rccl()
    w.g.set_chained_runs(True)
    outs = [w.step().copy() for _ in range(nsteps[0])]               # sqmc_gpu_shard_step
    outs = np.concatenate([np.array(outs)] + [w.run(n)[0] for n in nsteps[1:]])      # sqmc_gpu_shard_run
    w.g.set_chained_runs(False)
    wk = w.g.download_walkers()
    extra = {}
    if diag:
        local, glob = w.g.spawn_diagnostics(), w.spawn_diagnostics()
        extra = dict({"local_" + k: local[k] for k in HISTS}, **{k: np.asarray(v) for k, v in glob.items()})
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), outs=outs, reached=np.array([w.pc.reached]), tail=np.array(w.g.tail_stats()),
             up=wk["up"], dn=wk["dn"], wt=wk["wt"], imp_distance=wk["imp_distance"], initiator=wk["initiator"], **extra)
    w.close()
    dist.barrier()
    dist.destroy_process_group()


def _inlib_runs(tmp_path, world, fake, port, semi, nsteps, env=None):
    """the walk with the diagnostics on and off, one after the other; per run the ranks' files"""
    runs = []
    for k, diag in enumerate((True, False)):
        out = os.path.join(str(tmp_path), "diag%d" % k); os.makedirs(out)
        _spawn_all([(_inlib_diag_worker, (r, world, port + k, out, fake, diag, semi, nsteps, env)) for r in range(world)])
        runs.append([np.load(os.path.join(out, "rank%d.npz" % r)) for r in range(world)])
    return runs


INLIB_STEPS = (12, 20, 1, 9)


@pytest.mark.parametrize("force_retry", [False, True])
def test_in_library_two_ranks_count_once_per_step(tmp_path, force_retry):
    """Two ranks over the transport double of the sharded tests (tests/fake_rccl through SQMC_RCCL_LIB and attach_rccl): the library's
    own sqmc_gpu_shard_step, then chained sqmc_gpu_shard_run calls past the target population -- where the walk without diagnostics
    enqueues every step's head (and the next step's deterministic weights) ahead and the walk with them does not.  The sums of every
    step and the final lists are bit-identical on and off on both ranks; every rank's sum(bins) is the sum of its own out[15] (the
    local child count of every returned step) and the all-reduced histogram the sum over the ranks.  force_retry: rank 1's bucket tail
    gives up on every third bucket step and the step is re-run (a second all-reduce of the sums on both ranks): nothing is counted
    twice."""
    from tests.test_gpu_sharded import _fake_rccl_lib
    env = {"SQMC_BUCKET_FORCE_RETRY": "3", "SQMC_BUCKET_FORCE_RETRY_RANK": "1", "SQMC_BUCKET_HOLDOFF": "0"} if force_retry else None
    on, off = _inlib_runs(tmp_path, 2, _fake_rccl_lib(), 29671 + 4 * int(force_retry), True, INLIB_STEPS, env)
    assert all(int(r["reached"][0]) == 2 for r in on + off)          # the run() calls of the walk without diagnostics were pipelined
    for a, b in zip(on, off):
        assert a["outs"].shape == (sum(INLIB_STEPS), 16) and np.array_equal(a["outs"], b["outs"])
        for key in ("up", "dn", "wt", "imp_distance", "initiator"):
            assert np.array_equal(a[key], b[key]), key
        assert np.array_equal(a["tail"], b["tail"])
    assert np.array_equal(on[0]["outs"][:, :7], on[1]["outs"][:, :7])
    if force_retry:
        print("retries per rank: %s" % [int(r["tail"][1]) for r in on])
        assert int(on[1]["tail"][1]) >= 3 and int(on[0]["tail"][1]) == 0          # the re-run really ran, on rank 1 alone
    children = [int(r["outs"][:, 15].sum()) for r in on]
    for r, n in zip(on, children):
        assert int(r["local_bins"].sum()) == n > 0
    for k in HISTS:
        assert np.array_equal(on[0][k], on[0]["local_" + k] + on[1]["local_" + k]), k
        assert np.array_equal(on[0][k], on[1][k])
    assert int(on[0]["bins"].sum()) == sum(children)
    for k in ("max_ratio", "min_ratio", "max_ratio_level", "max_ratio_by_level", "n_nan"):
        assert np.array_equal(on[0][k], on[1][k])
    assert int(on[0]["n_nan"]) == 0 and float(on[0]["max_ratio"]) == float(on[0]["max_ratio_by_level"].max()) > float(on[0]["min_ratio"]) > 0


def _single_run_worker(outdir, nsteps):
    os.environ["SQMC_BUCKET"] = "0"                # the radix tail, the one the sharded step is made to run
    sys.path.insert(0, ROOT)
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    w = H.GpuWalk(H.ChemHost(FCIDUMP, 8, 4, "d2h"), 2500, w_begin=3000, seed=SEED, mwalk=400000, spawn_diagnostics=True)
    w.g.set_chained_runs(True)
    outs = [w.step().copy() for _ in range(nsteps[0])]
    outs = np.concatenate([np.array(outs)] + [w.run(n)[0] for n in nsteps[1:]])
    d = w.spawn_diagnostics()
    np.savez(os.path.join(outdir, "single.npz"), outs=outs, **{k: np.asarray(v) for k, v in d.items()})
    w.close()


def test_in_library_one_rank_equals_single_gpu(tmp_path, monkeypatch):
    """One rank through the library's own sharded step and run (real RCCL, as test_in_library_rccl_exchange_single_rank runs it; radix
    tail on both sides) with the diagnostics on: the single-GPU walk's histograms, ratios and child counts bit for bit"""
    monkeypatch.setenv("SQMC_SHARD_BUCKET", "0")
    _spawn_all([(_inlib_diag_worker, (0, 1, 29681, str(tmp_path), None, True, True, INLIB_STEPS, None)), (_single_run_worker, (str(tmp_path), INLIB_STEPS))])
    a, b = np.load(os.path.join(str(tmp_path), "rank0.npz")), np.load(os.path.join(str(tmp_path), "single.npz"))
    assert int(a["reached"][0]) == 2
    assert np.array_equal(a["outs"][:, 15], b["outs"][:, 15])
    for k in HISTS + ("max_ratio_by_level", "max_ratio", "max_ratio_level", "min_ratio", "n_nan"):
        assert np.array_equal(a[k], b[k]), k
    assert int(a["bins"].sum()) == int(a["outs"][:, 15].sum()) > sum(INLIB_STEPS) * 1000


# ------------------------------------------------------------------------------------------------ 7. deck
def test_deck_prints_both_tables_and_changes_nothing_else():
    """--spawn-histograms on the C2 walk smoke deck: both tables behind the `Energy=` line, their totals those of
    spawn_diagnostics(); without the flag the deck prints what it prints with it minus the tables (the walk is the same walk)"""
    from sqmc_amd.walk_run import parse_walk_deck, run_walk
    deck = parse_walk_deck(open(os.path.join(ROOT, "tests", "golden", "C2_r1.24253_i_walk")).read())
    on, off = io.StringIO(), io.StringIO()
    r_on = run_walk(deck, FCIDUMP, out=on, spawn_histograms=True)
    r_off = run_walk(deck, FCIDUMP, out=off)
    assert "spawn_diagnostics" not in r_off
    lines_on, lines_off = on.getvalue().split("\n"), off.getvalue().split("\n")
    assert not any("Histogram" in l or l.startswith("Max Ratio") for l in lines_off)
    k = next(i for i, l in enumerate(lines_on) if l.startswith("Energy="))
    n_tab = 2 * SH.NBINS + 6
    timing = lambda l: l.startswith("sqmc_amd: set-up")          # wall-clock figures
    rest = lines_on[:k + 1] + lines_on[k + 1 + n_tab:]
    assert [l for l in rest if not timing(l)] == [l for l in lines_off if not timing(l)]
    d = r_on["spawn_diagnostics"]
    tab = lines_on[k + 1:k + 1 + n_tab]
    assert deck["ipr"] == 0 and not any(l.startswith("Max Ratio") for l in lines_on)          # the ratio line belongs to ipr >= 1
    assert "\n".join(tab) + "\n" == SH.expected_text(d)
    assert tab[0] == " Histogram of abs weight multipliers spawned by HF:" and tab[SH.NBINS + 3] == " Histogram of abs weight multipliers spawned by any states:"
    assert tab[SH.NBINS + 2] == " Total=%21d" % int(d["bins_hf"].sum())
    tot = [l for l in tab if l.startswith("Total=")][0]
    assert [int(v) for v in tot[6:].split()] == [int(d[k].sum()) for k in ("bins_single", "bins_double", "bins")]
    assert int(d["bins"].sum()) > 100 * r_on["n_blocks_total"] * 1000 and d["n_nan"] == 0


if __name__ == "__main__" and sys.argv[1:] == ["retry-job"]:
    _retry_job()
