"""proposal_method CauchySchwarz on the GPU: the test door bit for bit against the checker (tests/cauchy_checker.py),
the sampled distribution against the checker's exact enumerator, the two tails and the chained run on CS walks,
and a CauchySchwarz walk deck end to end."""
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
from tests import cauchy_checker as CC          # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
FCIDUMP = os.path.join(GOLD, "C2_r1.24253_FCIDUMP")
SYSTEMS = {"c2_8e": (8, 4, 0), "c2_10e": (10, 5, 0), "c2_8e_core1": (8, 4, 1)}
TAU = 0.005314


def _host(name):
    from sqmc_amd import host as H
    nelec, nup, nc = SYSTEMS[name]
    return H.ChemHost(FCIDUMP, nelec, nup, "d2h", n_core_orb=nc)


def _mix48(k):
    v = (k * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & ((1 << 64) - 1)
    v ^= v >> 30; v = (v * 0xBF58476D1CE4E5B9) & ((1 << 64) - 1)
    v ^= v >> 27; v = (v * 0x94D049BB133111EB) & ((1 << 64) - 1)
    v ^= v >> 31
    return v & CC.MASK48


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_door_matches_checker_bit_for_bit(name):
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    h = _host(name)
    cs = CC.from_host(h)
    g = h.gpu(proposal="cauchyschwarz", rng_mode=sqmc_amd.RNG_REPLAY, mwalk=0)
    try:
        cu, cd = h.connected_all(h.hf_up, h.hf_dn)
        rng = np.random.default_rng(11)
        pick = rng.choice(len(cu), size=199, replace=False)
        parents = [(h.hf_up, h.hf_dn)] + [(int(cu[k]), int(cd[k])) for k in pick]
        n = 10000
        states = [_mix48(k) for k in range(n)]
        # states whose k-th draw is the largest, (2^48 - 1) / 2^48 (the LCG's modular inverse, k = 1..5): every search's last candidate
        # is still found (on C2 no search falls through, tests/test_cauchy_schwarz.py)
        inv = pow(CC.LCG_MULT, -1, 1 << 48)
        x = CC.MASK48
        for k in range(5):
            x = (x * inv) & CC.MASK48
            states[k] = x
        pu = np.array([parents[k % len(parents)][0] for k in range(n)], np.uint64)
        pd = np.array([parents[k % len(parents)][1] for k in range(n)], np.uint64)
        seeds = np.array([CC.state_limbs(s) for s in states], np.int32)
        ju, jd, wj, sa = g.propose_cauchy_schwarz_batch(TAU, pu, pd, seeds)
        exp = []
        for k in range(n):
            r = CC.Rannyu(states[k])
            lev, a, b, p = cs.move(int(pu[k]), int(pd[k]), r)
            exp.append((lev, a, b, p, r.x))
        lev = np.array([e[0] for e in exp])
        assert np.array_equal(ju, np.array([e[1] for e in exp], np.uint64))
        assert np.array_equal(jd, np.array([e[2] for e in exp], np.uint64))
        assert np.array_equal(sa, np.array([CC.state_limbs(e[4]) for e in exp], np.int32))
        mv = np.nonzero(lev > 0)[0]
        hij = g.hamiltonian_chem_batch(pu[mv], pd[mv], ju[mv], jd[mv])
        want = np.zeros(n)
        want[mv] = [-TAU * float(hv) / exp[k][3] for hv, k in zip(hij, mv)]
        assert np.array_equal(wj, want)
        assert np.all(wj[lev == 0] == 0.0)
        assert (lev == 1).sum() > 0 and (lev == 2).sum() > n // 2
    finally:
        g.close()


@pytest.mark.gpu
def test_sampled_distribution_matches_enumerator():
    """2^22 proposals from one open-shell parent, one hashed seed each, against the enumerator's exact masses: G-test at a fixed seed"""
    from scipy.stats import chi2
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    h = _host("c2_8e")
    cs = CC.from_host(h)
    cu, cd = h.connected_all(h.hf_up, h.hf_dn)
    par = next((int(u), int(d)) for u, d in zip(cu, cd) if int(u) != int(d) and int(u) != h.hf_up and int(d) != h.hf_dn)
    paths, null, reported = cs.enumerate(*par)
    mass = {}
    for p in paths:
        mass[p[5]] = mass.get(p[5], 0.0) + p[6]
    g = h.gpu(proposal="cauchyschwarz", rng_mode=sqmc_amd.RNG_REPLAY, mwalk=0)
    try:
        n = 1 << 22
        st = (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)      # splitmix64 of the proposal index
        st ^= st >> np.uint64(30); st *= np.uint64(0xBF58476D1CE4E5B9)
        st ^= st >> np.uint64(27); st *= np.uint64(0x94D049BB133111EB); st ^= st >> np.uint64(31)
        st &= np.uint64(CC.MASK48)
        seeds = np.stack([(st >> np.uint64(36)) & np.uint64(4095), (st >> np.uint64(24)) & np.uint64(4095),
                          (st >> np.uint64(12)) & np.uint64(4095), st & np.uint64(4095)], axis=1).astype(np.int32)
        ju, jd, wj, _ = g.propose_cauchy_schwarz_batch(TAU, np.full(n, par[0], np.uint64), np.full(n, par[1], np.uint64), seeds)
    finally:
        g.close()
    moved = (ju != np.uint64(par[0])) | (jd != np.uint64(par[1]))      # a move with a zero matrix element has weight 0 but lands on its det_j
    keys = sorted(mass)
    index = {k: i for i, k in enumerate(keys)}
    obs = np.zeros(len(keys) + 1)
    pairs = np.stack([ju[moved], jd[moved]], axis=1)
    uniq, cnt = np.unique(pairs, axis=0, return_counts=True)
    for (a, b), c in zip(uniq, cnt):
        obs[index[(int(a), int(b))]] += c           # a KeyError here is a determinant the enumerator cannot reach
    obs[-1] = n - moved.sum()
    expv = np.array([mass[k] for k in keys] + [null]) * n
    small = expv < 5
    o = np.append(obs[~small], obs[small].sum()); e = np.append(expv[~small], expv[small].sum())
    keep = e > 0
    o, e = o[keep], e[keep]
    G = 2.0 * np.sum(np.where(o > 0, o * np.log(np.where(o > 0, o, 1) / e), 0.0))
    p = chi2.sf(G, len(o) - 1)
    worst = np.argsort(-np.abs(obs - expv) / np.sqrt(np.maximum(expv, 1.0)))[:5]
    assert p > 1e-6, (G, len(o), p, [(int(k), obs[k], expv[k]) for k in worst], int(obs[-1]), expv[-1])


WORKER_STEPS = 50


def _walk_worker(out, mode):
    """a CS walk under COUNTER: `step` -- WORKER_STEPS steps one by one; `run` -- one chained sqmc_gpu_run"""
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    h = H.ChemHost(FCIDUMP, 8, 4, "d2h")
    w = H.GpuWalk(h, 2000, w_begin=100, seed=(1346, 5634, 6635, 4361), rng_mode=H.RNG_COUNTER, proposal="cauchyschwarz")
    outs = []
    if mode == "step":
        for _ in range(WORKER_STEPS):
            outs.append(np.array(w.step()))
    else:
        stats, _ = w.run(WORKER_STEPS)
        outs = list(np.asarray(stats).reshape(WORKER_STEPS, -1))
    wk = w.g.download_walkers()
    np.savez(out, up=wk["up"], dn=wk["dn"], wt=wk["wt"], initiator=wk["initiator"], outs=np.array(outs), tail=np.array(w.g.tail_stats()))
    w.close()


def _spawn(tmp_path, tag, mode, env_extra):
    out = str(tmp_path / (tag + ".npz"))
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "worker", out, mode], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return np.load(out)


@pytest.mark.gpu
def test_tails_and_chained_run_agree(tmp_path):
    bucket = _spawn(tmp_path, "bucket", "step", {})
    radix = _spawn(tmp_path, "radix", "step", {"SQMC_BUCKET": "0"})
    chained = _spawn(tmp_path, "run", "run", {})
    assert bucket["tail"][0] > WORKER_STEPS // 2 and radix["tail"][0] == 0
    # the two tails hold the same determinants; their sums come out of different reduction trees (as for uniform2): weights to rounding
    assert np.array_equal(bucket["up"], radix["up"]) and np.array_equal(bucket["dn"], radix["dn"])
    assert np.array_equal(bucket["initiator"], radix["initiator"])
    assert np.allclose(bucket["wt"], radix["wt"], rtol=1e-11, atol=0)
    assert np.allclose(bucket["outs"][:, :16], radix["outs"][:, :16], rtol=1e-11, atol=1e-11)
    # sqmc_gpu_run and step-by-step: the same walk
    for k in ("up", "dn", "wt", "initiator"):
        assert np.array_equal(chained[k], bucket[k]), k


@pytest.mark.gpu
def test_replay_walk_steps_are_deterministic():
    """two identical REPLAY walks with the CS proposal (the prepass lane runs every proposal) leave the same walkers and RNG state"""
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    h = H.ChemHost(FCIDUMP, 8, 4, "d2h")
    res = []
    for _ in range(2):
        w = H.GpuWalk(h, 1000, w_begin=100, rng_mode=sqmc_amd.RNG_REPLAY, proposal="cauchyschwarz")
        for _ in range(10):
            out = w.step()
        wk = w.g.download_walkers()
        res.append((wk, w.g.rng_state(), np.array(out)))
        w.close()
    (a, ra, oa), (b, rb, ob) = res
    assert ra == rb and np.array_equal(oa, ob)
    for k in ("up", "dn", "wt"):
        assert np.array_equal(a[k], b[k])
    assert len(a["up"]) > 100


def _replay_step(cs, wk, prm, state, hij_of, hii_of):
    """one REPLAY step of a plain walk restated: the gate and the CS proposals from the single rannyu stream (k_replay_prepass's
    order: walkers in list order, the gate draw, then the children's proposals), death/clone 1 + tau (E_T - H_ii), every child an
    initiator child, min_wt = 0 (no rounding draws).  Returns the merged walkers {(up, dn): (weight, scale)}, the child count and the
    RNG state after."""
    r = CC.Rannyu(state)
    tau, cut = prm["tau"], prm["always_spawn_cutoff_wt"]
    kids = []
    nch = 0
    for u, d, w in zip(wk["up"].tolist(), wk["dn"].tolist(), wk["wt"].tolist()):
        if abs(w) < cut:
            if not r.draw() < abs(w / cut):
                continue
            nc, wc = 1, math.copysign(cut, w)
        else:
            nc = max(int(math.floor(abs(w) + 0.5)), 1)
            wc = w / nc
        for _ in range(nc):
            nch += 1
            lev, ju, jd, p = cs.move(u, d, r)
            if lev > 0:
                kids.append((u, d, ju, jd, wc, p))
    hij = hij_of([k[0] for k in kids], [k[1] for k in kids], [k[2] for k in kids], [k[3] for k in kids]) if kids else []
    hii = hii_of(wk["up"], wk["dn"])
    out = {}
    for u, d, w, e in zip(wk["up"].tolist(), wk["dn"].tolist(), wk["wt"].tolist(), hii.tolist()):
        v = w * (1.0 + tau * (prm["e_trial"] - e))
        out[(u, d)] = [v, abs(v)]
    for (u, d, ju, jd, wc, p), h in zip(kids, hij.tolist() if len(kids) else []):
        wj = wc * (-tau * h / p)
        if wj == 0.0:
            continue
        a = out.setdefault((ju, jd), [0.0, 0.0])
        a[0] += wj; a[1] += abs(wj)
    return out, nch, r.x


@pytest.mark.gpu
def test_replay_step_matches_checker():
    """A plain REPLAY walk with the CS proposal, one step at a time against the restatement: the gate and every proposal replayed
    by the checker from the same rannyu stream (so k_replay_prepass's draw counting and child_state offsets are checked), death /
    clone and the merge in numpy.  Walkers within 1e-12, out[15] (the child count) exact, the RNG state after the step equal; five
    chained steps, each re-seeded from the GPU's list."""
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    h = H.ChemHost(FCIDUMP, 8, 4, "d2h")
    cs = CC.from_host(h)
    g = h.gpu(proposal="cauchyschwarz", rng_mode=sqmc_amd.RNG_REPLAY, seed=(1346, 5634, 6635, 4361), mwalk=200000)
    try:
        s = h.setup_walk(g, 100, 1000, 0.1)
        g.set_ct_table(s.ct_up, s.ct_dn, s.ct_num, s.ct_den)
        wk = H.initial_walkers(s, 100)
        keep = wk["wt"] != 0
        wk = {k: v[keep] for k, v in wk.items()}
        prm = dict(tau=s.tau, e_trial=s.e_trial0, reweight_factor_inv=1.0, r_initiator=1.0, min_wt=0.0, always_spawn_cutoff_wt=0.5,
                   initiator_power=0, initiator_min_distance=0, c_t_initiator=0, semistochastic=0, reached_w_abs_gen=0)
        hij_of = lambda a, b, c, d: g.hamiltonian_chem_batch(np.array(a, np.uint64), np.array(b, np.uint64), np.array(c, np.uint64), np.array(d, np.uint64))
        hii_of = lambda u, d: g.hamiltonian_chem_batch(u, d, u, d)
        n_gate = n_multi = 0
        for step in range(5):
            n = len(wk["up"])
            wk = dict(up=wk["up"], dn=wk["dn"], wt=wk["wt"], imp_distance=np.ones(n, np.int8), initiator=np.full(n, 2, np.int8),
                      perm_sign=np.zeros(n, np.int8), matrix_elements=np.full(n, 1e51), e_num=np.full(n, 1e51), e_den=np.full(n, 1e51))
            n_gate += int((np.abs(wk["wt"]) < 0.5).sum()); n_multi += int((np.abs(wk["wt"]) >= 1.5).sum())
            g.upload_walkers(wk)
            state = CC.limbs_state(g.rng_state())
            want, nch, state_after = _replay_step(cs, wk, prm, state, hij_of, hii_of)
            out = g.step(prm)
            got = g.download_walkers()
            assert int(out[15]) == nch, (step, out[15], nch)
            assert CC.limbs_state(g.rng_state()) == state_after, step
            gk = {(int(a), int(b)): float(w) for a, b, w in zip(got["up"], got["dn"], got["wt"]) if w != 0.0}
            wk_ = {k: v for k, v in want.items() if v[0] != 0.0}
            assert set(gk) == set(wk_), (step, len(gk), len(wk_))
            for k, (v, sc) in wk_.items():
                assert abs(gk[k] - v) <= 1e-12 * sc, (step, k, gk[k], v)
            wk = got
        assert n_gate > 0 and n_multi > 0           # both kinds of parent (one gated child; several children) were exercised
    finally:
        g.close()


@pytest.mark.gpu
def test_library_stop_and_clamp_on_the_device(tmp_path):
    """sqmc_gpu_setup_cauchy_schwarz itself, on integrals the host has not clamped: an exchange integral of -1e-5 stops it with
    "Negative integrals!"; one of -1e-8 is clamped to 0 on the device, and H computed there equals H from integrals clamped on the host"""
    import sqmc_amd
    from sqmc_amd import host as H
    from sqmc_amd._lib import GpuChem
    sqmc_amd.set_device(0)
    src = open(FCIDUMP).read().splitlines(True)
    k = next(k for k, l in enumerate(src) if len(l.split()) == 5 and l.split()[1] == l.split()[3] and l.split()[2] == l.split()[4]
             and l.split()[1] != l.split()[2] and int(l.split()[2]) > 0)
    t = src[k].split()

    def host_with(value):
        lines = list(src); lines[k] = " %.16e %s %s %s %s\n" % (value, t[1], t[2], t[3], t[4])
        p = tmp_path / ("FCIDUMP_%g" % value); p.write_text("".join(lines))
        return H.ChemHost(str(p), 8, 4, "d2h")

    def ctx(h, ints):          # what ChemHost.gpu builds, without its host-side clamp
        return GpuChem(h.norb, h.nup, h.ndn, h.orbsym, h.prod.reshape(-1), h.combine_2.reshape(-1), ints, n_group=h.n_group, n_core_orb=h.n_core_orb)

    h = host_with(-1e-5)
    g = ctx(h, h.integrals)
    try:
        with pytest.raises(sqmc_amd.SqmcGpuError, match="Negative integrals!"):
            g.setup_cauchy_schwarz()
        with pytest.raises(sqmc_amd.SqmcGpuError, match="not called"):
            g.propose_cauchy_schwarz_batch(TAU, [h.hf_up], [h.hf_dn], [[1, 2, 3, 5]])      # nothing was installed
    finally:
        g.close()
    h = host_with(-1e-8)
    raw = np.array(h.integrals, copy=True)
    g = ctx(h, raw)
    assert h.cauchy_schwarz_clamp() == 1
    g_host = ctx(h, h.integrals)           # integrals clamped on the host
    g_raw = ctx(h, raw)                    # not clamped at all
    try:
        assert g.setup_cauchy_schwarz() == 1
        cu, cd = h.connected_all(h.hf_up, h.hf_dn)
        iu, id_ = np.full(len(cu), h.hf_up, np.uint64), np.full(len(cu), h.hf_dn, np.uint64)
        for a, b, c, d in ((iu, id_, cu, cd), (cu, cd, cu, cd)):
            hd, hh, hr = (x.hamiltonian_chem_batch(a, b, c, d) for x in (g, g_host, g_raw))
            assert np.array_equal(hd, hh)
        assert not np.array_equal(g.hamiltonian_chem_batch(cu, cd, cu, cd), g_raw.hamiltonian_chem_batch(cu, cd, cu, cd))
    finally:
        g.close(); g_host.close(); g_raw.close()


@pytest.mark.gpu
def test_deck_with_a_clamped_integral_runs_and_reports_it(tmp_path):
    from sqmc_amd.walk_run import parse_walk_deck, run_walk
    src = open(FCIDUMP).read().splitlines(True)
    k = next(k for k, l in enumerate(src) if len(l.split()) == 5 and l.split()[1] == l.split()[3] and l.split()[2] == l.split()[4]
             and l.split()[1] != l.split()[2] and int(l.split()[2]) > 0)
    t = src[k].split()
    src[k] = " %.16e %s %s %s %s\n" % (-1e-8, t[1], t[2], t[3], t[4])
    fd = tmp_path / "FCIDUMP"; fd.write_text("".join(src))
    deck = parse_walk_deck(open(_cs_deck(tmp_path)).read())
    buf = io.StringIO()
    res = run_walk(deck, str(fd), out=buf)
    assert " CauchySchwarz: 1 exchange integrals" in buf.getvalue() and "Energy=" in buf.getvalue()
    assert np.isfinite(res["energy"]) and res["n_imp"] > 0     # (an exchange integral of ~0.3 Ha is gone: not C2's energy any more)


@pytest.mark.gpu
def test_setup_order_and_exclusions():
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    h = H.ChemHost(FCIDUMP, 8, 4, "d2h")
    g = h.gpu(rng_mode=H.RNG_COUNTER, mwalk=200000)
    try:
        assert g.setup_cauchy_schwarz() == 0
        with pytest.raises(sqmc_amd.SqmcGpuError):
            g.setup_efficient_heatbath()           # fast heat-bath and CS exclude each other; the context keeps CS
        s = h.setup_walk(g, 100, 1000, 0.1)
        g.set_projector(s.prj_counts, s.prj_indices, s.prj_values)
        with pytest.raises(sqmc_amd.SqmcGpuError, match="must come before"):
            g.setup_cauchy_schwarz()
    finally:
        g.close()
    with pytest.raises(ValueError, match="hf_to_psit"):
        H.GpuWalk(h, 1000, proposal="cauchyschwarz", hf_to_psit=True)


def _cs_deck(tmp_path):
    txt = open(os.path.join(GOLD, "C2_r1.24253_i_walk")).read()
    lines = txt.splitlines(True)
    k = next(i for i, l in enumerate(lines) if "proposal_method" in l)
    lines[k] = lines[k].replace("uniform2", "CauchySchwarz", 1)
    path = tmp_path / "C2_cs_walk"
    path.write_text("".join(lines))
    return str(path)


@pytest.mark.gpu
def test_walk_deck_end_to_end(tmp_path):
    deck = _cs_deck(tmp_path)
    r = subprocess.run([sys.executable, "-m", "sqmc_amd.run", "-i", deck, "--fcidump", FCIDUMP], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "CauchySchwarz" in r.stdout and "iblk, w_perm_initiator, nwalk, w_abs, w_abs_imp=" in r.stdout and "Energy=" in r.stdout
    from sqmc_amd.walk_run import parse_walk_deck, run_walk
    buf = io.StringIO()
    res = run_walk(parse_walk_deck(open(deck).read()), FCIDUMP, out=buf)
    assert " CauchySchwarz: 0 exchange integrals" in buf.getvalue()
    assert res["n_imp"] == 1002
    assert abs(res["energy"] - (-75.72854)) < max(5 * res["energy_err"], 3e-3), (res["energy"], res["energy_err"])


if __name__ == "__main__" and len(sys.argv) == 4 and sys.argv[1] == "worker":
    _walk_worker(sys.argv[2], sys.argv[3])
