"""proposal_method CauchySchwarz with time-reversal symmetry on the GPU: the test door bit for bit against the checker
(tests/cauchy_ts_checker.py), the sampled distribution of representatives against the enumerator, five REPLAY steps against the
checker plus numpy, the two tails and the chained run, the one-rank sharded walk, and a time-symmetric CauchySchwarz deck."""
import io
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import cauchy_checker as CC          # noqa: E402
from tests import cauchy_ts_checker as TS       # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
FCIDUMP = os.path.join(GOLD, "C2_r1.24253_FCIDUMP")
# (z, hf_symmetry, n_core_orb)
SYSTEMS = {"z+1": (1, 1, 0), "z-1": (-1, 2, 0), "z+1_core1": (1, 1, 1)}
TAU = 0.005314
SEED = (1346, 5634, 6635, 4361)


def _host(name):
    from sqmc_amd import host as H
    z, hs, nc = SYSTEMS[name]
    return H.ChemHost(FCIDUMP, 8, 4, "d2h", time_sym=True, z=z, n_core_orb=nc, hf_symmetry=hs)


def _mix48(k):
    v = (k * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & ((1 << 64) - 1)
    v ^= v >> 30; v = (v * 0xBF58476D1CE4E5B9) & ((1 << 64) - 1)
    v ^= v >> 27; v = (v * 0x94D049BB133111EB) & ((1 << 64) - 1)
    v ^= v >> 31
    return v & CC.MASK48


def _finish_all(g, cs, z, tau, moves):
    """TS.finish for every (iu, id, level, ju, jd, prob) of `moves`, the plain matrix elements of both pathways from
    sqmc_gpu_hamiltonian_chem_batch: a first pass collects the pairs the finish asks for, a second one uses them"""
    need = {}
    rec = lambda iu, id_, ju, jd, lev: need.setdefault((iu, id_, ju, jd), 0.0)
    for iu, id_, lev, ju, jd, p in moves:
        TS.finish(cs, z, tau, iu, id_, ju, jd, lev, p, rec)
    keys = list(need)
    if keys:
        a = [np.array([k[q] for k in keys], np.uint64) for q in range(4)]
        for k, v in zip(keys, g.hamiltonian_chem_batch(*a).tolist()):
            need[k] = v
    ham = lambda iu, id_, ju, jd, lev: need[(iu, id_, ju, jd)]
    return [TS.finish(cs, z, tau, iu, id_, ju, jd, lev, p, ham) for iu, id_, lev, ju, jd, p in moves]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_door_matches_checker_bit_for_bit(name):
    import sqmc_amd
    sqmc_amd.set_device(0)
    h = _host(name)
    z = SYSTEMS[name][0]
    cs = CC.from_host(h)
    g = h.gpu(proposal="cauchyschwarz", rng_mode=sqmc_amd.RNG_REPLAY, mwalk=0)
    try:
        assert h.hf_up <= h.hf_dn
        cu, cd = h.connected_all(h.hf_up, h.hf_dn)
        m = (1 << h.n_core_orb) - 1
        pool = [(int(u), int(d)) for u, d in zip(cu, cd) if (int(u), int(d)) != (h.hf_up, h.hf_dn) and (int(u) & m) == m and (int(d) & m) == m
                and not (z < 0 and int(u) == int(d))]
        assert all(u <= d for u, d in pool)
        rng = np.random.default_rng(11)
        parents = [(h.hf_up, h.hf_dn)] + [pool[k] for k in rng.choice(len(pool), size=199, replace=False)]
        n = 10000
        states = [_mix48(k) for k in range(n)]
        inv = pow(CC.LCG_MULT, -1, 1 << 48)        # states whose k-th draw is the largest, (2^48 - 1) / 2^48
        x = CC.MASK48
        for k in range(5):
            x = (x * inv) & CC.MASK48
            states[k] = x
        pu = np.array([parents[k % len(parents)][0] for k in range(n)], np.uint64)
        pd = np.array([parents[k % len(parents)][1] for k in range(n)], np.uint64)
        seeds = np.array([CC.state_limbs(s) for s in states], np.int32)
        ju, jd, wj, sa = g.propose_cauchy_schwarz_batch(TAU, pu, pd, seeds)
        base, after = [], []
        for k in range(n):
            r = CC.Rannyu(states[k])
            base.append(cs.move(int(pu[k]), int(pd[k]), r))
            after.append(r.x)
        assert np.array_equal(sa, np.array([CC.state_limbs(s) for s in after], np.int32))
        mv = [k for k in range(n) if base[k][0] > 0]
        fin = _finish_all(g, cs, z, TAU, [(int(pu[k]), int(pd[k]), base[k][0], base[k][1], base[k][2], base[k][3]) for k in mv])
        eu = np.array([b[1] for b in base], np.uint64); ed = np.array([b[2] for b in base], np.uint64); ew = np.zeros(n)
        for k, (a, b, w) in zip(mv, fin):
            eu[k], ed[k], ew[k] = a, b, w
        assert np.array_equal(ju, eu) and np.array_equal(jd, ed)
        assert np.array_equal(wj, ew)
        lev = np.array([b[0] for b in base])
        assert (lev == 1).sum() > 0 and (lev == 2).sum() > n // 2
        live = wj != 0
        assert np.all(ju[live] <= jd[live])
        # some det_j were swapped to their representative
        assert sum(1 for k, (a, b, w) in zip(mv, fin) if (a, b) != (base[k][1], base[k][2])) > 0
    finally:
        g.close()


@pytest.mark.gpu
def test_sampled_distribution_matches_enumerator():
    """2^22 proposals from one open-shell representative, one hashed seed each, against the enumerator's masses summed per
    representative (det_j and flip(det_j)): G-test at a fixed seed"""
    from scipy.stats import chi2
    import sqmc_amd
    sqmc_amd.set_device(0)
    h = _host("z+1")
    cs = CC.from_host(h)
    cu, cd = h.connected_all(h.hf_up, h.hf_dn)
    par = next((int(u), int(d)) for u, d in zip(cu, cd) if int(u) != int(d) and int(u) != h.hf_up and int(d) != h.hf_dn)
    paths, null, _ = cs.enumerate(*par)
    mass = {}
    for p in paths:
        a, b = p[5]
        r = (min(a, b), max(a, b))
        if r == par:
            null += p[6]                   # det_j = det_i or flip(det_i): weight 0
            continue
        mass[r] = mass.get(r, 0.0) + p[6]
    g = h.gpu(proposal="cauchyschwarz", rng_mode=sqmc_amd.RNG_REPLAY, mwalk=0)
    try:
        n = 1 << 22
        st = (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        st ^= st >> np.uint64(30); st *= np.uint64(0xBF58476D1CE4E5B9)
        st ^= st >> np.uint64(27); st *= np.uint64(0x94D049BB133111EB); st ^= st >> np.uint64(31)
        st &= np.uint64(CC.MASK48)
        seeds = np.stack([(st >> np.uint64(36)) & np.uint64(4095), (st >> np.uint64(24)) & np.uint64(4095),
                          (st >> np.uint64(12)) & np.uint64(4095), st & np.uint64(4095)], axis=1).astype(np.int32)
        ju, jd, wj, _ = g.propose_cauchy_schwarz_batch(TAU, np.full(n, par[0], np.uint64), np.full(n, par[1], np.uint64), seeds)
    finally:
        g.close()
    ru, rd = np.minimum(ju, jd), np.maximum(ju, jd)
    moved = (ru != np.uint64(par[0])) | (rd != np.uint64(par[1]))
    assert np.all(ju[moved] <= jd[moved])
    keys = sorted(mass)
    index = {k: i for i, k in enumerate(keys)}
    obs = np.zeros(len(keys) + 1)
    uniq, cnt = np.unique(np.stack([ru[moved], rd[moved]], axis=1), axis=0, return_counts=True)
    for (a, b), c in zip(uniq, cnt):
        obs[index[(int(a), int(b))]] += c
    obs[-1] = n - moved.sum()
    expv = np.array([mass[k] for k in keys] + [null]) * n
    small = expv < 5
    o = np.append(obs[~small], obs[small].sum()); e = np.append(expv[~small], expv[small].sum())
    keep = e > 0
    o, e = o[keep], e[keep]
    G = 2.0 * np.sum(np.where(o > 0, o * np.log(np.where(o > 0, o, 1) / e), 0.0))
    p = chi2.sf(G, len(o) - 1)
    assert p > 1e-6, (G, len(o), p)


def _replay_step(g, cs, z, wk, prm, state):
    """one REPLAY step of a plain time-symmetric walk restated (see test_gpu_cauchy_schwarz._replay_step): the gate and the CS
    proposals from the one rannyu stream, each ended by the checker's time-symmetric finish, death/clone with the time-symmetric H_ii"""
    r = CC.Rannyu(state)
    tau, cut = prm["tau"], prm["always_spawn_cutoff_wt"]
    kids, nch = [], 0
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
                kids.append(((u, d, lev, ju, jd, p), wc))
    fin = _finish_all(g, cs, z, tau, [k[0] for k in kids])
    hii = g.hamiltonian_batch(wk["up"], wk["dn"], wk["up"], wk["dn"])
    out = {}
    for u, d, w, e in zip(wk["up"].tolist(), wk["dn"].tolist(), wk["wt"].tolist(), hii.tolist()):
        v = w * (1.0 + tau * (prm["e_trial"] - e))
        out[(u, d)] = [v, abs(v)]
    for (_, wc), (a, b, wj) in zip(kids, fin):
        wj = wc * wj
        if wj == 0.0:
            continue
        acc = out.setdefault((a, b), [0.0, 0.0])
        acc[0] += wj; acc[1] += abs(wj)
    return out, nch, r.x


@pytest.mark.gpu
def test_replay_step_matches_checker():
    """Five chained REPLAY steps of a plain (semistochastic = f, min_wt = 0) time-symmetric CS walk against the checker plus numpy:
    RNG state and child count equal, walkers within 1e-12.  The finish draws nothing, so k_replay_prepass's counting holds."""
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    h = _host("z+1")
    cs = CC.from_host(h)
    g = h.gpu(proposal="cauchyschwarz", rng_mode=sqmc_amd.RNG_REPLAY, seed=SEED, mwalk=200000)
    try:
        s = h.setup_walk(g, 100, 1000, 0.1)
        g.set_ct_table(s.ct_up, s.ct_dn, s.ct_num, s.ct_den)
        wk = H.initial_walkers(s, 100)
        keep = wk["wt"] != 0
        wk = {k: v[keep] for k, v in wk.items()}
        prm = dict(tau=s.tau, e_trial=s.e_trial0, reweight_factor_inv=1.0, r_initiator=1.0, min_wt=0.0, always_spawn_cutoff_wt=0.5,
                   initiator_power=0, initiator_min_distance=0, c_t_initiator=0, semistochastic=0, reached_w_abs_gen=0)
        n_gate = n_multi = 0
        for step in range(5):
            n = len(wk["up"])
            wk = dict(up=wk["up"], dn=wk["dn"], wt=wk["wt"], imp_distance=np.ones(n, np.int8), initiator=np.full(n, 2, np.int8),
                      perm_sign=np.zeros(n, np.int8), matrix_elements=np.full(n, 1e51), e_num=np.full(n, 1e51), e_den=np.full(n, 1e51))
            assert np.all(wk["up"] <= wk["dn"])
            n_gate += int((np.abs(wk["wt"]) < 0.5).sum()); n_multi += int((np.abs(wk["wt"]) >= 1.5).sum())
            g.upload_walkers(wk)
            state = CC.limbs_state(g.rng_state())
            want, nch, state_after = _replay_step(g, cs, h.z, wk, prm, state)
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
        assert n_gate > 0 and n_multi > 0
    finally:
        g.close()


WORKER_STEPS = 50


def _walk_worker(out, mode):
    """a time-symmetric CS walk under COUNTER: `step` -- WORKER_STEPS steps one by one; `run` -- one chained sqmc_gpu_run"""
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    h = _host("z+1")
    w = H.GpuWalk(h, 2000, w_begin=100, seed=SEED, rng_mode=H.RNG_COUNTER, proposal="cauchyschwarz")
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
    assert np.array_equal(bucket["up"], radix["up"]) and np.array_equal(bucket["dn"], radix["dn"])
    assert np.array_equal(bucket["initiator"], radix["initiator"])
    assert np.allclose(bucket["wt"], radix["wt"], rtol=1e-11, atol=0)
    assert np.allclose(bucket["outs"][:, :16], radix["outs"][:, :16], rtol=1e-11, atol=1e-11)
    for k in ("up", "dn", "wt", "initiator"):
        assert np.array_equal(chained[k], bucket[k]), k
    for r in (bucket, radix, chained):
        assert np.all(r["up"] <= r["dn"]) and len(r["up"]) > 100


SH_STEPS, SH_BEGIN, SH_TARGET = 40, 2000, 20000


def _sharded_worker(port, outdir):
    import torch                                   # before the HIP library (one libamdhip64 per process)
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=0, world_size=1)
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    w = H.ShardedWalk(_host("z+1"), SH_TARGET, 0, 1, w_begin=SH_BEGIN, seed=SEED, mwalk=400000, proposal="cauchyschwarz")
    outs = np.array([w.step().copy() for _ in range(SH_STEPS)])
    wk = w.g.download_walkers()
    np.savez(os.path.join(outdir, "sharded.npz"), outs=outs, **wk)
    w.close()
    dist.barrier()
    dist.destroy_process_group()


def _single_worker(outdir):
    os.environ["SQMC_BUCKET"] = "0"                # the radix tail, the one the sharded step runs
    sys.path.insert(0, ROOT)
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    ref = H.GpuWalk(_host("z+1"), SH_TARGET, w_begin=SH_BEGIN, seed=SEED, mwalk=400000, proposal="cauchyschwarz")
    outs = np.array([ref.step().copy() for _ in range(SH_STEPS)])
    wk = ref.g.download_walkers()
    np.savez(os.path.join(outdir, "single.npz"), outs=outs, tail=np.array(ref.g.tail_stats()), **wk)
    ref.close()


@pytest.mark.gpu
def test_one_rank_sharded_equals_single_rank(tmp_path, monkeypatch):
    """a uniform2 time-symmetric walk runs on a sharded context, so the time-symmetric CS walk does too: one rank equals the
    single-GPU walk bit for bit on the radix tail"""
    monkeypatch.setenv("SQMC_SHARD_BUCKET", "0")
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    ps = ctx.Process(target=_sharded_worker, args=(29771, str(tmp_path)))
    ps.start(); ps.join(600)
    assert ps.exitcode == 0
    pr = ctx.Process(target=_single_worker, args=(str(tmp_path),))
    pr.start(); pr.join(600)
    assert pr.exitcode == 0
    res = np.load(os.path.join(str(tmp_path), "sharded.npz"))
    wk = np.load(os.path.join(str(tmp_path), "single.npz"))
    assert tuple(wk["tail"]) == (0, 0)
    assert np.array_equal(res["up"], wk["up"]) and np.array_equal(res["dn"], wk["dn"])
    assert np.array_equal(res["wt"], wk["wt"]) and np.array_equal(res["initiator"], wk["initiator"])
    assert np.allclose(res["outs"], wk["outs"], rtol=1e-12, atol=1e-12)
    assert np.all(res["up"] <= res["dn"]) and len(res["up"]) > 1000


def _ts_deck(tmp_path):
    txt = open(os.path.join(GOLD, "C2_r1.24253_i_walk")).read()
    txt = re.sub(r"^uniform2(\s)", r"CauchySchwarz\1", txt, count=1, flags=re.M)
    txt = re.sub(r"^\.false\.(\s+time_sym)", ".true.\\1\n1                                 z", txt, count=1, flags=re.M)
    path = tmp_path / "C2_cs_ts_walk"
    path.write_text(txt)
    return str(path)


@pytest.mark.gpu
def test_walk_deck_end_to_end(tmp_path):
    deck = _ts_deck(tmp_path)
    r = subprocess.run([sys.executable, "-m", "sqmc_amd.run", "-i", deck, "--fcidump", FCIDUMP], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "CauchySchwarz" in r.stdout and "iblk, w_perm_initiator, nwalk, w_abs, w_abs_imp=" in r.stdout and "Energy=" in r.stdout
    from sqmc_amd.walk_run import parse_walk_deck, run_walk
    buf = io.StringIO()
    res = run_walk(parse_walk_deck(open(deck).read()), FCIDUMP, out=buf)
    assert " CauchySchwarz: 0 exchange integrals" in buf.getvalue()
    assert abs(res["energy"] - (-75.7285)) < max(5 * res["energy_err"], 3e-3), (res["energy"], res["energy_err"])


if __name__ == "__main__" and len(sys.argv) == 4 and sys.argv[1] == "worker":
    _walk_worker(sys.argv[2], sys.argv[3])
