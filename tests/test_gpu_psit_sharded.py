"""hf_to_psit on the sharded walk (sqmc_gpu_set_hf_to_psit_shard): several processes share one GPU and exchange through gloo
(caller-driven, sqmc_gpu_shard_finish_psit) or the library's own exchange (RCCL at one rank, the tests/fake_rccl transport double
at several).  One rank must be the one-rank hf_to_psit walk bit for bit; more ranks must keep the layout of the variant on every
rank -- its C(T) share at the head of its list, in C(T) order, at every step -- and every sharding invariant."""
import os
import sys
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")
FAKE_DIR = os.path.join(ROOT, "tests", "fake_rccl")
SEED = (1346, 5634, 6635, 4361)
NSTEPS, W_BEGIN, W_TARGET = 40, 100.0, 20000


def _fake_rccl_lib():
    import subprocess
    so, src = os.path.join(FAKE_DIR, "libfake_rccl.so"), os.path.join(FAKE_DIR, "fake_rccl.cpp")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-fPIC", "-shared", "-Wno-unused-result", src, "-o", so, "-lrt"])
    return so


def _host(H, system):
    if system == "heg":       # 14 electrons, 19 plane waves
        return H.HegHost(3, 0.5, 14, 7, 1.49), dict(n_truncate_trial_wf=20, size_deterministic=250)
    return H.ChemHost(FCIDUMP, 8, 4, "d2h"), {}


def _check_layout(H, w, rank, world):
    """this rank's list: its C(T) share first, in C(T) order (zero weights included), then its survivors outside C(T), sorted;
    nothing another rank owns"""
    wk = w.g.download_walkers()
    tb, s = w.shard_tables, w.setup
    n = len(tb["ct_index"])
    ok = np.array_equal(wk["up"][:n], s.ct_up[tb["ct_index"] - 1]) and np.array_equal(wk["dn"][:n], s.ct_dn[tb["ct_index"] - 1])
    u, d = wk["up"][n:], wk["dn"][n:]
    ok = ok and bool(np.all((u[1:] > u[:-1]) | ((u[1:] == u[:-1]) & (d[1:] > d[:-1]))))
    ok = ok and bool(np.all(w.g.det_owner(wk["up"], wk["dn"], world) == rank))
    ok = ok and (len(u) == 0 or int(wk["imp_distance"][n:].min()) >= 1)
    return ok, wk


def _worker(rank, world, port, outdir, system="c2", mode="gloo", sum_order=1, nsteps=NSTEPS, owner_hash=0, walk_kw=None, tag="",
            seed=SEED, w_target=W_TARGET, run_only=False):
    if mode == "fake":
        os.environ["SQMC_RCCL_LIB"] = _fake_rccl_lib()
    import torch                                   # noqa: F401  (before the HIP library: one libamdhip64 per process)
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    hst, kw = _host(H, system)
    kw.update(walk_kw or {})
    w = H.ShardedWalk(hst, w_target, rank, world, w_begin=W_BEGIN, seed=seed, mwalk=400000, owner_hash=owner_hash, hf_to_psit=True,
                      sum_order=sum_order, **kw)
    if mode != "gloo":
        w.attach_rccl()
    outs, layout = [], []
    if run_only:
        w.pc.n_equil = 1500
        w.run(1500, keep_stats=False)
        _, tot = w.run(nsteps, keep_stats=False)
        outs = np.array([tot])
    else:
        n_step = nsteps if mode == "gloo" else nsteps // 2
        for _ in range(n_step):
            outs.append(w.step().copy())
            layout.append(_check_layout(H, w, rank, world)[0])
        if mode != "gloo":                         # the rest inside sqmc_gpu_shard_run
            b, _ = w.run(nsteps - n_step)
            outs = list(outs) + list(b)
            layout.append(_check_layout(H, w, rank, world)[0])
        outs = np.array(outs)
    wk = w.g.download_walkers()
    tb = w.shard_tables
    np.savez(os.path.join(outdir, "rank%d%s.npz" % (rank, tag)), outs=outs, layout=np.array(layout, bool), own_first=tb["own_first"],
             n_ct_local=len(tb["ct_index"]), n_psit_local=len(tb["psit_mask"]), n_ct=len(w.setup.ct_up),
             n_imp=int(np.count_nonzero(w.shard_tables["walkers"]["imp_distance"] == 0)), **wk)
    w.close()
    dist.barrier()
    dist.destroy_process_group()


def _run(world, outdir, port, **kw):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    ps = [ctx.Process(target=_worker, args=(r, world, port, str(outdir)), kwargs=kw) for r in range(world)]
    for p in ps: p.start()
    for p in ps: p.join(600)
    alive = [p for p in ps if p.is_alive()]
    for p in alive: p.terminate()
    assert not alive, "sharded hf_to_psit walk did not finish (deadlock?)"
    assert all(p.exitcode == 0 for p in ps), [p.exitcode for p in ps]
    return [np.load(os.path.join(str(outdir), "rank%d%s.npz" % (r, kw.get("tag", "")))) for r in range(world)]


def _one_rank_worker(outdir, system, sum_order, nsteps):
    sys.path.insert(0, ROOT)
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    hst, kw = _host(H, system)
    g = H.GpuWalk(hst, W_TARGET, w_begin=W_BEGIN, seed=SEED, mwalk=400000, hf_to_psit=True, sum_order=sum_order, **kw)
    outs = np.array([g.step().copy() for _ in range(nsteps)])
    np.savez(os.path.join(outdir, "one.npz"), outs=outs, **g.g.download_walkers())
    g.close()


def _one_rank(outdir, system, sum_order, nsteps=NSTEPS):
    import torch.multiprocessing as mp
    pr = mp.get_context("spawn").Process(target=_one_rank_worker, args=(str(outdir), system, sum_order, nsteps))
    pr.start(); pr.join(600)
    assert pr.exitcode == 0
    return np.load(os.path.join(str(outdir), "one.npz"))


def _same_walk(a, ref):
    for k in ("up", "dn", "wt", "initiator", "imp_distance"):
        assert np.array_equal(a[k], ref[k]), k
    assert np.allclose(a["outs"], ref["outs"], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("system,sum_order,modes", [("c2", 1, ("gloo", "rccl", "fake")), ("c2", 0, ("gloo", "fake")), ("heg", 1, ("gloo", "fake"))])
def test_one_rank_sharded_psit_equals_one_rank_psit(tmp_path, system, sum_order, modes):
    """one rank: the caller-driven step (gloo), the library's step and run (single-rank RCCL, the transport double) all walk the
    one-rank hf_to_psit trajectory; the in-library runs switch to sqmc_gpu_shard_run half way, so shard_run = repeated shard_step"""
    ref = _one_rank(tmp_path, system, sum_order)
    for k, mode in enumerate(modes):
        res = _run(1, tmp_path, 29710 + 10 * sum_order + k + (50 if system == "heg" else 0), system=system, mode=mode, sum_order=sum_order, tag=mode)[0]
        assert bool(res["own_first"]) and int(res["n_ct_local"]) == int(res["n_ct"])
        assert res["layout"].all()
        _same_walk(res, ref)


def _invariants(res, world):
    for r in res[1:]:
        assert np.array_equal(r["outs"][:, :7], res[0]["outs"][:, :7])          # the all-reduced sums: the same bits on every rank
    assert all(r["layout"].all() for r in res)                                   # C(T) share first, in order, owner-only, every step
    assert sum(bool(r["own_first"]) for r in res) == 1
    assert sum(int(r["n_ct_local"]) for r in res) == int(res[0]["n_ct"])
    keys = []
    for r in res:
        keys += [(int(a), int(b)) for a, b in zip(r["up"], r["dn"])]
        assert np.count_nonzero(r["imp_distance"] == 0) == int(r["n_imp"])
    assert len(keys) == len(set(keys))                                           # a determinant lives on one rank only
    assert int(res[0]["outs"][-1][5]) == len(keys)                               # global nwalk = the sum of the shards
    assert np.isclose(sum(float(np.abs(r["wt"]).sum()) for r in res), res[0]["outs"][-1][1], rtol=1e-12)


def test_two_ranks_gloo_deterministic(tmp_path):
    a = _run(2, tmp_path, 29801, tag="a")
    _invariants(a, 2)
    b = _run(2, tmp_path, 29802, tag="b")
    for x, y in zip(a, b):
        for k in ("outs", "up", "dn", "wt", "initiator"):
            assert np.array_equal(x[k], y[k]), k
    assert len(a[0]["up"]) + len(a[1]["up"]) > 3000


@pytest.mark.parametrize("mode", ["gloo", "fake"])
def test_three_ranks_first_state_off_rank_0(tmp_path, mode):
    """the reference's owner hash puts the first state of C2 on rank 1 of 3: ranks 0 and 2 carry no first state, the T^-1 update reaches
    them through the exchange"""
    res = _run(3, tmp_path, 29811 if mode == "gloo" else 29812, mode=mode, owner_hash=1)
    assert [bool(r["own_first"]) for r in res] == [False, True, False]
    _invariants(res, 3)
    if mode == "fake":          # the library's run, twice: the same bits
        again = _run(3, tmp_path, 29813, mode=mode, owner_hash=1, tag="b")
        for x, y in zip(res, again):
            assert np.array_equal(x["outs"], y["outs"]) and np.array_equal(x["wt"], y["wt"])


def test_rank_without_psit_determinant(tmp_path):
    """a four-determinant Psi_T over three ranks (the reference's owner hash): rank 0 holds C(T) determinants but no Psi_T one"""
    res = _run(3, tmp_path, 29821, owner_hash=1, walk_kw=dict(n_truncate_trial_wf=3))
    assert int(res[0]["n_psit_local"]) == 0 and int(res[0]["n_ct_local"]) > 0
    assert sum(int(r["n_psit_local"]) for r in res) >= 2
    _invariants(res, 3)


def test_two_rank_psit_energy(tmp_path):
    """C2: the projected energy of 2-rank hf_to_psit runs (the library's exchange over the transport double) agrees with the one-rank
    hf_to_psit walk's and with this geometry's HCI+PT2 total, to the tolerances of the one-rank test"""
    from sqmc_amd import host as H
    seeds = ((1346, 5634, 6635, 4361), (2726, 5165, 6543, 6524), (911, 2202, 3303, 4405))
    two, one = [], []
    for k, seed in enumerate(seeds):
        res = _run(2, tmp_path, 29831 + k, mode="fake", seed=seed, nsteps=2500, run_only=True, tag="e%d" % k)
        assert np.array_equal(res[0]["outs"][:, :7], res[1]["outs"][:, :7])
        two.append(res[0]["outs"][0][3] / res[0]["outs"][0][2])
    import sqmc_amd
    sqmc_amd.set_device(0)
    h = H.ChemHost(FCIDUMP, 8, 4, "d2h")
    for seed in seeds:
        gw = H.GpuWalk(h, W_TARGET, w_begin=W_BEGIN, hf_to_psit=True, seed=seed)
        gw.pc.n_equil = 1500
        gw.run(1500, keep_stats=False)
        _, tot = gw.run(2500, keep_stats=False)
        one.append(tot[3] / tot[2])
        gw.close()
    es = {True: np.array(two), False: np.array(one)}
    mean = {k: v.mean() for k, v in es.items()}
    err = {k: max(v.std(ddof=1) / np.sqrt(len(v)), 3e-4) for k, v in es.items()}
    assert abs(mean[True] - mean[False]) < 4 * np.hypot(err[True], err[False]), (es, mean, err)
    assert abs(mean[True] - (-75.72854)) < 4 * err[True] + 2e-3, (es, mean, err)
