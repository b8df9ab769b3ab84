"""proposal_method fast_heatbath on the sharded walk.  A heat-bath child holds two walker slots (the single and the double excitation
of one proposal, do_walk.f90:3604-3611), so a sharded step has 2 * nch spawn slots: the capacity check, the routing by owner, the
packing and the in-library exchange all count slots, while n_children stays a count of proposals.

The system is the shipped C2 cc-pVDZ integrals with 10 electrons, on which the reference's own check accepts heat-bath
(tests/golden/README_heatbath.md).  Several processes share one GPU, as in tests/test_gpu_sharded.py: gloo for the caller-driven
exchange, the tests/fake_rccl transport double for the library's own."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.test_gpu_sharded import FCIDUMP, NSTEPS, SEED, W_BEGIN, W_TARGET, _fake_rccl_lib  # noqa: E402

pytestmark = pytest.mark.gpu
HB = {"proposal": "heatbath"}
MWALK = 400000
ERR_MWALK, ERR_SPAWN_OVERFLOW, ERR_UNSUPPORTED = 1, 2, -3      # include/sqmc_gpu.h
JOIN_S = 300                      # time limit of every process join; a worker alive after it fails the test
PROFILE = os.path.join(ROOT, "profiles", "heatbath_sharded.json")


# ---------------------------------------------------------------------------------------------------------------- workers
def _gloo_worker(rank, world, port, outdir, w_begin=None, w_target=None, nsteps=None, walk_kw=None, mwalk=MWALK):
    """caller-driven sharded heat-bath walk (sqmc_gpu_shard_begin / _pack / _finish, exchanges through gloo); a walk that the library
    stops is recorded with its status and the steps it finished"""
    w_begin, w_target, nsteps = w_begin or W_BEGIN, w_target or W_TARGET, nsteps or NSTEPS
    import torch                                   # noqa: F401  (before the HIP library: one libamdhip64 per process)
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    hst = H.ChemHost(FCIDUMP, 10, 5, "d2h")
    w = H.ShardedWalk(hst, w_target, rank, world, w_begin=w_begin, seed=SEED, mwalk=mwalk, **dict(HB, **(walk_kw or {})))
    status, msg, outs = 0, "", []
    try:
        for _ in range(nsteps):
            outs.append(w.step().copy())
    except sqmc_amd.SqmcGpuError as exc:
        status, msg = exc.code, str(exc)
    wk = w.g.download_walkers()                    # after a refused step: the list the step found
    owner = w.g.det_owner(wk["up"], wk["dn"], world)
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), outs=np.array(outs).reshape(-1, 16), owner=owner, n_imp_global=w.n_imp_global,
             status=np.array([status]), msg=np.array([msg]), **wk)
    w.close()
    dist.barrier()
    dist.destroy_process_group()


def _single_worker(outdir, seed=SEED, nsteps=None, name="single_hb.npz"):
    """the single-GPU heat-bath walk on the radix tail (heat-bath steps always take it)"""
    sys.path.insert(0, ROOT)
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    hst = H.ChemHost(FCIDUMP, 10, 5, "d2h")
    ref = H.GpuWalk(hst, W_TARGET, w_begin=W_BEGIN, seed=seed, mwalk=MWALK, proposal="heatbath")
    outs = np.array([ref.step().copy() for _ in range(nsteps or NSTEPS)])
    wk = ref.g.download_walkers()
    np.savez(os.path.join(outdir, name), outs=outs, tail=np.array(ref.g.tail_stats()), **wk)
    ref.close()


def _inlib_worker(rank, world, port, outdir, fake, w_begin=None, w_target=None, nsteps=None, mwalk=MWALK):
    """the library's own exchange over the transport double: half the steps through sqmc_gpu_shard_step, half through the
    (pipelined, once the target is reached) sqmc_gpu_shard_run"""
    w_begin, w_target, nsteps = w_begin or W_BEGIN, w_target or W_TARGET, nsteps or NSTEPS
    import torch                                   # noqa: F401
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ["SQMC_RCCL_LIB"] = fake             # before the library binds its communication entry points
    dist.init_process_group("gloo", rank=rank, world_size=world)     # only carries the unique id
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    hst = H.ChemHost(FCIDUMP, 10, 5, "d2h")
    w = H.ShardedWalk(hst, w_target, rank, world, w_begin=w_begin, seed=SEED, mwalk=mwalk, **HB)
    w.attach_rccl()
    outs = [w.step().copy() for _ in range(nsteps // 2)]
    b, _ = w.run(nsteps - nsteps // 2)
    outs = np.concatenate([np.array(outs), b])
    wk = w.g.download_walkers()
    owner = w.g.det_owner(wk["up"], wk["dn"], world)
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), outs=outs, owner=owner, n_imp_global=w.n_imp_global, reached=np.array([w.pc.reached]), **wk)
    w.close()
    dist.barrier()
    dist.destroy_process_group()


def _pack_worker(outdir, owner_hash):
    """One spawn step of a plain walk on a context configured as rank 0 of 1 and on one configured as rank 0 of 2: same walker list,
    same raw seed, same step number, hence the same children; the send buffers and counts of both."""
    import torch                                   # before the HIP library
    sys.path.insert(0, ROOT)
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    hst = H.ChemHost(FCIDUMP, 10, 5, "d2h")
    res, s, wk = {}, None, None
    for world in (1, 2):
        g = hst.gpu(rng_mode=H.RNG_COUNTER, seed=SEED, mwalk=MWALK)
        g.set_owner_hash(owner_hash)
        assert g.setup_efficient_heatbath()
        if s is None:
            s = hst.setup_walk(g, 100, 1000, 0.1)
            cu, cd = hst.connected_all(hst.hf_up, hst.hf_dn)          # sorted, unique: 2090 determinants; with those of a neighbour, more than 3000
            for k in (1, 2, 3):
                if len(cu) >= 3000:
                    break
                bu, bd = hst.connected_all(int(cu[k]), int(cd[k]))
                cu, cd = np.concatenate((cu, bu)), np.concatenate((cd, bd))
                o = H.sort_dets(cu, cd)
                cu, cd = cu[o], cd[o]
                new = np.ones(len(cu), bool); new[1:] = (cu[1:] != cu[:-1]) | (cd[1:] != cd[:-1])
                cu, cd = cu[new], cd[new]
            n = min(3000, len(cu))
            i = np.arange(n)
            wk = dict(up=cu[:n].copy(), dn=cd[:n].copy(), wt=np.where(i % 2 == 0, 1.0, -1.0) * (3.0 + (i % 5)),
                      imp_distance=np.ones(n, np.int8), initiator=np.full(n, 2, np.int8), perm_sign=np.zeros(n, np.int8),
                      matrix_elements=np.full(n, 1e51), e_num=np.full(n, 1e51), e_den=np.full(n, 1e51))
        g.set_ct_table(s.ct_up, s.ct_dn, s.ct_num, s.ct_den)
        g.shard_config(0, world, [])
        g.upload_walkers(wk)
        prm = H.PopControl(s.tau, s.e_trial0, 1e5).params(min_wt=0.5, semistochastic=0)
        dev = torch.device("cuda", 0)
        xg = torch.zeros(1, dtype=torch.float64, device=dev)
        send = torch.zeros((MWALK, 4), dtype=torch.int64, device=dev)
        nch = g.shard_begin(prm, xg.data_ptr())
        counts = g.shard_pack(prm, xg.data_ptr(), send.data_ptr(), MWALK, world)
        torch.cuda.synchronize()
        ns = int(counts.sum())
        rec = send[:ns].cpu().numpy().view(np.uint64)
        own = g.det_owner(rec[:, 0], rec[:, 1], 2)
        res["nch%d" % world], res["counts%d" % world], res["rec%d" % world], res["own%d" % world] = nch, counts, rec, own
        # the same step packed again (nothing of it is consumed before sqmc_gpu_shard_finish; the owners now come from the k_child_owner
        # fallback, k_spawn's were used up): into a buffer said to be one record short, then into one that just fits
        short = torch.full((MWALK, 4), -1, dtype=torch.int64, device=dev)
        try:
            g.shard_pack(prm, xg.data_ptr(), short.data_ptr(), ns - 1, world)
            code = 0
        except sqmc_amd.SqmcGpuError as exc:
            code = exc.code
        torch.cuda.synchronize()
        res["short_code%d" % world], res["short_untouched%d" % world] = code, bool((short == -1).all().item())
        counts_b = g.shard_pack(prm, xg.data_ptr(), short.data_ptr(), ns, world)
        torch.cuda.synchronize()
        res["counts_again%d" % world], res["rec_again%d" % world] = counts_b, short[:ns].cpu().numpy().view(np.uint64)
        res["tail_untouched%d" % world] = bool((short[ns:] == -1).all().item())
        g.close()
    np.savez(os.path.join(outdir, "pack%d.npz" % owner_hash), n_list=len(wk["up"]), **res)


def _refusal_worker(outdir):
    """heat-bath tables together with sqmc_gpu_set_hf_to_psit_shard, in either order; the ShardedWalk front door"""
    import torch                                   # noqa: F401
    sys.path.insert(0, ROOT)
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    hst = H.ChemHost(FCIDUMP, 10, 5, "d2h")
    got = {}

    def psit_ctx(tables_first):
        g = hst.gpu(rng_mode=H.RNG_COUNTER, seed=SEED, mwalk=MWALK)
        if tables_first:
            assert g.setup_efficient_heatbath()
        s = hst.setup_walk(g, 100, 1000, 0.1, rediagonalize=True)
        ix, cdet, diag, pc_, pi_, pv_, in_imp = H.psit_tables(g, s)
        owner = g.det_owner(s.ct_up, s.ct_dn, 1)
        tb = H.psit_shard_tables(s, ix, cdet, diag, in_imp, owner, 0, 100.0)
        g.set_projector(pc_, pi_, pv_)
        g.set_ct_table(s.ct_up, s.ct_dn, s.ct_num, s.ct_den)
        g.shard_config(0, 1, tb["imp_rows"])
        return g, tb, cdet

    g, tb, cdet = psit_ctx(True)                    # tables, then hf_to_psit
    try:
        g.set_hf_to_psit_shard(tb["ct_index"], tb["diag"], tb["psit_slot"], tb["psit_mask"], cdet, 1)
        got["tables_first"] = (0, "")
    except sqmc_amd.SqmcGpuError as exc:
        got["tables_first"] = (exc.code, str(exc))
    g.close()
    g, tb, cdet = psit_ctx(False)                   # hf_to_psit, then tables (built by the library, and handed over)
    g.set_hf_to_psit_shard(tb["ct_index"], tb["diag"], tb["psit_slot"], tb["psit_mask"], cdet, 1)
    try:
        g.setup_efficient_heatbath()
        got["psit_first"] = (0, "")
    except sqmc_amd.SqmcGpuError as exc:
        got["psit_first"] = (exc.code, str(exc))
    g.close()
    for key, kw, host in (("walk_psit", dict(HB, hf_to_psit=True), hst), ("walk_8e", HB, H.ChemHost(FCIDUMP, 8, 4, "d2h"))):
        try:
            H.ShardedWalk(host, W_TARGET, 0, 1, w_begin=W_BEGIN, seed=SEED, mwalk=MWALK, **kw).close()
            got[key] = (0, "")
        except ValueError as exc:
            got[key] = (-1, str(exc))
    with open(os.path.join(outdir, "refusals.json"), "w") as f:
        json.dump(got, f)


# ---------------------------------------------------------------------------------------------------------------- helpers
def _join(ps, what):
    for p in ps: p.start()
    for p in ps: p.join(JOIN_S)
    alive = [p for p in ps if p.is_alive()]
    for p in alive: p.terminate()
    assert not alive, what + " did not finish within its time limit"
    assert all(p.exitcode == 0 for p in ps), [p.exitcode for p in ps]


def _run_gloo(world, outdir, port, **kw):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    os.makedirs(str(outdir), exist_ok=True)
    _join([ctx.Process(target=_gloo_worker, args=(r, world, port, str(outdir)), kwargs=kw) for r in range(world)], "sharded heat-bath walk")
    return [np.load(os.path.join(str(outdir), "rank%d.npz" % r)) for r in range(world)]


def _run_inlib(world, outdir, port, **kw):
    import torch.multiprocessing as mp
    fake = _fake_rccl_lib()
    ctx = mp.get_context("spawn")
    os.makedirs(str(outdir), exist_ok=True)
    _join([ctx.Process(target=_inlib_worker, args=(r, world, port, str(outdir), fake), kwargs=kw) for r in range(world)], "in-library exchange")
    return [np.load(os.path.join(str(outdir), "rank%d.npz" % r)) for r in range(world)]


def _run_single(outdir, **kw):
    import torch.multiprocessing as mp
    os.makedirs(str(outdir), exist_ok=True)
    _join([mp.get_context("spawn").Process(target=_single_worker, args=(str(outdir),), kwargs=kw)], "single-GPU heat-bath walk")
    return np.load(os.path.join(str(outdir), kw.get("name", "single_hb.npz")))


@pytest.fixture(scope="module")
def single_hb(tmp_path_factory):
    """the single-GPU heat-bath walk (the one test_heatbath_walk_trajectory_bit_exact pins to the oracle): computed once, read-only"""
    return _run_single(tmp_path_factory.mktemp("single_hb"))


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    """the one-rank sharded heat-bath walk on the radix tail (the workers inherit the environment)"""
    old = os.environ.get("SQMC_SHARD_BUCKET")
    os.environ["SQMC_SHARD_BUCKET"] = "0"
    try:
        return _run_gloo(1, tmp_path_factory.mktemp("one_rank"), 29801)[0]
    finally:
        if old is None: del os.environ["SQMC_SHARD_BUCKET"]
        else: os.environ["SQMC_SHARD_BUCKET"] = old


@pytest.fixture(scope="module")
def two_rank_gloo(tmp_path_factory):
    """the two-rank walk over gloo, twice"""
    d = tmp_path_factory.mktemp("two_rank")
    return [_run_gloo(2, d / ("run%d" % k), 29811 + k) for k in range(2)]


def _invariants(res):
    for r in res[1:]:
        assert np.array_equal(r["outs"][:, :7], res[0]["outs"][:, :7])      # every rank saw the same all-reduced sums
    keys, n_imp = [], 0
    for rank, r in enumerate(res):
        assert np.all(r["owner"] == rank)                                    # every walker sits on its owner
        k = [(int(a), int(b)) for a, b in zip(r["up"], r["dn"])]
        assert k == sorted(set(k))
        keys += k
        n_imp += int((r["imp_distance"] == 0).sum())
    assert len(keys) == len(set(keys))                                       # no determinant on two ranks
    out = res[0]["outs"][-1]
    assert int(out[5]) == len(keys) and len(keys) > 2000                     # global nwalk = total over ranks
    assert np.isclose(sum(float(np.abs(r["wt"]).sum()) for r in res), out[1], rtol=1e-12, atol=0)
    assert n_imp == int(res[0]["n_imp_global"])


def _energy(outs):
    return float(outs[10:, 3].sum() / outs[10:, 2].sum())


def _same_run(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x["outs"], y["outs"])
        for k in ("up", "dn", "wt", "initiator", "imp_distance"):
            assert np.array_equal(x[k], y[k]), k


# ---------------------------------------------------------------------------------------------------------------- tests
def test_one_rank_sharded_heatbath_equals_single_gpu_heatbath(one_rank, single_hb):
    """With one rank the sharded pipeline (two slots per child bucketed, packed, unpacked) must walk the single-GPU heat-bath
    trajectory: walkers, weights and flags bit for bit, all 16 sums of every step to 1e-12.  The single-GPU walk is the one
    test_heatbath_walk_trajectory_bit_exact pins to the oracle; everything else in this file is measured against this test."""
    res, wk = one_rank, single_hb
    assert int(res["status"][0]) == 0 and tuple(wk["tail"]) == (0, 0)
    assert len(wk["up"]) > 2000 and len(res["outs"]) == NSTEPS
    for k in ("up", "dn", "wt", "initiator"):
        assert np.array_equal(res[k], wk[k]), k
    assert np.allclose(res["outs"], wk["outs"], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("owner_hash", [0, 1])
def test_pack_routes_every_slot(tmp_path, owner_hash):
    """sqmc_gpu_shard_begin + sqmc_gpu_shard_pack of ONE plain step on a context configured as rank 0 of 1 and on one configured as
    rank 0 of 2, from the same walker list, seed and step number -- the children depend on nothing else, so both propose the same
    ones.  The one-rank context packs every filled slot in slot order; the two-rank context must route exactly those records, each
    to the owner of its own determinant, in the same order inside a bucket, and none of the empty slots.

    The test cannot tell which records are a child's SECOND slot.  That both slots are covered rests on the rate
    test_heatbath_proposals_bit_exact measures for this system -- more than 20 of 10^4 proposals fill both slots -- and on the step
    having at least 10^4 children (asserted below): a pack that dropped or misrouted second slots would lose records of the one-rank
    list, whose own packing of both slots the one-rank trajectory test pins."""
    import torch.multiprocessing as mp
    _join([mp.get_context("spawn").Process(target=_pack_worker, args=(str(tmp_path), owner_hash))], "pack worker")
    r = np.load(os.path.join(str(tmp_path), "pack%d.npz" % owner_hash))
    nch = int(r["nch1"])
    assert nch >= 10000 and int(r["n_list"]) == 3000
    assert int(r["nch2"]) == nch                                             # 1. the same children
    c1, c2, rec1, rec2 = r["counts1"], r["counts2"], r["rec1"], r["rec2"]
    assert len(c1) == 1 and len(c2) == 2 and int(c1.sum()) == int(c2.sum()) == len(rec1) == len(rec2)      # 2. the same record count
    assert c2.min() > 0
    own2 = r["own2"]
    assert np.all(own2[:c2[0]] == 0) and np.all(own2[c2[0]:] == 1)           # 3. every record in the bucket of its determinant's owner
    own1 = r["own1"]                                                         # (owner among 2 ranks of the one-rank list's records)
    for q, b in enumerate((rec2[:c2[0]], rec2[c2[0]:])):
        assert np.array_equal(b, rec1[own1 == q])                            # 4. each bucket: the one-rank list's records of that owner, in order
    assert sorted(map(tuple, rec1.tolist())) == sorted(map(tuple, rec2.tolist()))      # 5. together: the one-rank list as a multiset
    for rec in (rec1, rec2):
        assert np.all(rec[:, 2].view(np.float64) != 0.0)                     # 6. no empty slot was packed
        assert np.all(rec[:, 3] >> np.uint64(32) == 0)
    assert len(rec1) > nch / 3                                               # 7. the move rate of this system
    assert len(rec1) <= 2 * nch
    for wd in (1, 2):        # a send buffer one record short: SQMC_ERR_SPAWN_OVERFLOW and not a word written; one that just fits: the same records
        assert int(r["short_code%d" % wd]) == ERR_SPAWN_OVERFLOW and bool(r["short_untouched%d" % wd])
        assert np.array_equal(r["counts_again%d" % wd], r["counts%d" % wd]) and np.array_equal(r["rec_again%d" % wd], r["rec%d" % wd])
        assert bool(r["tail_untouched%d" % wd])


def test_two_rank_heatbath_walk_over_gloo(two_rank_gloo, single_hb):
    """Two ranks, caller-driven exchanges: deterministic (two runs are the same bits), every rank sees the same sums, every walker
    sits on its owner, no determinant is on two ranks, nwalk and sum |w| add up, the deterministic space is complete.

    Energy: outs[10:, 3].sum() / outs[10:, 2].sum() against the same quantity of the single-GPU heat-bath walk (another random
    stream: the ranks draw with their own seeds).  The bound is four times the spread (sample standard deviation) of that
    quantity over seeds of the single-GPU walk, measured by tools/heatbath_sharded_energy.py and kept, with the per-seed
    values, in profiles/heatbath_sharded.json ("energy")."""
    runs = two_rank_gloo
    assert all(int(r["status"][0]) == 0 for r in runs[0])
    _invariants(runs[0])
    _same_run(runs[0], runs[1])
    with open(PROFILE) as f:
        prof = json.load(f)["energy"]
    assert len(prof["single_gpu_seeds"]) >= 5 and prof["bound"] == 4.0 * prof["spread"]
    e2, e1 = _energy(runs[0][0]["outs"]), _energy(single_hb["outs"])
    print("energy two ranks %.6f single GPU %.6f difference %.6f bound %.6f" % (e2, e1, e2 - e1, prof["bound"]))
    assert abs(e2 - e1) <= prof["bound"]


def test_two_rank_heatbath_walk_over_the_transport_double(tmp_path):
    """attach_rccl(), steps through sqmc_gpu_shard_step and then the pipelined sqmc_gpu_shard_run (the target is passed early, so
    heads are launched from the device-side walker count): the same invariants, and two runs are the same bits."""
    runs = [_run_inlib(2, tmp_path / ("run%d" % k), 29821 + k, w_target=4000, nsteps=60) for k in range(2)]
    assert all(int(r["reached"][0]) == 2 for r in runs[0])
    _invariants(runs[0])
    _same_run(runs[0], runs[1])


def test_in_library_heatbath_equals_caller_driven_at_tiny_population(tmp_path):
    """The two drivers of the sharded step walk the same heat-bath trajectory on two ranks at a handful of walkers (steps with one
    child, or none, on a rank occur), bit for bit: both run the same kernels on the same local lists, and with two ranks every
    all-reduce adds two addends, which no order of addition can change -- so the reduced sums, the population control that
    follows them and every weight must be the same bits under both drivers (the three-rank model of this test,
    test_in_library_exchange_equals_host_driven_at_tiny_population, allows round-off because three addends can be added in two orders)."""
    kw = dict(w_begin=1.5, w_target=3, nsteps=80)
    a = _run_inlib(2, tmp_path / "inlib", 29831, **kw)
    b = _run_gloo(2, tmp_path / "host", 29832, **kw)
    few = 0
    for rank, (ra, rb) in enumerate(zip(a, b)):
        d = np.abs(ra["outs"] - rb["outs"])
        print("rank %d: largest difference of the sums, by column: %s; of the weights: %g" % (
            rank, d.max(axis=0).tolist(), float(np.abs(ra["wt"] - rb["wt"]).max()) if len(ra["wt"]) == len(rb["wt"]) else float("nan")))
    for ra, rb in zip(a, b):
        assert np.array_equal(ra["outs"], rb["outs"])
        for k in ("up", "dn", "wt", "imp_distance", "initiator"):
            assert np.array_equal(ra[k], rb[k]), k
        few += int((ra["outs"][:, 15] <= 1).sum())
    assert few > 0                           # the case under test really occurred


def test_capacity_counts_two_slots_per_child(tmp_path, one_rank):
    """MWALK between n0 + nch and n0 + 2 * nch of a step (counts read from the one-rank walk with ample room: with one rank out[5] of
    the step before is n0, out[15] is nch): ShardedWalk.step() must stop AT that step with 'nwalk>MWALK', without a fault, and leave
    the walker list whole -- as many walkers as the step found, sorted, unique.  A check that counted one slot per child would let
    the step through, and k_spawn -- which checks two slots -- would have written nothing for it to pack.
    (The send-buffer half of the capacity rule, one record short, is checked where the record count is known exactly:
    test_pack_routes_every_slot.)"""
    outs = one_rank["outs"]
    n0 = np.concatenate(([0], outs[:-1, 5])).astype(np.int64); nch = outs[:, 15].astype(np.int64)
    k = 30
    mwalk = int(n0[k] + nch[k] + nch[k] // 2)
    first = int(np.argmax(n0[1:] + 2 * nch[1:] > mwalk)) + 1        # the first step the two-slot rule refuses (step 0 starts from the initial list: far smaller)
    assert n0[first] + 2 * nch[first] > mwalk >= n0[first] + nch[first] and first >= 5
    old = os.environ.get("SQMC_SHARD_BUCKET"); os.environ["SQMC_SHARD_BUCKET"] = "0"
    try:
        res = _run_gloo(1, tmp_path / "small", 29841, mwalk=mwalk)[0]
    finally:
        if old is None: del os.environ["SQMC_SHARD_BUCKET"]
        else: os.environ["SQMC_SHARD_BUCKET"] = old
    assert int(res["status"][0]) == ERR_MWALK and "nwalk>MWALK" in str(res["msg"][0])
    assert len(res["outs"]) == first
    assert np.array_equal(res["outs"], outs[:first])                         # the steps before it are the ample walk's
    assert len(res["up"]) == n0[first] and np.all(res["owner"] == 0)         # the list the refused step found
    k_ = [(int(a), int(b)) for a, b in zip(res["up"], res["dn"])]
    assert k_ == sorted(set(k_)) and np.all(np.isfinite(res["wt"]))


def test_refusals(tmp_path):
    """heat-bath tables and sqmc_gpu_set_hf_to_psit_shard refuse each other in either order; ShardedWalk refuses heat-bath with
    hf_to_psit, and the 8-electron C2 system with the reference's 'may be biased' message."""
    import torch.multiprocessing as mp
    _join([mp.get_context("spawn").Process(target=_refusal_worker, args=(str(tmp_path),))], "refusal worker")
    with open(os.path.join(str(tmp_path), "refusals.json")) as f:
        got = json.load(f)
    for key in ("tables_first", "psit_first"):
        assert got[key][0] == ERR_UNSUPPORTED and "fast_heatbath" in got[key][1], (key, got[key])
    assert got["walk_psit"][0] == -1 and "hf_to_psit" in got["walk_psit"][1]
    assert got["walk_8e"] == [-1, "Heatbath may be biased for this system!"]
