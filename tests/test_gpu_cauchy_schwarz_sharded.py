"""proposal_method CauchySchwarz on the sharded walk: one rank equals the single-GPU CS walk bit for bit (radix tail, as
test_one_rank_sharded_equals_single_rank_step does for uniform2), and two ranks over gloo and over the tests/fake_rccl transport
double are deterministic and keep the ownership invariants.  The workers are the sharded suite's, with proposal= passed through."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.test_gpu_sharded import (FCIDUMP, NSTEPS, SEED, W_BEGIN, W_TARGET, _fake_rccl_lib, _inlib_multi_worker,  # noqa: E402
                                    _run)

CS = {"proposal": "cauchyschwarz"}


def _single_cs_worker(outdir):
    os.environ["SQMC_BUCKET"] = "0"                # the radix tail, the one the sharded step runs (read once per process)
    sys.path.insert(0, ROOT)
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    hst = H.ChemHost(FCIDUMP, 8, 4, "d2h")
    ref = H.GpuWalk(hst, W_TARGET, w_begin=W_BEGIN, seed=SEED, mwalk=400000, proposal="cauchyschwarz")
    outs = np.array([ref.step().copy() for _ in range(NSTEPS)])
    wk = ref.g.download_walkers()
    np.savez(os.path.join(outdir, "single_cs.npz"), outs=outs, tail=np.array(ref.g.tail_stats()), **wk)
    ref.close()


def _invariants(res):
    for r in res[1:]:
        assert np.array_equal(r["outs"][:, :7], res[0]["outs"][:, :7])      # every rank saw the same all-reduced sums
    keys, n_imp = [], 0
    for rank, r in enumerate(res):
        assert np.all(r["owner"] == rank)
        k = [(int(a), int(b)) for a, b in zip(r["up"], r["dn"])]
        assert k == sorted(set(k))
        keys += k
        n_imp += int((r["imp_distance"] == 0).sum())
    assert len(keys) == len(set(keys))
    assert n_imp == int(res[0]["n_imp_global"])
    out = res[0]["outs"][-1]
    assert int(out[5]) == len(keys)
    assert np.isclose(sum(float(np.abs(r["wt"]).sum()) for r in res), out[1], rtol=1e-12)
    e = res[0]["outs"][10:, 3].sum() / res[0]["outs"][10:, 2].sum()
    assert -75.80 < e < -75.55


@pytest.mark.gpu
def test_one_rank_sharded_cs_equals_single_rank_cs(tmp_path, monkeypatch):
    monkeypatch.setenv("SQMC_SHARD_BUCKET", "0")
    import torch.multiprocessing as mp
    res = _run(1, tmp_path, 29741, walk_kw=CS)[0]
    pr = mp.get_context("spawn").Process(target=_single_cs_worker, args=(str(tmp_path),))
    pr.start(); pr.join(600)
    assert pr.exitcode == 0
    wk = np.load(os.path.join(str(tmp_path), "single_cs.npz"))
    assert tuple(wk["tail"]) == (0, 0)
    assert np.array_equal(res["up"], wk["up"]) and np.array_equal(res["dn"], wk["dn"])
    assert np.array_equal(res["wt"], wk["wt"]) and np.array_equal(res["initiator"], wk["initiator"])
    assert np.allclose(res["outs"], wk["outs"], rtol=1e-12, atol=1e-12)


@pytest.mark.gpu
def test_two_rank_cs_walk_over_gloo(tmp_path):
    runs = []
    for k in range(2):
        d = tmp_path / ("run%d" % k); d.mkdir()
        runs.append(_run(2, d, 29751 + k, walk_kw=CS))
    _invariants(runs[0])
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a["outs"], b["outs"])
        assert np.array_equal(a["up"], b["up"]) and np.array_equal(a["dn"], b["dn"]) and np.array_equal(a["wt"], b["wt"])


@pytest.mark.gpu
def test_two_rank_cs_walk_over_the_transport_double(tmp_path):
    import torch.multiprocessing as mp
    fake = _fake_rccl_lib()
    ctx = mp.get_context("spawn")
    runs = []
    for k in range(2):
        out = os.path.join(str(tmp_path), "run%d" % k); os.makedirs(out)
        ps = [ctx.Process(target=_inlib_multi_worker, args=(r, 2, 29761 + k, out, fake, 4000, 60), kwargs=dict(walk_kw=CS)) for r in range(2)]
        for p in ps: p.start()
        for p in ps: p.join(300)
        alive = [p for p in ps if p.is_alive()]
        for p in alive: p.terminate()
        assert not alive, "in-library exchange did not finish"
        assert all(p.exitcode == 0 for p in ps), [p.exitcode for p in ps]
        runs.append([np.load(os.path.join(out, "rank%d.npz" % r)) for r in range(2)])
    res = runs[0]
    assert np.array_equal(res[1]["outs"][:, :7], res[0]["outs"][:, :7])
    keys = []
    for rank, r in enumerate(res):
        assert np.all(r["owner"] == rank)
        k = [(int(a), int(b)) for a, b in zip(r["up"], r["dn"])]
        assert k == sorted(set(k))
        keys += k
    assert len(keys) == len(set(keys)) and int(res[0]["outs"][-1][5]) == len(keys)
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a["outs"], b["outs"])
        assert np.array_equal(a["up"], b["up"]) and np.array_equal(a["dn"], b["dn"]) and np.array_equal(a["wt"], b["wt"])
