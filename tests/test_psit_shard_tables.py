"""CPU checks of host.psit_shard_tables: one rank's share of the hf_to_psit tables (do_walk.f90:1808-1886) on the C2 set-up, with
synthetic owner arrays.  The shares of all ranks must partition the global tables and map back onto them."""
import numpy as np
import pytest

from sqmc_amd.host import psit_shard_tables


@pytest.fixture(scope="module")
def c2_psit_cpu(oracle, c2_walk):
    s = oracle.setup_walk(c2_walk, 100, 1000, 0.1, rediagonalize=True)
    return s, oracle.psit_setup(c2_walk, s)


def _owners(n, world, kind):
    rng = np.random.default_rng(7 + world)
    if kind == "random":
        return rng.integers(0, world, n)
    if kind == "first_elsewhere":          # the first state owned by the last rank
        o = rng.integers(0, world, n); o[0] = world - 1
        return o
    if kind == "no_psit_on_0":             # rank 0 holds C(T) determinants but no Psi_T determinant
        return None
    raise ValueError(kind)


def _split(s, q, owner, world, w=100.0):
    return [psit_shard_tables(s, q.loc_psit + 1, q.cdet, q.diag_elems, q.in_imp, owner, r, w) for r in range(world)]


@pytest.mark.parametrize("world,kind", [(1, "random"), (2, "random"), (3, "random"), (3, "first_elsewhere"), (2, "no_psit_on_0")])
def test_shares_partition_the_global_tables(c2_psit_cpu, world, kind):
    s, q = c2_psit_cpu
    n_ct, n_psit = len(s.ct_up), len(q.cdet)
    owner = _owners(n_ct, world, kind)
    if owner is None:
        owner = np.zeros(n_ct, np.int64)
        owner[q.loc_psit] = 1
    tb = _split(s, q, owner, world)
    # C(T): every position exactly once, each share in C(T) order
    allct = np.concatenate([t["ct_index"] for t in tb])
    assert sorted(allct.tolist()) == list(range(1, n_ct + 1))
    for r, t in enumerate(tb):
        assert np.all(np.diff(t["ct_index"]) > 0)
        assert np.all(owner[t["ct_index"] - 1] == r)
        np.testing.assert_array_equal(t["diag"], q.diag_elems[t["ct_index"] - 1])
    # Psi_T: the masks partition 1..n_psit, and slot -> C(T) position -> the global location of that Psi_T entry
    allm = np.concatenate([t["psit_mask"] for t in tb])
    assert sorted(allm.tolist()) == list(range(1, n_psit + 1))
    for t in tb:
        assert len(t["psit_slot"]) == len(t["psit_mask"])
        assert np.all(np.diff(t["psit_slot"]) > 0) and np.all(np.diff(t["psit_mask"]) > 0)
        np.testing.assert_array_equal(t["ct_index"][t["psit_slot"] - 1] - 1, q.loc_psit[t["psit_mask"] - 1])
    # the first state: on exactly one rank, at slot 1 of its share, Psi_T entry 1 there
    firsts = [r for r, t in enumerate(tb) if t["own_first"]]
    assert firsts == [int(owner[0])]
    t0 = tb[firsts[0]]
    assert t0["ct_index"][0] == 1 and t0["psit_mask"][0] == 1 and t0["psit_slot"][0] == 1
    if kind == "first_elsewhere":
        assert firsts == [world - 1] and world > 1
    if kind == "no_psit_on_0":
        assert len(tb[0]["psit_mask"]) == 0 and len(tb[0]["ct_index"]) > 0
    # deterministic space: global rows partition 0..n_imp-1, each in the share's order
    n_imp = int(np.sum(q.in_imp))
    rows = np.concatenate([t["imp_rows"] for t in tb])
    assert sorted(rows.tolist()) == list(range(n_imp))
    for t in tb:
        assert np.all(np.diff(t["imp_rows"]) > 0)


@pytest.mark.parametrize("world", [1, 2, 3])
def test_initial_weight_only_on_the_first_owner(oracle, c2_psit_cpu, world):
    s, q = c2_psit_cpu
    owner = _owners(len(s.ct_up), world, "first_elsewhere")
    tb = _split(s, q, owner, world, w=250.0)
    ref = oracle.initial_walkers_psit(s, q, 250.0)
    for r, t in enumerate(tb):
        wk = t["walkers"]
        np.testing.assert_array_equal(wk["up"], s.ct_up[t["ct_index"] - 1])
        np.testing.assert_array_equal(wk["dn"], s.ct_dn[t["ct_index"] - 1])
        np.testing.assert_array_equal(wk["imp_distance"] == 0, q.in_imp[t["ct_index"] - 1])
        nz = np.flatnonzero(wk["wt"])
        if t["own_first"]:
            assert nz.tolist() == [0] and wk["wt"][0] == ref["wt"][0]
            assert wk["initiator"][0] == ref["initiator"][0]
        else:
            assert len(nz) == 0 and not np.any(wk["initiator"] == 3)
