"""hubbardk with space_sym on the GPU against tests/hubbardk_sym_checker.py (4x4, t = 1, U = 4 unless said): the images door, the
symmetrised elements, one RNG_REPLAY step against the serial stream, the proposal door, the connection generator and sym_sparse_ham, a walk with nothing stochastic in it in each
of the four (z, p) sectors, a stochastic walk, two ranks, the deck runner, the refusals, and the dispatch with the flag off.
The walks target the lowest eigenvalue of the checker's M = V^T A V, never the plain ground state (which is in none of the sectors)."""
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import proposal_checker as PC          # noqa: E402
from tests import hubbardk_checker as HK          # noqa: E402
from tests import hubbardk_sym_checker as HS      # noqa: E402

pytestmark = pytest.mark.gpu
T_HOP, U, TAU = 1.0, 4.0, 0.01
SEED = (1346, 5634, 6635, 4361)
SECTORS = [(1, 1), (1, -1), (-1, 1), (-1, -1)]
START = (17, 3)                                    # 2 up 2 dn at total momentum 0 (the first orbitals have momentum (-4, 0))
DECK = os.path.join(ROOT, "tests", "golden", "hubbardk4x4_sym_i_walk")
UNSUPPORTED, BAD_ARG = -3, -1                      # SQMC_ERR_UNSUPPORTED, SQMC_ERR_BAD_ARG of include/sqmc_gpu.h
E0_11 = -10.910328101765
PLAIN_E0 = -11.530292402630


def _host(z, p, nup=2, ndn=2, l=4, start=START):
    import sqmc_amd
    from sqmc_amd.host import HubbardKHost
    sqmc_amd.set_device(0)
    return HubbardKHost(l, l, nup, ndn, T_HOP, U, space_sym=True, z=z, p=p, start=start)


@pytest.fixture(scope="module")
def model():
    """the checker's plain sector and its four symmetry sectors, computed once"""
    H = HK.HubbardKH(4, 4, T_HOP, U)
    dets = HK.sector(H, 2, 2, (0, 0))
    A = HK.dense(H, dets, lambda u, d: HK.excitations_hubbardk(H, u, d))
    return H, dets, {zp: HS.Sector(H, 2, 2, zp[0], zp[1], dets, A) for zp in SECTORS}


def _ctx(H, nup, ndn, z, p, **kw):
    """a context with the maps of the CHECKER (not the host's): the library's entry is tested on its own"""
    import sqmc_amd
    from sqmc_amd._lib import GpuChem
    sqmc_amd.set_device(0)
    kv = np.array(H.k, np.int32)
    g = GpuChem.hubbardk(H.l_x, H.l_y, nup, ndn, T_HOP, U, kv, np.array(H.eps), **kw)
    c4, rf = HS.Group(H, nup, ndn, z, p).maps_one_based()
    g.set_hubbardk_space_sym(z, p, c4, rf)
    return g


# ------------------------------------------------------------------------------------------------ 1. the images door
@pytest.mark.parametrize("z,p", SECTORS)
def test_images_door_all_912_determinants(model, z, p):
    H, dets, S = model
    G = S[(z, p)].G
    g = _ctx(H, 2, 2, z, p)
    try:
        o = g.hubbardk_sym_images([d[0] for d in dets], [d[1] for d in dets])
    finally:
        g.close()
    n_null = 0
    for i, d in enumerate(dets):
        imgs, phases, rep, pw, norm, nd = G.reduce(d)
        assert list(zip(o["images_up"][i].tolist(), o["images_dn"][i].tolist())) == imgs, d
        assert o["phases"][i].tolist() == phases, d
        assert (int(o["rep_up"][i]), int(o["rep_dn"][i])) == rep and int(o["phase_w_rep"][i]) == pw and int(o["num_distinct"][i]) == nd, d
        assert abs(float(o["norm"][i]) - norm) <= math.ulp(norm), d
        n_null += nd == 0
    assert (n_null > 0) == (len(S[(z, p)].live) < 102)


def test_images_door_8x8_across_the_word():
    """3 up 3 dn on 8x8, 200 seeded momentum-0 determinants that hold orbitals 1 and 64 (bits 0 and 63): the maps move bits across the whole word"""
    H = HK.HubbardKH(8, 8, T_HOP, U)
    rng = random.Random(11)
    dets = []
    while len(dets) < 200:
        up = 1 | (1 << 63) | (1 << rng.randrange(1, 63))
        a, b = rng.sample(range(64), 2)
        k = [sum(H.k[o][c] for o in PC._bits(up) + [a, b]) for c in (0, 1)]
        s = H.index[H.fold((-k[0], -k[1]))]
        if s in (a, b):
            continue
        d = (up, (1 << a) | (1 << b) | (1 << s))
        if PC._pop(up) == 3 and H.momentum(*d) == (0, 0) and d not in dets:
            dets.append(d)
    assert any(d[1] >> 63 & 1 for d in dets) and any(d[1] & 1 for d in dets)
    for z, p in ((1, 1), (-1, -1)):
        G = HS.Group(H, 3, 3, z, p)
        g = _ctx(H, 3, 3, z, p)
        try:
            o = g.hubbardk_sym_images([d[0] for d in dets], [d[1] for d in dets])
        finally:
            g.close()
        for i, d in enumerate(dets):
            imgs, phases, rep, pw, norm, nd = G.reduce(d)
            assert list(zip(o["images_up"][i].tolist(), o["images_dn"][i].tolist())) == imgs, d
            assert o["phases"][i].tolist() == phases and (int(o["rep_up"][i]), int(o["rep_dn"][i])) == rep, d
            assert int(o["phase_w_rep"][i]) == pw and int(o["num_distinct"][i]) == nd and abs(float(o["norm"][i]) - norm) <= math.ulp(norm), d


# ------------------------------------------------------------------------------------------------ 2. elements
@pytest.mark.parametrize("z,p", SECTORS)
def test_hamiltonian_batch_is_the_symmetrised_matrix(model, z, p):
    """all pairs of live representatives against M, |diff| <= 1e-12 (values O(10), at most 64 roundings of 2.2e-16 x 10 = 1.4e-13);
    a bra that is not a representative gives its representative's element; a pair with a null member gives exactly 0"""
    H, dets, S = model
    S = S[(z, p)]
    live = S.live
    pairs = [a + b for a in live for b in live]
    rng = random.Random(5)
    others = [d for d in dets if S.rep_of[d] != d and S.is_live(d)]
    extra = [rng.choice(others) + rng.choice(live) for _ in range(300)]
    null = [d for d in dets if not S.is_live(d)]
    nulls = [rng.choice(null) + rng.choice(live) for _ in range(100)] + [rng.choice(live) + rng.choice(null) for _ in range(100)] if null else []
    a = np.array(pairs + extra + nulls, np.uint64)
    g = _ctx(H, 2, 2, z, p)
    try:
        got = g.hamiltonian_batch(a[:, 0], a[:, 1], a[:, 2], a[:, 3])
    finally:
        g.close()
    n = len(live)
    worst = float(np.max(np.abs(got[:n * n].reshape(n, n) - S.M)))
    print("(z, p) = (%d, %d): %d live representatives, worst |H - M| = %.3g" % (z, p, n, worst))
    assert worst <= 1e-12
    for q, x in zip(extra, got[n * n:n * n + len(extra)]):
        assert abs(x - S.element(q[:2], q[2:])) <= 1e-12, q
    assert np.all(got[n * n + len(extra):] == 0.0)
    assert len(nulls) > 0 or (z, p) == (1, 1) and len(live) == 91


# ------------------------------------------------------------------------------------------------ 3. one RNG_REPLAY step
LCG_MULT, MASK48 = 11 ** 13 % (1 << 48), (1 << 48) - 1


def test_replay_step_matches_the_serial_stream(model):
    """One RNG_REPLAY step (k_replay_prepass, k_spawn, k_diag, the merge) from 40 seeded representatives with weights 0.5 .. 7.3 of both
    signs, against the single rannyu stream walked here: walker by walker in list order, max(nint|w|, 1) children of weight w / n each,
    three random_int draws per child (up electron, dn electron, empty up orbital -- the plain move's, blocked or not), the triple they
    pick put through the checker's move.  No weight lies below always_spawn_cutoff_wt and min_wt = 0, so nothing else draws.
    The device's list after the step must be the merge of the parents times 1 + tau (E_T - M_ii) and of the children: the same
    determinants (every one a live representative; a child without weight in the model leaves none), weights to 1e-12 of the sum
    of the absolute terms, the stream at the same state (every child took three draws), the same number of children.  H_ii: the
    parents' after the step, and after a second step that of every determinant the first one created, equal diag(M) to 1e-12."""
    import sqmc_amd
    H, dets, S = model
    S = S[(1, 1)]
    rng = random.Random(31)
    parents = sorted(rng.sample(S.live, 40))
    wt = np.linspace(0.5, 7.3, 40)
    wt[1::3] *= -1.0
    perm = list(range(40)); rng.shuffle(perm)
    wt = wt[perm]
    tau = TAU
    hst = _host(1, 1)
    g = hst.gpu(rng_mode=sqmc_amd.RNG_REPLAY, seed=SEED, mwalk=100000)
    try:
        s = hst.setup_walk(g, 20, 30, 0.5)
        g.set_ct_table(s.ct_up, s.ct_dn, s.ct_num, s.ct_den)
        e_trial = s.e_trial0
        n = len(parents)
        g.upload_walkers(dict(up=np.array([d[0] for d in parents], np.uint64), dn=np.array([d[1] for d in parents], np.uint64), wt=wt.copy(),
                              imp_distance=np.ones(n, np.int8), initiator=np.full(n, 2, np.int8), perm_sign=np.zeros(n, np.int8),
                              matrix_elements=np.full(n, 1e51), e_num=np.full(n, 1e51), e_den=np.full(n, 1e51)))
        limbs = g.rng_state()
        x = ((limbs[0] << 36) + (limbs[1] << 24) + (limbs[2] << 12) + limbs[3]) & MASK48
        prm = dict(tau=tau, e_trial=e_trial, reweight_factor_inv=1.0, r_initiator=0.0, min_wt=0.0, always_spawn_cutoff_wt=0.5, initiator_power=0,
                   initiator_min_distance=0, c_t_initiator=0, semistochastic=0, reached_w_abs_gen=0)
        out = g.step(prm)
        after = g.rng_state()
        wk = g.download_walkers()
        g.step(prm)
        wk2 = g.download_walkers()
    finally:
        g.close()

    def rint(k):
        nonlocal x
        x = (x * LCG_MULT) & MASK48
        return int(k * (x * 2.0 ** -48)) + 1

    acc, sab, nch, n_zero, n_empty = {}, {}, 0, 0, H.norb - 2
    for par, w in zip(parents, wt.tolist()):
        f = 1.0 + tau * (e_trial - S.element(par, par))
        acc[par] = acc.get(par, 0.0) + w * f
        sab[par] = sab.get(par, 0.0) + abs(w * f)
        tr = HK.triples_hubbardk(H, *par)
        nc = max(int(math.floor(abs(w) + 0.5)), 1)
        for _ in range(nc):
            a, b, c = rint(2), rint(2), rint(n_empty)
            t = tr[((a - 1) * 2 + (b - 1)) * n_empty + (c - 1)]
            assert (t[0], t[1], t[2]) == (PC._bits(par[0])[a - 1], PC._bits(par[1])[b - 1], [o for o in range(H.norb) if not par[0] >> o & 1][c - 1])
            j, wm = S.move(par, t[4], tau)
            nch += 1
            if wm == 0.0:
                n_zero += 1
                continue
            assert j in S.pos and j != par
            acc[j] = acc.get(j, 0.0) + (w / nc) * wm
            sab[j] = sab.get(j, 0.0) + abs((w / nc) * wm)
    assert int(out[15]) == nch
    assert after == [(x >> 36) & 4095, (x >> 24) & 4095, (x >> 12) & 4095, x & 4095]          # every child, blocked or not, took three draws
    got = {(int(a), int(b)): float(v) for a, b, v in zip(wk["up"], wk["dn"], wk["wt"])}
    assert all(k in S.pos for k in got)                        # every determinant of the list is a live representative
    assert set(got) == set(acc), (sorted(set(got) - set(acc))[:5], sorted(set(acc) - set(got))[:5])
    worst = max(abs(got[k] - acc[k]) / sab[k] for k in acc)
    new = [k for k in acc if k not in set(parents)]
    print("replay step: %d children of 40 parents, %d without weight, %d new determinants, worst |dw| / sum|terms| = %.3g" % (nch, n_zero, len(new), worst))
    assert worst <= 1e-12 and n_zero > 10 and len(new) > 10
    me1 = {(int(a), int(b)): float(v) for a, b, v in zip(wk["up"], wk["dn"], wk["matrix_elements"])}
    for k in parents:
        assert abs(me1[k] - S.element(k, k)) <= 1e-12, k
    me2 = {(int(a), int(b)): float(v) for a, b, v in zip(wk2["up"], wk2["dn"], wk2["matrix_elements"])}
    seen_new = [k for k in new if k in me2]
    assert len(seen_new) > 10
    for k in seen_new:
        assert abs(me2[k] - S.element(k, k)) <= 1e-12, (k, me2[k])


# ------------------------------------------------------------------------------------------------ 4. the proposal door
N_DOOR = 20000


def _door_parents(S):
    start = S.rep_of[START]                        # the start determinant's representative, (3, 17)
    full = next(r for r in S.live if S.G.reduce(r)[5] == 16 and r != start)
    part = next(r for r in S.live if 0 < S.G.reduce(r)[5] < 16 and r != start)
    return [("start", start), ("num_distinct_16", full), ("num_distinct_lt_16", part)]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_proposal_door_is_unbiased(model, which):
    """20,000 COUNTER proposals: per child representative the mean weight (zero-weight proposals included) is within 5 standard
    errors of -tau M[:, i]; no child is a null state or the parent; every child is a representative"""
    H, dets, S = model
    S = S[(1, 1)]
    name, par = _door_parents(S)[which]
    assert S.rep_of[par] == par and S.is_live(par)
    st = PC.splitmix_states(N_DOOR)
    g = _ctx(H, 2, 2, 1, 1)
    try:
        ju, jd, w, _ = g.propose_batch(TAU, np.full(N_DOOR, par[0], np.uint64), np.full(N_DOOR, par[1], np.uint64), PC.state_limbs(st))
    finally:
        g.close()
    keys, cnt, sw, sw2, _, _ = PC.tally(ju, jd, w)
    seen = dict(zip(keys, zip(cnt, sw, sw2)))
    want = {j: -TAU * S.element(j, par) for j in S.live if j != par}
    for k in keys:
        assert k != par and k in S.pos, (name, k)
    worst = 0.0
    for j, x in want.items():
        c, s1, s2 = seen.get(j, (0.0, 0.0, 0.0))
        mean = s1 / N_DOOR
        var = max(s2 / N_DOOR - mean * mean, 0.0)
        se = math.sqrt(var / N_DOOR)
        if x == 0.0:
            assert c == 0, (name, j)
            continue
        assert c > 0, (name, j, x)
        assert abs(mean - x) <= 5.0 * se, (name, j, mean, x, se)
        worst = max(worst, abs(mean - x) / se)
    print("proposal door %s %s: %d children, worst deviation %.2f standard errors" % (name, par, len(keys), worst))
    assert len(keys) > 5


# ------------------------------------------------------------------------------------------------ 5. the generator
@pytest.mark.parametrize("diag_mode", [0, 1, 2])
def test_connections_sum_to_the_symmetrised_matrix(model, diag_mode):
    H, dets, S = model
    S = S[(1, 1)]
    rng = random.Random(23)
    refs = sorted(rng.sample(S.live, 12))
    coeffs = [rng.choice((-1, 1)) * rng.uniform(0.1, 1.0) for _ in refs]
    coeffs[4] = 0.0
    want = S.connections(refs, coeffs, 1 if diag_mode == 1 else 0)
    g = _ctx(H, 2, 2, 1, 1)
    try:
        cu, cd, num, den = g.hci_connections([r[0] for r in refs], [r[1] for r in refs], coeffs, 1e-300, diag_mode=diag_mode)
    finally:
        g.close()
    keys = list(zip(cu.tolist(), cd.tolist()))
    assert all(k in S.pos for k in keys)                       # every determinant returned is a live representative
    if diag_mode == 2:                                         # raw: the unmerged terms, e_mix_den = the source's index; summed here
        got = {}
        for k, x, i in zip(keys, num.tolist(), den.tolist()):
            assert coeffs[int(i)] != 0.0
            got[k] = got.get(k, 0.0) + x
    else:
        assert keys == sorted(set(keys))
        got = dict(zip(keys, num.tolist()))
        own = dict(zip(refs, coeffs))
        assert all(d == own.get(k, 0.0) for k, d in zip(keys, den.tolist()))
    assert set(got) == set(want)
    worst = max(abs(got[k] - want[k]) for k in want)
    print("diag_mode %d: %d connections of 12 representatives, worst |d| = %.3g" % (diag_mode, len(want), worst))
    assert worst <= 1e-12


def test_sym_sparse_ham_is_m(model):
    H, dets, S = model
    S = S[(1, 1)]
    hst = _host(1, 1)
    g = hst.gpu()
    try:
        cnt, idx, val = hst.sym_sparse_ham([r[0] for r in S.live], [r[1] for r in S.live], g)
    finally:
        g.close()
    n = len(S.live)
    X = np.zeros((n, n))
    rows = np.repeat(np.arange(n), cnt)
    assert np.all(idx - 1 <= rows) and len(set(zip(rows.tolist(), idx.tolist()))) == len(idx)
    X[rows, idx - 1] = val
    X[idx - 1, rows] = val
    assert np.max(np.abs(X - S.M)) <= 1e-12
    assert all(v != 0.0 for r, c, v in zip(rows.tolist(), (idx - 1).tolist(), val.tolist()) if r != c)


# ------------------------------------------------------------------------------------------------ 6. a deterministic walk
class _Levels:
    def __init__(self, hst, n_levels):
        self._h, self._n = hst, n_levels

    def __getattr__(self, name):
        return getattr(self._h, name)

    def setup_walk(self, g, n_truncate_trial_wf, size_deterministic, tau_multiplier):
        return self._h.setup_walk(g, n_truncate_trial_wf, size_deterministic, tau_multiplier, n_levels=self._n)


@pytest.mark.parametrize("z,p", SECTORS)
def test_walk_with_nothing_stochastic_finds_the_sector_ground_state(model, z, p):
    """every live representative is in the deterministic space: power iteration, converging to the sector's lowest eigenvalue of M (step
    count and tolerance of the plain test).  The start is 17 / 3 where it has a state in the sector, which is (1, 1) only: its orbit vector
    vanishes in the other three, where the host must refuse it and the walk starts from the representative with the largest component in
    the checker's lowest eigenvector."""
    from sqmc_amd import host as Hh
    H, dets, S = model
    S = S[(z, p)]
    wm, X = np.linalg.eigh(S.M)
    e0 = float(wm[0])
    assert S.is_live(START) == ((z, p) == (1, 1))
    if S.is_live(START):
        hst = _host(z, p)
        assert (hst.hf_up, hst.hf_dn) == S.rep_of[START]
    else:
        with pytest.raises(ValueError):
            _host(z, p)
        hst = _host(z, p, start=S.live[int(np.argmax(np.abs(X[:, 0])))])
    w = Hh.GpuWalk(_Levels(hst, 8), 1.0e4, w_begin=1.0e4, n_truncate_trial_wf=20, size_deterministic=10 * len(S.live), tau_multiplier=0.5, seed=SEED)
    try:
        assert sorted(zip(w.setup.imp_up.tolist(), w.setup.imp_dn.tolist())) == S.live
        prev, steps, e = None, 0, 0.0
        while steps < 8000:
            out = w.step(); steps += 1
            e = out[3] / out[2]
            if prev is not None and abs(e - prev) < 1e-13:
                break
            prev = e
    finally:
        w.close()
    print("(z, p) = (%d, %d): %d representatives, E0 = %.12f, walk %.12f after %d steps" % (z, p, len(S.live), e0, e, steps))
    assert steps < 8000
    assert abs(e - e0) <= 1e-10
    if (z, p) == (1, 1):
        assert abs(e - PLAIN_E0) > 0.5 and abs(e0 - E0_11) < 1e-9


# ------------------------------------------------------------------------------------------------ 7. a stochastic walk
def test_stochastic_walk_stays_among_representatives(model):
    from sqmc_amd import host as Hh
    H, dets, S = model
    S = S[(1, 1)]
    hst = _host(1, 1)
    w = Hh.GpuWalk(hst, 5.0e3, w_begin=1000.0, n_truncate_trial_wf=20, size_deterministic=10, tau_multiplier=0.5, seed=SEED)
    try:
        for _ in range(300):
            w.step()
        outs, nb = [], 30
        for b in range(nb):
            outs += [w.step().copy() for _ in range(100)]
            wk = w.g.download_walkers()
            keys = list(zip(wk["up"].tolist(), wk["dn"].tolist()))
            assert all(k in S.pos for k in keys), b                # every walker is a live representative
    finally:
        w.close()
    outs = np.array(outs)
    assert keys == sorted(set(keys))
    assert int(outs[-1][5]) == len(keys)
    assert np.isclose(float(np.abs(wk["wt"]).sum()), outs[-1][1], rtol=1e-12)
    e = outs[:, 3].sum() / outs[:, 2].sum()
    blocks = [outs[k:k + 100, 3].sum() / outs[k:k + 100, 2].sum() for k in range(0, len(outs), 100)]
    se = float(np.std(blocks, ddof=1) / math.sqrt(len(blocks)))
    print("stochastic walk (1, 1): E = %.6f, E0 = %.6f, deviation %.3g, standard error %.3g, %d walkers" % (e, E0_11, e - E0_11, se, len(keys)))
    assert abs(e - E0_11) <= 4.0 * se


# ------------------------------------------------------------------------------------------------ 8. two ranks
def _shard_worker(rank, world, port, outdir):
    import torch                                   # noqa: F401  before the HIP library (one libamdhip64 per process)
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    hst = H.HubbardKHost(4, 4, 2, 2, T_HOP, U, space_sym=True, z=1, p=1, start=START)
    w = H.ShardedWalk(hst, 5000, rank, world, w_begin=1000, seed=SEED, mwalk=100000, n_truncate_trial_wf=20, size_deterministic=10, tau_multiplier=0.5)
    for _ in range(200):
        w.step()
    outs = [w.step().copy() for _ in range(1000)]
    wk = w.g.download_walkers()
    owner = w.g.det_owner(wk["up"], wk["dn"], world)
    np.savez(os.path.join(outdir, "rank%d.npz" % rank), outs=np.array(outs), owner=owner, n_imp_global=w.n_imp_global, **wk)
    w.close()
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_walk_invariants_and_energy(model, tmp_path):
    """the invariants of test_gpu_hubbardk.test_sharded_walk_invariants with space_sym, every walker a live representative, and the
    energy of 1000 steps (blocks of 50) within 4 standard errors of the sector's lowest eigenvalue"""
    import socket
    import torch.multiprocessing as mp
    H, dets, S = model
    S = S[(1, 1)]
    ctx = mp.get_context("spawn")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ps = [ctx.Process(target=_shard_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for q in ps: q.start()
    for q in ps: q.join(600)
    assert all(q.exitcode == 0 for q in ps), [q.exitcode for q in ps]
    res = [np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in range(2)]
    assert np.array_equal(res[1]["outs"][:, :7], res[0]["outs"][:, :7])
    keys, n_imp = [], 0
    for rank, r in enumerate(res):
        assert np.all(r["owner"] == rank)
        k = [(int(a), int(b)) for a, b in zip(r["up"], r["dn"])]
        assert k == sorted(set(k)) and all(x in S.pos for x in k)
        keys += k
        n_imp += int((r["imp_distance"] == 0).sum())
    assert len(keys) == len(set(keys)) and n_imp == int(res[0]["n_imp_global"])
    outs = res[0]["outs"]
    assert int(outs[-1][5]) == len(keys)
    assert np.isclose(sum(float(np.abs(r["wt"]).sum()) for r in res), outs[-1][1], rtol=1e-12)
    assert all(len(r["up"]) > 0 for r in res)
    e = outs[:, 3].sum() / outs[:, 2].sum()
    blocks = [outs[k:k + 50, 3].sum() / outs[k:k + 50, 2].sum() for k in range(0, 1000, 50)]
    se = float(np.std(blocks, ddof=1) / math.sqrt(len(blocks)))
    print("two ranks (1, 1): E = %.6f, E0 = %.6f, standard error %.3g, %d walkers" % (e, E0_11, se, len(keys)))
    assert abs(e - E0_11) <= 4.0 * se


# ------------------------------------------------------------------------------------------------ 9. the deck
def _run_deck(path):
    return subprocess.run([sys.executable, "-m", "sqmc_amd.run", "-i", path], cwd=ROOT, capture_output=True, text=True, timeout=600)


def test_deck_runs_end_to_end():
    r = _run_deck(DECK)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "Spatial + time symmetries of hubbardk being used" in r.stdout
    assert "z(time reversal), p(reflection about y-axis)=   1   1" in r.stdout
    import re
    m = re.search(r"Energy=\s*(-?\d+\.\d+)\(\s*(\d+)\)\s*(-?\d+\.\d+)\(\s*(\d+)\)\s*(-?\d+\.\d+)\(\s*(\d+)\)", r.stdout)
    assert m, r.stdout[-1500:]
    e, se = float(m.group(5)), 1e-8 * float(m.group(6))           # the block average with its corrected error (in units of 1e-8)
    print("deck: Energy = %.8f +- %.8f, exact -7.83892719" % (e, se))
    assert abs(e - (-7.838927194942)) <= 4.0 * (se + 0.5e-8) + 0.5e-8          # (both printed figures are rounded to eight decimals)


@pytest.mark.parametrize("old,new,text", [("1 1      ", "2 1      ", "Time symmetry for hubbardk will not work when nup and ndn are not equal! Stopping the program...."),
                                          ("4 4      ", "4 3      ", "space_sym = t needs a square lattice of even side")])
def test_deck_refusals(tmp_path, old, new, text):
    lines = open(DECK).read().split("\n")
    hit = [i for i, l in enumerate(lines) if l.startswith(old) and ("nup, ndn" in l or "l_x, l_y" in l)]
    assert len(hit) == 1
    lines[hit[0]] = new + lines[hit[0]][len(old):]
    path = str(tmp_path / "deck")
    open(path, "w").write("\n".join(lines))
    r = _run_deck(path)
    assert r.returncode != 0 and text in r.stdout + r.stderr, r.stdout[-1500:] + r.stderr[-1500:]


# ------------------------------------------------------------------------------------------------ 10. refusals
def test_refusals(model):
    import sqmc_amd
    from sqmc_amd._lib import GpuChem, Pt2StochasticPlan
    H, dets, S = model
    S11, Smm = S[(1, 1)], S[(-1, -1)]
    kv, ke = np.array(H.k, np.int32), np.array(H.eps)
    c4, rf = S11.G.maps_one_based()

    def refused(call, code, name):
        with pytest.raises(sqmc_amd.SqmcGpuError) as ei:
            call()
        assert ei.value.code == code, (name, str(ei.value))

    g = _ctx(H, 2, 2, -1, -1, mwalk=1000)
    try:
        one, two = np.ones(1, np.int64), np.ones(1)
        r = Smm.live[0]
        refused(lambda: g.set_hf_to_psit(one, two, two), UNSUPPORTED, "hf_to_psit")
        refused(lambda: g.hci_set_diag_update(1), UNSUPPORTED, "diag-update mode")
        refused(lambda: Pt2StochasticPlan(g, [r[0]], [r[1]], [1.0], -1.0, 1e-9, 1e-3, 10), UNSUPPORTED, "stochastic-PT plan")
        refused(lambda: g.hci_pt2([r[0]], [r[1]], [1.0], -1.0, 1e-9), UNSUPPORTED, "hci_pt2")
        refused(lambda: g.build_sparse_ham([r[0]], [r[1]]), UNSUPPORTED, "build_sparse_ham")
        refused(lambda: sqmc_amd.SpmvPlan.from_dets(g, [r[0]], [r[1]]), UNSUPPORTED, "build_spmv_plan")
        not_rep = next(d for d in dets if Smm.rep_of[d] != d and Smm.is_live(d))
        null = next(d for d in Smm.reps if not Smm.is_live(d))
        for bad in (not_rep, null):
            wk = dict(up=np.array([bad[0]], np.uint64), dn=np.array([bad[1]], np.uint64), wt=np.ones(1), imp_distance=np.ones(1, np.int8),
                      initiator=np.full(1, 2, np.int8), perm_sign=np.zeros(1, np.int8), matrix_elements=np.full(1, 1e51), e_num=np.full(1, 1e51), e_den=np.full(1, 1e51))
            refused(lambda: g.upload_walkers(wk), BAD_ARG, "upload of %s" % (bad,))
            refused(lambda: g.set_ct_table([bad[0]], [bad[1]], [1.0], [1.0]), BAD_ARG, "C(T) with %s" % (bad,))
        wk["up"][0], wk["dn"][0] = r
        g.upload_walkers(wk)                                    # a live representative is accepted ...
        refused(lambda: g.set_hubbardk_space_sym(1, 1, c4, rf), BAD_ARG, "space_sym on a context with walkers")
    finally:
        g.close()
    g = GpuChem.hubbardk(4, 4, 2, 2, T_HOP, U, kv, ke)          # the images door on a context whose flag was never set
    try:
        refused(lambda: g.hubbardk_sym_images([3], [17]), UNSUPPORTED, "images door without space_sym")
    finally:
        g.close()
    bad_perm = [row[:] for row in c4]; bad_perm[5] = bad_perm[4][:]
    swap = [row[:] for row in c4]
    lo, hi = int(np.argmin(ke)), int(np.argmax(ke))
    for row in swap:                                            # a permutation that exchanges the lowest and the highest orbital in map 1
        row[0] = {lo + 1: hi + 1, hi + 1: lo + 1}.get(row[0], row[0])
    not_c4 = [[row[1], row[1], row[2]] for row in c4]           # map1 = map2: permutations that preserve the energies but do not compose
    cases = [(dict(c4=bad_perm), BAD_ARG), (dict(c4=swap), BAD_ARG), (dict(c4=not_c4), BAD_ARG), (dict(z=2), BAD_ARG), (dict(p=0), BAD_ARG),
             (dict(nup=3), UNSUPPORTED), (dict(l=(4, 3)), UNSUPPORTED), (dict(l=(3, 3)), UNSUPPORTED)]
    for bad, code in cases:
        l = bad.get("l", (4, 4))
        Hb = H if l == (4, 4) else HK.HubbardKH(l[0], l[1], T_HOP, U)
        n = l[0] * l[1]
        g = GpuChem.hubbardk(l[0], l[1], bad.get("nup", 2), 2, T_HOP, U, np.array(Hb.k, np.int32), np.array(Hb.eps))
        try:
            refused(lambda: g.set_hubbardk_space_sym(bad.get("z", 1), bad.get("p", 1), np.resize(np.array(bad.get("c4", c4), np.int32), (n, 3)),
                                                     np.resize(np.array(rf, np.int32), n)), code, str(bad)[:40])
        finally:
            g.close()
    from sqmc_amd.host import HubbardKHost
    with pytest.raises(ValueError):
        HubbardKHost(4, 4, 2, 2, T_HOP, U, space_sym=True)      # the first-orbitals start of 2 up 2 dn has momentum (-4, 0)
    with pytest.raises(ValueError):
        HubbardKHost(4, 4, 1, 1, T_HOP, U, space_sym=True, z=-1, p=1)      # 1 up 1 dn has no state outside (1, 1)


# ------------------------------------------------------------------------------------------------ 11. the flag off
def test_flag_off_is_bit_identical():
    """a hubbardk context whose flag was never set against a second one of the same configuration: elements and one COUNTER step"""
    import sqmc_amd
    from sqmc_amd.host import HubbardKHost
    sqmc_amd.set_device(0)
    H = HK.HubbardKH(4, 4, T_HOP, U)
    dets = random.Random(2).sample(HK.sector(H, 2, 2, (0, 0)), 200)
    a = np.array([x + y for x in dets[:40] for y in dets], np.uint64)
    res = []
    for _ in range(2):
        hst = HubbardKHost(4, 4, 2, 2, T_HOP, U, start=START)
        g = hst.gpu(rng_mode=sqmc_amd.RNG_COUNTER, mwalk=1 << 16)
        try:
            h = g.hamiltonian_batch(a[:, 0], a[:, 1], a[:, 2], a[:, 3])
            s = hst.setup_walk(g, 20, 30, 0.5)
            g.set_projector(s.prj_counts, s.prj_indices, s.prj_values)
            g.set_ct_table(s.ct_up, s.ct_dn, s.ct_num, s.ct_den)
            from sqmc_amd.host import initial_walkers
            g.upload_walkers(initial_walkers(s, 500.0))
            out = g.step(dict(tau=s.tau, e_trial=s.e_trial0, reweight_factor_inv=1.0, r_initiator=1.0, min_wt=0.5, always_spawn_cutoff_wt=0.5,
                              initiator_power=0, initiator_min_distance=0, c_t_initiator=0, semistochastic=1, reached_w_abs_gen=0))
            wk = g.download_walkers()
        finally:
            g.close()
        res.append((h, np.array(out), wk))
    ref = [H.element(*map(int, r))[0] for r in a[:400]]
    assert np.allclose(res[0][0][:400], ref, rtol=0, atol=1e-14)
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    for k in ("up", "dn", "wt"):
        assert np.array_equal(res[0][2][k], res[1][2][k])
    assert len(res[0][2]["up"]) > 30
