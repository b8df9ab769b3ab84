"""The independent annihilation model (tests/anneal_checker.py) against the oracle's restatement of the same three pieces of the
reference -- merge_original_with_spawned2, reduce_my_walker and the sums of a generation -- on the inputs of the existing
annihilation-door tests (tests/test_gpu_parity.py: test_annihilate_door_matches_oracle_merge and
test_annihilate_door_random_parameters, same seeds), plus dyadic inputs with residents outside the deterministic space, which
those tests do not have (their 1,002 residents all carry imp_distance 0).

Outcome: the two agree on all of them -- determinants, weights, imp_distance and initiator bit for bit in the reference's own
left-to-right arithmetic, both RNG disciplines, with the model handed the oracle's random numbers for the rounding draws; the
weight sums bit for bit on dyadic weights; every sum within proposal_checker.rounding_bound of the correctly rounded one
otherwise (the oracle adds left to right, the model with math.fsum).  Neither had to be changed to follow the reference's text.
The model with the imp_distance 0 / -1 exception taken out, or with the fold made blind to the order inside a run, fails
test_model_equals_oracle_on_door_inputs (tried once on a scratch copy: flags fold(..., no_exception=True / order_blind=True),
kept as test_a_broken_model_is_noticed).

The plain step (semistochastic = f: the same fold, join_walker2, every zero dropped, the reweighting -- anneal_checker.plain_step)
against orc_merge_sort_walkers + orc_merge_original_with_spawned2 + orc_join_walker2 on random non-dyadic lists with the same
draws, both disciplines, bit for bit: test_plain_model_equals_oracle."""
import ctypes as C

import numpy as np
import pytest

import anneal_checker as AC
import proposal_checker as PC

SEED = (1346, 5634, 6635, 4361)


def _inputs_matches(oracle, c2_setup, rng_mode, rfi, heavy):
    """the hand-made collision-heavy list of test_annihilate_door_matches_oracle_merge"""
    rs = np.random.RandomState(1234 + rng_mode)
    main = oracle.initial_walkers(c2_setup, 300)
    n0 = len(main["up"])
    pool = rs.choice(len(c2_setup.ct_up), 6 if heavy else 80, replace=False)
    ns = 14000 if heavy else 4000
    from_main = rs.rand(ns) < (0.03 if heavy else 0.4)
    im, ip = rs.randint(0, n0, ns), pool[rs.randint(0, len(pool), ns)]
    up = np.where(from_main, main["up"][im], c2_setup.ct_up[ip]).astype(np.uint64)
    dn = np.where(from_main, main["dn"][im], c2_setup.ct_dn[ip]).astype(np.uint64)
    wt = rs.choice([-1.0, 1.0], ns) * rs.choice([0.05, 0.2, 0.25, 0.4, 0.5, 0.75, 1.0, 1.5], ns)
    wt[rs.rand(ns) < 0.05] = 0.0
    impd = rs.choice([-1, 1, 2, 3, 5], ns).astype(np.int8)
    init = np.where(impd == -1, 1, rs.randint(0, 2, ns)).astype(np.int8)
    if heavy:
        one = (~from_main) & (ip == pool[0])
        wt[one] = 0.3; impd[one] = 2; init[one] = 0
        imp_dets = np.nonzero(main["imp_distance"] == 0)[0]
        sel = rs.rand(ns) < 0.12
        up[sel], dn[sel] = main["up"][imp_dets[5]], main["dn"][imp_dets[5]]
        wt[sel] = -0.2; impd[sel] = np.where(rs.rand(int(sel.sum())) < 0.5, -1, 2); init[sel] = 1
    prm = dict(tau=c2_setup.tau, e_trial=-75.7, reweight_factor_inv=rfi, r_initiator=1.0, min_wt=0.5, always_spawn_cutoff_wt=0.5,
               initiator_power=0, initiator_min_distance=0, c_t_initiator=0, semistochastic=1, reached_w_abs_gen=2)
    return main, dict(up=up, dn=dn, wt=wt, imp_distance=impd, initiator=init), prm, rng_mode


def _inputs_random(oracle, c2_setup, trial):
    """test_annihilate_door_random_parameters"""
    rs = np.random.RandomState(900 + trial)
    rng_mode = trial % 2
    main = oracle.initial_walkers(c2_setup, 300)
    n0 = len(main["up"])
    npool = int(rs.choice([2, 5, 40, 300]))
    pool = rs.choice(len(c2_setup.ct_up), npool, replace=False)
    ns = int(rs.choice([3000, 9000]))
    from_main = rs.rand(ns) < rs.choice([0.02, 0.3])
    im, ip = rs.randint(0, n0, ns), pool[rs.randint(0, len(pool), ns)]
    up = np.where(from_main, main["up"][im], c2_setup.ct_up[ip]).astype(np.uint64)
    dn = np.where(from_main, main["dn"][im], c2_setup.ct_dn[ip]).astype(np.uint64)
    wt = rs.choice([-1.0, 1.0], ns, p=[0.3, 0.7]) * rs.choice([0.05, 0.2, 0.25, 0.4, 0.5, 0.75, 1.0, 1.5, 2.5], ns)
    wt[rs.rand(ns) < 0.04] = 0.0
    impd = rs.choice([-1, 1, 2, 3, 5, 127], ns, p=[0.12, 0.38, 0.25, 0.15, 0.08, 0.02]).astype(np.int8)
    init = np.where(impd == -1, 1, rs.randint(0, 3, ns)).astype(np.int8)
    prm = dict(tau=c2_setup.tau, e_trial=-75.7, reweight_factor_inv=float(rs.choice([1.0, 0.97, 1.02])), r_initiator=float(rs.choice([0.5, 1.0, 2.0, -1.0])),
               min_wt=float(rs.choice([0.3, 0.5, 1.0])), always_spawn_cutoff_wt=0.5, initiator_power=int(rs.choice([0, 1, 2])),
               initiator_min_distance=int(rs.choice([0, 1, 2])), c_t_initiator=int(rs.choice([0, 1])), semistochastic=1, reached_w_abs_gen=2)
    return main, dict(up=up, dn=dn, wt=wt, imp_distance=impd, initiator=init), prm, rng_mode


def _inputs_dyadic(oracle, c2_setup, trial):
    """weights k/4, residents of every kind: deterministic space, C(T)-like (imp_distance -2), stochastic space at several distances,
    initiators 0-3 -- what makes every sum exact and no draw necessary"""
    rs = np.random.RandomState(4100 + trial)
    main = oracle.initial_walkers(c2_setup, 300)
    keep = np.sort(rs.choice(len(main["up"]), 260, replace=False))
    if 0 not in keep and trial % 2:
        keep[0] = 0
    res = {k: v[keep].copy() for k, v in main.items()}
    n0 = len(keep)
    res["wt"] = rs.randint(-16, 17, n0) / 4.0
    kind = rs.randint(0, 4, n0)
    perm = res["initiator"] == 3
    res["imp_distance"] = np.where(kind == 0, 0, np.where(kind == 1, -2, rs.randint(1, 5, n0))).astype(np.int8)
    res["initiator"] = np.where(perm, 3, rs.randint(0, 3, n0)).astype(np.int8)
    res["wt"][(res["imp_distance"] >= 1) & (res["wt"] == 0)] = 0.5       # a stochastic-space resident has a weight
    pool = rs.choice(len(c2_setup.ct_up), 60, replace=False)
    ns = 5000
    from_main = rs.rand(ns) < 0.6
    im, ip = rs.randint(0, n0, ns), pool[rs.randint(0, len(pool), ns)]
    up = np.where(from_main, res["up"][im], c2_setup.ct_up[ip]).astype(np.uint64)
    dn = np.where(from_main, res["dn"][im], c2_setup.ct_dn[ip]).astype(np.uint64)
    wt = rs.randint(-8, 9, ns) / 4.0
    impd = rs.choice([-1, 1, 2, 3, 5, 127], ns).astype(np.int8)
    init = np.where(impd == -1, 1, rs.randint(0, 2, ns)).astype(np.int8)
    prm = AC.default_params(tau=c2_setup.tau, reweight_factor_inv=(1.0, 0.5)[trial % 2], r_initiator=(1.0, -1.0, 2.0)[trial % 3],
                            initiator_power=trial % 2, c_t_initiator=(trial // 2) % 2)
    return res, dict(up=up, dn=dn, wt=wt, imp_distance=impd, initiator=init), prm, trial % 2


def _oracle_three_routines(oracle, c2_walk, c2_setup, main, sp, prm, rng_mode):
    """sort, merge, reduce, reweighting and the sums, each through the oracle's own routine; also the random numbers its reduce
    routine saw, as a draw(up, dn) for the model"""
    n0 = len(main["up"])
    ow = oracle.OracleWalk(c2_walk, c2_setup, main, n0 + len(sp["up"]) + 16, list(SEED), rng_mode=rng_mode)
    L = oracle.lib()
    L.orc_det_rank.restype = C.c_uint64
    L.orc_det_rank.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_uint64]
    L.orc_rng_seek.argtypes = [C.c_void_p, C.c_int, C.c_uint64]
    L.orc_rannyu.restype = C.c_double
    L.orc_rannyu.argtypes = [C.c_void_p]
    rng = oracle.Rng.from_buffer_copy(ow.w.rng)

    def draw(up, dn):
        L.orc_rng_seek(C.byref(rng), 2, L.orc_det_rank(int(c2_walk.norb), int(c2_walk.ndn), up, dn))
        return L.orc_rannyu(C.byref(rng))
    w, nz = ow.w, np.nonzero(sp["wt"])[0]
    for k, j in enumerate(nz):
        i = n0 + k
        w.up[i], w.dn[i], w.wt[i] = int(sp["up"][j]), int(sp["dn"][j]), float(sp["wt"][j])
        w.imp_distance[i], w.initiator[i] = int(sp["imp_distance"][j]), int(sp["initiator"][j])
        w.matrix_elements[i] = w.e_num_walker[i] = w.e_den_walker[i] = 1e51
    n = n0 + len(nz)
    p = oracle.StepParams(**prm)
    L.orc_reduce_my_walker.restype = C.c_int64
    L.orc_reduce_my_walker.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.orc_merge_original_with_spawned2.restype = C.c_int64
    L.orc_generation_sums.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.orc_merge_sort_walkers(ow.h, n)
    n = L.orc_merge_original_with_spawned2(ow.h, n, C.byref(p))
    n = L.orc_reduce_my_walker(ow.h, n, C.byref(p))
    ow.w.nwalk = n
    for i in range(n):
        w.wt[i] = w.wt[i] * prm["reweight_factor_inv"]
    out = np.zeros(16)
    L.orc_generation_sums(ow.h, n, C.byref(p), out.ctypes.data_as(C.c_void_p))
    ref = ow.walkers(); ow.close()
    return ref, out, draw


def _ct(c2_setup):
    return {(int(u), int(d)): (float(a), float(b)) for u, d, a, b in zip(c2_setup.ct_up, c2_setup.ct_dn, c2_setup.ct_num, c2_setup.ct_den)}


CASES = [("matches", a) for a in [(0, 1.0, False), (1, 1.0, False), (1, 0.93, False), (0, 1.0, True), (1, 0.93, True)]] + \
        [("random", t) for t in range(12)] + [("dyadic", t) for t in range(6)]


def _make(oracle, c2_setup, kind, arg):
    if kind == "matches":
        return _inputs_matches(oracle, c2_setup, *arg)
    return (_inputs_random if kind == "random" else _inputs_dyadic)(oracle, c2_setup, arg)


@pytest.fixture(scope="module")
def ct_table(c2_setup):
    return _ct(c2_setup)


@pytest.mark.parametrize("kind,arg", CASES, ids=lambda x: str(x).replace(" ", ""))
def test_model_equals_oracle_on_door_inputs(oracle, c2_walk, c2_setup, ct_table, kind, arg):
    main, sp, prm, rng_mode = _make(oracle, c2_setup, kind, arg)
    ref, out, draw = _oracle_three_routines(oracle, c2_walk, c2_setup, main, sp, prm, rng_mode)
    got = AC.fold(main, sp, prm, exact=False, draw=draw)
    assert len(got["up"]) == len(ref["up"]) == int(out[5])
    for k in ("up", "dn", "wt", "imp_distance", "initiator"):
        assert np.array_equal(got[k], ref[k]), k
    st, spread = AC.sums(got, prm, ct_table, 0, 0.0)
    n = len(got["up"])
    wsum = float(np.abs(got["wt"]).sum())
    for k in AC.EXACT_STATS:
        bound = 0.0 if kind == "dyadic" else PC.rounding_bound(n, wsum * max(1.0, float(np.abs(got["wt"]).max())))
        assert abs(st[k] - out[k]) <= bound, (AC.STAT_NAMES[k], st[k], out[k])
    for k in AC.TABLE_STATS:
        assert abs(st[k] - out[k]) <= PC.rounding_bound(*spread[k]), (AC.STAT_NAMES[k], st[k], out[k])
    assert abs(st[3]) > 1.0 and abs(st[2]) > 0.1          # the table sums are not vacuous
    if kind == "dyadic":      # exact arithmetic gives the same bits, no draw is consumed, and the rule-free invariants hold exactly
        AC.check_precondition(main, sp, prm)
        ex = AC.fold(main, sp, prm, exact=True)
        for k in ("up", "dn", "wt", "imp_distance", "initiator"):
            assert np.array_equal(ex[k], got[k]), k
        assert not AC.invariants(main, sp, prm, ref, ex["discarded"], ex["reset"])
        assert len(ex["rounded"]) == 0
    else:
        bad = AC.invariants(main, sp, prm, got, got["discarded"], got["reset"], tol=2.0 ** -40)
        bad = [b for b in bad if not (b[0] == "b" and b[1] in set(got["rounded"]))]          # a drawn weight is min_wt, not the sum
        lost = {k for k in got["rounded"]} - {(int(u), int(d)) for u, d in zip(got["up"], got["dn"])}
        bad = [b for b in bad if not (b[0] == "c" and set(b[2]) <= lost and not b[1])]
        assert not bad, bad[:3]


def test_a_broken_model_is_noticed(oracle, c2_walk, c2_setup):
    """the two mistakes the twin test must catch: the imp_distance 0 / -1 exception dropped, the fold blind to the order in a run"""
    main, sp, prm, rng_mode = _inputs_dyadic(oracle, c2_setup, 0)
    ref, out, draw = _oracle_three_routines(oracle, c2_walk, c2_setup, main, sp, prm, rng_mode)
    good = AC.fold(main, sp, prm)
    assert np.array_equal(good["wt"], ref["wt"]) and np.array_equal(good["initiator"], ref["initiator"])
    no_exc = AC.fold(main, sp, prm, no_exception=True)
    assert not (len(no_exc["wt"]) == len(ref["wt"]) and np.array_equal(no_exc["wt"], ref["wt"]))
    assert AC.invariants(main, sp, prm, no_exc, no_exc["discarded"], no_exc["reset"])          # invariant (b) sees it without any flag rule
    blind = AC.fold(main, sp, prm, order_blind=True)
    assert not (len(blind["up"]) == len(ref["up"]) and np.array_equal(blind["initiator"], ref["initiator"]))


# ------------------------------------------------------------------------------------------------ semistochastic = f
def _oracle_plain_step(oracle, c2_walk, c2_setup, main, sp, prm, rng_mode):
    """sort, merge, join_walker2 and the reweighting through the oracle's routines; also the generator its joins drew from, as a
    draw(index of the later walker) for the model: COUNTER stage 2 keyed by that index, REPLAY the stream in join order"""
    n0 = len(main["up"])
    ow = oracle.OracleWalk(c2_walk, c2_setup, main, n0 + len(sp["up"]) + 16, list(SEED), rng_mode=rng_mode)
    L = oracle.lib()
    L.orc_rng_seek.argtypes = [C.c_void_p, C.c_int, C.c_uint64]
    L.orc_rannyu.restype = C.c_double
    L.orc_rannyu.argtypes = [C.c_void_p]
    rng = oracle.Rng.from_buffer_copy(ow.w.rng)

    def draw(i):
        L.orc_rng_seek(C.byref(rng), 2, int(i))          # does nothing in the REPLAY discipline
        return L.orc_rannyu(C.byref(rng))
    w, nz = ow.w, np.nonzero(sp["wt"])[0]
    for k, j in enumerate(nz):
        i = n0 + k
        w.up[i], w.dn[i], w.wt[i] = int(sp["up"][j]), int(sp["dn"][j]), float(sp["wt"][j])
        w.imp_distance[i], w.initiator[i] = int(sp["imp_distance"][j]), int(sp["initiator"][j])
        w.matrix_elements[i] = w.e_num_walker[i] = w.e_den_walker[i] = 1e51
    n = n0 + len(nz)
    p = oracle.StepParams(**prm)
    L.orc_merge_original_with_spawned2.restype = C.c_int64
    L.orc_join_walker2.restype = C.c_int64
    L.orc_join_walker2.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.orc_merge_sort_walkers(ow.h, n)
    n = L.orc_merge_original_with_spawned2(ow.h, n, C.byref(p))
    n_merged = n
    n = L.orc_join_walker2(ow.h, n, C.byref(p))
    ow.w.nwalk = n
    for i in range(n):
        w.wt[i] = w.wt[i] * prm["reweight_factor_inv"]
    ref = ow.walkers(); ow.close()
    return ref, n_merged, draw


@pytest.mark.parametrize("trial", range(8))
def test_plain_model_equals_oracle(oracle, c2_walk, c2_setup, trial):
    """random non-dyadic lists, the reference's left-to-right arithmetic, the same draws, both disciplines (odd trials COUNTER)"""
    main, sp, prm, rng_mode = _inputs_random(oracle, c2_setup, trial)
    prm = dict(prm, semistochastic=0)
    if trial >= 4:          # residents of the stochastic space too, some of them small
        main = {k: v.copy() for k, v in main.items()}
        rs = np.random.RandomState(trial)
        out = rs.rand(len(main["up"])) < 0.5
        main["imp_distance"] = np.where(out & (main["initiator"] < 3), 2, main["imp_distance"]).astype(np.int8)
        main["wt"] = np.where(out & (main["initiator"] < 3), rs.choice([-0.07, 0.13, 0.2, -0.45, 1.1], len(out)), main["wt"])
    rs = np.random.RandomState(50 + trial)          # 600 lone children below min_wt on determinants of their own: the joins' candidates
    ix = rs.choice(len(c2_setup.ct_up), 600, replace=False)
    sp = dict(up=np.concatenate([sp["up"], c2_setup.ct_up[ix].astype(np.uint64)]), dn=np.concatenate([sp["dn"], c2_setup.ct_dn[ix].astype(np.uint64)]),
              wt=np.concatenate([sp["wt"], rs.uniform(-0.29, 0.29, 600)]), imp_distance=np.concatenate([sp["imp_distance"], rs.choice([1, 2, 3], 600).astype(np.int8)]),
              initiator=np.concatenate([sp["initiator"], np.ones(600, np.int8)]))
    ref, n_merged, draw = _oracle_plain_step(oracle, c2_walk, c2_setup, main, sp, prm, rng_mode)
    got = AC.plain_step(main, sp, prm, draw, exact=False)
    assert len(got["heads"]["up"]) == n_merged and got["joins"] > 300
    assert len(got["up"]) == len(ref["up"])
    for k in ("up", "dn", "wt", "imp_distance", "initiator"):
        assert np.array_equal(got[k], ref[k]), k
    assert not (got["wt"] == 0).any()


def test_precondition_refuses_an_input_that_needs_a_draw():
    res = dict(up=np.array([15], np.uint64), dn=np.array([15], np.uint64), wt=np.array([1.0]), imp_distance=np.array([2], np.int8),
               initiator=np.array([2], np.int8), perm_sign=np.zeros(1, np.int8))
    sp = dict(up=np.array([23], np.uint64), dn=np.array([15], np.uint64), wt=np.array([0.125]), imp_distance=np.array([3], np.int8), initiator=np.array([1], np.int8))
    with pytest.raises(AssertionError):
        AC.check_precondition(res, sp, AC.default_params())
    sp["wt"] = np.array([0.25])
    AC.check_precondition(res, sp, AC.default_params())
    with pytest.raises(AC.NeedsDraw):          # a dyadic weight below min_wt after a partial cancellation cannot occur at 0.25; at min_wt 0.5 it can
        AC.fold(res, sp, AC.default_params(min_wt=0.5))


def test_first_record_of_the_list_keeps_its_minus_one(oracle):
    """5985-5988 turn imp_distance -1 into 1 when a run's first record is copied into place; the list's own first record is never
    copied (the loop starts at 2) and keeps -1 until 6032-6036: it is then no target for min(., |imp_distance|) = 1 -- the same value --
    and not discarded by 5970, only by 6038 when the whole list is one run.  A one-run and a two-run list through model and oracle."""
    import ctypes as C
    L = oracle.lib()
    for n_runs in (1, 2):
        recs = [(15, 15, 0.5, -1, 1), (15, 15, -0.5, 2, 0)] + ([(23, 15, 1.0, 3, 1)] if n_runs == 2 else [])
        sp = dict(up=np.array([r[0] for r in recs], np.uint64), dn=np.array([r[1] for r in recs], np.uint64), wt=np.array([r[2] for r in recs]),
                  imp_distance=np.array([r[3] for r in recs], np.int8), initiator=np.array([r[4] for r in recs], np.int8))
        res = dict(up=np.zeros(0, np.uint64), dn=np.zeros(0, np.uint64), wt=np.zeros(0), imp_distance=np.zeros(0, np.int8), initiator=np.zeros(0, np.int8),
                   perm_sign=np.zeros(0, np.int8))
        got = AC.fold(res, sp, AC.default_params())
        h = L.orc_walk_new(16)
        w = oracle.Walk.from_address(h)
        for i, r in enumerate(recs):
            w.up[i], w.dn[i], w.wt[i], w.imp_distance[i], w.initiator[i] = r
            w.matrix_elements[i] = w.e_num_walker[i] = w.e_den_walker[i] = 1e51
        p = oracle.StepParams(**AC.default_params())
        L.orc_merge_original_with_spawned2.restype = C.c_int64
        L.orc_reduce_my_walker.restype = C.c_int64
        L.orc_reduce_my_walker.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
        n = L.orc_merge_original_with_spawned2(h, len(recs), C.byref(p))
        assert n == (0, 2)[n_runs - 1]          # the cancelled first run survives the merge only where 5970 judges it, with -1 (6038 sees 1)
        n = L.orc_reduce_my_walker(h, n, C.byref(p))
        assert n == len(got["up"])
        for i in range(n):
            assert (w.up[i], w.wt[i], w.imp_distance[i], w.initiator[i]) == (got["up"][i], got["wt"][i], got["imp_distance"][i], got["initiator"][i])
        L.orc_walk_free(h)
