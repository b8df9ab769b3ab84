"""The child program of tests/test_gpu_shard_phases.py: one process drives R ranks' worth of the three-phase sharded step
(sqmc_gpu_shard_begin / _pack / _finish take device pointers and communicate nothing), does the exchanges in numpy, and holds
every phase to the model of tests/shard_checker.py (the finish: anneal_checker.fold / sums).

    python shard_phase_cases.py MODE OUTDIR

MODE  projection / projection_radix      projection at row-length seams: one rank (step, run of 2 steps plain and chained), sharded
                        R = 2, 3 by hash and R = 3 by hand; bit for bit (projection_radix: SQMC_BUCKET=0, see run_projection)
      physics           death/clone and the real projector against the independent H, R = 3; writes projector.npz for the parent
      routing_c2 / routing_heg57 / routing_heatbath     the send buffer of (r, R) against route() of the (0, 1) twin's records;
                        routing_c2 also holds the refusals of sqmc_gpu_shard_config / _begin
      finish_radix / finish_bucket      sqmc_gpu_shard_finish on records built here, exact and RNG-free (the environment selects the tail)
      natural           R = 2 and 3: buckets delivered in rank order, conservation, ownership, no determinant twice

Every check prints one JSON line {"case", "ok", "why"}; the last line counts the failures and gives the wall time.  Exit 0: all
checks hold; 1: a mismatch; 3: the library reported a HIP failure (the program stops at once and starts nothing more).
The R contexts of a case live side by side in this process: nothing in the library is process-global but the environment
switches it reads once."""
import json
import math
import os
import sys
import time
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import anneal_checker as AC      # noqa: E402
import proposal_checker as PC    # noqa: E402
import shard_checker as SC       # noqa: E402

FCIDUMP = os.path.join(ROOT, "tests", "golden", "C2_r1.24253_FCIDUMP")
SEED = (1346, 5634, 6635, 4361)
MWALK = 200000
CAP = 1 << 16                       # records of a send / receive buffer (every case spawns far fewer)
NSEAM = 224
TAU, E_TRIAL = 2.0 ** -6, -75.75
BIG_MIN_WT = 2.0 ** 200             # see run_projection

ENV = {"projection": {}, "projection_radix": {"SQMC_BUCKET": "0"}, "physics": {}, "routing_c2": {}, "routing_heg57": {}, "routing_heatbath": {},
       "finish_radix": {"SQMC_SHARD_BUCKET": "0"}, "finish_bucket": {"SQMC_BUCKET_HOLDOFF": "0"}, "natural": {}}

_T = {}          # torch, sqmc_amd, host, device: imported by main() (torch before the HIP library)
_N = {"bad": 0}


def say(case, why=None, **kw):
    rec = dict(case=case, ok=why is None)
    if why is not None:
        rec["why"] = str(why); _N["bad"] += 1
    rec.update(kw)
    print(json.dumps(rec, default=str), flush=True)


def first(*msgs):
    for m in msgs:
        if m is not None:
            return m
    return None


def params(**kw):
    p = dict(tau=TAU, e_trial=E_TRIAL, reweight_factor_inv=0.5, r_initiator=1.0, min_wt=0.25, always_spawn_cutoff_wt=0.25, initiator_power=0,
             initiator_min_distance=0, c_t_initiator=0, semistochastic=1, reached_w_abs_gen=2)
    p.update(kw)
    return p


def walkers(up, dn, wt, imp, init, psign=None):
    n = len(up)
    big = np.full(n, 1e51)
    bc = lambda v, t: np.ascontiguousarray(np.broadcast_to(np.asarray(v, t), (n,)))
    return dict(up=np.asarray(up, np.uint64), dn=np.asarray(dn, np.uint64), wt=bc(wt, np.float64), imp_distance=bc(imp, np.int8), initiator=bc(init, np.int8),
                perm_sign=bc(0 if psign is None else psign, np.int8), matrix_elements=big, e_num=big.copy(), e_den=big.copy())


def take(w, mask):
    return {k: v[mask] for k, v in w.items()}


def join_sorted(a, b):
    """two walker dicts with no determinant in common, as one list sorted by (up, dn)"""
    if b is None or len(b["up"]) == 0:
        return a
    m = {k: np.concatenate([a[k], b[k]]) for k in a}
    o = np.lexsort((m["dn"], m["up"]))
    keys = list(zip(m["up"][o].tolist(), m["dn"][o].tolist()))
    assert len(set(keys)) == len(keys)
    return {k: v[o] for k, v in m.items()}


def keyset(up, dn):
    return set(zip((int(x) for x in up), (int(x) for x in dn)))


def ct_outside(s, exclude, idx):
    """determinants of the C(T) list at the given positions, those of `exclude` left out"""
    keep = [i for i in idx if (int(s.ct_up[i]), int(s.ct_dn[i])) not in exclude]
    return s.ct_up[keep].copy(), s.ct_dn[keep].copy()


def c2_setup():
    H = _T["H"]
    hst = H.ChemHost(FCIDUMP, 8, 4, "d2h")
    g = hst.gpu(rng_mode=H.RNG_COUNTER, seed=SEED, mwalk=MWALK)
    s = hst.setup_walk(g, 100, 1000, 0.1)
    g.close()
    return hst, s


def c2_ctx(hst, s, prj, seed=SEED, rng_mode=None, table=True):
    H = _T["H"]
    g = hst.gpu(rng_mode=H.RNG_COUNTER if rng_mode is None else rng_mode, seed=seed, mwalk=MWALK)
    if prj is not None:
        g.set_projector(*prj)
    if table:
        g.set_ct_table(s.ct_up, s.ct_dn, s.ct_num, s.ct_den)
    return g


def dev_buffers(n_x):
    torch = _T["torch"]
    xg = torch.full((max(n_x, 1),), 123.0, dtype=torch.float64, device=_T["dev"])          # shard_begin zeroes it itself: the fill must not survive
    send = torch.full((CAP, 4), -1, dtype=torch.int64, device=_T["dev"])
    return xg, send


def read_x(xg, n):
    _T["torch"].cuda.synchronize()
    return xg[:n].cpu().numpy().copy()


def write_x(xg, x):
    torch = _T["torch"]
    xg[:len(x)].copy_(torch.from_numpy(np.array(x, np.float64)))
    torch.cuda.synchronize()


def read_send(send, counts):
    """(the first sum(counts) records as 64-bit words, are the rows behind them untouched)"""
    _T["torch"].cuda.synchronize()
    ns = int(np.sum(counts))
    return send[:ns].cpu().numpy().view(np.uint64).reshape(-1, 4).copy(), bool((send[ns:] == -1).all().item())


def to_dev(words):
    torch = _T["torch"]
    a = np.ascontiguousarray(np.asarray(words, np.uint64).reshape(-1, 4)).view(np.int64)
    t = torch.zeros((max(len(a), 1), 4), dtype=torch.int64, device=_T["dev"])
    if len(a):
        t[:len(a)].copy_(torch.from_numpy(a))
    torch.cuda.synchronize()
    return t


# ================================================================================================ projection at row-length seams
def seam_setting(s):
    counts, indices, values, hubs = SC.seam_projector(NSEAM)
    rows = SC.expand_upper(counts, indices, values)
    lengths = [len(r) for r in rows]
    assert set(SC.SEAM_LENGTHS) <= set(lengths), "the synthetic projector lacks a seam length"
    w = SC.seam_weights(NSEAM)
    up, dn = s.imp_up[:NSEAM].copy(), s.imp_dn[:NSEAM].copy()
    assert all((int(a), int(b)) < (int(c), int(d)) for a, b, c, d in zip(up[:-1], dn[:-1], up[1:], dn[1:]))
    det = walkers(up, dn, w, 0, 2)
    return (counts, indices, values), rows, hubs, det


def exact_steps(rows, w, nsteps, rfi=0.5):
    """the model applied nsteps times: per step (the mid-step weights, the weights after reweighting), every one asserted to be an
    exact double -- the precondition of the bit comparison"""
    x, out = [float(v) for v in w], []
    for _ in range(nsteps):
        y = SC.project(rows, x, E_TRIAL, TAU, exact=True)
        z = [q * Fraction(rfi) for q in y]
        assert all(SC.is_exact_double(q) for q in y) and all(SC.is_exact_double(q) and q != 0 for q in z), "the dyadic case left the doubles"
        out.append((np.array([float(q) for q in y]), np.array([float(q) for q in z])))
        x = [float(q) for q in z]
    return out


def det_part(wk, det):
    """the deterministic walkers of a downloaded list and whether they are exactly the determinants `det` in order"""
    sel = wk["imp_distance"] == 0
    same = np.array_equal(wk["up"][sel], det["up"]) and np.array_equal(wk["dn"][sel], det["dn"])
    return sel, None if same else "the walkers of imp_distance 0 are not the deterministic space (%d of %d)" % (int(sel.sum()), len(det["up"]))


def run_projection(outdir):
    """Weights, projector values, tau, e_trial and reweight_factor_inv are dyadic, so every product and sum is exact and the
    library must return the model's bits whatever order it adds in.  The population is the deterministic walkers alone: all their
    children carry imp_distance -1 (spawn_emit, sqmc_amd/csrc/walk_kernels.h: "if (p.semi && pd == 0) d = -1"), and the merge
    does not add such a child onto a determinant of the deterministic space (bk_fold, bucket_kernels.h:
    "if (!(d == 0 && d2 == -1)) wt = wt + w2", do_walk.f90:5950): the child is not dropped when it is spawned, it is dropped when
    it is merged, and no child touches a deterministic weight.  Children that land outside the deterministic space would become
    stochastic walkers and spawn back into it in the second step; min_wt = 2^200 makes reduce_my_walker round every one of them
    away (survival probability |w| / min_wt < 2^-190 against a draw of k / 2^48), so the second step is the model applied twice.
    Routes of the second step of sqmc_gpu_run: behind a bucket tail the pipelined head computes y = A x itself (d_prj_y) and the
    step only adds the closing line; behind a radix tail (SQMC_BUCKET=0, mode projection_radix) k_prj_apply runs as a kernel of
    its own.  The library has no door that names the route: the child reports sqmc_gpu_last_tail and the count of bucket steps."""
    hst, s = c2_setup()
    prj, rows, hubs, det = seam_setting(s)
    prm = params(min_wt=BIG_MIN_WT, always_spawn_cutoff_wt=0.5)
    steps = exact_steps(rows, det["wt"], 2)
    n = NSEAM
    # ---- one rank, sqmc_gpu_step
    g = c2_ctx(hst, s, prj)
    g.upload_walkers(det)
    out = g.step(prm)
    wk = g.download_walkers()
    sel, why = det_part(wk, det)
    why = first(why, SC.compare_bits("weights after sqmc_gpu_step", wk["wt"][sel], steps[0][1]) if why is None else None,
                None if out[6] == math.fsum(abs(v) for v in steps[0][1]) else "w_abs_gen_imp = %r" % out[6])
    say("one_rank_step", why, tail=g.last_tail(), nwalk=len(wk["up"]), children=int(out[15]))
    g.close()
    # ---- one rank, sqmc_gpu_run of 2 steps, plain and chained
    H = _T["H"]
    for chained in (False, True):
        g = c2_ctx(hst, s, prj)
        if chained:
            g.set_chained_runs(True)
        g.upload_walkers(det)
        pc = H.PopControl(TAU, E_TRIAL, 1000.0, n_equil_steps=0)
        pc.reached, pc.rfi, pc.rfi_max = 2, 0.5, 0.5          # past the target; reweight_factor_inv clamped to [0.5, 0.5]; e_trial moves in equilibration only
        c = pc.to_c(float(np.abs(det["wt"]).sum()), min_wt=BIG_MIN_WT, cutoff=0.5)
        stats, _ = g.run(c, 2)
        wk = g.download_walkers()
        sel, why = det_part(wk, det)
        why = first(why, None if (c.reweight_factor_inv == 0.5 and c.e_trial == E_TRIAL and c.tau == TAU) else "the population control moved a scalar",
                    SC.compare_bits("weights after 2 steps", wk["wt"][sel], steps[1][1]) if why is None else None,
                    None if stats[0][6] == math.fsum(abs(v) for v in steps[0][1]) else "step 1: w_abs_gen_imp = %r" % stats[0][6],
                    None if stats[1][6] == math.fsum(abs(v) for v in steps[1][1]) else "step 2: w_abs_gen_imp = %r" % stats[1][6])
        say("one_rank_run2_%s" % ("chained" if chained else "plain"), why, last_tail=g.last_tail(), bucket_steps=g.tail_stats()[0], nwalk=len(wk["up"]))
        g.close()
    # ---- sharded: every rank of R = 2 and R = 3 by hash, R = 3 by hand
    g = c2_ctx(hst, s, None, table=False)
    by_hash = {R: g.det_owner(det["up"], det["dn"], R) for R in (2, 3)}
    g.close()
    hand = np.where(np.arange(n) % 2 == 1, 1, 0)
    hand[hubs[64]] = hand[hubs[128]] = 1                      # one rank owns the rows of 64 and of 128 ...
    xu, xd = ct_outside(s, keyset(det["up"], det["dn"]), range(5000, 5000 + 40 * 50, 50))
    extra = walkers(xu, xd, np.where(np.arange(len(xu)) % 2 == 0, 1.5, -2.25), 1, 2)      # ... and one owns no row at all, but has walkers
    for tag, R, owners, extras in (("hash_R2", 2, by_hash[2], {}), ("hash_R3", 3, by_hash[3], {}), ("hand_R3", 3, hand, {2: extra})):
        ranks = []
        for r in range(R):
            g = c2_ctx(hst, s, prj, seed=H.rank_seed(SEED, r))
            mine = owners == r
            rows_r = np.nonzero(mine)[0]
            wk0 = join_sorted(take(det, mine), extras.get(r))
            g.shard_config(r, R, rows_r)
            g.upload_walkers(wk0)
            xg, send = dev_buffers(n)
            nch = g.shard_begin(prm, xg.data_ptr())
            x_r = read_x(xg, n)
            why = SC.compare_bits("x_global", x_r, SC.gather(wk0["wt"][wk0["imp_distance"] == 0], rows_r, n))
            say("%s_rank%d_begin" % (tag, r), why, rows=len(rows_r), walkers=len(wk0["up"]), children=nch)
            ranks.append((g, rows_r, wk0, xg, send, x_r))
        xsum = np.sum([t[5] for t in ranks], axis=0)
        say("%s_allreduce" % tag, SC.compare_bits("sum of the ranks' vectors", xsum, det["wt"]))
        for r, (g, rows_r, wk0, xg, send, _) in enumerate(ranks):
            write_x(xg, xsum)
            counts = g.shard_pack(prm, xg.data_ptr(), send.data_ptr(), CAP, R)
            mid = g.download_walkers()
            sel = mid["imp_distance"] == 0
            want = np.array([float(q) for q in SC.project(rows, xsum, E_TRIAL, TAU, exact=True, only=rows_r)])
            assert np.array_equal(want, steps[0][0][rows_r])
            why = first(None if (np.array_equal(mid["up"], wk0["up"]) and np.array_equal(mid["dn"], wk0["dn"])) else "the mid-step list is not the resident list",
                        SC.compare_bits("projected weights", mid["wt"][sel], want))
            # controls: what the library returned does NOT agree with the model once a mistake is planted in the model
            if set(len(rows[i]) for i in rows_r) & {64, 128}:
                short = [float(q) for q in SC.project(rows, xsum, E_TRIAL, TAU, exact=True, only=rows_r, drop_last_at_64=True)]
                why = first(why, None if SC.compare_bits("control", mid["wt"][sel], short) is not None else "control: a model that drops the last term of a row of 64 agrees with the library")
            if not np.array_equal(rows_r, np.arange(len(rows_r))):
                x_bad = SC.gather(wk0["wt"][wk0["imp_distance"] == 0], rows_r, n, rows_as_local=True)
                why = first(why, None if SC.compare_bits("control", ranks[r][5], x_bad) is not None else "control: a model that takes global_row as the local index agrees with the library")
            say("%s_rank%d_pack" % (tag, r), why, rows=len(rows_r), lengths=sorted(set(len(rows[i]) for i in rows_r) & set(SC.SEAM_LENGTHS)), sent=int(counts.sum()))
        for t in ranks:
            t[0].close()


# ================================================================================================ death/clone and the real projector
def real_population(s, n_extra=1500):
    """initial_walkers(s, 2000) with every zero deterministic weight replaced (x is dense), and, because that list lies wholly
    inside the deterministic space, n_extra stochastic walkers on C(T) determinants outside it"""
    H = _T["H"]
    wk = H.initial_walkers(s, 2000)
    i = np.arange(len(wk["up"]))
    zero = (wk["wt"] == 0) & (wk["imp_distance"] == 0)
    wk["wt"] = np.where(zero, np.where(i % 2 == 0, 1.0, -1.0) * (0.013 + 0.0007 * (i % 37)), wk["wt"])
    xu, xd = ct_outside(s, keyset(wk["up"], wk["dn"]), np.linspace(1000, len(s.ct_up) - 1000, n_extra).astype(np.int64))
    k = np.arange(len(xu))
    extra = walkers(xu, xd, np.where(k % 3 == 0, -1.0, 1.0) * (0.61 + 0.37 * (k % 11) + 1e-3 * (k % 7)), 1 + k % 3, np.where(k % 3 == 0, 2, 1))
    return join_sorted(wk, extra)


def imp_rows(s, wk):
    where = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(s.imp_up, s.imp_dn))}
    return np.array([where[(int(a), int(b))] for a, b, d in zip(wk["up"], wk["dn"], wk["imp_distance"]) if d == 0], np.int64)


def run_physics(outdir):
    """Tolerances, derived: H_ii of the library against fsum of the independent H's terms: rounding_bound(n_terms, sum |terms|) = b.
    w' = w f, f = 1 + tau (e_trial - H_ii): the subtraction and the product with tau round once each, relative to
    tau (|e_trial| + |H_ii|); the sum with 1 once, relative to |f|; the product with w once, relative to |w f|; a fused
    multiply-add only removes roundings.  So |w' - model| <= |w| tau b + 2^-53 (2 |w| tau (|e_trial| + |H_ii|) + 4 |w| max(|f|, 1)),
    the last term with the model's own two roundings.  Deterministic walkers: shard_checker.project(exact=False) and its bound."""
    hst, s = c2_setup()
    H = _T["H"]
    np.savez(os.path.join(outdir, "projector.npz"), counts=s.prj_counts, indices=s.prj_indices, values=s.prj_values, imp_up=s.imp_up, imp_dn=s.imp_dn,
             tau=s.tau, orb_order=np.array([int(hst.orb_order[i]) for i in range(1, hst.norb + 1)]))
    HH = PC.ChemH(FCIDUMP, [int(hst.orb_order[i]) for i in range(1, hst.norb + 1)])
    wk = real_population(s)
    prj = (s.prj_counts, s.prj_indices, s.prj_values)
    rows = SC.expand_upper(*prj)
    n = len(s.imp_up)
    prm = params(tau=s.tau, e_trial=s.e_trial0, reweight_factor_inv=1.0, min_wt=0.5, always_spawn_cutoff_wt=0.5)
    R = 3
    g = c2_ctx(hst, s, None, table=False)
    owners = g.det_owner(wk["up"], wk["dn"], R)
    g.close()
    ranks = []
    for r in range(R):
        g = c2_ctx(hst, s, prj, seed=H.rank_seed(SEED, r))
        wk0 = take(wk, owners == r)
        rows_r = imp_rows(s, wk0)
        g.shard_config(r, R, rows_r)
        g.upload_walkers(wk0)
        xg, send = dev_buffers(n)
        nch = g.shard_begin(prm, xg.data_ptr())
        x_r = read_x(xg, n)
        say("physics_rank%d_begin" % r, SC.compare_bits("x_global", x_r, SC.gather(wk0["wt"][wk0["imp_distance"] == 0], rows_r, n)), rows=len(rows_r), walkers=len(wk0["up"]), children=nch)
        ranks.append((g, rows_r, wk0, xg, send, x_r))
    xsum = np.sum([t[5] for t in ranks], axis=0)
    assert np.all(xsum != 0), "x is meant to be dense"
    u = 2.0 ** -53
    for r, (g, rows_r, wk0, xg, send, _) in enumerate(ranks):
        write_x(xg, xsum)
        g.shard_pack(prm, xg.data_ptr(), send.data_ptr(), CAP, R)
        mid = g.download_walkers()
        why = None if (np.array_equal(mid["up"], wk0["up"]) and np.array_equal(mid["dn"], wk0["dn"])) else "the mid-step list is not the resident list"
        det = wk0["imp_distance"] == 0
        ys, bounds = SC.project(rows, xsum, prm["e_trial"], prm["tau"], exact=False, only=rows_r)
        why = first(why, SC.compare_within("projected weights", mid["wt"][det], ys, bounds))
        want_w, tol_w, want_h, tol_h = [], [], [], []
        for a, b, w in zip(wk0["up"][~det], wk0["dn"][~det], wk0["wt"][~det]):
            hii, nt, sa = HH.element(int(a), int(b), int(a), int(b))
            bnd = PC.rounding_bound(nt, sa)
            f = 1 + Fraction(prm["tau"]) * (Fraction(prm["e_trial"]) - Fraction(hii))
            want_w.append(float(Fraction(float(w)) * f))
            tol_w.append(abs(w) * prm["tau"] * bnd + u * (2 * abs(w) * prm["tau"] * (abs(prm["e_trial"]) + abs(hii)) + 4 * abs(w) * max(abs(float(f)), 1.0)))
            want_h.append(hii); tol_h.append(bnd)
        why = first(why, SC.compare_within("H_ii (matrix_elements)", mid["matrix_elements"][~det], want_h, tol_h),
                    SC.compare_within("weights after death/clone", mid["wt"][~det], want_w, tol_w))
        say("physics_rank%d_pack" % r, why, deterministic=int(det.sum()), stochastic=int((~det).sum()), compared=int(det.sum()) + len(want_w), walkers=len(wk0["up"]))
    for t in ranks:
        t[0].close()


# ================================================================================================ routing
def pack_one(g, prm, wk, rank, R, rows, owner_hash, n_x):
    g.set_owner_hash(owner_hash)
    g.shard_config(rank, R, rows)
    g.upload_walkers(wk)
    xg, send = dev_buffers(n_x)
    nch = g.shard_begin(prm, xg.data_ptr())
    counts = g.shard_pack(prm, xg.data_ptr(), send.data_ptr(), CAP, R)
    words, untouched = read_send(send, counts)
    return nch, counts, words, untouched, (xg, send)


def owners_of(twin, words, R, owner_hash):
    """the independent owner of every record: owner_djb for hash 1; for hash 0 (the library's own mix) the det_owner door of a
    context left in mode 0"""
    if owner_hash == 1:
        return np.array([SC.owner_djb(int(r[0]), int(r[1]), R) for r in words], np.int64)
    return twin.det_owner(words[:, 0], words[:, 1], R).astype(np.int64)


def routing_cases(tag, make_ctx, prm, big, small, rows, n_x, door_ctx):
    """(r, R) in {(1, 2), (2, 3), (100, 255)} x both hashes against the (0, 1) twin of the same walker list, seed and step number"""
    twins = {}
    for name, wk in (("big", big), ("small", small)):
        g = make_ctx()
        nch, counts, words, untouched, keep = pack_one(g, prm, wk, 0, 1, rows, 0, n_x)
        twins[name] = (g, nch, words, keep)
        say("%s_twin_%s" % (tag, name), first(None if untouched else "rows behind the records were written", None if len(counts) == 1 else "counts"), children=nch, records=len(words),
            walkers=len(wk["up"]))
    out = {}
    for (r, R) in ((1, 2), (2, 3), (100, 255)):
        name = "small" if R == 255 else "big"
        wk = small if R == 255 else big
        tg, tnch, twords, _ = twins[name]
        for h in (0, 1):
            g = make_ctx()
            nch, counts, words, untouched, keep = pack_one(g, prm, wk, r, R, rows, h, n_x)
            own = owners_of(door_ctx, twords, R, h)
            why = first(None if nch == tnch else "%d children, the twin %d" % (nch, tnch),
                        None if (own.min() >= 0 and own.max() < R) else "an owner outside [0, R)",
                        SC.compare_route(words, counts, twords, own, R),
                        None if untouched else "rows of the send buffer behind sum(counts) were written",
                        None if np.all(words[:, 2].view(np.float64) != 0.0) else "a record of weight 0 was sent")
            if why is None and len(words) > 100:      # control: a routing that is not stable inside a destination does not pass
                c_bad, w_bad = SC.route(twords, own, R, unstable=True)
                if not ((w_bad != words).any() and np.array_equal(c_bad, counts)):
                    why = "control: an unstable routing of the twin's records equals the send buffer"
            if R == 3 and why is None and np.bincount(own, minlength=3).min() * 5 < len(own):
                why = "R = 3: a destination with less than a fifth of the records %r" % np.bincount(own, minlength=3).tolist()
            if R == 255 and why is None and int((counts == 0).sum()) < 200:
                why = "R = 255: only %d destinations with count 0" % int((counts == 0).sum())
            say("%s_r%d_R%d_hash%d" % (tag, r, R, h), why, children=nch, records=len(words), empty_destinations=int((counts == 0).sum()))
            out[(r, R, h)] = (words, counts, own)
            g.close()
    return twins, out


def run_routing_c2(outdir):
    hst, s = c2_setup()
    H, E = _T["H"], _T["sqmc_amd"].SqmcGpuError
    wk = real_population(s)
    prj = (s.prj_counts, s.prj_indices, s.prj_values)
    rows = imp_rows(s, wk)
    n = len(s.imp_up)
    prm = params(tau=s.tau, e_trial=s.e_trial0, reweight_factor_inv=1.0, min_wt=0.5, always_spawn_cutoff_wt=0.5)
    # the small list: the whole deterministic space (its rows must all be owned) at weights that spawn nothing, and a few stochastic walkers that do
    det = wk["imp_distance"] == 0
    small = take(wk, det)
    small["wt"] = small["wt"] * 0.0 + 1e-9 * np.where(np.arange(int(det.sum())) % 2 == 0, 1.0, -1.0)
    few = take(wk, ~det)
    few = {k: v[:10].copy() for k, v in few.items()}
    few["wt"] = np.where(np.arange(10) % 2 == 0, 3.0, -3.0)
    small = join_sorted(small, few)
    door = c2_ctx(hst, s, None, table=False)
    # ---- refusals first, on the context that then serves as a twin: each returns its documented error and leaves the context usable
    g = c2_ctx(hst, s, None)
    xg, send = dev_buffers(n)
    codes = {}

    def refused(what, fn):
        try:
            fn(); codes[what] = (0, "")
        except E as exc:
            codes[what] = (exc.code, str(exc))
    refused("rows_without_projector", lambda: g.shard_config(0, 1, [0, 1]))
    refused("begin_before_config", lambda: g.shard_begin(prm, xg.data_ptr()))
    g.set_projector(*prj)
    refused("rank_ge_nranks", lambda: g.shard_config(2, 2, rows))
    refused("nranks_0", lambda: g.shard_config(0, 0, rows))
    refused("nranks_256", lambda: g.shard_config(0, 256, rows))
    twice = rows.copy(); twice[5] = twice[4]
    refused("row_twice", lambda: g.shard_config(0, 1, twice))
    for bad in (n, -1):
        out_of_range = rows.copy(); out_of_range[7] = bad
        refused("row_%d" % bad, lambda: g.shard_config(0, 1, out_of_range))
    g_replay = c2_ctx(hst, s, prj, rng_mode=_T["sqmc_amd"].RNG_REPLAY)
    g_replay.shard_config(0, 1, rows); g_replay.upload_walkers(wk)
    refused("begin_in_replay", lambda: g_replay.shard_begin(prm, xg.data_ptr()))
    g_replay.close()
    want = dict(rows_without_projector=-1, begin_before_config=-1, rank_ge_nranks=-1, nranks_0=-1, nranks_256=-1, row_twice=-1, begin_in_replay=-3)
    want["row_%d" % n] = want["row_-1"] = -1
    for what, code in want.items():
        say("refusal_" + what, None if codes[what][0] == code else "returned %r, documented %d" % (codes[what], code), message=codes[what][1])
    abused = g
    made = []

    def make_ctx():
        if not made:
            made.append(1)
            return abused                      # the first twin (the big list) runs on the context that was refused nine times
        return c2_ctx(hst, s, prj)
    twins, _ = routing_cases("c2", make_ctx, prm, wk, small, rows, n, door)
    # the refused context against a fresh one: the same records
    gf = c2_ctx(hst, s, prj)
    nch, counts, words, untouched, keep = pack_one(gf, prm, wk, 0, 1, rows, 0, n)
    say("refusals_leave_the_context_usable", None if (nch == twins["big"][1] and np.array_equal(words, twins["big"][2])) else "the refused context packs other records than a fresh one", records=len(words))
    gf.close()
    for t in twins.values():
        t[0].close()
    door.close()


def run_routing_heg57(outdir):
    """the electron gas of 57 plane waves: sort keys of 56 bits, keys and walker indices in two arrays (pack == 0) in k_child_owner /
    get_key; a plain walk (semistochastic = 0, no projector).  The twin finishes its step so that sqmc_gpu_last_tail can say
    that the keys were not packed."""
    H = _T["H"]
    hst = H.HegHost(3, 1.0, 14, 7, 2.3)
    assert hst.norb == 57
    cu, cd = hst.connected(hst.hf_up, hst.hf_dn)
    n = min(3000, len(cu))
    i = np.arange(n)
    big = walkers(cu[:n], cd[:n], np.where(i % 2 == 0, 1.0, -1.0) * (3.0 + (i % 5)), 1, 2)
    small = {k: v[:8].copy() for k, v in big.items()}
    small["wt"] = np.where(np.arange(8) % 2 == 0, 3.0, -3.0)
    prm = params(tau=0.01, e_trial=58.0, reweight_factor_inv=1.0, min_wt=0.5, always_spawn_cutoff_wt=0.5, semistochastic=0)

    def make_ctx():
        g = hst.gpu(rng_mode=H.RNG_COUNTER, seed=SEED, mwalk=MWALK)
        g.set_ct_table(np.array([hst.hf_up], np.uint64), np.array([hst.hf_dn], np.uint64), np.array([1.0]), np.array([1.0]))
        return g
    door = make_ctx()
    twins, _ = routing_cases("heg57", make_ctx, prm, big, small, [], 0, door)
    g, nch, words, keep = twins["big"]
    recv = to_dev(words)
    out = g.shard_finish(prm, recv.data_ptr(), len(words))
    tail = g.last_tail()
    say("heg57_keys_are_not_packed", first(None if not tail["packed"] else "last_tail reports packed keys", None if int(out[7]) == n + len(words) else "nwalk_before_merge %r" % out[7]), tail=tail)
    for t in twins.values():
        t[0].close()
    door.close()


def run_routing_heatbath(outdir):
    """fast_heatbath on the 10-electron C2: a child holds two walker slots, each routed by its own determinant.  To tell which two
    records are one child's, the parents are random determinants with |w| = 1 (one child each); a record within a double
    excitation of exactly one parent is that parent's, and a parent with two such records has one child with both slots filled."""
    H = _T["H"]
    hst = H.ChemHost(FCIDUMP, 10, 5, "d2h")
    rs = np.random.RandomState(20)
    norb = hst.norb

    def rand_dets(m):
        return np.array([sum(1 << int(o) for o in rs.choice(norb, 5, replace=False)) for _ in range(m)], np.uint64)
    pu, pd = rand_dets(9000), rand_dets(9000)
    o = np.lexsort((pd, pu))
    pu, pd = pu[o], pd[o]
    new = np.ones(len(pu), bool); new[1:] = (pu[1:] != pu[:-1]) | (pd[1:] != pd[:-1])
    pu, pd = pu[new], pd[new]
    n = len(pu)
    big = walkers(pu, pd, np.where(np.arange(n) % 2 == 0, 1.0, -1.0), 1, 2)
    small = {k: v[:8].copy() for k, v in big.items()}
    small["wt"] = np.where(np.arange(8) % 2 == 0, 3.0, -3.0)
    prm = params(tau=0.005, e_trial=-75.6, reweight_factor_inv=1.0, min_wt=0.5, always_spawn_cutoff_wt=0.5, semistochastic=0)

    def make_ctx():
        g = hst.gpu(rng_mode=H.RNG_COUNTER, seed=SEED, mwalk=MWALK)
        assert g.setup_efficient_heatbath()
        g.set_ct_table(np.array([hst.hf_up], np.uint64), np.array([hst.hf_dn], np.uint64), np.array([1.0]), np.array([1.0]))
        return g
    door = hst.gpu(rng_mode=H.RNG_COUNTER, seed=SEED, mwalk=0)
    twins, got = routing_cases("heatbath", make_ctx, prm, big, small, [], 0, door)
    g, nch, words, keep = twins["big"]
    why = None if (nch == n and 0 < len(words) <= 2 * nch) else "%d children of %d parents, %d records" % (nch, n, len(words))
    # whose child is every record
    parent = np.full(len(words), -1, np.int64)
    for a in range(0, len(words), 256):
        ru, rd = words[a:a + 256, 0], words[a:a + 256, 1]
        dist = np.bitwise_count(ru[:, None] ^ pu[None, :]).astype(np.int32) + np.bitwise_count(rd[:, None] ^ pd[None, :])
        near = dist <= 4                                         # a single or a double excitation: 2 or 4 bits
        one = near.sum(axis=1) == 1
        parent[a:a + 256] = np.where(one, near.argmax(axis=1), -1)
    ids, cnt = np.unique(parent[parent >= 0], return_counts=True)
    both = ids[cnt == 2]
    split = {}
    for h in (0, 1):
        own = got[(2, 3, h)][2]
        split[h] = sum(1 for p in both if len(set(own[parent == p].tolist())) == 2)
        if why is None and split[h] < 1:
            why = "hash %d: no child of %d with both slots filled has them on different destinations" % (h, len(both))
    say("heatbath_two_slots_two_destinations", why, children=nch, records=len(words), identified=int((parent >= 0).sum()), children_with_both_slots=len(both), split=split)
    for t in twins.values():
        t[0].close()
    door.close()


# ================================================================================================ finish on received records
def is_dyadic(ws):
    return all(abs(w) < 2.0 ** 20 and w * 2.0 ** 20 == math.floor(w * 2.0 ** 20) for w in (float(x) for x in ws))


def finish_records(s, mid, n_recv, seed):
    """received records with integer weights of magnitude 4 .. 16 (built with shard_checker.encode, in a shuffled arrival order):
    runs of 1, 2, 5 and 70 on determinants no resident holds (some cancel to exactly zero), runs on deterministic residents
    (sources of imp_distance -1 among them), at most one record on any stochastic resident, records on the smallest and the
    largest resident, before the first and behind the last"""
    rs = np.random.RandomState(seed)
    res = keyset(mid["up"], mid["dn"])
    n0 = len(mid["up"])
    det_ix = np.nonzero(mid["imp_distance"] == 0)[0].tolist()
    sto_ix = np.nonzero(mid["imp_distance"] != 0)[0].tolist()
    recs = []
    W = lambda: float(rs.randint(4, 17)) * float(rs.choice([-1.0, 1.0]))
    flag = lambda: (int(rs.choice([-1, 1, 2, 3])), int(rs.randint(0, 2)))
    if n_recv == 0:
        return np.zeros((0, 4), np.uint64)
    free = [(int(a), int(b)) for a, b in zip(s.ct_up, s.ct_dn) if (int(a), int(b)) not in res]
    if n0:
        lo, hi = (int(mid["up"][0]), int(mid["dn"][0])), (int(mid["up"][-1]), int(mid["dn"][-1]))
        below, above = [k for k in free if k < lo], [k for k in free if k > hi]
        inside = [k for k in free if lo < k < hi]
    else:
        below, above, inside = [], [], free
    if n_recv == 1:
        k = inside[len(inside) // 2]
        return np.array([SC.encode(k[0], k[1], 8.0, 2, 1)], np.uint64)
    used_sto = set()
    if n0 and n_recv > 100:
        assert below and above, "no free determinant before the first resident or behind the last"
        for k in (below[0], below[-1], above[0], above[-1]):
            for _ in range(3):
                recs.append(SC.encode(k[0], k[1], W(), *flag()))
        for i in (0, n0 - 1):                                      # the smallest and the largest resident
            if i in sto_ix:
                used_sto.add(i); recs.append(SC.encode(mid["up"][i], mid["dn"][i], W(), 2, 1))
            else:
                for _ in range(3):
                    recs.append(SC.encode(mid["up"][i], mid["dn"][i], W(), *flag()))
        for i in det_ix[3:len(det_ix):5]:                          # runs on deterministic residents
            for _ in range(int(rs.randint(2, 6))):
                recs.append(SC.encode(mid["up"][i], mid["dn"][i], W(), *flag()))
        for i in sto_ix[2:len(sto_ix):3]:                          # one record on a stochastic resident: one addition, order-free
            if i not in used_sto:
                used_sto.add(i); recs.append(SC.encode(mid["up"][i], mid["dn"][i], W(), *flag()))
    pool = inside[7::max(1, len(inside) // 900)]
    lens, q = (1, 2, 5, 1, 2, 70, 5, 2, 1), 0
    while len(recs) < n_recv and q < len(pool):
        L = min(lens[q % len(lens)], n_recv - len(recs))
        k = pool[q]
        if q % 2 == 1 and L > 1:                                   # a run that cancels to exactly zero (every length gets its turn: the cycle of lengths is odd)
            ws = ([8.0, -4.0, -4.0] if L % 2 else []) + [4.0, -4.0] * ((L - 3 * (L % 2)) // 2)
        else:
            ws = [W() for _ in range(L)]
        for w in ws[:L]:
            recs.append(SC.encode(k[0], k[1], w, *flag()))
        q += 1
    assert len(recs) == n_recv, (len(recs), n_recv)
    order = rs.permutation(len(recs))
    return np.array([recs[i] for i in order], np.uint64)


def finish_compare(tag, g, prm, mid, words, nch, ct, want_kind):
    spawns = SC.records_to_spawns(words)
    res = dict(up=mid["up"], dn=mid["dn"], wt=mid["wt"], imp_distance=mid["imp_distance"], initiator=mid["initiator"], perm_sign=np.zeros(len(mid["up"]), np.int8))
    try:
        m = AC.fold(res, spawns, prm, exact=False)
    except AC.NeedsDraw as exc:
        say(tag, "the case is not RNG-free: %s" % exc)
        return
    recv = to_dev(words)
    out = g.shard_finish(prm, recv.data_ptr(), len(words))
    got = g.download_walkers()
    tail = g.last_tail()
    why = None if tail["kind"] == want_kind else "tail %r, this case is written for %r" % (tail["kind"], want_kind)
    if why is None and len(got["up"]) != len(m["up"]):
        why = "length %d, model %d" % (len(got["up"]), len(m["up"]))
    if why is None:
        for k in ("up", "dn", "imp_distance", "initiator"):
            if not np.array_equal(got[k], m[k]):
                i = int(np.nonzero(got[k] != m[k])[0][0])
                why = "%s differs first at %d: %r, model %r" % (k, i, got[k][i], m[k][i]); break
    why = first(why, SC.compare_bits("weights", got["wt"], m["wt"]) if why is None else None)
    st, spread = AC.sums(m, prm, ct, m["n_before"], m["w_abs_before"])
    st[15] = float(nch)
    dyadic = is_dyadic(list(mid["wt"]) + list(spawns["wt"]))
    n1, nb = len(m["wt"]), m["n_before"]
    bound = {k: 0.0 for k in range(16)}
    if not dyadic:      # sums of weights that carry the death/clone factor: any order of n additions, proposal_checker.rounding_bound
        bound.update({0: PC.rounding_bound(n1, st[1]), 1: PC.rounding_bound(n1, st[1]), 8: PC.rounding_bound(n1, st[8]), 14: PC.rounding_bound(nb, st[14])})
    for k in AC.TABLE_STATS:
        bound[k] = PC.rounding_bound(*spread[k])
    if len(words) == 0 and len(mid["up"]) == 0:
        st = np.zeros(16); bound = {k: 0.0 for k in range(16)}      # an empty shard that receives nothing: all 16 entries are 0
    if why is None:
        for k in range(16):
            if not abs(out[k] - st[k]) <= bound[k]:
                why = "out_stats[%d] (%s) = %r, model %r, bound %r" % (k, AC.STAT_NAMES[k], out[k], st[k], bound[k]); break
    why = first(why, SC.conservation(mid, words, out) if (len(words) or len(mid["up"])) else None)
    say(tag, why, tail=tail, n0=len(mid["up"]), n_recv=len(words), nwalk=len(got["up"]), discarded=len(m["discarded"]), dyadic=dyadic)


def run_finish(outdir, variant):
    """R = 3 by hand: rank 0 owns the odd rows of the seam projector (dyadic mid-step weights) and about 600 stochastic residents,
    rank 2 owns nothing at all.  The bucket tail is eligible on the first step with SQMC_BUCKET_HOLDOFF=0 once the list holds 64
    residents and something arrives; without arrivals (nall == n0) and on the empty rank the library takes the radix tail."""
    hst, s = c2_setup()
    H = _T["H"]
    prj, rows, hubs, det = seam_setting(s)
    prm = params()
    n = NSEAM
    ct = {(int(a), int(b)): (float(x), float(y)) for a, b, x, y in zip(s.ct_up, s.ct_dn, s.ct_num, s.ct_den)}
    mine = np.arange(n) % 2 == 1
    rows_0 = np.nonzero(mine)[0]
    xu, xd = ct_outside(s, keyset(det["up"], det["dn"]), np.linspace(9000, len(s.ct_up) - 9000, 600).astype(np.int64))
    k = np.arange(len(xu))
    sto = walkers(xu, xd, np.where(k % 2 == 0, 1.0, -1.0) * (1.0 + (k % 9) / 4.0), 1 + k % 3, np.where(k % 3 == 2, 1, 2))
    wk0 = join_sorted(take(det, mine), sto)
    for n_recv in (0, 1, 1500):
        g = c2_ctx(hst, s, prj, seed=H.rank_seed(SEED, 0))
        g.shard_config(0, 3, rows_0)
        g.upload_walkers(wk0)
        xg, send = dev_buffers(n)
        nch = g.shard_begin(prm, xg.data_ptr())
        write_x(xg, det["wt"])                                      # the all-reduced vector: every rank's rows
        g.shard_pack(prm, xg.data_ptr(), send.data_ptr(), CAP, 3)
        mid = g.download_walkers()
        sel = mid["imp_distance"] == 0
        want = np.array([float(q) for q in SC.project(rows, det["wt"], E_TRIAL, TAU, exact=True, only=rows_0)])
        assert SC.compare_bits("mid-step deterministic weights", mid["wt"][sel], want) is None and len(mid["up"]) == len(wk0["up"]) >= 256
        words = finish_records(s, mid, n_recv, 100 + n_recv)
        kind = "bucket" if (variant == "bucket" and n_recv > 0) else "radix"
        finish_compare("finish_%s_rank0_recv%d" % (variant, n_recv), g, prm, mid, words, nch, ct, kind)
        g.close()
    empty = walkers(np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0), 1, 1)
    for n_recv in (0, 40):
        g = c2_ctx(hst, s, prj, seed=H.rank_seed(SEED, 2))
        g.shard_config(2, 3, [])
        g.upload_walkers(empty)
        xg, send = dev_buffers(n)
        nch = g.shard_begin(prm, xg.data_ptr())
        x_r = read_x(xg, n)
        write_x(xg, det["wt"])
        counts = g.shard_pack(prm, xg.data_ptr(), send.data_ptr(), CAP, 3)
        mid = g.download_walkers()
        assert nch == 0 and int(counts.sum()) == 0 and len(mid["up"]) == 0 and not np.any(x_r)
        words = finish_records(s, mid, n_recv, 7)
        finish_compare("finish_%s_empty_rank_recv%d" % (variant, n_recv), g, prm, mid, words, nch, ct, "radix")
        g.close()


# ================================================================================================ the natural step
def run_natural(outdir):
    """begin on every rank, the sum of the R vectors, pack, every bucket delivered to its destination in rank order then sender's
    order, finish: what went into a rank's finish is what its sums report (conservation), every record sits in the bucket of its
    determinant's owner (R = 2: the det_owner door on hash 0; R = 3: owner_djb on hash 1), no determinant ends on two ranks, every
    walker ends on its owner, and entries 0..6 summed over the ranks are the sums of the union of the final lists
    (anneal_checker.sums; bound: rounding_bound(n, sum |terms|) for the order of the additions, twice: per rank and across)."""
    hst, s = c2_setup()
    H = _T["H"]
    wk = real_population(s)
    prj = (s.prj_counts, s.prj_indices, s.prj_values)
    n = len(s.imp_up)
    prm = params(tau=s.tau, e_trial=s.e_trial0, reweight_factor_inv=1.0, min_wt=0.5, always_spawn_cutoff_wt=0.5)
    ct = {(int(a), int(b)): (float(x), float(y)) for a, b, x, y in zip(s.ct_up, s.ct_dn, s.ct_num, s.ct_den)}
    psign = {(int(a), int(b)): int(p) for a, b, p in zip(wk["up"], wk["dn"], wk["perm_sign"]) if p}
    for R, h in ((2, 0), (3, 1)):
        door = c2_ctx(hst, s, None, table=False)
        door.set_owner_hash(h)
        own_fn = (lambda u, d: np.array([SC.owner_djb(int(a), int(b), R) for a, b in zip(u, d)], np.int64)) if h == 1 else (lambda u, d: door.det_owner(u, d, R).astype(np.int64))
        owners = own_fn(wk["up"], wk["dn"])
        ranks = []
        for r in range(R):
            g = c2_ctx(hst, s, prj, seed=H.rank_seed(SEED, r))
            g.set_owner_hash(h)
            wk0 = take(wk, owners == r)
            rows_r = imp_rows(s, wk0)
            g.shard_config(r, R, rows_r)
            g.upload_walkers(wk0)
            xg, send = dev_buffers(n)
            nch = g.shard_begin(prm, xg.data_ptr())
            ranks.append(dict(g=g, xg=xg, send=send, x=read_x(xg, n), nch=nch, n0=len(wk0["up"])))
        xsum = np.sum([t["x"] for t in ranks], axis=0)
        why = None
        for r, t in enumerate(ranks):
            write_x(t["xg"], xsum)
            t["counts"] = t["g"].shard_pack(prm, t["xg"].data_ptr(), t["send"].data_ptr(), CAP, R)
            t["words"], untouched = read_send(t["send"], t["counts"])
            t["mid"] = t["g"].download_walkers()
            dest = np.repeat(np.arange(R), t["counts"])
            own = own_fn(t["words"][:, 0], t["words"][:, 1])
            why = first(why, None if untouched else "rank %d wrote behind its records" % r,
                        None if np.array_equal(own, dest) else "rank %d: %d records sit in another bucket than their owner's" % (r, int((own != dest).sum())))
        say("natural_R%d_every_record_goes_to_its_owner" % R, why, sent=[int(t["counts"].sum()) for t in ranks])
        union = {k: [] for k in ("up", "dn", "wt", "imp_distance", "initiator")}
        total = np.zeros(7)
        for q, t in enumerate(ranks):
            parts = []
            for p_ in ranks:                                       # rank order, then the sender's order
                off = int(p_["counts"][:q].sum())
                parts.append(p_["words"][off:off + int(p_["counts"][q])])
            recv_words = np.concatenate(parts) if parts else np.zeros((0, 4), np.uint64)
            recv = to_dev(recv_words)
            out = t["g"].shard_finish(prm, recv.data_ptr(), len(recv_words))
            fin = t["g"].download_walkers()
            o2 = own_fn(fin["up"], fin["dn"])
            why = first(SC.conservation(t["mid"], recv_words, out), None if np.all(o2 == q) else "a walker of rank %d belongs to another rank" % q,
                        None if int(out[5]) == len(fin["up"]) else "nwalk %r, list %d" % (out[5], len(fin["up"])),
                        None if int(out[15]) == t["nch"] else "out_stats[15] %r, children %d" % (out[15], t["nch"]))
            say("natural_R%d_rank%d_finish" % (R, q), why, n0=t["n0"], n_recv=len(recv_words), nwalk=len(fin["up"]), tail=t["g"].last_tail()["kind"])
            for k in union:
                union[k].append(fin[k])
            total += out[:7]
        u = {k: np.concatenate(v) for k, v in union.items()}
        o = np.lexsort((u["dn"], u["up"]))
        u = {k: v[o] for k, v in u.items()}
        keys = list(zip(u["up"].tolist(), u["dn"].tolist()))
        why = None if len(set(keys)) == len(keys) else "%d determinants are on two ranks" % (len(keys) - len(set(keys)))
        u["perm_sign"] = np.array([psign.get(k, 0) if i == 3 else 0 for k, i in zip(keys, u["initiator"])], np.int8)
        st, spread = AC.sums(u, prm, ct)
        nn = len(keys)
        bound = {0: PC.rounding_bound(nn, st[1]), 1: PC.rounding_bound(nn, st[1]), 4: PC.rounding_bound(nn, abs(st[4])), 5: 0.0, 6: PC.rounding_bound(nn, st[6]),
                 2: PC.rounding_bound(*spread[2]), 3: PC.rounding_bound(*spread[3])}
        if why is None:
            for k in range(7):
                if not abs(total[k] - st[k]) <= 2 * bound[k]:
                    why = "entry %d (%s) summed over ranks = %r, of the union of the lists %r, bound %r" % (k, AC.STAT_NAMES[k], total[k], st[k], 2 * bound[k]); break
        say("natural_R%d_union" % R, why, nwalk=nn, sums=total.tolist())
        for t in ranks:
            t["g"].close()
        door.close()


def main(argv):
    mode, outdir = argv[1], argv[2]
    for k, v in ENV[mode].items():
        assert os.environ.get(k) == v, "the environment of this process does not select %s" % mode
    import torch
    import sqmc_amd
    from sqmc_amd import host as H
    sqmc_amd.set_device(0)
    _T.update(torch=torch, sqmc_amd=sqmc_amd, H=H, dev=torch.device("cuda", 0))
    t0 = time.time()
    try:
        if mode.startswith("projection"):
            run_projection(outdir)
        elif mode.startswith("finish_"):
            run_finish(outdir, mode.split("_", 1)[1])
        else:
            globals()["run_" + mode](outdir)
    except sqmc_amd.SqmcGpuError as exc:
        print(json.dumps(dict(mode=mode, library_error=exc.code, message=str(exc))), flush=True)
        return 3
    print(json.dumps(dict(mode=mode, failed=_N["bad"], seconds=round(time.time() - t0, 2))), flush=True)
    return 1 if _N["bad"] else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
