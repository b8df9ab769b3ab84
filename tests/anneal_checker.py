"""An independent model of the annihilation step and the sums that follow it, CPU only.

Written from the reference's text -- merge_original_with_spawned2 with its initiator rules (do_walk.f90:5866-6083),
reduce_my_walker (7196-7254), the reweighting (2487) and the sums of a generation (2573-2790 with binary_search_list_and_update,
more_tools.f90:4041-4098) -- and from nothing under oracle/.  It shares no data structure with that restatement: there is no
sort of the records and no in-place compaction by a running shift.  Records are grouped by determinant in a dict that keeps
their arrival order (residents first, then the spawns in creation order: the order the reference's stable sort leaves inside a
run of equal determinants), every group is folded by the reference's rules, and the groups are emitted in (up, dn) order.

Two arithmetics: `exact=True` adds weights as fractions.Fraction (any order gives the same sum; what the dyadic GPU cases
use), `exact=False` adds doubles one after the other as the reference's loop does (bit-comparable with any faithful
restatement on arbitrary weights).  The sums of a generation are math.fsum's, correctly rounded.

A step with semistochastic = f (`params["semistochastic"] == 0`) takes the same fold -- reduce_my_walker is not called, so no
rounding draw is ever asked for -- then join_walker2 (6990-7103) over the merged list, which drops every zero weight, then the
reweighting: plain_step.  Its draws come from the caller, draw(index of the later walker in the merged list); chain_layer states
what holds of the result for any draws.

What the model leaves to the caller: the stochastic rounding of reduce_my_walker needs a random number per small weight; pass
`draw(up, dn)`, or none -- then an input that would need one raises NeedsDraw (the RNG-free cases assert exactly that).
"""
import math
from fractions import Fraction

import numpy as np

STAT_NAMES = ("w_gen", "w_abs_gen", "e_den_gen", "e_num_gen", "w_perm_initiator_gen", "nwalk", "w_abs_gen_imp", "nwalk_before_merge",
              "w2_gen", "e_num2", "e_den2", "e_num_abs", "e_den_abs", "e_num_e_den", "w_abs_before_merge", "n_proposals")
EXACT_STATS = (0, 1, 4, 5, 6, 7, 8, 14, 15)          # sums of the weights alone: exact for dyadic weights
TABLE_STATS = (2, 3, 9, 10, 11, 12, 13)             # sums that carry the C(T) table's numbers


class NeedsDraw(AssertionError):
    """an input of an RNG-free case would consume a rounding draw"""


def default_params(**kw):
    p = dict(tau=0.01, e_trial=-75.7, reweight_factor_inv=1.0, r_initiator=1.0, min_wt=0.25, always_spawn_cutoff_wt=0.25,
             initiator_power=0, initiator_min_distance=0, c_t_initiator=0, semistochastic=1, reached_w_abs_gen=2)
    p.update(kw)
    return p


def _records(residents, spawns):
    """(up, dn, wt, imp_distance, initiator, perm_sign) in arrival order; a spawn of weight 0 is no walker (do_walk.f90:3676)"""
    col = lambda d, k: np.asarray(d[k]).tolist()
    n0 = len(residents["up"])
    ps = col(residents, "perm_sign") if residents.get("perm_sign") is not None else [0] * n0
    out = [(int(u), int(d), float(w), int(a), int(b), int(s)) for u, d, w, a, b, s in
           zip(col(residents, "up"), col(residents, "dn"), col(residents, "wt"), col(residents, "imp_distance"), col(residents, "initiator"), ps)]
    out += [(int(u), int(d), float(w), int(a), int(b), 0) for u, d, w, a, b in
            zip(col(spawns, "up"), col(spawns, "dn"), col(spawns, "wt"), col(spawns, "imp_distance"), col(spawns, "initiator")) if w != 0.0]
    return out


def _imp_rule(t, s):
    """5906-5916 = 5927-5937"""
    if t == -2:
        return 0 if s == 0 else t
    if s == -2:
        return -2 if t != 0 else t
    if t != 0:
        return min(t, abs(s))
    return t


def _threshold(imp, p):
    return p["r_initiator"] * (max(0, imp - p["initiator_min_distance"]) ** p["initiator_power"])


def fold(residents, spawns, params, exact=True, draw=None, no_exception=False, order_blind=False):
    """The merged list and everything the invariants and the sums need.

    residents: dict of arrays up, dn, wt, imp_distance, initiator, perm_sign (sorted by (up, dn), unique); spawns: dict of arrays
    up, dn, wt, imp_distance, initiator in creation order.  Returns dict(up, dn, wt, imp_distance, initiator: the new list;
    n_before, w_abs_before; discarded: the determinants 5970 / 6038 dropped; reset: permanent initiators whose weight 5954 /
    5995 replaced; rounded: determinants whose weight reduce_my_walker drew for).
    no_exception / order_blind: two deliberate mistakes, for showing that the twin test notices them."""
    p = params
    plain = not p.get("semistochastic", 1)
    num = Fraction if exact else float
    recs = _records(residents, spawns)
    groups = {}
    for r in recs:
        groups.setdefault((r[0], r[1]), []).append(r)
    keys = sorted(groups)
    r_init = p["r_initiator"]
    cti = bool(p["c_t_initiator"])
    out = dict(up=[], dn=[], wt=[], imp_distance=[], initiator=[])
    discarded, reset, rounded = [], [], []
    for pos, key in enumerate(keys):
        g = groups[key]
        if order_blind:
            g = sorted(g, key=lambda r: (r[2], r[3], r[4]))
        first, last = pos == 0, pos == len(keys) - 1
        _, _, w0, imp, init, psign = g[0]
        wt = num(w0)
        if imp == -1 and not first:          # 5985-5988: every first record of a run but the list's own first one arrives by the copy
            imp = 1
        for (_, _, ws, imp_s, init_s, ps_s) in g[1:]:
            ws = num(ws)
            if psign == 0 and ps_s != 0:
                psign = ps_s
            if ws * wt > 0:                  # 5898
                init = max(init, init_s)
                imp = _imp_rule(imp, imp_s)
            else:
                imp = _imp_rule(imp, imp_s)
                if abs(wt) < abs(ws):        # 5939
                    if init != 3 or r_init == -1.0:
                        init = init_s
                elif abs(wt) == abs(ws):     # 5943
                    if init != 3 or r_init == -1.0:
                        init = 0
            if no_exception or not (imp == 0 and imp_s == -1):      # 5950
                wt = wt + ws
        # the run is complete: 5952-5968 = 5993-6029
        if init == 3 and r_init >= 0:
            assert psign in (1, -1), "a permanent initiator needs its sign"
            if wt * psign < 1:
                wt = num(psign)
                reset.append(key)
        elif init == 2 and ((abs(wt) <= _threshold(imp, p) and imp > 0) or ((abs(wt) <= r_init and not cti) and imp == -2)):
            init = 1
        elif init < 2 and ((abs(wt) > _threshold(imp, p) and imp >= 0) or ((abs(wt) > r_init or cti) and imp == -2)):
            init += 1
        if last and imp == -1:               # 6032-6036 come in front of the last run's test 6038 ...
            imp = 1
        drop = ((wt == 0 and (init != 3 or r_init < 0)) or init == 0) and imp >= 1      # 5970 / 6038
        if imp == -1:                        # ... and behind every other run's 5970
            imp = 1
        if drop:
            discarded.append(key)
            continue
        if plain:                            # semistochastic = f: join_walker2 (2475) and the reweighting come behind the whole list, in plain_step
            assert not exact or Fraction(float(wt)) == wt, "a weight of an exact case is a double"
        else:
            # reduce_my_walker, 7222-7249
            if imp >= 1 and abs(wt) < p["min_wt"]:
                if wt != 0:
                    if draw is None:
                        raise NeedsDraw("determinant %r: |w| = %r < min_wt = %r" % (key, float(abs(wt)), p["min_wt"]))
                    rounded.append(key)
                    wt = num(math.copysign(p["min_wt"], wt)) if draw(key[0], key[1]) < float(abs(wt)) / p["min_wt"] else num(0)
                if wt == 0:
                    continue
            wt = wt * num(p["reweight_factor_inv"])      # 2487
        out["up"].append(key[0]); out["dn"].append(key[1]); out["wt"].append(float(wt))
        out["imp_distance"].append(imp); out["initiator"].append(init)
    res = dict(up=np.array(out["up"], np.uint64), dn=np.array(out["dn"], np.uint64), wt=np.array(out["wt"], np.float64),
               imp_distance=np.array(out["imp_distance"], np.int8), initiator=np.array(out["initiator"], np.int8))
    res["n_before"] = len(recs)
    res["w_abs_before"] = math.fsum(abs(r[2]) for r in recs)      # 2342
    res["discarded"], res["reset"], res["rounded"] = discarded, reset, rounded
    signs = {}
    for r in recs:
        if r[5]:
            signs[(r[0], r[1])] = r[5]
    res["perm_sign"] = np.array([signs.get((int(u), int(d)), 0) if i == 3 else 0 for u, d, i in zip(res["up"], res["dn"], res["initiator"])], np.int8)
    return res


# ------------------------------------------------------------------------------------------------ semistochastic = f: the joins
def join_walker2(wt, initiator, min_wt, draw, exact=True, close_at_ge=False, carrier_inverted=False, perm_initiator_joins=False):
    """join_walker2 (do_walk.f90:6990-7069) on a merged list, before its zeros are dropped: the positive pass, then the negative
    one.  A candidate has the pass's sign, |wt| < min_wt (strict) and initiator < 3.  The first candidate opens a chain; each later
    one is joined to the chain's carrier: wttot = |w_i| + |w_carrier|, and if draw(i) > |w_i| / wttot the earlier walker keeps
    wttot, otherwise the later one takes it; the chain closes when wttot > min_wt (strict).  draw(i): the random number of the
    join whose later walker has index i (0-based) in this list.

    Returns (weights, chains, joins): chains[+1 / -1] = [(member indices, exact total, closed)] in list order -- where a chain
    begins and ends depends on the running sums alone, not on the draws.
    close_at_ge / carrier_inverted / perm_initiator_joins: three deliberate mistakes."""
    num = Fraction if exact else float
    w = [num(float(x)) for x in wt]
    chains, joins = {1: [], -1: []}, 0
    for sign in (1, -1):
        carrier, members, total = None, [], num(0)
        for i in range(len(w)):
            wi = w[i]
            if not ((wi > 0 if sign > 0 else wi < 0) and abs(wi) < min_wt and (int(initiator[i]) < 3 or perm_initiator_joins)):
                continue
            if carrier is None:                               # 7007-7009
                carrier, members, total = i, [i], abs(wi)
                continue
            wttot = abs(wi) + abs(w[carrier])                 # 7011
            joins += 1
            earlier_keeps = draw(i) > float(abs(wi)) / float(wttot)      # 7012
            if carrier_inverted:
                earlier_keeps = not earlier_keeps
            if earlier_keeps:
                w[carrier] = wttot if w[carrier] > 0 else -wttot; w[i] = num(0)
            else:
                w[i] = wttot if wi > 0 else -wttot; w[carrier] = num(0); carrier = i
            members.append(i); total = wttot
            if (wttot >= min_wt) if close_at_ge else (wttot > min_wt):   # 7030
                chains[sign].append((members, total, True)); carrier = None
        if carrier is not None:
            chains[sign].append((members, total, False))
    return w, chains, joins


def plain_step(residents, spawns, params, draw, exact=True, **mistakes):
    """What a step with semistochastic = f leaves of a list (do_walk.f90:2373-2487): merge_original_with_spawned2, join_walker2,
    every zero weight dropped -- the deterministic space included (7075) -- then the reweighting.  Returns fold()'s dict for the
    new list, plus heads (the merged list the joins saw: up, dn, wt, imp_distance, initiator), chains, joins."""
    assert not params["semistochastic"]
    m = fold(residents, spawns, params, exact=exact)
    w, chains, joins = join_walker2(m["wt"], m["initiator"], params["min_wt"], draw, exact=exact, **mistakes)
    keep = np.array([i for i in range(len(w)) if w[i] != 0], np.int64)   # 7071-7092
    rfi = (Fraction if exact else float)(params["reweight_factor_inv"])
    out = dict(m)
    out["heads"] = {k: m[k] for k in ("up", "dn", "wt", "imp_distance", "initiator")}
    for k in ("up", "dn", "imp_distance", "initiator", "perm_sign"):
        out[k] = m[k][keep]
    out["wt"] = np.array([float(w[i] * rfi) for i in keep], np.float64)  # 2487
    out["chains"], out["joins"] = chains, joins
    return out


def chain_layer(heads, chains, params, got):
    """The statements about an output list `got` (up, dn, wt, imp_distance, initiator) that hold for ANY draws: every non-member
    of a chain is unchanged (dropped if its weight is zero); a chain of one is untouched; a chain of two or more leaves exactly
    one survivor, one of its members, with that member's flags and weight sign x total (x reweight_factor_inv).  Returns a list
    of violations."""
    bad = []
    rfi = Fraction(params["reweight_factor_inv"])
    have = {(int(u), int(d)): (float(w), int(a), int(b)) for u, d, w, a, b in zip(got["up"], got["dn"], got["wt"], got["imp_distance"], got["initiator"])}
    if len(have) != len(got["up"]):
        bad.append(("a determinant twice",))
    key = lambda i: (int(heads["up"][i]), int(heads["dn"][i]))
    flags = lambda i: (int(heads["imp_distance"][i]), int(heads["initiator"][i]))
    member = set()
    for sign in (1, -1):
        for mem, total, closed in chains[sign]:
            member.update(mem)
            if len(mem) == 1:
                i = mem[0]
                if have.pop(key(i), None) != (float(Fraction(float(heads["wt"][i])) * rfi),) + flags(i):
                    bad.append(("chain of one changed", i))
                continue
            alive = [(i, have.pop(key(i))) for i in mem if key(i) in have]
            if len(alive) != 1:
                bad.append(("chain with %d survivors" % len(alive), mem[0], mem[-1])); continue
            i, rec = alive[0]
            if rec != (float(sign * Fraction(total) * rfi),) + flags(i):
                bad.append(("survivor", i, rec, float(sign * Fraction(total) * rfi)))
    for i in range(len(heads["up"])):
        if i in member:
            continue
        w = float(heads["wt"][i])
        rec = have.pop(key(i), None)
        if (rec is not None) if w == 0.0 else (rec != (float(Fraction(w) * rfi),) + flags(i)):
            bad.append(("non-candidate changed", i, rec))
    if have:
        bad.append(("determinants nobody had", sorted(have)[:3]))
    return bad


def check_precondition(residents, spawns, params):
    """What makes a case exact and RNG-free: weights multiples of 0.25 with |w| <= 4, min_wt = cutoff = 0.25, reweight_factor_inv 1 or
    0.5.  Raises AssertionError (NeedsDraw if the fold would consume a draw): a case that breaks it fails, it is not skipped."""
    for w in list(residents["wt"]) + list(spawns["wt"]):
        assert abs(w) <= 4.0 and float(w) * 4.0 == math.floor(float(w) * 4.0), "weight %r is no multiple of 0.25 within [-4, 4]" % w
    assert params["min_wt"] == 0.25 and params["always_spawn_cutoff_wt"] == 0.25, "min_wt and the cutoff are 0.25"
    assert params["reweight_factor_inv"] in (1.0, 0.5), "reweight_factor_inv is 1 or 0.5"
    m = fold(residents, spawns, params, exact=True, draw=None)
    if not params["semistochastic"]:         # a plain step of such a list makes no join either: no head has 0 < |w| < min_wt
        assert not any(0 < abs(float(w)) < params["min_wt"] for w in m["wt"]), "a head below min_wt: the plain step would join it"


def sums(merged, params, ct, n_before=0, w_abs_before=0.0):
    """out_stats[16] of include/sqmc_gpu.h for a finished list (do_walk.f90:2573-2598, 2755-2759): ct maps (up, dn) -> (e_num, e_den).
    Also returns, per table sum, (number of terms, sum of |terms|) for proposal_checker.rounding_bound."""
    wt = [float(x) for x in merged["wt"]]
    ps = merged.get("perm_sign")
    st = [0.0] * 16
    st[0] = math.fsum(wt)
    st[1] = math.fsum(abs(x) for x in wt)
    st[4] = math.fsum(w * int(s) for w, s, i in zip(wt, ps, merged["initiator"]) if i == 3) if ps is not None else 0.0
    st[5] = float(len(wt))
    st[6] = math.fsum(abs(w) for w, d in zip(wt, merged["imp_distance"]) if d == 0 or (d == -2 and params["c_t_initiator"]))
    st[7] = float(n_before)
    st[8] = math.fsum(Fraction(w) ** 2 for w in wt) if wt else 0.0
    st[8] = float(st[8])
    st[14] = float(w_abs_before)
    en_t, ed_t = [], []
    for u, d, w in zip(merged["up"], merged["dn"], wt):
        e = ct.get((int(u), int(d)))
        if e is None:
            continue
        en, ed = e[0] * w, e[1] * w
        if en != 0.0:                        # more_tools.f90:4084
            if abs(ed) < 1e-22:
                ed = abs(ed)
            en_t.append(en); ed_t.append(ed)
    terms = {2: ed_t, 3: en_t, 9: [x * x for x in en_t], 10: [x * x for x in ed_t], 11: [x * math.copysign(1.0, y) for x, y in zip(en_t, ed_t)],
             12: [abs(x) for x in ed_t], 13: [x * y for x, y in zip(en_t, ed_t)]}
    spread = {}
    for k, t in terms.items():
        st[k] = math.fsum(t)
        spread[k] = (len(t), math.fsum(abs(x) for x in t))
    return np.array(st), spread


# ------------------------------------------------------------------------------------------------ rule-free invariants
def invariants(residents, spawns, params, got, discarded=(), reset=(), tol=0.0):
    """Three statements about ANY output list `got` (dict up, dn, wt) that need no initiator rule:
    (a) keys strictly increasing;
    (b) per determinant, the output weight is reweight_factor_inv times the exact sum of its inputs, without the sources of
        imp_distance -1 onto a determinant of the deterministic space (5950), a permanent initiator whose weight was reset (`reset`)
        excepted; tol: 0 for dyadic inputs, else the rounding of a left-to-right sum, relative to sum |w|;
    (c) the output determinants are the inputs that were not discarded (`discarded`, by 5970 / 6038) and whose sum is not zero --
        a zero sum stays only where reduce_my_walker leaves it: imp_distance 0 or -2, and a permanent initiator.
    Returns a list of violations (empty: all three hold)."""
    bad = []
    keys = [(int(u), int(d)) for u, d in zip(got["up"], got["dn"])]
    for a, b in zip(keys, keys[1:]):
        if not a < b:
            bad.append(("a", a, b))
    det_space, stays = set(), set()
    for i in range(len(residents["up"])):
        k = (int(residents["up"][i]), int(residents["dn"][i]))
        if int(residents["imp_distance"][i]) == 0:
            det_space.add(k)
        if int(residents["imp_distance"][i]) in (0, -2):
            stays.add(k)
    total, mass = {}, {}
    for (u, d, w, imp, init, ps) in _records(residents, spawns):
        k = (u, d)
        total.setdefault(k, Fraction(0)); mass.setdefault(k, Fraction(0))
        if imp == -1 and k in det_space:
            continue
        total[k] += Fraction(w); mass[k] += abs(Fraction(w))
    rfi = Fraction(params["reweight_factor_inv"])
    skip = set(reset)
    gone = set(discarded)
    out_w = dict(zip(keys, (float(x) for x in got["wt"])))
    for k, w in out_w.items():
        if k not in total:
            bad.append(("c", k, "not among the inputs")); continue
        if k in skip:
            continue
        if abs(Fraction(w) - total[k] * rfi) > tol * float(mass[k]):
            bad.append(("b", k, w, float(total[k] * rfi)))
    expect = {k for k in total if k not in gone and (total[k] != 0 or k in stays or k in skip)}
    if set(keys) != expect:
        bad.append(("c", sorted(set(keys) - expect)[:5], sorted(expect - set(keys))[:5]))
    return bad


# ------------------------------------------------------------------------------------------------ C(T) from the independent H
def ct_from_h(H, psi_up, psi_dn, psi_c, dets):
    """e_num(i) = sum_j H_ij c_j over Psi_T, e_den(i) = c_i (0 outside Psi_T) for every determinant of `dets`, with the
    second-quantised H of proposal_checker (semistoch.f90:2039-2063).  Returns {(up, dn): (e_num, e_den)} and, per determinant,
    (terms, sum |terms|) of e_num for rounding_bound."""
    c_of = {(int(u), int(d)): float(c) for u, d, c in zip(psi_up, psi_dn, psi_c)}
    ct, spread = {}, {}
    for (u, d) in dets:
        tm = []
        for (ju, jd), c in c_of.items():
            for x in H.terms(ju, jd, u, d):
                tm.append(x * c)
        ct[(u, d)] = (math.fsum(tm), c_of.get((u, d), 0.0))
        spread[(u, d)] = (len(tm), math.fsum(abs(x) for x in tm))
    return ct, spread
