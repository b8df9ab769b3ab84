"""An independent model of the step variant hf_to_psit = .true., CPU only: plain Python with numpy.

Written from the reference's text -- do_walk.f90:1267-1300 (the three segments), 2262-2323 (the projection), 2394-2462 (T^-1, its
transpose and check_initiator over C(T)), 2487, 2590-2598, 2701-2722 (the sums), 3574-3589 and 3676 (the first state neither draws
nor is spawned onto), 3743-3793 (death/clone), 6484-6833 (merge_my_original_with_spawned3), more_tools.f90:3656-3667 -- with the two
stated departures of tests/golden/README_hf_to_psit.md: Q1, the outside segment becomes the ordered union of its survivors and the new
determinants that passed check_initiator; Q2, imp_distance -1 -> 1 once kept.  Nothing here comes from oracle/ or from the kernels.

Everything outside C(T) is folded by anneal_checker.fold: the variant treats those determinants exactly as
merge_original_with_spawned2 + reduce_my_walker do (6590-6693 = 5897-6038; 7196-7254 with i_start behind C(T)).  What is new here:

  head(walkers, tables, params)                      the resident weights in front of the merge
  tail(premerge_weights, flags, spawns, tables, params)      the new list and the 16 sums
  children(walkers, params)                          children per slot for always_spawn_cutoff_wt = 0 (draw-free)

Every long sum (first row over C(T), first row over the Psi_T locations, T^-1) comes in three forms, ordered_sums(): left to right
(sum_order 0, the reference's loop), the documented 64-ary tree (sum_order 1: chunks of 64 consecutive terms left to right, then the
chunk sums, then the block sums), and the exact rational value of the same doubles.  head() and tail() return weights for both
orders, so a caller compares the one it ran bit for bit and holds both against the exact value.

tables: dict(ct_up, ct_dn, ct_num, ct_den: the C(T) list and e_loc_num / e_loc_den; loc_psit: 0-based slots of Psi_T's determinants
in label order; cdet; diag_elems; loc_imp: 0-based slots of the deterministic space; prj_counts, prj_indices (1-based), prj_values:
the deterministic-space matrix, rows of an upper-triangular storage as fast_sparse_matrix_multiply_upper_triangular reads them).

No draws: an input that would need a rounding draw raises anneal_checker.NeedsDraw, unless the caller hands tail() the generator's
draw(up, dn) (the frozen trajectory of tests/golden/psit_c2_8steps.json needs them; no pinned GPU case does).

Deliberate mistakes (keyword switches, for showing that named cases notice them): chunk_off_by_one, drop_last_block,
tinv_from_premerge, discard_ct_zero, cti_checks_all, first_row_enum_raw.
"""
import math
from fractions import Fraction

import numpy as np

import anneal_checker as AC

U = 2.0 ** -53
SUM_NAMES = ("ct_row", "psit_row", "tinv")


# ------------------------------------------------------------------------------------------------ the three forms of a long sum
def exact_sum(terms):
    """the rational value of a list of doubles (big integers over a common power of two)"""
    if not len(terms):
        return Fraction(0)
    me = [math.frexp(float(t)) for t in terms]
    emin = min(e for m, e in me if m != 0.0) - 53 if any(m != 0.0 for m, e in me) else 0
    tot = 0
    for m, e in me:
        if m != 0.0:
            tot += int(math.ldexp(m, 53)) << (e - 53 - emin)
    return Fraction(tot) * Fraction(2) ** emin


def left_to_right(terms):
    s = float(terms[0])
    for t in terms[1:]:
        s = s + t
    return s


def tree64(terms, chunk_off_by_one=False, drop_last_block=False):
    """chunks of 64 consecutive terms left to right (level 1), the 64 chunk sums of a block of 4096 terms left to right (level 2), the
    block sums left to right (level 3).  Returns (sum, longest chain of additions a term goes through)."""
    n = len(terms)
    assert 0 < n <= 64 ** 3
    blocks = []
    for b0 in range(0, n, 4096):
        blk = terms[b0:b0 + 4096]
        chunks = []
        for c0 in range(0, len(blk), 64):
            ch = blk[c0:c0 + 64]
            if chunk_off_by_one and len(ch) < 64:
                ch = ch[:-1]
            chunks.append(left_to_right(ch) if ch else 0.0)
        blocks.append(left_to_right(chunks))
    if drop_last_block and len(blocks) > 1:
        blocks = blocks[:-1]
    nb = (n + 4095) // 4096
    chain = (min(n, 64) - 1) + (min((n + 63) // 64, 64) - 1) + (nb - 1)
    return left_to_right(blocks), chain


def ordered_sums(terms, **mistakes):
    """dict(lr, tree: the two doubles; exact: Fraction; mass: sum |term| as a Fraction; chain: {0, 1: longest chain of additions})"""
    t = [float(x) for x in terms]
    if not t:
        return dict(lr=0.0, tree=0.0, exact=Fraction(0), mass=Fraction(0), chain={0: 0, 1: 0}, n=0)
    tr, chain = tree64(t, **{k: v for k, v in mistakes.items() if k in ("chunk_off_by_one", "drop_last_block")})
    return dict(lr=left_to_right(t), tree=tr, exact=exact_sum(t), mass=exact_sum([abs(x) for x in t]), chain={0: len(t) - 1, 1: chain}, n=len(t))


def within_bound(s):
    """each form lies within K 2^-53 sum|term| of the exact value, K the longest chain of additions of that form: every addition
    rounds its result by at most 2^-53 of it, a partial sum is at most sum|term| (1 + K 2^-53) in magnitude, and a term's share of the
    error is one such rounding per addition it goes through -- at most K of them.  (Second order, K^2 2^-106, is 3e-11 of the bound at
    the longest chain there is, 64^3 - 1, and is covered by the factor 1 + 2^-20.)  Returns {0, 1: |form - exact| / (2^-53 mass)}."""
    out = {}
    for order, name in ((0, "lr"), (1, "tree")):
        err = abs(Fraction(s[name]) - s["exact"])
        assert err <= s["chain"][order] * Fraction(U) * s["mass"] * (1 + Fraction(1, 2 ** 20)), (name, float(err), s["chain"][order], float(s["mass"]))
        out[order] = float(err / (Fraction(U) * s["mass"])) if s["mass"] else 0.0
    return out


def _pick(s, order):
    return s["tree"] if order else s["lr"]


# ------------------------------------------------------------------------------------------------ the gate
def children(walkers, params):
    """number of children per slot, do_walk.f90:3574-3589 with always_spawn_cutoff_wt = 0: no walker is below the cutoff, so every one
    spawns max(nint(|w|), 1) children without a draw; the first state spawns none (3574)"""
    assert params["always_spawn_cutoff_wt"] == 0.0, "a walker below the cutoff takes a gate draw"
    w = np.abs(np.asarray(walkers["wt"], np.float64))
    n = np.maximum(np.floor(w + 0.5), 1.0).astype(np.int64)          # nint: halves away from zero
    n[0] = 0
    return n


# ------------------------------------------------------------------------------------------------ the head
def _upper_triangular_product(tables, x):
    """fast_sparse_matrix_multiply_upper_triangular's general branch, more_tools.f90:3646-3655, addition by addition"""
    ans = [0.0] * len(x)
    k = 0
    idx, val = tables["prj_indices"], tables["prj_values"]
    for i, cnt in enumerate(np.asarray(tables["prj_counts"]).tolist()):
        for _ in range(cnt):
            m = int(idx[k]) - 1
            v = float(val[k])
            ans[i] = ans[i] + v * x[m]
            if i != m:
                ans[m] = ans[m] + v * x[i]
            k += 1
    return ans


def head(walkers, tables, params, **mistakes):
    """The weights of the residents in front of the merge.  walkers: dict wt, imp_distance, matrix_elements (H_ii, for the walkers
    outside C(T)) of the list [C(T) | outside].  Returns dict(wt={0, 1: array}, sums={'ct_row', 'psit_row': ordered_sums})."""
    tau, et = float(params["tau"]), float(params["e_trial"])
    w0 = np.array(walkers["wt"], np.float64)
    n_ct = len(tables["ct_up"])
    num, den = np.asarray(tables["ct_num"], np.float64), np.asarray(tables["ct_den"], np.float64)
    loc, cdet = np.asarray(tables["loc_psit"], np.int64), np.asarray(tables["cdet"], np.float64)
    loc_imp = np.asarray(tables["loc_imp"], np.int64)
    assert loc[0] == 0 and loc_imp[0] == 0 and np.all(loc_imp < n_ct), "the reference's set-up assumptions"
    # 2262: the deterministic-space product, without the E_T term of 2290; it reads the weights in front of the move (C(T) is not moved)
    dw_imp = _upper_triangular_product(tables, w0[loc_imp].tolist())
    # 2286 with diag_elems (more_tools.f90:3656-3662): first row, first column and the extra diagonal over C(T)
    wc = w0[:n_ct]
    a_ct = 0.0 + num * wc[0]
    a_ct = a_ct + np.asarray(tables["diag_elems"], np.float64) * wc
    t_ct = num * wc
    t_ct[0] = (num[0] if mistakes.get("first_row_enum_raw") else num[0] / den[0]) * wc[0]
    s_ct = ordered_sums(t_ct.tolist(), **mistakes)
    # 2287 (more_tools.f90:3663-3667): the Psi_T locations with (1 + tau E_T) c
    val = (1.0 + tau * et) * cdet
    a_ps = 0.0 + val * wc[loc[0]]
    s_ps = ordered_sums((val[1:] * wc[loc[1:]]).tolist(), **mistakes)
    out = {}
    for order in (0, 1):
        w = w0.copy()
        # 3743-3793: the diagonal move of every walker outside the deterministic space and C(T)
        if len(w) > n_ct:
            assert np.all(np.asarray(walkers["imp_distance"])[n_ct:] >= 1)
            f = 1.0 + tau * (et - np.asarray(walkers["matrix_elements"], np.float64)[n_ct:])
            assert np.all(np.abs(f) < 1e40), "H_ii of a walker outside C(T) is needed"
            w[n_ct:] = w[n_ct:] * np.where(f < 0, 0.0, f)
        a = a_ct.copy()
        a[0] = 0.0 + _pick(s_ct, order)
        w[:n_ct] = wc - tau * a + (tau * et) * wc                      # 2313-2315
        ap = a_ps.copy()
        ap[0] = (0.0 + _pick(s_ps, order)) if len(loc) > 1 else 0.0
        w[loc] = w[loc] + ap                                           # 2316-2318 (the locations are distinct)
        w[loc_imp] = w[loc_imp] + np.array(dw_imp)                     # 2321-2323
        out[order] = w
    return dict(wt=out, sums=dict(ct_row=s_ct, psit_row=s_ps))


# ------------------------------------------------------------------------------------------------ the tail
def _check_initiator(w, imp, init, ps, p):
    """check_initiator without the discard (the caller decides), as 5952-5968 state it; returns (w, init)"""
    r_init, cti = p["r_initiator"], bool(p["c_t_initiator"])
    thr = r_init * (max(0, imp - p["initiator_min_distance"]) ** p["initiator_power"])
    if init == 3 and r_init >= 0:
        assert ps in (1, -1), "a permanent initiator needs its sign"
        if w * ps < 1:
            w = float(ps)
    elif init == 2 and ((abs(w) <= thr and imp > 0) or ((abs(w) <= r_init and not cti) and imp == -2)):
        init = 1
    elif init < 2 and ((abs(w) > thr and imp >= 0) or ((abs(w) > r_init or cti) and imp == -2)):
        init += 1
    return w, init


def tail(premerge_weights, flags, spawns, tables, params, draw=None, **mistakes):
    """What merge_my_original_with_spawned3, T^-1, check_initiator over C(T), reduce_my_walker and the reweighting leave of a list.
    premerge_weights: the residents' weights in front of the merge; flags: dict up, dn, imp_distance, initiator, perm_sign of the
    residents [C(T) | outside]; spawns: dict up, dn, wt, imp_distance, initiator in creation order (weight 0: no walker).
    draw(up, dn): the rounding draw of a determinant outside C(T), for inputs that need one (the pinned cases need none).
    Returns {0, 1: dict(up, dn, wt, imp_distance, initiator, stats, stats_seq, spread)} per sum order and 'sums': {'tinv': ordered_sums};
    stats: the 16 sums correctly rounded, stats_seq: added in the reference's order, spread[k] = (terms, sum |terms|)."""
    p = params
    assert p["semistochastic"], "the variant is semistochastic by definition"
    n_ct = len(tables["ct_up"])
    n0 = len(premerge_weights)
    w_pre = np.asarray(premerge_weights, np.float64)
    imp0, ini0 = np.asarray(flags["imp_distance"]).astype(int), np.asarray(flags["initiator"]).astype(int)
    ps0 = np.asarray(flags["perm_sign"]).astype(int)
    assert set(np.unique(imp0[:n_ct]).tolist()) <= {0, -2} and (n0 == n_ct or imp0[n_ct:].min() >= 1), "1267-1300: C(T) carries 0 / -2, the rest >= 1"
    slot = {(int(u), int(d)): i for i, (u, d) in enumerate(zip(np.asarray(tables["ct_up"]).tolist(), np.asarray(tables["ct_dn"]).tolist()))}
    su, sd, sw = np.asarray(spawns["up"]).tolist(), np.asarray(spawns["dn"]).tolist(), np.asarray(spawns["wt"], np.float64).tolist()
    si, sn = np.asarray(spawns["imp_distance"]).astype(int).tolist(), np.asarray(spawns["initiator"]).astype(int).tolist()
    r_init = p["r_initiator"]
    # ---- 6543-6586: a spawn on a determinant of C(T) folds into the resident -- the pairwise initiator rule, the weight added unless the
    #      resident is in the deterministic space and the spawn came from there; no imp_distance rule, no initiator test, no discard
    wct, ict = w_pre[:n_ct].tolist(), ini0[:n_ct].tolist()
    outside = []
    n_live = 0
    for k in range(len(su)):
        if sw[k] == 0.0:
            continue
        n_live += 1
        i = slot.get((su[k], sd[k]))
        if i is None:
            outside.append(k)
            continue
        wr, ws = wct[i], sw[k]
        if ws * wr > 0:
            ict[i] = max(ict[i], sn[k])
        elif abs(wr) < abs(ws):
            if ict[i] != 3 or r_init == -1.0:
                ict[i] = sn[k]
        elif abs(wr) == abs(ws):
            if ict[i] != 3 or r_init == -1.0:
                ict[i] = 0
        if not (imp0[i] == 0 and si[k] == -1):                         # 6563
            wct[i] = wr + ws
    # ---- everything else: merge_original_with_spawned2's fold, test and discard, reduce_my_walker and the reweighting.  Q2: the first
    #      record of a new determinant arrives with -1 turned into 1, as every first record of a run does at 5985-5986
    first_seen = {(int(u), int(d)) for u, d in zip(np.asarray(flags["up"])[n_ct:].tolist(), np.asarray(flags["dn"])[n_ct:].tolist())}
    o_imp = []
    for k in outside:
        key = (su[k], sd[k])
        o_imp.append(1 if (si[k] == -1 and key not in first_seen) else si[k])
        first_seen.add(key)
    res_out = dict(up=np.asarray(flags["up"])[n_ct:], dn=np.asarray(flags["dn"])[n_ct:], wt=w_pre[n_ct:], imp_distance=imp0[n_ct:], initiator=ini0[n_ct:],
                   perm_sign=ps0[n_ct:])
    sp_out = dict(up=[su[k] for k in outside], dn=[sd[k] for k in outside], wt=[sw[k] for k in outside], imp_distance=o_imp, initiator=[sn[k] for k in outside])
    m = AC.fold(res_out, sp_out, p, exact=False, draw=draw)              # without draw(up, dn): raises NeedsDraw where reduce_my_walker would draw
    assert not len(m["wt"]) or (m["imp_distance"].min() >= 1 and m["initiator"].max() <= 2)
    keep = np.ones(n_ct, bool)
    if mistakes.get("discard_ct_zero"):
        keep = ~((np.array(wct) == 0.0) & (imp0[:n_ct] != 0))
    # ---- 2394-2442: T^-1 and its transpose on the Psi_T locations, from the MERGED weights
    loc, cdet = np.asarray(tables["loc_psit"], np.int64), np.asarray(tables["cdet"], np.float64)
    src = w_pre[:n_ct] if mistakes.get("tinv_from_premerge") else np.array(wct)
    s_ti = ordered_sums((cdet[1:] * src[loc[1:]]).tolist(), **mistakes)
    num, den = np.asarray(tables["ct_num"], np.float64), np.asarray(tables["ct_den"], np.float64)
    n_perm = int(ini0[0] == 3)
    w_abs_before = math.fsum([abs(x) for x in w_pre.tolist()] + [abs(x) for x in sw])
    out = dict(sums=dict(tinv=s_ti), n_before=n0 + n_live, discarded=m["discarded"])
    for order in (0, 1):
        w = np.array(wct)
        tmp = (0.0 + _pick(s_ti, order)) if len(loc) > 1 else 0.0
        w1 = w[loc[0]] - tmp
        w1 = w1 / cdet[0]
        w1 = w1 / cdet[0]
        w[loc[0]] = w1
        w[loc[1:]] = w[loc[1:]] - cdet[1:] * w1
        # ---- 2444-2462: check_initiator over C(T), nothing discarded; with c_t_initiator only the first n_permanent_initiator slots
        ini = list(ict)
        w = w.tolist()
        upto = n_ct if (not p["c_t_initiator"] or mistakes.get("cti_checks_all")) else n_perm
        for i in range(upto):
            w[i], ini[i] = _check_initiator(w[i], int(imp0[i]), ini[i], int(ps0[i]), p)
        w = np.array(w) * p["reweight_factor_inv"]                       # 2487
        new = dict(up=np.concatenate([np.asarray(tables["ct_up"], np.uint64)[keep], m["up"]]), dn=np.concatenate([np.asarray(tables["ct_dn"], np.uint64)[keep], m["dn"]]),
                   wt=np.concatenate([w[keep], m["wt"]]), imp_distance=np.concatenate([imp0[:n_ct][keep], m["imp_distance"]]).astype(np.int8),
                   initiator=np.concatenate([np.array(ini)[keep], m["initiator"]]).astype(np.int8))
        # ---- 2573-2598 over the list, 2701-2722 over C(T)
        wl = new["wt"].tolist()
        terms = {k: [] for k in (0, 1, 2, 3, 4, 6, 8, 9, 10, 11, 12, 13)}
        for x, d, i, s in zip(wl, new["imp_distance"].tolist(), new["initiator"].tolist(), np.concatenate([ps0[:n_ct][keep], np.zeros(len(m["wt"]), int)]).tolist()):
            if i == 3:
                terms[4].append(x * s)
            terms[0].append(x); terms[8].append(x * x); terms[1].append(abs(x))
            if d == 0 or (d == -2 and p["c_t_initiator"]):
                terms[6].append(abs(x))
        for j, jj in enumerate(np.nonzero(keep)[0].tolist()):
            if jj == 0:
                en = (num[0] if mistakes.get("first_row_enum_raw") else num[0] / den[0]) * wl[j]; ed = wl[j]
            else:
                en = num[jj] * wl[j]; ed = den[jj] * wl[j]
            if abs(ed) < 1e-22:
                ed = abs(ed)
            terms[2].append(ed); terms[10].append(ed * ed); terms[12].append(abs(ed))
            terms[3].append(en); terms[9].append(en * en); terms[11].append(en * math.copysign(1.0, ed)); terms[13].append(en * ed)
        st, seq, spread = [0.0] * 16, [0.0] * 16, {}
        for k, t in terms.items():
            st[k] = math.fsum(t)
            acc = 0.0
            for x in t:
                acc += x
            seq[k] = acc
            spread[k] = (len(t), math.fsum(abs(x) for x in t))
        for k, v in ((5, float(len(wl))), (7, float(n0 + n_live)), (14, w_abs_before)):
            st[k] = seq[k] = v
        spread[14] = (n0 + n_live, w_abs_before)
        new["stats"], new["stats_seq"], new["spread"] = np.array(st), np.array(seq), spread
        out[order] = new
    return out
