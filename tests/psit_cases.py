"""Directed inputs for the step variant hf_to_psit -- psit_kernels.h, k_anneal<ITEMS, 1> with fold_slot<1>, the p.koff branches of k_gate,
k_spawn and k_spawn_keys -- their expected output from the independent model (tests/psit_checker.py), and the program that puts them
through the library.  The pattern is anneal_edge_cases.py's: the test process builds and solves, a fresh child per variant runs.

The operator is the C2 fixture; the TABLES ARE SYNTHETIC (C(T) list, e_loc_num / e_loc_den, Psi_T positions and coefficients, diag_elems,
deterministic-space matrix): the kernels read them as opaque tables, so any sorted set of determinants with the right electron numbers
serves as C(T), and small and exact shapes are reachable.

Set H: one sqmc_gpu_step each with always_spawn_cutoff_wt = 0 (a draw-free gate) and min_wt = 0 (no rounding draw), every C(T) slot
non-zero, at the named sizes of C(T) and Psi_T (H_PAIRS), in both sum orders.  Values are quantised (multiples of 2^-6: every head
sum is exact in any order, so a difference is an indexing error) or full-mantissa with terms that alternate in sign and nearly cancel
(the tree and the left-to-right sum differ in bits; only sizes beyond one chunk can tell them apart, so only those are pinned).
The child compares sqmc_gpu_debug_premerge with head(), out_stats[15] and the spawn slots with children(), and the downloaded list with
tail() of the device's own spawn records, bit for bit.

Set T: hand-built spawn lists through sqmc_gpu_annihilate (k_spawn_keys -> psit_key -> fold_slot<1>), written as their sorted list
(key' = rank, + koff outside C(T)) for a tile of 256 x ITEMS slots; weights multiples of 0.25, c_1 = 0.5 and the other coefficients
multiples of 0.25, so T^-1 is exact as well.  Spawns onto C(T) carry imp_distance -1, 1, 2 or 3 -- what k_spawn writes; a spawn flagged
0 or -2 is no output of the reference's move and is not pinned.

  python psit_cases.py FILE VARIANT    every case through the library; one JSON line per case; exit 0: all equal the model, 1: a mismatch,
                                       3: a HIP failure (it stops at once and starts nothing more on the GPU).
"""
import json
import math
import os
import pickle
import sys
import time
from itertools import combinations

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

SEED = (1346, 5634, 6635, 4361)
MAXTERMS = 64 ** 3
ERR_UNSUPPORTED = -3

# variant -> (environment, slots per thread of k_anneal<., 1> below 2^20 sorted slots)
VARIANTS = {
    "default": ({}, 2),
    "items3": ({"SQMC_ANNEAL_ITEMS": "3"}, 3),
    "unpacked": ({"SQMC_FORCE_UNPACKED": "1"}, 2),
    "items3_unpacked": ({"SQMC_ANNEAL_ITEMS": "3", "SQMC_FORCE_UNPACKED": "1"}, 3),
}
NO_SWITCH = ("default", "unpacked")          # the variants that choose the slots per thread by the list's length


def kernel_constants():
    import re
    csrc = os.path.join(ROOT, "sqmc_amd", "csrc")
    g = lambda name, f: int(re.search(r"#define %s (\d+)" % name, open(os.path.join(csrc, f)).read()).group(1))
    return dict(TPB=g("TPB", "sqmc_gpu.hip"), MERGE_SELF=g("MERGE_SELF", "walk_kernels.h"))


def universe(norb, nup, ndn, n_dn=18):
    """a sorted universe of determinants that owes nothing to any C(T): every up string with the n_dn smallest dn strings; its first
    determinant is the smallest there is (rank 0)"""
    strings = lambda k: sorted(sum(1 << o for o in c) for c in combinations(range(norb), k))
    ups, dns = strings(nup), strings(ndn)[:n_dn]
    return np.repeat(np.array(ups, np.uint64), len(dns)), np.tile(np.array(dns, np.uint64), len(ups))


def _prm(**kw):
    from anneal_checker import default_params
    return default_params(**kw)


# ------------------------------------------------------------------------------------------------ set H
# (n_ct, n_psit - 1, n_imp, c_t_initiator, first state a permanent initiator, Psi_T spread over C(T))
H_PAIRS = [
    (1, 0, 1, 0, 1, False),                # the smallest C(T) there is: the first state alone, no term in any Psi_T sum, no child
    (2, 1, 1, 1, 0, False),
    (63, 0, 4, 0, 0, False),
    (64, 63, 5, 1, 1, False),              # one full chunk in each sum
    (65, 64, 4, 0, 1, True),               # the chunk seam
    (4095, 65, 5, 1, 0, True),
    (4096, 1023, 4, 0, 0, False),          # one full block; 16 rows: the r0 loop's only round
    (4097, 1024, 5, 1, 1, True),           # level 3 of the C(T) row; Psi_T on slots 4095 and 4096; 17 rows
    (8192, 1025, 1, 0, 1, True),
    (8193, 4095, 4, 1, 0, False),
    (3 * 4096 + 37, 4096, 5, 0, 0, True),  # three blocks and a partial chunk; a full block of Psi_T terms
    (4 * 4096 + 37, 4097, 4, 1, 1, True),  # level 3 of the two Psi_T sums
    (5 * 4096, 2 * 4096 + 29, 5, 0, 1, True),      # two blocks and a partial chunk of Psi_T terms
    (MAXTERMS, 2 * 4096 + 29, 4, 0, 1, True),      # the limit
]


def h_case(uu, ud, n_ct, npm1, n_imp, cti, perm, spread, kind, seed):
    rs = np.random.RandomState(seed)
    n_psit = npm1 + 1
    assert n_psit <= n_ct and n_imp <= n_ct and kind in ("q", "f")
    if not spread or n_psit == n_ct:
        loc = np.arange(n_psit, dtype=np.int64)
    else:
        must = {0, n_ct - 1} | ({4095, 4096} if (n_ct > 4096 and n_psit >= 4) else set())
        assert len(must) <= n_psit
        rest = np.setdiff1d(np.arange(n_ct), np.array(sorted(must)))
        loc = np.sort(np.concatenate([np.array(sorted(must), np.int64), rs.choice(rest, n_psit - len(must), replace=False)]))
    imp = {0}
    if n_imp > 1 and n_psit > 1:
        imp.add(int(loc[1]))                   # in Psi_T and in the deterministic space: all three additions of k_psit_apply
    free = np.setdiff1d(np.arange(n_ct), loc)
    pool = free if len(free) >= n_imp else np.arange(n_ct)
    for x in rs.permutation(pool).tolist():
        if len(imp) >= n_imp:
            break
        imp.add(int(x))
    loc_imp = np.array(sorted(imp), np.int64)
    assert len(loc_imp) == n_imp
    sign = rs.choice([-1.0, 1.0], n_ct)
    if kind == "q":
        w = sign * rs.randint(1, 97, n_ct) / 64.0
        if n_ct >= 63:
            w[5], w[6], w[7] = 2.5, -3.5, 0.5          # nint rounds halves away from zero: 3, 4 and 1 children
        num = rs.randint(-128, 129, n_ct) / 64.0
        cdet = rs.choice([-1.0, 1.0], n_psit) * rs.randint(1, 33, n_psit) / 64.0
        cdet[0] = 0.5                                  # a power of two, and not 1: e_num(1) / e_den(1) stays exact
        diag = rs.randint(-64, 65, n_ct) / 16.0
        pv = lambda: float(rs.randint(-32, 33)) / 64.0
        tau, e_trial = 2.0 ** -6, -0.5
    else:
        w = sign * (0.5 + 1.4 * rs.rand(n_ct))
        alt = np.where(np.arange(n_ct) % 2 == 0, 1.0, -1.0)
        num = alt * (1.0 + 1e-3 * rs.standard_normal(n_ct)) / w                     # num_i w_i = +-(1 + 1e-3 r): the row nearly cancels
        cdet = np.where(np.arange(n_psit) % 2 == 0, 1.0, -1.0) * 0.05 * (1.0 + 0.3 * rs.rand(n_psit)) / w[loc]
        cdet[0] = 0.9
        diag = 3.0 * rs.standard_normal(n_ct)
        pv = lambda: 0.05 * float(rs.standard_normal())
        tau, e_trial = 0.0137, -0.613
    w[0] = abs(w[0]) + 1.0
    diag[loc_imp] = 0.0
    den = np.zeros(n_ct)
    den[loc] = cdet
    cnt, idx, val = [1], [1], [0.0]                    # the matrix without its first row and column; (1,1) kept, as 0
    for i in range(2, n_imp + 1):
        cnt.append(i - 1); idx += [i] + list(range(2, i)); val += [pv() for _ in range(i - 1)]
    impd = np.full(n_ct, -2, np.int8); impd[loc_imp] = 0
    init = np.where(rs.rand(n_ct) < 0.3, 1, 2).astype(np.int8); init[0] = 3 if perm else 2
    ps = np.zeros(n_ct, np.int8); ps[0] = 1 if perm else 0
    tables = dict(ct_up=uu[:n_ct].copy(), ct_dn=ud[:n_ct].copy(), ct_num=num, ct_den=den, loc_psit=loc, cdet=cdet, diag_elems=diag, loc_imp=loc_imp,
                  prj_counts=np.array(cnt, np.int64), prj_indices=np.array(idx, np.int64), prj_values=np.array(val))
    big = np.full(n_ct, 1e51)
    walkers = dict(up=tables["ct_up"], dn=tables["ct_dn"], wt=w, imp_distance=impd, initiator=init, perm_sign=ps, matrix_elements=big, e_num=big, e_den=big)
    prm = _prm(tau=tau, e_trial=e_trial, reweight_factor_inv=0.5 if seed % 2 else 1.0, r_initiator=1.0, min_wt=0.0, always_spawn_cutoff_wt=0.0, c_t_initiator=cti)
    name = "H_nct%d_np%d_%s" % (n_ct, n_psit, kind)
    meta = dict(set="H", kind=kind, n_ct=n_ct, n_psit=n_psit, n_imp=n_imp, cti=cti, perm=perm, spread=bool(spread and n_psit < n_ct))
    if n_ct == MAXTERMS:
        meta["only_runs"] = (("default", 1), ("unpacked", 0))      # the model's tail of 2.6e5 spawn records takes seconds: once per sum order
    return dict(name=name, tables=tables, walkers=walkers, prm=prm, meta=meta)


def build_h_cases(uu, ud):
    cases = []
    for k, (n_ct, npm1, n_imp, cti, perm, spread) in enumerate(H_PAIRS):
        cases.append(h_case(uu, ud, n_ct, npm1, n_imp, cti, perm, spread, "q", 100 + k))
        if n_ct > 65 and n_ct < MAXTERMS:              # up to 65 terms the tree IS the left-to-right sum; the limit is pinned once, quantised
            cases.append(h_case(uu, ud, n_ct, npm1, n_imp, cti, perm, spread, "f", 200 + k))
    return cases


def solve_h(case, **mistakes):
    """the model's head and gate of a set H case; returns the head's sums"""
    import psit_checker as PS
    h = PS.head(case["walkers"], case["tables"], case["prm"], **mistakes)
    nch = PS.children(case["walkers"], case["prm"])
    case["head"] = h["wt"]
    case["n_children"] = int(nch.sum())
    case["meta"]["mwalk"] = len(case["walkers"]["wt"]) + case["n_children"] + 4096
    return h["sums"]


# ------------------------------------------------------------------------------------------------ set T
class TB:
    """A set T case written as its sorted list: the C(T) determinants in order, each resident followed by its spawns, then the
    determinants outside C(T) in order.  C(T) takes the universe's even indices from ct_start on, everything else is outside."""

    def __init__(self, uu, ud, seed, ct_start=0):
        self.uu, self.ud, self.rs = uu, ud, np.random.RandomState(seed)
        self.next_ct, self.next_out = ct_start, ct_start + 1
        self.ct_recs, self.out_recs, self.marks, self.zeros = [], [], [], 0
        self.n_slots = 0

    def slots(self):
        return self.n_slots

    def _w(self):
        return float(self.rs.choice([-1.0, 1.0]) * self.rs.randint(1, 17) / 4.0)

    def ct(self, w=None, imp=-2, init=2, c=None, spawns=(), mark=None):
        """a C(T) resident (c: its Psi_T coefficient, if it has one) and the spawns onto it, (wt, imp_distance, initiator) each"""
        assert not self.out_recs, "C(T) sorts first"
        u = self.next_ct; self.next_ct += 2
        if not self.ct_recs:
            imp, c = 0, 0.5                                # the first state: of Psi_T, of C(T) and of the deterministic space
        at = self.n_slots
        self.ct_recs.append((u, self._w() if w is None else w, imp, init, c, list(spawns)))
        self.n_slots += 1 + len(spawns)
        if mark:
            self.marks.append((mark, u, 0, at))
        return at

    def pad_ct(self, upto):
        """plain C(T) residents without spawns up to slot `upto` (exclusive)"""
        while self.n_slots < upto:
            k = len(self.ct_recs)
            self.ct(imp=0 if k % 7 == 0 else -2, init=1 if k % 5 == 3 else 2, c=(float(self.rs.randint(1, 5)) / 4.0 * (1 if k % 2 else -1)) if k % 11 == 4 else None)

    def out(self, res=None, spawns=(), mark=None, at=None):
        """a determinant outside C(T): a survivor (wt, imp_distance >= 1, initiator) or none, and the spawns onto it"""
        u = self.next_out if at is None else at
        assert at is None or (at < self.ct_recs[0][0] and (not self.out_recs or at > self.out_recs[-1][0])), "below C(T)'s first determinant, in order"
        if at is None:
            self.next_out += 2
        slot = self.n_slots
        self.out_recs.append((u, res, list(spawns)))
        self.n_slots += (1 if res else 0) + len(spawns)
        if mark:
            self.marks.append((mark, u, 0, slot))
        return slot

    def finish(self, name, **meta):
        rs = self.rs
        n_ct = len(self.ct_recs)
        ct_u = np.array([r[0] for r in self.ct_recs], np.int64)
        assert np.all(np.diff(ct_u) > 0)
        loc = np.array([i for i, r in enumerate(self.ct_recs) if r[4] is not None], np.int64)
        cdet = np.array([self.ct_recs[i][4] for i in loc])
        impd = np.array([r[2] for r in self.ct_recs], np.int8)
        loc_imp = np.nonzero(impd == 0)[0].astype(np.int64)
        num = rs.randint(-32, 33, n_ct) / 16.0
        den = np.zeros(n_ct); den[loc] = cdet
        diag = rs.randint(-16, 17, n_ct) / 4.0; diag[loc_imp] = 0.0
        n_imp = len(loc_imp)
        tables = dict(ct_up=self.uu[ct_u], ct_dn=self.ud[ct_u], ct_num=num, ct_den=den, loc_psit=loc, cdet=cdet, diag_elems=diag, loc_imp=loc_imp,
                      prj_counts=np.ones(n_imp, np.int64), prj_indices=np.arange(1, n_imp + 1, dtype=np.int64), prj_values=np.zeros(n_imp))
        outs = sorted((r for r in self.out_recs), key=lambda r: r[0])
        assert len({r[0] for r in outs}) == len(outs) and not (set(ct_u.tolist()) & {r[0] for r in outs})
        ores = [(r[0],) + tuple(r[1]) for r in outs if r[1]]
        ru = np.concatenate([ct_u, np.array([r[0] for r in ores], np.int64)])
        n0 = len(ru)
        first_perm = self.ct_recs[0][3] == 3
        res = dict(up=self.uu[ru], dn=self.ud[ru], wt=np.array([r[1] for r in self.ct_recs] + [r[1] for r in ores], np.float64),
                   imp_distance=np.concatenate([impd, np.array([r[2] for r in ores], np.int8)]).astype(np.int8),
                   initiator=np.array([r[3] for r in self.ct_recs] + [r[3] for r in ores], np.int8), perm_sign=np.zeros(n0, np.int8),
                   matrix_elements=100.0 + np.arange(n0) / 8.0, e_num=np.full(n0, 1e51), e_den=np.full(n0, 1e51))
        res["perm_sign"][0] = 1 if first_perm else 0
        runs = [(r[0], r[5]) for r in self.ct_recs if r[5]] + [(r[0], r[2]) for r in outs if r[2]]
        flat = [(u, k) for u, sp in runs for k in range(len(sp))]
        by = {u: sp for u, sp in runs}
        order = rs.permutation(len(flat)).tolist()
        cursor = {u: 0 for u in by}
        sp = []
        for j in order:                                  # a shuffle that keeps the order inside every run
            u = flat[j][0]
            sp.append((u,) + tuple(by[u][cursor[u]])); cursor[u] += 1
        if self.zeros:
            zu = rs.randint(0, len(self.uu), self.zeros)
            za = np.sort(rs.randint(0, len(sp) + 1, self.zeros))
            su = np.insert(np.array([s[0] for s in sp], np.int64), za, zu)
            col = lambda k, fill, dt: np.insert(np.array([s[k] for s in sp], dt), za, np.full(self.zeros, fill, dt))
            spd = dict(up=self.uu[su], dn=self.ud[su], wt=col(1, 0.0, np.float64), imp_distance=col(2, 2, np.int8), initiator=col(3, 1, np.int8))
            spu = su
        else:
            spu = np.array([s[0] for s in sp], np.int64)
            spd = dict(up=self.uu[spu] if len(spu) else np.zeros(0, np.uint64), dn=self.ud[spu] if len(spu) else np.zeros(0, np.uint64), wt=np.array([s[1] for s in sp], np.float64),
                       imp_distance=np.array([s[2] for s in sp], np.int8), initiator=np.array([s[3] for s in sp], np.int8))
        meta = dict(meta, set="T", n_ct=n_ct, marks=self.marks, res_univ=ru, sp_univ=spu, slots=self.n_slots, mwalk=meta.get("mwalk", n0 + len(spd["wt"]) + 4096))
        prm = _prm(reweight_factor_inv=0.5 if len(name) % 2 else 1.0, r_initiator=1.0, min_wt=0.25, always_spawn_cutoff_wt=0.25, c_t_initiator=meta.get("cti", 0))
        return dict(name=name, tables=tables, res=res, sp=spd, prm=prm, meta=meta)


def sorted_slots(case):
    """the sorted order restated: key' = the determinant's rank among the universe for C(T), + koff (beyond every rank) outside it;
    residents in front of spawns, spawns in creation order; weight 0 is no walker.  Returns {(universe index, ordinal in its run): slot}."""
    m = case["meta"]
    koff = 1 << 40
    in_ct = set(m["res_univ"][:m["n_ct"]].tolist())
    key = lambda u: int(u) if int(u) in in_ct else int(u) + koff
    recs = [(key(u), 0, i) for i, u in enumerate(m["res_univ"].tolist())]
    recs += [(key(u), 1, i) for i, (u, w) in enumerate(zip(m["sp_univ"].tolist(), case["sp"]["wt"].tolist())) if w != 0.0]
    recs.sort()
    out, seen = {}, {}
    for slot, (k, kind, i) in enumerate(recs):
        u = k - koff if k >= koff else k
        o = seen.get(u, 0); seen[u] = o + 1
        out[(u, o)] = slot
    return out, len(recs)


def build_t_cases(uu, ud, T, consts):
    """set T for a tile of T slots.  meta['marks']: (label, universe index, ordinal in its run, slot) the CPU test re-derives"""
    MS = consts["MERGE_SELF"]
    cases, seed = [], [3000 + T]

    def B(**kw):
        seed[0] += 1
        return TB(uu, ud, seed[0], **kw)
    same = lambda n, w=0.25: [(w, (1, 2, 3)[k % 3], k % 2) for k in range(n)]
    mixed = lambda n: [((0.5 if k % 3 else -0.75), (2, -1, 1)[k % 3], (1, 0, 1)[k % 3]) for k in range(n)]
    tail_out = lambda b: (b.out(res=(1.0, 2, 2), spawns=[(0.5, 2, 1)]), b.out(spawns=[(0.75, 3, 1)]))
    # ---- n_ct against the tile: spawns on the last C(T) determinant and on the first determinant behind it
    for d in (-1, 0, 1):
        b = B(); b.pad_ct(T + d - 1)
        b.ct(w=1.5, init=1, spawns=[(0.5, 2, 1), (-0.25, -1, 0), (1.0, 3, 1)], mark="last_ct_resident")
        b.out(spawns=[(0.5, 2, 1), (-1.25, 2, 0), (0.25, 1, 1)], mark="first_record_behind_ct")
        tail_out(b)
        cases.append(b.finish("nct_is_tile%+d" % d, want_slots={"last_ct_resident": T + d - 1, "first_record_behind_ct": T + d + 3}))
    # ---- the boundary key < koff itself on the seam, and one slot to either side
    for d in (-1, 0, 1):
        b = B(); b.pad_ct(T + d - 6)
        b.ct(w=-2.0, spawns=same(5, -0.5), mark="last_ct_resident")
        b.out(res=(0.75, 1, 2), spawns=[(-0.75, 2, 1)], mark="first_record_behind_ct")          # a survivor cancelled: discarded, on the slot behind the seam
        b.out(spawns=[(0.5, -1, 1), (0.5, 2, 0)])
        tail_out(b)
        cases.append(b.finish("ct_boundary_on_slot_T%+d" % d, want_slots={"first_record_behind_ct": T + d}))
    # ---- runs on C(T) residents: MERGE_SELF followers and one more, 64 and 65, one sign (fold_chunk's fast branch) and mixed (the slow one)
    b = B(); b.pad_ct(37)
    for n in (MS, MS + 1, 64, 65):
        b.ct(w=0.5, imp=-2, spawns=same(n)); b.ct(w=0.5, imp=0, spawns=mixed(n)); b.ct(w=-1.0, spawns=mixed(n)); b.pad_ct(b.slots() + 3)
    tail_out(b)
    cases.append(b.finish("runs_of_%d_%d_64_65_followers_on_ct_residents" % (MS, MS + 1)))
    for tag, mk in (("one_sign", same), ("mixed_signs", mixed)):
        b = B(); b.pad_ct(T - 10)
        b.ct(w=0.75, init=1, spawns=mk(9 + 300), mark="head_of_the_long_run")
        b.pad_ct(b.slots() + 20); tail_out(b)
        cases.append(b.finish("run_leaves_the_tile_into_hbm_" + tag, want_slots={"head_of_the_long_run": T - 10}))
    # ---- Psi_T determinants that receive spawns on a tile's last and on a tile's first slot: T^-1 takes the merged weights
    b = B(); b.pad_ct(T - 1)
    b.ct(w=1.0, c=0.75, spawns=[(0.5, 2, 1), (0.25, 3, 1), (-2.0, 2, 0), (0.5, 1, 1)], mark="psit_on_last_slot")
    b.pad_ct(2 * T)
    b.ct(w=-0.5, c=-0.5, spawns=[(1.5, 2, 1), (0.25, 2, 1), (0.25, -1, 1)], mark="psit_on_first_slot")
    b.pad_ct(2 * T + 40); tail_out(b)
    cases.append(b.finish("psit_on_a_tiles_last_and_first_slot", want_slots={"psit_on_last_slot": T - 1, "psit_on_first_slot": 2 * T}))
    # ---- C(T) residents cancelled to exactly 0 stay in the list, in the deterministic space or not; imp_distance -1 onto 0 and onto -2
    b = B(); b.pad_ct(50)
    b.ct(w=1.5, imp=-2, init=2, spawns=[(-1.0, 2, 1), (-0.5, 3, 0)], mark="cancelled_outside_det_space")
    b.ct(w=0.75, imp=0, init=2, spawns=[(-0.75, 2, 1)], mark="cancelled_in_det_space")
    b.ct(w=-0.25, imp=-2, init=1, c=0.25, spawns=[(0.25, 1, 1)], mark="cancelled_psit")
    b.ct(w=1.0, imp=0, spawns=[(0.5, -1, 1)], mark="minus_one_onto_distance_0")
    b.ct(w=1.0, imp=-2, spawns=[(0.5, -1, 1)], mark="minus_one_onto_distance_-2")
    b.pad_ct(b.slots() + 30); tail_out(b)
    cases.append(b.finish("ct_residents_cancelled_to_zero"))
    # ---- outside C(T): merge_original_with_spawned2's cases, and Q1 / Q2
    b = B(); b.pad_ct(300)
    b.out(res=(1.0, 2, 1), spawns=[(-1.0, 2, 1)], mark="survivor_discarded")
    b.out(spawns=[(0.5, 2, 0)], mark="new_fails_the_initiator_test")
    b.out(spawns=[(0.5, 2, 1)], mark="new_passes")
    b.out(spawns=[(0.75, -1, 1)], mark="minus_one_becomes_one")
    b.out(res=(-0.5, 3, 2), spawns=[(0.25, 2, 0), (0.25, 1, 1)], mark="q1_first_survivor_discarded")
    b.out(spawns=[(1.25, 2, 1), (0.25, -1, 0)], mark="q1_new_between_two_survivors")
    b.out(res=(2.0, 1, 2), mark="q1_second_survivor")
    b.out(res=(0.5, 2, 1), spawns=[(0.25, 2, 1)])
    cases.append(b.finish("outside_ct_discards_new_determinants_q1_q2"))
    # ---- C(T) without the smallest determinant there is: an outside determinant whose key' is exactly koff
    b = B(ct_start=2); b.pad_ct(200)
    b.out(spawns=[(0.5, 2, 0)], at=0, mark="rank_zero_outside_fails_the_initiator_test")
    b.out(res=(1.0, 2, 2), spawns=[(0.5, 2, 1)], at=1)
    cases.append(b.finish("outside_determinant_with_key_koff"))
    # ---- the switch from two to three slots per thread at 2^20 sorted slots: almost all of them the "no walker" marker
    for n_all in ((1 << 20) - 1, 1 << 20):
        b = B(); b.pad_ct(700)
        b.ct(w=1.0, c=0.5, spawns=mixed(70)); b.pad_ct(b.slots() + 200)
        b.out(res=(1.0, 2, 1), spawns=[(-1.0, 2, 1)]); b.out(spawns=[(0.5, -1, 1)]); tail_out(b)
        b.zeros = n_all - b.slots()
        cases.append(b.finish("sorted_slots_%d" % n_all, only=NO_SWITCH, mwalk=(1 << 20) + 4096, n_all=n_all, items=2 if n_all < (1 << 20) else 3))
    return cases


def solve_t(case, **mistakes):
    import psit_checker as PS
    t = PS.tail(case["res"]["wt"], case["res"], case["sp"], case["tables"], case["prm"], **mistakes)
    case["want"] = {o: {k: t[o][k] for k in ("up", "dn", "wt", "imp_distance", "initiator", "stats", "spread")} for o in (0, 1)}
    case["n_discarded"] = len(t["discarded"])
    return t


def write(path, tables, cases, univ=None):
    """the file a child reads; univ = (up, dn): the child also tries the tables beyond 64^3"""
    blob = dict(tables=tables, cases=cases)
    if univ is not None:
        blob["universe"] = univ
    with open(path, "wb") as f:
        pickle.dump(blob, f, protocol=4)


# ------------------------------------------------------------------------------------------------ the child
def _ctx(blob, tb, mwalk, sum_order):
    import sqmc_amd
    t = blob["tables"]
    g = sqmc_amd.GpuChem(t["norb"], t["nup"], t["ndn"], t["orbsym"], t["prod"], t["combine_2"], t["integrals"], n_group=t["n_group"], rng_mode=1, seed=SEED, mwalk=mwalk)
    g.set_projector(tb["prj_counts"], tb["prj_indices"], tb["prj_values"])
    g.set_ct_table(tb["ct_up"], tb["ct_dn"], tb["ct_num"], tb["ct_den"])
    g.set_hf_to_psit(tb["loc_psit"] + 1, tb["cdet"], tb["diag_elems"], sum_order)
    return g


def stat_bound(spread, k):
    """|device - correctly rounded| for a sum of N terms added in ANY order: every term goes through at most N - 1 additions, each of
    which rounds by 2^-53 of a partial sum no larger than sum |terms| -- the bound of psit_checker.within_bound with the longest chain
    any reduction can have, K = N (derived from the reduction's shape, whatever it is; not the 1e-11 of test_gpu_parity._sums_close)"""
    n, mass = spread.get(k, (0, 0.0))
    return n * 2.0 ** -53 * mass * (1 + 2.0 ** -20)


def _compare(want, got, out, n_attempts=None):
    if len(got["up"]) != len(want["up"]):
        return "length %d, model %d" % (len(got["up"]), len(want["up"]))
    for k in ("up", "dn", "wt", "imp_distance", "initiator"):
        if not np.array_equal(got[k], want[k]):
            i = int(np.nonzero(got[k] != want[k])[0][0])
            return "%s differs first at %d: %r, model %r" % (k, i, got[k][i], want[k][i])
    for k in range(15):
        if not abs(out[k] - want["stats"][k]) <= stat_bound(want["spread"], k):
            return "out_stats[%d] = %r, model %r, bound %r" % (k, out[k], want["stats"][k], stat_bound(want["spread"], k))
    if n_attempts is not None and out[15] != n_attempts:
        return "out_stats[15] = %r, the gate's %d" % (out[15], n_attempts)
    return None


def run_h(blob, variant, case, order):
    import psit_checker as PS
    import sqmc_amd
    tb, wk, prm, meta = case["tables"], case["walkers"], case["prm"], case["meta"]
    rec = dict(case=case["name"], variant=variant, sum_order=order, n_ct=meta["n_ct"], n_psit=meta["n_psit"])
    t0 = time.time()
    g = _ctx(blob, tb, meta["mwalk"], order)
    try:
        g.upload_walkers(wk)
        try:
            out = g.step(prm)
        except sqmc_amd.SqmcGpuError as e:
            rec.update(status=e.code, ok=False, why=str(e))
            return rec
        rec["status"] = 0
        tail = g.last_tail(); rec["tail"] = tail
        pm = g.debug_premerge()
        why = None
        if tail != dict(kind="radix", items=VARIANTS[variant][1], merge=tail["merge"], packed="unpacked" not in variant):
            why = "tail %r" % (tail,)
        if why is None and not np.array_equal(pm["res_wt"], case["head"][order]):
            i = int(np.nonzero(pm["res_wt"] != case["head"][order])[0][0]) if len(pm["res_wt"]) == len(case["head"][order]) else -1
            why = "premerge weight differs first at slot %d: %r, head() %r" % (i, pm["res_wt"][i], case["head"][order][i])
        if why is None and not (len(pm["wt"]) == case["n_children"] == int(out[15])):
            why = "spawn slots %d, out_stats[15] %r, children() %d" % (len(pm["wt"]), out[15], case["n_children"])
        if why is None and np.any((pm["up"] == tb["ct_up"][0]) & (pm["dn"] == tb["ct_dn"][0]) & (pm["wt"] != 0.0)):
            why = "a spawn record with weight on the first determinant"
        if why is None:
            sp = {k: pm[k] for k in ("up", "dn", "wt", "imp_distance", "initiator")}
            want = PS.tail(pm["res_wt"], wk, sp, tb, prm)
            rec["ratio_tinv"] = PS.within_bound(want["sums"]["tinv"])
            rec["n_spawn_live"] = int(np.count_nonzero(pm["wt"])); rec["n_out"] = len(want[order]["up"]) - meta["n_ct"]; rec["n_discarded"] = len(want["discarded"])
            why = _compare(want[order], g.download_walkers(), out, case["n_children"])
        rec["ok"] = why is None
        if why:
            rec["why"] = why
    finally:
        g.close()
    rec["ms"] = round(1000 * (time.time() - t0), 1)
    return rec


def run_t(blob, variant, case, order):
    import sqmc_amd
    tb, res, sp, prm, meta = case["tables"], case["res"], case["sp"], case["prm"], case["meta"]
    rec = dict(case=case["name"], variant=variant, sum_order=order, n0=len(res["up"]), n_spawn=len(sp["up"]))
    t0 = time.time()
    g = _ctx(blob, tb, meta["mwalk"], order)
    try:
        g.upload_walkers(res)
        try:
            out = g.annihilate(prm, sp)
        except sqmc_amd.SqmcGpuError as e:
            rec.update(status=e.code, ok=False, why=str(e))
            return rec
        rec["status"] = 0
        tail = g.last_tail(); rec["tail"] = tail
        items = meta.get("items", VARIANTS[variant][1]) if variant in NO_SWITCH else VARIANTS[variant][1]
        why = None
        if tail != dict(kind="radix", items=items, merge=tail["merge"], packed="unpacked" not in variant):
            why = "tail %r, this case is written for %d slots per thread" % (tail, items)
        got = g.download_walkers()
        why = why or _compare(case["want"][order], got, out)
        if why is None:                                # the cached H_ii of every resident that stayed is the one it was uploaded with
            held = {(int(u), int(d)): float(m) for u, d, m in zip(res["up"], res["dn"], res["matrix_elements"])}
            for u, d, m in zip(got["up"].tolist(), got["dn"].tolist(), got["matrix_elements"].tolist()):
                if held.get((u, d), m) != m and not ((u, d) not in held and m > 1e50):
                    why = "matrix_elements of (%d, %d): %r, uploaded %r" % (u, d, m, held.get((u, d)))
                    break
        rec["ok"] = why is None
        if why:
            rec["why"] = why
    finally:
        g.close()
    rec["ms"] = round(1000 * (time.time() - t0), 1)
    return rec


def run_refusals(blob, variant):
    """n_ct = 64^3 + 1 and n_psit - 1 = 64^3 + 1 are refused with SQMC_ERR_UNSUPPORTED, and the context goes on to run a case"""
    import sqmc_amd
    uu, ud = blob["universe"]
    case = [c for c in blob["cases"] if c["meta"]["set"] == "T"][0]
    tb = case["tables"]
    t = blob["tables"]
    rec = dict(case="refusals_beyond_64^3", variant=variant)
    g = sqmc_amd.GpuChem(t["norb"], t["nup"], t["ndn"], t["orbsym"], t["prod"], t["combine_2"], t["integrals"], n_group=t["n_group"], rng_mode=1, seed=SEED, mwalk=case["meta"]["mwalk"])
    try:
        why = None
        n = MAXTERMS + 1
        g.set_projector(np.ones(1, np.int64), np.ones(1, np.int64), np.zeros(1))
        g.set_ct_table(uu[:n], ud[:n], np.ones(n), np.ones(n))
        for label, ix in (("n_ct", np.arange(1, 3, dtype=np.int64)), ("n_psit", np.arange(1, n + 2, dtype=np.int64))):
            if label == "n_psit":
                g.set_ct_table(tb["ct_up"], tb["ct_dn"], tb["ct_num"], tb["ct_den"])
            try:
                g.set_hf_to_psit(ix, np.full(len(ix), 0.5), np.zeros(n if label == "n_ct" else len(tb["ct_up"])), 1)
                why = why or "%s = 64^3 + 1 was accepted" % label
            except sqmc_amd.SqmcGpuError as e:
                if e.code != ERR_UNSUPPORTED or "64^3" not in str(e):
                    why = why or "%s = 64^3 + 1: status %d, %s" % (label, e.code, e)
        if why is None:                                # the context stays usable
            g.set_projector(tb["prj_counts"], tb["prj_indices"], tb["prj_values"])
            g.set_ct_table(tb["ct_up"], tb["ct_dn"], tb["ct_num"], tb["ct_den"])
            g.set_hf_to_psit(tb["loc_psit"] + 1, tb["cdet"], tb["diag_elems"], 1)
            g.upload_walkers(case["res"])
            out = g.annihilate(case["prm"], case["sp"])
            why = _compare(case["want"][1], g.download_walkers(), out)
        rec["ok"] = why is None
        if why:
            rec["why"] = why
    finally:
        g.close()
    return rec


def runs_in(case, variant, order):
    """the only filter there is: a case names the variants (meta['only']) or the (variant, sum order) pairs (meta['only_runs']) it runs in"""
    m = case["meta"]
    return (not m.get("only") or variant in m["only"]) and (not m.get("only_runs") or (variant, order) in m["only_runs"])


def main(argv):
    path, variant = argv[1], argv[2]
    for k in ("SQMC_ANNEAL_ITEMS", "SQMC_FORCE_UNPACKED"):
        assert os.environ.get(k) == VARIANTS[variant][0].get(k), "the environment of this process does not select variant %s" % variant
    with open(path, "rb") as f:
        blob = pickle.load(f)
    import sqmc_amd
    sqmc_amd.set_device(0)
    t0 = time.time()
    n_bad = 0
    jobs = [(run_h if c["meta"]["set"] == "H" else run_t, c, o) for c in blob["cases"] for o in (1, 0) if runs_in(c, variant, o)]
    for fn, case, order in jobs:
        rec = fn(blob, variant, case, order)
        print(json.dumps(rec, default=str), flush=True)
        if rec.get("status", 0) == -2:               # SQMC_ERR_HIP
            return 3
        n_bad += 0 if rec["ok"] else 1
    if "universe" in blob:
        rec = run_refusals(blob, variant)
        print(json.dumps(rec, default=str), flush=True)
        n_bad += 0 if rec["ok"] else 1
    print(json.dumps(dict(variant=variant, cases_failed=n_bad, jobs=len(jobs), seconds=round(time.time() - t0, 2))), flush=True)
    return 1 if n_bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
