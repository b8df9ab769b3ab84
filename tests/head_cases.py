"""Directed inputs for the head of a step -- the spawn gate (gate_children, k_replay_prepass, the gates fused into the annihilation
kernels), the child offsets of their five producers, gate_block_parents, k_spawn's parent search and spawn_emit's slots and flags --
their expected output from the independent model (tests/head_checker.py), and the program that puts them through the library.
The pattern is anneal_edge_cases.py's: the test process builds and solves, a fresh child per variant runs.

The determinants are generated universes (every up string with a few dn strings) of the C2 integrals with 8 electrons, with 10
electrons for the fast heat-bath proposal, and random determinants of the 57-orbital electron gas.  The C(T) table and the projector
are synthetic (a few determinants, a zero matrix with a stored diagonal): the head reads neither, and the tail is not re-tested here.
min_wt is 0 in the first-step sets, so no rounding draw is ever taken and REPLAY's generator ends where the model's ends.

Sets (build_first_step): G the gate; W the parent search on a first step (k_gate + scan, the 256-way narrowing); S the scan's tiles;
H the same on the heat-bath proposal (two slots per child) and on unpacked keys.  A list is written as segments --
  ("one", k)  k walkers of one child each      ("none", k)  k childless walkers      ("heavy", n)  one walker of n children
  ("w", [weights])  walkers of these weights
-- and every case names, in meta["claims"], the numbers of head_checker.layout() it is about.  A case whose layout misses a claim
FAILS as "seam not reached", on the CPU and in the child alike.

Set P (p_case): the second step of a pipelined sqmc_gpu_run, whose parents are the list L1 a twin context holds after one step.
L0 is built so that step 1 barely moves it; the child runs the model and layout() on the L1 it downloaded.

  python head_cases.py FILE VARIANT    every case of the variant through the library; one JSON line per case; exit 0: all equal the
                                       model, 1: a mismatch or a seam not reached, 3: a HIP failure (it stops at once and starts
                                       nothing more on the GPU).
"""
import json
import os
import pickle
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import head_checker as HC          # noqa: E402

SEED = (1346, 5634, 6635, 4361)
FCIDUMP = os.path.join(HERE, "golden", "C2_r1.24253_FCIDUMP")
ERR_MWALK, ERR_HIP = 1, -2
ULP = 2.0 ** -52
REPLAY_MAX_CHILDREN = 5000

# variant -> (environment, rng_mode, which cases, the head debug_last_head must report: pipelined, offsets, parent_hint)
VARIANTS = {
    "first_counter": ({}, 1, "first", (False, "gate_scan", False)),
    "first_replay": ({}, 0, "replay", (False, "replay_prepass", False)),
    "p_no_pipeline": ({"SQMC_NO_PIPELINE": "1"}, 1, "P", (False, "gate_scan", False)),
    "p_radix": ({"SQMC_BUCKET": "0"}, 1, "P+H", (True, "anneal_lookback", True)),
    "p_radix_no_offsets": ({"SQMC_BUCKET": "0", "SQMC_RADIX_NO_OFFSETS": "1"}, 1, "P", (True, "fused_gate_scan", False)),
    "p_radix_no_hint": ({"SQMC_BUCKET": "0", "SQMC_NO_PARENT_HINT": "1"}, 1, "P", (True, "anneal_lookback", False)),
    "p_bucket": ({"SQMC_BUCKET_HOLDOFF": "0"}, 1, "P", (True, "anneal_bucket", True)),
    "p_bucket_no_offsets": ({"SQMC_BUCKET_HOLDOFF": "0", "SQMC_BUCKET_NO_OFFSETS": "1"}, 1, "P", (True, "fused_gate_scan", False)),
    "p_split": ({"SQMC_BUCKET": "0", "SQMC_ANNEAL_SPLIT_MIN": "1"}, 1, "P", (True, "anneal_split_place", True)),
    "p_unpacked": ({"SQMC_FORCE_UNPACKED": "1"}, 1, "P", (True, "anneal_lookback", True)),
}
SWITCHES = sorted({k for v in VARIANTS.values() for k in v[0]})
BUCKET_TAIL = ("p_bucket", "p_bucket_no_offsets")


def universe(norb, nup, ndn, n_dn):
    """psit_cases.universe: every up string with the n_dn smallest dn strings, sorted by (up, dn)"""
    import psit_cases
    return psit_cases.universe(norb, nup, ndn, n_dn)


def heg_universe(norb, nup, ndn, n, seed=57):
    """n random determinants of nup + ndn electrons in norb plane waves, sorted by (up, dn)"""
    rs = np.random.RandomState(seed)
    dets = set()
    while len(dets) < n:
        u = sum(1 << int(o) for o in rs.choice(norb, nup, replace=False))
        d = sum(1 << int(o) for o in rs.choice(norb, ndn, replace=False))
        dets.add((u, d))
    dets = sorted(dets)
    return np.array([x[0] for x in dets], np.uint64), np.array([x[1] for x in dets], np.uint64)


def _prm(**kw):
    from anneal_checker import default_params
    p = default_params(tau=0.01, e_trial=-75.7, reweight_factor_inv=1.0, r_initiator=1.0, min_wt=0.0, always_spawn_cutoff_wt=0.5, semistochastic=1, reached_w_abs_gen=2)
    p.update(kw)
    return p


# ------------------------------------------------------------------------------------------------ building a list
IMP_CYCLE = (1, 2, -2, 3, 126, 127, 5, -2, 1)
INIT_CYCLE = (2, 1, 0, 3, 2, 1, 1, 2, 0, 3, 1)


def expand(segments, cutoff, seed):
    """the weights of a list written as segments.  A childless walker carries 0 or k 2^-30 cutoff (its draw never spawns it: checked by
    the model's own count); "one": |w| in [0.5, 1.5) at or above the cutoff; "heavy": |w| = n exactly or n + 0.25."""
    rs = np.random.RandomState(seed)
    w = []
    for kind, arg in segments:
        if kind == "one":
            a = rs.choice([0.75, 1.0, 1.25, 1.4375, 0.5], arg)
            w += (a * rs.choice([-1.0, 1.0], arg)).tolist()
        elif kind == "none":
            assert cutoff > 0
            a = np.where(rs.rand(arg) < 0.5, 0.0, rs.randint(1, 8, arg) * cutoff * 2.0 ** -30)
            w += (a * rs.choice([-1.0, 1.0], arg)).tolist()
        elif kind == "heavy":
            w.append(float(arg) * (1.0 if len(w) % 2 else -1.0) + (0.25 if arg % 2 else 0.0) * (1.0 if len(w) % 2 else -1.0))
        else:
            assert kind == "w"
            w += [float(x) for x in arg]
    return np.array(w, np.float64)


def make_case(name, set_, univ, wt, prm, claims=None, system="c2", **meta):
    """walkers on the first len(wt) determinants of an even spread over the universe; imp_distance 0 on the first and the last slot
    (the deterministic space: two rows), the other flags in cycles that meet every rule of 3703-3726"""
    uu, ud = univ
    n = len(wt)
    assert 2 <= n <= len(uu), (name, n, len(uu))
    ix = np.unique(np.linspace(0, len(uu) - 1, n).astype(np.int64))
    assert len(ix) == n
    k = np.arange(n)
    imp = np.array(IMP_CYCLE, np.int8)[k % len(IMP_CYCLE)]
    imp[0] = imp[-1] = 0
    ini = np.array(INIT_CYCLE, np.int8)[k % len(INIT_CYCLE)]
    ps = np.where(ini == 3, np.where(k % 2 == 0, 1, -1), 0).astype(np.int8)
    walkers = dict(up=uu[ix].copy(), dn=ud[ix].copy(), wt=np.asarray(wt, np.float64), imp_distance=imp, initiator=ini, perm_sign=ps)
    return dict(name=name, set=set_, system=system, walkers=walkers, prm=prm, claims=claims or {}, meta=meta)


def seg_case(name, set_, univ, segments, seed, cutoff=0.5, claims=None, system="c2", prm=None, **meta):
    prm = _prm(always_spawn_cutoff_wt=cutoff, c_t_initiator=seed % 2, **(prm or {}))
    return make_case(name, set_, univ, expand(segments, cutoff, seed), prm, claims, system, segments=[list(s) if s[0] != "w" else ["w", len(s[1])] for s in segments], **meta)


def check_claims(lay, claims):
    """None, or the first claim the layout misses.  A claim is a value, or (op, value) with op in ge / le / gt."""
    for k, want in claims.items():
        got = lay[k]
        if isinstance(want, tuple):
            op, v = want
            ok = got >= v if op == "ge" else got <= v if op == "le" else got > v
        else:
            ok = got == want
        if not ok:
            return "seam not reached: layout()[%r] = %r, the case is written for %r" % (k, got, want)
    if not lay["parents_ok"]:
        return "the restated search of layout() does not find np.repeat's parents"
    return None


def g_cases(univ):
    """set G.  The draw-deciding weights are set by draw_deciding() once the generator is at hand."""
    out = []
    for cutoff in (0.5, 0.25, 0.0):
        c = cutoff
        w = [1.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 1.5 - ULP, -(1.5 - ULP), 3.5, -4.5, 0.0, -0.0, 0.75, -1.25]      # 1.5 - ULP: the double below 1.5, one child
        if c > 0:
            w += [c, -c, c * (1 - ULP / 2), -c * (1 - ULP / 2), c * 2.0 ** -30, -c * 2.0 ** -30, c * 0.999, -c * 0.5, c * 0.25, c * 0.75]
        if c == 0.25:
            w += [0.25, 0.3, -0.4, 0.5 - ULP / 4, -0.49]      # [0.25, 0.5): nint = 0, one child of w
        if c == 0.0:
            w += [2.0 ** -1000, -2.0 ** -30, 0.3, -0.49, 5e-324]      # everything is at or above a cutoff of 0: max(nint, 1) = 1 child of w
        w += [1.0, -2.0]
        prm = _prm(always_spawn_cutoff_wt=c, c_t_initiator=1 if c == 0.25 else 0)
        out.append(make_case("G_cutoff_%g" % c, "G", univ, np.array(w), prm, dict(blocks=1)))
    return out


def draw_deciding(case_name, univ, streams_of, cutoff=0.5, n=24):
    """weights on both sides of their own gate draw d: cutoff * d (d < |w / cutoff| fails: no child) and cutoff * the double above d
    (one child).  cutoff is a power of two, so w / cutoff is exact.  In REPLAY the draw of walker i depends on what the walkers in
    front of it consumed: the list is built walker by walker with the model's own stream (streams_of(walkers) -> the next gate draw)."""
    uu, ud = univ
    base = make_case(case_name, "G", univ, np.ones(n), _prm(always_spawn_cutoff_wt=cutoff))
    wk = base["walkers"]
    w = np.zeros(n)
    for i in range(n):
        wk["wt"] = w
        d = streams_of(wk, i)
        if i % 4 == 3:
            w[i] = 1.0 if i % 8 == 3 else -2.0               # ordinary walkers in between: their children move the REPLAY stream
        else:
            w[i] = cutoff * (d if i % 2 == 0 else np.nextafter(d, 1.0)) * (1.0 if i % 3 else -1.0)
    wk["wt"] = w
    base["claims"] = dict(blocks=1)
    base["meta"]["want_children_of"] = {i: (0 if i % 2 == 0 else 1) for i in range(n) if i % 4 != 3}
    return base


def w_cases(univ, consts):
    """set W: the parent search on a first step"""
    T, W = consts["TPB"], consts["SPAWN_WIN"]
    out, seed = [], [100]

    def S(name, segments, claims, **kw):
        seed[0] += 1
        out.append(seg_case(name, "W", univ, segments, seed[0], claims=claims, **kw))
    for R in (W - 2, W - 1, W, W + 1):
        # (a) the run in the middle of block 0's children: the window starts on slot 0, the parent behind the run lies past it
        S("W_run%d_mid_block" % R, [("one", 100), ("none", R), ("one", 300)], dict(children_beyond_window=("ge", T - 100), longest_childless_run=R))
        # (b) the run directly in front of block 1's first child: an equal-offset run over many probe positions of the narrowing
        S("W_run%d_before_block_start" % R, [("one", T), ("none", R), ("one", 300)], dict(longest_childless_run=R, tie_probes=("ge", 2), narrowing_rounds=1))
    for R in (W - 3, W - 2, W - 1):
        # the window starts on the heavy parent of slot 0; the first parent behind the run sits on window entry R + 1: the last one the
        # window search can return (W - 2), the window's last entry (W - 1: its first child EQUALS s_win[W - 1]), one past it
        S("W_next_parent_on_window_entry_%d" % (R + 1), [("heavy", 300), ("none", R), ("one", 300)], dict(children_beyond_window=("ge", 1), longest_childless_run=R))
    S("W_n0_%d_no_narrowing" % W, [("one", 200), ("none", W - 500), ("one", 300)], dict(n0=W, narrowing_rounds=0))
    S("W_n0_%d_one_round" % (W + 1), [("one", 200), ("none", W - 499), ("one", 300)], dict(n0=W + 1, narrowing_rounds=1))
    heavy = (255, 256, 257, 511, 512, 513, 4097)
    for r in (0, 1, 255):
        segs, at = [("one", r)] if r else [], r
        for h in heavy:
            segs.append(("heavy", h)); at += h
            pad = (r - at) % T
            segs += [("one", pad)] if pad else []
            at += pad
        segs.append(("one", 7))
        S("W_heavy_parents_at_offset_%d_mod_%d" % (r, T), segs, dict(heavy_nchild=list(heavy), heavy_off_mod=[r] * len(heavy)))
    S("W_heavy_on_first_and_last_slot", [("heavy", 300), ("one", 50), ("none", 10), ("heavy", 513)], dict(heavy_slots=[0, 61], heavy_nchild=[300, 513]))
    S("W_children_0_mod_%d" % T, [("one", 2 * T)], dict(n_children=2 * T, n_children_mod=0))
    S("W_children_1_mod_%d" % T, [("one", 2 * T + 1)], dict(n_children_mod=1))
    S("W_no_children", [("none", 300)], dict(n_children=0, blocks=0))
    S("W_list_fills_mwalk", [("one", 300), ("heavy", 257), ("none", 40)], dict(n_children=557), mwalk_slack=0)
    S("W_one_slot_short_of_mwalk", [("one", 300), ("heavy", 257), ("none", 40)], dict(n_children=557), mwalk_slack=-1, status=ERR_MWALK)
    # 256 x 1024 walkers and one more: the second round of the narrowing.  Almost every walker childless; the children sit at both ends,
    # behind long childless stretches and in a cluster, so that blocks start in every part of the list
    for extra in (0, 1):
        n0 = T * W + extra
        segs = [("one", 700), ("none", 100000), ("heavy", 300), ("none", 60000 - 1), ("one", 1500), ("none", 5), ("one", 1200), None, ("one", 259), ("heavy", 257)]
        segs[7] = ("none", n0 - sum(1 if s[0] == "heavy" else s[1] for s in segs if s))
        S("W_n0_%d" % n0, segs, dict(n0=n0, narrowing_rounds=1 + extra, n_children=("le", 6000), children_beyond_window=("ge", 1)), replay=False)
    return out


def s_cases(univ, consts):
    """set S: the scan's tiles"""
    ST = consts["SCAN_TILE"]
    out = []
    for k, n0 in enumerate((ST - 1, ST, ST + 1, 2 * ST + 1)):
        segs = [("one", 300), ("none", 200), ("heavy", 257), ("one", n0 - 300 - 200 - 1 - 5), ("none", 4), ("heavy", 3)]
        out.append(seg_case("S_n0_%d" % n0, "S", univ, segs, 300 + k, claims=dict(n0=n0, scan_tiles=(n0 + ST - 1) // ST)))
    # tiles that are all zero next to a tile that sums past 2^20: the walker of weight 2^20 + 0.5 (set G's largest) sits in tile 1
    segs = [("none", ST), ("one", 10), ("w", [2.0 ** 20 + 0.5]), ("one", ST - 11), ("none", ST), ("one", 5)]
    out.append(seg_case("S_zero_tiles_beside_a_tile_past_2^20", "S", univ, segs, 310, claims=dict(scan_zero_tiles=2, scan_tiles_past_2_20=1, n_children=(1 << 20) + 1 + 10 + (ST - 11) + 5),
                        replay=False, big=True))
    return out


def h_cases(univ_hb, univ_heg, consts):
    """set H: the W structures on the heat-bath proposal (two slots per child) and on the 57-orbital electron gas (unpacked keys)"""
    W = consts["SPAWN_WIN"]
    segs = [("heavy", 300), ("none", W - 1), ("one", 300), ("none", 30), ("heavy", 513), ("one", 200)]
    return [seg_case("H_heatbath_two_slots_per_child", "H", univ_hb, segs, 401, claims=dict(children_beyond_window=("ge", 1)), system="c2hb"),
            seg_case("H_heg57_unpacked_keys", "H", univ_heg, segs, 402, claims=dict(children_beyond_window=("ge", 1)), system="heg57", prm=dict(tau=1e-3, e_trial=0.0))]


def bucket_target():
    import re
    txt = open(os.path.join(ROOT, "sqmc_amd", "csrc", "bucket_partition.h")).read()
    half = int(re.search(r"#define BK_HALF (\d+)", txt).group(1))
    return [int(x) for x in re.findall(r"#define BK_TARGET (\d+)", txt)][0 if half else 1]


def p_case(univ, consts, system="c2", name="P_second_step", prm=None):
    """L0 of set P: non-initiators, a tiny tau, a large r_initiator, min_wt below every weight -- step 1 leaves it almost as it is.
    Childless runs of below-cutoff weights longer than the window, heavy parents across block starts, and the heaviest parent in
    front of a childless stretch of more than two buckets' residents, placed so that with equal-residents boundaries (bucket b begins at
    resident b n0 / B) it is its bucket's last walker and the buckets behind it hold childless walkers only.  (No parent of thousands
    of children here: a quarter of them land beside it, and a bucket filled beyond 85 % sends the next steps to the radix tail.)"""
    W = consts["SPAWN_WIN"]
    head_, heavy, free = [("one", 100), ("none", W + 1), ("heavy", 257), ("one", 155), ("none", W - 1), ("one", 300), ("heavy", 513)], 1500, 1300 + 2 * W + 800
    tail_ = [("one", 40), ("heavy", 1025), ("none", 600), ("one", 255), ("none", 3), ("one", 30)]
    count = lambda segs: (sum(1 if s[0] == "heavy" else s[1] for s in segs), sum(s[1] for s in segs if s[0] != "none"))
    n0, nch = (x + y for x, y in zip(count(head_ + tail_), (free + 1, heavy)))
    B = -(-(n0 + nch) // bucket_target())
    pre = count(head_)[0]
    a = min((b * n0) // B - 1 - pre for b in range(1, B + 1) if (b * n0) // B - 1 - pre >= 1300)
    segs = head_ + [("none", a), ("heavy", heavy), ("none", free - a)] + tail_
    p = dict(tau=2.0 ** -30, r_initiator=1.0e6, min_wt=2.0 ** -40)
    p.update(prm or {})
    c = seg_case(name, "P", univ, segs, 501, system=system, prm=p,
                 claims=dict(children_beyond_window=("ge", 1), longest_childless_run=("ge", 2 * W), heavy_nchild=[257, 513, heavy, 1025], bpar_written=("ge", 16)),
                 buckets=B, heaviest_at=pre + a, n_children=nch)
    assert count(segs) == (n0, nch) and free - a >= 2 * W and any((b * n0) // B == pre + a + 1 for b in range(1, B)), (n0, nch, B, a)
    wk = c["walkers"]
    wk["wt"] = np.where(wk["wt"] == 0.0, 3 * 0.5 * 2.0 ** -30, wk["wt"])          # a zero weight would be dropped by step 1
    wk["initiator"] = np.ones(len(wk["wt"]), np.int8)
    wk["perm_sign"] = np.zeros(len(wk["wt"]), np.int8)
    wk["imp_distance"] = np.where(wk["imp_distance"] > 100, 3, wk["imp_distance"]).astype(np.int8)
    return c


# ------------------------------------------------------------------------------------------------ the systems and the model's answers
class Systems:
    """the oracle's systems and movers by name, built when first asked for"""

    def __init__(self, O):
        self.O, self._s = O, {}

    def get(self, name):
        if name not in self._s:
            O = self.O
            if name == "c2":
                s = O.ChemSystem(FCIDUMP, 8, 4, "d2h", time_sym=False, hf_mode=0)
                self._s[name] = (s, HC.chem_mover(O, s), None)
            elif name == "c2hb":
                s = O.ChemSystem(FCIDUMP, 10, 5, "d2h", time_sym=False, hf_mode=0)
                hb = O.HeatBath(s)
                self._s[name] = (s, HC.heatbath_mover(O, hb), hb)
            else:
                s = O.HegSystem(3, 1.0, 14, 7, 2.3)
                self._s[name] = (s, HC.heg_mover(O, s), None)
        return self._s[name]

    def streams(self, name, mode, step=0):
        s = self.get(name)[0]
        return HC.Counter(self.O, SEED, step, s.norb, s.ndn) if mode == 1 else HC.Replay(self.O, SEED)


def runs_in(case, which):
    if which == "first":
        return case["set"] in ("G", "W", "S", "H") and case["meta"].get("counter", True)
    if which == "replay":
        return case["set"] in ("G", "W") and case["meta"].get("replay", True)
    return case["set"] == "P" or (which == "P+H" and case["set"] == "PH")


def solve(case, systems, mode, consts, **mistakes):
    """the model's head of a case; checks the case's claims.  Returns the head (head_checker.head's dict plus layout)."""
    h = HC.head(case["walkers"], case["prm"], systems.streams(case["system"], mode), systems.get(case["system"])[1], consts, **mistakes)
    h["layout"] = HC.layout(h["nchild"], consts)
    return h


def build_first_step(O, consts=None):
    """sets G, W, S, H with the model's answers for both disciplines (want[1]: COUNTER, want[0]: REPLAY where the case runs there)"""
    consts = consts or HC.kernel_constants()
    systems = Systems(O)
    univ = universe(26, 4, 4, 18)
    cases = g_cases(univ)

    def next_draw(mode):
        def f(wk, i):
            st = systems.streams("c2", mode)
            if mode == 1:
                return st.gate_draw(int(wk["up"][i]), int(wk["dn"][i]))
            part = {k: v[:i] for k, v in wk.items()}
            if i:
                HC.head(part, _prm(), st, systems.get("c2")[1])
            return st.gate_draw(0, 0)
        return f
    c1 = draw_deciding("G_weights_on_both_sides_of_their_draw_counter", univ, next_draw(1)); c1["meta"]["replay"] = False
    c0 = draw_deciding("G_weights_on_both_sides_of_their_draw_replay", univ, next_draw(0)); c0["meta"]["counter"] = False
    cases += [c1, c0]
    cases += w_cases(univ, consts) + s_cases(univ, consts) + h_cases(universe(26, 5, 5, 3), heg_universe(57, 7, 7, 3000), consts)
    for c in cases:
        c["want"] = {}
        for mode in (1, 0):
            if not runs_in(c, "first" if mode else "replay"):
                continue
            h = solve(c, systems, mode, consts)
            if mode == 0 and h["n_children"] > REPLAY_MAX_CHILDREN:
                c["meta"]["replay"] = False
                continue
            miss = check_claims(h["layout"], c["claims"])
            assert miss is None, (c["name"], miss)
            for i, n in c["meta"].get("want_children_of", {}).items():
                assert int(h["nchild"][i]) == n, (c["name"], i, n, int(h["nchild"][i]))
            c["want"][mode] = dict(rec=h["rec"], n_children=h["n_children"], rng=h.get("rng"))
            c.setdefault("layout", dict(h["layout"]))          # COUNTER's where the case runs in both
        slots = systems.get(c["system"])[1].slots
        n0 = len(c["walkers"]["wt"])
        nch = max(w["n_children"] for w in c["want"].values())
        c["meta"]["mwalk"] = n0 + slots * nch + c["meta"].get("mwalk_slack", 4096)
    return cases


def build_p():
    consts = HC.kernel_constants()
    univ = universe(26, 4, 4, 18)
    ph = [p_case(universe(26, 5, 5, 3), consts, "c2hb", "P_heatbath_second_step"),
          p_case(heg_universe(57, 7, 7, 12000), consts, "heg57", "P_heg57_second_step", prm=dict(e_trial=0.0))]
    for c in ph:
        c["set"] = "PH"
    return [p_case(univ, consts)] + ph


def write(path, cases):
    with open(path, "wb") as f:
        pickle.dump(dict(cases=cases, consts=HC.kernel_constants()), f, protocol=4)


# ------------------------------------------------------------------------------------------------ the child
def _ctx(systems, case, rng_mode, mwalk):
    import sqmc_amd
    name = case["system"]
    s, _, hb = systems.get(name)
    if name == "heg57":
        g = sqmc_amd.GpuChem.heg(s.n_dim, s.norb, s.nup, s.ndn, s.length_cell, s.k_vectors(), rng_mode=rng_mode, seed=SEED, mwalk=mwalk)
    else:
        g = sqmc_amd.GpuChem(s.norb, s.nup, s.ndn, s.orbsym(), s.prod().reshape(-1), s.combine_2().reshape(-1), s.integrals(), n_group=s.s.n_group,
                             rng_mode=rng_mode, seed=SEED, mwalk=mwalk)
        if hb is not None:
            g.set_heatbath_tables(hb.fortran_arrays())
    wk = case["walkers"]
    n_imp = int((wk["imp_distance"] == 0).sum())
    g.set_projector(np.ones(n_imp, np.int64), np.arange(1, n_imp + 1, dtype=np.int64), np.zeros(n_imp))
    k = min(8, len(wk["up"]))
    g.set_ct_table(wk["up"][:k], wk["dn"][:k], np.full(k, -0.5), np.where(np.arange(k) == 0, 1.0, 0.0))
    return g


def _upload(g, wk):
    big = np.full(len(wk["up"]), 1e51)
    g.upload_walkers(dict(wk, matrix_elements=big, e_num=big, e_den=big))


def compare(rec, pm, out15, n_children, slots):
    """None, or the first difference between the model's records and debug_premerge's"""
    if not (int(out15) == n_children and len(pm["wt"]) == slots * n_children):
        return "out_stats[15] = %r, spawn slots %d, the model's children %d x %d slots" % (out15, len(pm["wt"]), n_children, slots)
    zero = rec["wt"] == 0.0
    if not np.array_equal(zero, pm["wt"] == 0.0):
        i = int(np.nonzero(zero != (pm["wt"] == 0.0))[0][0])
        return "slot %d: the model's weight %r, the record's %r (a weight of 0 means no walker)" % (i, rec["wt"][i], pm["wt"][i])
    live = ~zero
    for k in ("up", "dn", "wt", "imp_distance", "initiator"):
        if not np.array_equal(rec[k][live], pm[k][live]):
            i = int(np.nonzero(live & (rec[k] != pm[k]))[0][0])
            return "slot %d (child %d): %s = %r, the model's %r" % (i, i // slots, k, pm[k][i], rec[k][i])
    return None


def head_ok(info, variant):
    pipelined, offsets, hint = VARIANTS[variant][3]
    if (info["pipelined"], info["offsets"], info["parent_hint"]) != (pipelined, offsets, hint):
        return "debug_last_head %r: variant %s is written for pipelined=%r, offsets=%s, parent_hint=%r" % (info, variant, pipelined, offsets, hint)
    return None


def run_first(systems, variant, case):
    import sqmc_amd
    rng_mode = VARIANTS[variant][1]
    want, meta, wk = case["want"][rng_mode], case["meta"], case["walkers"]
    slots = systems.get(case["system"])[1].slots
    rec = dict(case=case["name"], variant=variant, n0=len(wk["wt"]), n_children=want["n_children"])
    t0 = time.time()
    g = _ctx(systems, case, rng_mode, meta["mwalk"])
    try:
        _upload(g, wk)
        status, out = 0, None
        try:
            out = g.step(case["prm"])
        except sqmc_amd.SqmcGpuError as e:
            status = e.code
        rec["status"] = status
        if status < 0:
            rec["ok"] = False; rec["why"] = "library failure"
            return rec
        why = None if status == meta.get("status", 0) else "status %d, expected %d" % (status, meta.get("status", 0))
        if status == 0 and why is None:
            rec["head"] = g.debug_last_head()
            why = head_ok(rec["head"], variant) or compare(want["rec"], g.debug_premerge(), out[15], want["n_children"], slots)
            if rng_mode == 0 and g.rng_state() != want["rng"]:
                why = why or "generator %r after the step, the model's ends on %r" % (g.rng_state(), want["rng"])
        if status == ERR_MWALK and why is None:
            # the context works again after a fresh upload: the same list without its last walker (the heavy parent's neighbours stay)
            wk2 = {k: v[:300].copy() for k, v in wk.items()}
            wk2["imp_distance"][-1] = 0
            _upload(g, wk2)
            st = systems.streams(case["system"], 1, step=0) if rng_mode == 1 else HC.Replay(systems.O, SEED, state=g.rng_state())      # (the refused step's pre-pass has drawn)
            out = g.step(case["prm"])
            h = HC.head(wk2, case["prm"], st, systems.get(case["system"])[1])
            why = compare(h["rec"], g.debug_premerge(), out[15], h["n_children"], slots)
            why = why and "the step after status %d: %s" % (status, why)
        rec["ok"] = why is None
        if why:
            rec["why"] = why
    finally:
        g.close()
    rec["ms"] = round(1000 * (time.time() - t0), 1)
    return rec


def _popctl(prm):
    from sqmc_amd._lib import PopCtl
    pc = PopCtl()
    pc.tau_sav = pc.tau = pc.tau_prev = prm["tau"]
    pc.e_trial = pc.e_est = prm["e_trial"]
    pc.w_abs_gen_target = pc.w_abs_gen = 1.0e4
    pc.r_initiator_sav = pc.r_initiator = prm["r_initiator"]
    pc.initiator_rescale_power, pc.population_control_exponent = 1.0, 10.0
    pc.reweight_factor_inv, pc.reweight_factor_inv_max = 1.0, 2.0
    pc.e_num_cum = pc.e_den_cum = 0.0
    pc.min_wt, pc.always_spawn_cutoff_wt = prm["min_wt"], prm["always_spawn_cutoff_wt"]
    pc.reached_w_abs_gen, pc.initiator_power, pc.initiator_min_distance, pc.c_t_initiator = 2, prm["initiator_power"], prm["initiator_min_distance"], prm["c_t_initiator"]
    pc.semistochastic, pc.istep, pc.n_equil = 1, 0, 0
    return pc


def run_p(systems, variant, case, consts):
    """Warm-up (one step: the bucket tail carries offsets only once the context knows the last step's sum of |w|), a fresh upload of L0,
    then sqmc_gpu_run of 2 steps: steps 1 and 2 of the context.  The twin does the same with a run of 1 step and holds L1."""
    import sqmc_amd
    wk, prm = case["walkers"], case["prm"]
    mover = systems.get(case["system"])[1]
    rec = dict(case=case["name"], variant=variant, n0=len(wk["wt"]))
    t0 = time.time()
    mwalk = len(wk["wt"]) + mover.slots * 12000
    g, twin = _ctx(systems, case, 1, mwalk), _ctx(systems, case, 1, mwalk)
    try:
        try:
            for ctx, nsteps in ((twin, 1), (g, 2)):
                _upload(ctx, wk)
                ctx.run(_popctl(prm), 1, keep_stats=False)
                _upload(ctx, wk)
                stats, _ = ctx.run(_popctl(prm), nsteps)
        except sqmc_amd.SqmcGpuError as e:
            rec.update(status=e.code, ok=False, why=str(e))
            return rec
        rec["status"] = 0
        L1 = twin.download_walkers()
        rec["n1"] = len(L1["wt"])
        rec["head"], rec["tail"] = g.debug_last_head(), g.last_tail()
        l1 = dict(L1, perm_sign=np.zeros(len(L1["wt"]), np.int8))
        h = HC.head(l1, prm, systems.streams(case["system"], 1, step=2), mover)
        lay = HC.layout(h["nchild"], consts, hint=VARIANTS[variant][3][2])
        rec["layout"] = {k: lay[k] for k in ("n0", "n_children", "blocks", "children_beyond_window", "longest_childless_run", "bpar_written", "heavy_nchild", "heavy_off_mod")}
        rec["n_children"] = h["n_children"]
        why = check_claims(lay, case["claims"]) or head_ok(rec["head"], variant)
        # (the tail of step 2; the head's producer says what step 1's was.  A bucket tail that gave up and was re-run counts as one.)
        want_tail = "bucket" if variant in BUCKET_TAIL else ("radix" if VARIANTS[variant][0].get("SQMC_BUCKET") == "0" or case["system"] != "c2" or variant == "p_unpacked" else None)
        if why is None and want_tail and not rec["tail"]["kind"].startswith(want_tail):
            why = "tail %r, variant %s is written for the %s tail" % (rec["tail"], variant, want_tail)
        why = why or compare(h["rec"], g.debug_premerge(), stats[1][15], h["n_children"], mover.slots)
        rec["ok"] = why is None
        if why:
            rec["why"] = why
    finally:
        g.close(); twin.close()
    rec["ms"] = round(1000 * (time.time() - t0), 1)
    return rec


def main(argv):
    path, variant = argv[1], argv[2]
    env, _, which, _ = VARIANTS[variant]
    for k in SWITCHES:
        assert os.environ.get(k) == env.get(k), "the environment of this process does not select variant %s (%s)" % (variant, k)
    with open(path, "rb") as f:
        blob = pickle.load(f)
    from oracle import oracle as O
    O.build()
    import sqmc_amd
    sqmc_amd.set_device(0)
    systems = Systems(O)
    t0 = time.time()
    n_bad = n_run = 0
    for case in blob["cases"]:
        if not runs_in(case, which) or (which in ("first", "replay") and VARIANTS[variant][1] not in case["want"]):
            continue
        rec = run_first(systems, variant, case) if which in ("first", "replay") else run_p(systems, variant, case, blob["consts"])
        print(json.dumps(rec, default=str), flush=True)
        n_run += 1
        if rec.get("status", 0) == ERR_HIP:
            return 3
        n_bad += 0 if rec["ok"] else 1
    print(json.dumps(dict(variant=variant, cases_run=n_run, cases_failed=n_bad, seconds=round(time.time() - t0, 2))), flush=True)
    return 1 if n_bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
